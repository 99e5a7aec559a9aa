// The link rule of the skeleton stage (include/clx.h, "skeleton" stage), the one copy the census (label_thin.hip) and the branch
// graph (skeleton_graph.hip) share: a FACE link joins two face neighbours of one label, a DIAGONAL link two diagonal neighbours
// of one label neither of whose two common face neighbours carries it; the DEGREE of a pixel is the number of its links.
#pragma once
#include "region_scan.h"

namespace {

// the eight directions: 0 .. 3 = E, S, SE, SW are the ones whose link the pixel OWNS (every link is owned by one of its two
// pixels), 4 .. 7 = W, N, NW, NE their opposites (k + 4 is the opposite of k); 0, 1, 4, 5 are the face directions
constexpr int LINK_DX[8] = {1, 0, 1, -1, -1, 0, -1, 1}, LINK_DY[8] = {0, 1, 1, 1, 0, -1, -1, -1};
constexpr int LINKS_OWNED = 4;
__device__ __forceinline__ bool link_is_face(int k) { return (k & 3) < 2; }

struct Links {
  bool on[8];                           // the pixel has a link in direction k
  bool block;                           // E, S and SE carry its value: the 2 x 2 window of which it is the first pixel is full
  __device__ __forceinline__ int degree() const { return on[0] + on[1] + on[2] + on[3] + on[4] + on[5] + on[6] + on[7]; }
  __device__ __forceinline__ int owned_face() const { return on[0] + on[1]; }
  __device__ __forceinline__ int owned_diag() const { return on[2] + on[3]; }
};

// the links of pixel p = (x, y) of a slice of Y x X pixels, which carries v != 0; rows and slices never wrap
__device__ __forceinline__ Links links_at(const int* __restrict__ lab, long long p, int x, int y, int Y, int X, int v) {
  bool nb[8];                           // the neighbour in direction k lies in the slice and carries v
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int dx = LINK_DX[k], dy = LINK_DY[k];
    const bool in = (dx < 0 ? x > 0 : dx > 0 ? x < X - 1 : true) && (dy < 0 ? y > 0 : dy > 0 ? y < Y - 1 : true);
    nb[k] = in && lab[p + (long long)dy * X + dx] == v;
  }
  const bool e = nb[0], so = nb[1], we = nb[4], no = nb[5];
  Links l;
  l.on[0] = e;
  l.on[1] = so;
  l.on[2] = nb[2] && !so && !e;
  l.on[3] = nb[3] && !so && !we;
  l.on[4] = we;
  l.on[5] = no;
  l.on[6] = nb[6] && !no && !we;
  l.on[7] = nb[7] && !no && !e;
  l.block = e && so && nb[2];
  return l;
}

}  // namespace
