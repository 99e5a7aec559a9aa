// The lock-free union-find the label kernels share (cc_label.hip, label_holes.hip, skeleton_graph.hip; the walk over the map
// they unite in is segments.h's).  L is a parent array over raster indices; links always point from the larger root to the
// smaller, so the final root of a set is its smallest index.  Stale reads of the parent array are harmless (parents only
// decrease along a chain; progress is made by the values returned from the atomics).  The rule its users keep: correctness
// across blocks and XCDs rests on the values returned by atomics and on kernel boundaries alone -- no block waits for another.
// BIAS is the offset at which parents are stored: node i's parent is L[i] - BIAS, and a parent p is written as p + BIAS.
// The default 0 stores the index itself; with BIAS = 1 the array can double as a label image whose background is 0
// (cc_label.hip's 2-D pipeline).  Arguments and results are always plain indices.
#pragma once
#include "clx_common.h"

namespace {

template <int BIAS = 0>
__device__ __forceinline__ int uf_find(const int* L, int a) {
  int p = L[a] - BIAS;
  while (p != a) { a = p; p = L[a] - BIAS; }
  return a;
}

// find with path halving: every visited node is re-pointed at its grandparent.  A plain store is
// enough: only non-roots are written (a root is changed by the atomicMin of a union alone), and any
// ancestor is a valid parent, so a lost or stale write merely leaves a longer path.
template <int BIAS = 0>
__device__ __forceinline__ int uf_find_halve(int* L, int a) {
  int p = L[a] - BIAS;
  while (p != a) {
    const int gp = L[p] - BIAS;
    if (gp != p) L[a] = gp + BIAS;
    a = p;
    p = gp;
  }
  return a;
}

template <int BIAS = 0>
__device__ __forceinline__ void uf_union(int* L, int a, int b) {
  bool done;
  do {
    a = uf_find_halve<BIAS>(L, a);
    b = uf_find_halve<BIAS>(L, b);
    if (a < b) {
      const int old = atomicMin(&L[b], a + BIAS) - BIAS;
      done = (old == b);
      b = old;
    } else if (b < a) {
      const int old = atomicMin(&L[a], b + BIAS) - BIAS;
      done = (old == a);
      a = old;
    } else {
      done = true;
    }
  } while (!done);
}

}  // namespace
