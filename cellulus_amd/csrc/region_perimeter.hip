// "measure" stage, clx_region_perimeter: the border pixels of every object by neighbourhood class (2-D).
// Perimeter (2-D): scikit-image's perimeter(mask, neighbourhood=4) restated on the full map.  A pixel of object i is a
// border pixel if one of its 4 neighbours is not i (another object, background or the outside of the image); its code is
// 1 + 2 n4 + 10 nd with n4 / nd the border pixels OF i among its 4 edge / 4 diagonal neighbours.  That is a 5 x 5
// dependency: a block stages a PT x PT tile with a halo of 2 in LDS, derives the border flags of the tile plus a halo of
// 1 (kept as the id itself, 0: no border pixel), then the codes of the tile, counted per id and weight class in the
// id-keyed LDS table and flushed once per block.
#include "region_scan.h"

namespace {

constexpr int PT = 32;                  // tile edge: PT * PT = TILE pixels, a lane takes 4 of a tile row
constexpr int PH = PT + 4, PB = PT + 2;
constexpr int NCLS = 4;                 // border pixels; codes of weight 1, sqrt 2, (1 + sqrt 2) / 2

__device__ __forceinline__ int perimeter_class(int n4, int nd) {
  if ((n4 == 2 || n4 == 3) && nd <= 2) return 1;        // codes 5 7 15 17 25 27
  if ((n4 == 0 && nd == 2) || (n4 == 1 && nd == 3)) return 2;   // 21 33
  if (n4 == 1 && (nd == 1 || nd == 2)) return 3;        // 13 23
  return 0;
}

// `packed`: one byte per class, each at most PPL
__device__ void add_classes(int* keys, unsigned int (*acc)[SLOTS], u64* classes, int label, unsigned int packed) {
  const int s = find_slot(keys, label);
#pragma unroll
  for (int q = 0; q < NCLS; ++q) {
    const unsigned int n = (packed >> (8 * q)) & 0xffu;
    if (n == 0) continue;
    if (s >= 0) atomicAdd(&acc[q][s], n);
    else atomicAdd(classes + (size_t)label * NCLS + q, (u64)n);
  }
}

__global__ void perimeter_init(u64* __restrict__ classes, int* __restrict__ bad, int nid) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *bad = 0;
  if (i >= nid) return;
  for (int q = 0; q < NCLS; ++q) classes[(size_t)i * NCLS + q] = 0;
}

__global__ __launch_bounds__(BLOCK) void perimeter_kernel(const int* __restrict__ lab, int Y, int X, int nid, int tiles_x,
                                                          long long ntiles, long long tiles_per_block, u64* __restrict__ classes,
                                                          int* __restrict__ bad) {
  __shared__ int keys[SLOTS];
  __shared__ unsigned int acc[NCLS][SLOTS];             // a block's pixels are below 2^32
  __shared__ int ls[PH][PH + 1];
  __shared__ int bs[PB][PB + 1];
  for (int s = threadIdx.x; s < SLOTS; s += BLOCK) {
    keys[s] = 0;
    for (int q = 0; q < NCLS; ++q) acc[q][s] = 0;
  }

  const long long t0 = (long long)blockIdx.x * tiles_per_block;
  const long long t1 = t0 + tiles_per_block < ntiles ? t0 + tiles_per_block : ntiles;
  const int row = threadIdx.x >> 3, col = (threadIdx.x & 7) * PPL;
  bool any_bad = false;
  for (long long t = t0; t < t1; ++t) {
    const int ty = (int)(t / tiles_x), tx = (int)(t - (long long)ty * tiles_x);
    const long long y0 = (long long)ty * PT - 2, x0 = (long long)tx * PT - 2;
    __syncthreads();                                    // the table is set up; the last trip's readers of ls / bs are done
    for (int i = threadIdx.x; i < PH * PH; i += BLOCK) {
      const int r = i / PH, c = i - r * PH;
      const long long gy = y0 + r, gx = x0 + c;
      int v = 0;
      if (gy >= 0 && gy < Y && gx >= 0 && gx < X) {
        v = lab[(size_t)gy * (size_t)X + (size_t)gx];
        if ((unsigned)v >= (unsigned)nid) { v = 0; any_bad = true; }
      }
      ls[r][c] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < PB * PB; i += BLOCK) {
      const int r = i / PB, c = i - r * PB;             // (r + 1, c + 1) in ls
      const int v = ls[r + 1][c + 1];
      const bool border = v > 0 && (ls[r][c + 1] != v || ls[r + 2][c + 1] != v || ls[r + 1][c] != v || ls[r + 1][c + 2] != v);
      bs[r][c] = border ? v : 0;
    }
    __syncthreads();
    int cur = 0;
    unsigned int packed = 0;
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      const int br = row + 1, bc = col + k + 1;         // the lane's pixel in bs
      const int v = bs[br][bc];
      if (v == 0) continue;
      const int n4 = (bs[br - 1][bc] == v) + (bs[br + 1][bc] == v) + (bs[br][bc - 1] == v) + (bs[br][bc + 1] == v);
      const int nd = (bs[br - 1][bc - 1] == v) + (bs[br - 1][bc + 1] == v) + (bs[br + 1][bc - 1] == v) + (bs[br + 1][bc + 1] == v);
      if (v != cur) {
        if (packed) add_classes(keys, acc, classes, cur, packed);
        cur = v;
        packed = 0;
      }
      const int cls = perimeter_class(n4, nd);
      packed += 1u + (cls ? 1u << (8 * cls) : 0u);
    }
    if (packed) add_classes(keys, acc, classes, cur, packed);
  }
  if (any_bad) *bad = 1;
  __syncthreads();

  for (int s = threadIdx.x; s < SLOTS; s += BLOCK) {
    const int label = keys[s];
    if (label == 0) continue;
#pragma unroll
    for (int q = 0; q < NCLS; ++q)
      if (acc[q][s]) atomicAdd(classes + (size_t)label * NCLS + q, (u64)acc[q][s]);
  }
}

}  // namespace

extern "C" int clx_region_perimeter(const int32_t* labels, int Y, int X, int nid, unsigned long long* classes, int32_t* bad,
                                    clx_stream stream) {
  CLX_REQUIRE(labels && classes && bad, "clx_region_perimeter: null pointer");
  CLX_REQUIRE(Y > 0 && X > 0, "clx_region_perimeter: bad shape");
  CLX_REQUIRE(nid >= 1 && nid <= (1 << 24), "clx_region_perimeter: nid must lie in [1, 2^24]");
  CLX_REQUIRE((unsigned long long)Y * (unsigned long long)X < (1ull << 32), "clx_region_perimeter: Y * X must be below 2^32");
  hipStream_t st = (hipStream_t)stream;
  perimeter_init<<<(nid + 255) / 256, 256, 0, st>>>(classes, bad, nid);
  const int tiles_x = (X + PT - 1) / PT;
  const long long ntiles = (long long)((Y + PT - 1) / PT) * tiles_x;
  const int grid = (int)(ntiles < MAX_GRID ? ntiles : MAX_GRID);
  perimeter_kernel<<<grid, BLOCK, 0, st>>>(labels, Y, X, nid, tiles_x, ntiles, (ntiles + grid - 1) / grid, classes, bad);
  CLX_CHECK_LAUNCH("clx_region_perimeter");
  return CLX_OK;
}
