// The reading frame the measure stage's per-object reductions share (measure.hip, label_distance.hip): a lane reads 4
// consecutive pixels of the label map, a ballot cuts the wave into runs of lanes that carry one id, and a block combines
// what it finds in a table in LDS keyed by id (open addressing, PROBES tries, then straight to global memory) which it
// adds to the outputs once, when its pixels are done.
#pragma once
#include "clx_common.h"

namespace {

typedef unsigned long long u64;
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int BLOCK = 256;
constexpr int PPL = 4;                  // pixels per lane
constexpr int TILE = BLOCK * PPL;       // pixels per block and trip
constexpr int SLOTS = 256;              // ids a block keeps in LDS (power of two)
constexpr int PROBES = 8;
constexpr int MAX_GRID = 1024;          // blocks; each takes a contiguous range of tiles

// slot of `label` in the block's table, claiming an empty one; -1: PROBES occupied slots of other ids
__device__ __forceinline__ int find_slot(int* keys, int label) {
  int s = label & (SLOTS - 1);          // ids of neighbouring objects are close: they fill neighbouring slots
  for (int i = 0; i < PROBES; ++i) {
    int k = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k == 0) k = atomicCAS(&keys[s], 0, label);
    if (k == 0 || k == label) return s;
    s = (s + 1) & (SLOTS - 1);
  }
  return -1;
}

// labels of the lane's 4 pixels; past the end of the image: background
__device__ __forceinline__ void load_labels(const int* __restrict__ lab, bool vec, long long p0, long long npix, int* l) {
  if (vec && p0 + PPL <= npix) {
    const i32x4 v = *reinterpret_cast<const i32x4*>(lab + p0);
    l[0] = v[0]; l[1] = v[1]; l[2] = v[2]; l[3] = v[3];
  } else {
#pragma unroll
    for (int k = 0; k < PPL; ++k) l[k] = p0 + k < npix ? lab[p0 + k] : 0;
  }
}

// out-of-range ids become background (never an index); returns whether there was one
__device__ __forceinline__ bool clamp_labels(int* l, int nid) {
  bool bad = false;
#pragma unroll
  for (int k = 0; k < PPL; ++k)
    if ((unsigned)l[k] >= (unsigned)nid) { l[k] = 0; bad = true; }
  return bad;
}

// lanes [lane, lane + return value) form the run this lane heads; `heads`: ballot of the lanes that start one
__device__ __forceinline__ int run_lanes(u64 heads, int lane) {
  const u64 above = lane == 63 ? 0ull : heads >> (lane + 1);
  return above ? __ffsll((long long)above) : 64 - lane;
}

struct Tiling {
  long long ntiles, per_block;
  int grid;
};
inline Tiling tiling_for(long long npix, int max_grid = MAX_GRID) {
  Tiling t;
  t.ntiles = (npix + TILE - 1) / TILE;
  t.grid = (int)(t.ntiles < max_grid ? t.ntiles : max_grid);
  t.per_block = (t.ntiles + t.grid - 1) / t.grid;
  return t;
}

}  // namespace
