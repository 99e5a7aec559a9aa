// The reading frame the measure and relate stages' per-object reductions share (region_*.hip, label_*.hip): a block takes
// a contiguous range of tiles, a lane reads 4 consecutive pixels of the label map, a ballot cuts the wave into runs of lanes
// that carry one id, a segmented wave reduction sums a run, and a block combines what it finds in a table in LDS keyed by id
// (open addressing, PROBES tries, then straight to global memory) which it adds to the outputs once, when its pixels are done.
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

// the tiles [t0, t1) of this block, and a lane's first pixel in trip t
struct Tiles {
  long long t0, t1;
};
__device__ __forceinline__ Tiles block_tiles(long long ntiles, long long tiles_per_block) {
  const long long t0 = (long long)blockIdx.x * tiles_per_block;
  return {t0, t0 + tiles_per_block < ntiles ? t0 + tiles_per_block : ntiles};
}
__device__ __forceinline__ long long lane_pixel(long long t) { return t * TILE + (long long)threadIdx.x * PPL; }

// The run rule.  A lane is uniform (`uni`) if its 4 values l[0 .. 3] (ids, pairs, cells) are one value that counts; a run is
// a stretch of uniform lanes with one value, and its first lane, the head, owns it; a lane that is not uniform is a head of
// its own.  `heads` is the ballot of the heads, for run_lanes.  Results come back by value, not through pointers: written
// that way the compiler's code stays the one of the spelled-out form, but for a few instructions.
struct Heads {
  u64 heads;
  bool head;
};
template <typename L>
__device__ __forceinline__ Heads run_heads(bool uni, const L* l, int lane) {
  const L lprev = __shfl_up(l[0], 1);
  const u64 unis = __ballot(uni);
  const bool head = !uni || lane == 0 || !((unis >> (lane - 1)) & 1ull) || lprev != l[0];
  return {__ballot(head), head};
}
// the same where a run must not continue into the next image row: `row` is the row of the lane's first pixel
template <typename L>
__device__ __forceinline__ Heads run_heads(bool uni, const L* l, unsigned int row, int lane) {
  const L lprev = __shfl_up(l[0], 1);
  const unsigned int rprev = __shfl_up(row, 1);
  const u64 unis = __ballot(uni);
  const bool head = !uni || lane == 0 || !((unis >> (lane - 1)) & 1ull) || lprev != l[0] || rprev != row;
  return {__ballot(head), head};
}

// Segmented reduction over the runs of a wave; `end`: one past the last lane of this lane's run.  V says how its fields
// cross the wave, shifted(d), and how two partial results combine, take(o): after the step with distance d a lane holds
// lanes [lane, min(lane + 2d, end)) of its run.
template <typename V>
__device__ __forceinline__ V reduce_run(V v, int lane, int end) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const V o = v.shifted(d);
    if (lane + d < end) v.take(o);
  }
  return v;
}
// a sum and the largest (MAX) or smallest key of a run
template <bool MAX> struct SumKey {
  u64 s, k;
  __device__ __forceinline__ SumKey shifted(int d) const { return {__shfl_down(s, d), __shfl_down(k, d)}; }
  __device__ __forceinline__ void take(const SumKey& o) {
    s += o.s;
    k = (MAX ? o.k > k : o.k < k) ? o.k : k;
  }
};

struct Pixel {
  int z, y, x;
};
// a pixel and the row it lies in, z * Y + y
struct PixelInRow {
  Pixel p;
  unsigned int row;
};
// pixel p0 (pixel 0 past the end of the image) by 32-bit divisions: npix < 2^32
__device__ __forceinline__ PixelInRow pixel_at(long long p0, long long npix, int Y, int X) {
  const unsigned int pu = p0 < npix ? (unsigned int)p0 : 0u;
  const unsigned int r = pu / (unsigned int)X;
  const int x = (int)(pu - r * (unsigned int)X);
  const int z = (int)(r / (unsigned int)Y);
  const int y = (int)(r - (unsigned int)z * (unsigned int)Y);
  return {{z, y, x}, r};
}
// the next pixel in raster order
__device__ __forceinline__ Pixel next_pixel(Pixel p, int Y, int X) {
  if (++p.x == X) { p.x = 0; if (++p.y == Y) { p.y = 0; ++p.z; } }
  return p;
}

// zeroes *bad and fills the rows of NW words of an output: word ONES of a row, where a minimum starts, gets ~0 (ONES < 0:
// no word does), the rest 0
template <int NW, int ONES>
__global__ void table_init(u64* __restrict__ out, int* __restrict__ bad, long long words) {
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 == 0) *bad = 0;
  for (long long i = i0; i < words; i += (long long)gridDim.x * blockDim.x)
    out[i] = ONES >= 0 && i % NW == ONES ? ~0ull : 0ull;
}
template <int NW, int ONES = -1>
inline void launch_table_init(u64* out, int* bad, int nid, hipStream_t st) {
  const long long words = (long long)nid * NW, blocks = (words + 255) / 256;
  table_init<NW, ONES><<<(int)(blocks < 1024 ? blocks : 1024), 256, 0, st>>>(out, bad, words);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

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
