// "measure" stage: the per-object table users take from skimage.measure.regionprops on the host
// (area, bounding box, centroid, second moments, mean / min / max intensity), as integer sums
// gathered in one pass over the label map on the device:
//   clx_region_moments    pixel count, bounding box, Σ coordinate and Σ coordinate products per id
//   clx_region_intensity  Σ quantised value and min / max (order-preserving keys) of one raw channel per id
// Both kernels share one structure.  A lane reads 4 consecutive pixels; a lane whose pixels all carry one
// object id (and lie in one image row, for the moments) is "uniform".  A ballot over the wave cuts the 64 lanes
// into runs of uniform lanes with the same id (and row); the first lane of a run owns it.  The geometric sums
// of a run follow in closed form from its start and length, the intensities from a segmented wave reduction.
// Lanes on an object's edge walk their 4 pixels one by one.  Runs are combined in a table in LDS keyed by id
// (open addressing, PROBES tries, then straight to global memory) which the block adds to the outputs when
// its pixels are done: one 64-bit integer atomic per id, quantity and block.  Integer adds, min and max
// commute, so the outputs are the same bits in every run.
#include "clx_common.h"

namespace {

enum { RAW_F32 = 0, RAW_F64 = 1, RAW_I32 = 2 };

typedef unsigned long long u64;
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int BLOCK = 256;
constexpr int PPL = 4;                  // pixels per lane
constexpr int TILE = BLOCK * PPL;       // pixels per block and trip
constexpr int SLOTS = 256;              // ids a block keeps in LDS (power of two)
constexpr int PROBES = 8;
constexpr int MAX_GRID = 1024;          // blocks; each takes a contiguous range of tiles
constexpr int NQ = 10;                  // area, Σz Σy Σx, Σzz Σyy Σxx Σzy Σzx Σyx

__device__ __forceinline__ u64 order_key(float v) {
  const unsigned int b = __float_as_uint(v);
  return (u64)((b & 0x80000000u) ? ~b : (b | 0x80000000u));
}
__device__ __forceinline__ u64 order_key(double v) {
  const u64 b = (u64)__double_as_longlong(v);
  return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ u64 order_key(int v) { return (u64)((unsigned int)v ^ 0x80000000u); }

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

struct MomentsOut {
  u64* area;
  u64* sum1;
  u64* sum2;
  int* bbox;
};

__device__ __forceinline__ u64* moments_addr(const MomentsOut& o, int label, int q) {
  if (q == 0) return o.area + label;
  if (q < 4) return o.sum1 + (size_t)label * 3 + (q - 1);
  return o.sum2 + (size_t)label * 6 + (q - 4);
}

__device__ __forceinline__ void box_to_global(int* b, int z0, int y0, int x0, int z1, int y1, int x1) {
  if (z0 < b[0]) atomicMin(b + 0, z0);  // the plain reads only filter, as in stats_kernel (nucleus.hip)
  if (y0 < b[1]) atomicMin(b + 1, y0);
  if (x0 < b[2]) atomicMin(b + 2, x0);
  if (z1 > b[3]) atomicMax(b + 3, z1);
  if (y1 > b[4]) atomicMax(b + 4, y1);
  if (x1 > b[5]) atomicMax(b + 5, x1);
}

// n pixels of `label` at (z, y, x0 .. x0 + n - 1).  No term exceeds the image's own Σ of that quantity, which the
// entry point bounds below 2^63.
__device__ void add_run(int* keys, u64 (*acc)[SLOTS], int (*box)[SLOTS], const MomentsOut& o, int label, int n,
                        int z, int y, int x0) {
  const u64 N = (u64)n, a = (u64)x0, Z = (u64)z, Yc = (u64)y;
  const u64 t1 = N * (N - 1) / 2;                       // Σ i,  i < n
  const u64 t2 = (N - 1) * N * (2 * N - 1) / 6;         // Σ i²
  const u64 sx = N * a + t1;
  const u64 v[NQ] = {N, N * Z, N * Yc, sx, N * Z * Z, N * Yc * Yc, N * a * a + 2 * a * t1 + t2, N * Z * Yc, Z * sx, Yc * sx};
  const int s = find_slot(keys, label);
  if (s >= 0) {
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      if (v[q]) atomicAdd(&acc[q][s], v[q]);
    atomicMin(&box[0][s], z); atomicMin(&box[1][s], y); atomicMin(&box[2][s], x0);
    atomicMax(&box[3][s], z); atomicMax(&box[4][s], y); atomicMax(&box[5][s], x0 + n - 1);
  } else {
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      if (v[q]) atomicAdd(moments_addr(o, label, q), v[q]);
    box_to_global(o.bbox + (size_t)label * 6, z, y, x0, z, y, x0 + n - 1);
  }
}

__global__ void moments_init(MomentsOut o, int* __restrict__ bad, int nid) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *bad = 0;
  if (i >= nid) return;
  o.area[i] = 0;
  for (int k = 0; k < 3; ++k) { o.sum1[(size_t)i * 3 + k] = 0; o.bbox[i * 6 + k] = 0x7fffffff; o.bbox[i * 6 + 3 + k] = -1; }
  for (int k = 0; k < 6; ++k) o.sum2[(size_t)i * 6 + k] = 0;
}

__global__ __launch_bounds__(BLOCK) void moments_kernel(const int* __restrict__ lab, int vec, long long npix, int Y, int X,
                                                        int nid, long long ntiles, long long tiles_per_block, MomentsOut o,
                                                        int* __restrict__ bad) {
  __shared__ int keys[SLOTS];
  __shared__ u64 acc[NQ][SLOTS];
  __shared__ int box[6][SLOTS];
  for (int s = threadIdx.x; s < SLOTS; s += BLOCK) {
    keys[s] = 0;
    for (int q = 0; q < NQ; ++q) acc[q][s] = 0;
    for (int k = 0; k < 3; ++k) { box[k][s] = 0x7fffffff; box[3 + k][s] = -1; }
  }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const long long t0 = (long long)blockIdx.x * tiles_per_block;
  const long long t1 = t0 + tiles_per_block < ntiles ? t0 + tiles_per_block : ntiles;
  bool any_bad = false;
  for (long long t = t0; t < t1; ++t) {
    const long long p0 = t * TILE + (long long)threadIdx.x * PPL;
    int l[PPL];
    load_labels(lab, vec != 0, p0, npix, l);
    any_bad |= clamp_labels(l, nid);
    // npix < 2^32: 32-bit divisions
    const unsigned int pu = p0 < npix ? (unsigned int)p0 : 0u;
    const unsigned int r = pu / (unsigned int)X;
    int x = (int)(pu - r * (unsigned int)X);
    int z = (int)(r / (unsigned int)Y);
    int y = (int)(r - (unsigned int)z * (unsigned int)Y);

    // a run never continues into the next image row: the closed forms hold inside one row only
    const bool uni = l[0] > 0 && l[0] == l[1] && l[1] == l[2] && l[2] == l[3] && x + PPL <= X;
    const int lprev = __shfl_up(l[0], 1);
    const unsigned int rprev = __shfl_up(r, 1);
    const u64 unis = __ballot(uni);
    const bool head = !uni || lane == 0 || !((unis >> (lane - 1)) & 1ull) || lprev != l[0] || rprev != r;
    const u64 heads = __ballot(head);
    if (uni) {
      if (head) add_run(keys, acc, box, o, l[0], PPL * run_lanes(heads, lane), z, y, x);
    } else {
      int cur = 0, n = 0, cz = 0, cy = 0, cx = 0;
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        if (l[k] != cur || x == 0) {
          if (cur > 0) add_run(keys, acc, box, o, cur, n, cz, cy, cx);
          cur = l[k]; n = 0; cz = z; cy = y; cx = x;
        }
        ++n;
        if (++x == X) { x = 0; if (++y == Y) { y = 0; ++z; } }
      }
      if (cur > 0) add_run(keys, acc, box, o, cur, n, cz, cy, cx);
    }
  }
  if (any_bad) *bad = 1;
  __syncthreads();

  for (int s = threadIdx.x; s < SLOTS; s += BLOCK) {
    const int label = keys[s];
    if (label == 0) continue;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      if (acc[q][s]) atomicAdd(moments_addr(o, label, q), acc[q][s]);
    box_to_global(o.bbox + (size_t)label * 6, box[0][s], box[1][s], box[2][s], box[3][s], box[4][s], box[5][s]);
  }
}

// ---------------------------------------------------------------------------------------------------------

template <typename T> struct alignas(16) Raw4 { T v[PPL]; };

// q of one raw value; false: not finite, or |q| above the bound
template <typename T>
__device__ __forceinline__ bool quantise(T v, int shift, long long bound, long long* q) {
  const double t = rint(ldexp((double)v, shift));       // NaN and ±Inf fail the comparison / exceed the bound
  if (!(fabs(t) <= (double)bound)) return false;        // bound is a power of two: exact as a double
  *q = (long long)t;
  return true;
}
template <>
__device__ __forceinline__ bool quantise<int>(int v, int, long long, long long* q) {
  *q = (long long)v;
  return true;
}

__device__ void add_values(int* keys, u64* ssum, u64* smin, u64* smax, long long* isum, u64* vkey, int label, long long s,
                           u64 kmin, u64 kmax) {
  const int slot = find_slot(keys, label);
  if (slot >= 0) {
    atomicAdd(&ssum[slot], (u64)s);                     // two's complement: the signed sum, modulo 2^64
    atomicMin(&smin[slot], kmin);
    atomicMax(&smax[slot], kmax);
  } else {
    atomicAdd(reinterpret_cast<u64*>(isum) + label, (u64)s);
    u64* v = vkey + (size_t)label * 2;
    if (kmin < v[0]) atomicMin(v + 0, kmin);
    if (kmax > v[1]) atomicMax(v + 1, kmax);
  }
}

__global__ void intensity_init(long long* __restrict__ isum, u64* __restrict__ vkey, int* __restrict__ bad, int nid) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *bad = 0;
  if (i >= nid) return;
  isum[i] = 0;
  vkey[(size_t)i * 2] = ~0ull;
  vkey[(size_t)i * 2 + 1] = 0ull;
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void intensity_kernel(const int* __restrict__ lab, const T* __restrict__ raw, int vec_lab,
                                                          int vec_raw, long long npix, int nid, int shift, long long bound,
                                                          long long ntiles, long long tiles_per_block,
                                                          long long* __restrict__ isum, u64* __restrict__ vkey,
                                                          int* __restrict__ bad) {
  __shared__ int keys[SLOTS];
  __shared__ u64 ssum[SLOTS], smin[SLOTS], smax[SLOTS];
  for (int s = threadIdx.x; s < SLOTS; s += BLOCK) { keys[s] = 0; ssum[s] = 0; smin[s] = ~0ull; smax[s] = 0; }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const long long t0 = (long long)blockIdx.x * tiles_per_block;
  const long long t1 = t0 + tiles_per_block < ntiles ? t0 + tiles_per_block : ntiles;
  int any_bad = 0;
  for (long long t = t0; t < t1; ++t) {
    const long long p0 = t * TILE + (long long)threadIdx.x * PPL;
    int l[PPL];
    load_labels(lab, vec_lab != 0, p0, npix, l);
    if (clamp_labels(l, nid)) any_bad |= 1;
    Raw4<T> rv;
    if (vec_raw && p0 + PPL <= npix) {
      rv = *reinterpret_cast<const Raw4<T>*>(raw + p0);
    } else {
#pragma unroll
      for (int k = 0; k < PPL; ++k) rv.v[k] = p0 + k < npix ? raw[p0 + k] : (T)0;
    }
    long long q[PPL];
    u64 key[PPL];
    long long s = 0;
    u64 kmin = ~0ull, kmax = 0ull;
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      q[k] = 0;
      key[k] = order_key(rv.v[k]);
      if (l[k] > 0 && !quantise<T>(rv.v[k], shift, bound, &q[k])) { l[k] = 0; any_bad |= 2; }   // the pixel is skipped
      s += q[k];
      kmin = key[k] < kmin ? key[k] : kmin;
      kmax = key[k] > kmax ? key[k] : kmax;
    }
    const bool uni = l[0] > 0 && l[0] == l[1] && l[1] == l[2] && l[2] == l[3];
    const int lprev = __shfl_up(l[0], 1);
    const u64 unis = __ballot(uni);
    const bool head = !uni || lane == 0 || !((unis >> (lane - 1)) & 1ull) || lprev != l[0];
    const u64 heads = __ballot(head);
    const int end = lane + run_lanes(heads, lane);
    // segmented reduction: after the step with distance d a lane holds lanes [lane, min(lane + 2d, end)) of its run
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long s2 = __shfl_down(s, d);
      const u64 lo2 = __shfl_down(kmin, d), hi2 = __shfl_down(kmax, d);
      if (lane + d < end) {
        s += s2;
        kmin = lo2 < kmin ? lo2 : kmin;
        kmax = hi2 > kmax ? hi2 : kmax;
      }
    }
    if (uni) {
      if (head) add_values(keys, ssum, smin, smax, isum, vkey, l[0], s, kmin, kmax);
    } else {
      int cur = 0;
      long long cs = 0;
      u64 clo = ~0ull, chi = 0ull;
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        if (l[k] != cur) {
          if (cur > 0) add_values(keys, ssum, smin, smax, isum, vkey, cur, cs, clo, chi);
          cur = l[k]; cs = 0; clo = ~0ull; chi = 0ull;
        }
        cs += q[k];
        clo = key[k] < clo ? key[k] : clo;
        chi = key[k] > chi ? key[k] : chi;
      }
      if (cur > 0) add_values(keys, ssum, smin, smax, isum, vkey, cur, cs, clo, chi);
    }
  }
  if (any_bad) atomicOr(bad, any_bad);
  __syncthreads();

  for (int s = threadIdx.x; s < SLOTS; s += BLOCK) {
    const int label = keys[s];
    if (label == 0) continue;
    if (ssum[s]) atomicAdd(reinterpret_cast<u64*>(isum) + label, ssum[s]);
    u64* v = vkey + (size_t)label * 2;
    if (smin[s] < v[0]) atomicMin(v + 0, smin[s]);
    if (smax[s] > v[1]) atomicMax(v + 1, smax[s]);
  }
}

struct Tiling {
  long long ntiles, per_block;
  int grid;
};
inline Tiling tiling_for(long long npix) {
  Tiling t;
  t.ntiles = (npix + TILE - 1) / TILE;
  t.grid = (int)(t.ntiles < MAX_GRID ? t.ntiles : MAX_GRID);
  t.per_block = (t.ntiles + t.grid - 1) / t.grid;
  return t;
}

inline int bit_length(unsigned long long v) {
  int n = 0;
  while (v) { ++n; v >>= 1; }
  return n;
}

}  // namespace

extern "C" int clx_region_moments(const int32_t* labels, int Z, int Y, int X, int nid, unsigned long long* area,
                                  int32_t* bbox, unsigned long long* sum1, unsigned long long* sum2, int32_t* bad,
                                  clx_stream stream) {
  CLX_REQUIRE(labels && area && bbox && sum1 && sum2 && bad, "clx_region_moments: null pointer");
  CLX_REQUIRE(Z > 0 && Y > 0 && X > 0, "clx_region_moments: bad shape");
  CLX_REQUIRE(nid >= 1 && nid <= (1 << 24), "clx_region_moments: nid must lie in [1, 2^24]");
  const unsigned __int128 npix128 = (unsigned __int128)Z * (unsigned)Y * (unsigned)X;
  CLX_REQUIRE(npix128 < ((unsigned __int128)1 << 32), "clx_region_moments: Z * Y * X must be below 2^32");
  const long long npix = (long long)npix128;
  const unsigned long long m = (unsigned long long)((Z > Y ? (Z > X ? Z : X) : (Y > X ? Y : X)) - 1);
  CLX_REQUIRE((unsigned __int128)(m * m) * (unsigned __int128)npix < ((unsigned __int128)1 << 63),
              "clx_region_moments: (largest extent - 1)^2 * Z * Y * X must be below 2^63 (the second moments are 64-bit)");
  hipStream_t st = (hipStream_t)stream;
  const MomentsOut o = {area, sum1, sum2, bbox};
  moments_init<<<(nid + 255) / 256, 256, 0, st>>>(o, bad, nid);
  const Tiling t = tiling_for(npix);
  moments_kernel<<<t.grid, BLOCK, 0, st>>>(labels, ((uintptr_t)labels & 15) == 0, npix, Y, X, nid, t.ntiles, t.per_block, o, bad);
  CLX_CHECK_LAUNCH("clx_region_moments");
  return CLX_OK;
}

extern "C" int clx_region_intensity(const int32_t* labels, const void* raw, int raw_type, long long npix, int nid, int shift,
                                    long long* isum, unsigned long long* vkey, int32_t* bad, clx_stream stream) {
  CLX_REQUIRE(labels && raw && isum && vkey && bad, "clx_region_intensity: null pointer");
  CLX_REQUIRE(raw_type >= RAW_F32 && raw_type <= RAW_I32, "clx_region_intensity: raw_type must be 0 (f32), 1 (f64) or 2 (i32)");
  CLX_REQUIRE(nid >= 1 && nid <= (1 << 24), "clx_region_intensity: nid must lie in [1, 2^24]");
  CLX_REQUIRE(npix > 0 && npix < (1ll << 32), "clx_region_intensity: npix must lie in [1, 2^32)");
  hipStream_t st = (hipStream_t)stream;
  const long long bound = (1ll << 62) >> bit_length((unsigned long long)npix);
  const int vl = ((uintptr_t)labels & 15) == 0, vr = ((uintptr_t)raw & 15) == 0;
  intensity_init<<<(nid + 255) / 256, 256, 0, st>>>(isum, vkey, bad, nid);
  const Tiling t = tiling_for(npix);
  if (raw_type == RAW_F32)
    intensity_kernel<float><<<t.grid, BLOCK, 0, st>>>(labels, (const float*)raw, vl, vr, npix, nid, shift, bound, t.ntiles,
                                                       t.per_block, isum, vkey, bad);
  else if (raw_type == RAW_F64)
    intensity_kernel<double><<<t.grid, BLOCK, 0, st>>>(labels, (const double*)raw, vl, vr, npix, nid, shift, bound, t.ntiles,
                                                        t.per_block, isum, vkey, bad);
  else
    intensity_kernel<int><<<t.grid, BLOCK, 0, st>>>(labels, (const int*)raw, vl, vr, npix, nid, shift, bound, t.ntiles,
                                                     t.per_block, isum, vkey, bad);
  CLX_CHECK_LAUNCH("clx_region_intensity");
  return CLX_OK;
}
