// "measure" stage: the per-object table users take from skimage.measure.regionprops on the host
// (area, bounding box, centroid, second moments, mean / min / max intensity), as integer sums
// gathered in one pass over the label map on the device:
//   clx_region_moments    pixel count, bounding box, Σ coordinate and Σ coordinate products per id
//   clx_region_intensity  Σ quantised value and min / max (order-preserving keys) of one raw channel per id
//   clx_region_contacts   faces between pixels of different ids, per id pair (a stencil; further down)
//   clx_region_perimeter  border pixels of every object by neighbourhood class (2-D; further down)
//   clx_region_topology   sums over the 2 x 2 (x 2) windows per id: Euler numbers, Crofton perimeter / surface (further down)
//   clx_region_hull       convex hull of every object's pixel corners: area, vertices, Feret diameters (further down)
// The first two kernels share one structure.  A lane reads 4 consecutive pixels; a lane whose pixels all carry one
// object id (and lie in one image row, for the moments) is "uniform".  A ballot over the wave cuts the 64 lanes
// into runs of uniform lanes with the same id (and row); the first lane of a run owns it.  The geometric sums
// of a run follow in closed form from its start and length, the intensities from a segmented wave reduction.
// Lanes on an object's edge walk their 4 pixels one by one.  Runs are combined in a table in LDS keyed by id
// (open addressing, PROBES tries, then straight to global memory) which the block adds to the outputs when
// its pixels are done: one 64-bit integer atomic per id, quantity and block.  Integer adds, min and max
// commute, so the outputs are the same bits in every run.
#include "pair_table.h"

namespace {

enum { RAW_F32 = 0, RAW_F64 = 1, RAW_I32 = 2 };

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

// ---------------------------------------------------------------------------------------------------------
// Contacts: every face (connectivity 1) between two pixels of different ids counts once for the pair (lo, hi); the
// outside of the image is id 0.  A pixel owns its forward faces (+x, +y, +z; past the last column / row / slice the
// neighbour is 0) and, in the first column / row / slice, the backward face to 0.  The output is a SET of pairs of
// unknown size: an open-addressing table in global memory keyed by (lo << 32) | hi (never 0, as hi >= 1), filled through
// a block-private table in LDS that is flushed once (pair_table.h, shared with label_overlap.hip).  A lane whose pixels
// and forward neighbours all carry one id away from the image edge has nothing to emit; a wave of such lanes skips the rest
// of the trip.

// a lane's faces in the order it meets them; equal pairs in a row (a horizontal edge gives four) become one add
struct PairRun {
  u64 key;
  unsigned int n;
};
__device__ __forceinline__ void face(PairRun& r, u64* lkeys, u64* lcnt, const ContactsOut& o, int a, int b) {
  if (a == b) return;
  const u64 key = a < b ? ((u64)(unsigned int)a << 32) | (unsigned int)b : ((u64)(unsigned int)b << 32) | (unsigned int)a;
  if (key == r.key) { ++r.n; return; }
  if (r.n) add_pair(lkeys, lcnt, o, r.key, r.n);
  r.key = key;
  r.n = 1;
}

__global__ __launch_bounds__(BLOCK) void contacts_kernel(const int* __restrict__ lab, int vec, int vec_y, int vec_z, int zfaces,
                                                         long long npix, int Z, int Y, int X, int nid, long long ntiles,
                                                         long long tiles_per_block, ContactsOut o) {
  __shared__ u64 lkeys[CSLOTS];
  __shared__ u64 lcnt[CSLOTS];
  for (int s = threadIdx.x; s < CSLOTS; s += BLOCK) { lkeys[s] = 0; lcnt[s] = 0; }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const long long plane = (long long)Y * X;
  const long long t0 = (long long)blockIdx.x * tiles_per_block;
  const long long t1 = t0 + tiles_per_block < ntiles ? t0 + tiles_per_block : ntiles;
  bool any_bad = false;
  for (long long t = t0; t < t1; ++t) {
    const long long p0 = t * TILE + (long long)threadIdx.x * PPL;
    int l[PPL], d[PPL], u[PPL];                         // own pixels, one row down, one slice down (flat index + X, + Y*X)
    load_labels(lab, vec != 0, p0, npix, l);
    any_bad |= clamp_labels(l, nid);
    load_labels(lab, vec_y != 0, p0 + X, npix, d);
    clamp_labels(d, nid);
    if (zfaces) {
      load_labels(lab, vec_z != 0, p0 + plane, npix, u);
      clamp_labels(u, nid);
    } else {
#pragma unroll
      for (int k = 0; k < PPL; ++k) u[k] = l[k];
    }
    // the +x neighbour of the lane's last pixel: the next lane's first, or a load for the wave's last lane
    int right = __shfl_down(l[0], 1);
    if (lane == 63) {
      right = p0 + PPL < npix ? lab[p0 + PPL] : 0;
      if ((unsigned)right >= (unsigned)nid) right = 0;
    }
    // npix < 2^32: 32-bit divisions
    const unsigned int pu = p0 < npix ? (unsigned int)p0 : 0u;
    const unsigned int r = pu / (unsigned int)X;
    int x = (int)(pu - r * (unsigned int)X);
    int z = (int)(r / (unsigned int)Y);
    int y = (int)(r - (unsigned int)z * (unsigned int)Y);

    // away from every image edge the stored neighbours are the real ones: nothing to emit if they all equal l[0]
    const bool interior = p0 + PPL <= npix && x > 0 && x + PPL < X && y > 0 && y + 1 < Y && (!zfaces || (z > 0 && z + 1 < Z));
    int diff = right ^ l[0];
#pragma unroll
    for (int k = 0; k < PPL; ++k) diff |= (l[k] ^ l[0]) | (d[k] ^ l[0]) | (u[k] ^ l[0]);
    const bool noisy = p0 < npix && (!interior || diff != 0);
    if (__ballot(noisy) == 0ull) continue;
    if (!noisy) continue;

    // per pixel: is it in the image, and on which edges
    bool in[PPL], x_lo[PPL], x_hi[PPL], y_lo[PPL], y_hi[PPL], z_lo[PPL], z_hi[PPL];
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      in[k] = p0 + k < npix;
      x_lo[k] = x == 0; x_hi[k] = x == X - 1;
      y_lo[k] = y == 0; y_hi[k] = y == Y - 1;
      z_lo[k] = z == 0; z_hi[k] = z == Z - 1;
      if (++x == X) { x = 0; if (++y == Y) { y = 0; ++z; } }
    }
    PairRun run = {0ull, 0u};
#pragma unroll
    for (int k = 0; k < PPL; ++k)
      if (in[k]) face(run, lkeys, lcnt, o, l[k], y_hi[k] ? 0 : d[k]);
#pragma unroll
    for (int k = 0; k < PPL; ++k)
      if (in[k] && y_lo[k]) face(run, lkeys, lcnt, o, l[k], 0);
    if (zfaces) {
#pragma unroll
      for (int k = 0; k < PPL; ++k)
        if (in[k]) face(run, lkeys, lcnt, o, l[k], z_hi[k] ? 0 : u[k]);
#pragma unroll
      for (int k = 0; k < PPL; ++k)
        if (in[k] && z_lo[k]) face(run, lkeys, lcnt, o, l[k], 0);
    }
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      if (!in[k]) continue;
      if (x_lo[k]) face(run, lkeys, lcnt, o, l[k], 0);
      face(run, lkeys, lcnt, o, l[k], x_hi[k] ? 0 : (k < PPL - 1 ? l[(k + 1) & (PPL - 1)] : right));
    }
    if (run.n) add_pair(lkeys, lcnt, o, run.key, run.n);
  }
  if (any_bad) atomicOr(o.info, 1);
  __syncthreads();

  for (int s = threadIdx.x; s < CSLOTS; s += BLOCK)
    if (lkeys[s]) pair_to_global(o, lkeys[s], lcnt[s], mix64(lkeys[s]));
}

// ---------------------------------------------------------------------------------------------------------
// Perimeter (2-D): scikit-image's perimeter(mask, neighbourhood=4) restated on the full map.  A pixel of object i is a
// border pixel if one of its 4 neighbours is not i (another object, background or the outside of the image); its code is
// 1 + 2 n4 + 10 nd with n4 / nd the border pixels OF i among its 4 edge / 4 diagonal neighbours.  That is a 5 x 5
// dependency: a block stages a PT x PT tile with a halo of 2 in LDS, derives the border flags of the tile plus a halo of
// 1 (kept as the id itself, 0: no border pixel), then the codes of the tile, counted per id and weight class in the
// id-keyed LDS table and flushed once per block.

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

// ---------------------------------------------------------------------------------------------------------
// Topology: per object the sums over all 2 x 2 (2-D) / 2 x 2 x 2 (3-D) windows of the zero-padded map from which the
// host forms the Euler numbers, the Crofton perimeter and the 3-D surface area (clx.h has the definitions).  For an id i
// and a window, bit v of the mask says whether voxel v = dz * 4 + dy * 2 + dx of the window is i; the five contributions
// T1 T2 T3 E_hi E_lo are functions of the mask alone, tabulated below from their definitions at compile time.  A window
// belongs to the pixel at its low corner; a pixel in the first column / row / slice also owns the windows that reach
// into the padding on that side (up to 2^nd for a corner pixel), as contacts_kernel assigns the backward faces.  The
// frame is contacts_kernel's: own pixels, one row down, one slice down and both down, each with its +x neighbour from
// the next lane; a wave none of whose lanes sees two different values (or one id next to the image edge) leaves the trip.
// One instantiation per window size: the 2-D one neither loads nor carries the two rows of the slice below.

constexpr int NT = 5;                   // T1 T2 T3 E_hi E_lo
constexpr int TOPO_2D = 256;            // the 16 masks of a 2 x 2 window follow the 256 of a 2 x 2 x 2 one

constexpr int popcount3(int v) { return (v & 1) + ((v >> 1) & 1) + ((v >> 2) & 1); }

// the five contributions of one mask, a signed byte each (none above 12 in absolute value: static_assert below), T1 lowest
constexpr u64 topo_entry(int nd, int m) {
  const int nv = 1 << nd;
  int v[NT] = {0, 0, 0, 0, 0};
  for (int a = 0; a < nv; ++a)                          // voxel pairs with different bits, by the coordinates they differ in
    for (int b = a + 1; b < nv; ++b)
      if (((m >> a) ^ (m >> b)) & 1) ++v[popcount3(a ^ b) - 1];
  for (int axes = 0; axes < nv; ++axes) {               // a d-cell through the vertex: d chosen axes and a side along each;
    const int d = popcount3(axes), w = 1 << (nd - d);   // its voxels are the w window voxels on those sides
    for (int side = 0; side < nv; ++side) {
      if (side & ~axes) continue;
      bool any = false, all = true;
      for (int k = 0; k < nv; ++k)
        if ((k & axes) == side) {
          if ((m >> k) & 1) any = true;
          else all = false;
        }
      if (any) v[3] += (d & 1) ? -w : w;
      if (all) v[4] += ((nd - d) & 1) ? -w : w;
    }
  }
  u64 e = 0;
  for (int q = 0; q < NT; ++q) e |= (u64)(unsigned char)(signed char)v[q] << (8 * q);
  return e;
}

struct TopoTable {
  u64 e[TOPO_2D + 16];
};
constexpr TopoTable make_topo_table() {
  TopoTable t = {};
  for (int m = 0; m < 256; ++m) t.e[m] = topo_entry(3, m);
  for (int m = 0; m < 16; ++m) t.e[TOPO_2D + m] = topo_entry(2, m);
  return t;
}
constexpr int topo_max_abs() {
  const TopoTable t = make_topo_table();
  int worst = 0;
  for (int m = 0; m < TOPO_2D + 16; ++m)
    for (int q = 0; q < NT; ++q) {
      const int v = (int)(signed char)(unsigned char)(t.e[m] >> (8 * q));
      worst = v > worst ? v : (-v > worst ? -v : worst);
    }
  return worst;
}
static_assert(topo_max_abs() <= 12, "a window adds at most 12 to a count: topology_kernel's 32-bit block sums rely on it");
__device__ const TopoTable topo_table = make_topo_table();

// what a lane has met of one id and not yet added to the block's table
struct TopoRun {
  int id;
  int v[NT];
};

__device__ void add_topology(int* keys, int (*acc)[SLOTS], long long* counts, const TopoRun& r) {
  const int s = find_slot(keys, r.id);
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    if (r.v[q] == 0) continue;
    if (s >= 0) atomicAdd(&acc[q][s], r.v[q]);
    else atomicAdd(reinterpret_cast<u64*>(counts) + (size_t)r.id * NT + q, (u64)(long long)r.v[q]);   // two's complement
  }
}

// one window, voxel v in w[v] (outside the image: 0): every distinct non-zero id gets the contributions of its mask
template <int NV>
__device__ __forceinline__ void topology_window(TopoRun& run, int* keys, int (*acc)[SLOTS], long long* counts,
                                                const u64* tab, const int (&w)[NV]) {
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int id = w[j];
    bool first = id != 0;
    int mask = 0;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (i < j) first = first && w[i] != id;
      mask |= (w[i] == id) << i;
    }
    if (!first) continue;
    const u64 e = tab[mask];
    if (e == 0) continue;                               // every voxel of the window is `id`
    if (id != run.id) {
      if (run.id) add_topology(keys, acc, counts, run);
      run.id = id;
#pragma unroll
      for (int q = 0; q < NT; ++q) run.v[q] = 0;
    }
#pragma unroll
    for (int q = 0; q < NT; ++q) run.v[q] += (int)(signed char)(unsigned char)(e >> (8 * q));
  }
}

__global__ void topology_init(long long* __restrict__ counts, int* __restrict__ bad, int nid) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *bad = 0;
  if (i >= nid) return;
  for (int q = 0; q < NT; ++q) counts[(size_t)i * NT + q] = 0;
}

struct TopoVec {
  int v[4];                             // 16-byte loads allowed for the own pixels, one row down, one slice down, both down
};

// ZWIN: 2 x 2 x 2 windows (nd == 3); else 2 x 2
template <bool ZWIN>
__global__ __launch_bounds__(BLOCK) void topology_kernel(const int* __restrict__ lab, TopoVec vec, long long npix, int Z, int Y, int X,
                                                         int nid, long long ntiles, long long tiles_per_block,
                                                         long long* __restrict__ counts, int* __restrict__ bad) {
  constexpr int NV = ZWIN ? 8 : 4;      // voxels of a window
  constexpr int NA = ZWIN ? 4 : 2;      // rows of pixels a lane holds: own, one row down, one slice down, both down
  __shared__ int keys[SLOTS];
  // A block's partial sums fit 32 bits: it owns at most tiles_per_block * TILE <= 2^22 + TILE pixels (npix < 2^32 over
  // MAX_GRID = 2^10 blocks), a pixel at most 8 windows, and a window adds at most 12 in absolute value to any of the
  // five counts of an id (12 pairs of a kind; the static_assert on the table covers E_hi and E_lo): below 2^30.
  __shared__ int acc[NT][SLOTS];
  __shared__ u64 tab[1 << NV];
  for (int s = threadIdx.x; s < SLOTS; s += BLOCK) {
    keys[s] = 0;
    for (int q = 0; q < NT; ++q) acc[q][s] = 0;
  }
  for (int s = threadIdx.x; s < (1 << NV); s += BLOCK) tab[s] = topo_table.e[(ZWIN ? 0 : TOPO_2D) + s];
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const long long plane = (long long)Y * X;
  const long long off[4] = {0, X, plane, plane + X};    // flat index of the four rows of pixels, from the own
  const long long t0 = (long long)blockIdx.x * tiles_per_block;
  const long long t1 = t0 + tiles_per_block < ntiles ? t0 + tiles_per_block : ntiles;
  bool any_bad = false;
  for (long long t = t0; t < t1; ++t) {
    const long long p0 = t * TILE + (long long)threadIdx.x * PPL;
    // v[a][0..3]: the lane's pixels (a == 0) and those one row / one slice / both down; v[a][4]: the +x neighbour of the
    // last, the next lane's first, or a load for the wave's last lane.  Every load of the trip is issued before the
    // first value is looked at: one round of memory latency per trip.
    int v[NA][PPL + 1];
    int right[NA];
    if ((t + 1) * TILE + off[NA - 1] < npix) {          // the same for the whole block: no load of the trip leaves the map
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        const int* src = lab + p0 + off[a];
        if (vec.v[a]) {
          const i32x4 q = *reinterpret_cast<const i32x4*>(src);
          v[a][0] = q[0]; v[a][1] = q[1]; v[a][2] = q[2]; v[a][3] = q[3];
        } else {
#pragma unroll
          for (int k = 0; k < PPL; ++k) v[a][k] = src[k];
        }
        right[a] = lane == 63 ? src[PPL] : 0;
      }
    } else {
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        load_labels(lab, vec.v[a] != 0, p0 + off[a], npix, v[a]);
        right[a] = lane == 63 && p0 + PPL + off[a] < npix ? lab[p0 + PPL + off[a]] : 0;
      }
    }
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const int next = __shfl_down(v[a][0], 1);
      v[a][PPL] = lane == 63 ? right[a] : next;
    }
    // smallest and largest of everything the lane holds, as unsigned: equal if it is all one value, and the largest
    // shows an id outside [0, nid).  Every value is a pixel of the map (or 0 past its end), so flagging it here is right.
    unsigned int lo = (unsigned int)v[0][0], hi = lo;
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
      for (int k = 0; k <= PPL; ++k) {
        lo = min(lo, (unsigned int)v[a][k]);
        hi = max(hi, (unsigned int)v[a][k]);
      }
    if (hi >= (unsigned int)nid) {                      // out-of-range ids become background (never an index)
      any_bad = true;
      lo = 0xffffffffu;
      hi = 0u;
#pragma unroll
      for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int k = 0; k <= PPL; ++k) {
          if ((unsigned int)v[a][k] >= (unsigned int)nid) v[a][k] = 0;
          lo = min(lo, (unsigned int)v[a][k]);
          hi = max(hi, (unsigned int)v[a][k]);
        }
    }
    // A lane that holds nothing but background adds nothing wherever it lies: its windows hold these values or the
    // outside.  A lane that holds one id adds nothing if it lies away from every image edge: the stored neighbours are
    // then the real ones, it owns no window in the padding, and each of its windows has every bit set.
    bool noisy = false;
    int x = 0, y = 0, z = 0;
    if (p0 < npix && hi != 0u) {
      // npix < 2^32: 32-bit divisions
      const unsigned int pu = (unsigned int)p0;
      const unsigned int r = pu / (unsigned int)X;
      x = (int)(pu - r * (unsigned int)X);
      z = (int)(r / (unsigned int)Y);
      y = (int)(r - (unsigned int)z * (unsigned int)Y);
      const bool interior = p0 + PPL <= npix && x > 0 && x + PPL < X && y > 0 && y + 1 < Y && (!ZWIN || (z > 0 && z + 1 < Z));
      noisy = lo != hi || !interior;
    }
    if (__ballot(noisy) == 0ull) continue;
    if (!noisy) continue;

    TopoRun run = {0, {0, 0, 0, 0, 0}};
#pragma unroll 1
    for (int k = 0; k < PPL; ++k) {
      // the lane's pixel k is element 0 of the rows, its +x neighbour element 1 (they move down below)
      if (p0 + k < npix) {
        const bool x_hi = x == X - 1, y_hi = y == Y - 1;
        // the pixel's forward cube c[dz * 4 + dy * 2 + dx]; past the last column / row / slice: outside, 0
        int c[NV];
        c[0] = v[0][0];
        c[1] = x_hi ? 0 : v[0][1];
        c[2] = y_hi ? 0 : v[1][0];
        c[3] = (y_hi || x_hi) ? 0 : v[1][1];
        // bit 0 / 1 / 2: the window's low corner lies one column / row / slice before the pixel, in the padding
        int lows = (x == 0 ? 1 : 0) | (y == 0 ? 2 : 0);
        if constexpr (ZWIN) {
          const bool z_hi = z == Z - 1;
          c[4] = z_hi ? 0 : v[2][0];
          c[5] = (z_hi || x_hi) ? 0 : v[2][1];
          c[6] = (z_hi || y_hi) ? 0 : v[3][0];
          c[7] = (z_hi || y_hi || x_hi) ? 0 : v[3][1];
          lows |= z == 0 ? 4 : 0;
        }
        // a cube of one value away from the low edges is one window with no bit or every bit set
        bool same = lows == 0;
#pragma unroll
        for (int j = 1; j < NV; ++j) same = same && c[j] == c[0];
#pragma unroll 1
        for (int s = same ? NV : 0; s < NV; ++s) {
          if (s & ~lows) continue;
          int w[NV];
#pragma unroll
          for (int j = 0; j < NV; ++j) w[j] = c[j];
          if (s & 1) {
#pragma unroll
            for (int j = 0; j < NV; j += 2) { w[j + 1] = w[j]; w[j] = 0; }
          }
          if (s & 2) {
#pragma unroll
            for (int j = 0; j < NV; j += 4) { w[j + 2] = w[j]; w[j + 3] = w[j + 1]; w[j] = w[j + 1] = 0; }
          }
          if constexpr (ZWIN) {
            if (s & 4) {
#pragma unroll
              for (int j = 0; j < 4; ++j) { w[j + 4] = w[j]; w[j] = 0; }
            }
          }
          topology_window<NV>(run, keys, acc, counts, tab, w);
        }
      }
#pragma unroll
      for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int j = 0; j < PPL; ++j) v[a][j] = v[a][j + 1];
      if (++x == X) { x = 0; if (++y == Y) { y = 0; ++z; } }
    }
    if (run.id) add_topology(keys, acc, counts, run);
  }
  if (any_bad) *bad = 1;
  __syncthreads();

  for (int s = threadIdx.x; s < SLOTS; s += BLOCK) {
    const int label = keys[s];
    if (label == 0) continue;
#pragma unroll
    for (int q = 0; q < NT; ++q)
      if (acc[q][s]) atomicAdd(reinterpret_cast<u64*>(counts) + (size_t)label * NT + q, (u64)(long long)acc[q][s]);
  }
}

// ---------------------------------------------------------------------------------------------------------
// Convex hull (clx.h has the definitions): an object is the union of its pixels as closed unit squares, so its hull is
// that of the pixels' corner lattice points, and the hull of a set is the hull of the extreme points of its rows.
//   hull_span_kernel    the map pass, in moments_kernel's frame: per (object, row) of the object's bounding box the
//                       smallest and the largest x that carries the id.  A run of one id in one row costs one atomicMin and
//                       one atomicMax, whatever its length; neither returns a value, so a lane waits for its box only.
//   hull_object_kernel  a wave per object.  First a lane per (slice, side) runs Andrew's monotone chain over the rows'
//                       corner points (on lattice line y' the left chain has min(xmin[y'-1], xmin[y']), the right one
//                       max(xmax[y'-1], xmax[y']) + 1; the rows are sorted by y already), keeping strict vertices only.
//                       Then the wave forms A2 and NV, F2 over all vertex pairs and (C, L2) over all edge x vertex pairs.
// The rows of object i start at row_base[i]; row (z, y) is row_base[i] + (z - zmin) (ymax - ymin + 1) + (y - ymin).  The
// bounding boxes and row_base come from the caller and are not trusted: hull_box checks a box against the image and the
// row count before any index is formed from it.

struct HullIn {
  const int* bbox;
  const long long* row_base;
  long long rows;
  int Z, Y, X;
};

// the workspace: 12 ints a row.  Chain `side` (0 left, 1 right) of the slice whose first row is r keeps its points
// (y, x) from point index side * 2 * rows + 2 * r on: a slice of h rows has at most h + 1 <= 2 h points a chain.
struct HullWs {
  int* xmin;                            // [rows]     0x7fffffff: no pixel of the id in the row
  int* xmax;                            // [rows]     -1: the same
  int* cnt;                             // [rows][2]  points of the two chains, at a slice's first row
  int* pts;                             // [4 * rows][2]
};
constexpr int HULL_WS_INTS = 12;
constexpr int HULL_BATCH = 8;           // rows a chain loads at once
constexpr int HULL_MAX_GRID = 4096;     // hull_span_kernel has no table to flush at a block's end: more, shorter blocks hide its latency

// b: the box of `id`, *base: its first row; false: absent, outside the image, or its rows do not lie in [0, rows)
__device__ __forceinline__ bool hull_box(const HullIn& in, int id, int* b, long long* base) {
#pragma unroll
  for (int k = 0; k < 6; ++k) b[k] = in.bbox[(size_t)id * 6 + k];
  if (b[0] < 0 || b[1] < 0 || b[2] < 0 || b[3] < b[0] || b[4] < b[1] || b[5] < b[2] || b[3] >= in.Z || b[4] >= in.Y || b[5] >= in.X)
    return false;
  const long long rb = in.row_base[id];
  const long long n = (long long)(b[3] - b[0] + 1) * (b[4] - b[1] + 1);        // <= Z * Y < 2^32
  if (rb < 0 || rb > in.rows - n) return false;
  *base = rb;
  return true;
}

// pixels x0 .. x1 of `label` in row (z, y); false: the id's box does not contain them (nothing is written)
__device__ bool add_span(const HullIn& in, const HullWs& w, int label, int z, int y, int x0, int x1) {
  int b[6];
  long long base;
  if (!hull_box(in, label, b, &base) || z < b[0] || z > b[3] || y < b[1] || y > b[4] || x0 < b[2] || x1 > b[5]) return false;
  const long long r = base + (long long)(z - b[0]) * (b[4] - b[1] + 1) + (y - b[1]);
  atomicMin(w.xmin + r, x0);
  atomicMax(w.xmax + r, x1);
  return true;
}

__global__ void hull_init(HullWs w, long long rows, int* __restrict__ bad) {
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 == 0) *bad = 0;
  for (long long i = i0; i < rows; i += (long long)gridDim.x * blockDim.x) {
    w.xmin[i] = 0x7fffffff;
    w.xmax[i] = -1;
  }
}

__global__ __launch_bounds__(BLOCK) void hull_span_kernel(const int* __restrict__ lab, int vec, long long npix, int nid,
                                                          long long ntiles, long long tiles_per_block, HullIn in, HullWs w,
                                                          int* __restrict__ bad) {
  const int lane = threadIdx.x & 63;
  const int Y = in.Y, X = in.X;
  const long long t0 = (long long)blockIdx.x * tiles_per_block;
  const long long t1 = t0 + tiles_per_block < ntiles ? t0 + tiles_per_block : ntiles;
  int any_bad = 0;
  for (long long t = t0; t < t1; ++t) {
    const long long p0 = t * TILE + (long long)threadIdx.x * PPL;
    int l[PPL];
    load_labels(lab, vec != 0, p0, npix, l);
    if (clamp_labels(l, nid)) any_bad |= 1;
    if (__ballot((l[0] | l[1] | l[2] | l[3]) != 0) == 0ull) continue;   // a wave of background
    // npix < 2^32: 32-bit divisions
    const unsigned int pu = p0 < npix ? (unsigned int)p0 : 0u;
    const unsigned int r = pu / (unsigned int)X;
    int x = (int)(pu - r * (unsigned int)X);
    int z = (int)(r / (unsigned int)Y);
    int y = (int)(r - (unsigned int)z * (unsigned int)Y);

    // a run never continues into the next image row
    const bool uni = l[0] > 0 && l[0] == l[1] && l[1] == l[2] && l[2] == l[3] && x + PPL <= X;
    const int lprev = __shfl_up(l[0], 1);
    const unsigned int rprev = __shfl_up(r, 1);
    const u64 unis = __ballot(uni);
    const bool head = !uni || lane == 0 || !((unis >> (lane - 1)) & 1ull) || lprev != l[0] || rprev != r;
    const u64 heads = __ballot(head);
    if (uni) {
      if (head && !add_span(in, w, l[0], z, y, x, x + PPL * run_lanes(heads, lane) - 1)) any_bad |= 2;
    } else {
      int cur = 0, n = 0, cz = 0, cy = 0, cx = 0;
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        if (l[k] != cur || x == 0) {
          if (cur > 0 && !add_span(in, w, cur, cz, cy, cx, cx + n - 1)) any_bad |= 2;
          cur = l[k]; n = 0; cz = z; cy = y; cx = x;
        }
        ++n;
        if (++x == X) { x = 0; if (++y == Y) { y = 0; ++z; } }
      }
      if (cur > 0 && !add_span(in, w, cur, cz, cy, cx, cx + n - 1)) any_bad |= 2;
    }
  }
  if (any_bad) atomicOr(bad, any_bad);
}

// is the width c_a / sqrt(l_a) the better (smaller; at equal widths the one over the shorter edge)?  l == 0: no candidate.
// c <= 2^31 (twice the area of a triangle inside a box of (Y+1)(X+1) <= 2^31 lattice points), so c^2 fits 64 bits; the
// products c_a^2 l_b and c_b^2 l_a are compared exactly as 128-bit numbers.
__device__ __forceinline__ bool narrower(u64 ca, u64 la, u64 cb, u64 lb) {
  if (la == 0 || lb == 0) return la != 0;
  const u64 qa = ca * ca, qb = cb * cb;
  const u64 ah = __umul64hi(qa, lb), al = qa * lb, bh = __umul64hi(qb, la), bl = qb * la;
  if (ah != bh) return ah < bh;
  if (al != bl) return al < bl;
  return la < lb;
}

__global__ __launch_bounds__(BLOCK) void hull_object_kernel(HullIn in, HullWs w, int nd, int nid, long long* __restrict__ hull) {
  const int lane = threadIdx.x & 63;
  const long long idl = (long long)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
  const int id = idl < nid ? (int)idl : 0;
  int b[6];
  long long base = 0;
  const bool valid = id > 0 && hull_box(in, id, b, &base);
  const long long S = valid ? b[3] - b[0] + 1 : 0;      // slices
  const long long h = valid ? b[4] - b[1] + 1 : 0;      // rows a slice
  const long long pts_side = 2 * in.rows;               // points of all left chains

  // a lane per chain: the points are met in the order of y, so the stack is the chain
  for (long long c = lane; c < 2 * S; c += 64) {
    const int side = (int)(c & 1);
    const long long r0 = base + (c >> 1) * h;
    const int* span = side ? w.xmax + r0 : w.xmin + r0;
    const int none = side ? -1 : 0x7fffffff;
    int* st = w.pts + 2 * (side * pts_side + 2 * r0);
    int n = 0, prev = none;
    long long ay = 0, ax = 0, by = 0, bx = 0;           // the two points on top of the stack, st[n - 2] and st[n - 1]
    for (long long k0 = 0; k0 <= h; k0 += HULL_BATCH) {
      // the rows of a batch are loaded before the first is looked at: one round of memory latency per batch, and a
      // line that pops nothing touches memory with its store only
      int s[HULL_BATCH];
#pragma unroll
      for (int j = 0; j < HULL_BATCH; ++j) s[j] = k0 + j < h ? span[k0 + j] : none;
#pragma unroll
      for (int j = 0; j < HULL_BATCH; ++j) {
        if (k0 + j > h) continue;                       // lattice line ymin + k, between rows k - 1 and k, k = k0 + j <= h
        const int cur = s[j];
        int px = side ? (prev > cur ? prev : cur) : (prev < cur ? prev : cur);
        prev = cur;
        if (px == none) continue;                       // both rows are empty: no corner on this line
        px += side;
        const int py = b[1] + (int)(k0 + j);
        while (n >= 2) {
          const long long cross = (by - ay) * (px - ax) - (bx - ax) * (py - ay);    // coordinates <= 2^30: below 2^61
          if (side ? cross < 0 : cross > 0) break;      // the middle point lies strictly outside the line a -> p
          --n;
          by = ay;
          bx = ax;
          if (n >= 2) { ay = st[2 * n - 4]; ax = st[2 * n - 3]; }
        }
        st[2 * n] = py;
        st[2 * n + 1] = px;
        ++n;
        ay = by; ax = bx;
        by = py; bx = px;
      }
    }
    w.cnt[2 * r0 + side] = n;
  }
  __syncthreads();                                      // the chains are in global memory for the whole wave
  if (idl >= nid) return;
  if (!valid) {
    if (lane < 5) hull[(size_t)id * 5 + lane] = 0;
    return;
  }

  // F2 over all pairs of chains (ca <= cb) and all pairs of their points; in 3-D a point of slice s stands at s and s + 1
  u64 f2 = 0;
  for (long long ca = 0; ca < 2 * S; ++ca) {
    const long long ra = base + (ca >> 1) * h;
    const int na = w.cnt[2 * ra + (ca & 1)];
    if (na == 0) continue;
    const int* pa = w.pts + 2 * ((ca & 1) * pts_side + 2 * ra);
    for (long long cb = ca; cb < 2 * S; ++cb) {
      const long long rb = base + (cb >> 1) * h;
      const int nb = w.cnt[2 * rb + (cb & 1)];
      if (nb == 0) continue;
      const int* pb = w.pts + 2 * ((cb & 1) * pts_side + 2 * rb);
      const long long dz = nd == 3 ? (cb >> 1) - (ca >> 1) + 1 : 0;
      const long long npairs = (long long)na * nb;
      for (long long t = lane; t < npairs; t += 64) {
        const long long ia = t / nb, ib = t - ia * nb;
        const long long dy = (long long)pa[2 * ia] - pb[2 * ib], dx = (long long)pa[2 * ia + 1] - pb[2 * ib + 1];
        const u64 d2 = (u64)(dy * dy + dx * dx + dz * dz);      // extents < 2^30: below 2^62
        f2 = d2 > f2 ? d2 : f2;
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const u64 o = __shfl_down(f2, d);
    f2 = o > f2 ? o : f2;
  }

  long long a2 = 0, nv = 0;
  u64 bc = 0, bl = 0;
  if (nd == 2) {
    // the polygon: the left chain downwards, then the right chain upwards.  The four chain ends are vertices (extreme on
    // the first / last lattice line) and the chains share no point (right x > left x on every line): NV = nL + nR.
    const int nl = w.cnt[2 * base], nr = w.cnt[2 * base + 1];
    const int* pl = w.pts + 2 * (2 * base);
    const int* pr = w.pts + 2 * (pts_side + 2 * base);
    const int V = nl + nr;
    nv = V;
    auto vertex = [&](int k, long long& vy, long long& vx) {
      const int* p = k < nl ? pl + 2 * k : pr + 2 * (nr - 1 - (k - nl));
      vy = p[0];
      vx = p[1];
    };
    if (V > 0) {
      long long oy, ox;
      vertex(0, oy, ox);
      for (int e = lane; e < V; e += 64) {
        long long ay, ax, by, bx;
        vertex(e, ay, ax);
        vertex(e + 1 < V ? e + 1 : 0, by, bx);
        a2 += (ay - oy) * (bx - ox) - (ax - ox) * (by - oy);    // shoelace about vertex 0: every term within the box
        const long long ey = by - ay, ex = bx - ax;
        u64 c = 0;
        for (int k = 0; k < V; ++k) {
          long long vy, vx;
          vertex(k, vy, vx);
          const long long cr = ey * (vx - ax) - ex * (vy - ay);
          const u64 m = (u64)(cr < 0 ? -cr : cr);
          c = m > c ? m : c;
        }
        const u64 len = (u64)(ey * ey + ex * ex);
        if (narrower(c, len, bc, bl)) { bc = c; bl = len; }
      }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      a2 += __shfl_down(a2, d);
      const u64 oc = __shfl_down(bc, d), ol = __shfl_down(bl, d);
      if (narrower(oc, ol, bc, bl)) { bc = oc; bl = ol; }
    }
    a2 = a2 < 0 ? -a2 : a2;
  }
  if (lane == 0) {
    long long* o = hull + (size_t)id * 5;
    o[0] = a2; o[1] = nv; o[2] = (long long)f2; o[3] = (long long)bc; o[4] = (long long)bl;
  }
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

extern "C" int clx_region_contacts(const int32_t* labels, int nd, int Z, int Y, int X, int nid, int capacity,
                                   unsigned long long* keys, unsigned long long* counts, int32_t* info, clx_stream stream) {
  CLX_REQUIRE(labels && keys && counts && info, "clx_region_contacts: null pointer");
  CLX_REQUIRE(nd == 2 || nd == 3, "clx_region_contacts: nd must be 2 or 3");
  CLX_REQUIRE(Z > 0 && Y > 0 && X > 0, "clx_region_contacts: bad shape");
  CLX_REQUIRE(nd == 3 || Z == 1, "clx_region_contacts: nd == 2 needs Z == 1");
  CLX_REQUIRE(nid >= 1 && nid <= (1 << 24), "clx_region_contacts: nid must lie in [1, 2^24]");
  CLX_REQUIRE(capacity >= 1024 && capacity <= (1 << 28) && (capacity & (capacity - 1)) == 0,
              "clx_region_contacts: capacity must be a power of two in [1024, 2^28]");
  const unsigned __int128 npix128 = (unsigned __int128)Z * (unsigned)Y * (unsigned)X;
  CLX_REQUIRE(npix128 < ((unsigned __int128)1 << 32), "clx_region_contacts: Z * Y * X must be below 2^32");
  const long long npix = (long long)npix128;
  hipStream_t st = (hipStream_t)stream;
  const ContactsOut o = contacts_out(keys, counts, info, capacity);
  contacts_init<<<(capacity + 255) / 256, 256, 0, st>>>(o, capacity);
  const Tiling t = tiling_for(npix);
  const int vec = ((uintptr_t)labels & 15) == 0;
  contacts_kernel<<<t.grid, BLOCK, 0, st>>>(labels, vec, vec && (X & 3) == 0, vec && (((long long)Y * X) & 3) == 0, nd == 3, npix,
                                            Z, Y, X, nid, t.ntiles, t.per_block, o);
  CLX_CHECK_LAUNCH("clx_region_contacts");
  return CLX_OK;
}

extern "C" int clx_region_topology(const int32_t* labels, int nd, int Z, int Y, int X, int nid, long long* counts, int32_t* bad,
                                   clx_stream stream) {
  CLX_REQUIRE(labels && counts && bad, "clx_region_topology: null pointer");
  CLX_REQUIRE(nd == 2 || nd == 3, "clx_region_topology: nd must be 2 or 3");
  CLX_REQUIRE(Z > 0 && Y > 0 && X > 0, "clx_region_topology: bad shape");
  CLX_REQUIRE(nd == 3 || Z == 1, "clx_region_topology: nd == 2 needs Z == 1");
  CLX_REQUIRE(nid >= 1 && nid <= (1 << 24), "clx_region_topology: nid must lie in [1, 2^24]");
  const unsigned __int128 npix128 = (unsigned __int128)Z * (unsigned)Y * (unsigned)X;
  CLX_REQUIRE(npix128 < ((unsigned __int128)1 << 32), "clx_region_topology: Z * Y * X must be below 2^32");
  const long long npix = (long long)npix128;
  hipStream_t st = (hipStream_t)stream;
  topology_init<<<(nid + 255) / 256, 256, 0, st>>>(counts, bad, nid);
  const Tiling t = tiling_for(npix);
  const long long plane = (long long)Y * X;
  const int vec = ((uintptr_t)labels & 15) == 0;
  const TopoVec tv = {{vec, vec && (X & 3) == 0, vec && (plane & 3) == 0, vec && ((plane + X) & 3) == 0}};
  if (nd == 3)
    topology_kernel<true><<<t.grid, BLOCK, 0, st>>>(labels, tv, npix, Z, Y, X, nid, t.ntiles, t.per_block, counts, bad);
  else
    topology_kernel<false><<<t.grid, BLOCK, 0, st>>>(labels, tv, npix, Z, Y, X, nid, t.ntiles, t.per_block, counts, bad);
  CLX_CHECK_LAUNCH("clx_region_topology");
  return CLX_OK;
}

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

extern "C" size_t clx_region_hull_workspace(long long rows) {
  if (rows < 0 || rows > (1ll << 56)) return 0;
  const size_t bytes = (size_t)rows * HULL_WS_INTS * sizeof(int);
  return bytes < 64 ? 64 : bytes;
}

extern "C" int clx_region_hull(const int32_t* labels, int nd, int Z, int Y, int X, int nid, const int32_t* bbox,
                               const long long* row_base, long long rows, void* workspace, size_t workspace_bytes,
                               long long* hull, int32_t* bad, clx_stream stream) {
  CLX_REQUIRE(labels && bbox && row_base && workspace && hull && bad, "clx_region_hull: null pointer");
  CLX_REQUIRE(nd == 2 || nd == 3, "clx_region_hull: nd must be 2 or 3");
  CLX_REQUIRE(Z > 0 && Y > 0 && X > 0, "clx_region_hull: bad shape");
  CLX_REQUIRE(nd == 3 || Z == 1, "clx_region_hull: nd == 2 needs Z == 1");
  CLX_REQUIRE(Z < (1 << 30) && Y < (1 << 30) && X < (1 << 30), "clx_region_hull: Z, Y and X must be below 2^30 (F2 is 64-bit)");
  CLX_REQUIRE(nid >= 1 && nid <= (1 << 24), "clx_region_hull: nid must lie in [1, 2^24]");
  const unsigned __int128 npix128 = (unsigned __int128)Z * (unsigned)Y * (unsigned)X;
  CLX_REQUIRE(npix128 < ((unsigned __int128)1 << 32), "clx_region_hull: Z * Y * X must be below 2^32");
  CLX_REQUIRE(nd == 3 || ((long long)Y + 1) * ((long long)X + 1) <= (1ll << 31),
              "clx_region_hull: nd == 2 needs (Y + 1) * (X + 1) <= 2^31 (C^2 is 64-bit)");
  // an id has at most Z * Y rows
  CLX_REQUIRE(rows >= 0 && rows <= (long long)(nid - 1) * Z * Y, "clx_region_hull: rows must lie in [0, (nid - 1) * Z * Y]");
  CLX_REQUIRE(workspace_bytes >= clx_region_hull_workspace(rows),
              "clx_region_hull: workspace_bytes is below clx_region_hull_workspace(rows)");
  CLX_REQUIRE(((uintptr_t)workspace & 7) == 0, "clx_region_hull: workspace must be 8-byte aligned");
  const long long npix = (long long)npix128;
  hipStream_t st = (hipStream_t)stream;
  int* ws = (int*)workspace;
  const HullWs w = {ws, ws + rows, ws + 2 * rows, ws + 4 * rows};
  const HullIn in = {bbox, row_base, rows, Z, Y, X};
  const long long init_blocks = (rows + 255) / 256;
  hull_init<<<(int)(init_blocks < 1 ? 1 : (init_blocks < 65536 ? init_blocks : 65536)), 256, 0, st>>>(w, rows, bad);
  const Tiling t = tiling_for(npix, HULL_MAX_GRID);
  hull_span_kernel<<<t.grid, BLOCK, 0, st>>>(labels, ((uintptr_t)labels & 15) == 0, npix, nid, t.ntiles, t.per_block, in, w, bad);
  hull_object_kernel<<<(nid + BLOCK / 64 - 1) / (BLOCK / 64), BLOCK, 0, st>>>(in, w, nd, nid, hull);
  CLX_CHECK_LAUNCH("clx_region_hull");
  return CLX_OK;
}
