// "measure" stage: the per-object table users take from skimage.measure.regionprops on the host
// (area, bounding box, centroid, second moments, mean / min / max intensity), as integer sums
// gathered in one pass over the label map on the device:
//   clx_region_moments    pixel count, bounding box, Σ coordinate and Σ coordinate products per id
//   clx_region_intensity  Σ quantised value and min / max (order-preserving keys) of one raw channel per id
// (contacts, perimeter, topology and hull have files of their own: region_contacts.hip, region_perimeter.hip,
// region_topology.hip, region_hull.hip.)
// The two kernels share one structure (region_scan.h).  A lane reads 4 consecutive pixels; a lane whose pixels all carry one
// object id (and lie in one image row, for the moments) is "uniform".  A ballot over the wave cuts the 64 lanes
// into runs of uniform lanes with the same id (and row); the first lane of a run owns it.  The geometric sums
// of a run follow in closed form from its start and length, the intensities from a segmented wave reduction.
// Lanes on an object's edge walk their 4 pixels one by one.  Runs are combined in a table in LDS keyed by id
// (open addressing, PROBES tries, then straight to global memory) which the block adds to the outputs when
// its pixels are done: one 64-bit integer atomic per id, quantity and block.  Integer adds, min and max
// commute, so the outputs are the same bits in every run.
#include "region_sums.h"

namespace {

constexpr int NQ = 10;                  // area, Σz Σy Σx, Σzz Σyy Σxx Σzy Σzx Σyx

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
  const Tiles tiles = block_tiles(ntiles, tiles_per_block);
  bool any_bad = false;
  for (long long t = tiles.t0; t < tiles.t1; ++t) {
    const long long p0 = lane_pixel(t);
    int l[PPL];
    load_labels(lab, vec != 0, p0, npix, l);
    any_bad |= clamp_labels(l, nid);
    const PixelInRow at = pixel_at(p0, npix, Y, X);
    Pixel p = at.p;

    // a run never continues into the next image row: the closed forms hold inside one row only
    const bool uni = l[0] > 0 && l[0] == l[1] && l[1] == l[2] && l[2] == l[3] && p.x + PPL <= X;
    const Heads h = run_heads(uni, l, at.row, lane);
    if (uni) {
      if (h.head) add_run(keys, acc, box, o, l[0], PPL * run_lanes(h.heads, lane), p.z, p.y, p.x);
    } else {
      int cur = 0, n = 0, cz = 0, cy = 0, cx = 0;
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        if (l[k] != cur || p.x == 0) {
          if (cur > 0) add_run(keys, acc, box, o, cur, n, cz, cy, cx);
          cur = l[k]; n = 0; cz = p.z; cy = p.y; cx = p.x;
        }
        ++n;
        p = next_pixel(p, Y, X);
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

// what a run sums of its pixels
struct Values {
  long long s;
  u64 kmin, kmax;
  __device__ __forceinline__ Values shifted(int d) const { return {__shfl_down(s, d), __shfl_down(kmin, d), __shfl_down(kmax, d)}; }
  __device__ __forceinline__ void take(const Values& o) {
    s += o.s;
    kmin = o.kmin < kmin ? o.kmin : kmin;
    kmax = o.kmax > kmax ? o.kmax : kmax;
  }
};

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
  const Tiles tiles = block_tiles(ntiles, tiles_per_block);
  int any_bad = 0;
  for (long long t = tiles.t0; t < tiles.t1; ++t) {
    const long long p0 = lane_pixel(t);
    int l[PPL];
    load_labels(lab, vec_lab != 0, p0, npix, l);
    if (clamp_labels(l, nid)) any_bad |= BAD_LABEL;
    Raw4<T> rv;                                         // load_raw spelled out: through it the int kernel ran 3 - 7 % slower
    if (vec_raw && p0 + PPL <= npix) {
      rv = *reinterpret_cast<const Raw4<T>*>(raw + p0);
    } else {
#pragma unroll
      for (int k = 0; k < PPL; ++k) rv.v[k] = p0 + k < npix ? raw[p0 + k] : (T)0;
    }
    long long q[PPL];
    u64 key[PPL];
    Values v = {0, ~0ull, 0ull};
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      q[k] = 0;
      key[k] = order_key(rv.v[k]);
      if (l[k] > 0 && !quantise<T>(rv.v[k], shift, bound, &q[k])) { l[k] = 0; any_bad |= BAD_VALUE; }   // the pixel is skipped
      v.s += q[k];
      v.kmin = key[k] < v.kmin ? key[k] : v.kmin;
      v.kmax = key[k] > v.kmax ? key[k] : v.kmax;
    }
    const bool uni = l[0] > 0 && l[0] == l[1] && l[1] == l[2] && l[2] == l[3];
    const Heads h = run_heads(uni, l, lane);
    v = reduce_run(v, lane, lane + run_lanes(h.heads, lane));
    if (uni) {
      if (h.head) add_values(keys, ssum, smin, smax, isum, vkey, l[0], v.s, v.kmin, v.kmax);
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

}  // namespace

extern "C" int clx_region_moments(const int32_t* labels, int Z, int Y, int X, int nid, unsigned long long* area,
                                  int32_t* bbox, unsigned long long* sum1, unsigned long long* sum2, int32_t* bad,
                                  clx_stream stream) {
  CLX_REQUIRE(labels && area && bbox && sum1 && sum2 && bad, "clx_region_moments: null pointer");
  CLX_REQUIRE(Z > 0 && Y > 0 && X > 0, "clx_region_moments: bad shape");
  CLX_REQUIRE(nid >= 1 && nid <= (1 << 24), "clx_region_moments: nid must lie in [1, 2^24]");
  long long npix = 0;
  if (clx_map_bound("clx_region_moments", Z, Y, X, 32, &npix) != CLX_OK) return CLX_ERR_ARG;
  const unsigned long long m = (unsigned long long)((Z > Y ? (Z > X ? Z : X) : (Y > X ? Y : X)) - 1);
  CLX_REQUIRE((unsigned __int128)(m * m) * (unsigned __int128)npix < ((unsigned __int128)1 << 63),
              "clx_region_moments: (largest extent - 1)^2 * Z * Y * X must be below 2^63 (the second moments are 64-bit)");
  hipStream_t st = (hipStream_t)stream;
  const MomentsOut o = {area, sum1, sum2, bbox};
  moments_init<<<(nid + 255) / 256, 256, 0, st>>>(o, bad, nid);
  const Tiling t = tiling_for(npix);
  moments_kernel<<<t.grid, BLOCK, 0, st>>>(labels, aligned16(labels), npix, Y, X, nid, t.ntiles, t.per_block, o, bad);
  CLX_CHECK_LAUNCH("clx_region_moments");
  return CLX_OK;
}

extern "C" int clx_region_intensity(const int32_t* labels, const void* raw, int raw_type, long long npix, int nid, int shift,
                                    long long* isum, unsigned long long* vkey, int32_t* bad, clx_stream stream) {
  const char* who = "clx_region_intensity";
  CLX_REQUIRE(labels && raw && isum && vkey && bad, "%s: null pointer", who);
  if (require_raw_channel(who, raw_type, nid) != CLX_OK) return CLX_ERR_ARG;
  CLX_REQUIRE(npix > 0 && npix < (1ll << 32), "%s: npix must lie in [1, 2^32)", who);
  hipStream_t st = (hipStream_t)stream;
  intensity_init<<<(nid + 255) / 256, 256, 0, st>>>(isum, vkey, bad, nid);
  const Tiling t = tiling_for(npix);
  launch_for_raw(raw_type, [&](auto v) {
    using T = decltype(v);
    intensity_kernel<T><<<t.grid, BLOCK, 0, st>>>(labels, (const T*)raw, aligned16(labels), aligned16(raw), npix, nid, shift,
                                                   value_bound(npix), t.ntiles, t.per_block, isum, vkey, bad);
  });
  CLX_CHECK_LAUNCH(who);
  return CLX_OK;
}
