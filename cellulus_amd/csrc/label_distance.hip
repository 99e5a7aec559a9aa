// Label-aware squared Euclidean distance map and the per-object reduction over it (the measure stage's thickness
// descriptor: the largest inscribed circle / ball).
//   clx_label_distance_sq   d2(p) = min |p - q|^2 over the pixels q whose value differs from labels[p]; 0 on background
//   clx_region_inscribed    per id: max d2, the smallest linear index that attains it, Σ d2
//
// The distance map is the separable min-plus transform of edt.hip with one change.  Pass X leaves, for an object pixel,
// g(p) = the squared distance to the nearest pixel OF ITS ROW with another value (INF: none).  Pass Y takes
//   min over q of the column of (y - y')^2 + f(q),   f(q) = g(q) if labels[q] == labels[p], else 0,
// and pass Z the same on pass Y's result.  Why f is right: split the candidates (pixels with another value than p's) by
// the column pixel q they share a row with.  If q has another value than p, q itself is a candidate and the nearest of its
// row: f = 0.  If q has p's value, "another value than q's" and "another value than p's" are the same set, so g(q), taken
// for q, is the row's answer for p as well.  The minimum over q of the two cases is the minimum over all candidates.
// The outward search stops at the first d with d^2 >= best: f >= 0, so nothing farther along the axis can win.  That is
// exact and needs no cap; the search of an object pixel ends within its own distance, background pixels are not searched.
// With `edge` the layer of 0 around the map adds the candidates (c + 1)^2 and (n - c)^2 on every counted axis (the nearest
// padding pixel along an axis lies straight out: the other coordinates stay).
// Stored values are at most INF = 2^30 and d^2 < best <= 2^30 inside a search, so a sum stays below 2^31: unsigned adds.
#include "region_scan.h"

namespace {

constexpr unsigned int DIST_INF = (unsigned int)CLX_DIST_INF;
constexpr int PASS_MAX_GRID = 4096;     // blocks of BLOCK pixels a trip

// candidates the padding adds along an axis of extent n at coordinate c: min(c + 1, n - c)^2 (n <= 2^15: at most 2^30)
__device__ __forceinline__ unsigned int padding_sq(int c, int n) {
  const unsigned int m = (unsigned int)min(c + 1, n - c);
  return m * m;
}

__global__ __launch_bounds__(BLOCK) void distance_pass_x(const int* __restrict__ lab, int* __restrict__ g, int X,
                                                         long long npix, int edge) {
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < npix; i += (long long)gridDim.x * BLOCK) {
    const int L = lab[i];
    unsigned int best = 0;
    if (L != 0) {
      const int x = (int)((unsigned int)i % (unsigned int)X);        // npix < 2^32
      const int* row = lab + (i - x);
      best = edge ? padding_sq(x, X) : DIST_INF;
      for (int d = 1; (unsigned int)(d * d) < best; ++d) {           // with edge: d < min(x + 1, X - x), both taps exist
        const int xl = x - d, xr = x + d;
        if (xl < 0 && xr >= X) break;
        if ((xl >= 0 && row[xl] != L) || (xr < X && row[xr] != L)) {
          best = (unsigned int)(d * d);
          break;
        }
      }
    }
    g[i] = (int)best;
  }
}

// the axis with stride `stride` and extent n (coordinate = (i / stride) % n); g: the pass before, read where the value agrees
__global__ __launch_bounds__(BLOCK) void distance_pass_axis(const int* __restrict__ lab, const int* __restrict__ g,
                                                            int* __restrict__ out, int n, long long stride, long long npix,
                                                            int edge) {
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < npix; i += (long long)gridDim.x * BLOCK) {
    const int L = lab[i];
    unsigned int best = 0;
    if (L != 0) {
      const int p = (int)(((unsigned int)i / (unsigned int)stride) % (unsigned int)n);
      best = (unsigned int)g[i];
      if (edge) best = min(best, padding_sq(p, n));
      for (int d = 1; (unsigned int)(d * d) < best; ++d) {
        const int lo = p - d, hi = p + d;
        if (lo < 0 && hi >= n) break;
        const unsigned int d2 = (unsigned int)(d * d);
        // both taps are loaded before either is used: four independent loads a step
        const long long jl = lo >= 0 ? i - (long long)d * stride : i, jh = hi < n ? i + (long long)d * stride : i;
        const int ll = lab[jl], lh = lab[jh];
        const unsigned int gl = (unsigned int)g[jl], gh = (unsigned int)g[jh];
        if (lo >= 0) best = min(best, d2 + (ll == L ? gl : 0u));
        if (hi < n) best = min(best, d2 + (lh == L ? gh : 0u));
      }
      best = min(best, DIST_INF);
    }
    out[i] = (int)best;
  }
}

// ---------------------------------------------------------------------------------------------------------
// Reduction, in the frame of moments_kernel / intensity_kernel (region_scan.h).  The maximum and where it is attained are
// one 64-bit key, (d2 << 32) | (0xFFFFFFFF - linear index): the larger distance wins, among equal distances the smaller
// index.  d2 <= 2^30 and index <= 2^32 - 2, so the key of a pixel is never 0, which marks an absent id; inscribed_decode
// unpacks the keys once every block has flushed.

__device__ void add_inscribed(int* keys, u64* ssum, u64* smax, u64* __restrict__ out, int label, u64 s, u64 kmax) {
  const int slot = find_slot(keys, label);
  if (slot >= 0) {
    atomicAdd(&ssum[slot], s);
    atomicMax(&smax[slot], kmax);
  } else {
    u64* o = out + (size_t)label * 3;
    atomicAdd(o + 2, s);
    if (kmax > o[0]) atomicMax(o, kmax);                  // the plain read only filters
  }
}

__global__ __launch_bounds__(BLOCK) void inscribed_kernel(const int* __restrict__ lab, const int* __restrict__ dist,
                                                          int vec_lab, int vec_dist, long long npix, int nid, long long ntiles,
                                                          long long tiles_per_block, u64* __restrict__ out,
                                                          int* __restrict__ bad) {
  __shared__ int keys[SLOTS];
  __shared__ u64 ssum[SLOTS], smax[SLOTS];
  for (int s = threadIdx.x; s < SLOTS; s += BLOCK) { keys[s] = 0; ssum[s] = 0; smax[s] = 0; }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const Tiles tiles = block_tiles(ntiles, tiles_per_block);
  int any_bad = 0;
  for (long long t = tiles.t0; t < tiles.t1; ++t) {
    const long long p0 = lane_pixel(t);
    int l[PPL], dv[PPL];
    load_labels(lab, vec_lab != 0, p0, npix, l);
    if (clamp_labels(l, nid)) any_bad |= 1;
    load_labels(dist, vec_dist != 0, p0, npix, dv);       // the same 4-pixel read; past the end: 0
    u64 key[PPL];
    SumKey<true> v = {0, 0};                              // Σ d2 and the largest key
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      if (l[k] > 0 && (unsigned int)dv[k] > DIST_INF) { l[k] = 0; any_bad |= 2; }       // the pixel is skipped
      key[k] = l[k] > 0 ? ((u64)(unsigned int)dv[k] << 32) | (u64)(0xFFFFFFFFu - (unsigned int)(p0 + k)) : 0ull;
      if (l[k] > 0) v.s += (u64)(unsigned int)dv[k];
      v.k = key[k] > v.k ? key[k] : v.k;
    }
    const bool uni = l[0] > 0 && l[0] == l[1] && l[1] == l[2] && l[2] == l[3];
    const Heads h = run_heads(uni, l, lane);
    v = reduce_run(v, lane, lane + run_lanes(h.heads, lane));
    if (uni) {
      if (h.head) add_inscribed(keys, ssum, smax, out, l[0], v.s, v.k);
    } else {
      int cur = 0;
      u64 cs = 0, ck = 0;
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        if (l[k] != cur) {
          if (cur > 0) add_inscribed(keys, ssum, smax, out, cur, cs, ck);
          cur = l[k]; cs = 0; ck = 0;
        }
        if (l[k] > 0) cs += (u64)(unsigned int)dv[k];
        ck = key[k] > ck ? key[k] : ck;
      }
      if (cur > 0) add_inscribed(keys, ssum, smax, out, cur, cs, ck);
    }
  }
  if (any_bad) atomicOr(bad, any_bad);
  __syncthreads();

  for (int s = threadIdx.x; s < SLOTS; s += BLOCK) {
    const int label = keys[s];
    if (label == 0) continue;
    u64* o = out + (size_t)label * 3;
    if (ssum[s]) atomicAdd(o + 2, ssum[s]);
    if (smax[s] > o[0]) atomicMax(o, smax[s]);
  }
}

__global__ void inscribed_decode(u64* __restrict__ out, int nid) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nid) return;
  const u64 k = out[(size_t)i * 3];
  if (k == 0) return;                                     // absent: the row stays zero
  out[(size_t)i * 3] = k >> 32;
  out[(size_t)i * 3 + 1] = (u64)(0xFFFFFFFFu - (unsigned int)k);
}

}  // namespace

extern "C" size_t clx_label_distance_workspace(long long npix) {
  if (npix < 1 || npix >= (1ll << 32)) return 0;
  return (size_t)npix * sizeof(int);
}

extern "C" int clx_label_distance_sq(const int32_t* labels, int nd, int Z, int Y, int X, int edge, int32_t* dist_sq,
                                     void* workspace, size_t workspace_bytes, clx_stream stream) {
  CLX_REQUIRE(labels && dist_sq && workspace, "clx_label_distance_sq: null pointer");
  CLX_REQUIRE_MAP(npix, "clx_label_distance_sq", nd, Z, Y, X, 32);
  CLX_REQUIRE(edge == 0 || edge == 1, "clx_label_distance_sq: edge must be 0 or 1");
  const long long dz = Z - 1, dy = Y - 1, dx = X - 1;
  CLX_REQUIRE(dz * dz + dy * dy + dx * dx < (long long)CLX_DIST_INF,
              "clx_label_distance_sq: (Z-1)^2 + (Y-1)^2 + (X-1)^2 must be below 2^30 (a finite distance stays below CLX_DIST_INF)");
  CLX_REQUIRE(workspace_bytes >= clx_label_distance_workspace(npix),
              "clx_label_distance_sq: workspace_bytes is below clx_label_distance_workspace(Z * Y * X)");
  CLX_REQUIRE(((uintptr_t)workspace & 3) == 0, "clx_label_distance_sq: workspace must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int grid = grid_for(npix, BLOCK, PASS_MAX_GRID);
  int* ws = (int*)workspace;
  // 2-D: X -> workspace, Y -> dist_sq.  3-D: X -> dist_sq, Y -> workspace, Z -> dist_sq.
  int* first = nd == 2 ? ws : dist_sq;
  int* second = nd == 2 ? dist_sq : ws;
  distance_pass_x<<<grid, BLOCK, 0, st>>>(labels, first, X, npix, edge);
  distance_pass_axis<<<grid, BLOCK, 0, st>>>(labels, first, second, Y, (long long)X, npix, edge);
  if (nd == 3) distance_pass_axis<<<grid, BLOCK, 0, st>>>(labels, second, dist_sq, Z, (long long)X * Y, npix, edge);
  CLX_CHECK_LAUNCH("clx_label_distance_sq");
  return CLX_OK;
}

extern "C" int clx_region_inscribed(const int32_t* labels, const int32_t* dist_sq, long long npix, int nid,
                                    unsigned long long* out, int32_t* bad, clx_stream stream) {
  CLX_REQUIRE(labels && dist_sq && out && bad, "clx_region_inscribed: null pointer");
  CLX_REQUIRE(nid >= 1 && nid <= (1 << 24), "clx_region_inscribed: nid must lie in [1, 2^24]");
  CLX_REQUIRE(npix > 0 && npix < (1ll << 32), "clx_region_inscribed: npix must lie in [1, 2^32)");
  hipStream_t st = (hipStream_t)stream;
  launch_table_init<3>(out, bad, nid, st);
  const Tiling t = tiling_for(npix);
  inscribed_kernel<<<t.grid, BLOCK, 0, st>>>(labels, dist_sq, aligned16(labels), aligned16(dist_sq), npix, nid, t.ntiles,
                                             t.per_block, out, bad);
  inscribed_decode<<<(nid + 255) / 256, 256, 0, st>>>(out, nid);
  CLX_CHECK_LAUNCH("clx_region_inscribed");
  return CLX_OK;
}
