// Exact Euclidean feature transform of a label map (the expand stage): for every pixel WHICH object is nearest and how far.
//   clx_label_nearest   dist_sq(p) = min |p - q|^2 over the object pixels q (0 < labels[q] < nid), nearest(p) = the smallest
//                       label among the object pixels at that distance; 0 / CLX_DIST_INF where there is none within the limit
//
// One 64-bit key per pixel, (d2 << 32) | id, and the unsigned minimum: the smaller distance wins, among equal distances the
// smaller id.  Adding (D << 32) to a key keeps its id and the order of two keys, so the minimum over all object pixels is the
// minimum over the rows of (dy^2 << 32) + (the row's minimum at the pixel's column), and the same one axis up: three min-plus
// passes give the definition, ties included, whatever the grid or the order of the blocks.  Between the passes a key lies in
// two int32 planes, id and d2 (0 / DIST_INF: no object pixel within the limit so far); a key whose d2 exceeds the limit can
// only grow and is dropped where it arises.
//   pass X     a scan, not a search.  A wave takes a row in segments of 64 pixels.  A first sweep, from the right, leaves
//              for every segment the first object pixel right of it; the second, from the left, carries the last object
//              pixel seen.  Inside a segment the nearest object pixel at or left (right) of a lane is the highest (lowest)
//              set bit of the ballot of object lanes below (above) it.  A pixel of an empty row costs O(1), not O(X).
//   pass Y, Z  distance_pass_axis' outward search (label_distance.hip) on keys: a thread per pixel, consecutive lanes
//              consecutive in x, both taps' planes loaded before either is used.  It stops at the first d with
//              (d^2 << 32) >= best: nothing farther along the axis can win or tie.  best starts at (limit_sq + 1) << 32.
// Cost: pass X is O(pixels); passes Y and Z are O(pixels x distance to the nearest object along the axis, at most
// sqrt(limit_sq)).  A map with one small object and no limit is the slow case: O(pixels x extent).
// d2 < 2^30 for a finite distance and d^2 < 2^30 inside a search, so a sum stays below 2^31.
#include "region_scan.h"

namespace {

constexpr unsigned int DIST_INF = (unsigned int)CLX_DIST_INF;
constexpr int PASS_MAX_GRID = 4096;     // blocks a launch: BLOCK pixels (passes Y, Z) or ROW_WAVES rows (pass X) each a trip
constexpr int SEG = 64;                 // pixels of a row a wave takes at a time
constexpr int ROW_WAVES = BLOCK / SEG;  // rows a block sweeps at a time, one per wave
constexpr int MAX_SEGS = 512;           // X <= 2^15: (X - 1)^2 < 2^30

__device__ __forceinline__ u64 make_key(unsigned int d2, int id) { return ((u64)d2 << 32) | (u64)(unsigned int)id; }

// the planes' form of a key: beyond `cap` (limit_sq + 1, or DIST_INF) there is no object
__device__ __forceinline__ void store_key(int* __restrict__ oid, int* __restrict__ od2, long long i, u64 key, unsigned int cap) {
  const bool none = (unsigned int)(key >> 32) >= cap;
  oid[i] = none ? 0 : (int)(unsigned int)key;
  od2[i] = (int)(none ? DIST_INF : (unsigned int)(key >> 32));
}

__global__ __launch_bounds__(BLOCK) void nearest_pass_x(const int* __restrict__ lab, int* __restrict__ oid, int* __restrict__ od2,
                                                        int X, long long rows, int nid, unsigned int cap, int* __restrict__ bad) {
  __shared__ int next_x[ROW_WAVES][MAX_SEGS];             // x of the first object pixel right of a segment; X: none
  const int lane = threadIdx.x & (SEG - 1), wave = threadIdx.x / SEG;
  const int nseg = (X + SEG - 1) / SEG;
  int any_bad = 0;
  // every wave of the block makes the same trips (a wave without a row reads nothing): the barriers are uniform
  for (long long r0 = (long long)blockIdx.x * ROW_WAVES; r0 < rows; r0 += (long long)gridDim.x * ROW_WAVES) {
    const long long r = r0 + wave;
    const bool live = r < rows;
    const int* row = lab + (live ? r : 0) * X;
    int carry = X;
    for (int s = nseg - 1; s >= 0; --s) {
      if (lane == 0) next_x[wave][s] = carry;
      const int x = s * SEG + lane;
      const int L = live && x < X ? row[x] : 0;
      if ((unsigned int)L >= (unsigned int)nid) any_bad = 1;
      const u64 m = __ballot(L > 0 && L < nid);
      if (m) carry = s * SEG + __ffsll((long long)m) - 1;
    }
    __syncthreads();                                      // next_x is written
    int last_x = -1, last_id = 0;                         // the last object pixel left of the segment
    for (int s = 0; s < nseg; ++s) {
      const int x = s * SEG + lane;
      int L = live && x < X ? row[x] : 0;
      if ((unsigned int)L >= (unsigned int)nid) L = 0;
      const u64 m = __ballot(L > 0);
      const u64 below = m & (~0ull >> (SEG - 1 - lane)), above = m >> lane;
      const int src_l = below ? SEG - 1 - __clzll((long long)below) : lane;
      const int src_r = above ? lane + __ffsll((long long)above) - 1 : lane;
      const int id_l = __shfl(L, src_l), id_r = __shfl(L, src_r);
      const int nx = next_x[wave][s];
      const int xl = below ? s * SEG + src_l : last_x, xr = above ? s * SEG + src_r : nx;
      const int il = below ? id_l : last_id;
      const int ir = above ? id_r : (live && nx < X ? row[nx] : 0);
      u64 best = make_key(DIST_INF, 0);
      if (xl >= 0) best = make_key((unsigned int)((x - xl) * (x - xl)), il);
      if (xr < X && ir > 0 && ir < nid) {
        const u64 k = make_key((unsigned int)((xr - x) * (xr - x)), ir);
        best = k < best ? k : best;
      }
      if (live && x < X) store_key(oid, od2, r * X + x, best, cap);
      if (m) {
        const int top = SEG - 1 - __clzll((long long)m);
        last_x = s * SEG + top;
        last_id = __shfl(L, top);
      }
    }
    __syncthreads();                                      // next_x is read: the next trip may write it
  }
  if (any_bad) atomicOr(bad, 1);
}

// the axis with stride `stride` and extent n (coordinate = (i / stride) % n) on the planes of the pass before
__global__ __launch_bounds__(BLOCK) void nearest_pass_axis(const int* __restrict__ gid, const int* __restrict__ gd2,
                                                           int* __restrict__ oid, int* __restrict__ od2, int n, long long stride,
                                                           long long npix, unsigned int cap) {
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < npix; i += (long long)gridDim.x * BLOCK) {
    const int p = (int)(((unsigned int)i / (unsigned int)stride) % (unsigned int)n);        // npix < 2^32
    u64 best = make_key((unsigned int)gd2[i], gid[i]);
    const u64 start = make_key(cap, 0);
    best = best < start ? best : start;
    for (int d = 1; d < n; ++d) {
      const unsigned int dd = (unsigned int)(d * d);
      if (make_key(dd, 0) >= best) break;                 // an object pixel d away ties at best: the smaller id may be there
      const int lo = p - d, hi = p + d;
      if (lo < 0 && hi >= n) break;
      // both taps are loaded before either is used: four independent loads a step
      const long long jl = lo >= 0 ? i - (long long)d * stride : i, jh = hi < n ? i + (long long)d * stride : i;
      const int il = gid[jl], ih = gid[jh];
      const unsigned int dl = (unsigned int)gd2[jl], dh = (unsigned int)gd2[jh];
      const u64 kl = make_key(dd + dl, il), kh = make_key(dd + dh, ih);
      if (lo >= 0 && kl < best) best = kl;
      if (hi < n && kh < best) best = kh;
    }
    store_key(oid, od2, i, best, cap);
  }
}

}  // namespace

extern "C" size_t clx_label_nearest_workspace(long long npix) {
  if (npix < 1 || npix >= (1ll << 32)) return 0;
  return (size_t)npix * 2 * sizeof(int);
}

extern "C" int clx_label_nearest(const int32_t* labels, int nd, int Z, int Y, int X, int nid, int limit_sq, int32_t* nearest,
                                 int32_t* dist_sq, int32_t* bad, void* workspace, size_t workspace_bytes, clx_stream stream) {
  CLX_REQUIRE(labels && nearest && dist_sq && bad && workspace, "clx_label_nearest: null pointer");
  CLX_REQUIRE_MAP(npix, "clx_label_nearest", nd, Z, Y, X, 32);
  CLX_REQUIRE(nid >= 1 && nid <= (1 << 24), "clx_label_nearest: nid must lie in [1, 2^24]");
  CLX_REQUIRE(limit_sq >= -1 && limit_sq < CLX_DIST_INF, "clx_label_nearest: limit_sq must lie in [-1, 2^30)");
  const long long dz = Z - 1, dy = Y - 1, dx = X - 1;
  CLX_REQUIRE(dz * dz + dy * dy + dx * dx < (long long)CLX_DIST_INF,
              "clx_label_nearest: (Z-1)^2 + (Y-1)^2 + (X-1)^2 must be below 2^30 (a finite distance stays below CLX_DIST_INF)");
  CLX_REQUIRE(workspace_bytes >= clx_label_nearest_workspace(npix),
              "clx_label_nearest: workspace_bytes is below clx_label_nearest_workspace(Z * Y * X)");
  CLX_REQUIRE(((uintptr_t)workspace & 3) == 0, "clx_label_nearest: workspace must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  CLX_REQUIRE(hipMemsetAsync(bad, 0, sizeof(int), st) == hipSuccess, "clx_label_nearest: hipMemsetAsync failed");
  const unsigned int cap = limit_sq < 0 ? DIST_INF : (unsigned int)limit_sq + 1u;
  int* wid = (int*)workspace;
  int* wd2 = wid + npix;
  // 2-D: X -> workspace, Y -> outputs.  3-D: X -> outputs, Y -> workspace, Z -> outputs.
  int* aid = nd == 2 ? wid : nearest;
  int* ad2 = nd == 2 ? wd2 : dist_sq;
  int* bid = nd == 2 ? nearest : wid;
  int* bd2 = nd == 2 ? dist_sq : wd2;
  const long long rows = (long long)Z * Y;
  const int grid = grid_for(npix, BLOCK, PASS_MAX_GRID);
  nearest_pass_x<<<grid_for(rows, ROW_WAVES, PASS_MAX_GRID), BLOCK, 0, st>>>(labels, aid, ad2, X, rows, nid, cap, bad);
  nearest_pass_axis<<<grid, BLOCK, 0, st>>>(aid, ad2, bid, bd2, Y, (long long)X, npix, cap);
  if (nd == 3) nearest_pass_axis<<<grid, BLOCK, 0, st>>>(bid, bd2, nearest, dist_sq, Z, (long long)X * Y, npix, cap);
  CLX_CHECK_LAUNCH("clx_label_nearest");
  return CLX_OK;
}
