// Radial intensity distribution (the measure stage's "where inside the object does the signal sit"): every object pixel is
// sorted into a ring of its own object by its distance to the object's boundary, and in 2-D into one of eight angular
// wedges around the object's inscribed centre; pixels and quantised values are summed per (object, ring, wedge).
//   clx_region_radial   count and Σ q per cell (row[id] * rings + ring) * wedges + wedge
// Three maps stream in (labels, clx_label_distance_sq's map, one raw channel) in the reading frame of region_scan.h; what
// an id needs (its output row, clx_region_inscribed's D2 and centre) is gathered when a lane meets another id than the
// one it holds, so once per run of pixels and not per pixel.
//
// The ring is decided in integers.  Relative mode: the smallest k with d2 * rings^2 <= (k + 1)^2 * D2, which is
// ceil(rings * sqrt(d2 / D2)) - 1 without a root: both sides are squared, and squaring keeps the order of non-negative
// numbers.  d2 <= D2 <= 2^30 and rings <= 32 bound both products by 2^40.  Absolute mode: the smallest k with
// d2 <= ((k + 1) * width)^2, at most (32 * 2^15)^2 = 2^40, the last ring taking what lies deeper.  Both are one monotone
// predicate  lhs <= (k + 1)^2 * scale  that a bisection over k settles in at most 5 comparisons.
// An `inscribed` that is not clx_region_inscribed's may hold any D2: it is cut at 2^41, above every d2 * rings^2 a 32-bit
// d2 can give, which leaves the ring it defines as it is (ring 0) and the products below 2^51.
//
// Pixels are combined as in intensity_kernel, with runs of equal CELL in place of runs of equal id: inside a large object
// consecutive pixels of a row mostly share ring and wedge, so a ballot cuts the wave into runs of lanes whose 4 pixels lie in
// one cell, a segmented wave reduction sums a run, and its first lane adds it to a table in LDS keyed by cell (open
// addressing, RPROBES tries, then straight to global memory) that the block flushes once.  Integer adds only.
#include "region_sums.h"

namespace {

constexpr int RSLOTS = 1024;            // cells a block keeps in LDS (power of two): 16 B a slot, 16 KiB a block
constexpr int RPROBES = 8;
constexpr int MAX_RINGS = 32;
constexpr int MAX_WIDTH = 32768;
constexpr u64 D2_CUT = 1ull << 41;      // above (2^31 - 1) * 32^2: a larger D2 gives the same ring
constexpr int INIT_GRID = 1024;
enum { BAD_MAP = 4, BAD_ROW = 8 };      // beside BAD_LABEL and BAD_VALUE

// smallest k in [0, rings) with lhs <= (k + 1)^2 * scale; rings - 1 where none has (absolute mode's last ring)
__device__ __forceinline__ int ring_of(u64 lhs, u64 scale, int rings) {
  int lo = 0, hi = rings - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const u64 m = (u64)(mid + 1);
    if (lhs <= m * m * scale) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// floor(atan2(dy, dx) / 45 deg) with the angle in [0, 360): a ray belongs to the wedge that starts at it, (0, 0) to wedge 0
__device__ __forceinline__ int wedge_of(int dy, int dx) {
  const int ay = dy < 0 ? -dy : dy, ax = dx < 0 ? -dx : dx;
  if (dy >= 0) {
    if (dx > 0) return ay < ax ? 0 : 1;
    if (dy == 0) return dx == 0 ? 0 : 4;
    return ax < ay ? 2 : 3;
  }
  if (dx < 0) return ay < ax ? 4 : 5;
  return ax < ay ? 6 : 7;
}

// what a lane holds of the id it met last
struct IdInfo {
  int id, row;                          // row < 0: the id is not taken
  u64 limit, scale;                     // d2 must lie in [1, limit]; ring_of's scale
  int cy, cx;
  bool centre_ok;
};

// slot of `cell` in the block's table (keys hold cell + 1), claiming an empty one; -1: RPROBES occupied slots of other cells
__device__ __forceinline__ int find_cell(int* keys, int cell) {
  const int key = cell + 1;
  int s = cell & (RSLOTS - 1);          // the cells of an object and of its neighbours in id are consecutive
  for (int i = 0; i < RPROBES; ++i) {
    int k = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k == 0) k = atomicCAS(&keys[s], 0, key);
    if (k == 0 || k == key) return s;
    s = (s + 1) & (RSLOTS - 1);
  }
  return -1;
}

__device__ void add_cell(int* keys, unsigned int* scnt, u64* ssum, u64* __restrict__ count, long long* __restrict__ isum, int cell,
                         unsigned int n, long long s) {
  const int slot = find_cell(keys, cell);
  if (slot >= 0) {
    atomicAdd(&scnt[slot], n);                          // a block sees fewer than 2^32 pixels
    if (s) atomicAdd(&ssum[slot], (u64)s);              // two's complement: the signed sum, modulo 2^64
  } else {
    atomicAdd(count + cell, (u64)n);
    if (isum && s) atomicAdd(reinterpret_cast<u64*>(isum) + cell, (u64)s);
  }
}

// what a run sums of its pixels
struct Sum {
  long long s;
  __device__ __forceinline__ Sum shifted(int d) const { return {__shfl_down(s, d)}; }
  __device__ __forceinline__ void take(const Sum& o) { s += o.s; }
};

__global__ void radial_init(u64* __restrict__ count, long long* __restrict__ isum, int* __restrict__ bad, long long cells) {
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 == 0) *bad = 0;
  for (long long i = i0; i < cells; i += (long long)gridDim.x * blockDim.x) {
    count[i] = 0;
    if (isum) isum[i] = 0;
  }
}

struct RadialArgs {
  const int* lab;
  const int* dist;
  const u64* inscribed;
  const int* row;
  long long npix, ntiles, tiles_per_block, bound;
  int vec_lab, vec_dist, vec_raw;
  int X, nid, nrows, rings, width, wedges, shift;
  u64* count;
  long long* isum;
  int* bad;
};

// RAW false: counts only, `raw` is never read
template <typename T, bool RAW>
__global__ __launch_bounds__(BLOCK) void radial_kernel(RadialArgs a, const T* __restrict__ raw) {
  __shared__ int keys[RSLOTS];
  __shared__ unsigned int scnt[RSLOTS];
  __shared__ u64 ssum[RSLOTS];
  for (int s = threadIdx.x; s < RSLOTS; s += BLOCK) { keys[s] = 0; scnt[s] = 0; ssum[s] = 0; }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const Tiles tiles = block_tiles(a.ntiles, a.tiles_per_block);
  const bool relative = a.width == 0;
  const u64 rings_sq = (u64)(a.rings * a.rings), width_sq = (u64)a.width * (u64)a.width;
  IdInfo c;
  c.id = 0; c.row = -1; c.limit = 0; c.scale = 0; c.cy = 0; c.cx = 0; c.centre_ok = false;
  int any_bad = 0;
  for (long long t = tiles.t0; t < tiles.t1; ++t) {
    const long long p0 = lane_pixel(t);
    int l[PPL], dv[PPL];
    load_labels(a.lab, a.vec_lab != 0, p0, a.npix, l);
    if (clamp_labels(l, a.nid)) any_bad |= BAD_LABEL;
    load_labels(a.dist, a.vec_dist != 0, p0, a.npix, dv);     // the same 4-pixel read; past the end: 0
    Raw4<T> rv;
    if (RAW) rv = load_raw<T>(raw, a.vec_raw != 0, p0, a.npix);
    int y = 0, x = 0;
    if (a.wedges == 8) {                                      // nd == 2, npix < 2^32: a 32-bit division
      const unsigned int pu = p0 < a.npix ? (unsigned int)p0 : 0u;
      y = (int)(pu / (unsigned int)a.X);
      x = (int)(pu - (unsigned int)y * (unsigned int)a.X);
    }
    int cell[PPL];
    long long q[PPL];
    long long s = 0;
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      cell[k] = -1;
      q[k] = 0;
      const int id = l[k];
      if (id > 0) {
        if (id != c.id) {                                     // id < nid: row and inscribed are read inside their arrays
          c.id = id;
          c.row = a.row[id];
          if (c.row >= a.nrows) { any_bad |= BAD_ROW; c.row = -1; }
          if (c.row >= 0) {
            if (relative) {
              c.limit = a.inscribed[(size_t)id * 3];
              c.scale = c.limit < D2_CUT ? c.limit : D2_CUT;
            } else {
              c.limit = (u64)CLX_DIST_INF;
              c.scale = width_sq;
            }
            if (a.wedges == 8) {
              const u64 ci = a.inscribed[(size_t)id * 3 + 1];
              c.centre_ok = ci < (u64)a.npix;
              const unsigned int cu = c.centre_ok ? (unsigned int)ci : 0u;
              c.cy = (int)(cu / (unsigned int)a.X);
              c.cx = (int)(cu - (unsigned int)c.cy * (unsigned int)a.X);
            }
          }
        }
        if (c.row >= 0) {
          bool ok = true;
          if (RAW && !quantise<T>(rv.v[k], a.shift, a.bound, &q[k])) { ok = false; q[k] = 0; any_bad |= BAD_VALUE; }
          const int d2 = dv[k];
          if (d2 < 1 || (u64)d2 > c.limit || (a.wedges == 8 && !c.centre_ok)) { ok = false; q[k] = 0; any_bad |= BAD_MAP; }
          if (ok) {                                           // the pixel is skipped otherwise
            const int ring = ring_of(relative ? (u64)d2 * rings_sq : (u64)d2, c.scale, a.rings);
            const int wedge = a.wedges == 8 ? wedge_of(y - c.cy, x - c.cx) : 0;
            cell[k] = (c.row * a.rings + ring) * a.wedges + wedge;       // < nrows * rings * wedges < 2^31
          }
        }
      }
      s += q[k];
      if (++x == a.X) { x = 0; ++y; }                         // used with wedges == 8 only
    }
    const bool uni = cell[0] >= 0 && cell[0] == cell[1] && cell[1] == cell[2] && cell[2] == cell[3];
    const Heads h = run_heads(uni, cell, lane);
    const int run = run_lanes(h.heads, lane);
    if (RAW) s = reduce_run(Sum{s}, lane, lane + run).s;
    if (uni) {
      if (h.head) add_cell(keys, scnt, ssum, a.count, a.isum, cell[0], (unsigned int)(PPL * run), s);
    } else {
      int cur = -1;
      unsigned int cn = 0;
      long long cs = 0;
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        if (cell[k] != cur) {
          if (cur >= 0) add_cell(keys, scnt, ssum, a.count, a.isum, cur, cn, cs);
          cur = cell[k]; cn = 0; cs = 0;
        }
        ++cn;
        cs += q[k];
      }
      if (cur >= 0) add_cell(keys, scnt, ssum, a.count, a.isum, cur, cn, cs);
    }
  }
  if (any_bad) atomicOr(a.bad, any_bad);
  __syncthreads();

  for (int s = threadIdx.x; s < RSLOTS; s += BLOCK) {
    const int key = keys[s];
    if (key == 0) continue;
    atomicAdd(a.count + (key - 1), (u64)scnt[s]);
    if (a.isum && ssum[s]) atomicAdd(reinterpret_cast<u64*>(a.isum) + (key - 1), ssum[s]);
  }
}

}  // namespace

extern "C" int clx_region_radial(const int32_t* labels, const int32_t* dist_sq, const void* raw, int raw_type, int nd, int Z, int Y,
                                 int X, int nid, const unsigned long long* inscribed, const int32_t* row, int nrows, int rings,
                                 int width, int wedges, int shift, unsigned long long* count, long long* isum, int32_t* bad,
                                 clx_stream stream) {
  const char* who = "clx_region_radial";
  CLX_REQUIRE(labels && dist_sq && inscribed && row && count && bad, "%s: null pointer", who);
  CLX_REQUIRE(!raw || isum, "%s: null pointer: isum may be null only where raw is", who);
  CLX_REQUIRE(!raw || (raw_type >= CLX_RAW_F32 && raw_type <= CLX_RAW_I32), "%s: raw_type must be 0 (f32), 1 (f64) or 2 (i32)", who);
  CLX_REQUIRE(nd == 2 || nd == 3, "%s: nd must be 2 or 3", who);
  CLX_REQUIRE(Z > 0 && Y > 0 && X > 0, "%s: extents must be positive", who);
  CLX_REQUIRE(nd == 3 || Z == 1, "%s: nd == 2 needs Z == 1", who);
  const unsigned __int128 npix128 = (unsigned __int128)Z * (unsigned)Y * (unsigned)X;
  CLX_REQUIRE(npix128 < ((unsigned __int128)1 << 32), "%s: Z*Y*X must be below 2^32", who);
  CLX_REQUIRE(nid >= 1 && nid <= (1 << 24), "%s: nid must lie in [1, 2^24]", who);
  CLX_REQUIRE(nrows >= 0 && nrows < nid, "%s: nrows must lie in [0, nid)", who);
  CLX_REQUIRE(rings >= 1 && rings <= MAX_RINGS, "%s: rings must lie in [1, 32]", who);
  CLX_REQUIRE(width >= 0 && width <= MAX_WIDTH, "%s: width must lie in [0, 32768]", who);
  CLX_REQUIRE(wedges == 1 || wedges == 8, "%s: wedges must be 1 or 8", who);
  CLX_REQUIRE(wedges == 1 || nd == 2, "%s: wedges == 8 needs nd == 2", who);
  const long long cells = (long long)nrows * rings * wedges;          // at most 2^24 * 32 * 8
  CLX_REQUIRE(cells < (1ll << 31), "%s: nrows * rings * wedges must be below 2^31", who);
  hipStream_t st = (hipStream_t)stream;
  const long long npix = (long long)npix128;
  const Tiling t = tiling_for(npix);
  RadialArgs a;
  a.lab = labels; a.dist = dist_sq; a.inscribed = inscribed; a.row = row;
  a.npix = npix; a.ntiles = t.ntiles; a.tiles_per_block = t.per_block;
  a.bound = value_bound(npix);
  a.vec_lab = aligned16(labels); a.vec_dist = aligned16(dist_sq); a.vec_raw = aligned16(raw);
  a.X = X; a.nid = nid; a.nrows = nrows; a.rings = rings; a.width = width; a.wedges = wedges; a.shift = shift;
  a.count = count; a.isum = raw ? isum : nullptr; a.bad = bad;
  const long long iblocks = (cells + 255) / 256;
  radial_init<<<(int)(iblocks < 1 ? 1 : iblocks < INIT_GRID ? iblocks : INIT_GRID), 256, 0, st>>>(count, isum, bad, cells);
  if (!raw)
    radial_kernel<int, false><<<t.grid, BLOCK, 0, st>>>(a, nullptr);
  else
    launch_for_raw(raw_type, [&](auto v) { radial_kernel<decltype(v), true><<<t.grid, BLOCK, 0, st>>>(a, (const decltype(v)*)raw); });
  CLX_CHECK_LAUNCH(who);
  return CLX_OK;
}
