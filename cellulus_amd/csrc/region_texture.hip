// Per-object grey-level co-occurrence matrices of one raw channel (the measure stage's Haralick texture columns):
//   clx_region_cooccurrence   per listed id, direction and pair of levels (a, b): the pixels p of the id at level a whose
//                             partner p + distance * offset lies in the map, carries the same id and is at level b
// The definitions (levels, directions, counts) are in include/clx.h.  A pair histogram with a same-object test is neither a
// per-pixel sum nor a selection, so this does not run in the reading frame of region_scan.h: it works object by object, on
// the bounding boxes clx_region_moments left on the device.
//
// Four kernels, none of whose grids grows with the number of objects:
//   level_kernel   one pass over labels and raw: the level of every object pixel as one byte (NO_LEVEL: background, a label
//                  outside [0, nid), a non-finite value), and the bad bits.  The float64 division is paid once per pixel here
//                  and not once per pair in the main kernel, which then reads 4 + 1 bytes per pixel and partner.
//   plan_kernel    one block: per row r of `ids` the number of slabs of the id's box, and their exclusive prefix sum
//                  item_base[nrows + 1].  A slab is a run of box rows (z, y) of about SLAB_PIXELS pixels of the box; a work
//                  item is one (row, slab).  Boxes are checked against the map here and again, by the same function, in the
//                  main kernel: a box that fails has no item.
//   init_kernel    zeroes seen, and the count rows that are not written by exactly one item
//   cooc_kernel    a block draws items from a counter, finds the item's row by bisection in item_base, zeroes its
//                  ndir x levels^2 matrices in LDS, walks the slab's pixels (a thread per pixel, consecutive along x) and adds
//                  the pairs that p owns with LDS atomics, then writes the matrices out once: plain stores where the object
//                  is one item, global atomic adds of the non-zero cells where it is shared.
// LDS: 13 x 32 x 32 x 4 bytes = 52 KiB at most (3-D, 32 levels), 1 KiB in 2-D at 8 levels; it is sized per launch, so small
// matrices leave room for as many blocks as a CU has wave slots for.
#include "clx_common.h"

namespace {

typedef unsigned long long u64;

constexpr int BLOCK = 256;
constexpr int SLAB_PIXELS = 8192;       // box pixels one work item walks (a whole number of box rows, at least one)
constexpr int MAIN_GRID = 2048;         // blocks of cooc_kernel; they draw items until none is left
constexpr int INIT_GRID = 4096;
constexpr int LEVEL_GRID = 4096;
constexpr int PLAN_BLOCK = 1024;
constexpr int MAX_LEVELS = 32;
constexpr int MAX_DISTANCE = 64;
constexpr unsigned int NO_LEVEL = 255;  // a pixel that takes part in no pair

__device__ __forceinline__ bool finite_double(double v) {
  return ((u64)__double_as_longlong(v) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}

// clx.h's level(v); the floor is clamped as a double, so the cast is always in range
__device__ __forceinline__ unsigned int level_of(double v, double lo, double hi, int levels) {
  if (hi == lo) return 0;
  const double f = floor((v - lo) / (hi - lo) * (double)levels);
  if (!(f >= 0.0)) return 0;
  return f > (double)(levels - 1) ? (unsigned int)(levels - 1) : (unsigned int)(int)f;
}

template <typename T>
__device__ __forceinline__ unsigned int pixel_level(const int* __restrict__ lab, const T* __restrict__ raw, long long p, int nid,
                                                    double lo, double hi, int levels, int& any_bad) {
  const int l = lab[p];
  if (l < 0 || l >= nid) { any_bad |= 1; return NO_LEVEL; }
  if (l == 0) return NO_LEVEL;
  const double v = (double)raw[p];
  if (!finite_double(v)) { any_bad |= 2; return NO_LEVEL; }
  return level_of(v, lo, hi, levels);
}

// four pixels per thread and trip, their bytes stored as one word (lev is 8-byte aligned)
template <typename T>
__global__ __launch_bounds__(BLOCK) void level_kernel(const int* __restrict__ lab, const T* __restrict__ raw, long long npix, int nid,
                                                      double lo, double hi, int levels, unsigned char* __restrict__ lev,
                                                      int* __restrict__ bad) {
  int any_bad = 0;
  const long long step = (long long)gridDim.x * BLOCK * 4;
  for (long long p0 = ((long long)blockIdx.x * BLOCK + threadIdx.x) * 4; p0 < npix; p0 += step) {
    if (p0 + 4 <= npix) {
      unsigned int w = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) w |= pixel_level(lab, raw, p0 + k, nid, lo, hi, levels, any_bad) << (8 * k);
      *reinterpret_cast<unsigned int*>(lev + p0) = w;
    } else {
      for (long long p = p0; p < npix; ++p) lev[p] = (unsigned char)pixel_level(lab, raw, p, nid, lo, hi, levels, any_bad);
    }
  }
  if (any_bad) atomicOr(bad, any_bad);
}

// the box of `id`, checked against the map, and how it is cut into slabs
struct Box {
  int z0, y0, x0, H, W;
  int rows_per_slab;
  long long rows;       // box rows (z, y)
  long long nslabs;
};

// false: `id` is no object id or its box does not lie inside the map (an absent id has max < min); nothing of it is visited
__device__ __forceinline__ bool load_box(const int* __restrict__ bbox, int id, int nid, int Z, int Y, int X, Box& b) {
  if (id < 1 || id >= nid) return false;
  const int* q = bbox + (size_t)id * 6;
  const int z0 = q[0], y0 = q[1], x0 = q[2], z1 = q[3], y1 = q[4], x1 = q[5];
  if (z0 < 0 || z1 < z0 || z1 >= Z || y0 < 0 || y1 < y0 || y1 >= Y || x0 < 0 || x1 < x0 || x1 >= X) return false;
  b.z0 = z0; b.y0 = y0; b.x0 = x0;
  b.H = y1 - y0 + 1;
  b.W = x1 - x0 + 1;
  b.rows_per_slab = SLAB_PIXELS / b.W > 1 ? SLAB_PIXELS / b.W : 1;
  b.rows = (long long)(z1 - z0 + 1) * b.H;
  b.nslabs = (b.rows + b.rows_per_slab - 1) / b.rows_per_slab;
  return true;
}

// item_base[r] = the slabs of the rows before r, item_base[nrows] = all of them; also zeroes bad and the item counter
__global__ __launch_bounds__(PLAN_BLOCK) void plan_kernel(const int* __restrict__ bbox, const int* __restrict__ ids, int nrows, int nid,
                                                          int Z, int Y, int X, u64* __restrict__ item_base, u64* __restrict__ counter,
                                                          int* __restrict__ bad) {
  __shared__ u64 wave_sum[PLAN_BLOCK / 64];
  __shared__ u64 running;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) { running = 0; *bad = 0; *counter = 0; }
  __syncthreads();
  for (int base = 0; base < nrows; base += PLAN_BLOCK) {
    const int r = base + tid;
    u64 n = 0;
    Box b;
    if (r < nrows && load_box(bbox, ids[r], nid, Z, Y, X, b)) n = (u64)b.nslabs;
    u64 inc = n;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const u64 t = __shfl_up(inc, d);
      if (lane >= d) inc += t;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    u64 before = running;
    for (int w = 0; w < wave; ++w) before += wave_sum[w];
    if (r < nrows) item_base[r] = before + inc - n;
    __syncthreads();
    if (tid == PLAN_BLOCK - 1) running = before + inc;
    __syncthreads();
  }
  if (tid == 0) item_base[nrows] = running;
}

__global__ __launch_bounds__(BLOCK) void init_kernel(const u64* __restrict__ item_base, int nrows, int cells, int* __restrict__ counts,
                                                     u64* __restrict__ seen) {
  for (int r = blockIdx.x; r < nrows; r += gridDim.x) {
    if (threadIdx.x == 0) seen[r] = 0;
    if (item_base[r + 1] - item_base[r] == 1) continue;     // one item: it stores the whole row
    int* row = counts + (size_t)r * cells;
    for (int i = threadIdx.x; i < cells; i += BLOCK) row[i] = 0;
  }
}

template <int ND>
__global__ __launch_bounds__(BLOCK) void cooc_kernel(const int* __restrict__ lab, const unsigned char* __restrict__ lev, int Z, int Y, int X,
                                                     int nid, const int* __restrict__ bbox, const int* __restrict__ ids, int nrows,
                                                     const u64* __restrict__ item_base, u64* __restrict__ counter, int levels,
                                                     int dist, int* __restrict__ counts, u64* __restrict__ seen) {
  constexpr int NDIR = ND == 2 ? 4 : 13;
  extern __shared__ int mat[];          // [NDIR][levels][levels]
  __shared__ u64 next_item;
  __shared__ int seen_here;
  const int cells = NDIR * levels * levels;
  const u64 total = item_base[nrows];
  for (;;) {
    if (threadIdx.x == 0) { next_item = atomicAdd(counter, 1ull); seen_here = 0; }
    for (int i = threadIdx.x; i < cells; i += BLOCK) mat[i] = 0;
    __syncthreads();
    const u64 item = next_item;
    if (item >= total) return;          // the same for the whole block
    // the row r with item_base[r] <= item < item_base[r + 1]; rows without items have item_base[r] == item_base[r + 1]
    int lo = 0, hi = nrows;
    while (hi - lo > 1) {
      const int mid = lo + (hi - lo) / 2;
      if (item_base[mid] <= item) lo = mid; else hi = mid;
    }
    const int r = lo;
    const int id = ids[r];
    const long long slab = (long long)(item - item_base[r]);
    Box b;
    const bool ok = load_box(bbox, id, nid, Z, Y, X, b) && slab < b.nslabs;      // what plan_kernel saw: always true
    if (ok) {
      const long long row0 = slab * b.rows_per_slab;
      const int nr = (int)(b.rows - row0 < b.rows_per_slab ? b.rows - row0 : b.rows_per_slab);
      const unsigned int n = (unsigned int)nr * (unsigned int)b.W;               // at most max(SLAB_PIXELS, W)
      int mine = 0;
      for (unsigned int j = threadIdx.x; j < n; j += BLOCK) {
        const unsigned int row = (unsigned int)row0 + j / (unsigned int)b.W;       // box rows are fewer than 2^31
        const int x = b.x0 + (int)(j % (unsigned int)b.W);
        const int z = b.z0 + (int)(row / (unsigned int)b.H), y = b.y0 + (int)(row % (unsigned int)b.H);
        const long long p = ((long long)z * Y + y) * X + x;
        if (lab[p] != id) continue;
        ++mine;
        const unsigned int a = lev[p];
        if (a >= (unsigned int)levels) continue;
#pragma unroll
        for (int k = 0; k < NDIR; ++k) {
          constexpr int FIRST = 14;     // (0, 0, 1) in the code (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1); ascending from there
          const int dz = (FIRST + k) / 9 - 1, dy = ((FIRST + k) / 3) % 3 - 1, dx = (FIRST + k) % 3 - 1;
          const int qz = z + dz * dist, qy = y + dy * dist, qx = x + dx * dist;
          if ((unsigned int)qx >= (unsigned int)X || (unsigned int)qy >= (unsigned int)Y) continue;
          if (ND == 3 && (unsigned int)qz >= (unsigned int)Z) continue;
          const long long q = ((long long)qz * Y + qy) * X + qx;
          if (lab[q] != id) continue;
          const unsigned int c = lev[q];
          if (c >= (unsigned int)levels) continue;
          atomicAdd(&mat[(k * levels + (int)a) * levels + (int)c], 1);
        }
      }
      if (mine) atomicAdd(&seen_here, mine);
    }
    __syncthreads();
    if (ok) {
      int* row = counts + (size_t)r * cells;
      if (b.nslabs == 1) {
        for (int i = threadIdx.x; i < cells; i += BLOCK) row[i] = mat[i];
      } else {
        for (int i = threadIdx.x; i < cells; i += BLOCK)
          if (mat[i]) atomicAdd(&row[i], mat[i]);
      }
      if (threadIdx.x == 0 && seen_here) atomicAdd(&seen[r], (u64)seen_here);
    }
    __syncthreads();                    // before mat, next_item and seen_here are reused
  }
}

// workspace: levels [npix rounded up to 8] | item_base [nrows + 1] | counter [1]
struct Layout {
  size_t item_base, counter, bytes;
};
inline Layout layout_for(long long npix, int nrows) {
  Layout L;
  L.item_base = ((size_t)npix + 7) & ~(size_t)7;
  L.counter = L.item_base + ((size_t)nrows + 1) * sizeof(u64);
  L.bytes = L.counter + sizeof(u64);
  return L;
}

inline bool finite_host(double v) { return v - v == 0.0; }

}  // namespace

extern "C" size_t clx_region_cooccurrence_workspace(long long npix, int nrows) {
  if (npix < 1 || npix >= (1ll << 31) || nrows < 0 || nrows > (1 << 24)) return 0;
  return layout_for(npix, nrows).bytes;
}

extern "C" int clx_region_cooccurrence(const int32_t* labels, const void* raw, int raw_type, int nd, int Z, int Y, int X, int nid,
                                       const int32_t* bbox, const int32_t* ids, int nrows, double lo, double hi, int levels,
                                       int distance, int32_t* counts, long long* seen, int32_t* bad, void* workspace,
                                       size_t workspace_bytes, clx_stream stream) {
  const char* who = "clx_region_cooccurrence";
  CLX_REQUIRE(labels && raw && bbox && ids && counts && seen && bad && workspace, "%s: null pointer", who);
  CLX_REQUIRE(raw_type >= CLX_RAW_F32 && raw_type <= CLX_RAW_I32, "%s: raw_type must be 0 (f32), 1 (f64) or 2 (i32)", who);
  CLX_REQUIRE(nd == 2 || nd == 3, "%s: nd must be 2 or 3", who);
  CLX_REQUIRE(nd == 3 || Z == 1, "%s: nd == 2 needs Z == 1", who);
  CLX_REQUIRE(Z > 0 && Y > 0 && X > 0, "%s: extents must be positive", who);
  CLX_REQUIRE((long long)Z * Y < (1ll << 31) && (long long)Z * Y * X < (1ll << 31), "%s: Z*Y*X must be below 2^31", who);
  CLX_REQUIRE(nid >= 1 && nid <= (1 << 24), "%s: nid must lie in [1, 2^24]", who);
  CLX_REQUIRE(nrows >= 0 && nrows < nid, "%s: nrows must lie in [0, nid)", who);
  CLX_REQUIRE(levels >= 2 && levels <= MAX_LEVELS, "%s: levels must lie in [2, 32]", who);
  CLX_REQUIRE(distance >= 1 && distance <= MAX_DISTANCE, "%s: distance must lie in [1, 64]", who);
  CLX_REQUIRE(finite_host(lo) && finite_host(hi), "%s: lo and hi must be finite", who);
  CLX_REQUIRE(hi >= lo, "%s: hi must not be below lo", who);
  const int ndir = nd == 2 ? 4 : 13;
  const int cells = ndir * levels * levels;                 // at most 13 312
  CLX_REQUIRE((unsigned long long)nrows <= (~(size_t)0) / sizeof(int32_t) / (size_t)cells, "%s: counts does not fit size_t", who);
  const long long npix = (long long)Z * Y * X;
  CLX_REQUIRE(workspace_bytes >= clx_region_cooccurrence_workspace(npix, nrows),
              "%s: workspace_bytes is below clx_region_cooccurrence_workspace(Z*Y*X, nrows)", who);
  CLX_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", who);
  hipStream_t st = (hipStream_t)stream;
  const Layout L = layout_for(npix, nrows);
  unsigned char* lev = (unsigned char*)workspace;
  u64* item_base = (u64*)((char*)workspace + L.item_base);
  u64* counter = (u64*)((char*)workspace + L.counter);
  plan_kernel<<<1, PLAN_BLOCK, 0, st>>>(bbox, ids, nrows, nid, Z, Y, X, item_base, counter, bad);
  const long long lblocks = (npix + 4 * BLOCK - 1) / (4 * BLOCK);
  const int lgrid = (int)(lblocks < LEVEL_GRID ? lblocks : LEVEL_GRID);
  if (raw_type == CLX_RAW_F32)
    level_kernel<float><<<lgrid, BLOCK, 0, st>>>(labels, (const float*)raw, npix, nid, lo, hi, levels, lev, bad);
  else if (raw_type == CLX_RAW_F64)
    level_kernel<double><<<lgrid, BLOCK, 0, st>>>(labels, (const double*)raw, npix, nid, lo, hi, levels, lev, bad);
  else
    level_kernel<int><<<lgrid, BLOCK, 0, st>>>(labels, (const int*)raw, npix, nid, lo, hi, levels, lev, bad);
  if (nrows > 0) {
    init_kernel<<<nrows < INIT_GRID ? nrows : INIT_GRID, BLOCK, 0, st>>>(item_base, nrows, cells, counts, (u64*)seen);
    // every row has at most Z*Y slabs (a slab is at least one box row): no more blocks than there can be items
    const long long most = (long long)nrows * ((long long)Z * Y);
    const int grid = (int)(most < MAIN_GRID ? most : MAIN_GRID);
    const size_t lds = (size_t)cells * sizeof(int);
    if (nd == 2)
      cooc_kernel<2><<<grid, BLOCK, lds, st>>>(labels, lev, Z, Y, X, nid, bbox, ids, nrows, item_base, counter, levels, distance, counts,
                                               (u64*)seen);
    else
      cooc_kernel<3><<<grid, BLOCK, lds, st>>>(labels, lev, Z, Y, X, nid, bbox, ids, nrows, item_base, counter, levels, distance, counts,
                                               (u64*)seen);
  }
  CLX_CHECK_LAUNCH(who);
  return CLX_OK;
}
