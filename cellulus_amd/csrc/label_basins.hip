// The split stage: a watershed of the label-aware distance map without a flood queue (declumping touching objects by shape).
//   clx_label_basins   root(p) = the summit the steepest ascent from p ends at, and the list of the summits
//   clx_basin_passes   per pair of neighbouring basins the height of the pass between them: a table of (rootA, rootB) -> max
//   clx_basin_relabel  out(p) = the id the host gave root(p)'s summit
//
// Height is a total order: key(p) = (dist_sq[p] << 32) | (0xFFFFFFFF - p), the larger distance is higher and among equal
// distances the smaller raster index.  No two pixels share a key, so there is no plateau to flood: up(p) is the neighbour (8 /
// 26 around p, inside the map, of p's label) with the largest key if that exceeds key(p), else p itself, a summit.  Keys rise
// strictly along p, up(p), up(up(p)), ..., so the chain ends at one summit whatever the order of the threads.
//   ascent     a thread per pixel, consecutive lanes consecutive in x: every tap of the stencil is a coalesced load that the
//              neighbouring rows' threads make too (L1 / L2 hits); taps outside the map read the pixel itself, whose key cannot
//              win, so all taps are loaded before any is used.  A summit takes a slot of the list with one atomic add.
//   roots      pointer jumping between two buffers, bounded per launch: a launch reads `src`, follows at most ROOT_LINKS links
//              in it and writes the ancestor reached to `dst`; no launch reads a word it writes, the kernel boundary publishes.
//              After k launches a pixel holds its ancestor min(chain, (ROOT_LINKS + 1)^k) links up, and (ROOT_LINKS + 1)^7 >
//              2^32 >= any chain, so ROOT_LAUNCHES = 7 launches always suffice (a serpentine one pixel wide has a chain as long
//              as itself).  A status word per launch lets the later ones return at once: 1 = a chain was cut short, 0 = every
//              pixel of dst holds its summit, 2 = that and the result lies in `root`.  The launches alternate workspace -> root
//              -> workspace ...; a launch that finds 0 with the result in the workspace copies it.  The count is odd, so the
//              last launch writes `root` in any case.  Everything is queued on the stream; the host never looks at a status.
//   passes     a thread per pixel again; a pixel owns its 4 / 13 forward neighbours, so every neighbouring pair is seen once.
//              Where two pixels of one label have different roots, min of their distances is a candidate for the pass of the
//              two basins: pair_table.h's table with atomicMax in place of the add.
// Integers only, and minima / maxima / a set: the same bits in every run (the order of the summit list aside, which the
// caller sorts).  Labels are only compared, never followed as an index.
#include "pair_table.h"

namespace {

constexpr unsigned int DIST_INF = (unsigned int)CLX_DIST_INF;
constexpr unsigned int NONE = 0xFFFFFFFFu;      // root / up of a pixel that belongs to no basin (CLX_BASIN_NONE)
constexpr int ROOT_LINKS = 64;                  // links a thread follows in one launch
constexpr int ROOT_LAUNCHES = 7;                // (ROOT_LINKS + 1)^7 > 2^32; odd: the last launch writes `root`
constexpr int STATUS_WORDS = 16;                // the head of the workspace: a status word per launch, zeroed by every call
constexpr int MAP_MAX_GRID = 4096;              // blocks of BLOCK pixels a trip (the root and relabel kernels)

__device__ __forceinline__ u64 height(unsigned int d2, unsigned int p) { return ((u64)d2 << 32) | (u64)(NONE - p); }

// pixel j * BLOCK + thread of tile t: the 4 pixels of a thread lie BLOCK apart, a wave reads 64 consecutive ones
__device__ __forceinline__ long long thread_pixel(long long t, int j) { return t * TILE + (long long)j * BLOCK + threadIdx.x; }

__global__ __launch_bounds__(BLOCK) void ascent_kernel(const int* __restrict__ lab, const int* __restrict__ dist,
                                                       unsigned int* __restrict__ up, unsigned int* __restrict__ summits,
                                                       unsigned int capacity, unsigned int* __restrict__ info, int zr, int Z, int Y,
                                                       int X, long long npix, long long ntiles, long long tiles_per_block) {
  const Tiles tiles = block_tiles(ntiles, tiles_per_block);
  unsigned int flags = 0;
  for (long long t = tiles.t0; t < tiles.t1; ++t) {
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      const long long p = thread_pixel(t, j);
      if (p >= npix) continue;
      const int L = lab[p];
      const unsigned int d = (unsigned int)dist[p];
      unsigned int res = NONE;
      if (L != 0 && d > DIST_INF) flags |= 2;
      if (L != 0 && d <= DIST_INF) {
        const Pixel c = pixel_at(p, npix, Y, X).p;
        u64 best = height(d, (unsigned int)p);
        res = (unsigned int)p;
#pragma unroll
        for (int dz = -1; dz <= 1; ++dz) {
          if (dz != 0 && !zr) continue;
#pragma unroll
          for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
              if (dz == 0 && dy == 0 && dx == 0) continue;
              const bool in = (unsigned int)(c.z + dz) < (unsigned int)Z && (unsigned int)(c.y + dy) < (unsigned int)Y &&
                              (unsigned int)(c.x + dx) < (unsigned int)X;
              const long long q = in ? p + ((long long)dz * Y + dy) * X + dx : p;       // outside: the pixel itself, which cannot win
              const int lq = lab[q];
              const unsigned int dq = (unsigned int)dist[q];
              const u64 k = height(dq, (unsigned int)q);
              if (lq == L && dq <= DIST_INF && k > best) { best = k; res = (unsigned int)q; }
            }
          }
        }
        if (res == (unsigned int)p) {
          const unsigned int slot = atomicAdd(info + 1, 1u);
          if (slot < capacity) summits[slot] = (unsigned int)p;
          else flags |= 4;
        }
      }
      up[p] = res;
    }
  }
  if (flags) atomicOr(info, flags);
}

// status[k - 1] is what launch k - 1 left (launch 1 has none and works); status[k] is this launch's own word
__global__ __launch_bounds__(BLOCK) void root_kernel(const unsigned int* __restrict__ src, unsigned int* __restrict__ dst,
                                                     const int* __restrict__ before, int* __restrict__ mine, int src_is_root,
                                                     long long npix) {
  const int state = before ? *before : 1;
  if (state == 2 || (state == 0 && src_is_root)) {        // the result lies in `root`: nothing to do, and the next launch shall know
    if (blockIdx.x == 0 && threadIdx.x == 0) *mine = 2;
    return;
  }
  int cut = 0;
  for (long long p = (long long)blockIdx.x * BLOCK + threadIdx.x; p < npix; p += (long long)gridDim.x * BLOCK) {
    unsigned int q = src[p];
    if (state == 1 && q != NONE) {
      bool open = true;
      for (int i = 0; i < ROOT_LINKS; ++i) {
        const unsigned int n = src[q];
        if (n == q) { open = false; break; }
        q = n;
      }
      if (open) cut = 1;
    }
    dst[p] = q;                                           // state 0: the copy of a finished map from the workspace into `root`
  }
  if (state == 0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *mine = 2;
  } else if (cut) {
    atomicOr(mine, 1);
  }
}

// a thread's candidates in the order it meets them; equal pairs in a row become one atomic
struct PassRun {
  u64 key;
  unsigned int v;
};
__device__ __forceinline__ void candidate(PassRun& r, u64* lkeys, u64* lmax, const ContactsOut& o, unsigned int a, unsigned int b,
                                          unsigned int v) {
  const u64 key = a < b ? ((u64)a << 32) | b : ((u64)b << 32) | a;
  if (key == r.key) { r.v = v > r.v ? v : r.v; return; }
  if (r.key) add_pair<PairMax>(lkeys, lmax, o, r.key, r.v);
  r.key = key;
  r.v = v;
}

__global__ __launch_bounds__(BLOCK) void passes_kernel(const int* __restrict__ lab, const int* __restrict__ dist,
                                                       const unsigned int* __restrict__ root, int zr, int Z, int Y, int X,
                                                       long long npix, long long ntiles, long long tiles_per_block, ContactsOut o) {
  __shared__ u64 lkeys[CSLOTS];
  __shared__ u64 lmax[CSLOTS];
  for (int s = threadIdx.x; s < CSLOTS; s += BLOCK) { lkeys[s] = 0; lmax[s] = 0; }
  __syncthreads();

  const Tiles tiles = block_tiles(ntiles, tiles_per_block);
  for (long long t = tiles.t0; t < tiles.t1; ++t) {
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      const long long p = thread_pixel(t, j);
      if (p >= npix) continue;
      const unsigned int r = root[p];
      if (r == NONE) continue;
      const Pixel c = pixel_at(p, npix, Y, X).p;
      // the roots of the forward neighbours, all loaded before any is used; outside the map: the pixel's own
      unsigned int rq[13];
      long long at[13];
      bool differ = false;
#pragma unroll
      for (int dz = 0; dz <= 1; ++dz) {
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            if (!(dz > 0 || dy > 0 || (dy == 0 && dx > 0))) continue;
            const int k = dz * 9 + (dy + 1) * 3 + dx + 1 - 5;                            // 0 .. 12, known when unrolled
            const bool in = (dz == 0 || zr) && (unsigned int)(c.z + dz) < (unsigned int)Z &&
                            (unsigned int)(c.y + dy) < (unsigned int)Y && (unsigned int)(c.x + dx) < (unsigned int)X;
            at[k] = in ? p + ((long long)dz * Y + dy) * X + dx : p;
            rq[k] = dz == 0 || zr ? root[at[k]] : r;
            differ |= rq[k] != r;
          }
        }
      }
      if (!differ) continue;                              // the inside of a basin: no label, no distance is read
      const int L = lab[p];
      const unsigned int d = (unsigned int)dist[p];
      PassRun run = {0ull, 0u};
#pragma unroll
      for (int k = 0; k < 13; ++k) {
        if (rq[k] == r || rq[k] == NONE) continue;
        if (lab[at[k]] != L) continue;                    // another object: no pass across labels
        const unsigned int dq = (unsigned int)dist[at[k]];
        candidate(run, lkeys, lmax, o, r, rq[k], d < dq ? d : dq);
      }
      if (run.key) add_pair<PairMax>(lkeys, lmax, o, run.key, run.v);
    }
  }
  __syncthreads();

  for (int s = threadIdx.x; s < CSLOTS; s += BLOCK)
    if (lkeys[s]) pair_to_global<PairMax>(o, lkeys[s], lmax[s], mix64(lkeys[s]));
}

__global__ void relabel_scatter(const unsigned int* __restrict__ summits, const int* __restrict__ ids, int n, long long npix,
                                int* __restrict__ id_of, int* __restrict__ bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned int s = summits[i];
  if ((long long)s < npix) id_of[s] = ids[i];
  else atomicOr(bad, 1);                                  // never followed as an index
}

__global__ __launch_bounds__(BLOCK) void relabel_kernel(const unsigned int* __restrict__ root, const int* __restrict__ id_of,
                                                        int* __restrict__ out, long long npix, int* __restrict__ bad) {
  int flags = 0;
  for (long long p = (long long)blockIdx.x * BLOCK + threadIdx.x; p < npix; p += (long long)gridDim.x * BLOCK) {
    const unsigned int r = root[p];
    int id = 0;
    if (r != NONE) {
      if ((long long)r < npix) id = id_of[r];
      if (id == 0) flags = 2;                             // a root that is no summit of the list, or outside the map
    }
    out[p] = id;
  }
  if (flags) atomicOr(bad, flags);
}

}  // namespace

extern "C" size_t clx_label_basins_workspace(long long npix) {
  if (npix < 1 || npix >= (1ll << 32)) return 0;
  return (size_t)STATUS_WORDS * sizeof(int) + (size_t)npix * sizeof(int);
}

extern "C" int clx_label_basins(const int32_t* labels, const int32_t* dist_sq, int nd, int Z, int Y, int X, int capacity,
                                int32_t* root, int32_t* summits, int32_t* info, void* workspace, size_t workspace_bytes,
                                clx_stream stream) {
  CLX_REQUIRE(labels && dist_sq && root && summits && info && workspace, "clx_label_basins: null pointer");
  CLX_REQUIRE_MAP(npix, "clx_label_basins", nd, Z, Y, X, 32);
  CLX_REQUIRE(capacity >= 1 && capacity <= (1 << 30), "clx_label_basins: capacity must lie in [1, 2^30]");
  CLX_REQUIRE(workspace_bytes >= clx_label_basins_workspace(npix),
              "clx_label_basins: workspace_bytes is below clx_label_basins_workspace(Z * Y * X)");
  CLX_REQUIRE(((uintptr_t)workspace & 3) == 0, "clx_label_basins: workspace must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  int* status = (int*)workspace;
  unsigned int* other = (unsigned int*)(status + STATUS_WORDS);
  CLX_REQUIRE(hipMemsetAsync(status, 0, STATUS_WORDS * sizeof(int), st) == hipSuccess, "clx_label_basins: hipMemsetAsync failed");
  CLX_REQUIRE(hipMemsetAsync(info, 0, 2 * sizeof(int), st) == hipSuccess, "clx_label_basins: hipMemsetAsync failed");
  const Tiling t = tiling_for(npix);
  ascent_kernel<<<t.grid, BLOCK, 0, st>>>(labels, dist_sq, other, (unsigned int*)summits, (unsigned int)capacity, (unsigned int*)info,
                                          nd == 3, Z, Y, X, npix, t.ntiles, t.per_block);
  const int grid = grid_for(npix, BLOCK, MAP_MAX_GRID);
  for (int k = 1; k <= ROOT_LAUNCHES; ++k) {              // odd launches: workspace -> root; even ones: root -> workspace
    const bool to_root = k & 1;
    root_kernel<<<grid, BLOCK, 0, st>>>(to_root ? other : (const unsigned int*)root, to_root ? (unsigned int*)root : other,
                                        k == 1 ? nullptr : status + k - 1, status + k, !to_root, npix);
  }
  CLX_CHECK_LAUNCH("clx_label_basins");
  return CLX_OK;
}

extern "C" int clx_basin_passes(const int32_t* labels, const int32_t* dist_sq, const int32_t* root, int nd, int Z, int Y, int X,
                                int capacity, unsigned long long* keys, unsigned long long* values, int32_t* info,
                                clx_stream stream) {
  CLX_REQUIRE(labels && dist_sq && root && keys && values && info, "clx_basin_passes: null pointer");
  CLX_REQUIRE_MAP(npix, "clx_basin_passes", nd, Z, Y, X, 32);
  CLX_REQUIRE(capacity >= 1024 && capacity <= (1 << 28) && (capacity & (capacity - 1)) == 0,
              "clx_basin_passes: capacity must be a power of two in [1024, 2^28]");
  hipStream_t st = (hipStream_t)stream;
  const ContactsOut o = contacts_out(keys, values, info, capacity);
  contacts_init<<<(capacity + 255) / 256, 256, 0, st>>>(o, capacity);
  const Tiling t = tiling_for(npix);
  passes_kernel<<<t.grid, BLOCK, 0, st>>>(labels, dist_sq, (const unsigned int*)root, nd == 3, Z, Y, X, npix, t.ntiles,
                                          t.per_block, o);
  CLX_CHECK_LAUNCH("clx_basin_passes");
  return CLX_OK;
}

extern "C" int clx_basin_relabel(const int32_t* root, long long npix, const int32_t* summits, const int32_t* ids, int n,
                                 int32_t* out, int32_t* bad, void* workspace, size_t workspace_bytes, clx_stream stream) {
  CLX_REQUIRE(root && out && bad && workspace && (n == 0 || (summits && ids)), "clx_basin_relabel: null pointer");
  CLX_REQUIRE(npix > 0 && npix < (1ll << 32), "clx_basin_relabel: npix must lie in [1, 2^32)");
  CLX_REQUIRE(n >= 0 && n <= (1 << 30), "clx_basin_relabel: n must lie in [0, 2^30]");
  CLX_REQUIRE(workspace_bytes >= clx_label_basins_workspace(npix),
              "clx_basin_relabel: workspace_bytes is below clx_label_basins_workspace(npix)");
  CLX_REQUIRE(((uintptr_t)workspace & 3) == 0, "clx_basin_relabel: workspace must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  int* id_of = (int*)workspace;
  CLX_REQUIRE(hipMemsetAsync(id_of, 0, (size_t)npix * sizeof(int), st) == hipSuccess, "clx_basin_relabel: hipMemsetAsync failed");
  CLX_REQUIRE(hipMemsetAsync(bad, 0, sizeof(int), st) == hipSuccess, "clx_basin_relabel: hipMemsetAsync failed");
  if (n > 0) relabel_scatter<<<(n + 255) / 256, 256, 0, st>>>((const unsigned int*)summits, ids, n, npix, id_of, bad);
  relabel_kernel<<<grid_for(npix, BLOCK, MAP_MAX_GRID), BLOCK, 0, st>>>((const unsigned int*)root, id_of, out, npix, bad);
  CLX_CHECK_LAUNCH("clx_basin_relabel");
  return CLX_OK;
}
