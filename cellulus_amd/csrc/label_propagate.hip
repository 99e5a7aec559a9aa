// The propagate stage: seeds grown inside a mask along the cheapest paths of an image, without a flood queue.
//   clx_label_propagate   key(p) = the smallest (cost, id) over the paths from a seed pixel to p: cost in `cost`, id in `owner`
//
// A step from p into a neighbour q (8 / 26 around p, inside the map) that is ENTERABLE -- allowed by the mask, no seed pixel,
// its weight in range -- costs reg * a + |weight[p] - weight[q]|, a = 3 / 4 / 5 for a face / edge / corner neighbour.  A pixel
// carries one 64-bit key, (cost << 32) | id, and the unsigned minimum: the smaller cost wins, among equal costs the smaller
// id.  Adding (step << 32) keeps the id and the order, and a key only grows along a path, so the minimum over all paths is the
// least fixed point of key[q] = min(key[q], key[p] + step(p, q)): the same whatever the order of the updates, zero-cost steps
// included.  Keys start at (0, id) on the seed pixels and (CLX_COST_INF, 0) elsewhere and only fall; every value a key takes
// is the cost of a real path, so the fixed point reached from above is the least one.
//   round      one launch.  A block of 256 threads takes a tile of 1024 pixels (64 x 16, or 16 x 8 x 8) and a halo of one
//              pixel: it loads the keys, the weights as 16-bit values and the enterable bits into LDS once, then makes Jacobi
//              sweeps between two LDS buffers of whole 64-bit keys -- a key is never torn -- until a sweep changes nothing, at
//              most MAX_SWEEPS of them (a tile cut short has changed and is taken up again in the next round), and writes its
//              interior.  No block waits for another: the halo is what the round before left.
//   planes     between rounds a key lies in two int32 planes; round r reads (owner, cost) and writes the workspace's pair if r
//              is even, the other way round if odd.  The rounds are queued, tiles at rest skipped and the call ended as
//              tile_rounds.h says, where the proof stands that a skipped tile would not have changed.
// Integers only, and minima: the same bits and the same rounds in every run.  cost <= 2^30 and a step < 2^19, so a candidate
// fits 32 bits; one above the limit can only grow and is dropped where it arises.  Ids are only compared, never an index.
#include "tile_rounds.h"

namespace {

constexpr unsigned int COST_INF = (unsigned int)CLX_COST_INF;
constexpr int MAX_SWEEPS = 32;          // Jacobi sweeps a tile makes in LDS in one round

template <int ND> struct TileShape;
template <> struct TileShape<2> { static constexpr int TZ = 1, TY = 16, TX = 64, ZH = 0; };
template <> struct TileShape<3> { static constexpr int TZ = 8, TY = 8, TX = 16, ZH = 1; };

// the planes, the flags and the words of the workspace
struct Planes {
  const int* seeds;
  const unsigned char* mask;
  const int* weight;
  int* owner;
  int* cost;
  int* wowner;
  int* wcost;
  Rounds w;
};

__global__ __launch_bounds__(BLOCK) void propagate_init(Planes q, long long npix, int nid, int* __restrict__ info) {
  int flags = 0;
  for (long long p = (long long)blockIdx.x * BLOCK + threadIdx.x; p < npix; p += (long long)gridDim.x * BLOCK) {
    int s = q.seeds[p];
    if ((unsigned int)s >= (unsigned int)nid) { s = 0; flags |= 1; }
    const bool allowed = q.mask ? q.mask[p] != 0 : true;
    const bool wok = q.weight ? (unsigned int)q.weight[p] <= 65535u : true;
    if (!wok && (allowed || s > 0)) flags |= 2;
    const bool source = s > 0 && wok;
    q.owner[p] = source ? s : 0;
    q.cost[p] = source ? 0 : (int)COST_INF;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) rounds_reset(q.w);
  if (flags) atomicOr(info, flags);
}

// launch k of a call
template <int ND>
__global__ __launch_bounds__(BLOCK) void propagate_round(Planes q, int k, int Z, int Y, int X, TileGrid g, int nid, unsigned int reg,
                                                         unsigned int limit) {
  typedef TileShape<ND> S;
  constexpr int HX = S::TX + 2, HY = S::TY + 2, HZ = S::TZ + 2 * S::ZH, HN = HX * HY * HZ;
  __shared__ u64 keys[2][HN];
  __shared__ unsigned short wl[HN];
  __shared__ unsigned char ent[HN];

  Round rd;
  if (!open_round(q.w, k, rd)) return;
  const int* __restrict__ sid = rd.odd ? q.wowner : q.owner;
  const int* __restrict__ scost = rd.odd ? q.wcost : q.cost;
  int* __restrict__ did = rd.odd ? q.owner : q.wowner;
  int* __restrict__ dcost = rd.odd ? q.cost : q.wcost;

  // a thread's 4 pixels of the interior, BLOCK apart: consecutive lanes consecutive in x
  int li[4], iz[4], iy[4], ix[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int j = m * BLOCK + threadIdx.x;
    ix[m] = j % S::TX;
    iy[m] = (j / S::TX) % S::TY;
    iz[m] = j / (S::TX * S::TY);
    li[m] = ((iz[m] + S::ZH) * HY + iy[m] + 1) * HX + ix[m] + 1;
  }

  for (long long t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
    const int tx = (int)(t % g.ntx), ty = (int)((t / g.ntx) % g.nty), tz = (int)(t / ((long long)g.ntx * g.nty));
    if (!tile_active<ND>(rd, g.ntz, g.nty, g.ntx, t, tz, ty, tx)) continue;

    const int z0 = tz * S::TZ - S::ZH, y0 = ty * S::TY - 1, x0 = tx * S::TX - 1;
    for (int i = threadIdx.x; i < HN; i += BLOCK) {
      const int hx = i % HX, hy = (i / HX) % HY, hz = i / (HX * HY);
      const int gz = z0 + hz, gy = y0 + hy, gx = x0 + hx;
      const bool in = (unsigned int)gz < (unsigned int)Z && (unsigned int)gy < (unsigned int)Y && (unsigned int)gx < (unsigned int)X;
      const bool inner = hx >= 1 && hx <= S::TX && hy >= 1 && hy <= S::TY && hz >= S::ZH && hz < S::TZ + S::ZH;
      u64 key = (u64)COST_INF << 32;
      unsigned int w = 0;
      bool e = false;
      if (in) {
        const long long p = ((long long)gz * Y + gy) * X + gx;
        const unsigned int c = (unsigned int)scost[p];
        key = ((u64)(c < COST_INF ? c : COST_INF) << 32) | (u64)(unsigned int)sid[p];
        const unsigned int wv = q.weight ? (unsigned int)q.weight[p] : 0u;
        const bool wok = wv <= 65535u;
        w = wok ? wv : 0u;
        if (inner) {
          const int s = q.seeds[p];
          const bool allowed = q.mask ? q.mask[p] != 0 : true;
          e = wok && allowed && !(s > 0 && s < nid);
        }
      }
      keys[0][i] = key;
      keys[1][i] = key;
      wl[i] = (unsigned short)w;
      ent[i] = e;
    }
    __syncthreads();

    bool em[4];
    unsigned int wm[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) { em[m] = ent[li[m]]; wm[m] = wl[li[m]]; }
    int cur = 0, tile_changed = 0;
    for (int s = 0; s < MAX_SWEEPS; ++s) {
      const u64* __restrict__ from = keys[cur];
      u64* __restrict__ to = keys[cur ^ 1];
      int changed = 0;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        if (!em[m]) continue;
        const int c = li[m];
        const u64 old = from[c];
        u64 best = old;
#pragma unroll
        for (int dz = -S::ZH; dz <= S::ZH; ++dz) {
#pragma unroll
          for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
              if (dz == 0 && dy == 0 && dx == 0) continue;
              const int at = c + (dz * HY + dy) * HX + dx;
              const unsigned int a = 2u + (unsigned int)((dz != 0) + (dy != 0) + (dx != 0));
              const unsigned int wq = wl[at];
              const unsigned int step = reg * a + (wm[m] > wq ? wm[m] - wq : wq - wm[m]);
              const u64 cand = from[at] + ((u64)step << 32);
              if ((unsigned int)(cand >> 32) <= limit && cand < best) best = cand;
            }
          }
        }
        to[c] = best;
        changed |= best != old;
      }
      const int any = __syncthreads_or(changed);
      cur ^= 1;
      if (!any) break;
      tile_changed = 1;
    }

#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int gz = tz * S::TZ + iz[m], gy = ty * S::TY + iy[m], gx = tx * S::TX + ix[m];
      if (gz < Z && gy < Y && gx < X) {
        const long long p = ((long long)gz * Y + gy) * X + gx;
        const u64 key = keys[cur][li[m]];
        did[p] = (int)(unsigned int)key;
        dcost[p] = (int)(unsigned int)(key >> 32);
      }
    }
    close_tile(q.w, rd, k, t, tile_changed);
  }
}

}  // namespace

extern "C" size_t clx_label_propagate_workspace(int nd, int Z, int Y, int X) {
  long long npix;
  if (clx_map_shape(nullptr, nd, Z, Y, X, 32, &npix) != CLX_OK) return 0;
  const TileGrid g = tile_grid<TileShape<2>, TileShape<3>>(nd, Z, Y, X);
  return ROUNDS_HEAD_BYTES + (size_t)npix * 2 * sizeof(int) + 2 * flag_bytes(g.ntiles);
}

extern "C" int clx_label_propagate(const int32_t* seeds, const uint8_t* mask, const int32_t* weight, int nd, int Z, int Y, int X,
                                   int nid, int reg, int limit, int rounds, int resume, int32_t* owner, int32_t* cost, int32_t* info,
                                   void* workspace, size_t workspace_bytes, clx_stream stream) {
  CLX_REQUIRE(seeds && owner && cost && info && workspace, "clx_label_propagate: null pointer");
  CLX_REQUIRE_MAP(npix, "clx_label_propagate", nd, Z, Y, X, 32);
  CLX_REQUIRE(nid >= 1 && nid <= (1 << 24), "clx_label_propagate: nid must lie in [1, 2^24]");
  CLX_REQUIRE(reg >= 0 && reg <= 65535, "clx_label_propagate: reg must lie in [0, 65535]");
  CLX_REQUIRE(limit >= -1 && limit < CLX_COST_INF, "clx_label_propagate: limit must lie in [-1, 2^30)");
  CLX_REQUIRE(rounds >= 1 && rounds <= MAX_ROUNDS, "clx_label_propagate: rounds must lie in [1, 64]");
  CLX_REQUIRE(resume == 0 || resume == 1, "clx_label_propagate: resume must be 0 or 1");
  CLX_REQUIRE(workspace_bytes >= clx_label_propagate_workspace(nd, Z, Y, X),
              "clx_label_propagate: workspace_bytes is below clx_label_propagate_workspace(nd, Z, Y, X)");
  CLX_REQUIRE(((uintptr_t)workspace & 3) == 0, "clx_label_propagate: workspace must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const TileGrid g = tile_grid<TileShape<2>, TileShape<3>>(nd, Z, Y, X);
  Planes q;
  q.seeds = seeds;
  q.mask = mask;
  q.weight = weight;
  q.owner = owner;
  q.cost = cost;
  q.wowner = rounds_carve(q.w, workspace);
  q.wcost = q.wowner + npix;
  rounds_carve_flags(q.w, q.wcost + npix, g);
  CLX_REQUIRE(rounds_begin(q.w, info, st), "clx_label_propagate: hipMemsetAsync failed");
  if (!resume) propagate_init<<<init_grid(npix), BLOCK, 0, st>>>(q, npix, nid, info);
  const int grid = round_grid(g);
  const unsigned int lim = limit < 0 ? COST_INF - 1u : (unsigned int)limit;
  for (int k = 0; k < rounds; ++k) {
    if (nd == 2) propagate_round<2><<<grid, BLOCK, 0, st>>>(q, k, Z, Y, X, g, nid, (unsigned int)reg, lim);
    else propagate_round<3><<<grid, BLOCK, 0, st>>>(q, k, Z, Y, X, g, nid, (unsigned int)reg, lim);
  }
  rounds_end(q.w, rounds, info, st);
  CLX_CHECK_LAUNCH("clx_label_propagate");
  return CLX_OK;
}
