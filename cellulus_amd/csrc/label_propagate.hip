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
//   ping-pong  between rounds a key lies in two int32 planes; round r reads (owner, cost) and writes the workspace's pair if r
//              is even, the other way round if odd: no launch reads a word it writes, and the state after round r is a
//              function of the inputs.  r counts over all calls since resume == 0 and lies in the workspace's head.
//   activity   a tile has a changed flag per round, in two arrays that alternate like the planes.  A tile is ACTIVE in round
//              r iff it or one of its 8 / 26 neighbour tiles changed in round r - 1 (round 0: all are).  An active tile always
//              writes its interior; an inactive one clears its flag and is done.  An inactive tile would not have changed: its
//              keys and its halo are those of the round in which it last came to rest.  By induction it holds equal values in
//              both pairs of planes: active and unchanged in round r - 1 it wrote what it read, inactive it had them already.
//              So when a round changes no tile both pairs are equal everywhere and hold the fixed point.
//   counters   a word per round of the call counts the tiles that changed in it; a launch that finds 0 in the word of the
//              round before returns at once, as do all after it.  The last launch of a call forms info from the counters and
//              leaves r and the last count in the head for a call with resume == 1.
// Integers only, and minima: the same bits and the same rounds in every run.  cost <= 2^30 and a step < 2^19, so a candidate
// fits 32 bits; one above the limit can only grow and is dropped where it arises.  Ids are only compared, never an index.
#include "region_scan.h"

namespace {

constexpr unsigned int COST_INF = (unsigned int)CLX_COST_INF;
constexpr int TILE_MAX_GRID = 1024;     // blocks a round; each takes the tiles blockIdx.x, blockIdx.x + gridDim.x, ...
constexpr int INIT_MAX_GRID = 4096;     // blocks of BLOCK pixels a trip (the first call's start values)
constexpr int MAX_SWEEPS = 32;          // Jacobi sweeps a tile makes in LDS in one round
constexpr int MAX_ROUNDS = 64;          // launches a call queues at most: the counters of a call
constexpr int HEAD_WORDS = 16;          // [0] rounds so far, [1] the tiles that changed in the last of them (or 1: none yet)

template <int ND> struct TileShape;
template <> struct TileShape<2> { static constexpr int TZ = 1, TY = 16, TX = 64, ZH = 0; };
template <> struct TileShape<3> { static constexpr int TZ = 8, TY = 8, TX = 16, ZH = 1; };

struct TileGrid {
  int ntz, nty, ntx;
  long long ntiles;
};
inline TileGrid tile_grid(int nd, int Z, int Y, int X) {
  TileGrid g;
  g.ntz = nd == 2 ? 1 : (Z + TileShape<3>::TZ - 1) / TileShape<3>::TZ;
  g.nty = nd == 2 ? (Y + TileShape<2>::TY - 1) / TileShape<2>::TY : (Y + TileShape<3>::TY - 1) / TileShape<3>::TY;
  g.ntx = nd == 2 ? (X + TileShape<2>::TX - 1) / TileShape<2>::TX : (X + TileShape<3>::TX - 1) / TileShape<3>::TX;
  g.ntiles = (long long)g.ntz * g.nty * g.ntx;
  return g;
}
inline size_t flag_bytes(long long ntiles) { return ((size_t)ntiles + 3) & ~(size_t)3; }

// the planes, the flags and the words of the workspace
struct Planes {
  const int* seeds;
  const unsigned char* mask;
  const int* weight;
  int* owner;
  int* cost;
  int* wowner;
  int* wcost;
  unsigned char* flag0;                 // written by the even rounds
  unsigned char* flag1;
  int* head;
  int* counters;
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
  if (blockIdx.x == 0 && threadIdx.x == 0) { q.head[0] = 0; q.head[1] = 1; }
  if (flags) atomicOr(info, flags);
}

// launch k of a call
template <int ND>
__global__ __launch_bounds__(BLOCK) void propagate_round(Planes q, int k, int Z, int Y, int X, TileGrid g, int nid, unsigned int reg,
                                                         unsigned int limit) {
  typedef TileShape<ND> S;
  constexpr int HX = S::TX + 2, HY = S::TY + 2, HZ = S::TZ + 2 * S::ZH, HN = HX * HY * HZ;
  constexpr int NTILES_AROUND = ND == 2 ? 9 : 27;
  __shared__ u64 keys[2][HN];
  __shared__ unsigned short wl[HN];
  __shared__ unsigned char ent[HN];

  if ((k == 0 ? q.head[1] : q.counters[k - 1]) == 0) return;        // the round before changed no tile: the fixed point is reached
  const unsigned int r = (unsigned int)q.head[0] + (unsigned int)k;
  const bool odd = r & 1u;
  const int* __restrict__ sid = odd ? q.wowner : q.owner;
  const int* __restrict__ scost = odd ? q.wcost : q.cost;
  int* __restrict__ did = odd ? q.owner : q.wowner;
  int* __restrict__ dcost = odd ? q.cost : q.wcost;
  const unsigned char* __restrict__ fin = odd ? q.flag0 : q.flag1;
  unsigned char* __restrict__ fout = odd ? q.flag1 : q.flag0;

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
    int active = r == 0;
    if (r != 0 && threadIdx.x < NTILES_AROUND) {
      const int i = threadIdx.x;
      const int nx = tx + i % 3 - 1, ny = ty + (i / 3) % 3 - 1, nz = tz + i / 9 - (ND == 2 ? 0 : 1);
      if ((unsigned int)nx < (unsigned int)g.ntx && (unsigned int)ny < (unsigned int)g.nty && (unsigned int)nz < (unsigned int)g.ntz)
        active = fin[((long long)nz * g.nty + ny) * g.ntx + nx];
    }
    if (!__syncthreads_or(active)) {                      // the barrier also ends the reads of the tile before
      if (threadIdx.x == 0) fout[t] = 0;
      continue;
    }

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
    if (threadIdx.x == 0) {
      fout[t] = (unsigned char)tile_changed;
      if (tile_changed) atomicAdd(q.counters + k, 1);
    }
  }
}

// the last launch of a call: info from the counters, and the head for the next call
__global__ void propagate_finish(int* __restrict__ head, const int* __restrict__ counters, int rounds, int* __restrict__ info) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int busy = 0;
  for (int k = 0; k < MAX_ROUNDS; ++k)
    if (k < rounds && counters[k] != 0) ++busy;
  info[1] = counters[rounds - 1];
  info[2] = busy;
  head[0] = (int)((unsigned int)head[0] + (unsigned int)rounds);
  head[1] = counters[rounds - 1];
}

}  // namespace

extern "C" size_t clx_label_propagate_workspace(int nd, int Z, int Y, int X) {
  if ((nd != 2 && nd != 3) || Z <= 0 || Y <= 0 || X <= 0 || (nd == 2 && Z != 1)) return 0;
  const unsigned __int128 npix128 = (unsigned __int128)Z * (unsigned)Y * (unsigned)X;
  if (npix128 >= ((unsigned __int128)1 << 32)) return 0;
  const TileGrid g = tile_grid(nd, Z, Y, X);
  return (size_t)(HEAD_WORDS + MAX_ROUNDS) * sizeof(int) + (size_t)npix128 * 2 * sizeof(int) + 2 * flag_bytes(g.ntiles);
}

extern "C" int clx_label_propagate(const int32_t* seeds, const uint8_t* mask, const int32_t* weight, int nd, int Z, int Y, int X,
                                   int nid, int reg, int limit, int rounds, int resume, int32_t* owner, int32_t* cost, int32_t* info,
                                   void* workspace, size_t workspace_bytes, clx_stream stream) {
  CLX_REQUIRE(seeds && owner && cost && info && workspace, "clx_label_propagate: null pointer");
  CLX_REQUIRE(nd == 2 || nd == 3, "clx_label_propagate: nd must be 2 or 3");
  CLX_REQUIRE(Z > 0 && Y > 0 && X > 0, "clx_label_propagate: bad shape");
  CLX_REQUIRE(nd == 3 || Z == 1, "clx_label_propagate: nd == 2 needs Z == 1");
  CLX_REQUIRE(nid >= 1 && nid <= (1 << 24), "clx_label_propagate: nid must lie in [1, 2^24]");
  CLX_REQUIRE(reg >= 0 && reg <= 65535, "clx_label_propagate: reg must lie in [0, 65535]");
  CLX_REQUIRE(limit >= -1 && limit < CLX_COST_INF, "clx_label_propagate: limit must lie in [-1, 2^30)");
  CLX_REQUIRE(rounds >= 1 && rounds <= MAX_ROUNDS, "clx_label_propagate: rounds must lie in [1, 64]");
  CLX_REQUIRE(resume == 0 || resume == 1, "clx_label_propagate: resume must be 0 or 1");
  const unsigned __int128 npix128 = (unsigned __int128)Z * (unsigned)Y * (unsigned)X;
  CLX_REQUIRE(npix128 < ((unsigned __int128)1 << 32), "clx_label_propagate: Z * Y * X must be below 2^32");
  const long long npix = (long long)npix128;
  CLX_REQUIRE(workspace_bytes >= clx_label_propagate_workspace(nd, Z, Y, X),
              "clx_label_propagate: workspace_bytes is below clx_label_propagate_workspace(nd, Z, Y, X)");
  CLX_REQUIRE(((uintptr_t)workspace & 3) == 0, "clx_label_propagate: workspace must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const TileGrid g = tile_grid(nd, Z, Y, X);
  Planes q;
  q.seeds = seeds;
  q.mask = mask;
  q.weight = weight;
  q.owner = owner;
  q.cost = cost;
  q.head = (int*)workspace;
  q.counters = q.head + HEAD_WORDS;
  q.wowner = q.counters + MAX_ROUNDS;
  q.wcost = q.wowner + npix;
  q.flag0 = (unsigned char*)(q.wcost + npix);
  q.flag1 = q.flag0 + flag_bytes(g.ntiles);
  CLX_REQUIRE(hipMemsetAsync(info, 0, 3 * sizeof(int), st) == hipSuccess, "clx_label_propagate: hipMemsetAsync failed");
  CLX_REQUIRE(hipMemsetAsync(q.counters, 0, MAX_ROUNDS * sizeof(int), st) == hipSuccess, "clx_label_propagate: hipMemsetAsync failed");
  if (!resume) {
    const long long blocks = (npix + BLOCK - 1) / BLOCK;
    propagate_init<<<(int)(blocks < INIT_MAX_GRID ? blocks : INIT_MAX_GRID), BLOCK, 0, st>>>(q, npix, nid, info);
  }
  const int grid = (int)(g.ntiles < TILE_MAX_GRID ? g.ntiles : TILE_MAX_GRID);
  const unsigned int lim = limit < 0 ? COST_INF - 1u : (unsigned int)limit;
  for (int k = 0; k < rounds; ++k) {
    if (nd == 2) propagate_round<2><<<grid, BLOCK, 0, st>>>(q, k, Z, Y, X, g, nid, (unsigned int)reg, lim);
    else propagate_round<3><<<grid, BLOCK, 0, st>>>(q, k, Z, Y, X, g, nid, (unsigned int)reg, lim);
  }
  propagate_finish<<<1, 64, 0, st>>>(q.head, q.counters, rounds, info);
  CLX_CHECK_LAUNCH("clx_label_propagate");
  return CLX_OK;
}
