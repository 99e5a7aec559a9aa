// The frame of a fixed point reached in queued rounds of tile-local work (label_propagate.hip, grey_morph.hip's reconstruction;
// label_thin.hip takes the activity test): a monotone update whose least (greatest) fixed point is a function of the inputs alone
// is iterated without a flood queue and without a block that waits for another.
//   round      one launch.  A block takes a tile and a halo, brings the tile to rest on chip under the caller's update rule -- or
//              is cut short at the caller's sweep limit: such a tile has changed and is taken up again in the next round -- and
//              writes its interior.  The halo is what the round before left and is only read.
//   ping-pong  between rounds the state lies in two sets of planes; round r reads one set and writes the other, by the parity
//              of r: no launch reads a word it writes, and the state after round r is a function of the inputs.  r counts over
//              all calls since resume == 0 and lies in the workspace's head.
//   activity   a tile has a changed flag per round, in two arrays that alternate like the planes.  A tile is ACTIVE in round
//              r iff it or one of its 8 / 26 face-, edge- or corner-adjacent tiles changed in round r - 1 (round 0: all are).
//              An active tile always writes its interior; an inactive one clears its flag and is done.  An inactive tile would
//              not have changed: its values and its halo -- which reaches into the adjacent tiles only -- are those of the round
//              in which it last came to rest.  By induction it holds equal values in both sets of planes: active and unchanged
//              in round r - 1 it wrote what it read, inactive it had them already.  So when a round changes no tile both sets
//              are equal everywhere and hold the fixed point.
//   counters   a word per round of the call counts the tiles that changed in it; a launch that finds 0 in the word of the
//              round before returns at once, as do all after it.  The last launch of a call forms info from the counters and
//              leaves r and the last count in the head for a call with resume == 1.
// A workspace starts with the head and the counters; where the flags lie is the caller's layout.
#pragma once
#include "region_scan.h"

namespace {

constexpr int TILE_MAX_GRID = 1024;     // blocks a round; each takes the tiles blockIdx.x, blockIdx.x + gridDim.x, ...
constexpr int INIT_MAX_GRID = 4096;     // blocks of BLOCK pixels a trip (the first call's start values)
constexpr int MAX_ROUNDS = 64;          // launches a call queues at most: the counters of a call
constexpr int HEAD_WORDS = 16;          // [0] rounds so far, [1] the tiles that changed in the last of them (or 1: none yet)

struct TileGrid {
  int ntz, nty, ntx;
  long long ntiles;
};
// the tiles of a map; S2 / S3: the tile shapes (TZ, TY, TX) for nd == 2 / 3
template <typename S2, typename S3>
inline TileGrid tile_grid(int nd, int Z, int Y, int X) {
  TileGrid g;
  g.ntz = nd == 2 ? 1 : (Z + S3::TZ - 1) / S3::TZ;
  g.nty = nd == 2 ? (Y + S2::TY - 1) / S2::TY : (Y + S3::TY - 1) / S3::TY;
  g.ntx = nd == 2 ? (X + S2::TX - 1) / S2::TX : (X + S3::TX - 1) / S3::TX;
  g.ntiles = (long long)g.ntz * g.nty * g.ntx;
  return g;
}
inline size_t flag_bytes(long long ntiles) { return ((size_t)ntiles + 3) & ~(size_t)3; }

// the words and the flags of the protocol in a workspace
struct Rounds {
  int* head;
  int* counters;
  unsigned char* flag0;                 // written by the even rounds
  unsigned char* flag1;
};

// a round: its number over all calls, its parity -- an odd round reads the planes an even one writes -- and the flags it
// reads (those of the round before) and writes
struct Round {
  unsigned int r;
  bool odd;
  const unsigned char* __restrict__ fin;
  unsigned char* __restrict__ fout;
};
__device__ __forceinline__ Round round_at(unsigned int r, unsigned char* flag0, unsigned char* flag1) {
  const bool odd = r & 1u;
  return {r, odd, odd ? flag0 : flag1, odd ? flag1 : flag0};
}

// the head before the first round, by one thread of an init kernel
__device__ __forceinline__ void rounds_reset(const Rounds& w) {
  w.head[0] = 0;
  w.head[1] = 1;
}

// opens launch k of a call; false: the round before changed no tile, the fixed point is reached
__device__ __forceinline__ bool open_round(const Rounds& w, int k, Round& rd) {
  if ((k == 0 ? w.head[1] : w.counters[k - 1]) == 0) return false;
  rd = round_at((unsigned int)w.head[0] + (unsigned int)k, w.flag0, w.flag1);
  return true;
}

// Is tile t = (tz, ty, tx) of ntz x nty x ntx active in the round?  The whole block asks: the answer goes through a barrier,
// which also ends the reads of the tile before.  An inactive tile's flag is cleared.  ND == 2 reads the 9 tiles of slice tz.
template <int ND>
__device__ __forceinline__ bool tile_active(const Round& rd, int ntz, int nty, int ntx, long long t, int tz, int ty, int tx) {
  constexpr int NTILES_AROUND = ND == 2 ? 9 : 27;
  int active = rd.r == 0;
  if (rd.r != 0 && threadIdx.x < NTILES_AROUND) {
    const int i = threadIdx.x;
    const int nx = tx + i % 3 - 1, ny = ty + (i / 3) % 3 - 1, nz = tz + i / 9 - (ND == 2 ? 0 : 1);
    if ((unsigned int)nx < (unsigned int)ntx && (unsigned int)ny < (unsigned int)nty && (unsigned int)nz < (unsigned int)ntz)
      active = rd.fin[((long long)nz * nty + ny) * ntx + nx];
  }
  if (__syncthreads_or(active)) return true;
  if (threadIdx.x == 0) rd.fout[t] = 0;
  return false;
}

// closes an active tile: its flag, and launch k's counter if it changed
__device__ __forceinline__ void close_tile(const Rounds& w, const Round& rd, int k, long long t, int tile_changed) {
  if (threadIdx.x == 0) {
    rd.fout[t] = (unsigned char)tile_changed;
    if (tile_changed) atomicAdd(w.counters + k, 1);
  }
}

// the last launch of a call: info from the counters, and the head for the next call
__global__ void rounds_finish(int* __restrict__ head, const int* __restrict__ counters, int rounds, int* __restrict__ info) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int busy = 0;
  for (int k = 0; k < MAX_ROUNDS; ++k)
    if (k < rounds && counters[k] != 0) ++busy;
  info[1] = counters[rounds - 1];
  info[2] = busy;
  head[0] = (int)((unsigned int)head[0] + (unsigned int)rounds);
  head[1] = counters[rounds - 1];
}

// ---- the host side of an entry point

constexpr size_t ROUNDS_HEAD_BYTES = (size_t)(HEAD_WORDS + MAX_ROUNDS) * sizeof(int);

// head and counters from the front of the workspace -> the first word after them
inline int* rounds_carve(Rounds& w, void* workspace) {
  w.head = (int*)workspace;
  w.counters = w.head + HEAD_WORDS;
  return w.counters + MAX_ROUNDS;
}
// the two flag arrays from `at` on -> the first byte after them
inline unsigned char* rounds_carve_flags(Rounds& w, void* at, const TileGrid& g) {
  w.flag0 = (unsigned char*)at;
  w.flag1 = w.flag0 + flag_bytes(g.ntiles);
  return w.flag1 + flag_bytes(g.ntiles);
}
// a call's prologue: info and the counters start at 0; false: a memset failed
inline bool rounds_begin(const Rounds& w, int* info, hipStream_t st) {
  return hipMemsetAsync(info, 0, 3 * sizeof(int), st) == hipSuccess &&
         hipMemsetAsync(w.counters, 0, MAX_ROUNDS * sizeof(int), st) == hipSuccess;
}
inline int init_grid(long long npix) { return grid_for(npix, BLOCK, INIT_MAX_GRID); }
inline int round_grid(const TileGrid& g) { return grid_for(g.ntiles, 1, TILE_MAX_GRID); }
// a call's epilogue, after its `rounds` launches
inline void rounds_end(const Rounds& w, int rounds, int* info, hipStream_t st) {
  rounds_finish<<<1, 64, 0, st>>>(w.head, w.counters, rounds, info);
}

}  // namespace
