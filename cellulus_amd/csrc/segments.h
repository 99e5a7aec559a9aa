// The frame of a pass that walks a map segment by segment (cc_label.hip's run pipeline, label_holes.hip, skeleton_graph.hip;
// label_thin.hip's passes over its bit planes, whose words are the segments):
//   segment    64 consecutive pixels of one row; a row of X pixels has nseg = ceil(X / 64) of them and the last may be short.
//              Segment w is segment w % nseg of row w / nseg, the rows counted over all slices: row = z * Y + y
//   wave       a wave owns a segment, lane l its pixel x = 64 * (w % nseg) + l, which is VALID if x < X.  The kernels run
//              BLOCK = 256 threads, 4 waves; the waves of the grid stride over the segments: FOR_EACH_SEGMENT.  All 64 lanes
//              stay in the loop body up to the last ballot or shuffle, valid or not
//   runs       a run is a stretch of lanes of ONE segment that belong together under the caller's rule, "I continue my left
//              lane's run"; one ballot gives the lanes that start one.  A run never crosses a segment's seam: what goes on
//              beyond it is the caller's to link.  A run's length is region_scan.h's run_lanes(starts, lane) at its start lane
//   rows       a kernel that appends a row per marked lane reserves the rows of many segments with one add and gives a lane
//              the slot base + rank_below(marks, lane); block_add2 is the end of such a kernel, two counters of the block
//              added to two words once
// A lane's y and z cost a division of the row; a kernel that does not read them does not pay for it.  One that reads them
// pays before its first load: cc_merge_runs, which skips most segments of a volume after that load, asks for seg_pos<false>
// and divides the row itself once it knows that it stays.  (It must not ask for y and z as well: the compiler merges the late
// division with seg_pos's equal one and keeps it in front of the load.  profiles/segments_ab.txt has the forms timed.)
// BLOCK, u64 and run_lanes are region_scan.h's, as in tile_rounds.h and skeleton_links.h; with them come that frame's other
// names, MAX_GRID among them, so a file that includes this one names its own caps otherwise (HOLES_MAX_GRID, GRAPH_MAX_GRID).
#pragma once
#include "region_scan.h"

namespace {

struct Segments {
  int Z, Y, X, nseg;
  long long nwaves;                     // Z * Y * nseg: the segments of the map, one wave each
};
// the segments of a map that CLX_REQUIRE_MAP has checked (nd == 2: Z == 1)
inline Segments segments_of(int Z, int Y, int X) {
  Segments s;
  s.Z = Z;
  s.Y = Y;
  s.X = X;
  s.nseg = (X + 63) / 64;
  s.nwaves = (long long)Z * Y * s.nseg;
  return s;
}
// blocks of a plain launch, one segment per wave and trip
inline int segment_grid(long long nwaves, int max_grid) { return grid_for(nwaves * 64, BLOCK, max_grid); }

// a lane's pixel: raster index, row (z * Y + y), coordinates, and whether it lies in the row
struct SegPos { long long i, row; int x, y, z; bool valid; };
template <bool YZ = true>              // false: y and z stay 0, for a kernel that divides the row itself, later
__device__ __forceinline__ SegPos seg_pos(long long w, const Segments& s, int lane) {
  const long long row = w / s.nseg;
  SegPos p;
  p.row = row;
  p.x = (int)(w - row * s.nseg) * 64 + lane;
  p.valid = p.x < s.X;
  p.y = YZ ? (int)(row % s.Y) : 0;
  p.z = YZ ? (int)(row / s.Y) : 0;
  p.i = row * s.X + p.x;
  return p;
}

#define FOR_EACH_SEGMENT(w, s)                                                                          \
  for (long long w = ((long long)blockIdx.x * BLOCK + threadIdx.x) >> 6; w < (s).nwaves;                 \
       w += ((long long)gridDim.x * BLOCK) >> 6)

// the lanes that start a run, and the lane of the first pixel of this lane's run (a lane that continues nothing: itself);
// all lanes call it
struct Runs {
  u64 starts;
  int start;
};
__device__ __forceinline__ Runs run_start_lane(bool continues_left, int lane) {
  const u64 starts = __ballot(!continues_left) | 1ull;         // lane 0 has no left lane
  return {starts, 63 - __builtin_clzll(starts & ((2ull << lane) - 1ull))};
}
__device__ __forceinline__ bool run_ends_here(u64 starts, int lane) { return lane == 63 || ((starts >> (lane + 1)) & 1ull); }

// the set lanes of a ballot below this one: the lane's slot among the rows the wave appends
__device__ __forceinline__ int rank_below(u64 ballot, int lane) { return __popcll(ballot & ((1ull << lane) - 1ull)); }

// words[0] += the block's sum of a, words[1] += that of b: one atomic each, none for a sum of 0; all threads call it, once
__device__ __forceinline__ void block_add2(int a, int b, int* words) {
  constexpr int WAVES = BLOCK / 64;
  __shared__ int wave_sums[2][WAVES];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_down(a, o, 64);
    b += __shfl_down(b, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    wave_sums[0][threadIdx.x >> 6] = a;
    wave_sums[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    int total = 0;
    for (int k = 0; k < WAVES; ++k) total += wave_sums[threadIdx.x][k];
    if (total) atomicAdd(&words[threadIdx.x], total);
  }
}

}  // namespace
