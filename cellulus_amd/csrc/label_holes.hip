// The fill stage: holes inside the objects of a label map, closed without a flood.
//   clx_label_holes   out = labels with every hole of a label L (a face-connected component of zeros that does not reach the
//                     border and whose object face neighbours all carry L) of at most max_size pixels set to L; one row per hole
//
// The zeros are labelled by the lock-free union-find of union_find.h over their horizontal RUNS, with face connectivity: the
// complement of the 8 / 26-connectivity the objects have in cc_label.hip.  The passes walk the map segment by segment
// (segments.h has the frame).  Five plain launches on the stream, no host synchronisation, and between two of them nothing but
// the kernel boundary:
//   1 runs     parent[i] = the first pixel of i's run of zeros inside its segment, -1 on object pixels.  The run starts are the
//              only possible roots: their attributes (area | border bit, smallest and largest neighbour value) are cleared here
//   2 link     a zero unions with the zero straight above it (and, outside planewise, straight before it in z) unless its left
//              lane belongs to the same pair of runs and has done so; lane 0 unions with a zero left of the segment's seam.
//              Only overlap counts: a diagonal never links
//   3 flatten  parent[i] = find(i), one find per run: a component's root is its smallest raster index.  A run that touches the
//              border sets the border bit of its root (once per root and wave, and not at all where a look says it is set)
//   4 reduce   the components WITHOUT the border bit -- the only ones that can be holes -- get their attributes at the root, one
//              set of integer atomics per run: the run's length, and the min / max over the object values of its pixels' face
//              neighbours (a segmented scan inside the wave first).  The background, the one component every run of which
//              would hit one address, makes no atomic here
//   5 fill     writes out; the pixel that is its own root counts the component and, if it is a hole, appends the row
//              (first, owner, area, kept) through the counter info[0] (one add per block and 32 segments) and adds its area to
//              info[1] (one add per block)
// A component that does not reach the border has an object face neighbour (left of its first pixel), so "all neighbours carry
// one value" is min == max and needs no bit of its own.
// Correctness across blocks and XCDs rests on the values returned by atomics and on kernel boundaries alone (union_find.h's
// rule): no block waits for another, every loop ends because a parent strictly decreases.  Integers only; ids are 32-bit raster
// indices (npix < 2^31); values of the map are compared, never an index.  The result is a function of the input; the ORDER of
// the hole rows is not (the host sorts them by `first`).
#include <limits.h>
#include "segments.h"
#include "union_find.h"

namespace {

constexpr int HOLES_MAX_GRID = 2048;            // blocks of launches 1 to 4: 8192 waves; a wave takes the segments w, w + 8192, ...
constexpr int FILL_SEGS = 8;                    // segments a wave of the last launch takes a trip
constexpr int FILL_MAX_GRID = 1024;             // blocks of the last launch: 32768 segments a trip
constexpr unsigned int BORDER = 0x80000000u;    // of area[root]; the low 31 bits are the area (npix < 2^31)

struct Shape : Segments {
  int zlinks;                                   // 3-D without planewise: z neighbours exist
};

struct Attr {                                   // planes of the workspace, read at roots only
  int* parent;
  unsigned int* area;
  int* lo;
  int* hi;
};

__global__ __launch_bounds__(BLOCK) void holes_runs(const int* __restrict__ labels, Attr a, Shape s) {
  const int lane = threadIdx.x & 63;
  FOR_EACH_SEGMENT(w, s) {
    const SegPos p = seg_pos(w, s, lane);
    const bool zero = p.valid && labels[p.i] == 0;
    const bool left_zero = __shfl_up((int)zero, 1, 64);
    const Runs runs = run_start_lane(zero && left_zero, lane);         // the runs of zeros
    const int st = runs.start;
    if (!p.valid) continue;
    a.parent[p.i] = zero ? (int)(p.i - lane + st) : -1;
    if (zero && st == lane) {
      a.area[p.i] = 0u;
      a.lo[p.i] = INT_MAX;
      a.hi[p.i] = INT_MIN;
    }
  }
}

__global__ __launch_bounds__(BLOCK) void holes_link(const int* __restrict__ labels, int* parent, Shape s) {
  const int lane = threadIdx.x & 63;
  const long long slice = (long long)s.Y * s.X;
  FOR_EACH_SEGMENT(w, s) {
    const SegPos p = seg_pos(w, s, lane);
    const bool zero = p.valid && labels[p.i] == 0;
    const bool left_in_run = __shfl_up((int)zero, 1, 64) && lane > 0;     // the left lane is a zero of this run
    if (!zero) continue;
    const int i = (int)p.i;
    if (lane == 0 && p.x > 0 && labels[p.i - 1] == 0) uf_union(parent, i, i - 1);       // the run goes on across the seam
    if (p.y > 0 && labels[p.i - s.X] == 0 && !(left_in_run && labels[p.i - s.X - 1] == 0)) uf_union(parent, i, i - s.X);
    if (s.zlinks && p.z > 0 && labels[p.i - slice] == 0 && !(left_in_run && labels[p.i - slice - 1] == 0))
      uf_union(parent, i, (int)(p.i - slice));
  }
}

__global__ __launch_bounds__(BLOCK) void holes_flatten(Attr a, Shape s) {
  const int lane = threadIdx.x & 63;
  FOR_EACH_SEGMENT(w, s) {
    const SegPos p = seg_pos(w, s, lane);
    const bool zero = p.valid && a.parent[p.i] >= 0;
    if (__ballot(zero) == 0ull) continue;
    const bool left_zero = __shfl_up((int)zero, 1, 64);
    const Runs runs = run_start_lane(zero && left_zero, lane);         // the runs of zeros
    const int st = runs.start;
    int root = (zero && st == lane) ? uf_find(a.parent, (int)p.i) : -1;
    root = __shfl(root, st, 64);
    if (zero) a.parent[p.i] = root;                      // roots keep pointing at themselves
    const bool row_on_border = p.y == 0 || p.y == s.Y - 1 || (s.zlinks && (p.z == 0 || p.z == s.Z - 1));
    const bool touches = zero && run_ends_here(runs.starts, lane) && (row_on_border || p.x == s.X - 1 || p.x - (lane - st) == 0);
    // one atomic per root and wave; a look first (it may be stale: then the atomic is merely repeated, the bit is only ever set)
    for (unsigned long long todo = __ballot(touches); todo != 0ull;) {
      const int leader = __builtin_ctzll(todo);
      const int r = __shfl(root, leader, 64);
      if (lane == leader && !(__hip_atomic_load(&a.area[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & BORDER))
        atomicOr(&a.area[r], BORDER);
      todo &= ~__ballot(touches && root == r);
    }
  }
}

__global__ __launch_bounds__(BLOCK) void holes_reduce(const int* __restrict__ labels, Attr a, Shape s) {
  const int lane = threadIdx.x & 63;
  const long long slice = (long long)s.Y * s.X;
  FOR_EACH_SEGMENT(w, s) {
    const SegPos p = seg_pos(w, s, lane);
    const int root = p.valid ? a.parent[p.i] : -1;
    const bool zero = root >= 0;
    // (the border bits are final: the launch before set them)
    const bool inner = zero && !(a.area[zero ? root : 0] & BORDER);
    if (__ballot(inner) == 0ull) continue;
    const bool left_zero = __shfl_up((int)zero, 1, 64);
    const Runs runs = run_start_lane(zero && left_zero, lane);         // the runs of zeros
    const int st = runs.start;
    int mn = INT_MAX, mx = INT_MIN;
    if (inner) {
      // an inner component does not reach the border: its pixels have all their face neighbours inside the map
      int nb[6];
      nb[0] = labels[p.i - 1];
      nb[1] = labels[p.i + 1];
      nb[2] = labels[p.i - s.X];
      nb[3] = labels[p.i + s.X];
      nb[4] = s.zlinks ? labels[p.i - slice] : 0;
      nb[5] = s.zlinks ? labels[p.i + slice] : 0;
#pragma unroll
      for (int k = 0; k < 6; ++k)
        if (nb[k] != 0) { mn = min(mn, nb[k]); mx = max(mx, nb[k]); }
    }
    // segmented inclusive scans towards higher lanes: the run's last lane holds the run's min and max
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int tn = __shfl_up(mn, d, 64), tx = __shfl_up(mx, d, 64);
      if (lane - d >= st) { mn = min(mn, tn); mx = max(mx, tx); }
    }
    if (inner && run_ends_here(runs.starts, lane)) {
      atomicAdd(&a.area[root], (unsigned int)(lane - st + 1));
      if (mn <= mx) {
        atomicMin(&a.lo[root], mn);
        atomicMax(&a.hi[root], mx);
      }
    }
  }
}

// A block takes a GROUP of 4 x FILL_SEGS consecutive segments a trip, a wave FILL_SEGS of them, and reserves the rows of all
// the group's holes with ONE add to info[0].  (One returning add per segment that held a hole was measured first: 37 000 adds to
// one word, which serves about 88 a microsecond, were 0.51 of the call's 0.59 ms on a 2048^2 map.)
__global__ __launch_bounds__(BLOCK) void holes_fill(const int* __restrict__ labels, Attr a, Shape s, long long max_size, int capacity,
                                                    int* __restrict__ out, int* __restrict__ holes, int* info) {
  constexpr int WAVES = BLOCK / 64;
  __shared__ int wave_holes[WAVES];
  __shared__ int block_base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long ngroups = (s.nwaves + WAVES * FILL_SEGS - 1) / (WAVES * FILL_SEGS);
  int ncomp = 0, filled = 0;                    // of this lane's pixels; summed over the block after the loop
  for (long long g = blockIdx.x; g < ngroups; g += gridDim.x) {         // the same trips for every thread of the block
    int first[FILL_SEGS], owner[FILL_SEGS], size[FILL_SEGS];
    bool kept[FILL_SEGS];
    unsigned long long hb[FILL_SEGS];           // the lanes that are the root of a hole, per segment
    int mine = 0;                               // the holes of this wave's segments
#pragma unroll
    for (int r = 0; r < FILL_SEGS; ++r) {
      const long long w = (g * WAVES + wave) * FILL_SEGS + r;
      bool hole_root = false;
      first[r] = owner[r] = size[r] = 0;
      kept[r] = false;
      if (w < s.nwaves) {
        const SegPos p = seg_pos(w, s, lane);
        const int v = p.valid ? labels[p.i] : 1;
        int value = v;
        if (v == 0) {
          const int root = a.parent[p.i];
          const unsigned int ab = a.area[root];
          bool hole = false;
          if (!(ab & BORDER)) {
            owner[r] = a.lo[root];
            hole = owner[r] == a.hi[root];
          }
          size[r] = (int)(ab & ~BORDER);
          kept[r] = hole && max_size >= 0 && (long long)size[r] > max_size;
          value = (hole && !kept[r]) ? owner[r] : 0;
          if (root == (int)p.i) {
            ++ncomp;
            hole_root = hole;
            first[r] = root;
            if (hole && !kept[r]) filled += size[r];
          }
        }
        if (p.valid) out[p.i] = value;
      }
      hb[r] = __ballot(hole_root);
      mine += __popcll(hb[r]);
    }
    if (lane == 0) wave_holes[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
      int total = 0;
      for (int k = 0; k < WAVES; ++k) total += wave_holes[k];
      block_base = total ? atomicAdd(&info[0], total) : 0;
    }
    __syncthreads();
    int slot = block_base;
    for (int k = 0; k < wave; ++k) slot += wave_holes[k];
#pragma unroll
    for (int r = 0; r < FILL_SEGS; ++r) {
      const int at = slot + rank_below(hb[r], lane);
      if (((hb[r] >> lane) & 1ull) && at < capacity) {
        int* row = holes + 4ll * at;
        row[0] = first[r];
        row[1] = owner[r];
        row[2] = size[r];
        row[3] = kept[r] ? 1 : 0;
      }
      slot += __popcll(hb[r]);
    }
    __syncthreads();                            // the next trip writes wave_holes and block_base again
  }
  block_add2(filled, ncomp, info + 1);
}

}  // namespace

extern "C" size_t clx_label_holes_workspace(int nd, int Z, int Y, int X) {
  long long npix;
  if (clx_map_shape(nullptr, nd, Z, Y, X, 31, &npix) != CLX_OK) return 0;
  return (size_t)npix * 4 * sizeof(int);        // parent | area and border bit | smallest | largest neighbour value
}

extern "C" int clx_label_holes(const int32_t* labels, int nd, int Z, int Y, int X, int planewise, long long max_size, int capacity,
                               int32_t* out, int32_t* holes, int32_t* info, void* workspace, size_t workspace_bytes, clx_stream stream) {
  CLX_REQUIRE(labels && out && info && workspace, "clx_label_holes: null pointer");
  CLX_REQUIRE(capacity >= 0, "clx_label_holes: capacity must be >= 0");
  CLX_REQUIRE(holes || capacity == 0, "clx_label_holes: null holes with capacity > 0");
  CLX_REQUIRE_MAP(npix, "clx_label_holes", nd, Z, Y, X, 31);
  CLX_REQUIRE(planewise == 0 || (planewise == 1 && nd == 3), "clx_label_holes: planewise must be 0, or 1 with nd == 3");
  CLX_REQUIRE(max_size >= -1, "clx_label_holes: max_size must be >= -1");
  CLX_REQUIRE(workspace_bytes >= clx_label_holes_workspace(nd, Z, Y, X),
              "clx_label_holes: workspace_bytes is below clx_label_holes_workspace(nd, Z, Y, X)");
  CLX_REQUIRE(((uintptr_t)workspace & 3) == 0, "clx_label_holes: workspace must be 4-byte aligned");
  CLX_REQUIRE(out != labels, "clx_label_holes: in-place operation is not supported");
  hipStream_t st = (hipStream_t)stream;
  const Shape s = {segments_of(Z, Y, X), nd == 3 && !planewise};
  Attr a;
  a.parent = (int*)workspace;
  a.area = (unsigned int*)(a.parent + npix);
  a.lo = (int*)(a.area + npix);
  a.hi = a.lo + npix;
  const int grid = segment_grid(s.nwaves, HOLES_MAX_GRID);
  CLX_REQUIRE(hipMemsetAsync(info, 0, 4 * sizeof(int), st) == hipSuccess, "clx_label_holes: hipMemsetAsync failed");
  holes_runs<<<grid, BLOCK, 0, st>>>(labels, a, s);
  holes_link<<<grid, BLOCK, 0, st>>>(labels, a.parent, s);
  holes_flatten<<<grid, BLOCK, 0, st>>>(a, s);
  holes_reduce<<<grid, BLOCK, 0, st>>>(labels, a, s);
  holes_fill<<<grid_for(s.nwaves, (BLOCK / 64) * FILL_SEGS, FILL_MAX_GRID), BLOCK, 0, st>>>(labels, a, s, max_size, capacity, out, holes, info);
  CLX_CHECK_LAUNCH("clx_label_holes");
  return CLX_OK;
}
