// "measure" stage, clx_region_topology: sums over the 2 x 2 (x 2) windows per id (Euler numbers, Crofton perimeter).
// Topology: per object the sums over all 2 x 2 (2-D) / 2 x 2 x 2 (3-D) windows of the zero-padded map from which the
// host forms the Euler numbers, the Crofton perimeter and the 3-D surface area (clx.h has the definitions).  For an id i
// and a window, bit v of the mask says whether voxel v = dz * 4 + dy * 2 + dx of the window is i; the five contributions
// T1 T2 T3 E_hi E_lo are functions of the mask alone, tabulated below from their definitions at compile time.  A window
// belongs to the pixel at its low corner; a pixel in the first column / row / slice also owns the windows that reach
// into the padding on that side (up to 2^nd for a corner pixel), as contacts_kernel assigns the backward faces.  The
// frame is contacts_kernel's: own pixels, one row down, one slice down and both down, each with its +x neighbour from
// the next lane; a wave none of whose lanes sees two different values (or one id next to the image edge) leaves the trip.
// One instantiation per window size: the 2-D one neither loads nor carries the two rows of the slice below.
#include "region_scan.h"

namespace {

constexpr int NT = 5;                   // T1 T2 T3 E_hi E_lo
constexpr int TOPO_2D = 256;            // the 16 masks of a 2 x 2 window follow the 256 of a 2 x 2 x 2 one

constexpr int popcount3(int v) { return (v & 1) + ((v >> 1) & 1) + ((v >> 2) & 1); }

// the five contributions of one mask, a signed byte each (none above 12 in absolute value: static_assert below), T1 lowest
constexpr u64 topo_entry(int nd, int m) {
  const int nv = 1 << nd;
  int v[NT] = {0, 0, 0, 0, 0};
  for (int a = 0; a < nv; ++a)                          // voxel pairs with different bits, by the coordinates they differ in
    for (int b = a + 1; b < nv; ++b)
      if (((m >> a) ^ (m >> b)) & 1) ++v[popcount3(a ^ b) - 1];
  for (int axes = 0; axes < nv; ++axes) {               // a d-cell through the vertex: d chosen axes and a side along each;
    const int d = popcount3(axes), w = 1 << (nd - d);   // its voxels are the w window voxels on those sides
    for (int side = 0; side < nv; ++side) {
      if (side & ~axes) continue;
      bool any = false, all = true;
      for (int k = 0; k < nv; ++k)
        if ((k & axes) == side) {
          if ((m >> k) & 1) any = true;
          else all = false;
        }
      if (any) v[3] += (d & 1) ? -w : w;
      if (all) v[4] += ((nd - d) & 1) ? -w : w;
    }
  }
  u64 e = 0;
  for (int q = 0; q < NT; ++q) e |= (u64)(unsigned char)(signed char)v[q] << (8 * q);
  return e;
}

struct TopoTable {
  u64 e[TOPO_2D + 16];
};
constexpr TopoTable make_topo_table() {
  TopoTable t = {};
  for (int m = 0; m < 256; ++m) t.e[m] = topo_entry(3, m);
  for (int m = 0; m < 16; ++m) t.e[TOPO_2D + m] = topo_entry(2, m);
  return t;
}
constexpr int topo_max_abs() {
  const TopoTable t = make_topo_table();
  int worst = 0;
  for (int m = 0; m < TOPO_2D + 16; ++m)
    for (int q = 0; q < NT; ++q) {
      const int v = (int)(signed char)(unsigned char)(t.e[m] >> (8 * q));
      worst = v > worst ? v : (-v > worst ? -v : worst);
    }
  return worst;
}
static_assert(topo_max_abs() <= 12, "a window adds at most 12 to a count: topology_kernel's 32-bit block sums rely on it");
__device__ const TopoTable topo_table = make_topo_table();

// what a lane has met of one id and not yet added to the block's table
struct TopoRun {
  int id;
  int v[NT];
};

__device__ void add_topology(int* keys, int (*acc)[SLOTS], long long* counts, const TopoRun& r) {
  const int s = find_slot(keys, r.id);
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    if (r.v[q] == 0) continue;
    if (s >= 0) atomicAdd(&acc[q][s], r.v[q]);
    else atomicAdd(reinterpret_cast<u64*>(counts) + (size_t)r.id * NT + q, (u64)(long long)r.v[q]);   // two's complement
  }
}

// one window, voxel v in w[v] (outside the image: 0): every distinct non-zero id gets the contributions of its mask
template <int NV>
__device__ __forceinline__ void topology_window(TopoRun& run, int* keys, int (*acc)[SLOTS], long long* counts,
                                                const u64* tab, const int (&w)[NV]) {
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int id = w[j];
    bool first = id != 0;
    int mask = 0;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (i < j) first = first && w[i] != id;
      mask |= (w[i] == id) << i;
    }
    if (!first) continue;
    const u64 e = tab[mask];
    if (e == 0) continue;                               // every voxel of the window is `id`
    if (id != run.id) {
      if (run.id) add_topology(keys, acc, counts, run);
      run.id = id;
#pragma unroll
      for (int q = 0; q < NT; ++q) run.v[q] = 0;
    }
#pragma unroll
    for (int q = 0; q < NT; ++q) run.v[q] += (int)(signed char)(unsigned char)(e >> (8 * q));
  }
}

__global__ void topology_init(long long* __restrict__ counts, int* __restrict__ bad, int nid) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *bad = 0;
  if (i >= nid) return;
  for (int q = 0; q < NT; ++q) counts[(size_t)i * NT + q] = 0;
}

struct TopoVec {
  int v[4];                             // 16-byte loads allowed for the own pixels, one row down, one slice down, both down
};

// ZWIN: 2 x 2 x 2 windows (nd == 3); else 2 x 2
template <bool ZWIN>
__global__ __launch_bounds__(BLOCK) void topology_kernel(const int* __restrict__ lab, TopoVec vec, long long npix, int Z, int Y, int X,
                                                         int nid, long long ntiles, long long tiles_per_block,
                                                         long long* __restrict__ counts, int* __restrict__ bad) {
  constexpr int NV = ZWIN ? 8 : 4;      // voxels of a window
  constexpr int NA = ZWIN ? 4 : 2;      // rows of pixels a lane holds: own, one row down, one slice down, both down
  __shared__ int keys[SLOTS];
  // A block's partial sums fit 32 bits: it owns at most tiles_per_block * TILE <= 2^22 + TILE pixels (npix < 2^32 over
  // MAX_GRID = 2^10 blocks), a pixel at most 8 windows, and a window adds at most 12 in absolute value to any of the
  // five counts of an id (12 pairs of a kind; the static_assert on the table covers E_hi and E_lo): below 2^30.
  __shared__ int acc[NT][SLOTS];
  __shared__ u64 tab[1 << NV];
  for (int s = threadIdx.x; s < SLOTS; s += BLOCK) {
    keys[s] = 0;
    for (int q = 0; q < NT; ++q) acc[q][s] = 0;
  }
  for (int s = threadIdx.x; s < (1 << NV); s += BLOCK) tab[s] = topo_table.e[(ZWIN ? 0 : TOPO_2D) + s];
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const long long plane = (long long)Y * X;
  const long long off[4] = {0, X, plane, plane + X};    // flat index of the four rows of pixels, from the own
  const long long t0 = (long long)blockIdx.x * tiles_per_block;
  const long long t1 = t0 + tiles_per_block < ntiles ? t0 + tiles_per_block : ntiles;
  bool any_bad = false;
  for (long long t = t0; t < t1; ++t) {
    const long long p0 = t * TILE + (long long)threadIdx.x * PPL;
    // v[a][0..3]: the lane's pixels (a == 0) and those one row / one slice / both down; v[a][4]: the +x neighbour of the
    // last, the next lane's first, or a load for the wave's last lane.  Every load of the trip is issued before the
    // first value is looked at: one round of memory latency per trip.
    int v[NA][PPL + 1];
    int right[NA];
    if ((t + 1) * TILE + off[NA - 1] < npix) {          // the same for the whole block: no load of the trip leaves the map
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        const int* src = lab + p0 + off[a];
        if (vec.v[a]) {
          const i32x4 q = *reinterpret_cast<const i32x4*>(src);
          v[a][0] = q[0]; v[a][1] = q[1]; v[a][2] = q[2]; v[a][3] = q[3];
        } else {
#pragma unroll
          for (int k = 0; k < PPL; ++k) v[a][k] = src[k];
        }
        right[a] = lane == 63 ? src[PPL] : 0;
      }
    } else {
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        load_labels(lab, vec.v[a] != 0, p0 + off[a], npix, v[a]);
        right[a] = lane == 63 && p0 + PPL + off[a] < npix ? lab[p0 + PPL + off[a]] : 0;
      }
    }
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const int next = __shfl_down(v[a][0], 1);
      v[a][PPL] = lane == 63 ? right[a] : next;
    }
    // smallest and largest of everything the lane holds, as unsigned: equal if it is all one value, and the largest
    // shows an id outside [0, nid).  Every value is a pixel of the map (or 0 past its end), so flagging it here is right.
    unsigned int lo = (unsigned int)v[0][0], hi = lo;
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
      for (int k = 0; k <= PPL; ++k) {
        lo = min(lo, (unsigned int)v[a][k]);
        hi = max(hi, (unsigned int)v[a][k]);
      }
    if (hi >= (unsigned int)nid) {                      // out-of-range ids become background (never an index)
      any_bad = true;
      lo = 0xffffffffu;
      hi = 0u;
#pragma unroll
      for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int k = 0; k <= PPL; ++k) {
          if ((unsigned int)v[a][k] >= (unsigned int)nid) v[a][k] = 0;
          lo = min(lo, (unsigned int)v[a][k]);
          hi = max(hi, (unsigned int)v[a][k]);
        }
    }
    // A lane that holds nothing but background adds nothing wherever it lies: its windows hold these values or the
    // outside.  A lane that holds one id adds nothing if it lies away from every image edge: the stored neighbours are
    // then the real ones, it owns no window in the padding, and each of its windows has every bit set.
    bool noisy = false;
    int x = 0, y = 0, z = 0;
    if (p0 < npix && hi != 0u) {
      // npix < 2^32: 32-bit divisions
      const unsigned int pu = (unsigned int)p0;
      const unsigned int r = pu / (unsigned int)X;
      x = (int)(pu - r * (unsigned int)X);
      z = (int)(r / (unsigned int)Y);
      y = (int)(r - (unsigned int)z * (unsigned int)Y);
      const bool interior = p0 + PPL <= npix && x > 0 && x + PPL < X && y > 0 && y + 1 < Y && (!ZWIN || (z > 0 && z + 1 < Z));
      noisy = lo != hi || !interior;
    }
    if (__ballot(noisy) == 0ull) continue;
    if (!noisy) continue;

    TopoRun run = {0, {0, 0, 0, 0, 0}};
#pragma unroll 1
    for (int k = 0; k < PPL; ++k) {
      // the lane's pixel k is element 0 of the rows, its +x neighbour element 1 (they move down below)
      if (p0 + k < npix) {
        const bool x_hi = x == X - 1, y_hi = y == Y - 1;
        // the pixel's forward cube c[dz * 4 + dy * 2 + dx]; past the last column / row / slice: outside, 0
        int c[NV];
        c[0] = v[0][0];
        c[1] = x_hi ? 0 : v[0][1];
        c[2] = y_hi ? 0 : v[1][0];
        c[3] = (y_hi || x_hi) ? 0 : v[1][1];
        // bit 0 / 1 / 2: the window's low corner lies one column / row / slice before the pixel, in the padding
        int lows = (x == 0 ? 1 : 0) | (y == 0 ? 2 : 0);
        if constexpr (ZWIN) {
          const bool z_hi = z == Z - 1;
          c[4] = z_hi ? 0 : v[2][0];
          c[5] = (z_hi || x_hi) ? 0 : v[2][1];
          c[6] = (z_hi || y_hi) ? 0 : v[3][0];
          c[7] = (z_hi || y_hi || x_hi) ? 0 : v[3][1];
          lows |= z == 0 ? 4 : 0;
        }
        // a cube of one value away from the low edges is one window with no bit or every bit set
        bool same = lows == 0;
#pragma unroll
        for (int j = 1; j < NV; ++j) same = same && c[j] == c[0];
#pragma unroll 1
        for (int s = same ? NV : 0; s < NV; ++s) {
          if (s & ~lows) continue;
          int w[NV];
#pragma unroll
          for (int j = 0; j < NV; ++j) w[j] = c[j];
          if (s & 1) {
#pragma unroll
            for (int j = 0; j < NV; j += 2) { w[j + 1] = w[j]; w[j] = 0; }
          }
          if (s & 2) {
#pragma unroll
            for (int j = 0; j < NV; j += 4) { w[j + 2] = w[j]; w[j + 3] = w[j + 1]; w[j] = w[j + 1] = 0; }
          }
          if constexpr (ZWIN) {
            if (s & 4) {
#pragma unroll
              for (int j = 0; j < 4; ++j) { w[j + 4] = w[j]; w[j] = 0; }
            }
          }
          topology_window<NV>(run, keys, acc, counts, tab, w);
        }
      }
#pragma unroll
      for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int j = 0; j < PPL; ++j) v[a][j] = v[a][j + 1];
      if (++x == X) { x = 0; if (++y == Y) { y = 0; ++z; } }
    }
    if (run.id) add_topology(keys, acc, counts, run);
  }
  if (any_bad) *bad = 1;
  __syncthreads();

  for (int s = threadIdx.x; s < SLOTS; s += BLOCK) {
    const int label = keys[s];
    if (label == 0) continue;
#pragma unroll
    for (int q = 0; q < NT; ++q)
      if (acc[q][s]) atomicAdd(reinterpret_cast<u64*>(counts) + (size_t)label * NT + q, (u64)(long long)acc[q][s]);
  }
}

}  // namespace

extern "C" int clx_region_topology(const int32_t* labels, int nd, int Z, int Y, int X, int nid, long long* counts, int32_t* bad,
                                   clx_stream stream) {
  CLX_REQUIRE(labels && counts && bad, "clx_region_topology: null pointer");
  CLX_REQUIRE_MAP(npix, "clx_region_topology", nd, Z, Y, X, 32);
  CLX_REQUIRE(nid >= 1 && nid <= (1 << 24), "clx_region_topology: nid must lie in [1, 2^24]");
  hipStream_t st = (hipStream_t)stream;
  topology_init<<<(nid + 255) / 256, 256, 0, st>>>(counts, bad, nid);
  const Tiling t = tiling_for(npix);
  const long long plane = (long long)Y * X;
  const int vec = aligned16(labels);
  const TopoVec tv = {{vec, vec && (X & 3) == 0, vec && (plane & 3) == 0, vec && ((plane + X) & 3) == 0}};
  if (nd == 3)
    topology_kernel<true><<<t.grid, BLOCK, 0, st>>>(labels, tv, npix, Z, Y, X, nid, t.ntiles, t.per_block, counts, bad);
  else
    topology_kernel<false><<<t.grid, BLOCK, 0, st>>>(labels, tv, npix, Z, Y, X, nid, t.ntiles, t.per_block, counts, bad);
  CLX_CHECK_LAUNCH("clx_region_topology");
  return CLX_OK;
}
