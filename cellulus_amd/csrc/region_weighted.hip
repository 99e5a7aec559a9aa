// Intensity-weighted moments and the location of the peak per object (the measure stage's weighted centroid, weighted
// covariance, mass displacement, integrated intensity and position of the brightest pixel): every counted pixel gives q,
// clx_region_intensity's quantised value, its coordinates z, y, x and its order key, and
//   clx_region_weighted   n, Σq, the first pixel whose key is the object's largest, and the exact Σq·a and Σq·a·b per id
// Two maps stream in (labels and one raw channel) in the reading frame of region_scan.h, as in products_kernel
// (region_coloc.hip): a lane reads 4 pixels, a ballot cuts the wave into runs of lanes that carry one id, a segmented wave
// reduction sums a run, and its first lane adds it to the block's table in LDS keyed by id (find_slot; PROBES occupied slots
// of other ids: straight to global memory), which the block adds to the output once.
//
// The bound.  With L = bit_length(npix), |q| <= 2^62 >> L and every coordinate is below npix < 2^L, so every term satisfies
// |q·a·b| < 2^(62-L)·2^(2L) = 2^(62+L), and a sum of fewer than 2^L of them stays below 2^(62+2L) <= 2^126 for L <= 32: every
// sum and every partial sum fits a signed 128-bit integer (region_sums.h has the limb scheme).  Σq itself stays below 2^62.
//
// As in moments_kernel a run never crosses an image row (x + PPL <= X, and the row index joins the head test).  Inside one
// row z and y are constants of the run, so the wave reduction carries only S0 = Σq (64 bits), S1 = Σq·x and S2 = Σq·x² (128
// bits each): five words through the six shuffle steps instead of nineteen.  The run's head forms the other six sums as
// z·S0, y·S0, z²·S0, y²·S0, z·y·S0, z·S1 and y·S1.  A lane on an object's edge or on a row's end walks its four pixels and
// cuts them into pieces of one id and one row, which leave through the same door.
// The peak needs no reduction: the host passes the largest order key of every id (clx_region_intensity's), a pixel that
// carries it is rare, and each one is a 64-bit atomicMin of its flat index on word 2, in LDS and then in global memory.
// Keys are compared on the raw value, not on q: the peak stays exact where the quantisation merges values.
//
// What a piece costs is not its arithmetic but its way into the table: every pass of a wave through add_piece is a find_slot
// and two LDS round trips, whichever lanes take part.  So (1) the low limbs of all of a piece's sums are added first, each
// returning its old value, then the high limbs plus the carries: add128's scheme with the waits taken together, no branch
// between two atomics; and (2) nearly every piece leaves through ONE call: a run's head brings the run, a lane on an edge the
// first piece of its walk, and only a lane's second and later pieces go on their own.  Measured at 4096^2 (profiles/
// weighted_4096.txt), the two together took the kernel from 1.3x clx_region_products' time (a == b) to 0.72 - 0.82x.
//
// The table: SLOTS = 256 ids.  A 3-D map keeps all NW = 21 words, 42 KiB, and 1 KiB of keys: three blocks share a CU's 160 KiB
// of LDS, __launch_bounds__(BLOCK, 3), and the grid is capped at 3 x 256 = 768 blocks, one full round on the 256 CUs of an
// MI355X (hipcc reports 115 VGPRs for float, 119 for double and 113 for int, no spills, 44032 bytes of LDS, three waves a
// SIMD).  A 2-D map (Z == 1) has z = 0 in every pixel: four of the nine sums are zero, the run's head forms three products
// instead of seven, and the table keeps 13 words, 26 KiB: __launch_bounds__(BLOCK, 4) and MAX_GRID = 1024 blocks, four a CU
// (91 / 95 / 89 VGPRs, no spills, 27648 bytes of LDS; five waves a SIMD would fit).  Words are the slow index
// (acc[word][slot]): the lanes of a flush walk consecutive banks.  What the kernel lives on is bytes in flight, so a lane
// issues the loads of its next trip before it works on this one.
#include "region_sums.h"

namespace {

constexpr int NW = 21;                  // words per id: n, Σq, peak, then nine (lo, hi) pairs
constexpr int NM = 9;                   // Σq·z Σq·y Σq·x Σq·zz Σq·yy Σq·xx Σq·zy Σq·zx Σq·yx
constexpr int NM2 = 5;                  // a 2-D map (Z == 1) has z = 0: Σq·y Σq·x Σq·yy Σq·xx Σq·yx are all there is to sum
constexpr int W_PEAK = 2, W_SUMS = 3;
constexpr int GRID_3D = 768;            // three blocks a CU (the table), 256 CUs; a 2-D table lets four share one: MAX_GRID
constexpr u64 NO_PEAK = ~0ull;          // what table_init leaves in word W_PEAK

// the sums a block's table keeps: all nine in 3-D, in 2-D the five without z; `sum_of` says which of the nine the j-th is
template <bool Z3> struct Table {
  static constexpr int sums = Z3 ? NM : NM2;
  static constexpr int words = W_SUMS + 2 * sums;
  static __device__ __forceinline__ constexpr int sum_of(int j) { return Z3 ? j : (j == 0 ? 1 : j == 1 ? 2 : j == 2 ? 4 : j == 3 ? 5 : 8); }
};

// a piece of one id in one image row (z, y): n pixels, S0 = Σq, S1 = Σq·x, S2 = Σq·x²
struct Piece {
  u64 n;
  long long s0;
  i128 s1, s2;
  // for reduce_run; n does not cross the wave: it is 4 pixels a lane, the run's length gives it
  __device__ __forceinline__ Piece shifted(int d) const { return {n, __shfl_down(s0, d), shfl_down128(s1, d), shfl_down128(s2, d)}; }
  __device__ __forceinline__ void take(const Piece& o) { s0 += o.s0; s1 += o.s1; s2 += o.s2; }
};

__device__ __forceinline__ void add_pixel(Piece& v, long long q, int x) {
  const u64 xx = (u64)x * (u64)x;                       // x < 2^32
  v.n += 1;
  v.s0 += q;
  v.s1 += (i128)q * x;
  v.s2 += (i128)q * (i128)xx;
}

// The nine (five) products of a piece and their adds.  In LDS the low limbs of all sums go first, each returning its old value,
// then the high limbs plus the carries: add128's scheme with the waits for the returned values taken together instead of
// one after the other (an add of zero is an add too: no branch sits between two atomics).
template <bool Z3>
__device__ void add_piece(int* keys, u64 (*acc)[SLOTS], u64* __restrict__ out, int label, const Piece& v, int z, int y) {
  constexpr int S = Table<Z3>::sums;
  const i128 s0 = v.s0;
  const i128 yy = (i128)((u64)y * (u64)y);
  i128 m[S];
  if (Z3) {
    const i128 zz = (i128)((u64)z * (u64)z), zy = (i128)((u64)z * (u64)y);
    m[0] = s0 * z; m[1] = s0 * y; m[2] = v.s1; m[3] = s0 * zz; m[4] = s0 * yy; m[5] = v.s2; m[6] = s0 * zy;
    m[S - 2] = v.s1 * z; m[S - 1] = v.s1 * y;
  } else {
    m[0] = s0 * y; m[1] = v.s1; m[2] = s0 * yy; m[3] = v.s2; m[4] = v.s1 * y;
  }
  const int slot = find_slot(keys, label);
  if (slot >= 0) {
    atomicAdd(&acc[0][slot], v.n);
    atomicAdd(&acc[1][slot], (u64)v.s0);
    u64 old[S];
#pragma unroll
    for (int j = 0; j < S; ++j) old[j] = atomicAdd(&acc[W_SUMS + 2 * j][slot], (u64)m[j]);
#pragma unroll
    for (int j = 0; j < S; ++j) {
      const u64 lo = (u64)m[j];
      atomicAdd(&acc[W_SUMS + 2 * j + 1][slot], (u64)((unsigned __int128)m[j] >> 64) + (old[j] + lo < old[j] ? 1ull : 0ull));
    }
  } else {
    u64* o = out + (size_t)label * NW;
    atomicAdd(o + 0, v.n);
    if (v.s0) atomicAdd(o + 1, (u64)v.s0);
#pragma unroll
    for (int j = 0; j < S; ++j) add128(o + W_SUMS + 2 * Table<Z3>::sum_of(j), o + W_SUMS + 2 * Table<Z3>::sum_of(j) + 1, m[j]);
  }
}

// pixel p of `label` carries the id's largest key
__device__ void add_peak(int* keys, u64 (*acc)[SLOTS], u64* __restrict__ out, int label, u64 p) {
  const int slot = find_slot(keys, label);
  if (slot >= 0) {
    atomicMin(&acc[W_PEAK][slot], p);
  } else {
    u64* o = out + (size_t)label * NW + W_PEAK;
    if (p < *o) atomicMin(o, p);                        // the plain read only filters
  }
}

struct WeightedArgs {
  const int* lab;
  const u64* peak_keys;
  long long npix, ntiles, tiles_per_block, bound;
  int vec_lab, vec_raw;
  int Y, X, nid, shift;
  u64* out;
  int* bad;
};

// what a lane reads in one trip; a p0 at or past npix reads nothing: background and zeros
template <typename T> struct Trip {
  int l[PPL];
  Raw4<T> r;
};
template <typename T>
__device__ __forceinline__ Trip<T> load_trip(const WeightedArgs& a, const T* __restrict__ raw, long long p0) {
  Trip<T> t;
  load_labels(a.lab, a.vec_lab != 0, p0, a.npix, t.l);
  t.r = load_raw<T>(raw, a.vec_raw != 0, p0, a.npix);
  return t;
}

template <typename T, bool Z3>
__global__ __launch_bounds__(BLOCK, Z3 ? 3 : 4) void weighted_kernel(WeightedArgs a, const T* __restrict__ raw) {
  constexpr int LW = Table<Z3>::words;
  __shared__ int keys[SLOTS];
  __shared__ u64 acc[LW][SLOTS];
  for (int s = threadIdx.x; s < SLOTS; s += BLOCK) {
    keys[s] = 0;
#pragma unroll
    for (int w = 0; w < LW; ++w) acc[w][s] = w == W_PEAK ? NO_PEAK : 0ull;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const Tiles tiles = block_tiles(a.ntiles, a.tiles_per_block);
  const long long t0 = tiles.t0, t1 = tiles.t1;
  int kid = 0;                                          // the id whose largest key the lane holds
  u64 kmax = NO_PEAK;
  int any_bad = 0;
  // the loads of the next trip are issued before the work of this one: twice the bytes in flight a wave
  Trip<T> next = load_trip<T>(a, raw, t0 < t1 ? lane_pixel(t0) : a.npix);
  for (long long t = t0; t < t1; ++t) {
    const long long p0 = lane_pixel(t);
    const Trip<T> now = next;
    int l[PPL];
#pragma unroll
    for (int k = 0; k < PPL; ++k) l[k] = now.l[k];
    if (clamp_labels(l, a.nid)) any_bad |= BAD_LABEL;
    // the largest keys of this trip's ids are gathered BEFORE the next trip's loads are issued: loads return in order, so
    // a gather behind them would wait for them all
    u64 pk[PPL];
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      if (a.peak_keys && l[k] > 0 && l[k] != kid) {     // l[k] < nid: inside the array
        kid = l[k];
        kmax = a.peak_keys[kid];
      }
      pk[k] = kmax;
    }
    next = load_trip<T>(a, raw, t + 1 < t1 ? lane_pixel(t + 1) : a.npix);
    long long q[PPL];
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      q[k] = 0;
      if (l[k] > 0) {
        if (!quantise<T>(now.r.v[k], a.shift, a.bound, &q[k])) { l[k] = 0; any_bad |= BAD_VALUE; }   // the pixel is skipped
        else if (a.peak_keys && order_key(now.r.v[k]) == pk[k]) add_peak(keys, acc, a.out, l[k], (u64)(p0 + k));
      }
    }
    const PixelInRow at = pixel_at(p0, a.npix, a.Y, a.X);
    Pixel p = at.p;

    // a run never continues into the next image row: z and y are constants of a run inside one row only
    const bool uni = l[0] > 0 && l[0] == l[1] && l[1] == l[2] && l[2] == l[3] && p.x + PPL <= a.X;
    const Heads h = run_heads(uni, l, at.row, lane);
    const int run = run_lanes(h.heads, lane);
    Piece v = {0ull, 0ll, 0, 0};
    if (uni) {
#pragma unroll
      for (int k = 0; k < PPL; ++k) add_pixel(v, q[k], p.x + k);
    }
    if (h.heads != ~0ull) v = reduce_run(v, lane, lane + run);   // the same for the whole wave: some run is longer than a lane
    // One door for nearly every piece: a run's head brings the run, a lane on an edge the first piece of its walk; only the
    // second and later pieces of such a lane (two objects and a gap inside four pixels, a row's end) leave on their own.
    // Each pass through add_piece costs a wave its LDS round trips, whichever lanes take part.
    int alabel = 0, az = p.z, ay = p.y;
    Piece first = v;
    if (uni) {
      if (h.head) {
        first.n = (u64)(PPL * run);
        alabel = l[0];
      }
    } else {
      int cur = 0, cz = 0, cy = 0;
      v = {0ull, 0ll, 0, 0};
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        if (l[k] != cur || p.x == 0) {
          if (cur > 0) {
            if (alabel == 0) { first = v; alabel = cur; az = cz; ay = cy; }
            else add_piece<Z3>(keys, acc, a.out, cur, v, cz, cy);
          }
          cur = l[k]; cz = p.z; cy = p.y;
          v = {0ull, 0ll, 0, 0};
        }
        if (cur > 0) add_pixel(v, q[k], p.x);
        p = next_pixel(p, a.Y, a.X);
      }
      if (cur > 0) {
        if (alabel == 0) { first = v; alabel = cur; az = cz; ay = cy; }
        else add_piece<Z3>(keys, acc, a.out, cur, v, cz, cy);
      }
    }
    if (alabel > 0) add_piece<Z3>(keys, acc, a.out, alabel, first, az, ay);
  }
  if (any_bad) atomicOr(a.bad, any_bad);
  __syncthreads();

  for (int s = threadIdx.x; s < SLOTS; s += BLOCK) {
    const int label = keys[s];
    if (label == 0) continue;
    u64* o = a.out + (size_t)label * NW;
    if (acc[0][s]) atomicAdd(o + 0, acc[0][s]);
    if (acc[1][s]) atomicAdd(o + 1, acc[1][s]);
    if (acc[W_PEAK][s] < o[W_PEAK]) atomicMin(o + W_PEAK, acc[W_PEAK][s]);
#pragma unroll
    for (int j = 0; j < Table<Z3>::sums; ++j)
      add128(o + W_SUMS + 2 * Table<Z3>::sum_of(j), o + W_SUMS + 2 * Table<Z3>::sum_of(j) + 1,
             (i128)(((unsigned __int128)acc[W_SUMS + 2 * j + 1][s] << 64) | acc[W_SUMS + 2 * j][s]));
  }
}

template <typename T>
void launch_weighted(const WeightedArgs& a, const void* raw, bool z3, int grid, hipStream_t st) {
  if (z3)
    weighted_kernel<T, true><<<grid, BLOCK, 0, st>>>(a, (const T*)raw);
  else
    weighted_kernel<T, false><<<grid, BLOCK, 0, st>>>(a, (const T*)raw);
}

}  // namespace

extern "C" int clx_region_weighted(const int32_t* labels, const void* raw, int raw_type, int Z, int Y, int X, int nid, int shift,
                                   const unsigned long long* peak_keys, unsigned long long* out, int32_t* bad,
                                   clx_stream stream) {
  const char* who = "clx_region_weighted";
  CLX_REQUIRE(labels && raw && out && bad, "%s: null pointer", who);
  if (require_raw_channel(who, raw_type, nid) != CLX_OK) return CLX_ERR_ARG;
  CLX_REQUIRE(Z > 0 && Y > 0 && X > 0, "%s: bad shape", who);
  long long npix = 0;
  if (clx_map_bound(who, Z, Y, X, 32, &npix) != CLX_OK) return CLX_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const Tiling t = tiling_for(npix, Z > 1 ? GRID_3D : MAX_GRID);
  WeightedArgs a;
  a.lab = labels; a.peak_keys = peak_keys;
  a.npix = npix; a.ntiles = t.ntiles; a.tiles_per_block = t.per_block;
  a.bound = value_bound(npix);
  a.vec_lab = aligned16(labels); a.vec_raw = aligned16(raw);
  a.Y = Y; a.X = X; a.nid = nid; a.shift = shift;
  a.out = out; a.bad = bad;
  launch_table_init<NW, W_PEAK>(out, bad, nid, st);
  launch_for_raw(raw_type, [&](auto v) { launch_weighted<decltype(v)>(a, raw, Z > 1, t.grid, st); });
  CLX_CHECK_LAUNCH(who);
  return CLX_OK;
}
