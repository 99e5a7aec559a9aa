// Second moments of two raw channels per object (the measure stage's intensity standard deviation and channel
// colocalization): every object pixel gives q_a and q_b, clx_region_intensity's quantised values of the two channels, and
//   clx_region_products   n, Σa, Σb and the exact Σaa, Σbb, Σab per id, each also over the pixels above per-id thresholds
// Three maps stream in (labels and the two channels) in the reading frame of region_scan.h, as in intensity_kernel: a lane
// reads 4 pixels, a ballot cuts the wave into runs of lanes that carry one id, a segmented wave reduction sums a run, and
// its first lane adds it to the block's table in LDS keyed by id (find_slot; PROBES occupied slots of other ids: straight
// to global memory), which the block adds to the output once.
//
// A product of two q is below 2^(124 - 2 L) with L = bit_length(npix) (|q| <= 2^62 >> L), a sum of at most npix < 2^L of
// them below 2^(124 - L): it fits a signed 128-bit integer, and so does every partial sum.  Products and partial sums
// are __int128 in registers.  In LDS and in global memory a 128-bit sum is two 64-bit words (lo, hi), two's complement,
// and an add to it is two 64-bit atomic adds: the low limbs first, whose returned old value says whether they wrapped,
// then the high limbs plus that carry.  Between the two a reader could see a sum whose carry is still on its way, but
// nothing reads a word before every add to it is done (the block's barrier, the end of the kernel), and adds modulo 2^128
// commute: the same map gives the same bits in every run.
//
// The table: SLOTS = 256 ids (find_slot) of the words a run carries, and 1 KiB of keys.  With thresholds that is all NW = 20
// words, 40 KiB: three blocks share a CU's 160 KiB of LDS, which is also what the 168 VGPRs of that variant allow.  Without
// thresholds the conditioned words are copies, so the table keeps 9 words (n, Σa, Σb and three pairs), 18 KiB, and the
// copies are made when a row leaves for global memory; four blocks share a CU (98 - 106 VGPRs).  512 slots would leave one
// block a CU with thresholds; 128 would double the ids that a block of a crowded map sends to global memory one atomic at
// a time.  Words are the slow index (acc[word][slot]): the lanes of a flush walk consecutive banks.
// What the kernel lives on is bytes in flight, so a lane issues the loads of its next trip before it works on this one.
#include "region_sums.h"

namespace {

constexpr int NW = 20;                  // words per id in the output and in the table
constexpr int NS = 8;                   // 64-bit words: n Σa Σb n_both Σa|above_a Σb|above_b Σa|both Σb|both
constexpr int NP = 6;                   // 128-bit sums, (lo, hi) from word NS on: Σaa Σbb Σab, then the three over `both`
// With thresholds a block's registers and its 41 KiB table let 3 blocks share a CU: on the 256 CUs of an MI355X 768 blocks run
// at once, and MAX_GRID = 1024 of them would be one full round and a second one a third full.  (Without thresholds 4 fit.)
constexpr int THR_GRID = 768;

// what a lane has summed of one id.  THR false (no thresholds): every pixel is above both, the conditioned words equal
// the unconditioned ones and are filled in by complete() when the sums leave the lane
struct Sums {
  u64 s[NS];                            // signed sums modulo 2^64
  i128 p[NP];
};

__device__ __forceinline__ void clear(Sums& v) {
#pragma unroll
  for (int i = 0; i < NS; ++i) v.s[i] = 0;
#pragma unroll
  for (int i = 0; i < NP; ++i) v.p[i] = 0;
}

template <bool THR>
__device__ __forceinline__ void add_pixel(Sums& v, long long a, long long b, bool above_a, bool above_b) {
  const i128 aa = (i128)a * a, bb = (i128)b * b, ab = (i128)a * b;
  v.s[0] += 1; v.s[1] += (u64)a; v.s[2] += (u64)b;
  v.p[0] += aa; v.p[1] += bb; v.p[2] += ab;
  if (THR) {
    if (above_a) v.s[4] += (u64)a;
    if (above_b) v.s[5] += (u64)b;
    if (above_a && above_b) {
      v.s[3] += 1; v.s[6] += (u64)a; v.s[7] += (u64)b;
      v.p[3] += aa; v.p[4] += bb; v.p[5] += ab;
    }
  }
}

template <bool THR>
__device__ __forceinline__ void complete(Sums& v) {
  if (!THR) {
    v.s[3] = v.s[0]; v.s[4] = v.s[1]; v.s[5] = v.s[2]; v.s[6] = v.s[1]; v.s[7] = v.s[2];
    v.p[3] = v.p[0]; v.p[4] = v.p[1]; v.p[5] = v.p[2];
  }
}

// the twenty words of one id to global memory
template <bool THR>
__device__ void to_global(u64* __restrict__ o, Sums v) {
  complete<THR>(v);
#pragma unroll
  for (int i = 0; i < NS; ++i)
    if (v.s[i]) atomicAdd(o + i, v.s[i]);
#pragma unroll
  for (int i = 0; i < NP; ++i) add128(o + NS + 2 * i, o + NS + 2 * i + 1, v.p[i]);
}

// a block's table holds what a run carries: LS 64-bit words, then LP (lo, hi) pairs
template <bool THR>
__device__ void add_sums(int* keys, u64 (*acc)[SLOTS], u64* __restrict__ out, int label, const Sums& v) {
  constexpr int LS = THR ? NS : 3, LP = THR ? NP : 3;
  const int slot = find_slot(keys, label);
  if (slot >= 0) {
#pragma unroll
    for (int i = 0; i < LS; ++i)
      if (v.s[i]) atomicAdd(&acc[i][slot], v.s[i]);
#pragma unroll
    for (int i = 0; i < LP; ++i) add128(&acc[LS + 2 * i][slot], &acc[LS + 2 * i + 1][slot], v.p[i]);
  } else {
    to_global<THR>(out + (size_t)label * NW, v);
  }
}

struct ProductsArgs {
  const int* lab;
  const long long* thr_a;
  const long long* thr_b;
  long long npix, ntiles, tiles_per_block, bound;
  int vec_lab, vec_a, vec_b;
  int nid, shift_a, shift_b;
  u64* out;
  int* bad;
};

// what a lane reads in one trip; a p0 at or past npix reads nothing: background and zeros
template <typename T> struct Trip {
  int l[PPL];
  Raw4<T> a, b;
};
template <typename T>
__device__ __forceinline__ Trip<T> load_trip(const ProductsArgs& a, const T* __restrict__ raw_a, const T* __restrict__ raw_b, long long p0) {
  Trip<T> r;
  load_labels(a.lab, a.vec_lab != 0, p0, a.npix, r.l);
  r.a = load_raw<T>(raw_a, a.vec_a != 0, p0, a.npix);
  r.b = load_raw<T>(raw_b, a.vec_b != 0, p0, a.npix);
  return r;
}

// THR false: thr_a and thr_b are never read
template <typename T, bool THR>
__global__ __launch_bounds__(BLOCK, THR ? 3 : 4) void products_kernel(ProductsArgs a, const T* __restrict__ raw_a, const T* __restrict__ raw_b) {
  constexpr int RS = THR ? NS : 3, RP = THR ? NP : 3;   // the words a run carries through the wave and the table keeps
  constexpr int LW = RS + 2 * RP;
  __shared__ int keys[SLOTS];
  __shared__ u64 acc[LW][SLOTS];
  for (int s = threadIdx.x; s < SLOTS; s += BLOCK) {
    keys[s] = 0;
#pragma unroll
    for (int w = 0; w < LW; ++w) acc[w][s] = 0;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const Tiles tiles = block_tiles(a.ntiles, a.tiles_per_block);
  const long long t0 = tiles.t0, t1 = tiles.t1;
  int tid = 0;                                          // the id whose thresholds the lane holds
  long long ta = 0, tb = 0;
  int any_bad = 0;
  // the loads of the next trip are issued before the work of this one: twice the bytes in flight a wave
  Trip<T> next = load_trip<T>(a, raw_a, raw_b, t0 < t1 ? lane_pixel(t0) : a.npix);
  for (long long t = t0; t < t1; ++t) {
    const Trip<T> now = next;
    int l[PPL];
#pragma unroll
    for (int k = 0; k < PPL; ++k) l[k] = now.l[k];
    if (clamp_labels(l, a.nid)) any_bad |= BAD_LABEL;
    // the thresholds of this trip's ids are gathered BEFORE the next trip's loads are issued: loads return in order, so a
    // gather behind them would wait for them all
    long long tha[PPL], thb[PPL];
    if (THR) {
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        if (l[k] > 0 && l[k] != tid) {                  // l[k] < nid: inside both arrays
          tid = l[k];
          ta = a.thr_a[tid];
          tb = a.thr_b[tid];
        }
        tha[k] = ta;
        thb[k] = tb;
      }
    }
    next = load_trip<T>(a, raw_a, raw_b, t + 1 < t1 ? lane_pixel(t + 1) : a.npix);
    const Raw4<T>& ra = now.a;
    const Raw4<T>& rb = now.b;
    long long qa[PPL], qb[PPL];
    bool ua[PPL], ub[PPL];                              // above a, above b
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      qa[k] = 0; qb[k] = 0; ua[k] = true; ub[k] = true;
      if (l[k] > 0) {
        const bool ok_a = quantise<T>(ra.v[k], a.shift_a, a.bound, &qa[k]);
        const bool ok_b = quantise<T>(rb.v[k], a.shift_b, a.bound, &qb[k]);
        if (!(ok_a && ok_b)) { l[k] = 0; any_bad |= BAD_VALUE; }         // the pixel is skipped
        if (THR) {
          ua[k] = qa[k] >= tha[k];
          ub[k] = qb[k] >= thb[k];
        }
      }
    }
    const bool uni = l[0] > 0 && l[0] == l[1] && l[1] == l[2] && l[2] == l[3];
    const Heads h = run_heads(uni, l, lane);
    const u64 heads = h.heads;
    const bool head = h.head;
    const int run = run_lanes(heads, lane);
    Sums v;
    clear(v);
    if (uni) {
#pragma unroll
      for (int k = 0; k < PPL; ++k) add_pixel<THR>(v, qa[k], qb[k], ua[k], ub[k]);
    }
    if (heads != ~0ull) {                               // the same for the whole wave: some run is longer than a lane
      // segmented reduction, spelled out (not region_scan.h's reduce_run): which words cross the wave depends on THR
      const int end = lane + run;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const bool take = lane + d < end;
#pragma unroll
        for (int i = 1; i < RS; ++i) {                  // s[0] is 4 pixels a lane: the run's length gives it
          const u64 o = __shfl_down(v.s[i], d);
          if (take) v.s[i] += o;
        }
#pragma unroll
        for (int i = 0; i < RP; ++i) {
          const i128 o = shfl_down128(v.p[i], d);
          if (take) v.p[i] += o;
        }
      }
    }
    if (uni) {
      if (head) {
        v.s[0] = (u64)(PPL * run);
        add_sums<THR>(keys, acc, a.out, l[0], v);
      }
    } else {
      int cur = 0;
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        if (l[k] != cur) {
          if (cur > 0) add_sums<THR>(keys, acc, a.out, cur, v);
          cur = l[k];
          clear(v);
        }
        if (cur > 0) add_pixel<THR>(v, qa[k], qb[k], ua[k], ub[k]);
      }
      if (cur > 0) add_sums<THR>(keys, acc, a.out, cur, v);
    }
  }
  if (any_bad) atomicOr(a.bad, any_bad);
  __syncthreads();

  for (int s = threadIdx.x; s < SLOTS; s += BLOCK) {
    const int label = keys[s];
    if (label == 0) continue;
    Sums v;
    clear(v);
#pragma unroll
    for (int i = 0; i < RS; ++i) v.s[i] = acc[i][s];
#pragma unroll
    for (int i = 0; i < RP; ++i) v.p[i] = (i128)(((unsigned __int128)acc[RS + 2 * i + 1][s] << 64) | acc[RS + 2 * i][s]);
    to_global<THR>(a.out + (size_t)label * NW, v);
  }
}

template <typename T>
void launch_products(const ProductsArgs& a, const void* raw_a, const void* raw_b, int grid, hipStream_t st) {
  if (a.thr_a)
    products_kernel<T, true><<<grid, BLOCK, 0, st>>>(a, (const T*)raw_a, (const T*)raw_b);
  else
    products_kernel<T, false><<<grid, BLOCK, 0, st>>>(a, (const T*)raw_a, (const T*)raw_b);
}

}  // namespace

extern "C" int clx_region_products(const int32_t* labels, const void* raw_a, const void* raw_b, int raw_type, long long npix,
                                   int nid, int shift_a, int shift_b, const long long* thr_a, const long long* thr_b,
                                   unsigned long long* out, int32_t* bad, clx_stream stream) {
  const char* who = "clx_region_products";
  CLX_REQUIRE(labels && raw_a && raw_b && out && bad, "%s: null pointer", who);
  CLX_REQUIRE((thr_a == nullptr) == (thr_b == nullptr), "%s: null pointer: thr_a and thr_b are given together or not at all", who);
  if (require_raw_channel(who, raw_type, nid) != CLX_OK) return CLX_ERR_ARG;
  CLX_REQUIRE(npix > 0 && npix < (1ll << 32), "%s: npix must lie in [1, 2^32)", who);
  hipStream_t st = (hipStream_t)stream;
  const Tiling t = tiling_for(npix, thr_a ? THR_GRID : MAX_GRID);
  ProductsArgs a;
  a.lab = labels; a.thr_a = thr_a; a.thr_b = thr_b;
  a.npix = npix; a.ntiles = t.ntiles; a.tiles_per_block = t.per_block;
  a.bound = value_bound(npix);
  a.vec_lab = aligned16(labels); a.vec_a = aligned16(raw_a); a.vec_b = aligned16(raw_b);
  a.nid = nid; a.shift_a = shift_a; a.shift_b = shift_b;
  a.out = out; a.bad = bad;
  launch_table_init<NW>(out, bad, nid, st);
  launch_for_raw(raw_type, [&](auto v) { launch_products<decltype(v)>(a, raw_a, raw_b, t.grid, st); });
  CLX_CHECK_LAUNCH(who);
  return CLX_OK;
}
