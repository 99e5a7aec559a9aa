// Per-object order statistics of one raw channel (the measure stage's quantiles, median and MAD):
//   clx_region_order_stats   per id and rank: the key of that rank among the order-preserving keys of the id's pixels
//   clx_region_order_phase   one of its two phases alone, for tools/bench_order_stats.py
// An order statistic cannot be accumulated in the one-pass frame of region_scan.h, so this runs in two phases.
//
// GATHER buckets the pixels by id.  The caller passes the pixel counts (clx_region_moments' area) and their exclusive
// prefix sum, so object i owns the segment [seg_base[i], seg_base[i] + area[i]) of a key buffer in the workspace.  One pass
// over labels and raw in the reading frame of region_scan.h: a run of uniform lanes with one id reserves its positions with
// one atomic add on the id's cursor, lanes on an object's edge reserve per stretch of equal ids, and a tile that is one id
// from end to end reserves once for the block.  Which run gets which
// positions depends on the order of the atomics, so the order inside a segment differs from run to run; the MULTISET of a
// segment's keys is determined by the map, and the key of a given rank in a multiset does not depend on its order.  That is
// why the outputs are the same bits in every run.
//
// SELECT has three regimes by the length of a segment (the constants are quoted in DESIGN.md 3.3g, from where the tests
// read them):
//   area <= SORT_MAX               one block loads the segment into LDS, sorts it (bitonic network) and reads the ranks off
//   SORT_MAX < area <= BLOCK_MAX   one block, most-significant-digit radix select with 8-bit digits: per pass a 256-bin
//                                  histogram in LDS of the keys that carry a rank's prefix, then the bin the rank falls into
//   area > BLOCK_MAX               the same passes by many blocks: the segment is cut into parts of PART_KEYS keys, a block
//                                  adds its part's histogram to one in global memory, one block per object picks the bins
// Ranks that fall into one bin share a prefix ("group") and a histogram, so the two ranks of a quantile, which are
// neighbours, cost one histogram until the last digits.  A pass compares a key with the at most nq distinct prefixes.
// float32 / int32 keys without a centre lie in the low 32 bits: their passes start at bit 24 (4 passes, not 8).
// LDS: the sort buffer and the histograms share 32 KiB (SORT_MAX keys of 8 bytes = 32 groups x 256 bins x 4 bytes), so four
// blocks (16 waves) fit the 160 KiB of a CU.  The number of launches does not depend on the objects or the ranks: init, gather, select,
// and where total > BLOCK_MAX one list kernel and two kernels per pass.
#include "region_sums.h"

namespace {

enum { BAD_AREA = 4, BAD_RANK = 8 };    // beside BAD_LABEL and BAD_VALUE

constexpr int MAX_NQ = 32;
constexpr int BINS = 256;
constexpr int SORT_MAX = 4096;          // keys sorted in LDS
constexpr long long BLOCK_MAX = 65536;  // keys one block selects from alone
constexpr int PART_KEYS = 16384;        // keys of a longer segment a block takes per pass
constexpr int LOADS = 4;                // keys a thread has in flight in a histogram pass
constexpr int SELECT_GRID = 2048;
constexpr int BIG_GRID = 2048;

__device__ __forceinline__ bool finite_value(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ bool finite_value(double v) {
  return ((u64)__double_as_longlong(v) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}
__device__ __forceinline__ bool finite_value(int) { return true; }

// whether [base, base + area) lies inside the key buffer: area and seg_base are the caller's, nothing is indexed before this
__device__ __forceinline__ bool segment_ok(u64 base, u64 area, u64 total) { return base <= total && area <= total - base; }

__global__ void order_init(u64* __restrict__ out, long long nout, u64* __restrict__ cursor, int nid, int* __restrict__ bad) {
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 == 0) *bad = 0;
  for (long long i = i0; i < nout; i += (long long)gridDim.x * blockDim.x) out[i] = ~0ull;
  for (long long i = i0; i < nid; i += (long long)gridDim.x * blockDim.x) cursor[i] = 0;
}

// ---------------------------------------------------------------------------------------------------------
// phase one

// one key into position `pos` of a segment of `a` keys at `b`; past its end the key is dropped: nothing is written outside
__device__ __forceinline__ int put_key(u64* __restrict__ keys, u64 a, u64 b, bool ok, u64 pos, u64 key) {
  if (ok && pos < a) { keys[b + pos] = key; return 0; }
  return BAD_AREA;
}

template <typename T, bool CENTRE>
__global__ __launch_bounds__(BLOCK) void gather_kernel(const int* __restrict__ lab, const T* __restrict__ raw, int vec_lab,
                                                       int vec_raw, long long npix, int nid, long long ntiles,
                                                       long long tiles_per_block, const u64* __restrict__ area,
                                                       const u64* __restrict__ seg_base, u64 total,
                                                       const double* __restrict__ centre, u64* __restrict__ cursor,
                                                       u64* __restrict__ keys, int* __restrict__ bad) {
  __shared__ int wave_id[2][BLOCK / 64];
  __shared__ u64 tile_pos;
  static_assert(BLOCK / 64 == 4, "whole_tile compares four waves");
  const int lane = threadIdx.x & 63;
  const Tiles tiles = block_tiles(ntiles, tiles_per_block);
  int any_bad = 0;
  for (long long t = tiles.t0; t < tiles.t1; ++t) {
    const long long p0 = lane_pixel(t);
    int l[PPL];
    load_labels(lab, vec_lab != 0, p0, npix, l);
    if (clamp_labels(l, nid)) any_bad |= BAD_LABEL;
    Raw4<T> rv;                                         // load_raw spelled out: through the helper the int kernel ran 5 % slower
    if (vec_raw && p0 + PPL <= npix) {
      rv = *reinterpret_cast<const Raw4<T>*>(raw + p0);
    } else {
#pragma unroll
      for (int k = 0; k < PPL; ++k) rv.v[k] = p0 + k < npix ? raw[p0 + k] : (T)0;
    }
    u64 key[PPL];
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      key[k] = 0;
      if (l[k] > 0) {
        if (!finite_value(rv.v[k])) any_bad |= BAD_VALUE;           // the key is still written: the segment stays full
        key[k] = CENTRE ? order_key(fabs((double)rv.v[k] - centre[l[k]])) : order_key(rv.v[k]);
      }
    }
    const bool uni = l[0] > 0 && l[0] == l[1] && l[1] == l[2] && l[2] == l[3];
    const Heads h = run_heads(uni, l, lane);
    const u64 heads = h.heads;
    const bool head = h.head;
    const int n = run_lanes(heads, lane);
    const int head_lane = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));     // lane 0 is always a head
    // a tile that is one id from end to end (the inside of a large object) reserves once for the block: on the map that is
    // one object everywhere every reservation goes to the same cursor, and they are what the pass waits for
    const bool whole_wave = heads == 1ull && (__ballot(uni) & 1ull);
    int* ids = wave_id[(int)(t & 1)];                     // two sets: a wave may be one tile ahead of the slowest
    if (lane == 0) ids[threadIdx.x >> 6] = whole_wave ? l[0] : 0;
    __syncthreads();
    const bool whole_tile = ids[0] > 0 && ids[1] == ids[0] && ids[2] == ids[0] && ids[3] == ids[0];
    u64 pos = 0;
    if (whole_tile) {                                     // the same for the whole block
      if (threadIdx.x == 0) tile_pos = atomicAdd(&cursor[l[0]], (u64)TILE);
      __syncthreads();
      pos = tile_pos + (u64)((threadIdx.x >> 6) * 64 * PPL);
    } else {
      if (uni && head) pos = atomicAdd(&cursor[l[0]], (u64)(n * PPL));        // one reservation for the whole run
      pos = __shfl(pos, head_lane);
    }
    if (uni) {
      const u64 a = area[l[0]], b = seg_base[l[0]];
      const bool ok = segment_ok(b, a, total);
      pos += (u64)((lane - head_lane) * PPL);
#pragma unroll
      for (int k = 0; k < PPL; ++k) any_bad |= put_key(keys, a, b, ok, pos + k, key[k]);
    } else {
      u64 a = 0, b = 0, at = 0;
      bool ok = false;
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        if (l[k] == 0) continue;
        if (k == 0 || l[k] != l[k - 1]) {                 // a stretch of equal ids starts: reserve it whole
          int n_same = 1;
          bool still = true;
#pragma unroll
          for (int j = k + 1; j < PPL; ++j) {
            still = still && l[j] == l[k];
            n_same += still ? 1 : 0;
          }
          at = atomicAdd(&cursor[l[k]], (u64)n_same);
          a = area[l[k]]; b = seg_base[l[k]];
          ok = segment_ok(b, a, total);
        }
        any_bad |= put_key(keys, a, b, ok, at, key[k]);
        ++at;
      }
    }
  }
  if (any_bad) atomicOr(bad, any_bad);
}

// ---------------------------------------------------------------------------------------------------------
// phase two

// what a radix select knows about the ranks of one object between two passes
struct SelState {
  u64 prefix[MAX_NQ];   // [group] the digits chosen so far (the key shifted right by the bits not yet decided)
  u64 rem[MAX_NQ];      // [rank column] the rank among the keys that carry its group's prefix
  u64 next[MAX_NQ];     // [rank column] scratch of select_bins
  int group[MAX_NQ];    // [rank column] -1: the rank is not below the area
  int ngroups;
};

// called by one thread
__device__ void state_start(SelState* S, const u64* __restrict__ rank_row, int nq, u64 area, int* __restrict__ bad) {
  bool over = false;
  for (int r = 0; r < nq; ++r) {
    const u64 rk = rank_row[r];
    S->group[r] = rk < area ? 0 : -1;
    S->rem[r] = rk;
    over |= rk >= area;
  }
  S->prefix[0] = 0;
  S->ngroups = 1;
  if (over) atomicOr(bad, BAD_RANK);
}

// adds the n keys at `seg` to the histograms hist[group][BINS] of the digit at `shift`; prefix / ngroups as in SelState.
// Called by the whole block.  Raw data often agrees in its leading digits (16-bit counts in an int32), so a wave whose
// lanes mostly hit one bin adds them with one atomic.
__device__ __forceinline__ void histogram_keys(const u64* __restrict__ seg, long long n, int shift, const u64* prefix, int ngroups,
                                               unsigned int* hist) {
  const int lane = threadIdx.x & 63;
  for (long long i0 = 0; i0 < n; i0 += BLOCK * LOADS) {
    u64 k[LOADS];
    bool ok[LOADS];
#pragma unroll
    for (int u = 0; u < LOADS; ++u) {
      const long long i = i0 + u * BLOCK + threadIdx.x;
      ok[u] = i < n;
      k[u] = ok[u] ? seg[i] : 0ull;
    }
#pragma unroll
    for (int u = 0; u < LOADS; ++u) {
      int bin = -1;
      if (ok[u]) {
        const u64 hi = shift >= 56 ? 0ull : k[u] >> (shift + 8);
        for (int g = 0; g < ngroups; ++g)
          if (prefix[g] == hi) { bin = g * BINS + (int)((k[u] >> shift) & 0xFFull); break; }
      }
      const u64 live = __ballot(bin >= 0);
      if (!live) continue;                                // the same for the whole wave
      const int lead = __ffsll((long long)live) - 1;
      const int lead_bin = __shfl(bin, lead);
      const u64 same = __ballot(bin == lead_bin);
      if (lane == lead) atomicAdd(&hist[lead_bin], (unsigned int)__popcll(same));
      else if (bin >= 0 && bin != lead_bin) atomicAdd(&hist[bin], 1u);
    }
  }
}

// from complete histograms: the bin every rank falls into, its rank inside that bin, and the groups of the next pass.
// Called by the whole block, which has synchronised after the last add to hist; synchronises before it returns.
__device__ void select_bins(SelState* S, const unsigned int* hist, int nq) {
  const int r = threadIdx.x;
  if (r < nq && S->group[r] >= 0) {
    const unsigned int* h = hist + S->group[r] * BINS;
    u64 before = 0;
    int b = 0;
    for (; b < BINS - 1; ++b) {                           // a rank below the group's count stops inside; else the last bin
      const u64 c = h[b];
      if (S->rem[r] < before + c) break;
      before += c;
    }
    S->rem[r] -= before;
    S->next[r] = (S->prefix[S->group[r]] << 8) | (u64)b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int ng = 0;
    for (int q = 0; q < nq; ++q) {
      if (S->group[q] < 0) continue;
      int g = 0;
      while (g < ng && S->prefix[g] != S->next[q]) ++g;
      if (g == ng) S->prefix[ng++] = S->next[q];
      S->group[q] = g;
    }
    S->ngroups = ng > 0 ? ng : 1;
  }
  __syncthreads();
}

__global__ __launch_bounds__(BLOCK) void select_kernel(const u64* __restrict__ keys, const u64* __restrict__ area,
                                                       const u64* __restrict__ seg_base, const u64* __restrict__ cursor,
                                                       const u64* __restrict__ rank, int nq, int nid, u64 total, int first_shift,
                                                       u64* __restrict__ counter, u64* __restrict__ out, int* __restrict__ bad) {
  if (blockIdx.x == 0 && threadIdx.x == 0) counter[0] = 0;          // big_list, the next launch, counts from here
  __shared__ u64 buf[SORT_MAX];                           // the sort buffer, or the histograms of MAX_NQ groups
  __shared__ SelState S;
  static_assert(sizeof(u64) * SORT_MAX >= sizeof(unsigned int) * MAX_NQ * BINS, "the histograms live in the sort buffer");
  unsigned int* hist = reinterpret_cast<unsigned int*>(buf);
  for (int id = 1 + blockIdx.x; id < nid; id += gridDim.x) {
    const u64 a = area[id], base = seg_base[id];          // the same for every thread: the branches below are uniform
    if (a == 0) continue;
    if (!segment_ok(base, a, total)) {
      if (threadIdx.x == 0) atomicOr(bad, BAD_AREA);
      continue;
    }
    if (threadIdx.x == 0 && cursor[id] != a) atomicOr(bad, BAD_AREA);
    if (a > (u64)BLOCK_MAX) continue;                     // big_* below
    const u64* seg = keys + base;
    const u64* rank_row = rank + (size_t)id * nq;
    u64* out_row = out + (size_t)id * nq;
    if (a <= (u64)SORT_MAX) {
      int m = 1;
      while ((u64)m < a) m <<= 1;
      for (int i = threadIdx.x; i < m; i += BLOCK) buf[i] = (u64)i < a ? seg[i] : ~0ull;
      __syncthreads();
      for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
          for (int i = threadIdx.x; i < m; i += BLOCK) {
            const int p = i ^ j;
            if (p > i) {
              const u64 x = buf[i], y = buf[p];
              if ((x > y) == ((i & k) == 0)) { buf[i] = y; buf[p] = x; }
            }
          }
          __syncthreads();
        }
      if (threadIdx.x < nq) {
        const u64 rk = rank_row[threadIdx.x];
        if (rk < a) out_row[threadIdx.x] = buf[rk];
        else atomicOr(bad, BAD_RANK);                     // the element stays ~0
      }
      __syncthreads();
    } else {
      if (threadIdx.x == 0) state_start(&S, rank_row, nq, a, bad);
      __syncthreads();
      for (int shift = first_shift; shift >= 0; shift -= 8) {
        for (int i = threadIdx.x; i < S.ngroups * BINS; i += BLOCK) hist[i] = 0;
        __syncthreads();
        histogram_keys(seg, (long long)a, shift, S.prefix, S.ngroups, hist);
        __syncthreads();
        select_bins(&S, hist, nq);
      }
      if (threadIdx.x < nq && S.group[threadIdx.x] >= 0) out_row[threadIdx.x] = S.prefix[S.group[threadIdx.x]];
      __syncthreads();
    }
  }
}

// segments longer than BLOCK_MAX: a list of them, then per pass big_histogram (many blocks) and big_select (one per object)
struct BigObject {
  int id;
  unsigned int part_base, parts;      // the object's parts are the work items [part_base, part_base + parts) of a pass
  int pad;
  SelState S;
};

// counter[0]: objects listed << 32 | parts handed out.  One atomic moves both, so the list is ascending in part_base.
__global__ void big_list(const u64* __restrict__ area, const u64* __restrict__ seg_base, const u64* __restrict__ rank, int nq,
                         int nid, u64 total, int max_big, u64* __restrict__ counter, BigObject* __restrict__ big,
                         unsigned int* __restrict__ big_hist, int* __restrict__ bad) {
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id < 1 || id >= nid) return;
  const u64 a = area[id];
  if (a <= (u64)BLOCK_MAX || !segment_ok(seg_base[id], a, total)) return;
  const unsigned int parts = (unsigned int)((a + PART_KEYS - 1) / PART_KEYS);
  const u64 old = atomicAdd(counter, (1ull << 32) | parts);
  const u64 slot = old >> 32;
  if (slot >= (u64)max_big) {                             // only where area does not add up to total
    atomicOr(bad, BAD_AREA);
    return;
  }
  BigObject* o = big + slot;
  o->id = id;
  o->part_base = (unsigned int)old;
  o->parts = parts;
  state_start(&o->S, rank + (size_t)id * nq, nq, a, bad);
  for (int i = 0; i < BINS; ++i) big_hist[slot * (MAX_NQ * BINS) + i] = 0;
}

__device__ __forceinline__ int listed(const u64* counter, int max_big) {
  const u64 n = *counter >> 32;
  return (int)(n < (u64)max_big ? n : (u64)max_big);
}

__global__ __launch_bounds__(BLOCK) void big_histogram(const u64* __restrict__ keys, const u64* __restrict__ area,
                                                       const u64* __restrict__ seg_base, const u64* __restrict__ counter,
                                                       int max_big, const BigObject* __restrict__ big,
                                                       unsigned int* __restrict__ big_hist, int shift) {
  __shared__ unsigned int hist[MAX_NQ * BINS];
  __shared__ u64 prefix[MAX_NQ];
  const int nbig = listed(counter, max_big);
  if (nbig == 0) return;
  const unsigned int nparts = (unsigned int)*counter;
  for (unsigned int w = blockIdx.x; w < nparts; w += gridDim.x) {
    int lo = 0, hi = nbig - 1;                            // the last object whose part_base is at most w
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (big[mid].part_base <= w) lo = mid; else hi = mid - 1;
    }
    const BigObject* o = big + lo;
    const unsigned int part = w - o->part_base;
    if (o->part_base > w || part >= o->parts) continue;   // parts of an object the list had no room for
    const int ng = o->S.ngroups;
    __syncthreads();                                      // the trip before has flushed
    if (threadIdx.x < ng) prefix[threadIdx.x] = o->S.prefix[threadIdx.x];
    for (int i = threadIdx.x; i < ng * BINS; i += BLOCK) hist[i] = 0;
    __syncthreads();
    const u64 a = area[o->id];
    const u64 begin = (u64)part * PART_KEYS;
    const long long n = (long long)(a - begin < (u64)PART_KEYS ? a - begin : (u64)PART_KEYS);
    histogram_keys(keys + seg_base[o->id] + begin, n, shift, prefix, ng, hist);
    __syncthreads();
    unsigned int* g = big_hist + (size_t)lo * (MAX_NQ * BINS);
    for (int i = threadIdx.x; i < ng * BINS; i += BLOCK)
      if (hist[i]) atomicAdd(&g[i], hist[i]);
  }
}

__global__ __launch_bounds__(BLOCK) void big_select(const u64* __restrict__ counter, int max_big, BigObject* __restrict__ big,
                                                    unsigned int* __restrict__ big_hist, int nq, int last,
                                                    u64* __restrict__ out) {
  __shared__ unsigned int hist[MAX_NQ * BINS];
  __shared__ SelState S;
  const int nbig = listed(counter, max_big);
  for (int s = blockIdx.x; s < nbig; s += gridDim.x) {
    BigObject* o = big + s;
    unsigned int* g = big_hist + (size_t)s * (MAX_NQ * BINS);
    __syncthreads();
    if (threadIdx.x < MAX_NQ) {
      const int r = threadIdx.x;
      S.prefix[r] = o->S.prefix[r]; S.rem[r] = o->S.rem[r]; S.group[r] = o->S.group[r];
      if (r == 0) S.ngroups = o->S.ngroups;
    }
    const int ng = o->S.ngroups;
    for (int i = threadIdx.x; i < ng * BINS; i += BLOCK) hist[i] = g[i];
    __syncthreads();
    select_bins(&S, hist, nq);
    if (threadIdx.x < MAX_NQ) {
      const int r = threadIdx.x;
      o->S.prefix[r] = S.prefix[r]; o->S.rem[r] = S.rem[r]; o->S.group[r] = S.group[r];
      if (r == 0) o->S.ngroups = S.ngroups;
      if (last && r < nq && S.group[r] >= 0) out[(size_t)o->id * nq + r] = S.prefix[S.group[r]];
    }
    for (int i = threadIdx.x; i < S.ngroups * BINS; i += BLOCK) g[i] = 0;     // for the next pass
  }
}

// workspace: keys [total] | cursor [nid] | counter [2] | BigObject [max_big] | histograms [max_big][MAX_NQ][BINS]
struct Layout {
  size_t cursor, counter, big, hist, bytes;
  int max_big;
};
inline Layout layout_for(long long total, int nid) {
  Layout L;
  L.max_big = (int)(total / BLOCK_MAX);                   // fewer than this many segments are longer than BLOCK_MAX
  L.cursor = (size_t)total * sizeof(u64);
  L.counter = L.cursor + (size_t)nid * sizeof(u64);
  L.big = L.counter + 2 * sizeof(u64);
  L.hist = L.big + (size_t)L.max_big * sizeof(BigObject);
  L.bytes = L.hist + (size_t)L.max_big * MAX_NQ * BINS * sizeof(unsigned int);
  return L;
}
static_assert(sizeof(BigObject) % 8 == 0, "the histograms behind the list stay 8-byte aligned");

}  // namespace

extern "C" size_t clx_region_order_workspace(long long total, int nid) {
  if (total < 0 || total >= (1ll << 32) || nid < 1 || nid > (1 << 24)) return 0;
  return layout_for(total, nid).bytes;
}

// phases: bit 0 initialise and gather, bit 1 select; who: the entry point the refusals name
static int order_run(const int32_t* labels, const void* raw, int raw_type, long long npix, int nid, const unsigned long long* area,
                     const unsigned long long* seg_base, long long total, const double* centre, const unsigned long long* rank,
                     int nq, unsigned long long* out, void* workspace, size_t workspace_bytes, int32_t* bad, int phases,
                     const char* who, clx_stream stream) {
  CLX_REQUIRE(labels && raw && area && seg_base && rank && out && workspace && bad, "%s: null pointer", who);
  if (require_raw_channel(who, raw_type, nid) != CLX_OK) return CLX_ERR_ARG;
  CLX_REQUIRE(npix > 0 && npix < (1ll << 32), "%s: npix must lie in [1, 2^32)", who);
  CLX_REQUIRE(nq >= 1 && nq <= MAX_NQ, "%s: nq must lie in [1, 32]", who);
  CLX_REQUIRE(total >= 0 && total <= npix, "%s: total must lie in [0, npix]", who);
  CLX_REQUIRE(workspace_bytes >= clx_region_order_workspace(total, nid),
              "%s: workspace_bytes is below clx_region_order_workspace(total, nid)", who);
  CLX_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", who);
  hipStream_t st = (hipStream_t)stream;
  const Layout L = layout_for(total, nid);
  char* ws = (char*)workspace;
  u64* keys = (u64*)ws;
  u64* cursor = (u64*)(ws + L.cursor);
  u64* counter = (u64*)(ws + L.counter);
  BigObject* big = (BigObject*)(ws + L.big);
  unsigned int* big_hist = (unsigned int*)(ws + L.hist);
  const long long nout = (long long)nid * nq;
  const long long init_blocks = (nout + 255) / 256;
  if (phases & 1)
    order_init<<<(int)(init_blocks < 4096 ? init_blocks : 4096), 256, 0, st>>>(out, nout, cursor, nid, bad);
  if (total > 0 && nid > 1 && (phases & 1)) {
    const Tiling t = tiling_for(npix);
    launch_for_raw(raw_type, [&](auto v) {
      using T = decltype(v);
      auto* gather = centre ? gather_kernel<T, true> : gather_kernel<T, false>;
      gather<<<t.grid, BLOCK, 0, st>>>(labels, (const T*)raw, aligned16(labels), aligned16(raw), npix, nid, t.ntiles, t.per_block,
                                       area, seg_base, (u64)total, centre, cursor, keys, bad);
    });
  }
  if (total > 0 && nid > 1 && (phases & 2)) {
    // float32 / int32 keys lie in the low 32 bits; |v - centre| is a float64 whatever the raw type
    const int first_shift = (raw_type == CLX_RAW_F64 || centre) ? 56 : 24;
    const int sgrid = nid - 1 < SELECT_GRID ? nid - 1 : SELECT_GRID;
    select_kernel<<<sgrid, BLOCK, 0, st>>>(keys, area, seg_base, cursor, rank, nq, nid, (u64)total, first_shift, counter, out, bad);
    if (L.max_big > 0) {
      big_list<<<(nid + 255) / 256, 256, 0, st>>>(area, seg_base, rank, nq, nid, (u64)total, L.max_big, counter, big, big_hist, bad);
      const long long max_parts = total / PART_KEYS + L.max_big;
      const int hgrid = (int)(max_parts < BIG_GRID ? max_parts : BIG_GRID);
      const int bgrid = L.max_big < 1024 ? L.max_big : 1024;
      for (int shift = first_shift; shift >= 0; shift -= 8) {
        big_histogram<<<hgrid, BLOCK, 0, st>>>(keys, area, seg_base, counter, L.max_big, big, big_hist, shift);
        big_select<<<bgrid, BLOCK, 0, st>>>(counter, L.max_big, big, big_hist, nq, shift == 0, out);
      }
    }
  }
  CLX_CHECK_LAUNCH(who);
  return CLX_OK;
}

extern "C" int clx_region_order_stats(const int32_t* labels, const void* raw, int raw_type, long long npix, int nid,
                                      const unsigned long long* area, const unsigned long long* seg_base, long long total,
                                      const double* centre, const unsigned long long* rank, int nq, unsigned long long* out,
                                      void* workspace, size_t workspace_bytes, int32_t* bad, clx_stream stream) {
  return order_run(labels, raw, raw_type, npix, nid, area, seg_base, total, centre, rank, nq, out, workspace, workspace_bytes, bad,
                   3, "clx_region_order_stats", stream);
}

extern "C" int clx_region_order_phase(const int32_t* labels, const void* raw, int raw_type, long long npix, int nid,
                                      const unsigned long long* area, const unsigned long long* seg_base, long long total,
                                      const double* centre, const unsigned long long* rank, int nq, unsigned long long* out,
                                      void* workspace, size_t workspace_bytes, int32_t* bad, int phase, clx_stream stream) {
  CLX_REQUIRE(phase == 1 || phase == 2, "clx_region_order_phase: phase must be 1 (gather) or 2 (select)");
  return order_run(labels, raw, raw_type, npix, nid, area, seg_base, total, centre, rank, nq, out, workspace, workspace_bytes, bad,
                   phase, "clx_region_order_phase", stream);
}
