// "relate" stage: what connects two label maps of the same image (cells and their nuclei, a prediction and a reference).
//   clx_label_overlaps     the sparse joint histogram: pixels per pair (a[p], b[p]) != (0, 0), a SET of unknown size
//   clx_region_clearance   per id of a, over its pixels inside the object of b it was assigned to: their number, the smallest
//                          value of b's distance map with the first pixel that attains it, and the map's sum
// Both stream 8 (12) bytes a pixel in the reading frame of region_scan.h: a lane reads 4 consecutive pixels of every map,
// 16-byte loads where that map's pointer allows, and a ballot cuts the wave into runs of lanes that carry one value.  The
// next trip's pixels are loaded before the current trip's are counted (5 - 9 % of the time at 4096^2).
//
// Overlaps.  The value is the 64-bit pair (a << 32) | b.  A lane whose four pairs are equal and not (0, 0) is uniform; the
// head of a run of uniform lanes with one pair adds 4 x run length with a single add: the count IS the length, so there is
// no wave reduction at all.  A wave whose pixels are all (0, 0) skips the trip.  A lane on an edge walks its four pixels and
// merges equal neighbours into one add, as face() does in contacts_kernel.  Adds go into the block's pair table in LDS
// (pair_table.h: keyed by the pair, hashed with mix64, CSLOTS slots, CPROBES tries, then straight to the global table),
// which is flushed into the global table once; the contract of the global table is clx_region_contacts'.
//
// Clearance.  A pixel counts when i = a[p] lies in [1, nid_a), parent[i] > 0 and b[p] == parent[i]; parent[] is the only
// indexed read, by the clamped i.  The frame is inscribed_kernel's (label_distance.hip) with the minimum in place of the
// maximum: (dist_sq << 32) | p is one 64-bit key whose atomicMin gives the smallest distance and the first pixel in raster
// order that attains it; a segmented wave reduction combines the keys and sums of a run, whose count again is its length.
// The block's table in LDS is keyed by id (find_slot) and flushed once.
//
// Integer adds and minima only: the same maps give the same set / rows in every run.
// hipcc --offload-arch=gfx950 -O3 reports: overlaps_kernel 42 VGPRs, no spills, 8192 bytes of LDS; clearance_kernel 61 VGPRs,
// no spills, 7168 bytes of LDS: 8 waves a SIMD for both.
#include "pair_table.h"

namespace {

constexpr unsigned int DIST_INF = (unsigned int)CLX_DIST_INF;
enum { BAD_A = 1, BAD_B = 2, BAD_DISTANCE = 2 };

__global__ __launch_bounds__(BLOCK) void overlaps_kernel(const int* __restrict__ a, const int* __restrict__ b, int vec_a, int vec_b,
                                                         long long npix, int nid_a, int nid_b, long long ntiles,
                                                         long long tiles_per_block, ContactsOut o) {
  __shared__ u64 lkeys[CSLOTS];
  __shared__ u64 lcnt[CSLOTS];
  for (int s = threadIdx.x; s < CSLOTS; s += BLOCK) { lkeys[s] = 0; lcnt[s] = 0; }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const Tiles tiles = block_tiles(ntiles, tiles_per_block);
  const long long t0 = tiles.t0, t1 = tiles.t1;
  int any_bad = 0;
  int na[PPL], nb[PPL];                                   // the next trip's pixels: on their way while this trip's are counted
  if (t0 < t1) {
    const long long p0 = lane_pixel(t0);
    load_labels(a, vec_a != 0, p0, npix, na);             // past the end of the maps: (0, 0), which is not counted
    load_labels(b, vec_b != 0, p0, npix, nb);
  }
  for (long long t = t0; t < t1; ++t) {
    int la[PPL], lb[PPL];
#pragma unroll
    for (int k = 0; k < PPL; ++k) { la[k] = na[k]; lb[k] = nb[k]; }
    if (t + 1 < t1) {
      const long long p1 = lane_pixel(t + 1);
      load_labels(a, vec_a != 0, p1, npix, na);
      load_labels(b, vec_b != 0, p1, npix, nb);
    }
    if (clamp_labels(la, nid_a)) any_bad |= BAD_A;
    if (clamp_labels(lb, nid_b)) any_bad |= BAD_B;
    u64 key[PPL];
#pragma unroll
    for (int k = 0; k < PPL; ++k) key[k] = ((u64)(unsigned int)la[k] << 32) | (u64)(unsigned int)lb[k];
    if (__ballot((key[0] | key[1] | key[2] | key[3]) != 0ull) == 0ull) continue;

    const bool uni = key[0] != 0ull && key[0] == key[1] && key[1] == key[2] && key[2] == key[3];
    const Heads h = run_heads(uni, key, lane);
    if (uni) {
      if (h.head) add_pair(lkeys, lcnt, o, key[0], (unsigned int)(PPL * run_lanes(h.heads, lane)));
    } else {
      u64 cur = 0ull;
      unsigned int n = 0;
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        if (key[k] != cur) {
          if (cur) add_pair(lkeys, lcnt, o, cur, n);
          cur = key[k]; n = 0;
        }
        ++n;
      }
      if (cur) add_pair(lkeys, lcnt, o, cur, n);
    }
  }
  if (any_bad) atomicOr(o.info, any_bad);
  __syncthreads();

  for (int s = threadIdx.x; s < CSLOTS; s += BLOCK)
    if (lkeys[s]) pair_to_global(o, lkeys[s], lcnt[s], mix64(lkeys[s]));
}

// ---------------------------------------------------------------------------------------------------------

// n counted pixels of `label`: Σ dist_sq = s, smallest key kmin
__device__ void add_clearance(int* keys, u64* scnt, u64* ssum, u64* smin, u64* __restrict__ out, int label, u64 n, u64 s, u64 kmin) {
  const int slot = find_slot(keys, label);
  if (slot >= 0) {
    atomicAdd(&scnt[slot], n);
    atomicAdd(&ssum[slot], s);
    atomicMin(&smin[slot], kmin);
  } else {
    u64* o = out + (size_t)label * 3;
    atomicAdd(o, n);
    if (s) atomicAdd(o + 2, s);
    if (kmin < o[1]) atomicMin(o + 1, kmin);              // the plain read only filters
  }
}

__global__ __launch_bounds__(BLOCK) void clearance_kernel(const int* __restrict__ a, const int* __restrict__ b,
                                                          const int* __restrict__ dist, const int* __restrict__ parent, int vec_a,
                                                          int vec_b, int vec_dist, long long npix, int nid_a, long long ntiles,
                                                          long long tiles_per_block, u64* __restrict__ out, int* __restrict__ bad) {
  __shared__ int keys[SLOTS];
  __shared__ u64 scnt[SLOTS], ssum[SLOTS], smin[SLOTS];
  for (int s = threadIdx.x; s < SLOTS; s += BLOCK) { keys[s] = 0; scnt[s] = 0; ssum[s] = 0; smin[s] = ~0ull; }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const Tiles tiles = block_tiles(ntiles, tiles_per_block);
  const long long t0 = tiles.t0, t1 = tiles.t1;
  int any_bad = 0;
  int na[PPL], nb[PPL], nd[PPL];                          // the next trip's pixels, as in overlaps_kernel
  if (t0 < t1) {
    const long long p0 = lane_pixel(t0);
    load_labels(a, vec_a != 0, p0, npix, na);
    load_labels(b, vec_b != 0, p0, npix, nb);
    load_labels(dist, vec_dist != 0, p0, npix, nd);
  }
  for (long long t = t0; t < t1; ++t) {
    const long long p0 = lane_pixel(t);
    int ia[PPL], lb[PPL], dv[PPL], l[PPL];                // l: the id of a counted pixel, or 0
#pragma unroll
    for (int k = 0; k < PPL; ++k) { ia[k] = na[k]; lb[k] = nb[k]; dv[k] = nd[k]; }
    if (t + 1 < t1) {
      const long long p1 = p0 + TILE;
      load_labels(a, vec_a != 0, p1, npix, na);
      load_labels(b, vec_b != 0, p1, npix, nb);           // only compared
      load_labels(dist, vec_dist != 0, p1, npix, nd);
    }
    if (clamp_labels(ia, nid_a)) any_bad |= BAD_A;
    if (__ballot((ia[0] | ia[1] | ia[2] | ia[3]) != 0) == 0ull) continue; // no pixel of a in the wave
    u64 key[PPL];
    SumKey<false> v = {0, ~0ull};                         // Σ dist_sq and the smallest key
    int par = 0;
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      if (k == 0 || ia[k] != ia[k - 1]) par = ia[k] > 0 ? parent[ia[k]] : 0;      // ia[k] < nid_a after the clamp
      bool counted = par > 0 && lb[k] == par;
      if (counted && (unsigned int)dv[k] > DIST_INF) { counted = false; any_bad |= BAD_DISTANCE; }     // the pixel is skipped
      l[k] = counted ? ia[k] : 0;
      key[k] = l[k] > 0 ? ((u64)(unsigned int)dv[k] << 32) | (u64)(unsigned int)(p0 + k) : ~0ull;
      if (l[k] > 0) v.s += (u64)(unsigned int)dv[k];
      v.k = key[k] < v.k ? key[k] : v.k;
    }
    const bool uni = l[0] > 0 && l[0] == l[1] && l[1] == l[2] && l[2] == l[3];
    const Heads h = run_heads(uni, l, lane);
    const int run = run_lanes(h.heads, lane);
    v = reduce_run(v, lane, lane + run);
    if (uni) {
      if (h.head) add_clearance(keys, scnt, ssum, smin, out, l[0], (u64)(PPL * run), v.s, v.k);
    } else {
      int cur = 0;
      u64 cn = 0, cs = 0, ck = ~0ull;
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        if (l[k] != cur) {
          if (cur > 0) add_clearance(keys, scnt, ssum, smin, out, cur, cn, cs, ck);
          cur = l[k]; cn = 0; cs = 0; ck = ~0ull;
        }
        ++cn;
        if (l[k] > 0) cs += (u64)(unsigned int)dv[k];
        ck = key[k] < ck ? key[k] : ck;
      }
      if (cur > 0) add_clearance(keys, scnt, ssum, smin, out, cur, cn, cs, ck);
    }
  }
  if (any_bad) atomicOr(bad, any_bad);
  __syncthreads();

  for (int s = threadIdx.x; s < SLOTS; s += BLOCK) {
    const int label = keys[s];
    if (label == 0) continue;
    u64* o = out + (size_t)label * 3;
    if (scnt[s]) atomicAdd(o, scnt[s]);
    if (ssum[s]) atomicAdd(o + 2, ssum[s]);
    if (smin[s] < o[1]) atomicMin(o + 1, smin[s]);
  }
}

}  // namespace

extern "C" int clx_label_overlaps(const int32_t* a, const int32_t* b, long long npix, int nid_a, int nid_b, int capacity,
                                  unsigned long long* keys, unsigned long long* counts, int32_t* info, clx_stream stream) {
  CLX_REQUIRE(a && b && keys && counts && info, "clx_label_overlaps: null pointer");
  CLX_REQUIRE(npix > 0 && npix < (1ll << 32), "clx_label_overlaps: npix must lie in [1, 2^32)");
  CLX_REQUIRE(nid_a >= 1 && nid_a <= (1 << 24), "clx_label_overlaps: nid_a must lie in [1, 2^24]");
  CLX_REQUIRE(nid_b >= 1 && nid_b <= (1 << 24), "clx_label_overlaps: nid_b must lie in [1, 2^24]");
  CLX_REQUIRE(capacity >= 1024 && capacity <= (1 << 28) && (capacity & (capacity - 1)) == 0,
              "clx_label_overlaps: capacity must be a power of two in [1024, 2^28]");
  hipStream_t st = (hipStream_t)stream;
  const ContactsOut o = contacts_out(keys, counts, info, capacity);
  contacts_init<<<(capacity + 255) / 256, 256, 0, st>>>(o, capacity);
  const Tiling t = tiling_for(npix);
  overlaps_kernel<<<t.grid, BLOCK, 0, st>>>(a, b, aligned16(a), aligned16(b), npix, nid_a, nid_b, t.ntiles, t.per_block, o);
  CLX_CHECK_LAUNCH("clx_label_overlaps");
  return CLX_OK;
}

extern "C" int clx_region_clearance(const int32_t* a, const int32_t* b, const int32_t* dist_sq, const int32_t* parent,
                                    long long npix, int nid_a, unsigned long long* out, int32_t* bad, clx_stream stream) {
  CLX_REQUIRE(a && b && dist_sq && parent && out && bad, "clx_region_clearance: null pointer");
  CLX_REQUIRE(npix > 0 && npix < (1ll << 32), "clx_region_clearance: npix must lie in [1, 2^32)");
  CLX_REQUIRE(nid_a >= 1 && nid_a <= (1 << 24), "clx_region_clearance: nid_a must lie in [1, 2^24]");
  hipStream_t st = (hipStream_t)stream;
  launch_table_init<3, 1>(out, bad, nid_a, st);         // word 1 is a minimum
  const Tiling t = tiling_for(npix);
  clearance_kernel<<<t.grid, BLOCK, 0, st>>>(a, b, dist_sq, parent, aligned16(a), aligned16(b), aligned16(dist_sq), npix, nid_a,
                                             t.ntiles, t.per_block, out, bad);
  CLX_CHECK_LAUNCH("clx_region_clearance");
  return CLX_OK;
}
