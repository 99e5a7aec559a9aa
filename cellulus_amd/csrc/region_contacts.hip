// "measure" stage, clx_region_contacts: the faces between pixels of different ids, per id pair (a stencil).
// Contacts: every face (connectivity 1) between two pixels of different ids counts once for the pair (lo, hi); the
// outside of the image is id 0.  A pixel owns its forward faces (+x, +y, +z; past the last column / row / slice the
// neighbour is 0) and, in the first column / row / slice, the backward face to 0.  The output is a SET of pairs of
// unknown size: an open-addressing table in global memory keyed by (lo << 32) | hi (never 0, as hi >= 1), filled through
// a block-private table in LDS that is flushed once (pair_table.h, shared with label_overlap.hip).  A lane whose pixels
// and forward neighbours all carry one id away from the image edge has nothing to emit; a wave of such lanes skips the rest
// of the trip.
#include "pair_table.h"

namespace {

// a lane's faces in the order it meets them; equal pairs in a row (a horizontal edge gives four) become one add
struct PairRun {
  u64 key;
  unsigned int n;
};
__device__ __forceinline__ void face(PairRun& r, u64* lkeys, u64* lcnt, const ContactsOut& o, int a, int b) {
  if (a == b) return;
  const u64 key = a < b ? ((u64)(unsigned int)a << 32) | (unsigned int)b : ((u64)(unsigned int)b << 32) | (unsigned int)a;
  if (key == r.key) { ++r.n; return; }
  if (r.n) add_pair(lkeys, lcnt, o, r.key, r.n);
  r.key = key;
  r.n = 1;
}

__global__ __launch_bounds__(BLOCK) void contacts_kernel(const int* __restrict__ lab, int vec, int vec_y, int vec_z, int zfaces,
                                                         long long npix, int Z, int Y, int X, int nid, long long ntiles,
                                                         long long tiles_per_block, ContactsOut o) {
  __shared__ u64 lkeys[CSLOTS];
  __shared__ u64 lcnt[CSLOTS];
  for (int s = threadIdx.x; s < CSLOTS; s += BLOCK) { lkeys[s] = 0; lcnt[s] = 0; }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const long long plane = (long long)Y * X;
  const long long t0 = (long long)blockIdx.x * tiles_per_block;
  const long long t1 = t0 + tiles_per_block < ntiles ? t0 + tiles_per_block : ntiles;
  bool any_bad = false;
  for (long long t = t0; t < t1; ++t) {
    const long long p0 = t * TILE + (long long)threadIdx.x * PPL;
    int l[PPL], d[PPL], u[PPL];                         // own pixels, one row down, one slice down (flat index + X, + Y*X)
    load_labels(lab, vec != 0, p0, npix, l);
    any_bad |= clamp_labels(l, nid);
    load_labels(lab, vec_y != 0, p0 + X, npix, d);
    clamp_labels(d, nid);
    if (zfaces) {
      load_labels(lab, vec_z != 0, p0 + plane, npix, u);
      clamp_labels(u, nid);
    } else {
#pragma unroll
      for (int k = 0; k < PPL; ++k) u[k] = l[k];
    }
    // the +x neighbour of the lane's last pixel: the next lane's first, or a load for the wave's last lane
    int right = __shfl_down(l[0], 1);
    if (lane == 63) {
      right = p0 + PPL < npix ? lab[p0 + PPL] : 0;
      if ((unsigned)right >= (unsigned)nid) right = 0;
    }
    // npix < 2^32: 32-bit divisions
    const unsigned int pu = p0 < npix ? (unsigned int)p0 : 0u;
    const unsigned int r = pu / (unsigned int)X;
    int x = (int)(pu - r * (unsigned int)X);
    int z = (int)(r / (unsigned int)Y);
    int y = (int)(r - (unsigned int)z * (unsigned int)Y);

    // away from every image edge the stored neighbours are the real ones: nothing to emit if they all equal l[0]
    const bool interior = p0 + PPL <= npix && x > 0 && x + PPL < X && y > 0 && y + 1 < Y && (!zfaces || (z > 0 && z + 1 < Z));
    int diff = right ^ l[0];
#pragma unroll
    for (int k = 0; k < PPL; ++k) diff |= (l[k] ^ l[0]) | (d[k] ^ l[0]) | (u[k] ^ l[0]);
    const bool noisy = p0 < npix && (!interior || diff != 0);
    if (__ballot(noisy) == 0ull) continue;
    if (!noisy) continue;

    // per pixel: is it in the image, and on which edges
    bool in[PPL], x_lo[PPL], x_hi[PPL], y_lo[PPL], y_hi[PPL], z_lo[PPL], z_hi[PPL];
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      in[k] = p0 + k < npix;
      x_lo[k] = x == 0; x_hi[k] = x == X - 1;
      y_lo[k] = y == 0; y_hi[k] = y == Y - 1;
      z_lo[k] = z == 0; z_hi[k] = z == Z - 1;
      if (++x == X) { x = 0; if (++y == Y) { y = 0; ++z; } }
    }
    PairRun run = {0ull, 0u};
#pragma unroll
    for (int k = 0; k < PPL; ++k)
      if (in[k]) face(run, lkeys, lcnt, o, l[k], y_hi[k] ? 0 : d[k]);
#pragma unroll
    for (int k = 0; k < PPL; ++k)
      if (in[k] && y_lo[k]) face(run, lkeys, lcnt, o, l[k], 0);
    if (zfaces) {
#pragma unroll
      for (int k = 0; k < PPL; ++k)
        if (in[k]) face(run, lkeys, lcnt, o, l[k], z_hi[k] ? 0 : u[k]);
#pragma unroll
      for (int k = 0; k < PPL; ++k)
        if (in[k] && z_lo[k]) face(run, lkeys, lcnt, o, l[k], 0);
    }
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      if (!in[k]) continue;
      if (x_lo[k]) face(run, lkeys, lcnt, o, l[k], 0);
      face(run, lkeys, lcnt, o, l[k], x_hi[k] ? 0 : (k < PPL - 1 ? l[(k + 1) & (PPL - 1)] : right));
    }
    if (run.n) add_pair(lkeys, lcnt, o, run.key, run.n);
  }
  if (any_bad) atomicOr(o.info, 1);
  __syncthreads();

  for (int s = threadIdx.x; s < CSLOTS; s += BLOCK)
    if (lkeys[s]) pair_to_global(o, lkeys[s], lcnt[s], mix64(lkeys[s]));
}

}  // namespace

extern "C" int clx_region_contacts(const int32_t* labels, int nd, int Z, int Y, int X, int nid, int capacity,
                                   unsigned long long* keys, unsigned long long* counts, int32_t* info, clx_stream stream) {
  CLX_REQUIRE(labels && keys && counts && info, "clx_region_contacts: null pointer");
  CLX_REQUIRE_MAP(npix, "clx_region_contacts", nd, Z, Y, X, 32);
  CLX_REQUIRE(nid >= 1 && nid <= (1 << 24), "clx_region_contacts: nid must lie in [1, 2^24]");
  CLX_REQUIRE(capacity >= 1024 && capacity <= (1 << 28) && (capacity & (capacity - 1)) == 0,
              "clx_region_contacts: capacity must be a power of two in [1024, 2^28]");
  hipStream_t st = (hipStream_t)stream;
  const ContactsOut o = contacts_out(keys, counts, info, capacity);
  contacts_init<<<(capacity + 255) / 256, 256, 0, st>>>(o, capacity);
  const Tiling t = tiling_for(npix);
  const int vec = aligned16(labels);
  contacts_kernel<<<t.grid, BLOCK, 0, st>>>(labels, vec, vec && (X & 3) == 0, vec && (((long long)Y * X) & 3) == 0, nd == 3, npix,
                                            Z, Y, X, nid, t.ntiles, t.per_block, o);
  CLX_CHECK_LAUNCH("clx_region_contacts");
  return CLX_OK;
}
