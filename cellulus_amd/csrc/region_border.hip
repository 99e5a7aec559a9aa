// Intensity on an object's rim (the measure stage's border columns, CellProfiler's *IntensityEdge): a pixel of object i is a
// border pixel if any of its 2·nd face neighbours is not i (another object, background, an out-of-range id or the outside of
// the image; clx_region_perimeter's definition, in 3-D too), and
//   clx_region_border_intensity   per id the border pixels, and over those whose value fits: their number, Σq, the smallest
//                                 and the largest order key and the exact Σq²
// with q clx_region_intensity's quantised value.  The stencil is contacts_kernel's frame (region_contacts.hip) looking both ways: a
// lane holds its four labels, the same four in the rows y - 1 and y + 1 and, for nd = 3, in the slices z - 1 and z + 1 (16-byte
// loads where the pointer is aligned and X, or Y·X, is a multiple of four; 4-byte loads otherwise), and takes the left and the
// right neighbour of its ends from the lanes beside it by shuffle, with a load at the wave's two ends.  A flat index ± X or
// ± Y·X is the neighbour only away from the image's faces, which every pixel tests on its own coordinates: the four pixels
// of a lane may lie in two rows.
// Labels alone decide which pixels are border pixels.  A wave in which no lane has one reads no raw value and emits nothing:
// most waves of a real map lie inside objects or on the background, so the raw channel is read along the rims only, four
// bytes at a time.  The three to five label loads of a trip are independent and in flight together; the kernel prefetches
// no further than that, since what it would prefetch, the raw values, is what the skip avoids.
// Border pixels are few, so nothing is reduced across the wave: a lane walks its four pixels, sums the border pixels of one
// id and adds them to the block's table in LDS keyed by id (find_slot; PROBES occupied slots of other ids: straight to global
// memory), seven words an id, 14 KiB, which the block adds to the output once.  Σq² is below 2^(124 - L) as in
// region_coloc.hip and is kept as (lo, hi) by region_sums.h's add128.  hipcc reports 54 - 58 VGPRs, no spills, and 15360 bytes of LDS:
// eight waves a SIMD.
#include "region_sums.h"

namespace {

constexpr int NW = 7;                   // border pixels, counted ones, Σq, smallest key, largest key, Σq² (lo, hi)
constexpr int W_MIN = 3, W_MAX = 4, W_SQ = 5;

// labels of the 4 pixels from flat index p0 on, p0 possibly negative; outside the image: background
__device__ __forceinline__ void load_labels_at(const int* __restrict__ lab, bool vec, long long p0, long long npix, int* l) {
  if (vec && p0 >= 0 && p0 + PPL <= npix) {
    const i32x4 v = *reinterpret_cast<const i32x4*>(lab + p0);
    l[0] = v[0]; l[1] = v[1]; l[2] = v[2]; l[3] = v[3];
  } else {
#pragma unroll
    for (int k = 0; k < PPL; ++k) l[k] = p0 + k >= 0 && p0 + k < npix ? lab[p0 + k] : 0;
  }
}

// what a lane has summed of one id
struct Rim {
  u64 nb, nc, sq, kmin, kmax;
  i128 sqq;
};

__device__ __forceinline__ void clear(Rim& v) {
  v.nb = 0; v.nc = 0; v.sq = 0; v.kmin = ~0ull; v.kmax = 0ull; v.sqq = 0;
}

__device__ void add_rim(int* keys, u64 (*acc)[SLOTS], u64* __restrict__ out, int label, const Rim& v) {
  const int slot = find_slot(keys, label);
  if (slot >= 0) {
    atomicAdd(&acc[0][slot], v.nb);
    if (v.nc) {
      atomicAdd(&acc[1][slot], v.nc);
      if (v.sq) atomicAdd(&acc[2][slot], v.sq);
      atomicMin(&acc[W_MIN][slot], v.kmin);
      atomicMax(&acc[W_MAX][slot], v.kmax);
      add128(&acc[W_SQ][slot], &acc[W_SQ + 1][slot], v.sqq);
    }
  } else {
    u64* o = out + (size_t)label * NW;
    atomicAdd(o + 0, v.nb);
    if (v.nc) {
      atomicAdd(o + 1, v.nc);
      if (v.sq) atomicAdd(o + 2, v.sq);
      if (v.kmin < o[W_MIN]) atomicMin(o + W_MIN, v.kmin);       // the plain reads only filter
      if (v.kmax > o[W_MAX]) atomicMax(o + W_MAX, v.kmax);
      add128(o + W_SQ, o + W_SQ + 1, v.sqq);
    }
  }
}

struct BorderArgs {
  const int* lab;
  long long npix, plane, ntiles, tiles_per_block, bound;
  int vec, vec_y, vec_z, zfaces;
  int Z, Y, X, nid, shift;
  u64* out;
  int* bad;
};

template <typename T>
__global__ __launch_bounds__(BLOCK) void border_kernel(BorderArgs a, const T* __restrict__ raw) {
  __shared__ int keys[SLOTS];
  __shared__ u64 acc[NW][SLOTS];
  for (int s = threadIdx.x; s < SLOTS; s += BLOCK) {
    keys[s] = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) acc[w][s] = w == W_MIN ? ~0ull : 0ull;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const Tiles tiles = block_tiles(a.ntiles, a.tiles_per_block);
  int any_bad = 0;
  for (long long t = tiles.t0; t < tiles.t1; ++t) {
    const long long p0 = lane_pixel(t);
    int l[PPL], n[PPL], s[PPL], u[PPL], d[PPL];         // own pixels; the rows y - 1 and y + 1; the slices z - 1 and z + 1
    load_labels(a.lab, a.vec != 0, p0, a.npix, l);
    if (clamp_labels(l, a.nid)) any_bad |= BAD_LABEL;
    load_labels_at(a.lab, a.vec_y != 0, p0 - a.X, a.npix, n);
    load_labels_at(a.lab, a.vec_y != 0, p0 + a.X, a.npix, s);
    clamp_labels(n, a.nid);
    clamp_labels(s, a.nid);
    if (a.zfaces) {
      load_labels_at(a.lab, a.vec_z != 0, p0 - a.plane, a.npix, u);
      load_labels_at(a.lab, a.vec_z != 0, p0 + a.plane, a.npix, d);
      clamp_labels(u, a.nid);
      clamp_labels(d, a.nid);
    } else {
#pragma unroll
      for (int k = 0; k < PPL; ++k) { u[k] = l[k]; d[k] = l[k]; }
    }
    // the -x neighbour of the lane's first pixel and the +x neighbour of its last: the lanes beside it, or a load at the
    // wave's two ends (which are a tile's and a block's ends too)
    int left = __shfl_up(l[PPL - 1], 1), right = __shfl_down(l[0], 1);
    if (lane == 0) {
      left = p0 > 0 && p0 <= a.npix ? a.lab[p0 - 1] : 0;
      if ((unsigned)left >= (unsigned)a.nid) left = 0;
    }
    if (lane == 63) {
      right = p0 + PPL < a.npix ? a.lab[p0 + PPL] : 0;
      if ((unsigned)right >= (unsigned)a.nid) right = 0;
    }
    Pixel p = pixel_at(p0, a.npix, a.Y, a.X).p;

    bool border[PPL];
    bool any = false;
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      const int c = l[k];                               // 0 past the end of the image
      const int lo = k == 0 ? left : l[(k + PPL - 1) & (PPL - 1)], hi = k == PPL - 1 ? right : l[(k + 1) & (PPL - 1)];
      bool b = p.x == 0 || lo != c || p.x == a.X - 1 || hi != c || p.y == 0 || n[k] != c || p.y == a.Y - 1 || s[k] != c;
      if (a.zfaces) b = b || p.z == 0 || u[k] != c || p.z == a.Z - 1 || d[k] != c;
      border[k] = c > 0 && b;
      any |= border[k];
      p = next_pixel(p, a.Y, a.X);
    }
    if (__ballot(any) == 0ull) continue;                // an interior or background wave: no raw value is read
    if (!any) continue;

    int cur = 0;
    Rim v;
    clear(v);
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      if (!border[k]) continue;
      if (l[k] != cur) {
        if (cur > 0) add_rim(keys, acc, a.out, cur, v);
        cur = l[k];
        clear(v);
      }
      v.nb += 1;
      const T value = raw[p0 + k];                      // a border pixel lies inside the image
      long long q;
      if (quantise<T>(value, a.shift, a.bound, &q)) {
        const u64 key = order_key(value);
        v.nc += 1;
        v.sq += (u64)q;
        v.kmin = key < v.kmin ? key : v.kmin;
        v.kmax = key > v.kmax ? key : v.kmax;
        v.sqq += (i128)q * q;
      } else {
        any_bad |= BAD_VALUE;                           // the pixel stays in word 0 only
      }
    }
    if (cur > 0) add_rim(keys, acc, a.out, cur, v);
  }
  if (any_bad) atomicOr(a.bad, any_bad);
  __syncthreads();

  for (int s = threadIdx.x; s < SLOTS; s += BLOCK) {
    const int label = keys[s];
    if (label == 0) continue;
    u64* o = a.out + (size_t)label * NW;
    if (acc[0][s]) atomicAdd(o + 0, acc[0][s]);
    if (acc[1][s]) {
      atomicAdd(o + 1, acc[1][s]);
      if (acc[2][s]) atomicAdd(o + 2, acc[2][s]);
      if (acc[W_MIN][s] < o[W_MIN]) atomicMin(o + W_MIN, acc[W_MIN][s]);
      if (acc[W_MAX][s] > o[W_MAX]) atomicMax(o + W_MAX, acc[W_MAX][s]);
      add128(o + W_SQ, o + W_SQ + 1, (i128)(((unsigned __int128)acc[W_SQ + 1][s] << 64) | acc[W_SQ][s]));
    }
  }
}

}  // namespace

extern "C" int clx_region_border_intensity(const int32_t* labels, const void* raw, int raw_type, int nd, int Z, int Y, int X,
                                           int nid, int shift, unsigned long long* out, int32_t* bad, clx_stream stream) {
  const char* who = "clx_region_border_intensity";
  CLX_REQUIRE(labels && raw && out && bad, "%s: null pointer", who);
  CLX_REQUIRE(raw_type >= CLX_RAW_F32 && raw_type <= CLX_RAW_I32, "%s: raw_type must be 0 (f32), 1 (f64) or 2 (i32)", who);
  CLX_REQUIRE_MAP(npix, who, nd, Z, Y, X, 32);
  CLX_REQUIRE(nid >= 1 && nid <= (1 << 24), "%s: nid must lie in [1, 2^24]", who);
  hipStream_t st = (hipStream_t)stream;
  const Tiling t = tiling_for(npix);
  BorderArgs a;
  a.lab = labels;
  a.npix = npix; a.plane = (long long)Y * X; a.ntiles = t.ntiles; a.tiles_per_block = t.per_block;
  a.bound = value_bound(npix);
  a.vec = aligned16(labels); a.vec_y = a.vec && (X & 3) == 0; a.vec_z = a.vec && (a.plane & 3) == 0;
  a.zfaces = nd == 3;
  a.Z = Z; a.Y = Y; a.X = X; a.nid = nid; a.shift = shift;
  a.out = out; a.bad = bad;
  launch_table_init<NW, W_MIN>(out, bad, nid, st);
  launch_for_raw(raw_type, [&](auto v) { border_kernel<decltype(v)><<<t.grid, BLOCK, 0, st>>>(a, (const decltype(v)*)raw); });
  CLX_CHECK_LAUNCH(who);
  return CLX_OK;
}
