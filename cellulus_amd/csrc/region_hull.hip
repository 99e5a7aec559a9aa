// "measure" stage, clx_region_hull: the convex hull of every object's pixel corners (area, vertices, Feret diameters).
// Convex hull (clx.h has the definitions): an object is the union of its pixels as closed unit squares, so its hull is
// that of the pixels' corner lattice points, and the hull of a set is the hull of the extreme points of its rows.
//   hull_span_kernel    the map pass, in moments_kernel's frame: per (object, row) of the object's bounding box the
//                       smallest and the largest x that carries the id.  A run of one id in one row costs one atomicMin and
//                       one atomicMax, whatever its length; neither returns a value, so a lane waits for its box only.
//   hull_object_kernel  a wave per object.  First a lane per (slice, side) runs Andrew's monotone chain over the rows'
//                       corner points (on lattice line y' the left chain has min(xmin[y'-1], xmin[y']), the right one
//                       max(xmax[y'-1], xmax[y']) + 1; the rows are sorted by y already), keeping strict vertices only.
//                       Then the wave forms A2 and NV, F2 over all vertex pairs and (C, L2) over all edge x vertex pairs.
// The rows of object i start at row_base[i]; row (z, y) is row_base[i] + (z - zmin) (ymax - ymin + 1) + (y - ymin).  The
// bounding boxes and row_base come from the caller and are not trusted: hull_box checks a box against the image and the
// row count before any index is formed from it.
#include "region_scan.h"

namespace {

struct HullIn {
  const int* bbox;
  const long long* row_base;
  long long rows;
  int Z, Y, X;
};

// the workspace: 12 ints a row.  Chain `side` (0 left, 1 right) of the slice whose first row is r keeps its points
// (y, x) from point index side * 2 * rows + 2 * r on: a slice of h rows has at most h + 1 <= 2 h points a chain.
struct HullWs {
  int* xmin;                            // [rows]     0x7fffffff: no pixel of the id in the row
  int* xmax;                            // [rows]     -1: the same
  int* cnt;                             // [rows][2]  points of the two chains, at a slice's first row
  int* pts;                             // [4 * rows][2]
};
constexpr int HULL_WS_INTS = 12;
constexpr int HULL_BATCH = 8;           // rows a chain loads at once
constexpr int HULL_MAX_GRID = 4096;     // hull_span_kernel has no table to flush at a block's end: more, shorter blocks hide its latency

// b: the box of `id`, *base: its first row; false: absent, outside the image, or its rows do not lie in [0, rows)
__device__ __forceinline__ bool hull_box(const HullIn& in, int id, int* b, long long* base) {
#pragma unroll
  for (int k = 0; k < 6; ++k) b[k] = in.bbox[(size_t)id * 6 + k];
  if (b[0] < 0 || b[1] < 0 || b[2] < 0 || b[3] < b[0] || b[4] < b[1] || b[5] < b[2] || b[3] >= in.Z || b[4] >= in.Y || b[5] >= in.X)
    return false;
  const long long rb = in.row_base[id];
  const long long n = (long long)(b[3] - b[0] + 1) * (b[4] - b[1] + 1);        // <= Z * Y < 2^32
  if (rb < 0 || rb > in.rows - n) return false;
  *base = rb;
  return true;
}

// pixels x0 .. x1 of `label` in row (z, y); false: the id's box does not contain them (nothing is written)
__device__ bool add_span(const HullIn& in, const HullWs& w, int label, int z, int y, int x0, int x1) {
  int b[6];
  long long base;
  if (!hull_box(in, label, b, &base) || z < b[0] || z > b[3] || y < b[1] || y > b[4] || x0 < b[2] || x1 > b[5]) return false;
  const long long r = base + (long long)(z - b[0]) * (b[4] - b[1] + 1) + (y - b[1]);
  atomicMin(w.xmin + r, x0);
  atomicMax(w.xmax + r, x1);
  return true;
}

__global__ void hull_init(HullWs w, long long rows, int* __restrict__ bad) {
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 == 0) *bad = 0;
  for (long long i = i0; i < rows; i += (long long)gridDim.x * blockDim.x) {
    w.xmin[i] = 0x7fffffff;
    w.xmax[i] = -1;
  }
}

__global__ __launch_bounds__(BLOCK) void hull_span_kernel(const int* __restrict__ lab, int vec, long long npix, int nid,
                                                          long long ntiles, long long tiles_per_block, HullIn in, HullWs w,
                                                          int* __restrict__ bad) {
  const int lane = threadIdx.x & 63;
  const int Y = in.Y, X = in.X;
  const Tiles tiles = block_tiles(ntiles, tiles_per_block);
  int any_bad = 0;
  for (long long t = tiles.t0; t < tiles.t1; ++t) {
    const long long p0 = lane_pixel(t);
    int l[PPL];
    load_labels(lab, vec != 0, p0, npix, l);
    if (clamp_labels(l, nid)) any_bad |= 1;
    if (__ballot((l[0] | l[1] | l[2] | l[3]) != 0) == 0ull) continue;   // a wave of background
    const PixelInRow at = pixel_at(p0, npix, Y, X);
    Pixel p = at.p;

    // a run never continues into the next image row
    const bool uni = l[0] > 0 && l[0] == l[1] && l[1] == l[2] && l[2] == l[3] && p.x + PPL <= X;
    const Heads h = run_heads(uni, l, at.row, lane);
    if (uni) {
      if (h.head && !add_span(in, w, l[0], p.z, p.y, p.x, p.x + PPL * run_lanes(h.heads, lane) - 1)) any_bad |= 2;
    } else {
      int cur = 0, n = 0, cz = 0, cy = 0, cx = 0;
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        if (l[k] != cur || p.x == 0) {
          if (cur > 0 && !add_span(in, w, cur, cz, cy, cx, cx + n - 1)) any_bad |= 2;
          cur = l[k]; n = 0; cz = p.z; cy = p.y; cx = p.x;
        }
        ++n;
        p = next_pixel(p, Y, X);
      }
      if (cur > 0 && !add_span(in, w, cur, cz, cy, cx, cx + n - 1)) any_bad |= 2;
    }
  }
  if (any_bad) atomicOr(bad, any_bad);
}

// is the width c_a / sqrt(l_a) the better (smaller; at equal widths the one over the shorter edge)?  l == 0: no candidate.
// c <= 2^31 (twice the area of a triangle inside a box of (Y+1)(X+1) <= 2^31 lattice points), so c^2 fits 64 bits; the
// products c_a^2 l_b and c_b^2 l_a are compared exactly as 128-bit numbers.
__device__ __forceinline__ bool narrower(u64 ca, u64 la, u64 cb, u64 lb) {
  if (la == 0 || lb == 0) return la != 0;
  const u64 qa = ca * ca, qb = cb * cb;
  const u64 ah = __umul64hi(qa, lb), al = qa * lb, bh = __umul64hi(qb, la), bl = qb * la;
  if (ah != bh) return ah < bh;
  if (al != bl) return al < bl;
  return la < lb;
}

__global__ __launch_bounds__(BLOCK) void hull_object_kernel(HullIn in, HullWs w, int nd, int nid, long long* __restrict__ hull) {
  const int lane = threadIdx.x & 63;
  const long long idl = (long long)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
  const int id = idl < nid ? (int)idl : 0;
  int b[6];
  long long base = 0;
  const bool valid = id > 0 && hull_box(in, id, b, &base);
  const long long S = valid ? b[3] - b[0] + 1 : 0;      // slices
  const long long h = valid ? b[4] - b[1] + 1 : 0;      // rows a slice
  const long long pts_side = 2 * in.rows;               // points of all left chains

  // a lane per chain: the points are met in the order of y, so the stack is the chain
  for (long long c = lane; c < 2 * S; c += 64) {
    const int side = (int)(c & 1);
    const long long r0 = base + (c >> 1) * h;
    const int* span = side ? w.xmax + r0 : w.xmin + r0;
    const int none = side ? -1 : 0x7fffffff;
    int* st = w.pts + 2 * (side * pts_side + 2 * r0);
    int n = 0, prev = none;
    long long ay = 0, ax = 0, by = 0, bx = 0;           // the two points on top of the stack, st[n - 2] and st[n - 1]
    for (long long k0 = 0; k0 <= h; k0 += HULL_BATCH) {
      // the rows of a batch are loaded before the first is looked at: one round of memory latency per batch, and a
      // line that pops nothing touches memory with its store only
      int s[HULL_BATCH];
#pragma unroll
      for (int j = 0; j < HULL_BATCH; ++j) s[j] = k0 + j < h ? span[k0 + j] : none;
#pragma unroll
      for (int j = 0; j < HULL_BATCH; ++j) {
        if (k0 + j > h) continue;                       // lattice line ymin + k, between rows k - 1 and k, k = k0 + j <= h
        const int cur = s[j];
        int px = side ? (prev > cur ? prev : cur) : (prev < cur ? prev : cur);
        prev = cur;
        if (px == none) continue;                       // both rows are empty: no corner on this line
        px += side;
        const int py = b[1] + (int)(k0 + j);
        while (n >= 2) {
          const long long cross = (by - ay) * (px - ax) - (bx - ax) * (py - ay);    // coordinates <= 2^30: below 2^61
          if (side ? cross < 0 : cross > 0) break;      // the middle point lies strictly outside the line a -> p
          --n;
          by = ay;
          bx = ax;
          if (n >= 2) { ay = st[2 * n - 4]; ax = st[2 * n - 3]; }
        }
        st[2 * n] = py;
        st[2 * n + 1] = px;
        ++n;
        ay = by; ax = bx;
        by = py; bx = px;
      }
    }
    w.cnt[2 * r0 + side] = n;
  }
  __syncthreads();                                      // the chains are in global memory for the whole wave
  if (idl >= nid) return;
  if (!valid) {
    if (lane < 5) hull[(size_t)id * 5 + lane] = 0;
    return;
  }

  // F2 over all pairs of chains (ca <= cb) and all pairs of their points; in 3-D a point of slice s stands at s and s + 1
  u64 f2 = 0;
  for (long long ca = 0; ca < 2 * S; ++ca) {
    const long long ra = base + (ca >> 1) * h;
    const int na = w.cnt[2 * ra + (ca & 1)];
    if (na == 0) continue;
    const int* pa = w.pts + 2 * ((ca & 1) * pts_side + 2 * ra);
    for (long long cb = ca; cb < 2 * S; ++cb) {
      const long long rb = base + (cb >> 1) * h;
      const int nb = w.cnt[2 * rb + (cb & 1)];
      if (nb == 0) continue;
      const int* pb = w.pts + 2 * ((cb & 1) * pts_side + 2 * rb);
      const long long dz = nd == 3 ? (cb >> 1) - (ca >> 1) + 1 : 0;
      const long long npairs = (long long)na * nb;
      for (long long t = lane; t < npairs; t += 64) {
        const long long ia = t / nb, ib = t - ia * nb;
        const long long dy = (long long)pa[2 * ia] - pb[2 * ib], dx = (long long)pa[2 * ia + 1] - pb[2 * ib + 1];
        const u64 d2 = (u64)(dy * dy + dx * dx + dz * dz);      // extents < 2^30: below 2^62
        f2 = d2 > f2 ? d2 : f2;
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const u64 o = __shfl_down(f2, d);
    f2 = o > f2 ? o : f2;
  }

  long long a2 = 0, nv = 0;
  u64 bc = 0, bl = 0;
  if (nd == 2) {
    // the polygon: the left chain downwards, then the right chain upwards.  The four chain ends are vertices (extreme on
    // the first / last lattice line) and the chains share no point (right x > left x on every line): NV = nL + nR.
    const int nl = w.cnt[2 * base], nr = w.cnt[2 * base + 1];
    const int* pl = w.pts + 2 * (2 * base);
    const int* pr = w.pts + 2 * (pts_side + 2 * base);
    const int V = nl + nr;
    nv = V;
    auto vertex = [&](int k, long long& vy, long long& vx) {
      const int* p = k < nl ? pl + 2 * k : pr + 2 * (nr - 1 - (k - nl));
      vy = p[0];
      vx = p[1];
    };
    if (V > 0) {
      long long oy, ox;
      vertex(0, oy, ox);
      for (int e = lane; e < V; e += 64) {
        long long ay, ax, by, bx;
        vertex(e, ay, ax);
        vertex(e + 1 < V ? e + 1 : 0, by, bx);
        a2 += (ay - oy) * (bx - ox) - (ax - ox) * (by - oy);    // shoelace about vertex 0: every term within the box
        const long long ey = by - ay, ex = bx - ax;
        u64 c = 0;
        for (int k = 0; k < V; ++k) {
          long long vy, vx;
          vertex(k, vy, vx);
          const long long cr = ey * (vx - ax) - ex * (vy - ay);
          const u64 m = (u64)(cr < 0 ? -cr : cr);
          c = m > c ? m : c;
        }
        const u64 len = (u64)(ey * ey + ex * ex);
        if (narrower(c, len, bc, bl)) { bc = c; bl = len; }
      }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      a2 += __shfl_down(a2, d);
      const u64 oc = __shfl_down(bc, d), ol = __shfl_down(bl, d);
      if (narrower(oc, ol, bc, bl)) { bc = oc; bl = ol; }
    }
    a2 = a2 < 0 ? -a2 : a2;
  }
  if (lane == 0) {
    long long* o = hull + (size_t)id * 5;
    o[0] = a2; o[1] = nv; o[2] = (long long)f2; o[3] = (long long)bc; o[4] = (long long)bl;
  }
}

}  // namespace

extern "C" size_t clx_region_hull_workspace(long long rows) {
  if (rows < 0 || rows > (1ll << 56)) return 0;
  const size_t bytes = (size_t)rows * HULL_WS_INTS * sizeof(int);
  return bytes < 64 ? 64 : bytes;
}

extern "C" int clx_region_hull(const int32_t* labels, int nd, int Z, int Y, int X, int nid, const int32_t* bbox,
                               const long long* row_base, long long rows, void* workspace, size_t workspace_bytes,
                               long long* hull, int32_t* bad, clx_stream stream) {
  CLX_REQUIRE(labels && bbox && row_base && workspace && hull && bad, "clx_region_hull: null pointer");
  CLX_REQUIRE_MAP(npix, "clx_region_hull", nd, Z, Y, X, 32);
  CLX_REQUIRE(Z < (1 << 30) && Y < (1 << 30) && X < (1 << 30), "clx_region_hull: Z, Y and X must be below 2^30 (F2 is 64-bit)");
  CLX_REQUIRE(nid >= 1 && nid <= (1 << 24), "clx_region_hull: nid must lie in [1, 2^24]");
  CLX_REQUIRE(nd == 3 || ((long long)Y + 1) * ((long long)X + 1) <= (1ll << 31),
              "clx_region_hull: nd == 2 needs (Y + 1) * (X + 1) <= 2^31 (C^2 is 64-bit)");
  // an id has at most Z * Y rows
  CLX_REQUIRE(rows >= 0 && rows <= (long long)(nid - 1) * Z * Y, "clx_region_hull: rows must lie in [0, (nid - 1) * Z * Y]");
  CLX_REQUIRE(workspace_bytes >= clx_region_hull_workspace(rows),
              "clx_region_hull: workspace_bytes is below clx_region_hull_workspace(rows)");
  CLX_REQUIRE(((uintptr_t)workspace & 7) == 0, "clx_region_hull: workspace must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  int* ws = (int*)workspace;
  const HullWs w = {ws, ws + rows, ws + 2 * rows, ws + 4 * rows};
  const HullIn in = {bbox, row_base, rows, Z, Y, X};
  const long long init_blocks = (rows + 255) / 256;
  hull_init<<<(int)(init_blocks < 1 ? 1 : (init_blocks < 65536 ? init_blocks : 65536)), 256, 0, st>>>(w, rows, bad);
  const Tiling t = tiling_for(npix, HULL_MAX_GRID);
  hull_span_kernel<<<t.grid, BLOCK, 0, st>>>(labels, aligned16(labels), npix, nid, t.ntiles, t.per_block, in, w, bad);
  hull_object_kernel<<<(nid + BLOCK / 64 - 1) / (BLOCK / 64), BLOCK, 0, st>>>(in, w, nd, nid, hull);
  CLX_CHECK_LAUNCH("clx_region_hull");
  return CLX_OK;
}
