// The skeleton stage's branch graph: the links of a (thinned) label map contracted to nodes and branches.
//   clx_skeleton_graph   one row per branch and per node, a map of the branches and nodes, and the map with its short spurs
//                        pruned (one round); include/clx.h has the definitions
//
// The pixel graph is the census's (skeleton_links.h): a pixel's links and degree come from its eight neighbours, and its KIND
// from the degree -- isolated 0, end 1, path 2, junction >= 3.  Nothing about a pixel is stored: a kernel that needs the kind
// of a linked neighbour takes it from the labels again (object pixels are a few per cent of a thinned map).  Path pixels are
// united over the links between two of them and junction pixels over the links between two of them by the lock-free union-find
// of union_find.h over raster indices; a set's root is its smallest pixel: a branch's `first`, a node's id.  The passes walk
// the map segment by segment (segments.h has the frame).  Six plain launches on the stream, no host synchronisation, and
// between two of them nothing but the kernel boundary:
//   1 classify  parent[i] = i on path and junction pixels, -1 elsewhere; these are the only possible roots: their attributes
//               are cleared here
//   2 link      a path pixel unions with the path pixels, a junction pixel with the junction pixels it has a link to; a link is
//               taken once, by the pixel that has it towards E, S, SE or SW
//   3 flatten   parent[i] = find(i)
//   4 reduce    a path pixel adds to its root: 1 pixel, its links (one between two path pixels once, by its owner; a TERMINAL
//               link, to a pixel that is no path pixel, by the path pixel), the terminal pixel to the smallest and the largest
//               terminal of the branch, and its dist_sq.  A junction pixel adds to its root: 1 pixel, its links to pixels that
//               are no junction pixels, and the links to junction pixels that it owns
//   5 emit      the pixel that is its own root appends its row; an end or isolated pixel appends its node row, an end pixel
//               whose link leads to a junction pixel or to a larger end pixel the row of that DIRECT branch.  A wave counts the
//               rows of 8 segments and reserves them with one add to info[0] and one to info[1].  The root of a pruned spur
//               sets the PRUNED bit of its pixel count
//   6 write     branch_map and out; a path pixel reads the PRUNED bit at its root, an end pixel finds its branch through its
//               single link
// A path pixel has two links, so a branch has two terminal links or none (a cycle): the smallest and the largest terminal
// pixel are all its terminals.
// Correctness across blocks and XCDs rests on the values returned by atomics and on kernel boundaries alone (union_find.h's
// rule): no block waits for another, every loop ends because a parent strictly decreases.  Integer atomics only; ids are 32-bit
// raster indices (npix < 2^31); values of the map are compared, never an index.  Everything the call writes is a function of
// the input but the ORDER of the rows (the host sorts them by `first`).
#include <limits.h>
#include "segments.h"
#include "skeleton_links.h"
#include "union_find.h"

namespace {

constexpr int GRAPH_MAX_GRID = 2048;            // blocks of launches 1 to 4 and 6: 8192 waves; a wave takes the segments w, w + 8192, ...
constexpr int EMIT_SEGS = 8;                    // segments a wave of launch 5 takes a trip
constexpr int EMIT_MAX_GRID = 1024;             // blocks of launch 5: 32768 segments a trip
constexpr unsigned int PRUNED = 0x80000000u;    // of pixels[root] of a branch; the low 31 bits are the count (npix < 2^31)
constexpr int BRANCH_WORDS = 13, NODE_WORDS = 7;
constexpr int ISOLATED = 0, END = 1, PATH = 2, JUNCTION = 3;    // a pixel's kind; ISOLATED, END and JUNCTION are a node's too
constexpr int END_END = 0, SPUR = 1, JUNCTION_JUNCTION = 2, CYCLE = 3;

struct Planes {                                 // the workspace: planes over raster indices, all but `parent` read at roots only
  u64* sum;                                     // branch: the sum of dist_sq over the path pixels
  int* parent;
  int* pixels;                                  // branch: path pixels | PRUNED            node: junction pixels
  int* face;                                    // branch: face links                      node: links out
  int* diag;                                    // branch: diagonal links                  node: inner face links
  int* lo;                                      // branch: the smallest terminal pixel     node: inner diagonal links
  int* hi;                                      // branch: the largest terminal pixel
  int* mn;                                      // branch: the extremes of dist_sq
  int* mx;
};

// the neighbour of p in direction k; it lies in the slice wherever p has a link in that direction
__device__ __forceinline__ SegPos towards(const SegPos& p, const Segments& s, int k) {
  return {p.i + (long long)LINK_DY[k] * s.X + LINK_DX[k], p.row + LINK_DY[k], p.x + LINK_DX[k], p.y + LINK_DY[k], p.z, true};
}
__device__ __forceinline__ SegPos pos_at(int i, const Segments& s) {
  const int row = i / s.X;
  return {(long long)i, (long long)row, i - row * s.X, row % s.Y, row / s.Y, true};
}

__device__ __forceinline__ int kind_of(const Links& l) {
  const int degree = l.degree();
  return degree >= 3 ? JUNCTION : degree;
}
__device__ __forceinline__ int kind_at(const int* __restrict__ lab, const Segments& s, const SegPos& p, int v) {
  return kind_of(links_at(lab, p.i, p.x, p.y, s.Y, s.X, v));
}

// face + sqrt(2) diag < limit_q10 / 1024, in integers: limit_q10 < 2^30, so both squares lie below 2^61
__device__ __forceinline__ bool spur_pruned(long long face, long long diag, long long limit_q10) {
  const long long F = 1024 * face, D = 1024 * diag, T = limit_q10;
  if (F >= T || D >= T) return false;
  return 2 * D * D < (T - F) * (T - F);
}

__global__ __launch_bounds__(BLOCK) void graph_classify(const int* __restrict__ lab, Planes a, Segments s) {
  const int lane = threadIdx.x & 63;
  FOR_EACH_SEGMENT(w, s) {
    const SegPos p = seg_pos(w, s, lane);
    if (!p.valid) continue;
    const int v = lab[p.i];
    const int kind = v != 0 ? kind_at(lab, s, p, v) : ISOLATED;
    const bool root = v != 0 && kind >= PATH;
    a.parent[p.i] = root ? (int)p.i : -1;
    if (root) {
      a.pixels[p.i] = a.face[p.i] = a.diag[p.i] = 0;
      a.lo[p.i] = kind == PATH ? INT_MAX : 0;
      a.hi[p.i] = -1;
      a.sum[p.i] = 0ull;
      a.mn[p.i] = CLX_DIST_INF;
      a.mx[p.i] = -1;
    }
  }
}

__global__ __launch_bounds__(BLOCK) void graph_link(const int* __restrict__ lab, int* parent, Segments s) {
  const int lane = threadIdx.x & 63;
  FOR_EACH_SEGMENT(w, s) {
    const SegPos p = seg_pos(w, s, lane);
    const int v = p.valid ? lab[p.i] : 0;
    if (v == 0) continue;
    const Links l = links_at(lab, p.i, p.x, p.y, s.Y, s.X, v);
    const int kind = kind_of(l);
    if (kind < PATH) continue;
#pragma unroll
    for (int k = 0; k < LINKS_OWNED; ++k)
      if (l.on[k]) {
        const SegPos q = towards(p, s, k);
        if (kind_at(lab, s, q, v) == kind) uf_union(parent, (int)p.i, (int)q.i);
      }
  }
}

__global__ __launch_bounds__(BLOCK) void graph_flatten(int* parent, Segments s) {
  const int lane = threadIdx.x & 63;
  FOR_EACH_SEGMENT(w, s) {
    const SegPos p = seg_pos(w, s, lane);
    if (p.valid && parent[p.i] >= 0) parent[p.i] = uf_find(parent, (int)p.i);        // roots keep pointing at themselves
  }
}

__global__ __launch_bounds__(BLOCK) void graph_reduce(const int* __restrict__ lab, const int* __restrict__ dist, Planes a, Segments s,
                                                      int* __restrict__ info) {
  const int lane = threadIdx.x & 63;
  int flags = 0;
  FOR_EACH_SEGMENT(w, s) {
    const SegPos p = seg_pos(w, s, lane);
    const int v = p.valid ? lab[p.i] : 0;
    if (v == 0) continue;
    const Links l = links_at(lab, p.i, p.x, p.y, s.Y, s.X, v);
    const int kind = kind_of(l);
    if (kind < PATH) continue;
    const int root = a.parent[p.i];
    int n0 = 0, n1 = 0, n2 = 0;         // path: face, diagonal links; junction: links out, inner face, inner diagonal links
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (l.on[k]) {
        const SegPos q = towards(p, s, k);
        const bool inner = kind_at(lab, s, q, v) == kind;
        if (kind == PATH) {
          if (!inner) {
            atomicMin(&a.lo[root], (int)q.i);
            atomicMax(&a.hi[root], (int)q.i);
          }
          if (!inner || k < LINKS_OWNED) (link_is_face(k) ? n0 : n1) += 1;
        } else if (!inner) {
          n0 += 1;
        } else if (k < LINKS_OWNED) {
          (link_is_face(k) ? n1 : n2) += 1;
        }
      }
    atomicAdd(&a.pixels[root], 1);
    if (n0) atomicAdd(&a.face[root], n0);
    if (n1) atomicAdd(&a.diag[root], n1);
    if (kind == JUNCTION && n2) atomicAdd(&a.lo[root], n2);
    if (kind == PATH && dist) {
      const int d = dist[p.i];
      if (d < 0 || d >= CLX_DIST_INF) flags |= 2;
      else {
        atomicAdd(&a.sum[root], (u64)d);
        atomicMin(&a.mn[root], d);
        atomicMax(&a.mx[root], d);
      }
    }
  }
  if (flags) atomicOr(&info[4], flags);
}

// what a pixel appends in launch 5
struct Item {
  int v, kind;
  bool branch, node;
  int other, other_kind;                // of an end pixel: the pixel its link leads to
  bool other_face;
};
__device__ __forceinline__ Item item_of(const int* __restrict__ lab, const int* __restrict__ parent, const Segments& s, const SegPos& p) {
  Item it = {0, ISOLATED, false, false, -1, ISOLATED, false};
  it.v = p.valid ? lab[p.i] : 0;
  if (it.v == 0) return it;
  const Links l = links_at(lab, p.i, p.x, p.y, s.Y, s.X, it.v);
  it.kind = kind_of(l);
  if (it.kind >= PATH) {
    const bool root = parent[p.i] == (int)p.i;
    it.branch = root && it.kind == PATH;
    it.node = root && it.kind == JUNCTION;
    return it;
  }
  it.node = true;
  if (it.kind == END) {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (l.on[k]) {
        const SegPos q = towards(p, s, k);
        it.other = (int)q.i;
        it.other_kind = kind_at(lab, s, q, it.v);
        it.other_face = link_is_face(k);
      }
    it.branch = it.other_kind == JUNCTION || (it.other_kind == END && (int)p.i < it.other);
  }
  return it;
}

__global__ __launch_bounds__(BLOCK) void graph_emit(const int* __restrict__ lab, Planes a, Segments s, long long limit_q10, int capacity_b,
                                                    int capacity_n, long long* __restrict__ branches, long long* __restrict__ nodes,
                                                    int* info) {
  constexpr int WAVES = BLOCK / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long ngroups = (s.nwaves + EMIT_SEGS - 1) / EMIT_SEGS;
  int pruned_pixels = 0, pruned_spurs = 0;      // of this lane's pixels; summed over the block after the loop
  for (long long g = (long long)blockIdx.x * WAVES + wave; g < ngroups; g += (long long)gridDim.x * WAVES) {
    u64 bb[EMIT_SEGS], nb[EMIT_SEGS];           // the lanes that append a branch row, a node row, per segment
    int nbranch = 0, nnode = 0;
#pragma unroll
    for (int r = 0; r < EMIT_SEGS; ++r) {
      const long long w = g * EMIT_SEGS + r;
      Item it = {0, ISOLATED, false, false, -1, ISOLATED, false};
      if (w < s.nwaves) it = item_of(lab, a.parent, s, seg_pos(w, s, lane));
      bb[r] = __ballot(it.branch);
      nb[r] = __ballot(it.node);
      nbranch += __popcll(bb[r]);
      nnode += __popcll(nb[r]);
    }
    int bslot = 0, nslot = 0;
    if (lane == 0) {
      if (nbranch) bslot = atomicAdd(&info[0], nbranch);
      if (nnode) nslot = atomicAdd(&info[1], nnode);
    }
    bslot = __shfl(bslot, 0, 64);
    nslot = __shfl(nslot, 0, 64);
#pragma unroll
    for (int r = 0; r < EMIT_SEGS; ++r) {
      const bool has_branch = (bb[r] >> lane) & 1ull, has_node = (nb[r] >> lane) & 1ull;
      if (has_branch || has_node) {
        const SegPos p = seg_pos(g * EMIT_SEGS + r, s, lane);
        const int i = (int)p.i;
        const Item it = item_of(lab, a.parent, s, p);
        if (has_node) {
          const int at = nslot + rank_below(nb[r], lane);
          if (at < capacity_n) {
            long long* row = nodes + (long long)NODE_WORDS * at;
            const bool cluster = it.kind == JUNCTION;
            row[0] = i;
            row[1] = it.v;
            row[2] = it.kind;
            row[3] = cluster ? a.pixels[i] : 1;
            row[4] = cluster ? a.face[i] : it.kind == END ? 1 : 0;
            row[5] = cluster ? a.diag[i] : 0;
            row[6] = cluster ? a.lo[i] : 0;
          }
        }
        if (has_branch) {
          long long pixels = 0, face, diag, lo, hi, node_lo, node_hi, sum = 0, mn = CLX_DIST_INF, mx = -1;
          int kind;
          if (it.kind == PATH) {
            pixels = a.pixels[i];
            face = a.face[i];
            diag = a.diag[i];
            lo = a.lo[i];
            hi = a.hi[i];
            sum = (long long)a.sum[i];
            mn = a.mn[i];
            mx = a.mx[i];
            if (hi < 0) {
              kind = CYCLE;
              lo = hi = node_lo = node_hi = -1;
            } else {
              const int klo = kind_at(lab, s, pos_at((int)lo, s), it.v), khi = kind_at(lab, s, pos_at((int)hi, s), it.v);
              kind = klo == END ? (khi == END ? END_END : SPUR) : khi == END ? SPUR : JUNCTION_JUNCTION;
              node_lo = klo == JUNCTION ? a.parent[lo] : lo;
              node_hi = khi == JUNCTION ? a.parent[hi] : hi;
            }
          } else {                              // the direct branch of an end pixel
            face = it.other_face ? 1 : 0;
            diag = 1 - face;
            kind = it.other_kind == END ? END_END : SPUR;
            const long long node = it.other_kind == JUNCTION ? a.parent[it.other] : it.other;
            lo = i < it.other ? i : it.other;
            hi = i < it.other ? it.other : i;
            node_lo = i < it.other ? i : node;
            node_hi = i < it.other ? node : i;
          }
          if (kind == SPUR && spur_pruned(face, diag, limit_q10)) {
            if (it.kind == PATH) a.pixels[i] = (int)((unsigned int)pixels | PRUNED);
            pruned_pixels += (int)pixels + 1;
            pruned_spurs += 1;
          }
          const int at = bslot + rank_below(bb[r], lane);
          if (at < capacity_b) {
            long long* row = branches + (long long)BRANCH_WORDS * at;
            row[0] = i;
            row[1] = it.v;
            row[2] = kind;
            row[3] = pixels;
            row[4] = face;
            row[5] = diag;
            row[6] = lo;
            row[7] = hi;
            row[8] = node_lo;
            row[9] = node_hi;
            row[10] = sum;
            row[11] = mn;
            row[12] = mx;
          }
        }
      }
      bslot += __popcll(bb[r]);
      nslot += __popcll(nb[r]);
    }
  }
  block_add2(pruned_pixels, pruned_spurs, info + 2);
}

__global__ __launch_bounds__(BLOCK) void graph_write(const int* __restrict__ lab, Planes a, Segments s, long long limit_q10,
                                                     int* __restrict__ branch_map, int* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  FOR_EACH_SEGMENT(w, s) {
    const SegPos p = seg_pos(w, s, lane);
    if (!p.valid) continue;
    const int v = lab[p.i];
    int id = 0;                                 // of the branch map
    bool pruned = false;
    if (v != 0) {
      const Links l = links_at(lab, p.i, p.x, p.y, s.Y, s.X, v);
      const int kind = kind_of(l);
      if (kind >= PATH) {
        const int root = a.parent[p.i];
        id = kind == PATH ? root + 1 : -(root + 1);
        pruned = kind == PATH && ((unsigned int)a.pixels[root] & PRUNED);
      } else {
        id = -((int)p.i + 1);
        if (kind == END) {
#pragma unroll
          for (int k = 0; k < 8; ++k)
            if (l.on[k]) {
              const SegPos q = towards(p, s, k);
              const int other = kind_at(lab, s, q, v);
              if (other == PATH) pruned = (unsigned int)a.pixels[a.parent[q.i]] & PRUNED;
              if (other == JUNCTION) pruned = spur_pruned(link_is_face(k), !link_is_face(k), limit_q10);
            }
        }
      }
    }
    if (branch_map) branch_map[p.i] = id;
    if (out) out[p.i] = pruned ? 0 : v;
  }
}

}  // namespace

extern "C" size_t clx_skeleton_graph_workspace(int nd, int Z, int Y, int X) {
  long long npix;
  if (clx_map_shape(nullptr, nd, Z, Y, X, 31, &npix) != CLX_OK) return 0;
  return (size_t)npix * (sizeof(u64) + 8 * sizeof(int));        // the nine planes of `Planes`
}

extern "C" int clx_skeleton_graph(const int32_t* labels, const int32_t* dist_sq, int nd, int Z, int Y, int X, long long limit_q10,
                                  int capacity_b, int capacity_n, int32_t* branch_map, int32_t* out, long long* branches,
                                  long long* nodes, int32_t* info, void* workspace, size_t workspace_bytes, clx_stream stream) {
  CLX_REQUIRE(labels && info && workspace, "clx_skeleton_graph: null pointer");
  CLX_REQUIRE(capacity_b >= 0 && capacity_n >= 0, "clx_skeleton_graph: capacity_b and capacity_n must be >= 0");
  CLX_REQUIRE(branches || capacity_b == 0, "clx_skeleton_graph: null branches with capacity_b > 0");
  CLX_REQUIRE(nodes || capacity_n == 0, "clx_skeleton_graph: null nodes with capacity_n > 0");
  CLX_REQUIRE_MAP(npix, "clx_skeleton_graph", nd, Z, Y, X, 31);
  CLX_REQUIRE(limit_q10 >= 0 && limit_q10 < (1ll << 30), "clx_skeleton_graph: limit_q10 must lie in [0, 2^30)");
  CLX_REQUIRE(out || limit_q10 == 0, "clx_skeleton_graph: null out with limit_q10 > 0");
  CLX_REQUIRE(workspace_bytes >= clx_skeleton_graph_workspace(nd, Z, Y, X),
              "clx_skeleton_graph: workspace_bytes is below clx_skeleton_graph_workspace(nd, Z, Y, X)");
  CLX_REQUIRE(((uintptr_t)workspace & 7) == 0, "clx_skeleton_graph: workspace must be 8-byte aligned");
  CLX_REQUIRE(out != labels && branch_map != labels, "clx_skeleton_graph: in-place operation is not supported");
  CLX_REQUIRE(!out || out != branch_map, "clx_skeleton_graph: out and branch_map must not be one buffer");
  hipStream_t st = (hipStream_t)stream;
  const Segments s = segments_of(Z, Y, X);
  Planes a;
  a.sum = (u64*)workspace;
  a.parent = (int*)(a.sum + npix);
  a.pixels = a.parent + npix;
  a.face = a.pixels + npix;
  a.diag = a.face + npix;
  a.lo = a.diag + npix;
  a.hi = a.lo + npix;
  a.mn = a.hi + npix;
  a.mx = a.mn + npix;
  const int grid = segment_grid(s.nwaves, GRAPH_MAX_GRID);
  CLX_REQUIRE(hipMemsetAsync(info, 0, 6 * sizeof(int), st) == hipSuccess, "clx_skeleton_graph: hipMemsetAsync failed");
  graph_classify<<<grid, BLOCK, 0, st>>>(labels, a, s);
  graph_link<<<grid, BLOCK, 0, st>>>(labels, a.parent, s);
  graph_flatten<<<grid, BLOCK, 0, st>>>(a.parent, s);
  graph_reduce<<<grid, BLOCK, 0, st>>>(labels, dist_sq, a, s, info);
  graph_emit<<<grid_for(s.nwaves, (BLOCK / 64) * EMIT_SEGS, EMIT_MAX_GRID), BLOCK, 0, st>>>(labels, a, s, limit_q10, capacity_b,
                                                                                            capacity_n, branches, nodes, info);
  if (branch_map || out) graph_write<<<grid, BLOCK, 0, st>>>(labels, a, s, limit_q10, branch_map, out);
  CLX_CHECK_LAUNCH("clx_skeleton_graph");
  return CLX_OK;
}
