// The skeleton stage: every object of a label map thinned to its centre lines, and the census of the lines.
//   clx_label_thin        out = labels where the pixel survives Guo & Hall's thinning with two alternating sub-iterations
//                         (algorithm A1: bwmorph('thin'), skimage.morphology.thin), label-aware, slice by slice
//   clx_skeleton_census   per label of a thinned map: pixels, links, blocks, ends, junction pixels, isolated pixels, d2 words
//
// Thinning is a synchronous rule on 3 x 3 neighbourhoods, a boolean function of nine bits: the pixel is alive, and for each of
// its eight neighbours "it lies in the slice, carries my label and is alive".  The labels are read ONCE:
//   init       a wave takes a segment (segments.h has the frame of this pass, of write and of the census) and ballots ten bit
//              planes, one 64-bit word per segment (bit i of word w of a row is pixel x = 64 w + i): the alive plane, twice,
//              and eight SAME planes, "neighbour k lies in my slice and has my non-zero label".  Since alive pixels are object
//              pixels, Pk = SAME_k & alive(neighbour k) from then on
//   steps      one launch advances the whole map by up to 8 iterations (16 sub-iterations).  A block of 256 threads takes an
//              EXTENT of 8 words x 128 rows (512 x 128 pixels): a TILE of 6 words x 96 rows and a halo of one word (64 pixels)
//              left and right and 16 rows above and below.  A thread owns 4 words of the extent: their SAME words stay in its
//              registers (64 VGPRs) for the whole launch, the alive words ping-pong between two LDS buffers of 8 KB.  A
//              sub-iteration is bit-sliced: the x neighbours are shifts across the word seams, the y neighbours the rows above
//              and below, C == 1 and 2 <= min(N1, N2) <= 3 adder networks on whole words: about 60 64-bit operations for 64
//              pixels.  What lies beyond the extent is unknown, so after s sub-iterations the outer s pixels of the extent are
//              wrong; 16 sub-iterations leave the tile exact.  (The words left and right of a row's ends in LDS are those of
//              the rows before and after: they reach the outermost pixel only, which is wrong from the first sub-iteration on.
//              Beyond the map everything is dead and stays dead, and the SAME planes already hold the map's edges.)
//   lockstep   every tile advances by the same number of sub-iterations a launch, and every launch runs whole iterations, so
//              the state after launch r is the global synchronous schedule's, whatever the tiles.
//   ping-pong  launch r (counted over all calls since resume == 0) reads alive plane r & 1 and writes the tile to the other:
//              no launch reads a word it writes.
//   activity   a tile has a deleted-something flag per launch, and a tile none of whose 9 tiles of the slice deleted a pixel
//              in the launch before is skipped: tile_rounds.h has the rule and the proof, with "deleted a pixel" for "changed".
//              It holds here because the halo reaches into the neighbour tiles only (or beyond the map) and a launch runs
//              whole iterations: an inactive tile sees the state its last launch started from, in which a whole iteration
//              deleted nothing in it and around it.
//   counters   two words per launch of a call: the pixels deleted in the launch, and in its last iteration.  A launch that
//              finds 0 in the second word of the launch before returns at once, as do all after it.  `finish` forms info and
//              leaves the launch count and the last word in the head for a call with resume == 1; `write` forms out from the
//              labels and the current plane.
// Integers only, in fact bits; the labels are compared and never an index.  The same bits in every run.
#include "segments.h"
#include "skeleton_links.h"
#include "tile_rounds.h"

namespace {

constexpr int EW = 8, ER = 128;                 // the extent a block loads: words x rows
constexpr int HALO_W = 1, HALO_R = 16;          // halo: one word left and right, 16 rows above and below
constexpr int TW = EW - 2 * HALO_W;             // the tile: 6 words (384 pixels) ...
constexpr int TR = ER - 2 * HALO_R;             // ... x 96 rows
constexpr int WPT = EW * ER / BLOCK;            // words a thread owns: 4, 32 extent rows apart
constexpr int LAUNCH_ITERATIONS = HALO_R / 2;   // iterations a launch runs at most: 2 sub-iterations use up 2 halo pixels
constexpr int MAX_ITERATIONS = 64;              // iterations a call queues at most
constexpr int MAX_LAUNCHES = MAX_ITERATIONS / LAUNCH_ITERATIONS;
constexpr int THIN_MAX_GRID = 1024;             // blocks a launch; each takes the tiles blockIdx.x, blockIdx.x + gridDim.x, ...
constexpr int PLANE_MAX_GRID = 2048;            // blocks of the passes over the words (init, write, census)
constexpr int CENSUS_INIT_MAX_GRID = 1024;      // blocks of 256 words of the census table
constexpr int PAD = 16;                         // zero words before and after an LDS buffer: a neighbour is at most 9 words away
constexpr int NWORDS = 10;                      // words per label of the census

struct Shape : Segments {                       // a word of a bit plane is a segment: nseg words per row, nwaves in all
  int ntx, nty;                                 // tiles per slice
  long long ntiles;
};

struct Bits {                                   // the workspace
  int* head;                                    // [HEAD_WORDS]: [0] launches so far, [1] pixels the last iteration deleted (or 1)
  int* counters;                                // [MAX_LAUNCHES][2]
  u64* same;                                    // [8][nwaves]: N, NE, E, SE, S, SW, W, NW
  u64* alive0;                                  // read by the even launches
  u64* alive1;
  unsigned char* flag0;                         // written by the even launches
  unsigned char* flag1;
};

// the words and the tiles of a checked map: Z * Y * X < 2^31
inline Shape thin_shape(int Z, int Y, int X) {
  Shape s = {segments_of(Z, Y, X), 0, 0, 0};
  s.ntx = (s.nseg + TW - 1) / TW;
  s.nty = (Y + TR - 1) / TR;
  s.ntiles = (long long)Z * s.nty * s.ntx;
  return s;
}
inline size_t thin_flag_bytes(long long ntiles) { return ((size_t)ntiles + 7) & ~(size_t)7; }

// does neighbour (dx, dy) of the pixel lie in its slice?
__device__ __forceinline__ bool has_neighbour(const SegPos& a, const Shape& s, int dx, int dy) {
  return (dx < 0 ? a.x > 0 : dx > 0 ? a.x < s.X - 1 : true) && (dy < 0 ? a.y > 0 : dy > 0 ? a.y < s.Y - 1 : true);
}

__global__ __launch_bounds__(BLOCK) void thin_init(const int* __restrict__ labels, Bits b, Shape s) {
  const int lane = threadIdx.x & 63;
  if (blockIdx.x == 0 && threadIdx.x == 0) { b.head[0] = 0; b.head[1] = 1; }
  FOR_EACH_SEGMENT(w, s) {
    const SegPos a = seg_pos(w, s, lane);
    const int v = a.valid ? labels[a.i] : 0;
    const bool obj = v != 0;
    const u64 alive = __ballot(obj);
    if (lane == 8) b.alive0[w] = alive;
    if (lane == 9) b.alive1[w] = alive;
    constexpr int DX[8] = {0, 1, 1, 1, 0, -1, -1, -1}, DY[8] = {-1, -1, 0, 1, 1, 1, 0, -1};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const bool same = obj && has_neighbour(a, s, DX[k], DY[k]) && labels[a.i + (long long)DY[k] * s.X + DX[k]] == v;
      const u64 m = __ballot(same);
      if (lane == k) b.same[k * s.nwaves + w] = m;
    }
  }
}

// the pixels of word i of `from` that a sub-iteration deletes; `same`: the word's eight SAME words
__device__ __forceinline__ u64 thin_deleted(const u64* __restrict__ from, int i, u64 a, const u64* same, bool even) {
  const u64 n = from[i - EW], nl = from[i - EW - 1], nr = from[i - EW + 1];
  const u64 al = from[i - 1], ar = from[i + 1];
  const u64 so = from[i + EW], sl = from[i + EW - 1], sr = from[i + EW + 1];
  const u64 p2 = same[0] & n;
  const u64 p3 = same[1] & ((n >> 1) | (nr << 63));
  const u64 p4 = same[2] & ((a >> 1) | (ar << 63));
  const u64 p5 = same[3] & ((so >> 1) | (sr << 63));
  const u64 p6 = same[4] & so;
  const u64 p7 = same[5] & ((so << 1) | (sl >> 63));
  const u64 p8 = same[6] & ((a << 1) | (al >> 63));
  const u64 p9 = same[7] & ((n << 1) | (nl >> 63));
  // C == 1: exactly one of the four 0 -> 1 patterns
  const u64 t1 = ~p2 & (p3 | p4), t2 = ~p4 & (p5 | p6), t3 = ~p6 & (p7 | p8), t4 = ~p8 & (p9 | p2);
  const u64 c1 = ((t1 ^ t2) ^ (t3 ^ t4)) & ~((t1 & t2) | (t3 & t4));
  // 2 <= min(N1, N2) <= 3: both sums of four bits are >= 2 and not both are 4
  const u64 u1 = p9 | p2, u2 = p3 | p4, u3 = p5 | p6, u4 = p7 | p8;
  const u64 v1 = p2 | p3, v2 = p4 | p5, v3 = p6 | p7, v4 = p8 | p9;
  const u64 n1ge2 = (u1 & u2) | (u3 & u4) | ((u1 ^ u2) & (u3 ^ u4));
  const u64 n2ge2 = (v1 & v2) | (v3 & v4) | ((v1 ^ v2) & (v3 ^ v4));
  const u64 both4 = u1 & u2 & u3 & u4 & v1 & v2 & v3 & v4;
  const u64 m = even ? (p6 | p7 | ~p9) & p8 : (p2 | p3 | ~p5) & p4;
  return a & c1 & n1ge2 & n2ge2 & ~both4 & ~m;
}

// launch k of a call: `iterations` whole iterations on every active tile
__global__ __launch_bounds__(BLOCK) void thin_steps(Bits b, int k, int iterations, Shape s) {
  __shared__ u64 buf[2][PAD + EW * ER + PAD];
  __shared__ int sums[2][BLOCK / 64];

  if ((k == 0 ? b.head[1] : b.counters[2 * (k - 1) + 1]) == 0) return;       // the iteration before deleted nothing: the fixed point
  const Round rd = round_at((unsigned int)b.head[0] + (unsigned int)k, b.flag0, b.flag1);
  const u64* __restrict__ src = rd.odd ? b.alive1 : b.alive0;
  u64* __restrict__ dst = rd.odd ? b.alive0 : b.alive1;

  if (threadIdx.x < PAD) {
    buf[0][threadIdx.x] = buf[1][threadIdx.x] = 0ull;
    buf[0][PAD + EW * ER + threadIdx.x] = buf[1][PAD + EW * ER + threadIdx.x] = 0ull;
  }
  const int c = threadIdx.x & (EW - 1), er0 = threadIdx.x / EW;             // the thread's words: (er0 + 32 m, c), LDS index tid + 256 m
  const bool cin = c >= HALO_W && c < EW - HALO_W;
  int total = 0, last = 0;                                                  // pixels this thread deleted in tiles: all, last iteration

  for (long long t = blockIdx.x; t < s.ntiles; t += gridDim.x) {
    const int tx = (int)(t % s.ntx), ty = (int)((t / s.ntx) % s.nty), tz = (int)(t / ((long long)s.ntx * s.nty));
    if (!tile_active<2>(rd, s.Z, s.nty, s.ntx, t, tz, ty, tx)) continue;      // the slice stands for the tile's z

    const int wc = tx * TW - HALO_W + c;
    u64 same[WPT][8];
    long long gw[WPT];
    bool mine[WPT];                                     // a word of the tile, inside the map: counted and written
#pragma unroll
    for (int m = 0; m < WPT; ++m) {
      const int er = er0 + m * (BLOCK / EW);
      const int y = ty * TR - HALO_R + er;
      const bool in = (unsigned int)wc < (unsigned int)s.nseg && (unsigned int)y < (unsigned int)s.Y;
      gw[m] = ((long long)tz * s.Y + y) * s.nseg + wc;
      mine[m] = in && cin && er >= HALO_R && er < ER - HALO_R;
      const u64 a = in ? src[gw[m]] : 0ull;
      buf[0][PAD + threadIdx.x + m * BLOCK] = a;
#pragma unroll
      for (int q = 0; q < 8; ++q) same[m][q] = a ? b.same[q * s.nwaves + gw[m]] : 0ull;     // a dead word stays dead
    }
    __syncthreads();

    int cur = 0, tile_total = 0;
    for (int step = 0; step < 2 * iterations; ++step) {
      const u64* __restrict__ from = buf[cur] + PAD;
      u64* __restrict__ to = buf[cur ^ 1] + PAD;
      const bool final_iteration = step >= 2 * iterations - 2;
#pragma unroll
      for (int m = 0; m < WPT; ++m) {
        const int i = threadIdx.x + m * BLOCK;
        const u64 a = from[i];
        u64 del = 0ull;
        if (a) del = thin_deleted(from, i, a, same[m], step & 1);
        to[i] = a & ~del;
        if (mine[m]) {
          const int n = __popcll(del);
          tile_total += n;
          if (final_iteration) last += n;
        }
      }
      __syncthreads();
      cur ^= 1;
    }

#pragma unroll
    for (int m = 0; m < WPT; ++m)
      if (mine[m]) dst[gw[m]] = buf[cur][PAD + threadIdx.x + m * BLOCK];
    total += tile_total;
    const int changed = __syncthreads_or(tile_total);   // the barrier also ends the reads of this tile
    if (threadIdx.x == 0) rd.fout[t] = (unsigned char)(changed != 0);
  }

#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    total += __shfl_down(total, o, 64);
    last += __shfl_down(last, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    sums[0][threadIdx.x >> 6] = total;
    sums[1][threadIdx.x >> 6] = last;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    int sum = 0;
    for (int w = 0; w < BLOCK / 64; ++w) sum += sums[threadIdx.x][w];
    if (sum) atomicAdd(b.counters + 2 * k + threadIdx.x, sum);
  }
}

// the last but one launch of a call: info from the counters, and the head for the next call
__global__ void thin_finish(int* __restrict__ head, const int* __restrict__ counters, int launches, int* __restrict__ info) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int ran = 0, deleted = 0, before = head[1];
  for (int k = 0; k < MAX_LAUNCHES; ++k)
    if (k < launches && before != 0) {                  // launch k ran
      ++ran;
      deleted += counters[2 * k];
      before = counters[2 * k + 1];
    }
  info[1] = ran == launches ? before : 0;
  info[2] = deleted;
  head[0] = (int)((unsigned int)head[0] + (unsigned int)ran);
  head[1] = ran == launches ? before : 0;
}

// out from the labels and the plane the launches so far left the state in
__global__ __launch_bounds__(BLOCK) void thin_write(const int* __restrict__ labels, Bits b, Shape s, int* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const u64* __restrict__ alive = ((unsigned int)b.head[0] & 1u) ? b.alive1 : b.alive0;
  FOR_EACH_SEGMENT(w, s) {
    const SegPos a = seg_pos(w, s, lane);
    const u64 bits = alive[w];
    if (a.valid) out[a.i] = ((bits >> lane) & 1ull) ? labels[a.i] : 0;
  }
}

// ----------------------------------------------------------------------------------------------------------------- census

struct Census {                         // what a run of pixels of one label adds to its words
  unsigned int c0;                      // pixels | face links << 8 | diagonal links << 16 | blocks << 24: a run has <= 64 pixels
  unsigned int c1;                      // ends | junction pixels << 8 | isolated << 16
  u64 sum;
  int mn, mx;
  __device__ __forceinline__ Census shifted(int d) const {
    return {(unsigned int)__shfl_down((int)c0, d), (unsigned int)__shfl_down((int)c1, d), __shfl_down(sum, d), __shfl_down(mn, d),
            __shfl_down(mx, d)};
  }
  __device__ __forceinline__ void take(const Census& o) {
    c0 += o.c0;
    c1 += o.c1;
    sum += o.sum;
    mn = o.mn < mn ? o.mn : mn;
    mx = o.mx > mx ? o.mx : mx;
  }
};

__global__ void census_init(long long* __restrict__ words, int* __restrict__ bad, int nid) {
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 == 0) *bad = 0;
  for (long long i = i0; i < (long long)nid * NWORDS; i += (long long)gridDim.x * blockDim.x) {
    const int q = (int)(i % NWORDS);
    words[i] = q == 8 ? (long long)CLX_DIST_INF : q == 9 ? -1ll : 0ll;
  }
}

__global__ __launch_bounds__(BLOCK) void census_kernel(const int* __restrict__ lab, const int* __restrict__ dist, Shape s, int nid,
                                                       long long* __restrict__ words, int* __restrict__ bad) {
  __shared__ int keys[SLOTS];
  __shared__ u64 acc[8][SLOTS];
  __shared__ int smin[SLOTS], smax[SLOTS];
  for (int i = threadIdx.x; i < SLOTS; i += BLOCK) {
    keys[i] = 0;
    for (int q = 0; q < 8; ++q) acc[q][i] = 0ull;
    smin[i] = CLX_DIST_INF;
    smax[i] = -1;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  int flags = 0;
  FOR_EACH_SEGMENT(w, s) {
    const SegPos a = seg_pos(w, s, lane);
    int v = a.valid ? lab[a.i] : 0;
    if ((unsigned int)v >= (unsigned int)nid) { v = 0; flags |= 1; }
    Census r = {0u, 0u, 0ull, CLX_DIST_INF, -1};
    if (v != 0) {
      const Links l = links_at(lab, a.i, a.x, a.y, s.Y, s.X, v);      // (v lies in [1, nid): so does a neighbour that carries v)
      const int degree = l.degree();
      r.c0 = 1u | (unsigned int)l.owned_face() << 8 | (unsigned int)l.owned_diag() << 16 | (unsigned int)l.block << 24;
      r.c1 = (unsigned int)(degree == 1) | (unsigned int)(degree >= 3) << 8 | (unsigned int)(degree == 0) << 16;
      if (dist) {
        const int d = dist[a.i];
        if (d < 0 || d >= CLX_DIST_INF) flags |= 2;
        else { r.sum = (u64)d; r.mn = r.mx = d; }
      }
    }
    const int left = __shfl_up(v, 1, 64);
    const bool head = lane == 0 || left != v;
    const u64 heads = __ballot(head);
    r = reduce_run(r, lane, lane + run_lanes(heads, lane));
    if (head && v != 0) {
      const u64 q[8] = {r.c0 & 255u, (r.c0 >> 8) & 255u, (r.c0 >> 16) & 255u, r.c0 >> 24, r.c1 & 255u, (r.c1 >> 8) & 255u, (r.c1 >> 16) & 255u,
                        r.sum};
      const int slot = find_slot(keys, v);
      long long* row = words + (long long)v * NWORDS;
      if (slot >= 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (q[j]) atomicAdd(&acc[j][slot], q[j]);
        if (r.mx >= 0) { atomicMin(&smin[slot], r.mn); atomicMax(&smax[slot], r.mx); }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (q[j]) atomicAdd((u64*)row + j, q[j]);
        if (r.mx >= 0) { atomicMin(row + 8, (long long)r.mn); atomicMax(row + 9, (long long)r.mx); }
      }
    }
  }
  if (flags) atomicOr(bad, flags);
  __syncthreads();

  for (int i = threadIdx.x; i < SLOTS; i += BLOCK) {
    const int label = keys[i];
    if (label == 0) continue;
    long long* row = words + (long long)label * NWORDS;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (acc[j][i]) atomicAdd((u64*)row + j, acc[j][i]);
    if (smax[i] >= 0) { atomicMin(row + 8, (long long)smin[i]); atomicMax(row + 9, (long long)smax[i]); }
  }
}

}  // namespace

extern "C" size_t clx_label_thin_workspace(int nd, int Z, int Y, int X) {
  long long npix;
  if (clx_map_shape(nullptr, nd, Z, Y, X, 31, &npix) != CLX_OK) return 0;
  const Shape s = thin_shape(Z, Y, X);
  return (size_t)(HEAD_WORDS + 2 * MAX_LAUNCHES) * sizeof(int) + (size_t)s.nwaves * 10 * sizeof(u64) + 2 * thin_flag_bytes(s.ntiles);
}

extern "C" int clx_label_thin(const int32_t* labels, int nd, int Z, int Y, int X, int iterations, int resume, int32_t* out,
                              int32_t* info, void* workspace, size_t workspace_bytes, clx_stream stream) {
  CLX_REQUIRE(labels && out && info && workspace, "clx_label_thin: null pointer");
  CLX_REQUIRE_MAP(npix, "clx_label_thin", nd, Z, Y, X, 31);
  const Shape s = thin_shape(Z, Y, X);
  CLX_REQUIRE(iterations >= 1 && iterations <= MAX_ITERATIONS, "clx_label_thin: iterations must lie in [1, 64]");
  CLX_REQUIRE(resume == 0 || resume == 1, "clx_label_thin: resume must be 0 or 1");
  CLX_REQUIRE(workspace_bytes >= clx_label_thin_workspace(nd, Z, Y, X),
              "clx_label_thin: workspace_bytes is below clx_label_thin_workspace(nd, Z, Y, X)");
  CLX_REQUIRE(((uintptr_t)workspace & 7) == 0, "clx_label_thin: workspace must be 8-byte aligned");
  CLX_REQUIRE(out != labels, "clx_label_thin: in-place operation is not supported");
  hipStream_t st = (hipStream_t)stream;
  Bits b;
  b.head = (int*)workspace;
  b.counters = b.head + HEAD_WORDS;
  b.same = (u64*)(b.counters + 2 * MAX_LAUNCHES);
  b.alive0 = b.same + 8 * s.nwaves;
  b.alive1 = b.alive0 + s.nwaves;
  b.flag0 = (unsigned char*)(b.alive1 + s.nwaves);
  b.flag1 = b.flag0 + thin_flag_bytes(s.ntiles);
  CLX_REQUIRE(hipMemsetAsync(info, 0, 3 * sizeof(int), st) == hipSuccess, "clx_label_thin: hipMemsetAsync failed");
  CLX_REQUIRE(hipMemsetAsync(b.counters, 0, 2 * MAX_LAUNCHES * sizeof(int), st) == hipSuccess, "clx_label_thin: hipMemsetAsync failed");
  const int pgrid = segment_grid(s.nwaves, PLANE_MAX_GRID);
  if (!resume) thin_init<<<pgrid, BLOCK, 0, st>>>(labels, b, s);
  const int grid = grid_for(s.ntiles, 1, THIN_MAX_GRID);
  const int launches = (iterations + LAUNCH_ITERATIONS - 1) / LAUNCH_ITERATIONS;
  for (int k = 0; k < launches; ++k) {
    const int left = iterations - k * LAUNCH_ITERATIONS;
    thin_steps<<<grid, BLOCK, 0, st>>>(b, k, left < LAUNCH_ITERATIONS ? left : LAUNCH_ITERATIONS, s);
  }
  thin_finish<<<1, 64, 0, st>>>(b.head, b.counters, launches, info);
  thin_write<<<pgrid, BLOCK, 0, st>>>(labels, b, s, out);
  CLX_CHECK_LAUNCH("clx_label_thin");
  return CLX_OK;
}

extern "C" int clx_skeleton_census(const int32_t* skeleton, const int32_t* dist_sq, int nd, int Z, int Y, int X, int nid,
                                   long long* words, int32_t* bad, clx_stream stream) {
  CLX_REQUIRE(skeleton && words && bad, "clx_skeleton_census: null pointer");
  CLX_REQUIRE_MAP(npix, "clx_skeleton_census", nd, Z, Y, X, 31);
  const Shape s = thin_shape(Z, Y, X);
  CLX_REQUIRE(nid >= 1 && nid <= (1 << 24), "clx_skeleton_census: nid must lie in [1, 2^24]");
  hipStream_t st = (hipStream_t)stream;
  census_init<<<grid_for((long long)nid * NWORDS, 256, CENSUS_INIT_MAX_GRID), 256, 0, st>>>(words, bad, nid);
  census_kernel<<<segment_grid(s.nwaves, PLANE_MAX_GRID), BLOCK, 0, st>>>(skeleton, dist_sq, s, nid, words, bad);
  CLX_CHECK_LAUNCH("clx_skeleton_census");
  return CLX_OK;
}
