// Grey-scale morphology on a map of grey levels, for the granularity stage: erosion / dilation by the face neighbours and
// reconstruction by dilation, without a flood queue.
//   clx_grey_morph         out = the min (erode) / max (dilate) of `in` over the inside pixels within `steps` face steps
//   clx_grey_reconstruct   out = the least r >= min(marker, image) with r[p] = min(image[p], max(r[p], r[face neighbours]))
//
// Values are grey levels in [0, 65535] (16 bits in LDS); a pixel with mask[p] == 0 and everything beyond the map is OUTSIDE:
// it gets 0 and conducts nothing.  A value outside the range under an inside pixel counts as 0 and sets a bad bit.
//
// clx_grey_morph.  One launch makes all the steps on chip.  A block of 256 threads takes a tile (64 x 32, or 32 x 8 x 8) and a
// halo of `steps` pixels (at most 16, or 4) on every side: it loads the values and the inside bits into LDS once -- an outside
// pixel holds the operation's neutral value, 65535 or 0, and keeps it, so nothing passes through it -- and applies the step
// `steps` times between two LDS buffers.  Step s is exact on the region s pixels inside the loaded one and is only computed
// there; after `steps` of them that is the tile, which the block writes.  A wave takes whole rows, a lane the columns lane and
// lane + 64.
//
// clx_grey_reconstruct.  The value only rises from m = min(marker, image), and every value it takes is min(m[q], the smallest
// image value along a face path from q): so the fixed point reached from below is the least one, whatever the order of the
// updates, and a function of the inputs alone.
//   round      one launch.  A block takes a tile (256 x 32, or 64 x 8 x 8) and a halo of one pixel, loads the value and the image
//              as 16-bit words into LDS once -- an outside pixel is image 0, which clamps it to 0 -- and makes SWEEPS of
//              directional scans: +x, -x, +y, -y (+z, -z), until a sweep changes nothing, at most MAX_SWEEPS of them (a tile
//              cut short has changed and is taken up again in the next round), and writes its interior.  The halo is what the
//              round before left and is only read.  No block waits for another.
//   scans      along a row r[q] <- min(I[q], max(r[q], r[q - 1])) applies to the value that arrives from q - 1 the clamp
//              x -> min(hi, max(lo, x)) with (lo, hi) = (r[q], I[q]).  Clamp a, then clamp b, is again a clamp:
//              (min(hi_b, max(lo_b, lo_a)), min(hi_b, max(lo_b, hi_a))).  So 64 pixels of a row are one inclusive wave scan
//              over (lo, hi) pairs, packed in one 32-bit word, and the carry of the pixel before goes through the result;
//              a wave owns whole rows.  Along y and z a thread owns a line (consecutive lanes consecutive in x) and walks it
//              up and down with the carry in a register.
//   ping-pong  between rounds the value lies in an int32 plane; round r reads `out` and writes the workspace's plane if r is
//              even, the other way round if odd: no launch reads a word it writes, and the state after round r is a function
//              of the inputs.  r counts over all calls since resume == 0 and lies in the workspace's head.  The image, with
//              the mask and the range applied, lies in the workspace as 16-bit words.
//   activity   a tile has a changed flag per round, in two arrays that alternate like the planes.  A tile is ACTIVE in round r
//              iff it or one of its 8 / 26 face-, edge- or corner-adjacent tiles changed in round r - 1 (round 0: all are).  An
//              active tile always writes its interior; an inactive one clears its flag and is done.  An inactive tile would not
//              have changed: its values and its halo are those of the round in which it last came to rest.  By induction it
//              holds equal values in both planes, so when a round changes no tile both planes hold the fixed point.
//   counters   a word per round of the call counts the tiles that changed in it; a launch that finds 0 in the word of the
//              round before returns at once, as do all after it.  The last launch of a call forms info from the counters and
//              leaves r and the last count in the head for a call with resume == 1.
// Integer minima and maxima only: the same bits and the same rounds in every run.
#include "region_scan.h"

namespace {

constexpr unsigned int MAX_LEVEL = 65535u;
constexpr int TILE_MAX_GRID = 1024;     // blocks a launch; each takes the tiles blockIdx.x, blockIdx.x + gridDim.x, ...
constexpr int INIT_MAX_GRID = 4096;     // blocks of BLOCK pixels a trip (the first call's start values)
constexpr int MAX_SWEEPS = 16;          // sweeps of directional scans a tile makes in LDS in one round
constexpr int MAX_ROUNDS = 64;          // launches a call queues at most: the counters of a call
constexpr int HEAD_WORDS = 16;          // [0] rounds so far, [1] the tiles that changed in the last of them (or 1: none yet)
constexpr int WAVES = BLOCK / 64;

template <int ND> struct MorphShape;    // the tile of clx_grey_morph and the largest halo: the steps of one launch
template <> struct MorphShape<2> { static constexpr int TZ = 1, TY = 32, TX = 64, ZH = 0, HMAX = 16; };
template <> struct MorphShape<3> { static constexpr int TZ = 8, TY = 8, TX = 32, ZH = 1, HMAX = 4; };
template <int ND> struct ReconShape;    // the tile of clx_grey_reconstruct; TX is a multiple of 64: a wave scans 64 pixels
template <> struct ReconShape<2> { static constexpr int TZ = 1, TY = 32, TX = 256, ZH = 0; };
template <> struct ReconShape<3> { static constexpr int TZ = 8, TY = 8, TX = 64, ZH = 1; };

struct TileGrid {
  int ntz, nty, ntx;
  long long ntiles;
};
template <typename S2, typename S3>
inline TileGrid tile_grid(int nd, int Z, int Y, int X) {
  TileGrid g;
  g.ntz = nd == 2 ? 1 : (Z + S3::TZ - 1) / S3::TZ;
  g.nty = nd == 2 ? (Y + S2::TY - 1) / S2::TY : (Y + S3::TY - 1) / S3::TY;
  g.ntx = nd == 2 ? (X + S2::TX - 1) / S2::TX : (X + S3::TX - 1) / S3::TX;
  g.ntiles = (long long)g.ntz * g.nty * g.ntx;
  return g;
}
inline size_t flag_bytes(long long ntiles) { return ((size_t)ntiles + 3) & ~(size_t)3; }

__device__ __forceinline__ unsigned int umin(unsigned int a, unsigned int b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned int umax(unsigned int a, unsigned int b) { return a > b ? a : b; }

template <int ND, bool DILATE>
__global__ __launch_bounds__(BLOCK) void grey_morph_kernel(const int* __restrict__ in, const unsigned char* __restrict__ mask, int Z, int Y,
                                                           int X, TileGrid g, int steps, int* __restrict__ out, int* __restrict__ bad) {
  typedef MorphShape<ND> S;
  constexpr int PX = S::TX + 2 * S::HMAX, PY = S::TY + 2 * S::HMAX, PZ = S::TZ + 2 * S::HMAX * S::ZH, PN = PX * PY * PZ;
  constexpr unsigned int NEUTRAL = DILATE ? 0u : MAX_LEVEL;
  __shared__ unsigned short val[2][PN];
  __shared__ unsigned char ins[PN];
  const int H = steps, HZ = S::ZH ? steps : 0;
  const int nx = S::TX + 2 * H, ny = S::TY + 2 * H, nz = S::TZ + 2 * HZ;      // the loaded region; the pitches stay PX and PY
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int flags = 0;

  for (long long t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
    const int tx = (int)(t % g.ntx), ty = (int)((t / g.ntx) % g.nty), tz = (int)(t / ((long long)g.ntx * g.nty));
    const int z0 = tz * S::TZ - HZ, y0 = ty * S::TY - H, x0 = tx * S::TX - H;
    __syncthreads();                                      // ends the reads of the tile before
    for (int row = wave; row < nz * ny; row += WAVES) {
      const int hz = row / ny, hy = row - hz * ny;
      const int gz = z0 + hz, gy = y0 + hy;
      const bool rowin = (unsigned int)gz < (unsigned int)Z && (unsigned int)gy < (unsigned int)Y;
      for (int hx = lane; hx < nx; hx += 64) {
        const int gx = x0 + hx;
        unsigned int v = NEUTRAL;
        bool inside = false;
        if (rowin && (unsigned int)gx < (unsigned int)X) {
          const long long p = ((long long)gz * Y + gy) * X + gx;
          inside = mask ? mask[p] != 0 : true;
          if (inside) {
            v = (unsigned int)in[p];
            if (v > MAX_LEVEL) { v = 0; flags |= 1; }
          }
        }
        const int i = (hz * PY + hy) * PX + hx;
        val[0][i] = (unsigned short)v;
        ins[i] = inside;
      }
    }

    int cur = 0;
    for (int s = 1; s <= steps; ++s) {
      __syncthreads();
      const unsigned short* __restrict__ from = val[cur];
      unsigned short* __restrict__ to = val[cur ^ 1];
      const int sz = S::ZH ? s : 0, ry = ny - 2 * s, rows = (nz - 2 * sz) * ry;
      for (int row = wave; row < rows; row += WAVES) {
        const int qz = row / ry;
        const int hz = sz + qz, hy = s + row - qz * ry;
        for (int hx = s + lane; hx < nx - s; hx += 64) {
          const int i = (hz * PY + hy) * PX + hx;
          unsigned int v = NEUTRAL;
          if (ins[i]) {
            v = from[i];
            const unsigned int a = from[i - 1], b = from[i + 1], c = from[i - PX], d = from[i + PX];
            v = DILATE ? umax(umax(v, umax(a, b)), umax(c, d)) : umin(umin(v, umin(a, b)), umin(c, d));
            if (S::ZH) {
              const unsigned int e = from[i - PX * PY], f = from[i + PX * PY];
              v = DILATE ? umax(v, umax(e, f)) : umin(v, umin(e, f));
            }
          }
          to[i] = (unsigned short)v;
        }
      }
      cur ^= 1;
    }
    __syncthreads();

    for (int row = wave; row < S::TZ * S::TY; row += WAVES) {
      const int iz = row / S::TY, iy = row % S::TY;
      const int gz = tz * S::TZ + iz, gy = ty * S::TY + iy;
      if (gz >= Z || gy >= Y) continue;
      for (int ix = lane; ix < S::TX; ix += 64) {
        const int gx = tx * S::TX + ix;
        if (gx >= X) continue;
        const int i = ((iz + HZ) * PY + iy + H) * PX + ix + H;
        out[((long long)gz * Y + gy) * X + gx] = ins[i] ? (int)val[cur][i] : 0;
      }
    }
  }
  if (flags) atomicOr(bad, flags);
}

// the planes, the flags and the words of clx_grey_reconstruct's workspace
struct Planes {
  int* out;
  int* wout;
  unsigned short* image;                // the image with the mask and the range applied: 0 on outside pixels
  unsigned char* flag0;                 // written by the even rounds
  unsigned char* flag1;
  int* head;
  int* counters;
};

__global__ __launch_bounds__(BLOCK) void reconstruct_init(const int* __restrict__ marker, const int* __restrict__ image,
                                                          const unsigned char* __restrict__ mask, Planes q, long long npix,
                                                          int* __restrict__ info) {
  int flags = 0;
  for (long long p = (long long)blockIdx.x * BLOCK + threadIdx.x; p < npix; p += (long long)gridDim.x * BLOCK) {
    unsigned int m = 0, v = 0;
    if (mask ? mask[p] != 0 : true) {
      m = (unsigned int)marker[p];
      v = (unsigned int)image[p];
      if (m > MAX_LEVEL) { m = 0; flags |= 1; }
      if (v > MAX_LEVEL) { v = 0; flags |= 2; }
    }
    q.image[p] = (unsigned short)v;
    q.out[p] = (int)umin(m, v);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { q.head[0] = 0; q.head[1] = 1; }
  if (flags) atomicOr(info, flags);
}

// a + b for the clamps a, then b, as (lo | hi << 16)
__device__ __forceinline__ unsigned int clamp_then(unsigned int a, unsigned int lo_b, unsigned int hi_b) {
  return umin(hi_b, umax(lo_b, a & 0xffffu)) | (umin(hi_b, umax(lo_b, a >> 16)) << 16);
}

// The 64 pixels from `at` on, a lane each, scanned in the direction FWD (towards larger x) or against it: the pixel takes
// min(I, max(r, the value of the pixel before)), `carry` before the first.  Returns the last pixel's value, in every lane.
template <bool FWD>
__device__ __forceinline__ unsigned int scan_row(unsigned short* __restrict__ r, const unsigned short* __restrict__ im, int at, int lane,
                                                 unsigned int carry, int& changed) {
  const unsigned int old = r[at + lane], hi = im[at + lane];
  unsigned int f = old | (hi << 16);
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned int o = FWD ? __shfl_up(f, d) : __shfl_down(f, d);
    if (FWD ? lane >= d : lane + d < 64) f = clamp_then(o, f & 0xffffu, f >> 16);
  }
  const unsigned int v = umin(f >> 16, umax(f & 0xffffu, carry));
  if (v != old) { r[at + lane] = (unsigned short)v; changed = 1; }
  return __shfl(v, FWD ? 63 : 0);
}

// the line of `n` pixels `stride` apart from `at` on, walked up and then down
__device__ __forceinline__ void walk_line(unsigned short* __restrict__ r, const unsigned short* __restrict__ im, int at, int stride, int n,
                                          int& changed) {
  unsigned int carry = r[at - stride];
  for (int j = 0; j < n; ++j) {
    const int i = at + j * stride;
    const unsigned int old = r[i];
    carry = umin(im[i], umax(old, carry));
    if (carry != old) { r[i] = (unsigned short)carry; changed = 1; }
  }
  carry = r[at + n * stride];
  for (int j = n - 1; j >= 0; --j) {
    const int i = at + j * stride;
    const unsigned int old = r[i];
    carry = umin(im[i], umax(old, carry));
    if (carry != old) { r[i] = (unsigned short)carry; changed = 1; }
  }
}

// launch k of a call
template <int ND>
__global__ __launch_bounds__(BLOCK) void reconstruct_round(Planes q, int k, int Z, int Y, int X, TileGrid g) {
  typedef ReconShape<ND> S;
  constexpr int HX = S::TX + 2, HY = S::TY + 2, HZ = S::TZ + 2 * S::ZH, HN = HX * HY * HZ;
  constexpr int NTILES_AROUND = ND == 2 ? 9 : 27;
  constexpr int NPIX = S::TZ * S::TY * S::TX, SEGS = S::TX / 64;
  __shared__ unsigned short r[HN];
  __shared__ unsigned short im[HN];

  if ((k == 0 ? q.head[1] : q.counters[k - 1]) == 0) return;        // the round before changed no tile: the fixed point is reached
  const unsigned int round = (unsigned int)q.head[0] + (unsigned int)k;
  const bool odd = round & 1u;
  const int* __restrict__ src = odd ? q.wout : q.out;
  int* __restrict__ dst = odd ? q.out : q.wout;
  const unsigned char* __restrict__ fin = odd ? q.flag0 : q.flag1;
  unsigned char* __restrict__ fout = odd ? q.flag1 : q.flag0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  for (long long t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
    const int tx = (int)(t % g.ntx), ty = (int)((t / g.ntx) % g.nty), tz = (int)(t / ((long long)g.ntx * g.nty));
    int active = round == 0;
    if (round != 0 && threadIdx.x < NTILES_AROUND) {
      const int i = threadIdx.x;
      const int nx = tx + i % 3 - 1, ny = ty + (i / 3) % 3 - 1, nz = tz + i / 9 - (ND == 2 ? 0 : 1);
      if ((unsigned int)nx < (unsigned int)g.ntx && (unsigned int)ny < (unsigned int)g.nty && (unsigned int)nz < (unsigned int)g.ntz)
        active = fin[((long long)nz * g.nty + ny) * g.ntx + nx];
    }
    if (!__syncthreads_or(active)) {                      // the barrier also ends the reads of the tile before
      if (threadIdx.x == 0) fout[t] = 0;
      continue;
    }

    const int z0 = tz * S::TZ - S::ZH, y0 = ty * S::TY - 1, x0 = tx * S::TX - 1;
    for (int i = threadIdx.x; i < HN; i += BLOCK) {
      const int hx = i % HX, hy = (i / HX) % HY, hz = i / (HX * HY);
      const int gz = z0 + hz, gy = y0 + hy, gx = x0 + hx;
      unsigned int v = 0, w = 0;
      if ((unsigned int)gz < (unsigned int)Z && (unsigned int)gy < (unsigned int)Y && (unsigned int)gx < (unsigned int)X) {
        const long long p = ((long long)gz * Y + gy) * X + gx;
        w = q.image[p];
        v = umin((unsigned int)src[p], w);
      }
      r[i] = (unsigned short)v;
      im[i] = (unsigned short)w;
    }
    __syncthreads();

    int tile_changed = 0;
    for (int s = 0; s < MAX_SWEEPS; ++s) {
      int changed = 0;
      for (int row = wave; row < S::TZ * S::TY; row += WAVES) {         // +x, -x: a wave owns the row in both
        const int at = ((row / S::TY + S::ZH) * HY + row % S::TY + 1) * HX + 1;
        unsigned int carry = r[at - 1];
#pragma unroll
        for (int seg = 0; seg < SEGS; ++seg) carry = scan_row<true>(r, im, at + seg * 64, lane, carry, changed);
        carry = r[at + S::TX];
#pragma unroll
        for (int seg = SEGS - 1; seg >= 0; --seg) carry = scan_row<false>(r, im, at + seg * 64, lane, carry, changed);
      }
      __syncthreads();
      for (int line = threadIdx.x; line < S::TZ * S::TX; line += BLOCK)   // +y, -y: a thread owns the line in both
        walk_line(r, im, ((line / S::TX + S::ZH) * HY + 1) * HX + line % S::TX + 1, HX, S::TY, changed);
      if (S::ZH) {
        __syncthreads();
        for (int line = threadIdx.x; line < S::TY * S::TX; line += BLOCK)
          walk_line(r, im, (S::ZH * HY + line / S::TX + 1) * HX + line % S::TX + 1, HX * HY, S::TZ, changed);
      }
      if (!__syncthreads_or(changed)) break;
      tile_changed = 1;
    }

    for (int j = threadIdx.x; j < NPIX; j += BLOCK) {
      const int ix = j % S::TX, iy = (j / S::TX) % S::TY, iz = j / (S::TX * S::TY);
      const int gz = tz * S::TZ + iz, gy = ty * S::TY + iy, gx = tx * S::TX + ix;
      if (gz < Z && gy < Y && gx < X) dst[((long long)gz * Y + gy) * X + gx] = (int)r[((iz + S::ZH) * HY + iy + 1) * HX + ix + 1];
    }
    if (threadIdx.x == 0) {
      fout[t] = (unsigned char)tile_changed;
      if (tile_changed) atomicAdd(q.counters + k, 1);
    }
  }
}

// the last launch of a call: info from the counters, and the head for the next call
__global__ void reconstruct_finish(int* __restrict__ head, const int* __restrict__ counters, int rounds, int* __restrict__ info) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int busy = 0;
  for (int k = 0; k < MAX_ROUNDS; ++k)
    if (k < rounds && counters[k] != 0) ++busy;
  info[1] = counters[rounds - 1];
  info[2] = busy;
  head[0] = (int)((unsigned int)head[0] + (unsigned int)rounds);
  head[1] = counters[rounds - 1];
}

inline bool shape_ok(int nd, int Z, int Y, int X) {
  return (nd == 2 || nd == 3) && Z > 0 && Y > 0 && X > 0 && (nd == 3 || Z == 1) &&
         (unsigned __int128)Z * (unsigned)Y * (unsigned)X < ((unsigned __int128)1 << 32);
}

template <int ND, bool DILATE>
void launch_morph(const int* in, const unsigned char* mask, int Z, int Y, int X, int steps, int* out, int* bad, hipStream_t st) {
  const TileGrid g = tile_grid<MorphShape<2>, MorphShape<3>>(ND, Z, Y, X);
  const int grid = (int)(g.ntiles < TILE_MAX_GRID ? g.ntiles : TILE_MAX_GRID);
  grey_morph_kernel<ND, DILATE><<<grid, BLOCK, 0, st>>>(in, mask, Z, Y, X, g, steps, out, bad);
}

}  // namespace

extern "C" int clx_grey_morph(const int32_t* in, const uint8_t* mask, int nd, int Z, int Y, int X, int op, int steps, int32_t* out,
                              int32_t* bad, clx_stream stream) {
  CLX_REQUIRE(in && out && bad, "clx_grey_morph: null pointer");
  CLX_REQUIRE(nd == 2 || nd == 3, "clx_grey_morph: nd must be 2 or 3");
  CLX_REQUIRE(Z > 0 && Y > 0 && X > 0, "clx_grey_morph: bad shape");
  CLX_REQUIRE(nd == 3 || Z == 1, "clx_grey_morph: nd == 2 needs Z == 1");
  CLX_REQUIRE(shape_ok(nd, Z, Y, X), "clx_grey_morph: Z * Y * X must be below 2^32");
  CLX_REQUIRE(op == 0 || op == 1, "clx_grey_morph: op must be 0 (erode) or 1 (dilate)");
  CLX_REQUIRE(steps >= 1 && steps <= (nd == 2 ? MorphShape<2>::HMAX : MorphShape<3>::HMAX),
              "clx_grey_morph: steps must lie in [1, 16] (nd == 3: [1, 4])");
  CLX_REQUIRE(out != in && (const void*)out != (const void*)mask, "clx_grey_morph: out must not alias an input");
  hipStream_t st = (hipStream_t)stream;
  CLX_REQUIRE(hipMemsetAsync(bad, 0, sizeof(int), st) == hipSuccess, "clx_grey_morph: hipMemsetAsync failed");
  if (nd == 2) {
    if (op) launch_morph<2, true>(in, mask, Z, Y, X, steps, out, bad, st);
    else launch_morph<2, false>(in, mask, Z, Y, X, steps, out, bad, st);
  } else {
    if (op) launch_morph<3, true>(in, mask, Z, Y, X, steps, out, bad, st);
    else launch_morph<3, false>(in, mask, Z, Y, X, steps, out, bad, st);
  }
  CLX_CHECK_LAUNCH("clx_grey_morph");
  return CLX_OK;
}

extern "C" size_t clx_grey_reconstruct_workspace(int nd, int Z, int Y, int X) {
  if (!shape_ok(nd, Z, Y, X)) return 0;
  const size_t npix = (size_t)Z * (size_t)Y * (size_t)X;
  const TileGrid g = tile_grid<ReconShape<2>, ReconShape<3>>(nd, Z, Y, X);
  return (size_t)(HEAD_WORDS + MAX_ROUNDS) * sizeof(int) + npix * sizeof(int) + 2 * flag_bytes(g.ntiles) + npix * sizeof(unsigned short);
}

extern "C" int clx_grey_reconstruct(const int32_t* marker, const int32_t* image, const uint8_t* mask, int nd, int Z, int Y, int X,
                                    int rounds, int resume, int32_t* out, int32_t* info, void* workspace, size_t workspace_bytes,
                                    clx_stream stream) {
  CLX_REQUIRE(marker && image && out && info && workspace, "clx_grey_reconstruct: null pointer");
  CLX_REQUIRE(nd == 2 || nd == 3, "clx_grey_reconstruct: nd must be 2 or 3");
  CLX_REQUIRE(Z > 0 && Y > 0 && X > 0, "clx_grey_reconstruct: bad shape");
  CLX_REQUIRE(nd == 3 || Z == 1, "clx_grey_reconstruct: nd == 2 needs Z == 1");
  CLX_REQUIRE(shape_ok(nd, Z, Y, X), "clx_grey_reconstruct: Z * Y * X must be below 2^32");
  CLX_REQUIRE(rounds >= 1 && rounds <= MAX_ROUNDS, "clx_grey_reconstruct: rounds must lie in [1, 64]");
  CLX_REQUIRE(resume == 0 || resume == 1, "clx_grey_reconstruct: resume must be 0 or 1");
  CLX_REQUIRE(workspace_bytes >= clx_grey_reconstruct_workspace(nd, Z, Y, X),
              "clx_grey_reconstruct: workspace_bytes is below clx_grey_reconstruct_workspace(nd, Z, Y, X)");
  CLX_REQUIRE(((uintptr_t)workspace & 3) == 0, "clx_grey_reconstruct: workspace must be 4-byte aligned");
  CLX_REQUIRE(out != marker && out != image && (const void*)out != (const void*)mask, "clx_grey_reconstruct: out must not alias an input");
  const long long npix = (long long)Z * Y * X;
  hipStream_t st = (hipStream_t)stream;
  const TileGrid g = tile_grid<ReconShape<2>, ReconShape<3>>(nd, Z, Y, X);
  Planes q;
  q.out = out;
  q.head = (int*)workspace;
  q.counters = q.head + HEAD_WORDS;
  q.wout = q.counters + MAX_ROUNDS;
  q.flag0 = (unsigned char*)(q.wout + npix);
  q.flag1 = q.flag0 + flag_bytes(g.ntiles);
  q.image = (unsigned short*)(q.flag1 + flag_bytes(g.ntiles));
  CLX_REQUIRE(hipMemsetAsync(info, 0, 3 * sizeof(int), st) == hipSuccess, "clx_grey_reconstruct: hipMemsetAsync failed");
  CLX_REQUIRE(hipMemsetAsync(q.counters, 0, MAX_ROUNDS * sizeof(int), st) == hipSuccess, "clx_grey_reconstruct: hipMemsetAsync failed");
  if (!resume) {
    const long long blocks = (npix + BLOCK - 1) / BLOCK;
    reconstruct_init<<<(int)(blocks < INIT_MAX_GRID ? blocks : INIT_MAX_GRID), BLOCK, 0, st>>>(marker, image, mask, q, npix, info);
  }
  const int grid = (int)(g.ntiles < TILE_MAX_GRID ? g.ntiles : TILE_MAX_GRID);
  for (int k = 0; k < rounds; ++k) {
    if (nd == 2) reconstruct_round<2><<<grid, BLOCK, 0, st>>>(q, k, Z, Y, X, g);
    else reconstruct_round<3><<<grid, BLOCK, 0, st>>>(q, k, Z, Y, X, g);
  }
  reconstruct_finish<<<1, 64, 0, st>>>(q.head, q.counters, rounds, info);
  CLX_CHECK_LAUNCH("clx_grey_reconstruct");
  return CLX_OK;
}
