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
//   planes     between rounds the value lies in an int32 plane; round r reads `out` and writes the workspace's plane if r is
//              even, the other way round if odd.  The image, with the mask and the range applied, lies in the workspace as
//              16-bit words.  The rounds are queued, tiles at rest skipped and the call ended as tile_rounds.h says, where the
//              proof stands that a skipped tile would not have changed.
// Integer minima and maxima only: the same bits and the same rounds in every run.
#include "region_scan.h"
#include "tile_rounds.h"

namespace {

constexpr unsigned int MAX_LEVEL = 65535u;
constexpr int MAX_SWEEPS = 16;          // sweeps of directional scans a tile makes in LDS in one round
constexpr int WAVES = BLOCK / 64;

template <int ND> struct MorphShape;    // the tile of clx_grey_morph and the largest halo: the steps of one launch
template <> struct MorphShape<2> { static constexpr int TZ = 1, TY = 32, TX = 64, ZH = 0, HMAX = 16; };
template <> struct MorphShape<3> { static constexpr int TZ = 8, TY = 8, TX = 32, ZH = 1, HMAX = 4; };
template <int ND> struct ReconShape;    // the tile of clx_grey_reconstruct; TX is a multiple of 64: a wave scans 64 pixels
template <> struct ReconShape<2> { static constexpr int TZ = 1, TY = 32, TX = 256, ZH = 0; };
template <> struct ReconShape<3> { static constexpr int TZ = 8, TY = 8, TX = 64, ZH = 1; };

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
  Rounds w;
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
  if (blockIdx.x == 0 && threadIdx.x == 0) rounds_reset(q.w);
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
  constexpr int NPIX = S::TZ * S::TY * S::TX, SEGS = S::TX / 64;
  __shared__ unsigned short r[HN];
  __shared__ unsigned short im[HN];

  Round rd;
  if (!open_round(q.w, k, rd)) return;
  const int* __restrict__ src = rd.odd ? q.wout : q.out;
  int* __restrict__ dst = rd.odd ? q.out : q.wout;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  for (long long t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
    const int tx = (int)(t % g.ntx), ty = (int)((t / g.ntx) % g.nty), tz = (int)(t / ((long long)g.ntx * g.nty));
    if (!tile_active<ND>(rd, g.ntz, g.nty, g.ntx, t, tz, ty, tx)) continue;

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
    close_tile(q.w, rd, k, t, tile_changed);
  }
}

template <int ND, bool DILATE>
void launch_morph(const int* in, const unsigned char* mask, int Z, int Y, int X, int steps, int* out, int* bad, hipStream_t st) {
  const TileGrid g = tile_grid<MorphShape<2>, MorphShape<3>>(ND, Z, Y, X);
  const int grid = round_grid(g);
  grey_morph_kernel<ND, DILATE><<<grid, BLOCK, 0, st>>>(in, mask, Z, Y, X, g, steps, out, bad);
}

}  // namespace

extern "C" int clx_grey_morph(const int32_t* in, const uint8_t* mask, int nd, int Z, int Y, int X, int op, int steps, int32_t* out,
                              int32_t* bad, clx_stream stream) {
  CLX_REQUIRE(in && out && bad, "clx_grey_morph: null pointer");
  CLX_REQUIRE_MAP(npix, "clx_grey_morph", nd, Z, Y, X, 32);
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
  long long npix;
  if (clx_map_shape(nullptr, nd, Z, Y, X, 32, &npix) != CLX_OK) return 0;
  const TileGrid g = tile_grid<ReconShape<2>, ReconShape<3>>(nd, Z, Y, X);
  return ROUNDS_HEAD_BYTES + (size_t)npix * sizeof(int) + 2 * flag_bytes(g.ntiles) + (size_t)npix * sizeof(unsigned short);
}

extern "C" int clx_grey_reconstruct(const int32_t* marker, const int32_t* image, const uint8_t* mask, int nd, int Z, int Y, int X,
                                    int rounds, int resume, int32_t* out, int32_t* info, void* workspace, size_t workspace_bytes,
                                    clx_stream stream) {
  CLX_REQUIRE(marker && image && out && info && workspace, "clx_grey_reconstruct: null pointer");
  CLX_REQUIRE_MAP(npix, "clx_grey_reconstruct", nd, Z, Y, X, 32);
  CLX_REQUIRE(rounds >= 1 && rounds <= MAX_ROUNDS, "clx_grey_reconstruct: rounds must lie in [1, 64]");
  CLX_REQUIRE(resume == 0 || resume == 1, "clx_grey_reconstruct: resume must be 0 or 1");
  CLX_REQUIRE(workspace_bytes >= clx_grey_reconstruct_workspace(nd, Z, Y, X),
              "clx_grey_reconstruct: workspace_bytes is below clx_grey_reconstruct_workspace(nd, Z, Y, X)");
  CLX_REQUIRE(((uintptr_t)workspace & 3) == 0, "clx_grey_reconstruct: workspace must be 4-byte aligned");
  CLX_REQUIRE(out != marker && out != image && (const void*)out != (const void*)mask, "clx_grey_reconstruct: out must not alias an input");
  hipStream_t st = (hipStream_t)stream;
  const TileGrid g = tile_grid<ReconShape<2>, ReconShape<3>>(nd, Z, Y, X);
  Planes q;
  q.out = out;
  q.wout = rounds_carve(q.w, workspace);
  q.image = (unsigned short*)rounds_carve_flags(q.w, q.wout + npix, g);
  CLX_REQUIRE(rounds_begin(q.w, info, st), "clx_grey_reconstruct: hipMemsetAsync failed");
  if (!resume) reconstruct_init<<<init_grid(npix), BLOCK, 0, st>>>(marker, image, mask, q, npix, info);
  const int grid = round_grid(g);
  for (int k = 0; k < rounds; ++k) {
    if (nd == 2) reconstruct_round<2><<<grid, BLOCK, 0, st>>>(q, k, Z, Y, X, g);
    else reconstruct_round<3><<<grid, BLOCK, 0, st>>>(q, k, Z, Y, X, g);
  }
  rounds_end(q.w, rounds, info, st);
  CLX_CHECK_LAUNCH("clx_grey_reconstruct");
  return CLX_OK;
}
