// Data gradient of the network's first convolution (raw image -> num_fmaps, valid 3x3 / 3x3x3, 1-4 input channels) with
// respect to the raw image: what autograd of nn.Conv{2,3}d(in_channels, num_fmaps, 3) in l_conv.0.conv_pass.0
// (cellulus/models/unet.py:24-51) leaves in raw.grad.
//   dx[b][c][z][y][x] = sum over taps (kz, ky, kx) and n < N of w[n][c][kz][ky][kx] * dy[(b, z-kz, y-ky, x-kx)][n]
// (taps that fall outside dY are dropped).  Two steps per workgroup:
//   1. for every dY pixel of a halo patch, the F = cin * KD * 9 dot products Z[p][c][tap] = sum_n dy[p][n] w[n][c][tap]:
//      the patch's dY rows pass through LDS in chunks of 32 channels (16 bytes per lane, eight lanes on one row's 128-byte
//      run), each thread contracts one pixel's row with the weights, which are the same for the whole wavefront (scalar
//      loads, not LDS);
//   2. the col2im gather dx[q][c] = sum_tap Z[q - tap][c][tap] out of LDS.
// A workgroup owns a TY x TX tile of dx in (y, x) and a run of dx planes in z.  It walks the dY planes in order and keeps the
// partial sums of the KD dx planes each dY plane feeds in registers, so a dY plane is contracted once per tile plus the
// two-pixel halo in y and x.  Every dx element is written once, by one thread, its sums taken in a fixed order: no
// atomics, bit-reproducible.
#include "clx_common.h"

namespace {

constexpr int FD_NC = 32;            // dY channels per staged chunk
constexpr int FD_LDP = FD_NC + 4;    // padded LDS row: the 16 lanes of a ds_read_b128 group hit distinct banks
constexpr int FD_ZMAX = 6144;        // floats of Z per workgroup (24 KB): two workgroups per CU with the staging rows
constexpr int FD_PPT = 2;            // dx pixels per thread: tiles of at most 512 pixels

struct FirstDgradP {
  long long ld_dy;
  int N, OD, OH, OW, D, H, W;
  int TY, TX, PW, npatch, tiles_x, zc;
};

template <int CIN, int KD>
__global__ __launch_bounds__(256) void conv_first_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                                 float* __restrict__ dx, const FirstDgradP p) {
  constexpr int T = KD * 9, F = CIN * T;
  __shared__ float Ls[256 * FD_LDP];
  extern __shared__ float Zs[];        // [npatch][F]
  const int tid = threadIdx.x;
  const int b = blockIdx.z;
  const int y0 = (int)(blockIdx.x / p.tiles_x) * p.TY, x0 = (int)(blockIdx.x % p.tiles_x) * p.TX;
  const int zs = blockIdx.y * p.zc;
  const int ze = zs + p.zc < p.D ? zs + p.zc : p.D;
  const int nchunks = (p.N + FD_NC - 1) / FD_NC;
  const int q = tid & 7;               // staging role: channel quad q of pixels (tid >> 3) + 32 j
  float acc[KD][FD_PPT][CIN];
#pragma unroll
  for (int k = 0; k < KD; ++k)
#pragma unroll
    for (int i = 0; i < FD_PPT; ++i)
#pragma unroll
      for (int c = 0; c < CIN; ++c) acc[k][i][c] = 0.f;

  for (int zp = zs - (KD - 1); zp < ze; ++zp) {
    if (zp >= 0 && zp < p.OD) {
      // ---- 1. Z of the patch of dY plane zp, 256 pixels at a time
      for (int p0 = 0; p0 < p.npatch; p0 += 256) {
        long long row[8];              // dY row of each staged pixel, -1 outside dY
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int pix = p0 + (tid >> 3) + 32 * j;
          const int r = pix / p.PW, s = pix - r * p.PW;
          const int y = y0 - 2 + r, x = x0 - 2 + s;
          row[j] = (pix < p.npatch && y >= 0 && y < p.OH && x >= 0 && x < p.OW)
                       ? ((((long long)b * p.OD + zp) * p.OH + y) * p.OW + x) * p.ld_dy
                       : -1;
        }
        f32x4 pre[8];
        auto load = [&](int n0) {
          const int n = n0 + q * 4;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (row[j] >= 0 && n < p.N) {
              v = *reinterpret_cast<const f32x4*>(dy + row[j] + n);
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (n + e >= p.N) v[e] = 0.f;     // the pad lanes of dY are not guaranteed zero
            }
            pre[j] = v;
          }
        };
        load(0);
        float z[F];
#pragma unroll
        for (int f = 0; f < F; ++f) z[f] = 0.f;
        for (int ch = 0; ch < nchunks; ++ch) {
          __syncthreads();
#pragma unroll
          for (int j = 0; j < 8; ++j)
            *reinterpret_cast<f32x4*>(&Ls[((tid >> 3) + 32 * j) * FD_LDP + q * 4]) = pre[j];
          __syncthreads();
          const int n0 = ch * FD_NC;
          if (ch + 1 < nchunks) load(n0 + FD_NC);        // the next chunk's loads run under this chunk's FMAs
          const int nc = p.N - n0 < FD_NC ? p.N - n0 : FD_NC;
          const float* lrow = &Ls[tid * FD_LDP];
          const float* wr = w + (size_t)n0 * F;
#pragma unroll 4
          for (int k = 0; k < nc; ++k) {
            const float v = lrow[k];
#pragma unroll
            for (int f = 0; f < F; ++f) z[f] = fmaf(v, wr[k * F + f], z[f]);
          }
        }
        const int pix = p0 + tid;
        if (pix < p.npatch) {
#pragma unroll
          for (int f = 0; f < F; ++f) Zs[pix * F + f] = z[f];
        }
      }
      __syncthreads();
      // ---- 2. gather: the dx pixels of the tile, kz by kz into the partial sums of dx planes zp + kz
#pragma unroll
      for (int i = 0; i < FD_PPT; ++i) {
        const int t = tid + 256 * i;
        if (t < p.TY * p.TX) {
          const int ty = t / p.TX, tx = t - ty * p.TX;
#pragma unroll
          for (int c = 0; c < CIN; ++c)
#pragma unroll
            for (int kz = 0; kz < KD; ++kz) {
              float s = 0.f;
#pragma unroll
              for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
                  s += Zs[((ty + 2 - ky) * p.PW + tx + 2 - kx) * F + c * T + kz * 9 + ky * 3 + kx];
              acc[kz][i][c] += s;
            }
        }
      }
      // (the next plane's first write of Zs follows at least one barrier of its chunk loop)
    }
    // dx plane zp has all its terms now (dY planes zp - KD + 1 .. zp)
    if (zp >= zs) {
#pragma unroll
      for (int i = 0; i < FD_PPT; ++i) {
        const int t = tid + 256 * i;
        if (t < p.TY * p.TX) {
          const int ty = t / p.TX, tx = t - ty * p.TX;
          const int y = y0 + ty, x = x0 + tx;
          if (y < p.H && x < p.W) {
#pragma unroll
            for (int c = 0; c < CIN; ++c)
              dx[((((long long)b * CIN + c) * p.D + zp) * p.H + y) * p.W + x] = acc[0][i][c];
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k + 1 < KD; ++k)
#pragma unroll
      for (int i = 0; i < FD_PPT; ++i)
#pragma unroll
        for (int c = 0; c < CIN; ++c) acc[k][i][c] = acc[k + 1][i][c];
#pragma unroll
    for (int i = 0; i < FD_PPT; ++i)
#pragma unroll
      for (int c = 0; c < CIN; ++c) acc[KD - 1][i][c] = 0.f;
  }
}

// The TY x TX tile that computes the fewest patch pixels per dx pixel over the whole image (ties: the larger tile):
// at most 512 dx pixels and a patch of at most FD_ZMAX floats of Z
void pick_tile(int F, int H, int W, int& TY, int& TX) {
  double best = -1.0;
  TY = TX = 1;
  for (int ty = 1; ty <= 64; ++ty) {
    for (int tx = 1; tx <= 128; ++tx) {
      if (ty * tx > 256 * FD_PPT || (ty + 2) * (tx + 2) * F > FD_ZMAX) break;
      const double tiles = (double)((H + ty - 1) / ty) * ((W + tx - 1) / tx);
      const double score = (double)H * W / (tiles * (ty + 2) * (tx + 2));
      if (score > best + 1e-12 || (score > best - 1e-12 && ty * tx > TY * TX)) {
        best = score;
        TY = ty;
        TX = tx;
      }
    }
  }
}

template <int CIN>
void launch_first_dgrad(int KD, dim3 grid, size_t lds, hipStream_t st, const float* dy, const float* w, float* dx,
                        const FirstDgradP& p) {
  if (KD == 1) conv_first_dgrad_kernel<CIN, 1><<<grid, 256, lds, st>>>(dy, w, dx, p);
  else conv_first_dgrad_kernel<CIN, 3><<<grid, 256, lds, st>>>(dy, w, dx, p);
}

}  // namespace

extern "C" int clx_conv_first_dgrad(const float* dy, int ld_dy, const float* w, int N, int cin, int B, int OD, int OH,
                                    int OW, int KD, float* dx, clx_stream stream) {
  CLX_REQUIRE(dy && w && dx, "clx_conv_first_dgrad: null pointer");
  CLX_REQUIRE(((uintptr_t)dy & 15) == 0 && ((uintptr_t)w & 3) == 0 && ((uintptr_t)dx & 3) == 0,
              "clx_conv_first_dgrad: dy must be 16-byte aligned, w and dx 4-byte aligned");
  CLX_REQUIRE(cin >= 1 && cin <= 4, "clx_conv_first_dgrad: 1 to 4 input channels (got %d)", cin);
  CLX_REQUIRE(KD == 1 || KD == 3, "clx_conv_first_dgrad: a 3x3 or 3x3x3 kernel (KD = %d)", KD);
  CLX_REQUIRE(N >= 1 && ld_dy >= N && ld_dy % 4 == 0,
              "clx_conv_first_dgrad: need N >= 1, ld_dy >= N and ld_dy %% 4 == 0 (N = %d, ld_dy = %d)", N, ld_dy);
  CLX_REQUIRE(B >= 1 && B <= 65535 && OD >= 1 && OH >= 1 && OW >= 1, "clx_conv_first_dgrad: bad extents");
  const int D = OD + KD - 1, H = OH + 2, W = OW + 2;
  const int F = cin * KD * 9;
  FirstDgradP p{};
  p.ld_dy = ld_dy;
  p.N = N; p.OD = OD; p.OH = OH; p.OW = OW; p.D = D; p.H = H; p.W = W;
  pick_tile(F, H, W, p.TY, p.TX);
  p.PW = p.TX + 2;
  p.npatch = (p.TY + 2) * p.PW;
  p.tiles_x = cdiv(W, p.TX);
  const long long tiles = (long long)cdiv(H, p.TY) * p.tiles_x;
  CLX_REQUIRE(tiles < (1LL << 31), "clx_conv_first_dgrad: image too large");
  // runs of dx planes per workgroup: the whole depth where that gives two rounds of workgroups, else shorter runs (each
  // re-contracts KD - 1 dY planes)
  int zc = D;
  while (zc > 4 && tiles * B * cdiv(D, zc) < 512) zc = (zc + 1) / 2;
  p.zc = zc;
  const dim3 grid((unsigned)tiles, (unsigned)cdiv(D, zc), (unsigned)B);
  const size_t lds = (size_t)p.npatch * F * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  switch (cin) {
    case 1: launch_first_dgrad<1>(KD, grid, lds, st, dy, w, dx, p); break;
    case 2: launch_first_dgrad<2>(KD, grid, lds, st, dy, w, dx, p); break;
    case 3: launch_first_dgrad<3>(KD, grid, lds, st, dy, w, dx, p); break;
    default: launch_first_dgrad<4>(KD, grid, lds, st, dy, w, dx, p); break;
  }
  CLX_CHECK_LAUNCH("clx_conv_first_dgrad");
  return CLX_OK;
}
