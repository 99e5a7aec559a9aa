// Random crops with the elastic augmentation, a whole batch per call, from a data set that lives on the device: what
// gunpowder's RandomLocation + Normalize + ElasticAugment do in the reference's loader processes
// (cellulus/datasets/zarr_dataset.py:84-131) and ZarrDataset._random_crop / _elastic_crop restate on numpy / scipy.
// The random draws stay on the host (ZarrDataset.elastic_params); this file does the deformation field, the resampling
// and the per-crop maximum of the empty-crop rule.
//   rel_d(voxel) = sum_e A[d][e] (idx_e - (crop_e - 1) / 2) + sum_cp M_0[z][i] M_1[y][j] M_2[x][k] field_d[i][j][k]
// in float64, recomputed wherever it is needed (no coordinate tensor).  Two launches per batch:
//   1. aug_extent_kernel: per crop and axis the min / max of rel_d — wave shuffle, LDS across the waves, one partial per
//      block (min and max do not depend on the order they are taken in);
//   2. aug_sample_kernel: every block reduces its crop's partials again (a few hundred doubles), forms
//      room, the boundary mode and the origin as _elastic_crop does, and resamples: multilinear, float64 weights and sums
//      over the 4 / 8 corners of the float32-normalised source, one rounding to float32.
// The plain crop (elastic_deform = false) is a strided copy with the same normalisation.
// No float atomic adds: the per-crop maximum is an integer atomic max / min on the float's bits (order-free), so the
// same inputs give the same bits.  Built with -ffp-contract=off: both passes must evaluate rel with the same roundings
// (lo <= rel <= hi is what keeps every coordinate inside the source), and the fused multiply-adds are spelled out.
#include "clx_common.h"

namespace {

constexpr int AUG_THREADS = 256;
constexpr int AUG_VPT = 4;             // consecutive x voxels per thread: one 16-byte store per channel
constexpr int AUG_MAX_P1 = 64;         // blocks per crop of the extent pass
constexpr int AUG_MAX_BLOCKS = 2048;   // memory-bound kernels: cap the grid, stride the rest
constexpr size_t AUG_MAX_LDS = 60000;  // bytes of per-axis matrices + one crop's record a block may stage

struct AugP {
  int C, S, B;
  int sp[3], cr[3], cp[3];   // source / crop / control-point extents, indices [0, ND)
  int sp3[3], cr3[3];        // the same padded in front with 1s to (z, y, x): the plain crop is written once for 2-D and 3-D
  int nd;
  int matoff[3];             // start of axis d's (crop_d x cp_d) matrix, in doubles
  int nmat, ncp, stride;     // doubles of all matrices / of one field / of one crop's record
  int xq, items, tiles, p1;  // threads' items per crop row and per crop; blocks per crop of the launch / of the extent pass
  float factor;
  long long vol, nvox;       // voxels per channel of the source / of a crop
};

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// maxima[b] = max(maxima[b], the block's maximum): the block's waves through LDS, then one integer atomic on the
// float's bits (non-negative floats order as ints, negative ones in reverse as unsigned; the slot starts at -inf)
__device__ __forceinline__ void block_max_to(float* slot, float v, float* s_max) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) s_max[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) {
    float m = s_max[0];
    for (int w = 1; w < AUG_THREADS / 64; ++w) m = fmaxf(m, s_max[w]);
    if (__float_as_int(m) >= 0) atomicMax(reinterpret_cast<int*>(slot), __float_as_int(m));
    else atomicMin(reinterpret_cast<unsigned int*>(slot), __float_as_uint(m));
  }
}

// the matrices and the crop's record behind its sample index (A, u, fields) -> LDS
__device__ __forceinline__ void aug_stage(double* sm, const double* mats, const double* rec, const AugP& p) {
  for (int i = threadIdx.x; i < p.nmat; i += AUG_THREADS) sm[i] = mats[i];
  for (int i = threadIdx.x; i < p.stride - 1; i += AUG_THREADS) sm[p.nmat + i] = rec[1 + i];
  __syncthreads();
}

// rel of the item's AUG_VPT voxels (x clamped to the row: the caller drops the lanes beyond it); idx: the item's
// (z, y) or (y) and its first x
template <int ND>
__device__ __forceinline__ void aug_rel(const AugP& p, const double* sm, int item, int* idx, double (*rel)[AUG_VPT]) {
  const int row = item / p.xq, x0 = (item - row * p.xq) * AUG_VPT;
  if (ND == 3) {
    idx[0] = row / p.cr[1];
    idx[1] = row - idx[0] * p.cr[1];
  } else {
    idx[0] = row;
  }
  idx[ND - 1] = x0;
  const double* A = sm + p.nmat;
  const double* fields = A + ND * ND + ND;
  const double* M0 = sm + p.matoff[0] + idx[0] * p.cp[0];
  const double* M1 = ND == 3 ? sm + p.matoff[1] + idx[1] * p.cp[1] : nullptr;
  const double* MX = sm + p.matoff[ND - 1];
  const int cpx = p.cp[ND - 1], W = p.cr[ND - 1];
  int xv[AUG_VPT];
#pragma unroll
  for (int v = 0; v < AUG_VPT; ++v) xv[v] = x0 + v < W ? x0 + v : W - 1;
  double r0[ND];
#pragma unroll
  for (int e = 0; e + 1 < ND; ++e) r0[e] = (double)idx[e] - ((double)p.cr[e] - 1.0) / 2.0;
#pragma unroll
  for (int d = 0; d < ND; ++d) {
    const double* f = fields + d * p.ncp;
    double acc[AUG_VPT];
#pragma unroll
    for (int v = 0; v < AUG_VPT; ++v) acc[v] = 0.0;
    // axis by axis, as the host path up-samples: the leading axes first (shared by the item's voxels), x last
    for (int k = 0; k < cpx; ++k) {
      double t = 0.0;
      if (ND == 3) {
        for (int j = 0; j < p.cp[1]; ++j) {
          double u = 0.0;
          for (int i = 0; i < p.cp[0]; ++i) u = fma(M0[i], f[(i * p.cp[1] + j) * cpx + k], u);
          t = fma(M1[j], u, t);
        }
      } else {
        for (int i = 0; i < p.cp[0]; ++i) t = fma(M0[i], f[i * cpx + k], t);
      }
#pragma unroll
      for (int v = 0; v < AUG_VPT; ++v) acc[v] = fma(MX[xv[v] * cpx + k], t, acc[v]);
    }
#pragma unroll
    for (int v = 0; v < AUG_VPT; ++v) {
      double r = 0.0;
#pragma unroll
      for (int e = 0; e + 1 < ND; ++e) r += A[d * ND + e] * r0[e];
      r += A[d * ND + ND - 1] * ((double)xv[v] - ((double)W - 1.0) / 2.0);
      rel[d][v] = r + acc[v];
    }
  }
}

template <int ND>
__global__ __launch_bounds__(AUG_THREADS) void aug_extent_kernel(const double* __restrict__ params,
                                                                  const double* __restrict__ mats,
                                                                  double* __restrict__ partial, const AugP p) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ double red[AUG_THREADS / 64][2 * ND];
  const int b = blockIdx.x / p.p1, t = blockIdx.x - b * p.p1;
  aug_stage(sm, mats, params + (size_t)b * p.stride, p);
  double lo[ND], hi[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) {
    lo[d] = __builtin_inf();
    hi[d] = -__builtin_inf();
  }
  const int W = p.cr[ND - 1];
  for (int item = t * AUG_THREADS + threadIdx.x; item < p.items; item += p.p1 * AUG_THREADS) {
    int idx[ND];
    double rel[ND][AUG_VPT];
    aug_rel<ND>(p, sm, item, idx, rel);
#pragma unroll
    for (int d = 0; d < ND; ++d)
#pragma unroll
      for (int v = 0; v < AUG_VPT; ++v)
        if (idx[ND - 1] + v < W) {
          lo[d] = fmin(lo[d], rel[d][v]);
          hi[d] = fmax(hi[d], rel[d][v]);
        }
  }
#pragma unroll
  for (int d = 0; d < ND; ++d) {
    lo[d] = wave_min(lo[d]);
    hi[d] = wave_max(hi[d]);
  }
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) {
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      red[tid >> 6][d] = lo[d];
      red[tid >> 6][ND + d] = hi[d];
    }
  }
  __syncthreads();
  if (tid < 2 * ND) {
    double v = red[0][tid];
    for (int w = 1; w < AUG_THREADS / 64; ++w) v = tid < ND ? fmin(v, red[w][tid]) : fmax(v, red[w][tid]);
    partial[((size_t)b * p.p1 + t) * 2 * ND + tid] = v;
  }
}

// scipy's half-sample-symmetric `reflect` at order 1: the coordinate first ...
__device__ __forceinline__ double reflect_coord(double x, int n) {
  const double two_n = 2.0 * n;
  double y = fmod(x + 0.5, two_n);
  if (y < 0.0) y += two_n;
  if (y > (double)n) y = two_n - y;
  return y - 0.5;
}
// ... then every corner index
__device__ __forceinline__ long long reflect_index(long long i, int n) {
  long long m = i % (2LL * n);
  if (m < 0) m += 2LL * n;
  return m >= n ? 2LL * n - 1 - m : m;
}

template <int ND, typename T>
__global__ __launch_bounds__(AUG_THREADS) void aug_sample_kernel(const T* __restrict__ data,
                                                                  const double* __restrict__ params,
                                                                  const double* __restrict__ mats,
                                                                  const double* __restrict__ partial,
                                                                  float* __restrict__ raw, float* __restrict__ maxima,
                                                                  const AugP p) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ double s_origin[ND];
  __shared__ int s_room_ok[4];
  __shared__ float s_max[AUG_THREADS / 64];
  const int b = blockIdx.x / p.tiles, t = blockIdx.x - b * p.tiles;
  const int tid = threadIdx.x;
  const double* rec = params + (size_t)b * p.stride;
  aug_stage(sm, mats, rec, p);
  if (tid < ND) {
    double lo = __builtin_inf(), hi = -__builtin_inf();
    for (int j = 0; j < p.p1; ++j) {
      lo = fmin(lo, partial[((size_t)b * p.p1 + j) * 2 * ND + tid]);
      hi = fmax(hi, partial[((size_t)b * p.p1 + j) * 2 * ND + ND + tid]);
    }
    const double room = ((double)p.sp[tid] - 1.0) - (hi - lo);
    const double u = sm[p.nmat + ND * ND + tid];
    s_room_ok[tid] = room >= 0.0;
    s_origin[tid] = u * (room > 0.0 ? room : 0.0) - lo;
  }
  __syncthreads();
  bool constant = true;
  double origin[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) {
    constant = constant && s_room_ok[d];
    origin[d] = s_origin[d];
  }
  long long s = (long long)rec[0];
  s = s < 0 ? 0 : (s >= p.S ? p.S - 1 : s);          // (the binding checks the range; never read outside the data set)
  const T* src = data + s * p.C * p.vol;
  float* dst = raw + (size_t)b * p.C * p.nvox;
  const int W = p.cr[ND - 1];
  const bool vec = (W & 3) == 0;
  float vmax = -__builtin_inff();
  for (int item = t * AUG_THREADS + tid; item < p.items; item += p.tiles * AUG_THREADS) {
    int idx[ND];
    double rel[ND][AUG_VPT];
    aug_rel<ND>(p, sm, item, idx, rel);
    int off[AUG_VPT][1 << ND];             // within one channel of one sample: below 2^31 (checked at the entry)
    double wgt[AUG_VPT][1 << ND];
#pragma unroll
    for (int v = 0; v < AUG_VPT; ++v) {
      int ci[ND][2];
      double cw[ND][2];
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        const int n = p.sp[d];
        double c = rel[d][v] + origin[d];
        if (!constant) c = reflect_coord(c, n);
        const double fl = floor(c);
        const double tt = c - fl;
        const long long i0 = (long long)fl;
        cw[d][0] = 1.0 - tt;
        cw[d][1] = tt;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          long long i = i0 + k;
          if (constant) {
            if (i < 0 || i >= n) cw[d][k] = 0.0;     // cval = 0
            i = i < 0 ? 0 : (i >= n ? n - 1 : i);
          } else {
            i = reflect_index(i, n);
          }
          ci[d][k] = (int)i;
        }
      }
#pragma unroll
      for (int k = 0; k < (1 << ND); ++k) {
        // corner k: bit (ND - 1 - d) picks the upper neighbour along axis d — the last axis runs fastest
        int o = 0;
        double w = 1.0;
#pragma unroll
        for (int d = 0; d < ND; ++d) {
          const int bit = (k >> (ND - 1 - d)) & 1;
          o = o * p.sp[d] + ci[d][bit];
          w = w * cw[d][bit];
        }
        off[v][k] = o;
        wgt[v][k] = w;
      }
    }
    long long o_out = 0;
#pragma unroll
    for (int d = 0; d < ND; ++d) o_out = o_out * p.cr[d] + idx[d];
    for (int c = 0; c < p.C; ++c) {
      const T* ch = src + (long long)c * p.vol;
      float res[AUG_VPT];
#pragma unroll
      for (int v = 0; v < AUG_VPT; ++v) {
        double sum = 0.0;
#pragma unroll
        for (int k = 0; k < (1 << ND); ++k) {
          const float val = (float)ch[off[v][k]] * p.factor;      // normalised in float32 before it is interpolated
          sum += wgt[v][k] * (double)val;
        }
        res[v] = (float)sum;
      }
      float* o = dst + (long long)c * p.nvox + o_out;
      if (vec) {
        f32x4 q = {res[0], res[1], res[2], res[3]};
        *reinterpret_cast<f32x4*>(o) = q;
#pragma unroll
        for (int v = 0; v < AUG_VPT; ++v) vmax = fmaxf(vmax, res[v]);
      } else {
#pragma unroll
        for (int v = 0; v < AUG_VPT; ++v)
          if (idx[ND - 1] + v < W) {
            o[v] = res[v];
            vmax = fmaxf(vmax, res[v]);
          }
      }
    }
  }
  block_max_to(maxima + b, vmax, s_max);
}

// raw[b][c] = float32(data[s][c][offset + (z, y, x)]) * factor
template <typename T>
__global__ __launch_bounds__(AUG_THREADS) void aug_plain_kernel(const T* __restrict__ data,
                                                                 const double* __restrict__ params,
                                                                 float* __restrict__ raw, float* __restrict__ maxima,
                                                                 const AugP p) {
  __shared__ float s_max[AUG_THREADS / 64];
  const int b = blockIdx.x / p.tiles, t = blockIdx.x - b * p.tiles;
  const double* rec = params + (size_t)b * p.stride;
  long long s = (long long)rec[0];
  s = s < 0 ? 0 : (s >= p.S ? p.S - 1 : s);
  int o3[3] = {0, 0, 0};
  for (int d = 0; d < p.nd; ++d) {
    const int a = 3 - p.nd + d;
    long long o = (long long)rec[1 + d];
    const int room = p.sp3[a] - p.cr3[a];
    o3[a] = (int)(o < 0 ? 0 : (o > room ? room : o));   // never read outside the data set
  }
  const int W = p.cr3[2];
  const bool vec = (W & 3) == 0;
  const T* src = data + s * p.C * p.vol;
  float* dst = raw + (size_t)b * p.C * p.nvox;
  float vmax = -__builtin_inff();
  const int per_channel = p.items;
  const long long total = (long long)per_channel * p.C;
  for (long long it = (long long)t * AUG_THREADS + threadIdx.x; it < total; it += (long long)p.tiles * AUG_THREADS) {
    const int c = (int)(it / per_channel);
    const int item = (int)(it - (long long)c * per_channel);
    const int row = item / p.xq, x0 = (item - row * p.xq) * AUG_VPT;
    const int z = row / p.cr3[1], y = row - z * p.cr3[1];
    const T* in = src + (long long)c * p.vol + ((long long)(z + o3[0]) * p.sp3[1] + (y + o3[1])) * p.sp3[2] + o3[2] + x0;
    float* o = dst + (long long)c * p.nvox + (long long)row * W + x0;
    float res[AUG_VPT];
#pragma unroll
    for (int v = 0; v < AUG_VPT; ++v) res[v] = x0 + v < W ? (float)in[v] * p.factor : -__builtin_inff();
    if (vec) {
      f32x4 q = {res[0], res[1], res[2], res[3]};
      *reinterpret_cast<f32x4*>(o) = q;
    } else {
#pragma unroll
      for (int v = 0; v < AUG_VPT; ++v)
        if (x0 + v < W) o[v] = res[v];
    }
#pragma unroll
    for (int v = 0; v < AUG_VPT; ++v) vmax = fmaxf(vmax, res[v]);
  }
  block_max_to(maxima + b, vmax, s_max);
}

int extent_blocks(long long items) {
  const long long want = (items + 2 * AUG_THREADS - 1) / (2 * AUG_THREADS);
  return (int)(want < 1 ? 1 : (want > AUG_MAX_P1 ? AUG_MAX_P1 : want));
}

template <int ND, typename T>
void launch_elastic(const void* data, const double* params, const double* mats, double* partial, float* raw,
                    float* maxima, const AugP& p, size_t lds, hipStream_t st) {
  aug_extent_kernel<ND><<<dim3((unsigned)(p.B * p.p1)), AUG_THREADS, lds, st>>>(params, mats, partial, p);
  aug_sample_kernel<ND, T><<<dim3((unsigned)(p.B * p.tiles)), AUG_THREADS, lds, st>>>(
      static_cast<const T*>(data), params, mats, partial, raw, maxima, p);
}

template <typename T>
void launch_typed(const void* data, int elastic, const double* params, const double* mats, double* partial, float* raw,
                  float* maxima, const AugP& p, size_t lds, hipStream_t st) {
  if (!elastic)
    aug_plain_kernel<T><<<dim3((unsigned)(p.B * p.tiles)), AUG_THREADS, 0, st>>>(static_cast<const T*>(data), params,
                                                                                  raw, maxima, p);
  else if (p.nd == 2) launch_elastic<2, T>(data, params, mats, partial, raw, maxima, p, lds, st);
  else launch_elastic<3, T>(data, params, mats, partial, raw, maxima, p, lds, st);
}

}  // namespace

extern "C" size_t clx_elastic_crop_workspace(int nd, const int* crop, int B) {
  if ((nd != 2 && nd != 3) || !crop || B < 1) return 0;
  long long rows = 1;
  for (int d = 0; d + 1 < nd; ++d) rows *= crop[d] > 0 ? crop[d] : 1;
  const long long items = rows * ((crop[nd - 1] + AUG_VPT - 1) / AUG_VPT);
  return (size_t)B * extent_blocks(items) * 2 * nd * sizeof(double);
}

extern "C" int clx_elastic_crop(const void* data, int dtype, int S, int C, int nd, const int* spatial, const int* crop,
                                const int* cp_shape, float factor, int elastic, int B, const double* params,
                                const double* mats, void* workspace, float* raw, float* maxima, clx_stream stream) {
  CLX_REQUIRE(data && spatial && crop && params && raw && maxima, "clx_elastic_crop: null pointer");
  CLX_REQUIRE(nd == 2 || nd == 3, "clx_elastic_crop: 2 or 3 spatial dimensions (nd = %d)", nd);
  CLX_REQUIRE(dtype == CLX_AUG_U8 || dtype == CLX_AUG_U16 || dtype == CLX_AUG_F32,
              "clx_elastic_crop: element type %d is not uint8 (0), uint16 (1) or float32 (2)", dtype);
  CLX_REQUIRE(B >= 1 && B <= 65535, "clx_elastic_crop: need 1 <= B <= 65535 crops (B = %d)", B);
  CLX_REQUIRE(S >= 1 && C >= 1, "clx_elastic_crop: need S >= 1 samples and C >= 1 channels (S = %d, C = %d)", S, C);
  CLX_REQUIRE(!elastic || (cp_shape && mats && workspace),
              "clx_elastic_crop: null pointer (the elastic crop needs cp_shape, mats and workspace)");
  const int esize = dtype == CLX_AUG_U8 ? 1 : (dtype == CLX_AUG_U16 ? 2 : 4);
  // (rows of whole 16-byte groups are stored as such; with crop[nd - 1] % 4 == 0 every crop of an aligned batch is aligned)
  CLX_REQUIRE(((uintptr_t)data & (esize - 1)) == 0 && ((uintptr_t)raw & (crop[nd - 1] % 4 == 0 ? 15 : 3)) == 0 &&
                  ((uintptr_t)maxima & 3) == 0 && ((uintptr_t)params & 7) == 0 && ((uintptr_t)mats & 7) == 0 &&
                  ((uintptr_t)workspace & 7) == 0,
              "clx_elastic_crop: data must be aligned to its element, raw to 16 bytes (4 when the last crop extent is "
              "not a multiple of 4), maxima to 4, params / mats / workspace to 8");
  AugP p{};
  p.C = C; p.S = S; p.B = B; p.nd = nd; p.factor = factor;
  p.vol = 1; p.nvox = 1; p.ncp = 1; p.nmat = 0;
  for (int a = 0; a < 3; ++a) p.sp3[a] = p.cr3[a] = 1;
  long long rows = 1;
  for (int d = 0; d < nd; ++d) {
    CLX_REQUIRE(crop[d] >= 1 && spatial[d] >= 1 && crop[d] <= (1 << 20) && spatial[d] <= (1 << 20),
                "clx_elastic_crop: crop and data set extents must be in [1, 2^20] (axis %d: %d, %d)", d, crop[d], spatial[d]);
    CLX_REQUIRE(elastic || crop[d] <= spatial[d], "clx_elastic_crop: the plain crop must fit the data set (axis %d: %d > %d)",
                d, crop[d], spatial[d]);
    p.sp[d] = p.sp3[3 - nd + d] = spatial[d];
    p.cr[d] = p.cr3[3 - nd + d] = crop[d];
    p.vol *= spatial[d];
    p.nvox *= crop[d];
    if (d + 1 < nd) rows *= crop[d];
    if (elastic) {
      CLX_REQUIRE(cp_shape[d] >= 1 && cp_shape[d] <= 4096, "clx_elastic_crop: control-point extents must be in [1, 4096] (axis %d: %d)",
                  d, cp_shape[d]);
      p.cp[d] = cp_shape[d];
      p.matoff[d] = p.nmat;
      CLX_REQUIRE((long long)p.nmat + (long long)crop[d] * cp_shape[d] < (1 << 24) && (long long)p.ncp * cp_shape[d] < (1 << 24),
                  "clx_elastic_crop: too many control points");
      p.nmat += crop[d] * cp_shape[d];
      p.ncp *= cp_shape[d];
    }
  }
  p.xq = (crop[nd - 1] + AUG_VPT - 1) / AUG_VPT;
  CLX_REQUIRE(rows * p.xq < (1LL << 30) && p.vol < (1LL << 31) && p.nvox < (1LL << 31),
              "clx_elastic_crop: crop or data set too large (2^31 voxels per channel at most)");
  p.items = (int)(rows * p.xq);
  p.stride = elastic ? 1 + nd * nd + nd + nd * p.ncp : 1 + nd;
  const size_t lds = elastic ? (size_t)(p.nmat + p.stride - 1) * sizeof(double) : 0;
  CLX_REQUIRE(lds <= AUG_MAX_LDS,
              "clx_elastic_crop: the up-sampling matrices and one crop's control points take %zu bytes of LDS (limit %zu): "
              "use a larger control_point_spacing", lds, AUG_MAX_LDS);
  p.p1 = extent_blocks(p.items);
  const long long work = elastic ? p.items : (long long)p.items * C;
  const long long cap = AUG_MAX_BLOCKS / B > 1 ? AUG_MAX_BLOCKS / B : 1;
  const long long want = (work + AUG_THREADS - 1) / AUG_THREADS;
  p.tiles = (int)(want < cap ? want : cap);
  hipStream_t st = (hipStream_t)stream;
  // every crop's maximum starts at -inf
  hipError_t e = hipMemsetD32Async((hipDeviceptr_t)maxima, (int)0xFF800000u, (size_t)B, st);
  if (e != hipSuccess) {
    clx_set_error("clx_elastic_crop: hipMemsetD32Async failed: %s", hipGetErrorString(e));
    return CLX_ERR_LAUNCH;
  }
  double* partial = static_cast<double*>(workspace);
  switch (dtype) {
    case CLX_AUG_U8: launch_typed<uint8_t>(data, elastic, params, mats, partial, raw, maxima, p, lds, st); break;
    case CLX_AUG_U16: launch_typed<uint16_t>(data, elastic, params, mats, partial, raw, maxima, p, lds, st); break;
    default: launch_typed<float>(data, elastic, params, mats, partial, raw, maxima, p, lds, st); break;
  }
  CLX_CHECK_LAUNCH("clx_elastic_crop");
  return CLX_OK;
}
