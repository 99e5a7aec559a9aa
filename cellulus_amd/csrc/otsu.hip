// Histogram primitives behind skimage.filters.threshold_otsu as used on the
// std channel (cellulus/detect.py:88-91): min/max of an f64 image and
// numpy.histogram's uniform-bin index computation, reproduced step by step
// (scale, truncate, then the +-1 corrections against the linspace edges) so the
// counts are bit-exact.  Compiled with the default contraction but the index
// expression has no multiply-add pair to fuse.
#include "clx_common.h"

namespace {

// blocks of 256 threads over `work` items, 1 .. cap of them
inline int blocks_of(long long work, int cap) {
  const long long g = (work + 255) / 256;
  return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

typedef double f64x2 __attribute__((ext_vector_type(2)));

// What a lane loads at once: 16 bytes, N elements (8-byte accesses run at 0.54-0.70x the 16-byte rate).  float32 is the
// network's std channel handed over in device memory (cellulus_amd/infer.py::fused_stages): the float64 values the staged
// path reads back from zarr are these floats widened, so min / max / bin of the widened value are the staged path's bits.
template <typename T> struct Vec16;
template <> struct Vec16<double> { typedef f64x2 type; static constexpr int N = 2; };
template <> struct Vec16<float> { typedef f32x4 type; static constexpr int N = 4; };

constexpr int MM_BLOCKS = 512;      // grid cap of the min/max kernel: one pair of partials per block
static_assert(CLX_MINMAX_DOUBLES == 2 + 2 * MM_BLOCKS, "the caller's buffer holds the two results and every block's partials");
constexpr int HIST_BLOCKS = 1024;   // grid cap of the histogram kernel

// Block partials, then one small block over them: no two blocks meet on an address.  (Until round 4 every block ended
// with two float64 atomics on the SAME two words: they are served one after the other at the memory side, ~12 ns each —
// the kernel's time was proportional to its grid, 32 / 61 / 104 / 196 us for 512 / 2048 / 4096 / 8192 blocks over a
// 134-MB image that streams in 25 us.)  mm: [0] min, [1] max, [2 + 2 b], [3 + 2 b] the partials of block b.
template <typename T>
__device__ __forceinline__ void minmax_block_out(T lo, T hi, double* mm) {
  __shared__ double smin[4], smax[4];
  for (int o = 32; o > 0; o >>= 1) {
    // (the shuffles are issued with all lanes active, BEFORE the comparison: inside a conditional expression they would run
    //  under a partial EXEC mask and read zeros from the inactive lanes)
    const T l2 = __shfl_down(lo, o, 64), h2 = __shfl_down(hi, o, 64);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = (double)lo; smax[threadIdx.x >> 6] = (double)hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    mm[2 + 2 * blockIdx.x] = fmin(fmin(smin[0], smin[1]), fmin(smin[2], smin[3]));
    mm[3 + 2 * blockIdx.x] = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
  }
}

__global__ __launch_bounds__(256) void minmax_final(double* mm, int nblocks) {
  __shared__ double smin[4], smax[4];
  double lo = __longlong_as_double(0x7ff0000000000000ll), hi = -lo;
  for (int b = threadIdx.x; b < nblocks; b += 256) { lo = fmin(lo, mm[2 + 2 * b]); hi = fmax(hi, mm[3 + 2 * b]); }
  for (int o = 32; o > 0; o >>= 1) {
    lo = fmin(lo, __shfl_down(lo, o, 64));
    hi = fmax(hi, __shfl_down(hi, o, 64));
  }
  if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    mm[0] = fmin(fmin(smin[0], smin[1]), fmin(smin[2], smin[3]));
    mm[1] = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
  }
}

// min / max of one 16-byte piece folded into the running pair, in the element type (for floats fmin / fmax are the
// float overloads, i.e. fminf / fmaxf: v_min3_f32 / v_max3_f32, no conversion)
template <typename T, typename V>
__device__ __forceinline__ void minmax_piece(const V v, T& lo, T& hi) {
#pragma unroll
  for (int e = 0; e < Vec16<T>::N; ++e) { lo = fmin(lo, v[e]); hi = fmax(hi, v[e]); }
}

// A block reads ONE contiguous range, eight 4-KB pieces of it in flight per round: with the grid-strided walk the
// loads of a thread were 8 MB apart and a 4096^2 image ran at 2.3 TB/s.  The last n % N elements go to block 0's
// first threads.  The reduction runs in T and widens only in minmax_block_out.
template <typename T>
__global__ __launch_bounds__(256) void minmax_kernel(const T* __restrict__ x, long long n, double* mm) {
  typedef typename Vec16<T>::type V;
  constexpr int N = Vec16<T>::N;
  T lo = (T)__builtin_huge_valf(), hi = -lo;
  const long long nv = n / N;
  const V* xv = reinterpret_cast<const V*>(x);
  const long long per_block = (nv + gridDim.x - 1) / gridDim.x;
  const long long b0 = (long long)blockIdx.x * per_block, b1 = b0 + per_block < nv ? b0 + per_block : nv;
  long long i = b0 + threadIdx.x;
  for (; i + 7 * 256 < b1; i += 8 * 256) {
    V v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = xv[i + 256 * u];
#pragma unroll
    for (int u = 0; u < 8; ++u) minmax_piece(v[u], lo, hi);
  }
  for (; i < b1; i += 256) minmax_piece(xv[i], lo, hi);
  if (blockIdx.x == 0 && threadIdx.x < (int)(n % N)) {
    const T t = x[nv * N + threadIdx.x];
    lo = fmin(lo, t);
    hi = fmax(hi, t);
  }
  minmax_block_out(lo, hi, mm);
}

// A thread keeps the bin of its previous value and a count: images are smooth (the std channel of a
// cell image is two plateaus), so consecutive values of a thread mostly share a bin and one LDS
// atomic covers the run — with one atomic per value a two-valued image serialises 64 lanes on two
// addresses.
__device__ __forceinline__ void hist_one(double v, double first, double last, double denom, int nbins,
                                         const double* __restrict__ edges, unsigned int* local, int& cur,
                                         unsigned int& run) {
  if (!(v >= first) || !(v <= last)) return;
  // numpy: idx = int((v - first) / denom * nbins), then the two corrections against the edges — i.e. THE bin with
  // edges[idx] <= v < edges[idx + 1] (last bin closed) for any first guess within one bin of it.  The guess here is a
  // multiplication by nbins / denom (`denom` carries that quotient: the division cost a third of the kernel's
  // instructions), a few ulp from numpy's: the same bin after the corrections.
  int idx = (int)((v - first) * denom);
  idx = min(idx, nbins - 1);
  if (v < edges[idx]) idx -= 1;
  if (v >= edges[idx + 1] && idx != nbins - 1) idx += 1;
  if (idx == cur) {
    ++run;
  } else {
    if (run) atomicAdd(&local[cur], run);
    cur = idx;
    run = 1u;
  }
}

// per-WAVE private histograms in LDS (4 copies) cut the LDS-atomic contention; the bin
// edges are staged in LDS too (the +-1 corrections read them for every element).  Every element is widened to double
// in registers before it is binned.
template <typename T>
__global__ __launch_bounds__(256) void histogram_kernel(const T* __restrict__ x, long long n,
                                                        const double* __restrict__ edges, int nbins,
                                                        unsigned long long* __restrict__ counts) {
  typedef typename Vec16<T>::type V;
  constexpr int N = Vec16<T>::N;
  extern __shared__ unsigned char hist_smem[];
  double* eds = reinterpret_cast<double*>(hist_smem);                       // [nbins + 1]
  unsigned int* local = reinterpret_cast<unsigned int*>(eds + nbins + 1);   // [4][nbins]
  for (int k = threadIdx.x; k <= nbins; k += blockDim.x) eds[k] = edges[k];
  for (int k = threadIdx.x; k < 4 * nbins; k += blockDim.x) local[k] = 0u;
  __syncthreads();
  unsigned int* mine = local + (threadIdx.x >> 6) * nbins;
  const double first = eds[0], last = eds[nbins];
  const double denom = (double)nbins / (last - first);      // (see hist_one)
  const long long nv = n / N;
  const V* xv = reinterpret_cast<const V*>(x);
  int cur = 0;
  unsigned int run = 0u;
  // a block takes ONE contiguous range, four 4-KB pieces of it in flight per round (consecutive values of a thread are
  // then 4 KB apart instead of the whole grid's stride: same plateau, same bin, one LDS atomic per run)
  const long long per_block = (nv + gridDim.x - 1) / gridDim.x;
  const long long b0 = (long long)blockIdx.x * per_block, b1 = b0 + per_block < nv ? b0 + per_block : nv;
  long long i = b0 + threadIdx.x;
  for (; i + 3 * 256 < b1; i += 4 * 256) {
    V v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = xv[i + 256 * u];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < N; ++e) hist_one((double)v[u][e], first, last, denom, nbins, eds, mine, cur, run);
  }
  for (; i < b1; i += 256) {
    const V v = xv[i];
#pragma unroll
    for (int e = 0; e < N; ++e) hist_one((double)v[e], first, last, denom, nbins, eds, mine, cur, run);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)                  // the last n % N elements
    for (long long t = nv * N; t < n; ++t) hist_one((double)x[t], first, last, denom, nbins, eds, mine, cur, run);
  if (run) atomicAdd(&mine[cur], run);
  __syncthreads();
  for (int k = threadIdx.x; k < nbins; k += blockDim.x) {
    const unsigned int c = local[k] + local[nbins + k] + local[2 * nbins + k] + local[3 * nbins + k];
    if (c) atomicAdd(&counts[k], (unsigned long long)c);
  }
}

// the two entry points of each kernel: `who` is the entry's name in its messages
template <typename T>
int minmax_of(const char* who, const T* x, long long n, double* minmax, clx_stream stream) {
  CLX_REQUIRE(x && minmax && n > 0, "%s: bad arguments", who);
  CLX_REQUIRE(((uintptr_t)x & 15) == 0, "%s: x must be 16-byte aligned", who);
  hipStream_t st = (hipStream_t)stream;
  const int g = blocks_of(n / (8 * Vec16<T>::N) + 1, MM_BLOCKS);
  CLX_LAUNCH_KIND(CLX_PROF_MINMAX, minmax_kernel<T>, dim3(g), dim3(256), 0, st, x, n, minmax);
  CLX_LAUNCH_KIND(CLX_PROF_MINMAX, minmax_final, dim3(1), dim3(256), 0, st, minmax, g);
  CLX_CHECK_LAUNCH(who);
  return CLX_OK;
}

template <typename T>
int histogram_of(const char* who, const T* x, long long n, const double* edges, int nbins, long long* counts,
                 clx_stream stream) {
  CLX_REQUIRE(x && edges && counts && n > 0, "%s: bad arguments", who);
  CLX_REQUIRE(nbins > 0 && nbins <= 2048, "%s: nbins must be in 1..2048", who);
  CLX_REQUIRE(((uintptr_t)x & 15) == 0, "%s: x must be 16-byte aligned", who);
  const size_t lds = (size_t)(nbins + 1) * sizeof(double) + (size_t)4 * nbins * sizeof(unsigned int);
  CLX_LAUNCH_KIND(CLX_PROF_HISTOGRAM, histogram_kernel<T>, dim3(blocks_of(n / Vec16<T>::N + 1, HIST_BLOCKS)), dim3(256), lds,
                  (hipStream_t)stream, x, n, edges, nbins, (unsigned long long*)counts);
  CLX_CHECK_LAUNCH(who);
  return CLX_OK;
}

}  // namespace

extern "C" int clx_minmax_f32(const float* x, long long n, double* minmax, clx_stream stream) {
  return minmax_of("clx_minmax_f32", x, n, minmax, stream);
}

extern "C" int clx_minmax_f64(const double* x, long long n, double* minmax, clx_stream stream) {
  return minmax_of("clx_minmax_f64", x, n, minmax, stream);
}

extern "C" int clx_histogram_f32(const float* x, long long n, const double* edges, int nbins,
                                 long long* counts, clx_stream stream) {
  return histogram_of("clx_histogram_f32", x, n, edges, nbins, counts, stream);
}

extern "C" int clx_histogram_f64(const double* x, long long n, const double* edges, int nbins,
                                 long long* counts, clx_stream stream) {
  return histogram_of("clx_histogram_f64", x, n, edges, nbins, counts, stream);
}
