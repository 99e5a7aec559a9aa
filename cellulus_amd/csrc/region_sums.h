// What the measure stage's value reductions share on top of the reading frame of region_scan.h (region_moments.hip,
// region_coloc.hip, region_weighted.hip, region_border.hip, region_radial.hip, region_order.hip): the checks and the launch
// by type of a raw channel, clx_region_intensity's quantisation of a raw value and its order-preserving keys, a lane's four
// raw values, and the 128-bit sums: __int128 in registers, two 64-bit words (lo, hi), two's
// complement, in LDS and in global memory, where an add is two 64-bit atomic adds: the low limbs first, whose returned old
// value says whether they wrapped, then the high limbs plus that carry.
#pragma once
#include "region_scan.h"

namespace {

typedef __int128 i128;

enum { BAD_LABEL = 1, BAD_VALUE = 2 };

template <typename T> struct alignas(16) Raw4 { T v[PPL]; };

// q of one raw value as clx_region_intensity forms it; false: not finite, or |q| above the bound
template <typename T>
__device__ __forceinline__ bool quantise(T v, int shift, long long bound, long long* q) {
  const double t = rint(ldexp((double)v, shift));       // NaN and ±Inf fail the comparison / exceed the bound
  if (!(fabs(t) <= (double)bound)) return false;        // bound is a power of two: exact as a double
  *q = (long long)t;
  return true;
}
template <>
__device__ __forceinline__ bool quantise<int>(int v, int, long long, long long* q) {
  *q = (long long)v;
  return true;
}

// the keys of clx_region_intensity: unsigned order is the order of the values (-0.0 below +0.0)
__device__ __forceinline__ u64 order_key(float v) {
  const unsigned int b = __float_as_uint(v);
  return (u64)((b & 0x80000000u) ? ~b : (b | 0x80000000u));
}
__device__ __forceinline__ u64 order_key(double v) {
  const u64 b = (u64)__double_as_longlong(v);
  return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ u64 order_key(int v) { return (u64)((unsigned int)v ^ 0x80000000u); }

template <typename T>
__device__ __forceinline__ Raw4<T> load_raw(const T* __restrict__ raw, bool vec, long long p0, long long npix) {
  Raw4<T> rv;
  if (vec && p0 + PPL <= npix) {
    rv = *reinterpret_cast<const Raw4<T>*>(raw + p0);
  } else {
#pragma unroll
    for (int k = 0; k < PPL; ++k) rv.v[k] = p0 + k < npix ? raw[p0 + k] : (T)0;
  }
  return rv;
}

__device__ __forceinline__ i128 shfl_down128(i128 v, int d) {
  const u64 lo = __shfl_down((u64)v, d), hi = __shfl_down((u64)((unsigned __int128)v >> 64), d);
  return (i128)(((unsigned __int128)hi << 64) | lo);
}

// (*lo, *hi) += v modulo 2^128, in LDS or global memory: the returned old low limb tells the carry exactly
__device__ __forceinline__ void add128(u64* lo, u64* hi, i128 v) {
  const u64 vl = (u64)v;
  u64 vh = (u64)((unsigned __int128)v >> 64);
  if (vl) {
    const u64 old = atomicAdd(lo, vl);
    if (old + vl < old) ++vh;                           // the low limbs wrapped (vh may wrap to 0: nothing to add then)
  }
  if (vh) atomicAdd(hi, vh);
}

inline int bit_length(unsigned long long v) {
  int n = 0;
  while (v) { ++n; v >>= 1; }
  return n;
}
// the largest |q| of one pixel: a sum of npix of them stays below 2^62
inline long long value_bound(long long npix) { return (1ll << 62) >> bit_length((unsigned long long)npix); }

// what every entry point that reads a raw channel asks of raw_type and nid
inline int require_raw_channel(const char* who, int raw_type, int nid) {
  CLX_REQUIRE(raw_type >= CLX_RAW_F32 && raw_type <= CLX_RAW_I32, "%s: raw_type must be 0 (f32), 1 (f64) or 2 (i32)", who);
  CLX_REQUIRE(nid >= 1 && nid <= (1 << 24), "%s: nid must lie in [1, 2^24]", who);
  return CLX_OK;
}

// launch(T()) with T the element type that a checked raw_type names
template <typename F>
inline void launch_for_raw(int raw_type, F launch) {
  if (raw_type == CLX_RAW_F32) launch(float());
  else if (raw_type == CLX_RAW_F64) launch(double());
  else launch(int());
}

}  // namespace
