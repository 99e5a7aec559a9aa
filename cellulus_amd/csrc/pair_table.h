// The pair table the measure stage's SETS of id pairs are gathered in (region_contacts.hip: clx_region_contacts; label_overlap.hip:
// clx_label_overlaps), on top of the reading frame of region_scan.h: an open-addressing table in global memory keyed by a
// 64-bit pair (never 0), filled through a block-private table in LDS that is flushed once.  A pair that finds no slot in
// LDS goes straight to the global table; a pair that finds none there within `probes` tries sets bit 2 of info[0] and is
// dropped, and the caller discards the table.  What a pair's word gathers is the table's combining operation: the sum of
// the counts (PairAdd: contacts, overlaps) or the largest value (PairMax: label_basins.hip's passes).
#pragma once
#include "region_scan.h"

namespace {

constexpr int CSLOTS = 512;             // pairs a block keeps in LDS (power of two)
constexpr int CPROBES = 8;
constexpr unsigned int GPROBES = 4096;  // slots tried in the global table before the result is declared lost

struct ContactsOut {
  u64* keys;
  u64* counts;
  int* info;                            // [0] bit 0 (and 1): label outside [0, nid); bit 2: a pair was not placed.  [1] occupied slots
  unsigned int mask, probes;            // capacity - 1; min(capacity, GPROBES)
};

__device__ __forceinline__ u64 mix64(u64 k) {   // MurmurHash3's finaliser: ids of neighbours are close, their keys must not be
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
  return k ^ (k >> 33);
}

// how a value joins a pair's word, in LDS and in global memory alike
struct PairAdd {
  static __device__ __forceinline__ void combine(u64* word, u64 v) { atomicAdd(word, v); }
};
struct PairMax {
  static __device__ __forceinline__ void combine(u64* word, u64 v) { atomicMax(word, v); }
};

// n counts (Op = PairMax: the value n) of `key` into the global table.  Bounded: at most o.probes slots, all inside [0, capacity); a pair that finds
// neither its key nor an empty slot sets bit 2 and is dropped (the caller discards the table).  A stale read of a key
// can only show 0 for a claimed slot, which the compare-and-swap corrects; a claimed key never changes.
template <typename Op = PairAdd>
__device__ void pair_to_global(const ContactsOut& o, u64 key, u64 n, u64 h) {
  unsigned int s = (unsigned int)(h >> 32) & o.mask;
  for (unsigned int i = 0; i < o.probes; ++i) {
    u64 k = __hip_atomic_load(&o.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == 0) {
      k = atomicCAS(&o.keys[s], 0ull, key);
      if (k == 0) atomicAdd(o.info + 1, 1);
    }
    if (k == 0 || k == key) { Op::combine(&o.counts[s], n); return; }
    s = (s + 1) & o.mask;
  }
  atomicOr(o.info, 4);
}

template <typename Op = PairAdd>
__device__ void add_pair(u64* lkeys, u64* lcnt, const ContactsOut& o, u64 key, unsigned int n) {
  const u64 h = mix64(key);
  int s = (int)(h & (CSLOTS - 1));
  for (int i = 0; i < CPROBES; ++i) {
    u64 k = __hip_atomic_load(&lkeys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k == 0) k = atomicCAS(&lkeys[s], 0ull, key);
    if (k == 0 || k == key) { Op::combine(&lcnt[s], (u64)n); return; }
    s = (s + 1) & (CSLOTS - 1);
  }
  pair_to_global<Op>(o, key, n, h);
}

__global__ void contacts_init(ContactsOut o, long long capacity) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 2) o.info[i] = 0;
  if (i >= capacity) return;
  o.keys[i] = 0;
  o.counts[i] = 0;
}

inline ContactsOut contacts_out(u64* keys, u64* counts, int* info, int capacity) {
  return ContactsOut{keys, counts, info, (unsigned int)capacity - 1u,
                     (unsigned int)capacity < GPROBES ? (unsigned int)capacity : GPROBES};
}

}  // namespace
