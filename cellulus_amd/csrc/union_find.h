// The lock-free union-find the label kernels share (cc_label.hip, label_holes.hip).  L is a parent array over raster indices;
// links always point from the larger root to the smaller, so the final root of a set is its smallest index.  Stale reads of
// the parent array are harmless (parents only decrease along a chain; progress is made by the values returned from the
// atomics).
#pragma once
#include "clx_common.h"

namespace {

__device__ __forceinline__ int uf_find(const int* L, int a) {
  int p = L[a];
  while (p != a) { a = p; p = L[a]; }
  return a;
}

// find with path halving: every visited node is re-pointed at its grandparent.  A plain store is
// enough: only non-roots are written (a root is changed by the atomicMin of a union alone), and any
// ancestor is a valid parent, so a lost or stale write merely leaves a longer path.
__device__ __forceinline__ int uf_find_halve(int* L, int a) {
  int p = L[a];
  while (p != a) {
    const int gp = L[p];
    if (gp != p) L[a] = gp;
    a = p;
    p = gp;
  }
  return a;
}

__device__ __forceinline__ void uf_union(int* L, int a, int b) {
  bool done;
  do {
    a = uf_find_halve(L, a);
    b = uf_find_halve(L, b);
    if (a < b) {
      const int old = atomicMin(&L[b], a);
      done = (old == b);
      b = old;
    } else if (b < a) {
      const int old = atomicMin(&L[a], b);
      done = (old == a);
      a = old;
    } else {
      done = true;
    }
  } while (!done);
}

}  // namespace
