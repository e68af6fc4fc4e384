// glia_amd/csrc/union_find.hpp -- lock-free union-find on an array of 32-bit parent links, shared by the watershed's plateau step
// (watershed.hip) and the connected-component labelling (components.hip).
//
// parent[x] == x marks a root.  A link is only ever made from a root to a SMALLER index (atomic minimum), so
//   * a parent index is never larger than its child's: every root walk strictly descends and ends, in any interleaving of
//     concurrent unions;
//   * the root of a finished set is its smallest index.
// Scope: __HIP_MEMORY_SCOPE_AGENT for an array in global memory that several workgroups unite in one launch,
// __HIP_MEMORY_SCOPE_WORKGROUP for an array in LDS.  Nothing here waits for another thread: a lost race is noticed by the value the
// atomic returns and the union goes on from there.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace glia {

template <int Scope>
__device__ __forceinline__ uint32_t uf_root(const uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, Scope);
    if (p == x) return x;
    x = p;
  }
}
template <int Scope>
__device__ __forceinline__ void uf_unite(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = uf_root<Scope>(parent, a); b = uf_root<Scope>(parent, b);
    if (a == b) return;
    if (a > b) { const uint32_t t = a; a = b; b = t; }
    const uint32_t old = __hip_atomic_fetch_min(&parent[b], a, __ATOMIC_RELAXED, Scope);   // b was a root: now it points at the smaller root a
    if (old == b) return;
    b = old;                                           // somebody linked b meanwhile: go on from there
  }
}

}  // namespace glia
