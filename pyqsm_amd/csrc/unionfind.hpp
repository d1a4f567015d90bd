// unionfind.hpp — a generic device union-find over int32 nodes 0 .. n - 1 (mesh.hip). dbscan.hip and
// topology.hip keep their own, specialised ones.
//
// parent[x] <= x always: a root is hooked below the smaller of two roots with a 32-bit atomicMin, so
// there are no cycles and the root of a finished set is its smallest member, whatever order the
// unions arrived in. Use: k_uf_init, any number of kernels that call uf_union, then k_uf_flatten
// (a launch of its own: every union must have finished), after which parent[x] is that smallest
// member.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pyqsm {

// parent[] is read past the CU's vector cache: a stale value would still be an ancestor (parents
// only move towards the root), but the fresh one saves steps.
__device__ __forceinline__ int32_t uf_load(const int32_t* parent, int32_t x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int32_t uf_find(const int32_t* parent, int32_t x) {
  for (;;) {
    const int32_t p = uf_load(parent, x);
    if (p == x) return x;
    x = p;
  }
}

// Joins the sets of a and b. When the atomicMin finds that `a` stopped being a root meanwhile, a's
// entry may now point at b (b below its former parent `old`): a's subtree has moved to b, and the
// loop goes on to join `old`, the rest of a's former set, with b.
__device__ __forceinline__ void uf_union(int32_t* parent, int32_t a, int32_t b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const int32_t t = a;
      a = b;
      b = t;
    }
    const int32_t old = atomicMin(&parent[a], b);
    if (old == a) return;
    a = old;
  }
}

static __global__ __launch_bounds__(256) void k_uf_init(int n, int32_t* __restrict__ parent) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) parent[i] = i;
}

// parent[i] = root of i. Entries change under the readers' feet, but only from one ancestor to the
// root, so every walk still ends at the root.
static __global__ __launch_bounds__(256) void k_uf_flatten(int n, int32_t* parent) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) parent[i] = uf_find(parent, i);
}

}  // namespace pyqsm
