// mesh_halfedge.hpp — the sorted half-edge table of an indexed triangle mesh, shared by the mesh checks
// (mesh.hip) and the hole filling (holes.hip).
//
// Half-edge h = 3 t + k runs from corner k of triangle t to corner (k + 1) % 3. The 3T half-edges are
// sorted by (min, max) of their end vertices with two stable radix passes; runs of equal keys are the
// undirected edges, and inside a run the half-edges ascend.
#pragma once
#include "common.hpp"

namespace pyqsm {

__device__ __forceinline__ void half_edge(const int32_t* __restrict__ tris, int h, int& u, int& w) {
  const int t = h / 3, k = h - 3 * t;
  u = tris[h];
  w = tris[3 * t + (k == 2 ? 0 : k + 1)];
}

static __global__ __launch_bounds__(256) void k_mesh_he_keys(int n, const int32_t* __restrict__ tris,
                                                             const int32_t* __restrict__ perm /*may be null*/,
                                                             int want_min, uint32_t* __restrict__ keys,
                                                             int32_t* __restrict__ vals) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int h = perm ? perm[i] : i;
  int u, w;
  half_edge(tris, h, u, w);
  keys[i] = uint32_t(want_min ? min(u, w) : max(u, w));
  vals[i] = h;
}

// flags [n + 1]: 1 where a run of equal (min, max) begins, flags[n] = 0
static __global__ __launch_bounds__(256) void k_mesh_he_heads(int n, const int32_t* __restrict__ tris,
                                                              const int32_t* __restrict__ hs,
                                                              int32_t* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  int f = 0;
  if (i < n) {
    f = 1;
    if (i > 0) {
      int u0, w0, u1, w1;
      half_edge(tris, hs[i - 1], u0, w0);
      half_edge(tris, hs[i], u1, w1);
      f = (min(u0, w0) != min(u1, w1)) || (max(u0, w0) != max(u1, w1));
    }
  }
  flags[i] = f;
}

// x: the exclusive scan of the head flags. first [E + 1]: where each run begins, first[E] = n.
static __global__ __launch_bounds__(256) void k_mesh_he_first(int n, const int32_t* __restrict__ x,
                                                              int32_t* __restrict__ first) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (x[i + 1] != x[i]) first[x[i]] = i;
  if (i == 0) first[x[n]] = n;
}

// The sorted half-edges of d_tris [nt,3] (vertex indices below nv), all in the arena, enqueued only:
// *hs [nh] the half-edges by (min, max), *x [nh + 1] the exclusive scan of the run heads (sorted position
// i lies in edge x[i + 1] - 1, and x[nh] = E stays on the device) and *first [nh + 1], of which the
// first E + 1 entries are written: where each run begins, first[E] = nh.
inline int mesh_half_edge_runs(Ctx* c, const int32_t* d_tris, int nt, int nv, int32_t** hs, int32_t** x,
                               int32_t** first) {
  const int nh = 3 * nt, vbits = bit_length(uint64_t(nv));
  uint32_t *d_keys, *d_k2;
  int32_t *d_vals, *d_v2, *d_flags, *d_first;
  PQ_TRY(c->arena.get(size_t(nh), &d_keys));
  PQ_TRY(c->arena.get(size_t(nh), &d_vals));
  PQ_TRY(c->arena.get(size_t(nh), &d_k2));
  PQ_TRY(c->arena.get(size_t(nh), &d_v2));
  PQ_TRY(c->arena.get(size_t(nh) + 1, &d_flags));
  PQ_TRY(c->arena.get(size_t(nh) + 1, &d_first));
  // a stable pass by max, then one by min
  hipLaunchKernelGGL(k_mesh_he_keys, dim3(ceil_div(nh, 256)), dim3(256), 0, c->stream, nh, d_tris,
                     static_cast<const int32_t*>(nullptr), 0, d_keys, d_vals);
  PQ_HIP(hipGetLastError());
  PQ_TRY(stable_sort_pairs_u32(c, &d_keys, &d_vals, nh, vbits));
  hipLaunchKernelGGL(k_mesh_he_keys, dim3(ceil_div(nh, 256)), dim3(256), 0, c->stream, nh, d_tris,
                     static_cast<const int32_t*>(d_vals), 1, d_k2, d_v2);
  PQ_HIP(hipGetLastError());
  PQ_TRY(stable_sort_pairs_u32(c, &d_k2, &d_v2, nh, vbits));
  hipLaunchKernelGGL(k_mesh_he_heads, dim3(ceil_div(nh + 1, 256)), dim3(256), 0, c->stream, nh, d_tris,
                     static_cast<const int32_t*>(d_v2), d_flags);
  PQ_HIP(hipGetLastError());
  PQ_TRY(exclusive_scan_i32(c, d_flags, int64_t(nh) + 1));
  hipLaunchKernelGGL(k_mesh_he_first, dim3(ceil_div(nh, 256)), dim3(256), 0, c->stream, nh,
                     static_cast<const int32_t*>(d_flags), d_first);
  PQ_HIP(hipGetLastError());
  *hs = d_v2;
  *x = d_flags;
  *first = d_first;
  return 0;
}

}  // namespace pyqsm
