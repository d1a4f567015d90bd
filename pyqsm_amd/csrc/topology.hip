// topology.hip — from the contracted, down-sampled cloud to the cylinder table (pyQSM/geometry/
// skeletonize.py:36-146 and :375-441): the spanning forest of the kNN graph, the collapse of its
// degree-2 chains, the radius of every chain and the sampled cylinder surfaces. tests/
// topology_restatement.py states the contract in NumPy/SciPy; DESIGN.md §15 has the reasoning.
//
// Forest. Boruvka over the directed entries of the kNN table (knn.hip; entry (i, j) stands for the
// undirected pair {i, j}, so the union of both directions is covered). Entries that are padded, that
// name the point itself or whose d2 is not finite are no edges. A pair at distance exactly 0 joins the
// components of its ends but is never put out: what SciPy's minimum_spanning_tree does with explicit
// zeros (its Kruskal pass unites across them, its result drops them). The order on edges
// is (orderable bits of d2, packed (min, max)), strict and total. boruvka.hpp has the rounds, shared
// with the normal orientation, and what that order buys; the parity bit of its labels stays 0 here.
// A component hooks once in its life, so the edge it hooked along is kept in its own slot; the slots
// are compacted (scan.hip) and sorted by the packed pair with the atomic-free radix sort: the same
// bits every run.
//
// Chains. Degrees by integer atomics, a two-slot neighbour record per degree-2 node (slot order is
// irrelevant: a walk takes "the one I did not come from"), one walker per (kept node, incident
// edge); the walk from the smaller end emits. Count pass, sort by (a, b), scan, write pass.
//
// No device loop here is unbounded: pointer jumping and the rounds carry the caps of boruvka.hpp;
// chain walks stop after m steps and raise an error bit.
#include <algorithm>
#include <cmath>

#include "boruvka.hpp"
#include "common.hpp"
#include "knn.hpp"

namespace pyqsm {

static constexpr int kSurfLevels = 100, kSurfAngles = 20, kSurfPts = kSurfLevels * kSurfAngles;
static constexpr int kSurfSlots = 2048;        // keys sorted per cylinder (16 KB of LDS)

// bits of the error word the kernels raise
enum : int32_t { kErrWalk = 1, kErrEdge = 2, kErrIndex = 4, kErrWide = 8, kErrNonFinite = 16 };
// control words, one 16-byte block: error bits
enum { kCtlErr = 0, kCtlWords = 4 };

// ---- spanning forest ----------------------------------------------------------------------------
static constexpr unsigned long long kZeroKey = 0x8000000000000000ull;  // ord_bits(+0.0)

// The edge policy of boruvka.hpp. No edges: padded entries, the point itself, a weight that is
// negative or not finite. The weight is d2, an exact zero of either sign as kZeroKey; nothing flips.
// A hooking root keeps the edge and its weight in its own slot.
struct ForestEdges {
  const int32_t* idx;
  const double* d2;
  int k, m;
  unsigned long long *ek, *ew;
  __device__ void init(int i) const {
    ek[i] = ~0ull;
    ew[i] = ~0ull;
  }
  __device__ bool ends(int64_t e, int* i, int* j) const {
    *i = int(e / k);
    *j = idx[e];
    if (*j < 0 || *j >= m || *j == *i) return false;
    const double w = d2[e];
    return w >= 0.0 && w < __builtin_inf();
  }
  __device__ unsigned long long key(int64_t e, int, int) const {
    const double w = d2[e];
    return w == 0.0 ? kZeroKey : ord_bits(w);
  }
  __device__ uint32_t flip(int, int) const { return 0u; }
  __device__ void hooked(uint32_t c, unsigned long long pk, unsigned long long key) const {
    ek[c] = pk;
    ew[c] = key;
  }
};

// flags [m + 1] for compact_flagged: the slots that hold an edge of positive length
__global__ __launch_bounds__(256) void k_tp_flag(int m, const unsigned long long* __restrict__ ek,
                                                 const unsigned long long* __restrict__ ew,
                                                 int32_t* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i > m) return;
  flags[i] = (i < m && ek[i] != ~0ull && ew[i] != kZeroKey) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_tp_keys(int ne, const int64_t* __restrict__ slot,
                                                 const unsigned long long* __restrict__ ek, uint32_t* __restrict__ ka,
                                                 uint32_t* __restrict__ kb) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= ne) return;
  const unsigned long long pk = ek[slot[j]];
  ka[j] = uint32_t(pk >> 32);
  kb[j] = uint32_t(pk & 0xFFFFFFFFu);
}

__global__ __launch_bounds__(256) void k_tp_edges_out(int ne, const int32_t* __restrict__ perm,
                                                      const int64_t* __restrict__ slot,
                                                      const unsigned long long* __restrict__ ek,
                                                      const unsigned long long* __restrict__ ew,
                                                      int32_t* __restrict__ edges, double* __restrict__ d2) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= ne) return;
  const int64_t r = slot[perm[p]];
  const unsigned long long pk = ek[r];
  edges[2 * size_t(p)] = int32_t(pk >> 32);
  edges[2 * size_t(p) + 1] = int32_t(pk & 0xFFFFFFFFu);
  d2[p] = from_ord(ew[r]);
}

// ---- ordering rows by a packed pair ---------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tp_iota(int n, int32_t* __restrict__ v) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) v[i] = i;
}

__global__ __launch_bounds__(256) void k_tp_gather_u32(int n, const int32_t* __restrict__ at,
                                                       const uint32_t* __restrict__ src, uint32_t* __restrict__ dst) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[at[i]];
}

// *perm [n] (arena): the rows in ascending order of (ka, kb), both below 2^bits. Two stable radix
// sorts without global atomics: by kb, then by ka. kb is consumed.
static int order_by_pair(Ctx* c, const uint32_t* ka, uint32_t* kb, int64_t n, int bits, int32_t** perm) {
  int32_t* val;
  uint32_t* k2;
  PQ_TRY(c->arena.get(size_t(n), &val));
  PQ_TRY(c->arena.get(size_t(n), &k2));
  const int nb = ceil_div(n, 256);
  hipLaunchKernelGGL(k_tp_iota, dim3(nb), dim3(256), 0, c->stream, int(n), val);
  PQ_HIP(hipGetLastError());
  PQ_TRY(stable_sort_pairs_u32(c, &kb, &val, n, bits));
  hipLaunchKernelGGL(k_tp_gather_u32, dim3(nb), dim3(256), 0, c->stream, int(n), static_cast<const int32_t*>(val), ka,
                     k2);
  PQ_HIP(hipGetLastError());
  PQ_TRY(stable_sort_pairs_u32(c, &k2, &val, n, bits));
  *perm = val;
  return 0;
}

static int index_bits(int64_t m) {
  int bits = 1;
  while (bits < 32 && (int64_t(1) << bits) < m) ++bits;
  return bits;
}

static const char* topo_error_text(int32_t err) {
  if (err & kErrEdge) return "an edge names a node outside [0, n_nodes) or joins a node to itself";
  if (err & kErrWalk) return "a chain walk did not end within n_nodes steps: the edge list is not a forest";
  if (err & kErrIndex) return "a chain member or index_map entry is out of range";
  if (err & kErrNonFinite) return "a cylinder has a coordinate that is not finite";
  if (err & kErrWide) return "a cylinder is more than 2^21 mm across";
  return "internal error";
}

// Spanning forest of the kNN graph of the m points at d_xyz; d_edges i32 [m - 1, 2], d_d2 f64
// [m - 1] (all device).
static int forest_device(Ctx* c, const double* d_xyz, int64_t m, int32_t k, int32_t* d_edges, double* d_d2,
                         int64_t* n_edges, int32_t* rounds) {
  *n_edges = 0;
  *rounds = 0;
  if (m < 2) return 0;
  const int M = int(m);
  const int64_t ne = m * int64_t(k);
  int32_t *idx, *ctl, *flags;
  double* d2;
  uint32_t *lab, *hk;
  unsigned long long *bw, *be, *ek, *ew;
  PQ_TRY(c->arena.get(size_t(ne), &idx));
  PQ_TRY(c->arena.get(size_t(ne), &d2));
  PQ_TRY(c->arena.get(size_t(m), &lab));
  PQ_TRY(c->arena.get(size_t(m), &hk));
  PQ_TRY(c->arena.get(size_t(m), &bw));
  PQ_TRY(c->arena.get(size_t(m), &be));
  PQ_TRY(c->arena.get(size_t(m), &ek));
  PQ_TRY(c->arena.get(size_t(m), &ew));
  PQ_TRY(c->arena.get(size_t(m) + 1, &flags));
  PQ_TRY(c->arena.get(size_t(kBvCtlWords), &ctl));
  {
    ProfScope ps(c, "topo_knn");
    PQ_TRY(knn_device(c, d_xyz, m, k, 1, idx, d2));
  }
  {
    ProfScope ps(c, "topo_forest");
    PQ_TRY(boruvka_forest(c, "skeletal forest", m, ne, ForestEdges{idx, d2, int(k), M, ek, ew}, BvScopes{}, lab, hk,
                          bw, be, ctl, rounds));
  }
  ProfScope ps(c, "topo_forest_sort");
  int64_t* slot;
  PQ_TRY(c->arena.get(size_t(m), &slot));
  hipLaunchKernelGGL(k_tp_flag, dim3(ceil_div(m + 1, 256)), dim3(256), 0, c->stream, M,
                     static_cast<const unsigned long long*>(ek), static_cast<const unsigned long long*>(ew), flags);
  PQ_HIP(hipGetLastError());
  PQ_TRY(compact_flagged(c, flags, m, slot));
  int32_t cnt = 0;
  PQ_TRY(fetch(c, &cnt, flags + m));
  if (cnt < 0 || cnt > m - 1) return fail(PYQSM_EHIP, "skeletal forest: %d edges for %lld points", cnt, (long long)m);
  *n_edges = cnt;
  if (cnt == 0) return 0;
  uint32_t *ka, *kb;
  int32_t* perm;
  PQ_TRY(c->arena.get(size_t(cnt), &ka));
  PQ_TRY(c->arena.get(size_t(cnt), &kb));
  const int nb = ceil_div(cnt, 256);
  hipLaunchKernelGGL(k_tp_keys, dim3(nb), dim3(256), 0, c->stream, int(cnt), static_cast<const int64_t*>(slot),
                     static_cast<const unsigned long long*>(ek), ka, kb);
  PQ_HIP(hipGetLastError());
  PQ_TRY(order_by_pair(c, ka, kb, cnt, index_bits(m), &perm));
  hipLaunchKernelGGL(k_tp_edges_out, dim3(nb), dim3(256), 0, c->stream, int(cnt), static_cast<const int32_t*>(perm),
                     static_cast<const int64_t*>(slot), static_cast<const unsigned long long*>(ek),
                     static_cast<const unsigned long long*>(ew), d_edges, d_d2);
  PQ_HIP(hipGetLastError());
  return 0;
}

// ---- degree-2 chain collapse --------------------------------------------------------------------
__device__ __forceinline__ bool tc_edge(int64_t t, int m, const int32_t* __restrict__ edges, int* a, int* b) {
  *a = edges[2 * t];
  *b = edges[2 * t + 1];
  return *a >= 0 && *a < m && *b >= 0 && *b < m && *a != *b;
}

__global__ __launch_bounds__(256) void k_tc_degree(int64_t e, int m, const int32_t* __restrict__ edges,
                                                   int32_t* __restrict__ deg, int32_t* __restrict__ ctl) {
  const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (t >= e) return;
  int a, b;
  if (!tc_edge(t, m, edges, &a, &b)) {
    atomicOr(&ctl[kCtlErr], kErrEdge);
    return;
  }
  atomicAdd(&deg[a], 1);
  atomicAdd(&deg[b], 1);
}

// the two neighbours of every degree-2 node: exactly two edges claim a slot each
__global__ __launch_bounds__(256) void k_tc_neighbours(int64_t e, int m, const int32_t* __restrict__ edges,
                                                       const int32_t* __restrict__ deg, int32_t* __restrict__ fill,
                                                       int32_t* __restrict__ nb) {
  const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (t >= e) return;
  int a, b;
  if (!tc_edge(t, m, edges, &a, &b)) return;
  if (deg[a] == 2) {
    const int s = atomicAdd(&fill[a], 1);
    if (s < 2) nb[2 * size_t(a) + s] = b;
  }
  if (deg[b] == 2) {
    const int s = atomicAdd(&fill[b], 1);
    if (s < 2) nb[2 * size_t(b) + s] = a;
  }
}

// Walks from kept node u over its neighbour w to the next kept node: the number of degree-2 nodes
// passed (written to out when given, at most cap of them), or -1 after m steps without an end.
__device__ int tc_walk(int m, const int32_t* __restrict__ deg, const int32_t* __restrict__ nb, int u, int w,
                       int32_t* __restrict__ out, int cap, int* end) {
  int prev = u, cur = w, len = 0;
  for (int step = 0; step < m; ++step) {
    if (deg[cur] != 2) {
      *end = cur;
      return len;
    }
    if (out && len < cap) out[len] = cur;
    ++len;
    const int n0 = nb[2 * size_t(cur)], n1 = nb[2 * size_t(cur) + 1];
    const int nxt = n0 == prev ? n1 : n0;
    prev = cur;
    cur = nxt;
  }
  return -1;
}

// Count pass, one walker per directed edge slot t = 2 edge + side (flags [2 e + 1]): the walk from
// the smaller end of a chain is flagged and leaves the other end and the length.
__global__ __launch_bounds__(256) void k_tc_count(int64_t e, int m, const int32_t* __restrict__ edges,
                                                  const int32_t* __restrict__ deg, const int32_t* __restrict__ nb,
                                                  int32_t* __restrict__ flags, int32_t* __restrict__ wend,
                                                  int32_t* __restrict__ wlen, int32_t* __restrict__ ctl) {
  const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (t > 2 * e) return;
  flags[t] = 0;
  if (t == 2 * e) return;
  int a, b;
  if (!tc_edge(t >> 1, m, edges, &a, &b)) return;
  const int u = (t & 1) ? b : a, w = (t & 1) ? a : b;
  if (deg[u] == 2) return;
  int end = 0;
  const int len = tc_walk(m, deg, nb, u, w, nullptr, 0, &end);
  if (len < 0) {
    atomicOr(&ctl[kCtlErr], kErrWalk);
    return;
  }
  if (u < end) {
    flags[t] = 1;
    wend[t] = end;
    wlen[t] = len;
  }
}

__global__ __launch_bounds__(256) void k_tc_keys(int nc, const int64_t* __restrict__ slot,
                                                 const int32_t* __restrict__ edges, const int32_t* __restrict__ wend,
                                                 uint32_t* __restrict__ ka, uint32_t* __restrict__ kb) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nc) return;
  const int64_t t = slot[j];
  ka[j] = uint32_t(edges[t]);  // edges[2 (t >> 1) + (t & 1)]: the walker's own end
  kb[j] = uint32_t(wend[t]);
}

// Chains in their final order: ends, lengths (len [nc + 1], the last 0 for the scan), walker slots.
__global__ __launch_bounds__(256) void k_tc_chain_out(int nc, const int32_t* __restrict__ perm,
                                                      const int64_t* __restrict__ slot,
                                                      const int32_t* __restrict__ edges,
                                                      const int32_t* __restrict__ wend,
                                                      const int32_t* __restrict__ wlen, int32_t* __restrict__ ends,
                                                      int32_t* __restrict__ len, int64_t* __restrict__ walker) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p > nc) return;
  if (p == nc) {
    len[nc] = 0;
    return;
  }
  const int64_t t = slot[perm[p]];
  ends[2 * size_t(p)] = edges[t];
  ends[2 * size_t(p) + 1] = wend[t];
  len[p] = wlen[t];
  walker[p] = t;
}

// Write pass: chain_ptr [nc + 1] from the scanned lengths, and every chain's members by walking again.
__global__ __launch_bounds__(256) void k_tc_write(int nc, int m, const int32_t* __restrict__ edges,
                                                  const int32_t* __restrict__ deg, const int32_t* __restrict__ nb,
                                                  const int64_t* __restrict__ walker, const int32_t* __restrict__ off,
                                                  int64_t* __restrict__ chain_ptr, int32_t* __restrict__ members) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p > nc) return;
  chain_ptr[p] = off[p];
  if (p == nc) return;
  const int cap = off[p + 1] - off[p];
  if (cap <= 0) return;
  const int64_t t = walker[p];
  int end = 0;
  tc_walk(m, deg, nb, edges[t], edges[t ^ 1], members + off[p], cap, &end);
}

__global__ __launch_bounds__(256) void k_tc_kept_flag(int m, const int32_t* __restrict__ deg,
                                                      int32_t* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i > m) return;
  flags[i] = (i < m && deg[i] != 2) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_tc_narrow(int n, const int32_t* __restrict__ pos, int32_t* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;  // pos: the scanned flags [n + 1]
  if (i >= n) return;
  const int p = pos[i];
  if (pos[i + 1] != p) out[p] = i;
}

// Chain collapse of the forest d_edges i32 [e, 2] over m nodes; outputs (device) of the worst-case
// sizes m, e, e + 1 and m. counts: kept nodes, chains, members.
static int chains_device(Ctx* c, const int32_t* d_edges, int64_t e, int64_t m, int32_t* d_kept, int32_t* d_ends,
                         int64_t* d_ptr, int32_t* d_members, int64_t counts[3]) {
  counts[0] = counts[1] = counts[2] = 0;
  PQ_HIP(hipMemsetAsync(d_ptr, 0, 8, c->stream));
  if (m == 0) {
    PQ_HIP(hipStreamSynchronize(c->stream));
    return 0;
  }
  ProfScope ps(c, "topo_chains");
  const int M = int(m);
  int32_t *deg, *fill, *nb, *kflags, *ctl;
  PQ_TRY(c->arena.get(size_t(m), &deg));
  PQ_TRY(c->arena.get(size_t(m), &fill));
  PQ_TRY(c->arena.get(size_t(m) * 2, &nb));
  PQ_TRY(c->arena.get(size_t(m) + 1, &kflags));
  PQ_TRY(c->arena.get(size_t(kCtlWords), &ctl));
  PQ_HIP(hipMemsetAsync(deg, 0, size_t(m) * 4, c->stream));
  PQ_HIP(hipMemsetAsync(fill, 0, size_t(m) * 4, c->stream));
  PQ_HIP(hipMemsetAsync(nb, 0, size_t(m) * 8, c->stream));
  PQ_HIP(hipMemsetAsync(ctl, 0, kCtlWords * 4, c->stream));
  int32_t *flags = nullptr, *wend = nullptr, *wlen = nullptr;
  int64_t* slot = nullptr;
  if (e > 0) {
    const int eb = ceil_div(e, 256);
    PQ_TRY(c->arena.get(size_t(2 * e) + 1, &flags));
    PQ_TRY(c->arena.get(size_t(2 * e), &wend));
    PQ_TRY(c->arena.get(size_t(2 * e), &wlen));
    PQ_TRY(c->arena.get(size_t(2 * e), &slot));
    hipLaunchKernelGGL(k_tc_degree, dim3(eb), dim3(256), 0, c->stream, e, M, d_edges, deg, ctl);
    hipLaunchKernelGGL(k_tc_neighbours, dim3(eb), dim3(256), 0, c->stream, e, M, d_edges,
                       static_cast<const int32_t*>(deg), fill, nb);
    hipLaunchKernelGGL(k_tc_count, dim3(ceil_div(2 * e + 1, 256)), dim3(256), 0, c->stream, e, M, d_edges,
                       static_cast<const int32_t*>(deg), static_cast<const int32_t*>(nb), flags, wend, wlen, ctl);
    PQ_HIP(hipGetLastError());
    PQ_TRY(compact_flagged(c, flags, 2 * e, slot));
  }
  hipLaunchKernelGGL(k_tc_kept_flag, dim3(ceil_div(m + 1, 256)), dim3(256), 0, c->stream, M,
                     static_cast<const int32_t*>(deg), kflags);
  PQ_HIP(hipGetLastError());
  PQ_TRY(exclusive_scan_i32(c, kflags, m + 1));
  hipLaunchKernelGGL(k_tc_narrow, dim3(ceil_div(m, 256)), dim3(256), 0, c->stream, M,
                     static_cast<const int32_t*>(kflags), d_kept);
  PQ_HIP(hipGetLastError());
  int32_t n_kept = 0, nc = 0, h[kCtlWords] = {0, 0, 0, 0};
  PQ_TRY(download(c, &n_kept, kflags + m, 1));
  if (e > 0) PQ_TRY(download(c, &nc, flags + 2 * e, 1));
  PQ_TRY(download(c, h, ctl, kCtlWords));
  PQ_HIP(hipStreamSynchronize(c->stream));
  if (h[kCtlErr]) return fail(PYQSM_EINVAL, "collapse_chains: %s", topo_error_text(h[kCtlErr]));
  if (nc < 0 || nc > e) return fail(PYQSM_EHIP, "collapse_chains: %d chains for %lld edges", nc, (long long)e);
  counts[0] = n_kept;
  counts[1] = nc;
  if (nc == 0) return 0;
  uint32_t *ka, *kb;
  int32_t *perm, *len;
  int64_t* walker;
  PQ_TRY(c->arena.get(size_t(nc), &ka));
  PQ_TRY(c->arena.get(size_t(nc), &kb));
  PQ_TRY(c->arena.get(size_t(nc) + 1, &len));
  PQ_TRY(c->arena.get(size_t(nc), &walker));
  hipLaunchKernelGGL(k_tc_keys, dim3(ceil_div(nc, 256)), dim3(256), 0, c->stream, int(nc),
                     static_cast<const int64_t*>(slot), d_edges, static_cast<const int32_t*>(wend), ka, kb);
  PQ_HIP(hipGetLastError());
  PQ_TRY(order_by_pair(c, ka, kb, nc, index_bits(m), &perm));
  hipLaunchKernelGGL(k_tc_chain_out, dim3(ceil_div(nc + 1, 256)), dim3(256), 0, c->stream, int(nc),
                     static_cast<const int32_t*>(perm), static_cast<const int64_t*>(slot), d_edges,
                     static_cast<const int32_t*>(wend), static_cast<const int32_t*>(wlen), d_ends, len, walker);
  PQ_HIP(hipGetLastError());
  PQ_TRY(exclusive_scan_i32(c, len, int64_t(nc) + 1));
  int32_t total = 0;
  PQ_TRY(fetch(c, &total, len + nc));
  // every degree-2 node lies on one run and a run is emitted once, so this holds for any edge list
  if (total < 0 || total > m) return fail(PYQSM_EHIP, "collapse_chains: %d members for %lld nodes", total, (long long)m);
  hipLaunchKernelGGL(k_tc_write, dim3(ceil_div(nc + 1, 256)), dim3(256), 0, c->stream, int(nc), M, d_edges,
                     static_cast<const int32_t*>(deg), static_cast<const int32_t*>(nb),
                     static_cast<const int64_t*>(walker), static_cast<const int32_t*>(len), d_ptr, d_members);
  PQ_HIP(hipGetLastError());
  counts[2] = total;
  return 0;
}

// ---- radii --------------------------------------------------------------------------------------
// radius[p] = mean over the chain's members of |shift[member]| (or |shift[map[member]]|), the norm as
// sqrt((x x + y y) + z z); 0 for a chain without members. The sum takes the order of NumPy's
// pairwise summation (fewer than 8 terms: one at a time; up to 128: eight running sums, combined
// as a balanced tree, then the remainder; above: halves, the left one a multiple of 8), so that a
// radius is np.mean's as a rule; the contract is only the rounding bound of a sum of positive terms.
struct RadiiSrc {
  const int32_t* members;
  const double* shift;
  const int32_t* map;
  int64_t n, n_map;
  __device__ double at(int64_t s, bool* bad) const {
    int64_t id = members[s];
    if (map) {
      if (id < 0 || id >= n_map) {
        *bad = true;
        return 0.0;
      }
      id = map[id];
    }
    if (id < 0 || id >= n) {
      *bad = true;
      return 0.0;
    }
    const double x = shift[3 * id], y = shift[3 * id + 1], z = shift[3 * id + 2];
    return sqrt((x * x + y * y) + z * z);
  }
};

__device__ double radii_block_sum(const RadiiSrc& src, int64_t s0, int64_t n, bool* bad) {  // n <= 128
  if (n < 8) {
    double res = 0.0;
    for (int64_t i = 0; i < n; ++i) res = res + src.at(s0 + i, bad);
    return res;
  }
  double r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = src.at(s0 + j, bad);
  int64_t i = 8;
  for (; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = r[j] + src.at(s0 + i + j, bad);
  }
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res = res + src.at(s0 + i, bad);
  return res;
}

__global__ __launch_bounds__(256) void k_chain_radii(int nc, const int64_t* __restrict__ ptr,
                                                     const int32_t* __restrict__ members, int64_t n_members,
                                                     const double* __restrict__ shift, int64_t n,
                                                     const int32_t* __restrict__ map, int64_t n_map,
                                                     double* __restrict__ radius, int32_t* __restrict__ ctl) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= nc) return;
  const int64_t s0 = ptr[p], s1 = ptr[p + 1];
  radius[p] = 0.0;
  if (s0 < 0 || s1 > n_members || s1 < s0) {
    atomicOr(&ctl[kCtlErr], kErrIndex);
    return;
  }
  if (s1 == s0) return;
  const RadiiSrc src = {members, shift, map, n, n_map};
  bool bad = false;
  // the halving tree above 128 terms, walked with an explicit stack (depth <= log2 of the length)
  int64_t off[40], len[40];
  double left[40];
  int state[40];
  int sp = 0;
  off[0] = s0;
  len[0] = s1 - s0;
  state[0] = 0;
  double ret = 0.0;
  const int64_t max_steps = 3 * ((s1 - s0) / 32 + 2);  // three visits per node, at most len / 64 + 1 nodes
  for (int64_t step = 0; sp >= 0 && step < max_steps; ++step) {
    if (state[sp] == 0) {
      if (len[sp] <= 128 || sp >= 38) {
        ret = len[sp] <= 128 ? radii_block_sum(src, off[sp], len[sp], &bad) : 0.0;
        if (len[sp] > 128) bad = true;
        --sp;
      } else {
        int64_t n2 = len[sp] / 2;
        n2 -= n2 % 8;
        state[sp] = 1;
        off[sp + 1] = off[sp];
        len[sp + 1] = n2;
        state[sp + 1] = 0;
        ++sp;
      }
    } else if (state[sp] == 1) {
      int64_t n2 = len[sp] / 2;
      n2 -= n2 % 8;
      left[sp] = ret;
      state[sp] = 2;
      off[sp + 1] = off[sp] + n2;
      len[sp + 1] = len[sp] - n2;
      state[sp + 1] = 0;
      ++sp;
    } else {
      ret = left[sp] + ret;
      --sp;
    }
  }
  if (sp >= 0) bad = true;
  if (bad) {
    atomicOr(&ctl[kCtlErr], kErrIndex);
    return;
  }
  radius[p] = ret / double(s1 - s0);
}

// ---- cylinder surfaces --------------------------------------------------------------------------
// Per cylinder 14 doubles: centre, unit axis, u, v (3 each), radius, height. Point id = 20 level +
// angle is (centre + radius (cos u + sin v)) + along axis with NumPy's operation order, along from
// np.linspace(-height / 2, height / 2, 100): level * step + start, the last one = stop.
struct CylFrame {
  double cen[3], ax[3], u[3], v[3], radius, start, stop, delta, step;
};

__device__ __forceinline__ void cyl_point_mm(const CylFrame& f, const double* __restrict__ cs, int id, double mm[3]) {
  const int lev = id / kSurfAngles, a = id - lev * kSurfAngles;
  double along;
  if (lev == kSurfLevels - 1) along = f.stop;
  else if (f.step != 0.0) along = double(lev) * f.step + f.start;
  else along = (double(lev) / double(kSurfLevels - 1)) * f.delta + f.start;
  const double ca = cs[a], sa = cs[kSurfAngles + a];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double ring = f.radius * (ca * f.u[d] + sa * f.v[d]);
    const double p = (f.cen[d] + ring) + along * f.ax[d];
    mm[d] = rint(p * 1000.0);
  }
}

// One block per cylinder: the 2 000 points in millimetres, the 3 x 21-bit key of every point
// relative to the cylinder's minimum, a bitonic sort of (key, point id) in LDS, the first point of
// every run of equal keys. WRITE == false leaves the number of distinct rows in cnt[cyl]; WRITE ==
// true writes them (mm / 1000.0) from row cnt[cyl] on (cnt scanned in between).
template <bool WRITE>
__global__ __launch_bounds__(256) void k_cyl_surface(int q, const double* __restrict__ par,
                                                     const double* __restrict__ cs, int32_t* __restrict__ cnt,
                                                     double* __restrict__ out, int32_t* __restrict__ ctl) {
  __shared__ unsigned long long sk[kSurfSlots];
  __shared__ uint16_t si[kSurfSlots];
  __shared__ long long red[3][256];
  __shared__ int sc[256];
  const int cyl = blockIdx.x, tid = threadIdx.x;
  if (cyl >= q) return;
  const double* P = par + 14 * size_t(cyl);
  CylFrame f;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    f.cen[d] = P[d];
    f.ax[d] = P[3 + d];
    f.u[d] = P[6 + d];
    f.v[d] = P[9 + d];
  }
  f.radius = P[12];
  const double height = P[13];
  f.start = -height / 2.0;
  f.stop = height / 2.0;
  f.delta = f.stop - f.start;
  f.step = f.delta / double(kSurfLevels - 1);
  long long kx[8], ky[8], kz[8];
  long long mn[3] = {0x7FFFFFFFFFFFFFFFll, 0x7FFFFFFFFFFFFFFFll, 0x7FFFFFFFFFFFFFFFll};
  bool bad = false;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int id = tid + 256 * r;
    kx[r] = ky[r] = kz[r] = 0;
    if (id < kSurfPts) {
      double mm[3];
      cyl_point_mm(f, cs, id, mm);
#pragma unroll
      for (int d = 0; d < 3; ++d)
        if (!(fabs(mm[d]) < 4.0e15)) {
          bad = true;
          mm[d] = 0.0;
        }
      kx[r] = (long long)mm[0];
      ky[r] = (long long)mm[1];
      kz[r] = (long long)mm[2];
      mn[0] = min(mn[0], kx[r]);
      mn[1] = min(mn[1], ky[r]);
      mn[2] = min(mn[2], kz[r]);
    }
  }
  if (bad) atomicOr(&ctl[kCtlErr], kErrNonFinite);
#pragma unroll
  for (int d = 0; d < 3; ++d) red[d][tid] = mn[d];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int d = 0; d < 3; ++d) red[d][tid] = min(red[d][tid], red[d][tid + s]);
    }
    __syncthreads();
  }
  const long long m0 = red[0][0], m1 = red[1][0], m2 = red[2][0];
  bool wide = false;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int id = tid + 256 * r;
    if (id < kSurfPts) {
      unsigned long long a = (unsigned long long)(kx[r] - m0), b = (unsigned long long)(ky[r] - m1),
                         cc = (unsigned long long)(kz[r] - m2);
      if (a >= (1ull << 21) || b >= (1ull << 21) || cc >= (1ull << 21)) {
        wide = true;
        a &= (1ull << 21) - 1;
        b &= (1ull << 21) - 1;
        cc &= (1ull << 21) - 1;
      }
      sk[id] = (a << 42) | (b << 21) | cc;
      si[id] = uint16_t(id);
    } else {
      sk[id] = ~0ull;
      si[id] = 0xFFFF;
    }
  }
  if (wide) atomicOr(&ctl[kCtlErr], kErrWide);
  __syncthreads();
  for (int k2 = 2; k2 <= kSurfSlots; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < kSurfSlots; t += 256) {
        const int o = t ^ j;
        if (o > t) {
          const unsigned long long ka = sk[t], kb = sk[o];
          const uint16_t ia = si[t], ib = si[o];
          const bool a_gt_b = ka > kb || (ka == kb && ia > ib);
          if (a_gt_b == ((t & k2) == 0)) {
            sk[t] = kb;
            si[t] = ib;
            sk[o] = ka;
            si[o] = ia;
          }
        }
      }
      __syncthreads();
    }
  // heads of the runs: thread tid owns slots 8 tid .. 8 tid + 7
  int heads = 0;
  unsigned mask = 0;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int t = 8 * tid + r;
    const unsigned long long key = sk[t];
    const bool head = key != ~0ull && (t == 0 || sk[t - 1] != key);
    if (head) {
      ++heads;
      mask |= 1u << r;
    }
  }
  sc[tid] = heads;
  __syncthreads();
  for (int s = 1; s < 256; s <<= 1) {
    const int add = tid >= s ? sc[tid - s] : 0;
    __syncthreads();
    sc[tid] += add;
    __syncthreads();
  }
  if (!WRITE) {
    if (tid == 255) cnt[cyl] = sc[255];
    return;
  }
  size_t row = size_t(cnt[cyl]) + size_t(sc[tid] - heads);
#pragma unroll
  for (int r = 0; r < 8; ++r)
    if (mask & (1u << r)) {
      double mm[3];
      cyl_point_mm(f, cs, int(si[8 * tid + r]), mm);
      out[3 * row] = mm[0] / 1000.0;
      out[3 * row + 1] = mm[1] / 1000.0;
      out[3 * row + 2] = mm[2] / 1000.0;
      ++row;
    }
}

static int check_nodes(int64_t m) {
  if (m < 0) return fail(PYQSM_EINVAL, "negative size");
  if (m > 0x3FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^30 nodes per call");
  return 0;
}

static int check_forest_k(int32_t k) {
  if (k < 1 || k > kKnnMaxK) return fail(PYQSM_ERANGE, "k must be in [1, %d]", kKnnMaxK);
  return 0;
}

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_skeletal_forest_dev(const double* xyz_dev, int64_t m, int32_t k, int32_t* edges_dev, double* d2_dev,
                              int64_t* n_edges, int32_t* rounds, int32_t device) {
  PQ_API_RANGE("pyqsm_skeletal_forest_dev");
  PQ_TRY(check_nodes(m));
  PQ_TRY(check_forest_k(k));
  if (!n_edges) return fail(PYQSM_EINVAL, "pyqsm_skeletal_forest_dev: NULL out-parameter");
  *n_edges = 0;
  if (rounds) *rounds = 0;
  if (m > 1 && (!xyz_dev || !edges_dev || !d2_dev)) return fail(PYQSM_EINVAL, "pyqsm_skeletal_forest_dev: NULL pointer");
  if (m < 2) return 0;
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  int32_t r = 0;
  PQ_TRY(forest_device(c, xyz_dev, m, k, edges_dev, d2_dev, n_edges, &r));
  PQ_HIP(hipStreamSynchronize(c->stream));
  if (rounds) *rounds = r;
  return 0;
}

int pyqsm_skeletal_forest(const double* xyz, int64_t m, int32_t k, int32_t* edges, double* d2, int64_t* n_edges,
                          int32_t* rounds, int32_t device) {
  PQ_API_RANGE("pyqsm_skeletal_forest");
  PQ_TRY(check_nodes(m));
  PQ_TRY(check_forest_k(k));
  if (!n_edges) return fail(PYQSM_EINVAL, "pyqsm_skeletal_forest: NULL out-parameter");
  *n_edges = 0;
  if (rounds) *rounds = 0;
  if (m > 1 && (!xyz || !edges || !d2)) return fail(PYQSM_EINVAL, "pyqsm_skeletal_forest: NULL pointer");
  if (m < 2) return 0;
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double *d_xyz, *d_d2;
  int32_t* d_edges;
  PQ_TRY(c->arena.get(size_t(m) * 3, &d_xyz));
  PQ_TRY(c->arena.get(size_t(m) * 2, &d_edges));
  PQ_TRY(c->arena.get(size_t(m), &d_d2));
  PQ_TRY(copy_in(c, d_xyz, xyz, size_t(m) * 3));
  int32_t r = 0;
  int64_t ne = 0;
  PQ_TRY(forest_device(c, d_xyz, m, k, d_edges, d_d2, &ne, &r));
  if (ne > 0) {
    PQ_TRY(download(c, edges, d_edges, size_t(ne) * 2));
    PQ_TRY(download(c, d2, d_d2, size_t(ne)));
  }
  PQ_HIP(hipStreamSynchronize(c->stream));
  *n_edges = ne;
  if (rounds) *rounds = r;
  return 0;
}

static int check_chain_args(const char* who, int64_t e, int64_t m, const void* edges, const void* kept,
                            const void* ends, const void* ptr, const void* members, const void* counts) {
  PQ_TRY(check_nodes(m));
  if (e < 0) return fail(PYQSM_EINVAL, "%s: negative size", who);
  if (e > 0x3FFFFF00LL) return fail(PYQSM_ERANGE, "%s: more than 2^30 edges per call", who);
  if (!counts || !ptr) return fail(PYQSM_EINVAL, "%s: NULL out-parameter", who);
  if ((e > 0 && (!edges || !ends)) || (m > 0 && (!kept || !members))) return fail(PYQSM_EINVAL, "%s: NULL pointer", who);
  if (e > 0 && m == 0) return fail(PYQSM_EINVAL, "%s: edges without nodes", who);
  return 0;
}

int pyqsm_collapse_chains_dev(const int32_t* edges_dev, int64_t e, int64_t m, int32_t* kept_dev,
                              int32_t* chain_ends_dev, int64_t* chain_ptr_dev, int32_t* members_dev, int64_t* counts,
                              int32_t device) {
  PQ_API_RANGE("pyqsm_collapse_chains_dev");
  PQ_TRY(check_chain_args("pyqsm_collapse_chains_dev", e, m, edges_dev, kept_dev, chain_ends_dev, chain_ptr_dev,
                          members_dev, counts));
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  PQ_TRY(chains_device(c, edges_dev, e, m, kept_dev, chain_ends_dev, chain_ptr_dev, members_dev, counts));
  PQ_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int pyqsm_collapse_chains(const int32_t* edges, int64_t e, int64_t m, int32_t* kept, int32_t* chain_ends,
                          int64_t* chain_ptr, int32_t* members, int64_t* counts, int32_t device) {
  PQ_API_RANGE("pyqsm_collapse_chains");
  PQ_TRY(check_chain_args("pyqsm_collapse_chains", e, m, edges, kept, chain_ends, chain_ptr, members, counts));
  counts[0] = counts[1] = counts[2] = 0;
  chain_ptr[0] = 0;
  if (m == 0) return 0;
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  int32_t *d_edges = nullptr, *d_kept, *d_ends, *d_members;
  int64_t* d_ptr;
  PQ_TRY(c->arena.get(size_t(std::max<int64_t>(e, 1)) * 2, &d_edges));
  PQ_TRY(c->arena.get(size_t(m), &d_kept));
  PQ_TRY(c->arena.get(size_t(std::max<int64_t>(e, 1)) * 2, &d_ends));
  PQ_TRY(c->arena.get(size_t(e) + 1, &d_ptr));
  PQ_TRY(c->arena.get(size_t(m), &d_members));
  if (e > 0) PQ_TRY(copy_in(c, d_edges, edges, size_t(e) * 2));
  PQ_TRY(chains_device(c, d_edges, e, m, d_kept, d_ends, d_ptr, d_members, counts));
  if (counts[0] > 0) PQ_TRY(download(c, kept, d_kept, size_t(counts[0])));
  if (counts[1] > 0) {
    PQ_TRY(download(c, chain_ends, d_ends, size_t(counts[1]) * 2));
    PQ_TRY(download(c, chain_ptr, d_ptr, size_t(counts[1] + 1)));
  }
  if (counts[2] > 0) PQ_TRY(download(c, members, d_members, size_t(counts[2])));
  PQ_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int pyqsm_chain_radii(const double* shift, int64_t n, const int64_t* chain_ptr, int64_t n_chains,
                      const int32_t* members, const int32_t* index_map, int64_t n_map, double* radius,
                      int32_t device) {
  PQ_API_RANGE("pyqsm_chain_radii");
  if (n < 0 || n_chains < 0 || n_map < 0) return fail(PYQSM_EINVAL, "negative size");
  if (n_chains > 0x3FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^30 chains per call");
  if (n_chains == 0) return 0;
  if (!chain_ptr || !radius) return fail(PYQSM_EINVAL, "pyqsm_chain_radii: NULL pointer");
  const int64_t n_members = chain_ptr[n_chains];
  if (chain_ptr[0] != 0 || n_members < 0) return fail(PYQSM_EINVAL, "pyqsm_chain_radii: chain_ptr must run from 0 upwards");
  for (int64_t p = 0; p < n_chains; ++p)
    if (chain_ptr[p + 1] < chain_ptr[p]) return fail(PYQSM_EINVAL, "pyqsm_chain_radii: chain_ptr must not decrease");
  if (n_members > 0 && (!members || !shift)) return fail(PYQSM_EINVAL, "pyqsm_chain_radii: NULL pointer");
  if (index_map == nullptr) n_map = 0;
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  ProfScope ps(c, "topo_radii");
  double *d_shift, *d_rad;
  int64_t* d_ptr;
  int32_t *d_mem, *d_map = nullptr, *ctl;
  PQ_TRY(c->arena.get(size_t(std::max<int64_t>(n, 1)) * 3, &d_shift));
  PQ_TRY(c->arena.get(size_t(n_chains), &d_rad));
  PQ_TRY(c->arena.get(size_t(n_chains) + 1, &d_ptr));
  PQ_TRY(c->arena.get(size_t(std::max<int64_t>(n_members, 1)), &d_mem));
  PQ_TRY(c->arena.get(size_t(kCtlWords), &ctl));
  PQ_HIP(hipMemsetAsync(ctl, 0, kCtlWords * 4, c->stream));
  if (n > 0) PQ_TRY(copy_in(c, d_shift, shift, size_t(n) * 3));
  PQ_TRY(copy_in(c, d_ptr, chain_ptr, size_t(n_chains + 1)));
  if (n_members > 0) PQ_TRY(copy_in(c, d_mem, members, size_t(n_members)));
  if (index_map && n_map > 0) {
    PQ_TRY(upload(c, index_map, size_t(n_map), &d_map));
  } else if (index_map) {
    PQ_TRY(c->arena.get(size_t(1), &d_map));  // an empty map: every member is out of range
  }
  hipLaunchKernelGGL(k_chain_radii, dim3(ceil_div(n_chains, 256)), dim3(256), 0, c->stream, int(n_chains),
                     static_cast<const int64_t*>(d_ptr), static_cast<const int32_t*>(d_mem), n_members,
                     static_cast<const double*>(d_shift), n, static_cast<const int32_t*>(d_map), n_map, d_rad, ctl);
  PQ_HIP(hipGetLastError());
  int32_t h[kCtlWords];
  PQ_TRY(download(c, h, ctl, kCtlWords));
  PQ_TRY(fetch(c, radius, d_rad, size_t(n_chains)));
  if (h[kCtlErr]) return fail(PYQSM_EINVAL, "pyqsm_chain_radii: %s", topo_error_text(h[kCtlErr]));
  return 0;
}

int pyqsm_cylinder_surfaces(const double* params, int64_t q, const double* cos_sin, int64_t* surface_ptr,
                            double** points_out, int64_t* total_out, int32_t device) {
  PQ_API_RANGE("pyqsm_cylinder_surfaces");
  if (q < 0) return fail(PYQSM_EINVAL, "negative size");
  if (q > 1000000) return fail(PYQSM_ERANGE, "more than 10^6 cylinders per call");
  if (!surface_ptr || !points_out || !total_out) return fail(PYQSM_EINVAL, "pyqsm_cylinder_surfaces: NULL out-parameter");
  *points_out = nullptr;
  *total_out = 0;
  surface_ptr[0] = 0;
  if (q == 0) return 0;
  if (!params || !cos_sin) return fail(PYQSM_EINVAL, "pyqsm_cylinder_surfaces: NULL pointer");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  ProfScope ps(c, "topo_surfaces");
  double *d_par, *d_cs, *d_out;
  int32_t *cnt, *ctl;
  PQ_TRY(c->arena.get(size_t(q) * 14, &d_par));
  PQ_TRY(c->arena.get(size_t(2 * kSurfAngles), &d_cs));
  PQ_TRY(c->arena.get(size_t(q) + 1, &cnt));
  PQ_TRY(c->arena.get(size_t(kCtlWords), &ctl));
  PQ_HIP(hipMemsetAsync(ctl, 0, kCtlWords * 4, c->stream));
  PQ_HIP(hipMemsetAsync(cnt, 0, size_t(q + 1) * 4, c->stream));
  PQ_TRY(copy_in(c, d_par, params, size_t(q) * 14));
  PQ_TRY(copy_in(c, d_cs, cos_sin, size_t(2 * kSurfAngles)));
  hipLaunchKernelGGL(k_cyl_surface<false>, dim3(unsigned(q)), dim3(256), 0, c->stream, int(q),
                     static_cast<const double*>(d_par), static_cast<const double*>(d_cs), cnt,
                     static_cast<double*>(nullptr), ctl);
  PQ_HIP(hipGetLastError());
  PQ_TRY(exclusive_scan_i32(c, cnt, q + 1));
  std::vector<int32_t> off(size_t(q) + 1);
  int32_t h[kCtlWords];
  PQ_TRY(download(c, off.data(), cnt, size_t(q + 1)));
  PQ_TRY(download(c, h, ctl, kCtlWords));
  PQ_HIP(hipStreamSynchronize(c->stream));
  if (h[kCtlErr])
    return fail((h[kCtlErr] & kErrWide) ? PYQSM_ERANGE : PYQSM_EINVAL, "pyqsm_cylinder_surfaces: %s",
                topo_error_text(h[kCtlErr]));
  const int64_t total = off[size_t(q)];
  if (total < q || total > q * int64_t(kSurfPts)) return fail(PYQSM_EHIP, "pyqsm_cylinder_surfaces: %lld rows", (long long)total);
  PQ_TRY(c->arena.get(size_t(total) * 3, &d_out));
  hipLaunchKernelGGL(k_cyl_surface<true>, dim3(unsigned(q)), dim3(256), 0, c->stream, int(q),
                     static_cast<const double*>(d_par), static_cast<const double*>(d_cs), cnt, d_out, ctl);
  PQ_HIP(hipGetLastError());
  OutBufs out;
  double* host = out.get<double>(size_t(total) * 3);
  if (!host) return fail(PYQSM_ENOMEM, "pyqsm_cylinder_surfaces: host allocation of %lld rows failed", (long long)total);
  PQ_TRY(fetch(c, host, d_out, size_t(total) * 3));
  out.kept = true;
  for (int64_t p = 0; p <= q; ++p) surface_ptr[p] = off[size_t(p)];
  *points_out = host;
  *total_out = total;
  return 0;
}

}  // extern "C"
