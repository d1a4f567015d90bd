// convex_hull.hip — pyqsm_convex_hull: the exact convex hull of lattice points, batched over segments
// (DESIGN.md section 24). Every decision is an int64 predicate of hull_exact.hpp.
//
// Gift wrapping by brute force. A hull edge a -> b that lacks the facet on its left is open; its facet's
// plane is found by a reduction over the segment's points (p beats q iff orient3d(a, b, q, p) > 0), and the
// facet is then handled as a unit: the convex polygon of all points on that plane is wrapped inside the
// plane (2-D orientation on the projection along the normal's dominant axis), the fan from its vertex of
// lowest index gives the triangles, its directed edges go into a hash set of directed edges. A facet
// depends on its plane alone, so every open edge of one facet finds the same polygon; the one with the
// smallest (a, b) emits it, the others stand back. The next round's candidates are the reverses of the
// edges a round added. Rounds are launched by the host, which reads eight counters after each: the size
// of the next launch, the running count of tests (max_tests), the error word.
//
// In front of it the exact form of hull.hip's two filters: the extreme points of every segment along 26
// fixed directions plus four affinely independent points form a small cloud that is wrapped by the same
// code; every point strictly inside that polytope is dropped (compaction by scan), coincident points are
// merged by a sort, and the survivors are wrapped.
//
// Atomics: 64-bit integer atomicAdd on cursors and counters, 64-bit atomicCAS into the directed-edge set,
// 64-bit atomicOr on the error word, 32/64-bit LDS atomicAdd / atomicMin inside a block. The set's content,
// the counters and, after the closing sort by (a, b, c), the rows do not depend on the arrival order.
#include <algorithm>
#include <climits>

#include "common.hpp"
#include "hull_exact.hpp"

namespace pyqsm {
using namespace hullx;

static constexpr int kFacetMaxVerts = PYQSM_HULL_MAX_FACET_VERTS;
static constexpr int kExtDirs = 13;    // and their negatives
static constexpr int kExtSlots = 30;   // 26 extreme points and 4 affinely independent ones
static constexpr int kExtChunk = 4096;
static constexpr int64_t kHullDefaultMaxTests = PYQSM_HULL_DEFAULT_MAX_TESTS;
static constexpr unsigned long long kEmpty = ~0ull;

enum { W_TESTS = 0, W_NEXT, W_FACETS, W_POLY, W_TRIS, W_DEGEN, W_ERR, W_WORDS = 8 };
enum { ERR_FACET = 1, ERR_SET = 2, ERR_CAP = 4, ERR_WRAP = 8 };

// ---- the set of directed edges: open addressing, linear probing ----------------------------------
struct EdgeSet {
  unsigned long long* tab;
  unsigned long long mask;
  int shift;
};
__device__ __forceinline__ unsigned long long ekey(int a, int b) {
  return ((unsigned long long)(unsigned)a << 32) | (unsigned)b;
}
__device__ __forceinline__ bool set_has(const EdgeSet& h, unsigned long long key) {
  unsigned long long s = (key * 0x9E3779B97F4A7C15ull) >> h.shift;
  for (unsigned long long it = 0; it <= h.mask; ++it) {
    const unsigned long long v = h.tab[s];
    if (v == key) return true;
    if (v == kEmpty) return false;
    s = (s + 1) & h.mask;
  }
  return false;
}
__device__ __forceinline__ bool set_insert(const EdgeSet& h, unsigned long long key) {
  unsigned long long s = (key * 0x9E3779B97F4A7C15ull) >> h.shift;
  for (unsigned long long it = 0; it <= h.mask; ++it) {
    const unsigned long long old = atomicCAS(&h.tab[s], kEmpty, key);
    if (old == kEmpty || old == key) return true;
    s = (s + 1) & h.mask;
  }
  return false;  // full: cannot happen at twice the edge bound; reported, never waited for
}

// ---- reductions of a block over the points [lo, hi) of its segment ----------------------------------
// rule.eligible(q), rule.beats(best, q): a total preorder on the eligible points; returns a maximum (-1
// when nothing is eligible). count: an LDS word that receives the number of eligible points.
template <class Rule>
__device__ int block_best(int lo, int hi, const Rule& rule, int* sh, int* count) {
  int best = -1, cnt = 0;
  if (count && threadIdx.x == 0) *count = 0;
  for (int q = lo + int(threadIdx.x); q < hi; q += 256)
    if (rule.eligible(q)) {
      ++cnt;
      if (best < 0 || rule.beats(best, q)) best = q;
    }
  sh[threadIdx.x] = best;
  __syncthreads();
  if (count && cnt) atomicAdd(count, cnt);
  for (int off = 128; off > 0; off >>= 1) {
    if (int(threadIdx.x) < off) {
      const int o = sh[threadIdx.x + off], b = sh[threadIdx.x];
      if (o >= 0 && (b < 0 || rule.beats(b, o))) sh[threadIdx.x] = o;
    }
    __syncthreads();
  }
  const int r = sh[0];
  __syncthreads();
  return r;
}

struct LexRule {  // the lexicographically smallest point
  const int32_t* P;
  __device__ bool eligible(int) const { return true; }
  __device__ bool beats(int b, int q) const {
    const int32_t *pb = P + 3 * size_t(b), *pq = P + 3 * size_t(q);
    if (pq[0] != pb[0]) return pq[0] < pb[0];
    if (pq[1] != pb[1]) return pq[1] < pb[1];
    if (pq[2] != pb[2]) return pq[2] < pb[2];
    return q < b;
  }
};
struct PivotRule {  // around the axis through u with direction e: q beats b iff q is strictly outside (u, e, b)
  const int32_t* P;
  int32_t u[3];
  V3 e;
  __device__ bool eligible(int q) const { return !is_zero(cross(e, diff(P + 3 * size_t(q), u))); }
  __device__ bool beats(int b, int q) const {
    return dot(cross(e, diff(P + 3 * size_t(b), u)), diff(P + 3 * size_t(q), u)) > 0;
  }
};
struct WrapRule {  // inside the plane (u, n): the next polygon vertex after y, counter-clockwise seen from outside
  const int32_t* P;
  int32_t u[3], yc[3];
  V3 n;
  int axis, y;
  bool npos;
  __device__ bool eligible(int q) const { return q != y && dot(n, diff(P + 3 * size_t(q), u)) == 0; }
  __device__ bool beats(int b, int q) const {
    const int o = orient2d_in_plane(yc, P + 3 * size_t(b), P + 3 * size_t(q), axis, npos);
    if (o) return o < 0;  // q right of y -> b
    return norm2(diff(P + 3 * size_t(q), yc)) > norm2(diff(P + 3 * size_t(b), yc));  // the farther of a line
  }
};
__device__ __forceinline__ void load3(const int32_t* P, int i, int32_t* out) {
  out[0] = P[3 * size_t(i)];
  out[1] = P[3 * size_t(i) + 1];
  out[2] = P[3 * size_t(i) + 2];
}

// One block per segment: a first directed hull edge. p0 is the lexicographically smallest point, so the
// line through p0 along z touches the hull and all points lie in less than a half turn around it: the
// pivot around that line gives a supporting plane, one wrap step inside it a hull edge p0 -> z. The
// reverse edge is put into the set, which makes p0 -> z an open edge like any other.
__global__ __launch_bounds__(256) void k_hull_seed(const int32_t* __restrict__ P, const int32_t* __restrict__ seg,
                                                   EdgeSet h, int32_t* __restrict__ edges,
                                                   unsigned long long* __restrict__ w) {
  __shared__ int sh[256];
  const int s = blockIdx.x, lo = seg[s], hi = seg[s + 1];
  if (threadIdx.x == 0) {
    edges[3 * size_t(s)] = -1;
    edges[3 * size_t(s) + 1] = -1;
    edges[3 * size_t(s) + 2] = s;
  }
  if (hi <= lo) return;
  const int p0 = block_best(lo, hi, LexRule{P}, sh, nullptr);
  PivotRule pr;
  pr.P = P;
  load3(P, p0, pr.u);
  pr.e = V3{0, 0, 1};
  const int p = block_best(lo, hi, pr, sh, nullptr);
  int z = -1;
  if (p >= 0) {
    WrapRule wr;
    wr.P = P;
    load3(P, p0, wr.u);
    load3(P, p0, wr.yc);
    wr.n = cross(pr.e, diff(P + 3 * size_t(p), pr.u));
    wr.axis = dominant_axis(wr.n);
    wr.npos = comp(wr.n, wr.axis) > 0;
    wr.y = p0;
    z = block_best(lo, hi, wr, sh, nullptr);
  }
  if (threadIdx.x != 0) return;
  atomicAdd(&w[W_TESTS], 3ull * (unsigned long long)(hi - lo));
  if (z < 0) {
    atomicOr(&w[W_ERR], (unsigned long long)ERR_WRAP);
    return;
  }
  if (!set_insert(h, ekey(z, p0))) atomicOr(&w[W_ERR], (unsigned long long)ERR_SET);
  edges[3 * size_t(s)] = p0;
  edges[3 * size_t(s) + 1] = z;
}

// One block per candidate edge (u, v, segment). Open: u -> v is not in the set and v -> u is.
__global__ __launch_bounds__(256) void k_hull_wrap(const int32_t* __restrict__ P, const int32_t* __restrict__ seg,
                                                   const int32_t* __restrict__ edges, EdgeSet h,
                                                   int32_t* __restrict__ pool, long long pool_cap,
                                                   int32_t* __restrict__ facets, long long facet_cap,
                                                   unsigned long long* __restrict__ w) {
  __shared__ int sh[256];
  __shared__ int poly[kFacetMaxVerts];
  __shared__ int s_cnt;
  __shared__ unsigned long long s_min;
  __shared__ long long s_base;
  const int u = edges[3 * size_t(blockIdx.x)], v = edges[3 * size_t(blockIdx.x) + 1],
            s = edges[3 * size_t(blockIdx.x) + 2];
  if (u < 0) return;
  if (set_has(h, ekey(u, v)) || !set_has(h, ekey(v, u))) return;  // block-uniform
  const int lo = seg[s], hi = seg[s + 1];
  unsigned long long passes = 1;
  PivotRule pr;
  pr.P = P;
  load3(P, u, pr.u);
  pr.e = diff(P + 3 * size_t(v), pr.u);
  const int p = block_best(lo, hi, pr, sh, nullptr);
  if (p < 0) {
    if (threadIdx.x == 0) atomicOr(&w[W_ERR], (unsigned long long)ERR_WRAP);
    return;
  }
  WrapRule wr;
  wr.P = P;
  load3(P, u, wr.u);
  wr.n = cross(pr.e, diff(P + 3 * size_t(p), pr.u));
  wr.axis = dominant_axis(wr.n);
  wr.npos = comp(wr.n, wr.axis) > 0;
  if (threadIdx.x == 0) {
    poly[0] = u;
    poly[1] = v;
  }
  int k = 2, y = v, on_plane = 0;
  for (;;) {  // every turn adds a vertex: at most kFacetMaxVerts turns
    wr.y = y;
    load3(P, y, wr.yc);
    const int z = block_best(lo, hi, wr, sh, k == 2 ? &s_cnt : nullptr);
    ++passes;
    if (k == 2) on_plane = s_cnt + 1;  // and v itself
    if (z < 0) {
      if (threadIdx.x == 0) atomicOr(&w[W_ERR], (unsigned long long)ERR_WRAP);
      return;
    }
    if (z == u) break;
    if (k >= kFacetMaxVerts) {
      if (threadIdx.x == 0) atomicOr(&w[W_ERR], (unsigned long long)ERR_FACET);
      return;
    }
    if (threadIdx.x == 0) poly[k] = z;
    ++k;
    y = z;
    if (on_plane == 3) break;  // u, v, z and nothing else: the facet is this triangle
  }
  if (threadIdx.x == 0) s_min = kEmpty;
  __syncthreads();
  for (int i = threadIdx.x; i < k; i += 256) {
    const int x = poly[i], yy = poly[i + 1 == k ? 0 : i + 1];
    if (!set_has(h, ekey(x, yy)) && set_has(h, ekey(yy, x))) atomicMin(&s_min, ekey(x, yy));
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(&w[W_TESTS], passes * (unsigned long long)(hi - lo));
    s_base = -1;
    if (s_min == ekey(u, v)) {  // the open edge of this facet with the smallest key emits it
      const long long f = (long long)atomicAdd(&w[W_FACETS], 1ull);
      const long long st = (long long)atomicAdd(&w[W_POLY], (unsigned long long)k);
      if (f >= facet_cap || st + k > pool_cap) {
        atomicOr(&w[W_ERR], (unsigned long long)ERR_CAP);
      } else {
        facets[3 * f] = int32_t(st);
        facets[3 * f + 1] = k;
        facets[3 * f + 2] = s;
        s_base = st;
        if (on_plane > 3) atomicAdd(&w[W_DEGEN], 1ull);
      }
    }
  }
  __syncthreads();
  if (s_base >= 0)
    for (int i = threadIdx.x; i < k; i += 256) pool[s_base + i] = poly[i];
}

// One block per facet of the round: its directed edges into the set, their reverses into the next
// candidates, the fan from the vertex of lowest index into the triangles.
__global__ __launch_bounds__(64) void k_hull_facets(const int32_t* __restrict__ facets, long long f_begin,
                                                    long long facet_cap, const int32_t* __restrict__ pool, EdgeSet h,
                                                    int32_t* __restrict__ next, long long next_cap,
                                                    int32_t* __restrict__ ta, int32_t* __restrict__ tb,
                                                    int32_t* __restrict__ tc, long long tri_cap,
                                                    unsigned long long* __restrict__ w) {
  __shared__ int s_v0, s_i0;
  __shared__ long long s_e, s_t;
  const long long f = f_begin + blockIdx.x;
  if (f >= (long long)w[W_FACETS] || f >= facet_cap) return;
  const int st = facets[3 * f], k = facets[3 * f + 1], s = facets[3 * f + 2];
  if (threadIdx.x == 0) s_v0 = INT_MAX;
  __syncthreads();
  for (int i = threadIdx.x; i < k; i += 64) atomicMin(&s_v0, pool[st + i]);
  __syncthreads();
  const int v0 = s_v0;
  for (int i = threadIdx.x; i < k; i += 64)
    if (pool[st + i] == v0) s_i0 = i;
  if (threadIdx.x == 0) {
    s_e = (long long)atomicAdd(&w[W_NEXT], (unsigned long long)k);
    s_t = (long long)atomicAdd(&w[W_TRIS], (unsigned long long)(k - 2));
    if (s_e + k > next_cap || s_t + (k - 2) > tri_cap) {
      atomicOr(&w[W_ERR], (unsigned long long)ERR_CAP);
      s_e = -1;
    }
  }
  __syncthreads();
  if (s_e < 0) return;
  const int i0 = s_i0;
  for (int i = threadIdx.x; i < k; i += 64) {
    const int x = pool[st + i], y = pool[st + (i + 1 == k ? 0 : i + 1)];
    if (!set_insert(h, ekey(x, y))) atomicOr(&w[W_ERR], (unsigned long long)ERR_SET);
    next[3 * (s_e + i)] = y;
    next[3 * (s_e + i) + 1] = x;
    next[3 * (s_e + i) + 2] = s;
  }
  for (int r = threadIdx.x; r < k - 2; r += 64) {  // the edges that do not touch v0, in polygon order
    const int x = pool[st + (i0 + 1 + r) % k], y = pool[st + (i0 + 2 + r) % k];
    ta[s_t + r] = v0;
    tb[s_t + r] = x;
    tc[s_t + r] = y;
  }
}

// ---- clouds: points, their original indices, segment offsets ----------------------------------------
struct Cloud {
  int32_t* pts = nullptr;   // [m,3]
  int32_t* orig = nullptr;  // [m] index into the caller's array; null: the identity
  int32_t* seg = nullptr;   // device [S + 1]
  std::vector<int32_t> hseg;
  int64_t m = 0, S = 0;
};

__device__ __forceinline__ int seg_of(const int32_t* __restrict__ seg, int S, int i) {
  int lo = 0, hi = S;  // the last s with seg[s] <= i: skips empty segments
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_hull_seg_after(int S1, const int32_t* __restrict__ seg,
                                                        const int32_t* __restrict__ pos, int32_t* __restrict__ out) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s < S1) out[s] = pos[seg[s]];
}
__global__ __launch_bounds__(256) void k_hull_gather(int m, const int32_t* __restrict__ pos,
                                                     const int32_t* __restrict__ pts, const int32_t* __restrict__ orig,
                                                     int32_t* __restrict__ opts, int32_t* __restrict__ oorig) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const int p = pos[i];
  if (pos[i + 1] == p) return;
  opts[3 * size_t(p)] = pts[3 * size_t(i)];
  opts[3 * size_t(p) + 1] = pts[3 * size_t(i) + 1];
  opts[3 * size_t(p) + 2] = pts[3 * size_t(i) + 2];
  oorig[p] = orig ? orig[i] : i;
}

// keeps the flagged points (flags [m + 1], flags[m] == 0, scanned in place); one read-back of the offsets
static int compact_cloud(Ctx* c, const Cloud& in, int32_t* flags, Cloud* out) {
  PQ_TRY(exclusive_scan_i32(c, flags, in.m + 1));
  out->S = in.S;
  PQ_TRY(c->arena.get(size_t(in.S) + 1, &out->seg));
  hipLaunchKernelGGL(k_hull_seg_after, dim3(ceil_div(in.S + 1, 256)), dim3(256), 0, c->stream, int(in.S + 1),
                     static_cast<const int32_t*>(in.seg), static_cast<const int32_t*>(flags), out->seg);
  PQ_HIP(hipGetLastError());
  out->hseg.resize(size_t(in.S) + 1);
  PQ_TRY(fetch(c, out->hseg.data(), out->seg, size_t(in.S) + 1));
  out->m = out->hseg[size_t(in.S)];
  PQ_TRY(c->arena.get(size_t(out->m) * 3 + 3, &out->pts));
  PQ_TRY(c->arena.get(size_t(out->m) + 1, &out->orig));
  if (in.m > 0)
    hipLaunchKernelGGL(k_hull_gather, dim3(ceil_div(in.m, 256)), dim3(256), 0, c->stream, int(in.m),
                       static_cast<const int32_t*>(flags), static_cast<const int32_t*>(in.pts),
                       static_cast<const int32_t*>(in.orig), out->pts, out->orig);
  PQ_HIP(hipGetLastError());
  return 0;
}

__global__ __launch_bounds__(256) void k_hull_dedup_keys(int m, const int32_t* __restrict__ pts,
                                                         const int32_t* __restrict__ seg, int S,
                                                         const int32_t* __restrict__ segmin, int32_t* __restrict__ kx,
                                                         int32_t* __restrict__ ky, int32_t* __restrict__ kz,
                                                         int32_t* __restrict__ ks) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const int s = seg_of(seg, S, i);
  kx[i] = pts[3 * size_t(i)] - segmin[3 * size_t(s)];  // in [0, 2^20]
  ky[i] = pts[3 * size_t(i) + 1] - segmin[3 * size_t(s) + 1];
  kz[i] = pts[3 * size_t(i) + 2] - segmin[3 * size_t(s) + 2];
  ks[i] = s;
}
// perm orders the points by (segment, x, y, z, index): the first of every run of equal keys stays
__global__ __launch_bounds__(256) void k_hull_dedup_flags(int m, const int32_t* __restrict__ perm,
                                                          const int32_t* __restrict__ kx, const int32_t* __restrict__ ky,
                                                          const int32_t* __restrict__ kz, const int32_t* __restrict__ ks,
                                                          int32_t* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i > m) return;
  if (i == m) {
    flags[m] = 0;
    return;
  }
  const int j = perm[i];
  int keep = 1;
  if (i > 0) {
    const int q = perm[i - 1];
    keep = !(kx[q] == kx[j] && ky[q] == ky[j] && kz[q] == kz[j] && ks[q] == ks[j]);
  }
  flags[j] = keep;
}

static int dedup_cloud(Ctx* c, const Cloud& in, const int32_t* d_segmin, Cloud* out) {
  const int64_t m = in.m;
  int32_t *kx, *ky, *kz, *ks, *flags, *perm = nullptr;
  PQ_TRY(c->arena.get(size_t(m) + 1, &kx));
  PQ_TRY(c->arena.get(size_t(m) + 1, &ky));
  PQ_TRY(c->arena.get(size_t(m) + 1, &kz));
  PQ_TRY(c->arena.get(size_t(m) + 1, &ks));
  PQ_TRY(c->arena.get(size_t(m) + 1, &flags));
  if (m > 0) {
    hipLaunchKernelGGL(k_hull_dedup_keys, dim3(ceil_div(m, 256)), dim3(256), 0, c->stream, int(m),
                       static_cast<const int32_t*>(in.pts), static_cast<const int32_t*>(in.seg), int(in.S), d_segmin,
                       kx, ky, kz, ks);
    PQ_HIP(hipGetLastError());
    PQ_TRY(refine_order_by_key(c, m, kz, &perm, 21));
    PQ_TRY(refine_order_by_key(c, m, ky, &perm, 21));
    PQ_TRY(refine_order_by_key(c, m, kx, &perm, 21));
    PQ_TRY(refine_order_by_key(c, m, ks, &perm, bit_length(uint64_t(in.S))));
  }
  hipLaunchKernelGGL(k_hull_dedup_flags, dim3(ceil_div(m + 1, 256)), dim3(256), 0, c->stream, int(m),
                     static_cast<const int32_t*>(perm), static_cast<const int32_t*>(kx),
                     static_cast<const int32_t*>(ky), static_cast<const int32_t*>(kz), static_cast<const int32_t*>(ks),
                     flags);
  PQ_HIP(hipGetLastError());
  return compact_cloud(c, in, flags, out);
}

// ---- the wrap of a cloud without coincident points whose non-empty segments are three-dimensional ------
struct WrapOut {
  int32_t* tris = nullptr;     // device [T,3], original indices, ascending by the cloud's (a, b, c)
  int32_t* tri_ptr = nullptr;  // device [S + 1]
  int64_t T = 0, rounds = 0, degenerate = 0;
};

__global__ __launch_bounds__(256) void k_hull_rows(int T, const int32_t* __restrict__ perm,
                                                   const int32_t* __restrict__ ta, const int32_t* __restrict__ tb,
                                                   const int32_t* __restrict__ tc, const int32_t* __restrict__ orig,
                                                   int32_t* __restrict__ rows) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= T) return;
  const int j = perm[i];
  rows[3 * size_t(i)] = orig[ta[j]];
  rows[3 * size_t(i) + 1] = orig[tb[j]];
  rows[3 * size_t(i) + 2] = orig[tc[j]];
}
// tri_ptr[s] = the rows whose first vertex lies before segment s
__global__ __launch_bounds__(256) void k_hull_tri_ptr(int S1, const int32_t* __restrict__ seg, int T,
                                                      const int32_t* __restrict__ perm, const int32_t* __restrict__ ta,
                                                      int32_t* __restrict__ tri_ptr) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= S1) return;
  const int first = seg[s];
  int lo = 0, hi = T;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ta[perm[mid]] < first) lo = mid + 1; else hi = mid;
  }
  tri_ptr[s] = lo;
}

static int wrap_cloud(Ctx* c, const Cloud& cl, int64_t max_tests, int64_t* tests, WrapOut* out) {
  const int64_t C = cl.m, S = cl.S;
  // a polytope of C vertices has at most 2 C - 4 triangles and 3 C - 6 edges, 6 C - 12 directed ones; every facet
  // is emitted once, so the polygon vertices listed over all rounds are the directed edges
  const long long tri_cap = 2 * C + 4, facet_cap = 2 * C + 4, pool_cap = 6 * C + 4, edge_cap = 6 * C + S + 4;
  int64_t hsize = 64;
  while (hsize < 2 * edge_cap) hsize *= 2;
  EdgeSet h;
  h.mask = (unsigned long long)hsize - 1;
  h.shift = 64 - (bit_length(uint64_t(hsize)) - 1);
  int32_t *e_cur, *e_next, *pool, *facets, *ta, *tb, *tc;
  unsigned long long* d_w;
  PQ_TRY(c->arena.get(size_t(hsize), &h.tab));
  PQ_TRY(c->arena.get(size_t(edge_cap) * 3, &e_cur));
  PQ_TRY(c->arena.get(size_t(edge_cap) * 3, &e_next));
  PQ_TRY(c->arena.get(size_t(pool_cap), &pool));
  PQ_TRY(c->arena.get(size_t(facet_cap) * 3, &facets));
  PQ_TRY(c->arena.get(size_t(tri_cap), &ta));
  PQ_TRY(c->arena.get(size_t(tri_cap), &tb));
  PQ_TRY(c->arena.get(size_t(tri_cap), &tc));
  PQ_TRY(c->arena.get(size_t(W_WORDS), &d_w));
  PQ_HIP(hipMemsetAsync(h.tab, 0xFF, size_t(hsize) * 8, c->stream));
  PQ_HIP(hipMemsetAsync(d_w, 0, W_WORDS * 8, c->stream));
  unsigned long long w[W_WORDS] = {};
  const int64_t tests0 = *tests;
  {
    ProfScope ps(c, "hull_rounds");
    hipLaunchKernelGGL(k_hull_seed, dim3(unsigned(S)), dim3(256), 0, c->stream, static_cast<const int32_t*>(cl.pts),
                       static_cast<const int32_t*>(cl.seg), h, e_cur, d_w);
    PQ_HIP(hipGetLastError());
    long long m = S, f_begin = 0;
    // every round with an open edge adds a facet, and there are fewer than 2 C facets: the cap is never
    // reached by a correct run and ends an incorrect one
    const int64_t round_cap = 2 * C + 8;
    while (m > 0) {
      if (out->rounds >= round_cap)
        return fail(PYQSM_EHIP, "pyqsm_convex_hull: internal error, %lld rounds for %lld points",
                    (long long)out->rounds, (long long)C);
      PQ_HIP(hipMemsetAsync(d_w + W_NEXT, 0, 8, c->stream));
      hipLaunchKernelGGL(k_hull_wrap, dim3(unsigned(m)), dim3(256), 0, c->stream,
                         static_cast<const int32_t*>(cl.pts), static_cast<const int32_t*>(cl.seg),
                         static_cast<const int32_t*>(e_cur), h, pool, pool_cap, facets, facet_cap, d_w);
      PQ_HIP(hipGetLastError());
      hipLaunchKernelGGL(k_hull_facets, dim3(unsigned(m)), dim3(64), 0, c->stream,
                         static_cast<const int32_t*>(facets), f_begin, facet_cap, static_cast<const int32_t*>(pool), h,
                         e_next, edge_cap, ta, tb, tc, tri_cap, d_w);
      PQ_HIP(hipGetLastError());
      PQ_TRY(fetch(c, w, d_w, size_t(W_WORDS)));
      ++out->rounds;
      *tests = tests0 + int64_t(w[W_TESTS]);
      if (w[W_ERR] & ERR_FACET)
        return fail(PYQSM_ERANGE, "pyqsm_convex_hull: a facet with more than %d vertices", kFacetMaxVerts);
      if (w[W_ERR])
        return fail(PYQSM_EHIP, "pyqsm_convex_hull: internal error %llu in round %lld", w[W_ERR],
                    (long long)out->rounds);
      if (*tests > max_tests)
        return fail(PYQSM_ERANGE, "pyqsm_convex_hull: %lld orient tests after %lld rounds exceed max_tests = %lld",
                    (long long)*tests, (long long)out->rounds, (long long)max_tests);
      f_begin = (long long)w[W_FACETS];
      m = (long long)w[W_NEXT];
      std::swap(e_cur, e_next);
    }
  }
  out->T = int64_t(w[W_TRIS]);
  out->degenerate = int64_t(w[W_DEGEN]);
  const int T = int(out->T);
  PQ_TRY(c->arena.get(size_t(T) * 3 + 3, &out->tris));
  PQ_TRY(c->arena.get(size_t(S) + 1, &out->tri_ptr));
  ProfScope ps(c, "hull_sort");
  int32_t* perm = nullptr;
  if (T > 0) {
    const int bits = bit_length(uint64_t(C));
    PQ_TRY(refine_order_by_key(c, T, tc, &perm, bits));
    PQ_TRY(refine_order_by_key(c, T, tb, &perm, bits));
    PQ_TRY(refine_order_by_key(c, T, ta, &perm, bits));
    hipLaunchKernelGGL(k_hull_rows, dim3(ceil_div(T, 256)), dim3(256), 0, c->stream, T,
                       static_cast<const int32_t*>(perm), static_cast<const int32_t*>(ta),
                       static_cast<const int32_t*>(tb), static_cast<const int32_t*>(tc),
                       static_cast<const int32_t*>(cl.orig), out->tris);
    PQ_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_hull_tri_ptr, dim3(ceil_div(S + 1, 256)), dim3(256), 0, c->stream, int(S + 1),
                     static_cast<const int32_t*>(cl.seg), T, static_cast<const int32_t*>(perm),
                     static_cast<const int32_t*>(ta), out->tri_ptr);
  PQ_HIP(hipGetLastError());
  return 0;
}

// ---- the prefilter --------------------------------------------------------------------------------
__device__ const int kHullDir[kExtDirs][3] = {{1, 0, 0}, {0, 1, 0},  {0, 0, 1},  {1, 1, 0},  {1, -1, 0},
                                              {1, 0, 1}, {1, 0, -1}, {0, 1, 1},  {0, 1, -1}, {1, 1, 1},
                                              {1, 1, -1}, {1, -1, 1}, {1, -1, -1}};

// per task (a chunk of one segment): the point of largest and of smallest d . x for the 13 directions,
// the lowest index on ties
__global__ __launch_bounds__(256) void k_hull_extreme(const int32_t* __restrict__ ijk, const int32_t* __restrict__ task,
                                                      long long* __restrict__ pval, int32_t* __restrict__ pidx) {
  __shared__ long long sv[256];
  __shared__ int si[256];
  const int lo = task[2 * size_t(blockIdx.x)], hi = task[2 * size_t(blockIdx.x) + 1];
  long long mx[kExtDirs], mn[kExtDirs];
  int imx[kExtDirs], imn[kExtDirs];
#pragma unroll
  for (int d = 0; d < kExtDirs; ++d) {
    mx[d] = LLONG_MIN;
    mn[d] = LLONG_MAX;
    imx[d] = imn[d] = INT_MAX;
  }
  for (int i = lo + int(threadIdx.x); i < hi; i += 256) {  // ascending i: a strict comparison keeps the lowest
    const long long x = ijk[3 * size_t(i)], y = ijk[3 * size_t(i) + 1], z = ijk[3 * size_t(i) + 2];
#pragma unroll
    for (int d = 0; d < kExtDirs; ++d) {
      const long long v = kHullDir[d][0] * x + kHullDir[d][1] * y + kHullDir[d][2] * z;
      if (v > mx[d]) {
        mx[d] = v;
        imx[d] = i;
      }
      if (v < mn[d]) {
        mn[d] = v;
        imn[d] = i;
      }
    }
  }
#pragma unroll
  for (int d = 0; d < 2 * kExtDirs; ++d) {
    const bool neg = d >= kExtDirs;
    const int dd = neg ? d - kExtDirs : d;
    const int mi = neg ? imn[dd] : imx[dd];
    sv[threadIdx.x] = mi == INT_MAX ? LLONG_MIN : (neg ? -mn[dd] : mx[dd]);
    si[threadIdx.x] = mi;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if (int(threadIdx.x) < off) {
        const long long ov = sv[threadIdx.x + off];
        const int oi = si[threadIdx.x + off];
        if (ov > sv[threadIdx.x] || (ov == sv[threadIdx.x] && oi < si[threadIdx.x])) {
          sv[threadIdx.x] = ov;
          si[threadIdx.x] = oi;
        }
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      pval[size_t(blockIdx.x) * 2 * kExtDirs + d] = sv[0];
      pidx[size_t(blockIdx.x) * 2 * kExtDirs + d] = si[0];
    }
    __syncthreads();
  }
}
// one block per segment: folds its tasks, adds the four independent points, gathers the small cloud
__global__ __launch_bounds__(64) void k_hull_extreme_fold(const int32_t* __restrict__ task_start,
                                                          const long long* __restrict__ pval,
                                                          const int32_t* __restrict__ pidx, const int32_t* __restrict__ tet,
                                                          const int32_t* __restrict__ eseg, const int32_t* __restrict__ ijk,
                                                          int32_t* __restrict__ epts, int32_t* __restrict__ eorig) {
  const int s = blockIdx.x, d = threadIdx.x;
  if (eseg[s + 1] == eseg[s] || d >= kExtSlots) return;
  int idx;
  if (d < 2 * kExtDirs) {
    long long bv = LLONG_MIN;
    idx = INT_MAX;
    for (int t = task_start[s]; t < task_start[s + 1]; ++t) {
      const long long v = pval[size_t(t) * 2 * kExtDirs + d];
      const int i = pidx[size_t(t) * 2 * kExtDirs + d];
      if (i != INT_MAX && (v > bv || (v == bv && i < idx))) {
        bv = v;
        idx = i;
      }
    }
  } else {
    idx = tet[4 * size_t(s) + (d - 2 * kExtDirs)];
  }
  const size_t o = size_t(eseg[s]) + d;
  epts[3 * o] = ijk[3 * size_t(idx)];
  epts[3 * o + 1] = ijk[3 * size_t(idx) + 1];
  epts[3 * o + 2] = ijk[3 * size_t(idx) + 2];
  eorig[o] = idx;
}

struct HullPlane {
  long long nx, ny, nz;
  int32_t ax, ay, az, pad;
};
__global__ __launch_bounds__(256) void k_hull_planes(int T, const int32_t* __restrict__ tris,
                                                     const int32_t* __restrict__ ijk, HullPlane* __restrict__ pl) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const int32_t *a = ijk + 3 * size_t(tris[3 * size_t(t)]), *b = ijk + 3 * size_t(tris[3 * size_t(t) + 1]),
                *cc = ijk + 3 * size_t(tris[3 * size_t(t) + 2]);
  const V3 n = cross(diff(b, a), diff(cc, a));
  pl[t] = HullPlane{n.x, n.y, n.z, a[0], a[1], a[2], 0};
}
// flags[i] = 1 unless point i is strictly inside its segment's polytope (a segment without one: 0)
__global__ __launch_bounds__(256) void k_hull_prefilter(int n, const int32_t* __restrict__ ijk,
                                                        const int32_t* __restrict__ seg, int S,
                                                        const HullPlane* __restrict__ pl,
                                                        const int32_t* __restrict__ tri_ptr, int32_t* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  if (i == n) {
    flags[n] = 0;
    return;
  }
  const int s = seg_of(seg, S, i);
  const int32_t* q = ijk + 3 * size_t(i);
  int out = 0;
  for (int t = tri_ptr[s]; t < tri_ptr[s + 1]; ++t) {
    const HullPlane p = pl[t];
    const int32_t a[3] = {p.ax, p.ay, p.az};
    if (dot(V3{p.nx, p.ny, p.nz}, diff(q, a)) >= 0) {
      out = 1;
      break;
    }
  }
  flags[i] = out;
}

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_convex_hull(const int32_t* ijk, int64_t n, const int64_t* seg_start, int64_t n_seg, int64_t max_tests,
                      int32_t** tris, int64_t** tri_ptr, int32_t* dim, int64_t* stats, int32_t device) {
  PQ_API_RANGE("pyqsm_convex_hull");
  if (tris) *tris = nullptr;
  if (tri_ptr) *tri_ptr = nullptr;
  if (stats) std::fill(stats, stats + PYQSM_HULL_N_STATS, int64_t(0));
  if (n < 0 || n_seg < 0) return fail(PYQSM_EINVAL, "negative size");
  if (!seg_start || !tris || !tri_ptr || (n > 0 && !ijk) || (n_seg > 0 && !dim))
    return fail(PYQSM_EINVAL, "pyqsm_convex_hull: NULL pointer");
  if (seg_start[0] != 0 || seg_start[n_seg] != n) return fail(PYQSM_EINVAL, "seg_start must run from 0 to n");
  for (int64_t s = 0; s < n_seg; ++s)
    if (seg_start[s + 1] < seg_start[s]) return fail(PYQSM_EINVAL, "seg_start must not decrease");
  if (n > 0x7FFFFF00LL / 4 || n_seg > 0x7FFFFF00LL / kExtSlots)
    return fail(PYQSM_ERANGE, "more than 2^29 points per call");
  if (max_tests <= 0) max_tests = kHullDefaultMaxTests;

  // per segment on the host: the extent, the affine dimension and, when that is 3, four independent points
  std::vector<int32_t> segmin(size_t(n_seg) * 3 + 3, 0), tet(size_t(n_seg) * 4 + 4, 0), hseg(size_t(n_seg) + 1),
      eseg(size_t(n_seg) + 1), task, task_start(size_t(n_seg) + 1);
  int64_t n_active = 0;
  for (int64_t s = 0; s < n_seg; ++s) {
    const int64_t lo = seg_start[s], hi = seg_start[s + 1];
    hseg[size_t(s)] = int32_t(lo);
    eseg[size_t(s)] = int32_t(n_active * kExtSlots);
    task_start[size_t(s)] = int32_t(task.size() / 2);
    dim[s] = -1;
    if (hi == lo) continue;
    int32_t mn[3], mx[3];
    for (int a = 0; a < 3; ++a) mn[a] = mx[a] = ijk[3 * lo + a];
    for (int64_t i = lo; i < hi; ++i)
      for (int a = 0; a < 3; ++a) {
        mn[a] = std::min(mn[a], ijk[3 * i + a]);
        mx[a] = std::max(mx[a], ijk[3 * i + a]);
      }
    for (int a = 0; a < 3; ++a) {
      if (int64_t(mx[a]) - mn[a] > kHullMaxExtent)
        return fail(PYQSM_EINVAL, "segment %lld spans %lld lattice units, more than 2^20: use a coarser quantum",
                    (long long)s, (long long)(int64_t(mx[a]) - mn[a]));
      segmin[3 * size_t(s) + a] = mn[a];
    }
    int d = 0;
    int64_t p1 = -1, p2 = -1, p3 = -1;
    const int32_t* p0 = ijk + 3 * lo;
    V3 e1{0, 0, 0}, nrm{0, 0, 0};
    for (int64_t i = lo + 1; i < hi && d < 3; ++i) {
      const V3 w = diff(ijk + 3 * i, p0);
      if (d == 0) {
        if (!is_zero(w)) {
          p1 = i;
          e1 = w;
          d = 1;
        }
      } else if (d == 1) {
        const V3 cr = cross(e1, w);
        if (!is_zero(cr)) {
          p2 = i;
          nrm = cr;
          d = 2;
        }
      } else if (dot(nrm, w) != 0) {
        p3 = i;
        d = 3;
      }
    }
    dim[s] = d;
    if (d < 3) continue;
    const int64_t t4[4] = {lo, p1, p2, p3};
    for (int a = 0; a < 4; ++a) tet[4 * size_t(s) + a] = int32_t(t4[a]);
    for (int64_t b = lo; b < hi; b += kExtChunk) {
      task.push_back(int32_t(b));
      task.push_back(int32_t(std::min<int64_t>(b + kExtChunk, hi)));
    }
    ++n_active;
  }
  hseg[size_t(n_seg)] = int32_t(n);
  eseg[size_t(n_seg)] = int32_t(n_active * kExtSlots);
  task_start[size_t(n_seg)] = int32_t(task.size() / 2);

  OutBufs ob;
  int64_t* h_ptr = ob.get<int64_t>(size_t(n_seg) + 1);
  if (!h_ptr) return fail(PYQSM_ENOMEM, "pyqsm_convex_hull: no host memory");
  std::fill(h_ptr, h_ptr + n_seg + 1, int64_t(0));
  if (n_active == 0) {  // no segment has a three-dimensional hull: no device work
    ob.kept = true;
    *tri_ptr = h_ptr;
    return 0;
  }

  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  const int64_t S = n_seg, n_task = int64_t(task.size() / 2);
  Cloud full, ext, ext1, cand, cand1;
  int32_t *d_segmin, *d_tet, *d_task, *d_task_start, *d_pidx, *d_flags;
  long long* d_pval;
  full.m = n;
  full.S = S;
  full.hseg = hseg;
  PQ_TRY(upload(c, ijk, size_t(n) * 3, &full.pts));
  PQ_TRY(upload(c, hseg.data(), size_t(S) + 1, &full.seg));
  PQ_TRY(upload(c, segmin.data(), size_t(S) * 3 + 3, &d_segmin));
  PQ_TRY(upload(c, tet.data(), size_t(S) * 4 + 4, &d_tet));
  PQ_TRY(upload(c, task.data(), task.size(), &d_task));
  PQ_TRY(upload(c, task_start.data(), size_t(S) + 1, &d_task_start));
  ext.m = n_active * kExtSlots;
  ext.S = S;
  ext.hseg = eseg;
  PQ_TRY(upload(c, eseg.data(), size_t(S) + 1, &ext.seg));
  PQ_TRY(c->arena.get(size_t(ext.m) * 3, &ext.pts));
  PQ_TRY(c->arena.get(size_t(ext.m), &ext.orig));
  PQ_TRY(c->arena.get(size_t(n_task) * 2 * kExtDirs, &d_pval));
  PQ_TRY(c->arena.get(size_t(n_task) * 2 * kExtDirs, &d_pidx));
  PQ_TRY(c->arena.get(size_t(n) + 1, &d_flags));

  int64_t tests = 0;
  WrapOut small, big;
  {
    ProfScope ps(c, "hull_prefilter");
    hipLaunchKernelGGL(k_hull_extreme, dim3(unsigned(n_task)), dim3(256), 0, c->stream,
                       static_cast<const int32_t*>(full.pts), static_cast<const int32_t*>(d_task), d_pval, d_pidx);
    PQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_hull_extreme_fold, dim3(unsigned(S)), dim3(64), 0, c->stream,
                       static_cast<const int32_t*>(d_task_start), static_cast<const long long*>(d_pval),
                       static_cast<const int32_t*>(d_pidx), static_cast<const int32_t*>(d_tet),
                       static_cast<const int32_t*>(ext.seg), static_cast<const int32_t*>(full.pts), ext.pts, ext.orig);
    PQ_HIP(hipGetLastError());
    PQ_TRY(dedup_cloud(c, ext, d_segmin, &ext1));
    PQ_TRY(wrap_cloud(c, ext1, max_tests, &tests, &small));
    HullPlane* d_pl;
    PQ_TRY(c->arena.get(size_t(small.T) + 1, &d_pl));
    hipLaunchKernelGGL(k_hull_planes, dim3(ceil_div(small.T, 256)), dim3(256), 0, c->stream, int(small.T),
                       static_cast<const int32_t*>(small.tris), static_cast<const int32_t*>(full.pts), d_pl);
    PQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_hull_prefilter, dim3(ceil_div(n + 1, 256)), dim3(256), 0, c->stream, int(n),
                       static_cast<const int32_t*>(full.pts), static_cast<const int32_t*>(full.seg), int(S),
                       static_cast<const HullPlane*>(d_pl), static_cast<const int32_t*>(small.tri_ptr), d_flags);
    PQ_HIP(hipGetLastError());
    PQ_TRY(compact_cloud(c, full, d_flags, &cand));
    PQ_TRY(dedup_cloud(c, cand, d_segmin, &cand1));
  }
  PQ_TRY(wrap_cloud(c, cand1, max_tests, &tests, &big));

  std::vector<int32_t> h_tp(size_t(S) + 1);
  int32_t* h_tris = ob.get<int32_t>(size_t(big.T) * 3);
  if (!h_tris) return fail(PYQSM_ENOMEM, "pyqsm_convex_hull: no host memory for %lld triangles", (long long)big.T);
  PQ_TRY(download(c, h_tris, big.tris, size_t(big.T) * 3));
  PQ_TRY(fetch(c, h_tp.data(), big.tri_ptr, size_t(S) + 1));
  for (int64_t s = 0; s <= S; ++s) h_ptr[s] = h_tp[size_t(s)];
  if (h_ptr[S] != big.T)
    return fail(PYQSM_EHIP, "pyqsm_convex_hull: internal error, %lld rows listed, %lld counted", (long long)h_ptr[S],
                (long long)big.T);
  if (stats) {
    stats[0] = cand.m;
    stats[1] = big.rounds;
    stats[2] = tests;
    stats[3] = big.degenerate;
    stats[4] = cand.m - cand1.m;
    stats[5] = small.rounds;
  }
  ob.kept = true;
  *tris = h_tris;
  *tri_ptr = h_ptr;
  return 0;
}

}  // extern "C"
