// mesh.hip — checks of a triangle mesh before rays are cast at it: what
// pyQSM's geometry/mesh_processing.py asks of Open3D (cluster_connected_triangles, the manifold
// tests, is_orientable, get_self_intersecting_triangles), specified here by a contract of integer
// decisions with a fixed output order.
//
// pyqsm_mesh_topology: the 3T half-edges are sorted by (min, max) with two stable radix passes; runs
// of equal keys are the edges. Three union-finds (unionfind.hpp) hang on the runs: triangles (the
// clusters), the 3T corners (the fan test of vertex manifoldness) and the double cover (t, flip)
// (orientability). Cluster areas are summed by one wave per cluster in a fixed order.
//
// pyqsm_mesh_self_intersections: an upper-triangular brute-force sweep of 256 x 256 tiles of integer
// boxes; the rare survivors go to an exact tri-tri test in int64 on lattice coordinates.
#include <algorithm>

#include "common.hpp"
#include "mesh_halfedge.hpp"
#include "unionfind.hpp"

namespace pyqsm {

namespace {

constexpr int64_t kMeshMaxTris = int64_t(1) << 29;      // 3T half-edges stay below 2^31
constexpr int64_t kMeshMaxExtent = int64_t(1) << 20;    // lattice units per axis: orient3d fits int64
constexpr int kRows = PYQSM_MESH_TILE_ROWS;             // row and column triangles of a tile
constexpr int kColTiles = 8;                            // column tiles one block sweeps
constexpr int64_t kSweepMaxTris = int64_t(1) << 26;     // grid.y = tiles / kColTiles <= 65535
static_assert(kRows == 256, "one thread per row triangle of a 256-thread block");

// ---------------------------------------------------------------- topology

// The half-edge convention, the sort and the runs: mesh_halfedge.hpp, shared with holes.hip.

// One thread per sorted half-edge. The head of a run writes the edge's row; every other half-edge
// of the run is linked to the head: their triangles, their corners at both end vertices and, on an
// edge of exactly two triangles, their nodes of the double cover.
__global__ __launch_bounds__(256) void k_mesh_edges(int n, const int32_t* __restrict__ tris,
                                                    const int32_t* __restrict__ hs, const int32_t* __restrict__ x,
                                                    const int32_t* __restrict__ first, int32_t* __restrict__ edges,
                                                    int32_t* __restrict__ edge_count, uint8_t* __restrict__ edge_flags,
                                                    int32_t* par_tri, int32_t* par_corner, int32_t* par_cover,
                                                    unsigned long long* __restrict__ counters) {
  __shared__ unsigned s_cnt[3];
  if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const int e = x[i + 1] - 1, f = first[e], cnt = first[e + 1] - f;
    const int h = hs[i];
    int u, w;
    half_edge(tris, h, u, w);
    if (i == f) {
      int flags = cnt == 1 ? 1 : (cnt > 2 ? 2 : 0);
      if (cnt == 2) {
        int u1, w1;
        half_edge(tris, hs[f + 1], u1, w1);
        if (u1 == u) flags |= 4;
      }
      edges[2 * size_t(e)] = min(u, w);
      edges[2 * size_t(e) + 1] = max(u, w);
      edge_count[e] = cnt;
      edge_flags[e] = uint8_t(flags);
      if (flags & 1) atomicAdd(&s_cnt[0], 1u);
      if (flags & 2) atomicAdd(&s_cnt[1], 1u);
      if (flags & 4) atomicAdd(&s_cnt[2], 1u);
    } else {
      const int h0 = hs[f];
      int u0, w0;
      half_edge(tris, h0, u0, w0);
      const int t = h / 3, t0 = h0 / 3;
      const int k = h - 3 * t, k0 = h0 - 3 * t0;
      const int nxt = 3 * t + (k == 2 ? 0 : k + 1), nxt0 = 3 * t0 + (k0 == 2 ? 0 : k0 + 1);
      const bool same = u0 == u;  // both run min -> max, or both max -> min
      uf_union(par_tri, t0, t);
      // corner h holds u, corner nxt holds w: link the corners that hold the same vertex
      uf_union(par_corner, h0, same ? h : nxt);
      uf_union(par_corner, nxt0, same ? nxt : h);
      if (cnt == 2) {  // same direction: the two triangles need different flips
        uf_union(par_cover, 2 * t0, 2 * t + (same ? 1 : 0));
        uf_union(par_cover, 2 * t0 + 1, 2 * t + (same ? 0 : 1));
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < 3 && s_cnt[threadIdx.x]) atomicAdd(&counters[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_mesh_root_flags(int n, const int32_t* __restrict__ parent,
                                                         int32_t* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i <= n) flags[i] = (i < n && parent[i] == i) ? 1 : 0;
}

// clusters numbered by ascending smallest member: the rank of the root among the roots
__global__ __launch_bounds__(256) void k_mesh_tri_cluster(int n, const int32_t* __restrict__ parent,
                                                          const int32_t* __restrict__ x, int32_t* __restrict__ cl,
                                                          uint32_t* __restrict__ keys, int32_t* __restrict__ vals) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = x[parent[i]];
  cl[i] = c;
  keys[i] = uint32_t(c);
  vals[i] = i;
}

// keys: the cluster of every triangle, sorted; every cluster has a member
__global__ __launch_bounds__(256) void k_mesh_cluster_start(int n, int ncl, const uint32_t* __restrict__ keys,
                                                            int32_t* __restrict__ start) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (i == 0 || keys[i] != keys[i - 1]) start[keys[i]] = i;
  if (i == 0) start[ncl] = n;
}

__device__ __forceinline__ double tri_area(const double* __restrict__ verts, const int32_t* __restrict__ tris, int t) {
  const double* a = verts + 3 * size_t(tris[3 * size_t(t)]);
  const double* b = verts + 3 * size_t(tris[3 * size_t(t) + 1]);
  const double* c = verts + 3 * size_t(tris[3 * size_t(t) + 2]);
  const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
  const double vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
  const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
  return 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
}

// One wave per cluster, its triangles in ascending order: lane l adds members l, l + 64, ... in that
// order, then the 64 partial sums are folded by a fixed butterfly. No atomics: the same bits on every run.
__global__ __launch_bounds__(256) void k_mesh_cluster_sums(int ncl, const int32_t* __restrict__ start,
                                                           const int32_t* __restrict__ members,
                                                           const int32_t* __restrict__ tris,
                                                           const double* __restrict__ verts /*may be null*/,
                                                           int64_t* __restrict__ cluster_n,
                                                           double* __restrict__ cluster_area) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= ncl) return;  // wave-uniform
  const int lo = start[c], hi = start[c + 1];
  if (lane == 0) cluster_n[c] = hi - lo;
  if (!verts) return;
  double s = 0.0;
  for (int p = lo + lane; p < hi; p += 64) s += tri_area(verts, tris, members[p]);
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  if (lane == 0) cluster_area[c] = s;
}

// vroots[v]: how many corner sets meet at v (0: no triangle there)
__global__ __launch_bounds__(256) void k_mesh_vertex_roots(int n, const int32_t* __restrict__ par_corner,
                                                           const int32_t* __restrict__ tris,
                                                           int32_t* __restrict__ vroots) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n && par_corner[i] == i) atomicAdd(&vroots[tris[i]], 1);
}

__global__ __launch_bounds__(256) void k_mesh_vertex_flags(int nv, const int32_t* __restrict__ vroots,
                                                           uint8_t* __restrict__ vflags,
                                                           unsigned long long* __restrict__ counters) {
  __shared__ unsigned s_cnt[2];
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v < nv) {
    const int r = vroots[v];
    vflags[v] = r > 1 ? 1 : 0;
    if (r > 1) atomicAdd(&s_cnt[0], 1u);
    if (r == 0) atomicAdd(&s_cnt[1], 1u);
  }
  __syncthreads();
  if (threadIdx.x < 2 && s_cnt[threadIdx.x])
    atomicAdd(&counters[3 + threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// non-orientable iff some triangle meets its own flipped copy
__global__ __launch_bounds__(256) void k_mesh_cover_check(int nt, const int32_t* __restrict__ par_cover,
                                                          unsigned long long* __restrict__ counters) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < nt && par_cover[2 * t] == par_cover[2 * t + 1]) atomicOr(&counters[5], 1ull);
}

// ---------------------------------------------------------------- self-intersection

// Per triangle: box[2 t] = (min x, y, z, degenerate), box[2 t + 1] = (max x, y, z, 0) and
// tv[3 t ..] = the nine coordinates and the three vertex indices, all relative to `origin` (so in
// [0, 2^20]).
__global__ __launch_bounds__(256) void k_mesh_tri_setup(int nt, const int32_t* __restrict__ ijk,
                                                        const int32_t* __restrict__ tris, int ox, int oy, int oz,
                                                        int4* __restrict__ box, int4* __restrict__ tv,
                                                        unsigned long long* __restrict__ counters) {
  __shared__ unsigned s_deg;
  if (threadIdx.x == 0) s_deg = 0;
  __syncthreads();
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < nt) {
    const int ia = tris[3 * size_t(t)], ib = tris[3 * size_t(t) + 1], ic = tris[3 * size_t(t) + 2];
    const int ax = ijk[3 * size_t(ia)] - ox, ay = ijk[3 * size_t(ia) + 1] - oy, az = ijk[3 * size_t(ia) + 2] - oz;
    const int bx = ijk[3 * size_t(ib)] - ox, by = ijk[3 * size_t(ib) + 1] - oy, bz = ijk[3 * size_t(ib) + 2] - oz;
    const int cx = ijk[3 * size_t(ic)] - ox, cy = ijk[3 * size_t(ic) + 1] - oy, cz = ijk[3 * size_t(ic) + 2] - oz;
    const int64_t ux = bx - ax, uy = by - ay, uz = bz - az, vx = cx - ax, vy = cy - ay, vz = cz - az;
    const int deg = (uy * vz - uz * vy == 0) && (uz * vx - ux * vz == 0) && (ux * vy - uy * vx == 0);
    box[2 * size_t(t)] = make_int4(min(ax, min(bx, cx)), min(ay, min(by, cy)), min(az, min(bz, cz)), deg);
    box[2 * size_t(t) + 1] = make_int4(max(ax, max(bx, cx)), max(ay, max(by, cy)), max(az, max(bz, cz)), 0);
    tv[3 * size_t(t)] = make_int4(ax, ay, az, bx);
    tv[3 * size_t(t) + 1] = make_int4(by, bz, cx, cy);
    tv[3 * size_t(t) + 2] = make_int4(cz, ia, ib, ic);
    if (deg) atomicAdd(&s_deg, 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_deg) atomicAdd(&counters[3], (unsigned long long)s_deg);
}

struct I3 {
  int64_t x, y, z;
};

// Every difference is at most 2^20 in magnitude: a cross component is below 2^41, the determinant
// below 3 * 2^61 < 2^63.
__device__ __forceinline__ int64_t orient3d(const I3& a, const I3& b, const I3& c, const I3& d) {
  const int64_t ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z;
  const int64_t vx = c.x - a.x, vy = c.y - a.y, vz = c.z - a.z;
  const int64_t wx = d.x - a.x, wy = d.y - a.y, wz = d.z - a.z;
  return wx * (uy * vz - uz * vy) + wy * (uz * vx - ux * vz) + wz * (ux * vy - uy * vx);
}

__device__ __forceinline__ int sgn(int64_t v) { return (v > 0) - (v < 0); }

struct I2 {
  int64_t x, y;
};

__device__ __forceinline__ int64_t orient2d(const I2& a, const I2& b, const I2& c) {
  return (b.x - a.x) * (c.y - a.y) - (b.y - a.y) * (c.x - a.x);
}

// c, known to lie on the line through a and b, lies on the closed segment ab
__device__ __forceinline__ bool on_segment(const I2& a, const I2& b, const I2& c) {
  return min(a.x, b.x) <= c.x && c.x <= max(a.x, b.x) && min(a.y, b.y) <= c.y && c.y <= max(a.y, b.y);
}

__device__ bool seg_seg_2d(const I2& p, const I2& q, const I2& a, const I2& b) {
  const int d1 = sgn(orient2d(p, q, a)), d2 = sgn(orient2d(p, q, b));
  const int d3 = sgn(orient2d(a, b, p)), d4 = sgn(orient2d(a, b, q));
  if (d1 * d2 < 0 && d3 * d4 < 0) return true;
  if (d1 == 0 && on_segment(p, q, a)) return true;
  if (d2 == 0 && on_segment(p, q, b)) return true;
  if (d3 == 0 && on_segment(a, b, p)) return true;
  if (d4 == 0 && on_segment(a, b, q)) return true;
  return false;
}

// no strict sign disagreement among three values
__device__ __forceinline__ bool agree(int a, int b, int c) {
  return !((a > 0 || b > 0 || c > 0) && (a < 0 || b < 0 || c < 0));
}

__device__ bool point_in_tri_2d(const I2& p, const I2* t) {
  return agree(sgn(orient2d(t[0], t[1], p)), sgn(orient2d(t[1], t[2], p)), sgn(orient2d(t[2], t[0], p)));
}

__device__ __forceinline__ I2 drop_axis(const I3& v, int axis) {
  return axis == 0 ? I2{v.y, v.z} : (axis == 1 ? I2{v.z, v.x} : I2{v.x, v.y});
}

// The closed segment pq meets the closed, non-degenerate triangle t; axis: where t's normal is largest.
__device__ __noinline__ bool seg_tri(const I3& p, const I3& q, const I3* t, int axis) {
  const int sp = sgn(orient3d(t[0], t[1], t[2], p)), sq = sgn(orient3d(t[0], t[1], t[2], q));
  if (sp * sq > 0) return false;
  if (sp == 0 && sq == 0) {  // in t's plane: 2-D, the projection along `axis` is one to one there
    const I2 p2 = drop_axis(p, axis), q2 = drop_axis(q, axis);
    const I2 t2[3] = {drop_axis(t[0], axis), drop_axis(t[1], axis), drop_axis(t[2], axis)};
    return point_in_tri_2d(p2, t2) || point_in_tri_2d(q2, t2) || seg_seg_2d(p2, q2, t2[0], t2[1]) ||
           seg_seg_2d(p2, q2, t2[1], t2[2]) || seg_seg_2d(p2, q2, t2[2], t2[0]);
  }
  // pq crosses the plane in one point: inside t iff the line passes the three edges on one side
  return agree(sgn(orient3d(p, q, t[0], t[1])), sgn(orient3d(p, q, t[1], t[2])), sgn(orient3d(p, q, t[2], t[0])));
}

__device__ __forceinline__ int normal_axis(const I3* t) {
  const int64_t ux = t[1].x - t[0].x, uy = t[1].y - t[0].y, uz = t[1].z - t[0].z;
  const int64_t vx = t[2].x - t[0].x, vy = t[2].y - t[0].y, vz = t[2].z - t[0].z;
  int64_t nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
  nx = nx < 0 ? -nx : nx;
  ny = ny < 0 ? -ny : ny;
  nz = nz < 0 ? -nz : nz;
  return (nx >= ny && nx >= nz) ? 0 : (ny >= nz ? 1 : 2);
}

// two non-degenerate closed triangles have a common point iff an edge of one meets the other
__device__ bool tri_tri(const I3* a, const I3* b) {
  const int axa = normal_axis(a), axb = normal_axis(b);
#pragma unroll 1
  for (int k = 0; k < 3; ++k) {
    const int k1 = k == 2 ? 0 : k + 1;
    if (seg_tri(a[k], a[k1], b, axb)) return true;
    if (seg_tri(b[k], b[k1], a, axa)) return true;
  }
  return false;
}

__device__ __forceinline__ void load_tri(const int4* __restrict__ tv, int t, I3* v, int* idx) {
  const int4 r0 = tv[3 * size_t(t)], r1 = tv[3 * size_t(t) + 1], r2 = tv[3 * size_t(t) + 2];
  v[0] = I3{r0.x, r0.y, r0.z};
  v[1] = I3{r0.w, r1.x, r1.y};
  v[2] = I3{r1.z, r1.w, r2.x};
  idx[0] = r2.y;
  idx[1] = r2.z;
  idx[2] = r2.w;
}

// The narrow phase of one box survivor i < j. Returns bit 0: skipped for a shared index, bit 1: exact
// test run. Out of line, so that the sweep's inner loop keeps its registers.
__device__ __noinline__ int mesh_narrow(int i, int j, int degenerate, const int4* __restrict__ tv,
                                        uint32_t* __restrict__ hit, unsigned long long* __restrict__ cursor,
                                        long long cap, int32_t* __restrict__ pi, int32_t* __restrict__ pj) {
  I3 a[3], b[3];
  int ia[3], ib[3];
  load_tri(tv, i, a, ia);
  load_tri(tv, j, b, ib);
  for (int k = 0; k < 3; ++k)
    if (ia[k] == ib[0] || ia[k] == ib[1] || ia[k] == ib[2]) return 1;
  if (degenerate) return 0;
  if (tri_tri(a, b)) {
    atomicOr(&hit[i >> 2], 1u << (8 * (i & 3)));
    atomicOr(&hit[j >> 2], 1u << (8 * (j & 3)));
    const unsigned long long slot = atomicAdd(cursor, 1ull);
    if ((long long)slot < cap) {
      pi[slot] = i;
      pj[slot] = j;
    }
  }
  return 2;
}

// Block (x = row tile ti, y = chunk): the 256 row triangles of tile ti, one per thread with its box in
// registers, against column tiles ti + 8 y .. ti + 8 y + 7, each staged in LDS (every lane reads
// the same address: a broadcast). Rows and columns past T carry an empty box.
// counters: 0 box survivors, 1 skipped for a shared index, 2 exact tests, 3 degenerate triangles
// (k_mesh_tri_setup), 4 the pair cursor.
__global__ __launch_bounds__(256) void k_mesh_sweep(int nt, int ntile, const int4* __restrict__ box,
                                                    const int4* __restrict__ tv, uint32_t* __restrict__ hit,
                                                    unsigned long long* __restrict__ counters, long long cap,
                                                    int32_t* __restrict__ pi, int32_t* __restrict__ pj) {
  __shared__ int4 s_box[2 * kRows];
  __shared__ unsigned long long s_cnt[3];
  const int ti = blockIdx.x, tj0 = ti + int(blockIdx.y) * kColTiles;
  if (tj0 >= ntile) return;  // block-uniform
  if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
  const int4 kEmptyLo = make_int4(INT32_MAX, INT32_MAX, INT32_MAX, 0), kEmptyHi = make_int4(-1, -1, -1, 0);
  const int i = ti * kRows + int(threadIdx.x);
  const int4 lo = i < nt ? box[2 * size_t(i)] : kEmptyLo, hi = i < nt ? box[2 * size_t(i) + 1] : kEmptyHi;
  unsigned n_surv = 0, n_skip = 0, n_exact = 0;
  const int tj1 = min(tj0 + kColTiles, ntile);
  for (int tj = tj0; tj < tj1; ++tj) {
    __syncthreads();  // the previous tile has been read
    const int jl = tj * kRows + int(threadIdx.x);
    s_box[2 * threadIdx.x] = jl < nt ? box[2 * size_t(jl)] : kEmptyLo;
    s_box[2 * threadIdx.x + 1] = jl < nt ? box[2 * size_t(jl) + 1] : kEmptyHi;
    __syncthreads();
    const int c0 = tj == ti ? int(threadIdx.x) + 1 : 0;  // the diagonal tile: columns j > i only
    for (int c = c0; c < kRows; ++c) {
      const int4 clo = s_box[2 * c], chi = s_box[2 * c + 1];
      if (lo.x <= chi.x && clo.x <= hi.x && lo.y <= chi.y && clo.y <= hi.y && lo.z <= chi.z && clo.z <= hi.z) {
        ++n_surv;
        const int r = mesh_narrow(i, tj * kRows + c, lo.w | clo.w, tv, hit, counters + 4, cap, pi, pj);
        n_skip += r & 1;
        n_exact += r >> 1;
      }
    }
  }
  if (n_surv) atomicAdd(&s_cnt[0], (unsigned long long)n_surv);
  if (n_skip) atomicAdd(&s_cnt[1], (unsigned long long)n_skip);
  if (n_exact) atomicAdd(&s_cnt[2], (unsigned long long)n_exact);
  __syncthreads();
  if (threadIdx.x < 3 && s_cnt[threadIdx.x]) atomicAdd(&counters[threadIdx.x], s_cnt[threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_mesh_pair_rows(int n, const int32_t* __restrict__ perm,
                                                        const int32_t* __restrict__ pi, const int32_t* __restrict__ pj,
                                                        int32_t* __restrict__ rows) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int q = perm[p];
  rows[2 * size_t(p)] = pi[q];
  rows[2 * size_t(p) + 1] = pj[q];
}

}  // namespace

}  // namespace pyqsm

using namespace pyqsm;

#define PQ_LAUNCH(kernel, blocks, ...)                                               \
  do {                                                                               \
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, c->stream, __VA_ARGS__);  \
    PQ_HIP(hipGetLastError());                                                       \
  } while (0)

extern "C" {

int pyqsm_mesh_topology(const int32_t* tris, int64_t n_tris, int64_t n_verts, const double* verts, int32_t** edges,
                        int32_t** edge_count, uint8_t** edge_flags, int32_t* tri_cluster, int64_t** cluster_n,
                        double** cluster_area, uint8_t* vertex_flags, int64_t* summary, int32_t device) {
  PQ_API_RANGE("pyqsm_mesh_topology");
  if (edges) *edges = nullptr;
  if (edge_count) *edge_count = nullptr;
  if (edge_flags) *edge_flags = nullptr;
  if (cluster_n) *cluster_n = nullptr;
  if (cluster_area) *cluster_area = nullptr;
  if (n_tris < 0 || n_verts < 0) return fail(PYQSM_EINVAL, "negative size");
  if (!edges || !edge_count || !edge_flags || !cluster_n || !cluster_area || !summary ||
      (n_tris > 0 && (!tris || !tri_cluster)) || (n_verts > 0 && !vertex_flags))
    return fail(PYQSM_EINVAL, "pyqsm_mesh_topology: NULL pointer");
  if (n_tris >= kMeshMaxTris) return fail(PYQSM_ERANGE, "pyqsm_mesh_topology: 2^29 triangles or more");
  if (n_verts > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "pyqsm_mesh_topology: more than 2^31 vertices");
  for (int64_t t = 0; t < n_tris; ++t) {
    const int32_t a = tris[3 * t], b = tris[3 * t + 1], d = tris[3 * t + 2];
    if (a < 0 || b < 0 || d < 0 || a >= n_verts || b >= n_verts || d >= n_verts)
      return fail(PYQSM_EINVAL, "triangle %lld has a vertex index outside [0, %lld)", (long long)t,
                  (long long)n_verts);
    if (a == b || b == d || a == d)
      return fail(PYQSM_EINVAL, "triangle %lld repeats a vertex index (remove degenerate triangles first)",
                  (long long)t);
  }
  std::fill(summary, summary + 8, int64_t(0));
  summary[6] = 1;
  summary[7] = n_verts;
  if (n_verts > 0) std::fill(vertex_flags, vertex_flags + n_verts, uint8_t(0));
  if (n_tris == 0) return 0;  // nothing to launch

  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  const int nt = int(n_tris), nh = 3 * nt, nv = int(n_verts);
  int32_t *d_tris, *d_vals, *d_par_tri, *d_par_corner, *d_par_cover, *d_vroots, *d_cl;
  uint32_t* d_keys;
  double* d_verts = nullptr;
  unsigned long long* d_counters;
  uint8_t* d_vflags;
  PQ_TRY(c->arena.get(size_t(nh), &d_tris));
  PQ_TRY(c->arena.get(size_t(nt), &d_keys));
  PQ_TRY(c->arena.get(size_t(nt), &d_vals));
  PQ_TRY(c->arena.get(size_t(nt), &d_par_tri));
  PQ_TRY(c->arena.get(size_t(nh), &d_par_corner));
  PQ_TRY(c->arena.get(size_t(nt) * 2, &d_par_cover));
  PQ_TRY(c->arena.get(size_t(nv), &d_vroots));
  PQ_TRY(c->arena.get(size_t(nt), &d_cl));
  PQ_TRY(c->arena.get(size_t(8), &d_counters));
  PQ_TRY(c->arena.get(size_t(nv), &d_vflags));
  if (verts) PQ_TRY(c->arena.get(size_t(nv) * 3, &d_verts));
  PQ_TRY(copy_in(c, d_tris, tris, size_t(nh)));
  if (verts) PQ_TRY(copy_in(c, d_verts, verts, size_t(nv) * 3));
  PQ_HIP(hipMemsetAsync(d_counters, 0, 64, c->stream));
  PQ_HIP(hipMemsetAsync(d_vroots, 0, size_t(nv) * 4, c->stream));

  // the half-edges sorted by (min, max) and their runs (mesh_halfedge.hpp). Inside a run the
  // half-edges ascend, so its head is the lowest one.
  int32_t e_total = 0;
  int32_t *d_hs = nullptr, *d_flags = nullptr, *d_first = nullptr;
  {
    ProfScope ps(c, "mesh_edge_sort");
    PQ_TRY(mesh_half_edge_runs(c, d_tris, nt, nv, &d_hs, &d_flags, &d_first));
    PQ_TRY(fetch(c, &e_total, d_flags + nh));  // E sizes the edge table
  }
  if (e_total < 1 || e_total > nh) return fail(PYQSM_EHIP, "pyqsm_mesh_topology: %d edges counted", e_total);
  const int ne = e_total;
  int32_t *d_edges, *d_ecount;
  uint8_t* d_eflags;
  PQ_TRY(c->arena.get(size_t(ne) * 2, &d_edges));
  PQ_TRY(c->arena.get(size_t(ne), &d_ecount));
  PQ_TRY(c->arena.get(size_t(ne), &d_eflags));
  int32_t n_clusters = 0;
  {
    ProfScope ps(c, "mesh_union");
    PQ_LAUNCH(k_uf_init, ceil_div(nt, 256), nt, d_par_tri);
    PQ_LAUNCH(k_uf_init, ceil_div(nh, 256), nh, d_par_corner);
    PQ_LAUNCH(k_uf_init, ceil_div(2 * nt, 256), 2 * nt, d_par_cover);
    PQ_LAUNCH(k_mesh_edges, ceil_div(nh, 256), nh, static_cast<const int32_t*>(d_tris),
              static_cast<const int32_t*>(d_hs), static_cast<const int32_t*>(d_flags),
              static_cast<const int32_t*>(d_first), d_edges, d_ecount, d_eflags, d_par_tri, d_par_corner,
              d_par_cover, d_counters);
    PQ_LAUNCH(k_uf_flatten, ceil_div(nt, 256), nt, d_par_tri);
    PQ_LAUNCH(k_uf_flatten, ceil_div(nh, 256), nh, d_par_corner);
    PQ_LAUNCH(k_uf_flatten, ceil_div(2 * nt, 256), 2 * nt, d_par_cover);
    // d_flags is free again: the roots of the triangle sets, scanned, number the clusters
    PQ_LAUNCH(k_mesh_root_flags, ceil_div(nt + 1, 256), nt, static_cast<const int32_t*>(d_par_tri), d_flags);
    PQ_TRY(exclusive_scan_i32(c, d_flags, int64_t(nt) + 1));
    PQ_TRY(download(c, &n_clusters, d_flags + nt, 1));
    PQ_LAUNCH(k_mesh_vertex_roots, ceil_div(nh, 256), nh, static_cast<const int32_t*>(d_par_corner),
              static_cast<const int32_t*>(d_tris), d_vroots);
    PQ_LAUNCH(k_mesh_vertex_flags, ceil_div(nv, 256), nv, static_cast<const int32_t*>(d_vroots), d_vflags,
              d_counters);
    PQ_LAUNCH(k_mesh_cover_check, ceil_div(nt, 256), nt, static_cast<const int32_t*>(d_par_cover), d_counters);
    PQ_HIP(hipStreamSynchronize(c->stream));  // C sizes the cluster table
  }
  if (n_clusters < 1 || n_clusters > nt)
    return fail(PYQSM_EHIP, "pyqsm_mesh_topology: %d clusters counted", n_clusters);
  const int ncl = n_clusters;
  int32_t* d_cstart;
  int64_t* d_cn;
  double* d_carea;
  PQ_TRY(c->arena.get(size_t(ncl) + 1, &d_cstart));
  PQ_TRY(c->arena.get(size_t(ncl), &d_cn));
  PQ_TRY(c->arena.get(size_t(ncl), &d_carea));
  {
    ProfScope ps(c, "mesh_clusters");
    PQ_LAUNCH(k_mesh_tri_cluster, ceil_div(nt, 256), nt, static_cast<const int32_t*>(d_par_tri),
              static_cast<const int32_t*>(d_flags), d_cl, d_keys, d_vals);
    PQ_TRY(stable_sort_pairs_u32(c, &d_keys, &d_vals, nt, bit_length(uint64_t(ncl))));
    PQ_LAUNCH(k_mesh_cluster_start, ceil_div(nt, 256), nt, ncl, static_cast<const uint32_t*>(d_keys), d_cstart);
    PQ_LAUNCH(k_mesh_cluster_sums, ceil_div(ncl, 4), ncl, static_cast<const int32_t*>(d_cstart),
              static_cast<const int32_t*>(d_vals), static_cast<const int32_t*>(d_tris),
              static_cast<const double*>(d_verts), d_cn, d_carea);
  }
  OutBufs out;
  int32_t* h_edges = out.get<int32_t>(size_t(ne) * 2);
  int32_t* h_ecount = out.get<int32_t>(size_t(ne));
  uint8_t* h_eflags = out.get<uint8_t>(size_t(ne));
  int64_t* h_cn = out.get<int64_t>(size_t(ncl));
  double* h_carea = verts ? out.get<double>(size_t(ncl)) : nullptr;
  if (!h_edges || !h_ecount || !h_eflags || !h_cn || (verts && !h_carea))
    return fail(PYQSM_ENOMEM, "pyqsm_mesh_topology: no host memory for %d edges and %d clusters", ne, ncl);
  unsigned long long counters[8];
  PQ_TRY(download(c, h_edges, d_edges, size_t(ne) * 2));
  PQ_TRY(download(c, h_ecount, d_ecount, size_t(ne)));
  PQ_TRY(download(c, h_eflags, d_eflags, size_t(ne)));
  PQ_TRY(download(c, h_cn, d_cn, size_t(ncl)));
  if (verts) PQ_TRY(download(c, h_carea, d_carea, size_t(ncl)));
  PQ_TRY(download(c, tri_cluster, d_cl, size_t(nt)));
  PQ_TRY(download(c, vertex_flags, d_vflags, size_t(nv)));
  PQ_TRY(download(c, counters, d_counters, 8));
  PQ_HIP(hipStreamSynchronize(c->stream));
  summary[0] = ne;
  summary[1] = int64_t(counters[0]);
  summary[2] = int64_t(counters[1]);
  summary[3] = int64_t(counters[2]);
  summary[4] = int64_t(counters[3]);
  summary[5] = ncl;
  summary[6] = (counters[1] == 0 && counters[5] == 0) ? 1 : 0;
  summary[7] = int64_t(counters[4]);
  out.kept = true;
  *edges = h_edges;
  *edge_count = h_ecount;
  *edge_flags = h_eflags;
  *cluster_n = h_cn;
  *cluster_area = h_carea;
  return 0;
}

int pyqsm_mesh_self_intersections(const int32_t* ijk, int64_t n_verts, const int32_t* tris, int64_t n_tris,
                                  int32_t flags, int64_t max_tests, int64_t* n_pairs, int32_t** pairs,
                                  uint8_t* tri_hit, int64_t* stats, int32_t device) {
  PQ_API_RANGE("pyqsm_mesh_self_intersections");
  if (pairs) *pairs = nullptr;
  if (n_pairs) *n_pairs = 0;
  if (stats) std::fill(stats, stats + 6, int64_t(0));
  if (flags & ~PYQSM_MESH_PAIRS) return fail(PYQSM_EINVAL, "pyqsm_mesh_self_intersections: unknown flag");
  const bool want_pairs = (flags & PYQSM_MESH_PAIRS) != 0;
  if (n_tris < 0 || n_verts < 0) return fail(PYQSM_EINVAL, "negative size");
  if (!n_pairs || (want_pairs && !pairs) || (n_tris > 0 && (!tris || !tri_hit)) || (n_verts > 0 && !ijk))
    return fail(PYQSM_EINVAL, "pyqsm_mesh_self_intersections: NULL pointer");
  if (n_tris > kSweepMaxTris) return fail(PYQSM_ERANGE, "pyqsm_mesh_self_intersections: more than 2^26 triangles");
  if (n_verts > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "pyqsm_mesh_self_intersections: more than 2^31 vertices");
  for (int64_t k = 0; k < 3 * n_tris; ++k)
    if (tris[k] < 0 || tris[k] >= n_verts)
      return fail(PYQSM_EINVAL, "triangle %lld has a vertex index outside [0, %lld)", (long long)(k / 3),
                  (long long)n_verts);
  int32_t lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  for (int64_t v = 0; v < n_verts; ++v)
    for (int a = 0; a < 3; ++a) {
      const int32_t x = ijk[3 * v + a];
      if (v == 0 || x < lo[a]) lo[a] = x;
      if (v == 0 || x > hi[a]) hi[a] = x;
    }
  for (int a = 0; a < 3; ++a)
    if (int64_t(hi[a]) - lo[a] > kMeshMaxExtent)
      return fail(PYQSM_EINVAL, "the vertices span %lld lattice units on axis %d, more than 2^20: use a coarser quantum",
                  (long long)(int64_t(hi[a]) - lo[a]), a);
  if (max_tests <= 0) {
    if (PYQSM_MESH_DEFAULT_MAX_TESTS <= 0)
      return fail(PYQSM_EINVAL, "pyqsm_mesh_self_intersections: give max_tests: there is no default until the sweep's "
                                "rate has been measured");
    max_tests = PYQSM_MESH_DEFAULT_MAX_TESTS;
  }
  const int64_t considered = n_tris * (n_tris - 1) / 2;  // T <= 2^26: below 2^51
  if (considered > max_tests)
    return fail(PYQSM_ERANGE,
                "pyqsm_mesh_self_intersections: %lld triangle pairs exceed max_tests = %lld (split the mesh or raise "
                "max_tests)",
                (long long)considered, (long long)max_tests);
  if (n_tris > 0) std::fill(tri_hit, tri_hit + n_tris, uint8_t(0));
  if (stats) stats[0] = considered;
  if (n_tris == 0) return 0;

  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  const int nt = int(n_tris), nv = int(n_verts), ntile = ceil_div(nt, kRows), nword = ceil_div(nt, 4);
  int32_t *d_ijk, *d_tris;
  int4 *d_box, *d_tv;
  uint32_t* d_hit;
  unsigned long long* d_counters;
  PQ_TRY(c->arena.get(size_t(nv) * 3, &d_ijk));
  PQ_TRY(c->arena.get(size_t(nt) * 3, &d_tris));
  PQ_TRY(c->arena.get(size_t(nt) * 2, &d_box));
  PQ_TRY(c->arena.get(size_t(nt) * 3, &d_tv));
  PQ_TRY(c->arena.get(size_t(nword), &d_hit));
  PQ_TRY(c->arena.get(size_t(8), &d_counters));
  PQ_TRY(copy_in(c, d_ijk, ijk, size_t(nv) * 3));
  PQ_TRY(copy_in(c, d_tris, tris, size_t(nt) * 3));
  PQ_HIP(hipMemsetAsync(d_hit, 0, size_t(nword) * 4, c->stream));
  PQ_HIP(hipMemsetAsync(d_counters, 0, 64, c->stream));
  PQ_LAUNCH(k_mesh_tri_setup, ceil_div(nt, 256), nt, static_cast<const int32_t*>(d_ijk),
            static_cast<const int32_t*>(d_tris), lo[0], lo[1], lo[2], d_box, d_tv, d_counters);

  // The pair list is never truncated: a sweep whose list does not fit is run again with room for
  // the count it found (at most once: the count does not depend on the capacity).
  const dim3 grid(unsigned(ntile), unsigned(ceil_div(ntile, kColTiles)));
  unsigned long long counters[8];
  int64_t cap = want_pairs ? std::max<int64_t>(4 * int64_t(nt), 4096) : 0;
  int32_t *d_pi = nullptr, *d_pj = nullptr;
  const Arena::Mark mark = c->arena.mark();
  for (int pass = 0; pass < 2; ++pass) {
    // timed apart, so that "mesh_sweep" is always one whole sweep (the inline narrow phase included)
    ProfScope ps(c, pass == 0 ? "mesh_sweep" : "mesh_sweep_rerun");
    if (cap > 0) {
      PQ_TRY(c->arena.get(size_t(cap), &d_pi));
      PQ_TRY(c->arena.get(size_t(cap), &d_pj));
    }
    hipLaunchKernelGGL(k_mesh_sweep, grid, dim3(256), 0, c->stream, nt, ntile, static_cast<const int4*>(d_box),
                       static_cast<const int4*>(d_tv), d_hit, d_counters, (long long)cap, d_pi, d_pj);
    PQ_HIP(hipGetLastError());
    PQ_TRY(fetch(c, counters, d_counters, 8));
    if (!want_pairs || int64_t(counters[4]) <= cap) break;
    if (pass == 1) return fail(PYQSM_EHIP, "pyqsm_mesh_self_intersections: the pair count changed between sweeps");
    if (counters[4] > 0x7FFFFF00ULL)
      return fail(PYQSM_ERANGE, "pyqsm_mesh_self_intersections: more than 2^31 intersecting pairs");
    cap = int64_t(counters[4]);
    c->arena.rewind(mark);
    PQ_HIP(hipMemsetAsync(d_counters, 0, 24, c->stream));         // the sweep's three counters
    PQ_HIP(hipMemsetAsync(d_counters + 4, 0, 8, c->stream));      // and the cursor; not the degenerate count
  }
  const int64_t found = int64_t(counters[4]);
  if (stats) {
    stats[1] = int64_t(counters[0]);
    stats[2] = int64_t(counters[1]);
    stats[3] = int64_t(counters[3]);
    stats[4] = int64_t(counters[2]);
    stats[5] = found;
  }
  PQ_TRY(fetch(c, tri_hit, reinterpret_cast<const uint8_t*>(d_hit), size_t(nt)));  // one byte per triangle
  *n_pairs = found;
  if (!want_pairs || found == 0) return 0;
  if (found > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "pyqsm_mesh_self_intersections: more than 2^31 intersecting pairs");

  // ascending (i, j): a stable pass by j, then one by i; the pairs are unique, so the list is the
  // same whatever order the cursor handed the slots out in
  const int np = int(found), bits = bit_length(uint64_t(nt));
  int32_t* d_rows;
  PQ_TRY(c->arena.get(size_t(np) * 2, &d_rows));
  {
    ProfScope ps(c, "mesh_pair_sort");
    int32_t* perm = nullptr;
    PQ_TRY(refine_order_by_key(c, np, d_pj, &perm, bits));
    PQ_TRY(refine_order_by_key(c, np, d_pi, &perm, bits));
    PQ_LAUNCH(k_mesh_pair_rows, ceil_div(np, 256), np, static_cast<const int32_t*>(perm),
              static_cast<const int32_t*>(d_pi), static_cast<const int32_t*>(d_pj), d_rows);
  }
  OutBufs out;
  int32_t* rows = out.get<int32_t>(size_t(np) * 2);
  if (!rows) return fail(PYQSM_ENOMEM, "pyqsm_mesh_self_intersections: no host memory for %d pairs", np);
  PQ_TRY(fetch(c, rows, d_rows, size_t(np) * 2));
  out.kept = true;
  *pairs = rows;
  return 0;
}

}  // extern "C"
