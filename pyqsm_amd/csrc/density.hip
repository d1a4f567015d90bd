// density.hip — the radius graph of a cloud on gfx950: an edge joins two points within `radius`.
//
//   pyqsm_radius_degrees     the degree of every point at up to 8 radii in one pass: the local density
//                            pyQSM takes from a Python loop over KDTree.query_pairs(r)
//                            (utils/lib_integration.py:48-71, scripts/graph_based_leaf_id.py:28-38),
//                            in O(n) memory, no pair stored.
//   pyqsm_radius_pairs       the pair list itself, i < j, ascending by (i, j).
//   pyqsm_radius_components  the connected components at up to 8 radii, ranked by (size descending, smallest
//                            member ascending): what pyQSM takes from rustworkx over the pair list
//                            (scripts/graph_based_leaf_id.py:80-97, qsm_generation.py:526-556). No pair is
//                            stored: the cell-run kernel joins the two ends of every edge in a union-find
//                            (unionfind.hpp), and the ranking is a histogram, a compaction and a stable sort.
// One rule: {i, j}, i != j, is an edge when d2 = ((dx*dx) + dy*dy) + dz*dz <= radius * radius, fp64,
// no contraction, inclusive; coincident points are joined (cKDTree's rule at p = 2, and
// pyqsm_cluster_adjacency's).
//
// The kernel is cell-wise (k_cell_runs). The cloud is binned into cells of the (largest) radius
// (grid.hpp: radius_grid). A block owns a RUN of query points of one cell: 64 consecutive sorted
// positions on one wave for cells of at most kLightMax points, 256 on four waves for the others. It
// stages the nine x-runs of the cell's 27-cell stencil through LDS in tiles of four candidates per
// thread, as fp64 whatever the grid's storage form, and every lane tests its own point against the
// tile: each LDS read is a broadcast, each candidate is fetched from L2 once per run instead of once
// per lane. A lane keeps its point's counters in registers and writes them once, through the grid's
// `order`: no atomics for the degrees. Points the robust box gave up sit in its outermost cells
// (clamped_cell), with the test on their true coordinates, as in the other radius kernels.
// Atomics: one 64-bit integer atomicAdd per block and radius for the sum of the degrees, two for the
// statistics. Integer sums: the same bits whatever the arrival order. The union mode hooks roots with
// 32-bit atomicMin: a finished set's root is its smallest member whatever the order of the unions, and
// the components' sizes are integer atomicAdds.
#include "unionfind.hpp"
#include "grid.hpp"

#include <algorithm>
#include <cmath>
#include <type_traits>

namespace pyqsm {

static constexpr int kDegMaxRadii = 8;
static constexpr int kLightMax = 128;  // cells of at most this many points are served 64 points per block
static constexpr int kTilePerThread = 4;  // a tile holds 4 candidates per thread: 256 (light), 1024 (heavy)

struct DegBounds {
  double r2[kDegMaxRadii];
};

// flags [2][n + 1] for the scans: the sorted positions that begin a light run, and a heavy run
__global__ __launch_bounds__(256) void k_run_flags(int n, const int32_t* __restrict__ start,
                                                   const int32_t* __restrict__ cell_of, int32_t* __restrict__ light,
                                                   int32_t* __restrict__ heavy) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q > n) return;
  int fl = 0, fh = 0;
  if (q < n) {
    const int c = cell_of[q];
    const int b = start[c], cnt = start[c + 1] - b;
    if (cnt <= kLightMax) fl = ((q - b) & 63) == 0;
    else fh = ((q - b) & 255) == 0;
  }
  light[q] = fl;
  heavy[q] = fh;
}

// the run lists, in ascending sorted position (pos = the scanned flags)
__global__ __launch_bounds__(256) void k_run_lists(int n, const int32_t* __restrict__ pos_l,
                                                   const int32_t* __restrict__ pos_h, int32_t* __restrict__ runs_l,
                                                   int32_t* __restrict__ runs_h) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  const int a = pos_l[q], b = pos_h[q];
  if (pos_l[q + 1] != a) runs_l[a] = q;
  if (pos_h[q + 1] != b) runs_h[b] = q;
}

template <int T, bool IDS>
struct alignas(16) RunTile {
  double x[T], y[T], z[T];
  int32_t id[IDS ? T : 4];  // original indices of the candidates (the pair and union modes)
};
template <int T>
struct alignas(16) UnionTile : RunTile<T, true> {
  int32_t par[T];  // the candidates' parents when the tile was staged (the union mode)
};

// The root of x; x's entry is lowered to it when the walk was longer than one step. An atomicMin of an
// ancestor keeps parent[x] <= x and x in its set, and loses no hook that arrives meanwhile.
__device__ __forceinline__ int32_t uf_find_compress(int32_t* parent, int32_t x) {
  const int32_t p = uf_load(parent, x);
  if (p == x) return x;
  const int32_t r = uf_find(parent, p);
  if (r != p) atomicMin(&parent[x], r);
  return r;
}

// Joins the sets of a and b and returns a member of the joined set for a's snapshot: the root when the
// two were one set already (the common case once a component has formed: two walks, no atomic unless a
// walk was long), else the smaller root, below which a and b are then hung as well, so that the blocks
// that stage them next see it. Both are below a and b and in their set.
__device__ __forceinline__ int32_t uf_join(int32_t* parent, int32_t a, int32_t b) {
  const int32_t ra = uf_find_compress(parent, a), rb = uf_find_compress(parent, b);
  if (ra == rb) return ra;
  uf_union(parent, ra, rb);
  const int32_t lo = ra < rb ? ra : rb;
  atomicMin(&parent[a], lo);
  atomicMin(&parent[b], lo);
  return lo;
}

// Before the union pass: every run (the block's points of one cell, as in k_cell_runs) is tied into a few
// sets. kLinkRounds times the first point not yet tied becomes the pivot, and every other such point
// within the radius of it (the contract's own test) joins it. After a flatten, the points of such a set
// carry one parent, and the union pass meets them one after the other in a tile.
static constexpr int kLinkRounds = 4;
template <class CO, int BT>
__global__ __launch_bounds__(BT) void k_run_links(const int32_t* __restrict__ runs, const int32_t* __restrict__ start,
                                                  const int32_t* __restrict__ cell_of,
                                                  const int32_t* __restrict__ order, CO co, double r2,
                                                  int32_t* __restrict__ parent) {
  __shared__ double piv[3];
  __shared__ int piv_id, lead;
  const int q0 = __builtin_amdgcn_readfirstlane(runs[blockIdx.x]);
  const int c = __builtin_amdgcn_readfirstlane(cell_of[q0]);
  const int cell_end = __builtin_amdgcn_readfirstlane(start[c + 1]);
  const int run_end = q0 + BT < cell_end ? q0 + BT : cell_end;
  const int p = q0 + int(threadIdx.x);
  bool tied = p >= run_end;
  double x = 0.0, y = 0.0, z = 0.0;
  int me = -1;
  if (!tied) {
    co.get(p, x, y, z);
    me = order[p];
  }
  for (int round = 0; round < kLinkRounds; ++round) {
    if (threadIdx.x == 0) lead = BT;
    __syncthreads();
    if (!tied) atomicMin(&lead, int(threadIdx.x));
    __syncthreads();
    const int l = lead;
    if (l == BT) return;  // block-uniform
    if (int(threadIdx.x) == l) {
      piv[0] = x;
      piv[1] = y;
      piv[2] = z;
      piv_id = me;
      tied = true;
    }
    __syncthreads();
    if (!tied && sqdist3(x, y, z, piv[0], piv[1], piv[2]) <= r2) {
      uf_union(parent, me, piv_id);
      tied = true;
    }
    __syncthreads();  // piv and lead are read before the next round writes them
  }
}

// MODE 0: out[k * n + i] = degree of point i at r2[k] (R radii; the point itself not counted).
// MODE 1: out[i] = number of j > i within r2[0]: the length of row i of the pair list.
// MODE 2: row i of the pair list: pi[s] = i, pj[s] = j for s from row_off[i], in the order the
//         candidates are met (the caller sorts); cap: the length of pi / pj.
// MODE 3: out is the union-find's parent [n] (k_uf_init before, k_uf_flatten after both launches): every
//         edge {me, j}, j < me, within r2[0] joins the two sets. A candidate whose parent, read when the
//         tile was staged, equals the lane's own snapshot, or the staged parent of the candidate the lane
//         joined last, is in the lane's set already and is skipped without touching memory: two entries
//         that point at one node belong to one set, and sets only grow.
// sums [R]: += the block's sum of what MODE 0 / 1 count. stats (may be null): [0] += distance tests
// of live lanes, [1] += candidates staged.
template <class CO, int BT, int R, int MODE>
__global__ __launch_bounds__(BT) void k_cell_runs(const int32_t* __restrict__ runs, const int32_t* __restrict__ start,
                                                  const int32_t* __restrict__ cell_of,
                                                  const int32_t* __restrict__ order, int nx, int nxy, int ncell,
                                                  CO co, DegBounds th, int n, int cap, int32_t* __restrict__ out,
                                                  const int32_t* __restrict__ row_off, int32_t* __restrict__ pi,
                                                  int32_t* __restrict__ pj, unsigned long long* __restrict__ sums,
                                                  unsigned long long* __restrict__ stats) {
  constexpr int T = BT * kTilePerThread;
  __shared__ std::conditional_t<MODE == 3, UnionTile<T>, RunTile<T, MODE != 0>> L;
  __shared__ unsigned long long wsum[R][BT / 64];
  const int q0 = __builtin_amdgcn_readfirstlane(runs[blockIdx.x]);
  const int c = __builtin_amdgcn_readfirstlane(cell_of[q0]);
  const int cell_end = __builtin_amdgcn_readfirstlane(start[c + 1]);
  const int run_end = q0 + BT < cell_end ? q0 + BT : cell_end;
  const int p = q0 + int(threadIdx.x);
  const bool live = p < run_end;
  double x = 0.0, y = 0.0, z = 0.0;
  int me = -1;
  if (live) {
    co.get(p, x, y, z);
    me = order[p];
  }
  int cnt[R];
#pragma unroll
  for (int k = 0; k < R; ++k) cnt[k] = 0;
  int cur = 0;
  if (MODE == 2 && live) cur = row_off[me];
  // MODE 3: two members of me's set: me's parent when last read, and the staged parent of the candidate
  // joined last (a set that k_run_links tied lies in one stretch of a tile and carries one parent)
  int mine = -1, seen = -1;
  if (MODE == 3 && live) mine = uf_load(out, me);
  long long staged = 0;
  // c is an interior cell (clamped_cell: 1 .. n - 2 on every axis), so the nine rows lie inside the grid
  // and row - 1, row + 2 inside the directory of ncell + 1 entries; the clamps cost two scalar instructions
  for (int w = 0; w < 9; ++w) {
    const int row = c + (w % 3 - 1) * nx + (w / 3 - 1) * nxy;
    const int qb = __builtin_amdgcn_readfirstlane(start[row - 1 < 0 ? 0 : row - 1]);
    const int qe = __builtin_amdgcn_readfirstlane(start[row + 2 > ncell ? ncell : row + 2]);
    for (int base = qb; base < qe; base += T) {
      const int m = qe - base < T ? qe - base : T;
      for (int t = threadIdx.x; t < m; t += BT) {
        co.get(base + t, L.x[t], L.y[t], L.z[t]);
        if (MODE != 0) L.id[t] = order[base + t];
        if constexpr (MODE == 3) L.par[t] = uf_load(out, L.id[t]);
      }
      // an odd count is made even by a candidate at infinity: d2 = +inf, never within a bound
      if ((m & 1) && threadIdx.x == 0) {
        L.x[m] = __builtin_inf();
        L.y[m] = 0.0;
        L.z[m] = 0.0;
        if (MODE != 0) L.id[m] = 0;
        if constexpr (MODE == 3) L.par[m] = 0;
      }
      __syncthreads();
      // two candidates a step, each coordinate pair one 16-byte LDS read at a wave-uniform address
#pragma unroll 2
      for (int j = 0; j < m; j += 2) {
        const double2 cx = *reinterpret_cast<const double2*>(&L.x[j]);
        const double2 cy = *reinterpret_cast<const double2*>(&L.y[j]);
        const double2 cz = *reinterpret_cast<const double2*>(&L.z[j]);
        const double d0 = sqdist3(x, y, z, cx.x, cy.x, cz.x);
        const double d1 = sqdist3(x, y, z, cx.y, cy.y, cz.y);
        if constexpr (MODE == 0) {
#pragma unroll
          for (int k = 0; k < R; ++k) cnt[k] += int(d0 <= th.r2[k]) + int(d1 <= th.r2[k]);
        } else if constexpr (MODE == 3) {
          // me = -1 on a lane without a point: no j is below it
          const int j0 = L.id[j], j1 = L.id[j + 1];
          const int p0 = L.par[j], p1 = L.par[j + 1];
          if (d0 <= th.r2[0] && j0 < me && p0 != mine && p0 != seen) {
            mine = uf_join(out, me, j0);
            seen = p0;
          }
          if (d1 <= th.r2[0] && j1 < me && p1 != mine && p1 != seen) {
            mine = uf_join(out, me, j1);
            seen = p1;
          }
        } else {
          const int j0 = L.id[j], j1 = L.id[j + 1];
          const bool t0 = d0 <= th.r2[0] && j0 > me, t1 = d1 <= th.r2[0] && j1 > me;
          if (MODE == 1) cnt[0] += int(t0) + int(t1);
          if (MODE == 2 && live) {
            if (t0 && cur < cap) {
              pi[cur] = me;
              pj[cur++] = j0;
            }
            if (t1 && cur < cap) {
              pi[cur] = me;
              pj[cur++] = j1;
            }
          }
        }
      }
      __syncthreads();
      staged += m;
    }
  }
  if (MODE >= 2) return;
  // the point itself is among the candidates exactly once, at d2 = 0 (MODE 1 left it out: j > i)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int v = live ? cnt[k] - (MODE == 0 ? 1 : 0) : 0;
    if (live) out[size_t(k) * size_t(n) + size_t(me)] = v;
    unsigned long long s = (unsigned long long)v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) wsum[k][wv] = s;
  }
  __syncthreads();
  if (threadIdx.x < R) {
    unsigned long long s = 0;
#pragma unroll
    for (int q = 0; q < BT / 64; ++q) s += wsum[threadIdx.x][q];
    if (s) atomicAdd(&sums[threadIdx.x], s);
  }
  if (stats && threadIdx.x == 0) {
    atomicAdd(&stats[0], (unsigned long long)(staged * (long long)(run_end - q0)));
    atomicAdd(&stats[1], (unsigned long long)staged);
  }
}

// The runs of the grid's cells: *runs_l / *runs_h the first sorted positions of the light and heavy
// runs, *n_l / *n_h how many (read back: synchronises).
struct CellRuns {
  int32_t *light, *heavy;
  int n_light, n_heavy;
};
static int cell_runs(Ctx* c, const DevGrid& g, int64_t n, CellRuns* cr) {
  int32_t *fl, *fh;
  PQ_TRY(c->arena.get(size_t(n) + 1, &fl));
  PQ_TRY(c->arena.get(size_t(n) + 1, &fh));
  PQ_TRY(c->arena.get(size_t(n), &cr->light));
  PQ_TRY(c->arena.get(size_t(n), &cr->heavy));
  hipLaunchKernelGGL(k_run_flags, dim3(ceil_div(n + 1, 256)), dim3(256), 0, c->stream, int(n),
                     static_cast<const int32_t*>(g.start), static_cast<const int32_t*>(g.cell_of), fl, fh);
  PQ_HIP(hipGetLastError());
  PQ_TRY(exclusive_scan_i32(c, fl, n + 1));
  PQ_TRY(exclusive_scan_i32(c, fh, n + 1));
  hipLaunchKernelGGL(k_run_lists, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, int(n),
                     static_cast<const int32_t*>(fl), static_cast<const int32_t*>(fh), cr->light, cr->heavy);
  PQ_HIP(hipGetLastError());
  int32_t h[2] = {0, 0};
  PQ_TRY(download(c, &h[0], fl + n, 1));
  PQ_TRY(download(c, &h[1], fh + n, 1));
  PQ_TRY(stream_sync(c));
  cr->n_light = h[0];
  cr->n_heavy = h[1];
  return 0;
}

// One pass of k_cell_runs over both run lists, for the storage form the grid holds.
template <int R, int MODE>
static int launch_runs(Ctx* c, const DevGrid& g, const CellRuns& cr, const DegBounds& th, int64_t n, int cap, int32_t* out,
                       const int32_t* row_off, int32_t* pi, int32_t* pj, unsigned long long* sums,
                       unsigned long long* stats) {
  const int nx = g.nx, nxy = g.nx * g.ny;
  on_coords(g, [&](auto co) {
    using CO = decltype(co);
    if (cr.n_light)
      hipLaunchKernelGGL((k_cell_runs<CO, 64, R, MODE>), dim3(unsigned(cr.n_light)), dim3(64), 0, c->stream,
                         static_cast<const int32_t*>(cr.light), static_cast<const int32_t*>(g.start),
                         static_cast<const int32_t*>(g.cell_of), static_cast<const int32_t*>(g.order), nx, nxy, int(g.ncell), co,
                         th, int(n), cap, out, row_off, pi, pj, sums, stats);
    if (cr.n_heavy)
      hipLaunchKernelGGL((k_cell_runs<CO, 256, R, MODE>), dim3(unsigned(cr.n_heavy)), dim3(256), 0, c->stream,
                         static_cast<const int32_t*>(cr.heavy), static_cast<const int32_t*>(g.start),
                         static_cast<const int32_t*>(g.cell_of), static_cast<const int32_t*>(g.order), nx, nxy, int(g.ncell), co,
                         th, int(n), cap, out, row_off, pi, pj, sums, stats);
  });
  PQ_HIP(hipGetLastError());
  return 0;
}

// k_run_links over both run lists
static int launch_links(Ctx* c, const DevGrid& g, const CellRuns& cr, double r2, int32_t* parent) {
  on_coords(g, [&](auto co) {
    using CO = decltype(co);
    if (cr.n_light)
      hipLaunchKernelGGL((k_run_links<CO, 64>), dim3(unsigned(cr.n_light)), dim3(64), 0, c->stream,
                         static_cast<const int32_t*>(cr.light), static_cast<const int32_t*>(g.start),
                         static_cast<const int32_t*>(g.cell_of), static_cast<const int32_t*>(g.order), co, r2, parent);
    if (cr.n_heavy)
      hipLaunchKernelGGL((k_run_links<CO, 256>), dim3(unsigned(cr.n_heavy)), dim3(256), 0, c->stream,
                         static_cast<const int32_t*>(cr.heavy), static_cast<const int32_t*>(g.start),
                         static_cast<const int32_t*>(g.cell_of), static_cast<const int32_t*>(g.order), co, r2, parent);
  });
  PQ_HIP(hipGetLastError());
  return 0;
}

template <int R>
static int launch_degrees(Ctx* c, int32_t want, const DevGrid& g, const CellRuns& cr, const DegBounds& th, int64_t n,
                          int32_t* out, unsigned long long* sums, unsigned long long* stats) {
  if constexpr (R > kDegMaxRadii) {
    return fail(PYQSM_ERANGE, "more than %d radii", kDegMaxRadii);
  } else {
    if (want == R) return launch_runs<R, 0>(c, g, cr, th, n, 0, out, nullptr, nullptr, nullptr, sums, stats);
    return launch_degrees<R + 1>(c, want, g, cr, th, n, out, sums, stats);
  }
}

// PYQSM_EINVAL unless every coordinate is finite
static int finite_cloud(const double* xyz, int64_t n) {
  for (int64_t i = 0; i < 3 * n; ++i)
    if (!std::isfinite(xyz[i])) return fail(PYQSM_EINVAL, "point coordinates must be finite");
  return 0;
}

// interleaves the sorted pair list: rows[2 s] = pi[perm[s]], rows[2 s + 1] = pj[perm[s]]
__global__ __launch_bounds__(256) void k_pair_rows(int np, const int32_t* __restrict__ perm,
                                                   const int32_t* __restrict__ pi, const int32_t* __restrict__ pj,
                                                   int32_t* __restrict__ rows) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= np) return;
  const int q = perm[s];
  rows[2 * size_t(s)] = pi[q];
  rows[2 * size_t(s) + 1] = pj[q];
}

// ---- the components' ranking, from the flattened parent (parent[i] = the smallest member of i's set) ----

// size[root] = the members of root's set, flags [n + 1] = 1 at the roots (flags[n] = 0). A wave adds its
// lanes of one root with one atomicAdd: a component of most of the cloud would otherwise be n atomics on
// one address. Integer sums, the same bits in any order.
__global__ __launch_bounds__(256) void k_comp_sizes(int n, const int32_t* __restrict__ parent,
                                                    int32_t* __restrict__ size, int32_t* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  if (i == n) {
    flags[n] = 0;
    return;
  }
  const int root = parent[i];
  flags[i] = root == i;
  for (;;) {  // the lanes that are still here: those of the first one's root leave together
    const int r0 = __builtin_amdgcn_readfirstlane(root);
    const unsigned long long peers = __ballot(root == r0);
    if (root == r0) {
      if ((__lane_id() & 63u) == unsigned(__ffsll((long long)peers) - 1)) atomicAdd(&size[r0], __popcll(peers));
      break;
    }
  }
}

// key[s] = n - size of the s-th root (roots ascending): ascending keys are descending sizes
__global__ __launch_bounds__(256) void k_comp_keys(int nc, int n, const int64_t* __restrict__ roots,
                                                   const int32_t* __restrict__ size, int32_t* __restrict__ key) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s < nc) key[s] = n - size[roots[s]];
}

// rank s belongs to the perm[s]-th root: rank_of[root] = s, sizes[s] = its size
__global__ __launch_bounds__(256) void k_comp_ranks(int nc, const int32_t* __restrict__ perm,
                                                    const int64_t* __restrict__ roots,
                                                    const int32_t* __restrict__ size, int32_t* __restrict__ rank_of,
                                                    int32_t* __restrict__ sizes) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= nc) return;
  const int root = int(roots[perm[s]]);
  rank_of[root] = s;
  sizes[s] = size[root];
}

__global__ __launch_bounds__(256) void k_comp_labels(int n, const int32_t* __restrict__ parent,
                                                     const int32_t* __restrict__ rank_of,
                                                     int32_t* __restrict__ component) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) component[i] = rank_of[parent[i]];
}

// The components at one radius, into the caller's rows: one union pass over the runs, then the ranking.
// Every temporary is the call's own and is released again (rewind) for the next radius.
static int components_at(Ctx* c, const DevGrid& g, const CellRuns& cr, double radius, int64_t n, int32_t* component,
                         int32_t* sizes, int32_t* members, int64_t* n_components) {
  const Arena::Mark mark = c->arena.mark();
  const int nb = ceil_div(n, 256);
  int32_t *parent, *size, *flags, *key, *rank_of, *d_sizes, *d_comp;
  int64_t* roots;
  PQ_TRY(c->arena.get(size_t(n), &parent));
  PQ_TRY(c->arena.get(size_t(n), &size));
  PQ_TRY(c->arena.get(size_t(n) + 1, &flags));
  PQ_TRY(c->arena.get(size_t(n), &roots));
  DegBounds th;
  for (int k = 0; k < kDegMaxRadii; ++k) th.r2[k] = radius * radius;
  {
    ProfScope ps(c, "radius_components_union");
    hipLaunchKernelGGL(k_uf_init, dim3(nb), dim3(256), 0, c->stream, int(n), parent);
    PQ_HIP(hipGetLastError());
    PQ_TRY(launch_links(c, g, cr, radius * radius, parent));
    hipLaunchKernelGGL(k_uf_flatten, dim3(nb), dim3(256), 0, c->stream, int(n), parent);
    PQ_HIP(hipGetLastError());
    PQ_TRY((launch_runs<1, 3>(c, g, cr, th, n, 0, parent, nullptr, nullptr, nullptr, nullptr, nullptr)));
    hipLaunchKernelGGL(k_uf_flatten, dim3(nb), dim3(256), 0, c->stream, int(n), parent);
    PQ_HIP(hipGetLastError());
  }
  {
    ProfScope ps(c, "radius_components_rank");
    PQ_HIP(hipMemsetAsync(size, 0, size_t(n) * 4, c->stream));
    hipLaunchKernelGGL(k_comp_sizes, dim3(ceil_div(n + 1, 256)), dim3(256), 0, c->stream, int(n),
                       static_cast<const int32_t*>(parent), size, flags);
    PQ_HIP(hipGetLastError());
    PQ_TRY(compact_flagged(c, flags, n, roots));
  }
  int32_t nc = 0;  // read back: it sizes the sort of the roots
  PQ_TRY(fetch(c, &nc, flags + n));
  if (nc < 1 || nc > n) return fail(PYQSM_EHIP, "pyqsm_radius_components: %d components of %lld points", nc, (long long)n);
  PQ_TRY(c->arena.get(size_t(nc), &key));
  PQ_TRY(c->arena.get(size_t(n), &rank_of));
  PQ_TRY(c->arena.get(size_t(nc), &d_sizes));
  PQ_TRY(c->arena.get(size_t(n), &d_comp));
  int32_t* by_comp = nullptr;
  {
    ProfScope ps(c, "radius_components_rank");  // the same timer: the read-back's gap is left out
    hipLaunchKernelGGL(k_comp_keys, dim3(ceil_div(nc, 256)), dim3(256), 0, c->stream, nc, int(n),
                       static_cast<const int64_t*>(roots), static_cast<const int32_t*>(size), key);
    PQ_HIP(hipGetLastError());
    // stable: equal sizes stay in ascending root order, which is ascending smallest member
    int32_t* perm = nullptr;
    PQ_TRY(refine_order_by_key(c, nc, key, &perm, bit_length(uint64_t(n))));
    hipLaunchKernelGGL(k_comp_ranks, dim3(ceil_div(nc, 256)), dim3(256), 0, c->stream, nc,
                       static_cast<const int32_t*>(perm), static_cast<const int64_t*>(roots),
                       static_cast<const int32_t*>(size), rank_of, d_sizes);
    PQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_comp_labels, dim3(nb), dim3(256), 0, c->stream, int(n),
                       static_cast<const int32_t*>(parent), static_cast<const int32_t*>(rank_of), d_comp);
    PQ_HIP(hipGetLastError());
    // (component, index) ascending: the identity refined by one stable pass on the component
    if (members) PQ_TRY(refine_order_by_key(c, n, d_comp, &by_comp, bit_length(uint64_t(nc - 1))));
  }
  PQ_TRY(download(c, component, d_comp, size_t(n)));
  PQ_TRY(download(c, sizes, d_sizes, size_t(nc)));
  if (members) PQ_TRY(download(c, members, by_comp, size_t(n)));
  PQ_TRY(stream_sync(c));
  *n_components = nc;
  c->arena.rewind(mark);
  return 0;
}

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_radius_degrees(const double* xyz, int64_t n, const double* radii, int32_t R, int32_t* degree,
                         int64_t* n_pairs, int64_t* stats, int32_t device) {
  PQ_API_RANGE("pyqsm_radius_degrees");
  if (n < 0) return fail(PYQSM_EINVAL, "negative size");
  if (!radii || !n_pairs || (n > 0 && (!xyz || !degree))) return fail(PYQSM_EINVAL, "pyqsm_radius_degrees: NULL pointer");
  if (R < 1 || R > kDegMaxRadii) return fail(PYQSM_ERANGE, "pyqsm_radius_degrees: %d radii, 1 to %d per call", R, kDegMaxRadii);
  double rmax = 0.0;
  DegBounds th;
  for (int k = 0; k < kDegMaxRadii; ++k) th.r2[k] = -1.0;
  for (int k = 0; k < R; ++k) {
    if (!(radii[k] > 0) || !std::isfinite(radii[k])) return fail(PYQSM_EINVAL, "radius must be positive and finite");
    th.r2[k] = radii[k] * radii[k];
    rmax = std::max(rmax, radii[k]);
  }
  if (n > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 points per call");
  for (int k = 0; k < R; ++k) n_pairs[k] = 0;
  if (stats) stats[0] = stats[1] = 0;
  if (n == 0) return 0;
  PQ_TRY(finite_cloud(xyz, n));
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double* d_xyz;
  int32_t* d_deg;
  unsigned long long* d_sums;  // [R] sums of the degrees, then [2] the statistics
  PQ_TRY(upload(c, xyz, size_t(n) * 3, &d_xyz));
  PQ_TRY(c->arena.get(size_t(R) * size_t(n), &d_deg));
  PQ_TRY(c->arena.get(size_t(kDegMaxRadii) + 2, &d_sums));
  PQ_HIP(hipMemsetAsync(d_sums, 0, (size_t(kDegMaxRadii) + 2) * 8, c->stream));
  DevGrid g;
  PQ_TRY(radius_grid(c, d_xyz, n, rmax, &g));
  CellRuns cr;
  PQ_TRY(cell_runs(c, g, n, &cr));
  {
    ProfScope ps(c, "radius_degrees");
    PQ_TRY(launch_degrees<1>(c, R, g, cr, th, n, d_deg, d_sums, stats ? d_sums + kDegMaxRadii : nullptr));
  }
  unsigned long long h_sums[kDegMaxRadii + 2];
  PQ_TRY(download(c, degree, d_deg, size_t(R) * size_t(n)));
  PQ_TRY(fetch(c, h_sums, d_sums, size_t(kDegMaxRadii) + 2));
  for (int k = 0; k < R; ++k) n_pairs[k] = int64_t(h_sums[k] / 2);
  if (stats) {
    stats[0] = int64_t(h_sums[kDegMaxRadii]);
    stats[1] = int64_t(h_sums[kDegMaxRadii + 1]);
  }
  return 0;
}

int pyqsm_radius_pairs(const double* xyz, int64_t n, double radius, int64_t capacity, int32_t* pairs, int64_t* count,
                       int32_t device) {
  PQ_API_RANGE("pyqsm_radius_pairs");
  if (n < 0 || capacity < 0) return fail(PYQSM_EINVAL, "negative size");
  if (!count || (n > 0 && !xyz) || (capacity > 0 && !pairs)) return fail(PYQSM_EINVAL, "pyqsm_radius_pairs: NULL pointer");
  *count = 0;
  if (!(radius > 0) || !std::isfinite(radius)) return fail(PYQSM_EINVAL, "radius must be positive and finite");
  if (n > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 points per call");
  if (n == 0) return 0;
  PQ_TRY(finite_cloud(xyz, n));
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double* d_xyz;
  int32_t* d_len;  // [n + 1] the rows' lengths, scanned into their offsets
  unsigned long long* d_sum;
  PQ_TRY(upload(c, xyz, size_t(n) * 3, &d_xyz));
  PQ_TRY(c->arena.get(size_t(n) + 1, &d_len));
  PQ_TRY(c->arena.get(1, &d_sum));
  PQ_HIP(hipMemsetAsync(d_sum, 0, 8, c->stream));
  PQ_HIP(hipMemsetAsync(d_len + n, 0, 4, c->stream));
  DevGrid g;
  PQ_TRY(radius_grid(c, d_xyz, n, radius, &g));
  CellRuns cr;
  PQ_TRY(cell_runs(c, g, n, &cr));
  DegBounds th;
  for (int k = 0; k < kDegMaxRadii; ++k) th.r2[k] = radius * radius;
  ProfScope ps(c, "radius_pairs");
  PQ_TRY((launch_runs<1, 1>(c, g, cr, th, n, 0, d_len, nullptr, nullptr, nullptr, d_sum, nullptr)));
  unsigned long long total = 0;
  PQ_TRY(fetch(c, &total, d_sum));
  *count = int64_t(total);
  if (total == 0 || capacity == 0) return 0;
  if (total > 0x7FFFFF00ULL) return fail(PYQSM_ERANGE, "pyqsm_radius_pairs: more than 2^31 pairs");
  const int np = int(total);
  int32_t *d_pi, *d_pj, *d_rows;
  PQ_TRY(c->arena.get(size_t(np), &d_pi));
  PQ_TRY(c->arena.get(size_t(np), &d_pj));
  PQ_TRY(exclusive_scan_i32(c, d_len, n + 1));
  PQ_TRY((launch_runs<1, 2>(c, g, cr, th, n, np, nullptr, d_len, d_pi, d_pj, nullptr, nullptr)));
  // ascending (i, j): a stable pass by j, then one by i; the pairs are unique and every row's place is
  // fixed by the scan, so the list is the same whatever order the candidates were met in
  const int bits = bit_length(uint64_t(n));
  int32_t* perm = nullptr;
  PQ_TRY(refine_order_by_key(c, np, d_pj, &perm, bits));
  PQ_TRY(refine_order_by_key(c, np, d_pi, &perm, bits));
  const int rows = int(std::min<int64_t>(np, capacity));
  PQ_TRY(c->arena.get(size_t(rows) * 2, &d_rows));
  hipLaunchKernelGGL(k_pair_rows, dim3(ceil_div(rows, 256)), dim3(256), 0, c->stream, rows,
                     static_cast<const int32_t*>(perm), static_cast<const int32_t*>(d_pi),
                     static_cast<const int32_t*>(d_pj), d_rows);
  PQ_HIP(hipGetLastError());
  return fetch(c, pairs, d_rows, size_t(rows) * 2);
}

int pyqsm_radius_components(const double* xyz, int64_t n, const double* radii, int32_t R, int32_t* component,
                            int32_t* sizes, int32_t* members, int64_t* n_components, int32_t device) {
  PQ_API_RANGE("pyqsm_radius_components");
  if (n < 0) return fail(PYQSM_EINVAL, "negative size");
  if (!radii || !n_components || (n > 0 && (!xyz || !component || !sizes)))
    return fail(PYQSM_EINVAL, "pyqsm_radius_components: NULL pointer");
  if (R < 1 || R > kDegMaxRadii)
    return fail(PYQSM_ERANGE, "pyqsm_radius_components: %d radii, 1 to %d per call", R, kDegMaxRadii);
  double rmax = 0.0;
  for (int k = 0; k < R; ++k) {
    if (!(radii[k] > 0) || !std::isfinite(radii[k])) return fail(PYQSM_EINVAL, "radius must be positive and finite");
    rmax = std::max(rmax, radii[k]);
  }
  if (n > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 points per call");
  for (int k = 0; k < R; ++k) n_components[k] = 0;
  if (n == 0) return 0;
  PQ_TRY(finite_cloud(xyz, n));
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double* d_xyz;
  PQ_TRY(upload(c, xyz, size_t(n) * 3, &d_xyz));
  DevGrid g;
  PQ_TRY(radius_grid(c, d_xyz, n, rmax, &g));
  CellRuns cr;
  PQ_TRY(cell_runs(c, g, n, &cr));
  for (int k = 0; k < R; ++k) {
    const size_t row = size_t(k) * size_t(n);
    PQ_TRY(components_at(c, g, cr, radii[k], n, component + row, sizes + row, members ? members + row : nullptr,
                         &n_components[k]));
  }
  return 0;
}

}  // extern "C"
