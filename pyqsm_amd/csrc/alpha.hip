// alpha.hip — the exact area of a 2-D alpha shape of lattice points, batched, on gfx950.
//
//   pyqsm_alpha_area    for every segment (an independent cloud of int32 lattice points) the total
//                       area of the cells of its Delaunay subdivision whose circumradius^2 <= A2: the
//                       quantity pyQSM's viz/ray_casting.py project_pcd reads off VTK's
//                       delaunay_2d(alpha).area, without a triangulation.
//
// Every directed edge a->b is decided on its own. With e = b - a, u = p - a, D = cross(e, u),
// N = u.(u - e) and t_p = N / D for a third point p: tl = min t_p over D > 0, tr = max t_p over
// D < 0; D == 0 with N < 0 (p strictly inside the segment) kills the edge. a->b is an edge of the
// subdivision iff it is not killed and one side is empty or tr < tl; its left cell has
// circumradius^2 |e|^2 (1 + tl^2) / 4 and is kept iff |e|^2 (D^2 + N^2) <= 4 A2 D^2 at the
// minimising point; a kept left cell adds cross(a, b) to twice the area (Green). The right cell is
// the left cell of b->a and follows from tr the same way: kept left, not kept right = boundary edge.
//
// Exactness. Coordinates are taken relative to the segment's corner, 0 <= x, y <= 2^20, and
// A2 <= 2^40 (the entry point refuses anything else). Then |e_x|, |u_x|, ... <= 2^20, so
//   |D| = |e_x u_y - e_y u_x| <= 2^41,  |N| = |u_x (u_x - e_x) + u_y (u_y - e_y)| <= 2^41,
//   |e|^2 <= 2^41, 4 A2 <= 2^42: D, N and |e|^2 are integers below 2^53, exact in fp64 and in i64;
//   the t comparisons N_p D_q <> N_q D_p are products below 2^82, exact in __int128;
//   |e|^2 (N^2 + D^2) <= 2^41 * 2^83 = 2^124 and 4 A2 D^2 <= 2^42 * 2^82 = 2^124, both below 2^127.
// The t comparisons of the inner loop are first evaluated in fp64: lhs = fl(N_p D_q),
// rhs = fl(N_q D_p), diff = fl(lhs - rhs). Each product carries a relative error of at most 2^-53
// and so does the subtraction: |diff - (N_p D_q - N_q D_p)| <= 2^-52 (|lhs| + |rhs|) (1 + 2^-52).
// The sign of diff is taken only when |diff| > 2^-50 (|lhs| + |rhs|), four times that bound;
// everything else (exact ties of cocircular points among it) is decided by the 128-bit integers.
// The decisions per edge (edge or not, kept or not) are integer comparisons only.
//
// Locality. A circle of radius <= alpha through a lies within 2 alpha of a, and any point that would
// lower tl or break tr < tl for a kept cell lies inside that cell's circle: with cells of edge
// >= 2 alpha the 3 x 3 stencil of a's cell decides every kept cell exactly. Cells that are not kept
// add nothing, whatever the stencil misses.
//
// One block serves up to 32 points of one grid cell (a cell of a projected stem holds hundreds of times
// the points of a cell of the crown): the directed edges a->b with a among them, b in the cell's stencil and
// |e|^2 <= 4 A2 are collected in an LDS queue (ballot-compacted, so no lane idles on a pair out of
// reach), one lane owns one edge and reduces tl / tr over the stencil, whose coordinates are staged
// in LDS in chunks and read as broadcasts. cross(a, b) is summed in wrapping 64-bit integers per
// block and added to the segment's total by one 64-bit integer atomicAdd: the same bits whatever
// the arrival order. Boundary edges are appended to a list and then sorted by (a, b), a unique key:
// the list that leaves the library does not depend on the order of the appends either.
#include "common.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace pyqsm {

static constexpr int kAlphaChunk = 2048;                       // stencil points staged at a time (32 KiB)
static constexpr int kAlphaSlice = 32;                         // points of a cell one block of the edge pass serves
static constexpr int64_t kAlphaMaxExtent = int64_t(1) << 20;   // per axis within a segment
static constexpr uint64_t kAlphaMaxA2 = uint64_t(1) << 40;
static constexpr int64_t kAlphaMaxCells = int64_t(1) << 30;
// ten seconds of the edge pass at the 4.0e11 tests per second measured on one MI355X (DESIGN.md §17,
// profiles/projection_perf.jsonl); executed tests never exceed the estimate the cap is compared with
static constexpr int64_t kAlphaDefaultMaxTests = PYQSM_ALPHA_DEFAULT_MAX_TESTS;

struct AlphaSeg {
  int32_t x0, y0;    // the segment's corner on the caller's lattice
  int32_t edge;      // cell edge in lattice units, edge^2 >= 4 A2
  int32_t nx, ny;    // cells per axis
  int32_t skip;      // decided on the host (fewer than three live points, or collinear)
};

__device__ __forceinline__ int alpha_seg_of_cell(const int32_t* __restrict__ cell0, int n_seg, int c) {
  int lo = 0, hi = n_seg;  // the last s with cell0[s] <= c (empty segments share a cell0: the last one wins,
  while (hi - lo > 1) {    // and a non-empty cell belongs to the only segment that owns cells there)
    const int mid = (lo + hi) >> 1;
    if (cell0[mid] <= c) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_alpha_keys(int n, const int32_t* __restrict__ ij,
                                                    const int32_t* __restrict__ seg_of,
                                                    const AlphaSeg* __restrict__ segs,
                                                    const int32_t* __restrict__ cell0, uint32_t ncell,
                                                    uint32_t* __restrict__ keys, int32_t* __restrict__ vals) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int s = seg_of[i];
  const AlphaSeg g = segs[s];
  uint32_t key = ncell;  // points of skipped segments sort behind every cell
  if (!g.skip) {
    const int cx = (ij[2 * i] - g.x0) / g.edge, cy = (ij[2 * i + 1] - g.y0) / g.edge;
    key = uint32_t(cell0[s] + cy * g.nx + cx);
  }
  keys[i] = key;
  vals[i] = i;
}

// start[c] = the first sorted position whose key is >= c, c in [0, ncell]
__global__ __launch_bounds__(256) void k_alpha_cell_start(int ncell, const uint32_t* __restrict__ keys, int n,
                                                          int32_t* __restrict__ start) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c > ncell) return;
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < uint32_t(c)) lo = mid + 1;
    else hi = mid;
  }
  start[c] = lo;
}

// flags[p] = 1 unless an earlier point of the cell (a lower original index: the sort is stable) has
// the same coordinates; flags[m] = 0 for the scan.
__global__ __launch_bounds__(256) void k_alpha_live(int m, const int32_t* __restrict__ order,
                                                    const uint32_t* __restrict__ keys,
                                                    const int32_t* __restrict__ start,
                                                    const int32_t* __restrict__ ij, int32_t* __restrict__ flags) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p > m) return;
  if (p == m) {
    flags[p] = 0;
    return;
  }
  const int i = order[p];
  const int x = ij[2 * i], y = ij[2 * i + 1];
  int live = 1;
  for (int q = start[keys[p]]; q < p; ++q) {
    const int j = order[q];
    if (ij[2 * j] == x && ij[2 * j + 1] == y) {
      live = 0;
      break;
    }
  }
  flags[p] = live;
}

// the live points in sorted order: coordinates relative to the segment's corner, original index
__global__ __launch_bounds__(256) void k_alpha_gather(int m, const int32_t* __restrict__ pos,
                                                      const int32_t* __restrict__ order,
                                                      const int32_t* __restrict__ ij,
                                                      const int32_t* __restrict__ seg_of,
                                                      const AlphaSeg* __restrict__ segs, int32_t* __restrict__ lx,
                                                      int32_t* __restrict__ ly, int32_t* __restrict__ lorig) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= m) return;
  const int q = pos[p];
  if (pos[p + 1] == q) return;
  const int i = order[p];
  const AlphaSeg g = segs[seg_of[i]];
  lx[q] = ij[2 * i] - g.x0;
  ly[q] = ij[2 * i + 1] - g.y0;
  lorig[q] = i;
}

__global__ __launch_bounds__(256) void k_alpha_live_start(int ncell, const int32_t* __restrict__ start,
                                                          const int32_t* __restrict__ pos,
                                                          int32_t* __restrict__ lstart) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c <= ncell) lstart[c] = pos[start[c]];
}

__global__ __launch_bounds__(256) void k_alpha_seg_live(int n_seg, const int32_t* __restrict__ cell0,
                                                        const int32_t* __restrict__ lstart,
                                                        int64_t* __restrict__ seg_live) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s < n_seg) seg_live[s] = lstart[cell0[s + 1]] - lstart[cell0[s]];
}

struct AlphaStencil {
  int lo[3], n[3];  // the three rows of the 3 x 3 stencil as ranges of live positions
  int total;
  __device__ __forceinline__ int at(int j) const {
    if (j < n[0]) return lo[0] + j;
    j -= n[0];
    if (j < n[1]) return lo[1] + j;
    return lo[2] + (j - n[1]);
  }
};

__device__ __forceinline__ AlphaStencil alpha_stencil(const AlphaSeg& g, int base, int local,
                                                      const int32_t* __restrict__ lstart) {
  AlphaStencil st;
  const int cy = local / g.nx, cx = local - cy * g.nx;
  const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx + 1 < g.nx ? cx + 1 : g.nx - 1;
  st.total = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int yy = cy + k - 1;
    st.lo[k] = 0;
    st.n[k] = 0;
    if (yy >= 0 && yy < g.ny) {
      const int row = base + yy * g.nx;
      st.lo[k] = lstart[row + x0];
      st.n[k] = lstart[row + x1 + 1] - st.lo[k];
    }
    st.total += st.n[k];
  }
  return st;
}

// nblk[c] = blocks of the edge pass for cell c (kAlphaSlice of its points each), nblk[ncell] = 0; scanned
// in place it maps a block to its cell: a projected cloud stacks points, and a cell of a stem holds
// hundreds of times the points of a cell of the crown.
__global__ __launch_bounds__(256) void k_alpha_blocks(int ncell, const int32_t* __restrict__ lstart,
                                                      int32_t* __restrict__ nblk) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c > ncell) return;
  nblk[c] = c < ncell ? (lstart[c + 1] - lstart[c] + kAlphaSlice - 1) / kAlphaSlice : 0;
}

// est[0] += low 32 bits, est[1] += high bits of (points of the cell) * (stencil count)^2, clamped to
// 2^62 per cell: two sums that cannot wrap, put together on the host.
__global__ __launch_bounds__(256) void k_alpha_estimate(int ncell, int n_seg, const AlphaSeg* __restrict__ segs,
                                                        const int32_t* __restrict__ cell0,
                                                        const int32_t* __restrict__ lstart,
                                                        unsigned long long* __restrict__ est) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ncell) return;
  const int m = lstart[c + 1] - lstart[c];
  if (m == 0) return;
  const int s = alpha_seg_of_cell(cell0, n_seg, c);
  const AlphaStencil st = alpha_stencil(segs[s], cell0[s], c - cell0[s], lstart);
  unsigned __int128 v = (unsigned __int128)(unsigned)st.total * (unsigned)st.total * (unsigned)m;
  const unsigned __int128 cap = (unsigned __int128)1 << 62;
  const unsigned long long w = (unsigned long long)(v < cap ? v : cap);
  atomicAdd(&est[0], w & 0xFFFFFFFFull);
  atomicAdd(&est[1], w >> 32);
}

// acc [n_seg]: twice the area; nbound [n_seg]: boundary edges; stats: [0] tests, [1] exact
// fallbacks, [2] directed edges within reach; cursor: boundary edges appended to ea / eb.
__global__ __launch_bounds__(256) void k_alpha_edges(int ncell, const int32_t* __restrict__ blk_start, int n_seg,
                                                     const AlphaSeg* __restrict__ segs,
                                                     const int32_t* __restrict__ cell0,
                                                     const int32_t* __restrict__ lstart,
                                                     const int32_t* __restrict__ lx, const int32_t* __restrict__ ly,
                                                     const int32_t* __restrict__ lorig, unsigned long long four_a2,
                                                     unsigned long long* __restrict__ acc,
                                                     unsigned long long* __restrict__ nbound,
                                                     unsigned long long* __restrict__ stats, long long edge_cap,
                                                     int32_t* __restrict__ ea, int32_t* __restrict__ eb,
                                                     unsigned long long* __restrict__ cursor) {
  __shared__ double sx[kAlphaChunk], sy[kAlphaChunk];
  __shared__ int qa[512], qb[512];
  __shared__ int qn, s_seg, s_cell;
  __shared__ unsigned long long s_acc, s_nb, s_tests, s_exact, s_edges;
  const int t = threadIdx.x;
  if (t == 0) {
    int lo = 0, hi = ncell;  // the cell c with blk_start[c] <= blockIdx.x < blk_start[c + 1]
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (blk_start[mid + 1] <= int(blockIdx.x)) lo = mid + 1;
      else hi = mid;
    }
    s_cell = lo;
    s_seg = alpha_seg_of_cell(cell0, n_seg, lo);
    qn = 0;
    s_acc = s_nb = s_tests = s_exact = s_edges = 0;
  }
  __syncthreads();
  const int c = s_cell, s = s_seg;
  const int first = (int(blockIdx.x) - blk_start[c]) * kAlphaSlice;  // this block's points of the cell
  const int a0 = lstart[c] + first;
  const int m = min(kAlphaSlice, lstart[c + 1] - a0);
  if (c >= ncell || m <= 0) return;  // block-uniform; cannot happen for a block inside the scanned total
  const AlphaStencil st = alpha_stencil(segs[s], cell0[s], c - cell0[s], lstart);
  const int S = st.total;
  const long long W = (long long)m * S;  // candidate pairs (a in the cell, b in the stencil)
  const bool one_chunk = S <= kAlphaChunk;
  if (one_chunk) {
    for (int j = t; j < S; j += 256) {
      const int p = st.at(j);
      sx[j] = double(lx[p]);
      sy[j] = double(ly[p]);
    }
    __syncthreads();
  }
  long long my_acc = 0;
  unsigned my_nb = 0, my_exact = 0, my_edges = 0;
  unsigned long long my_tests = 0;
  long long cand = 0;
  for (;;) {
    // fill the queue with pairs within reach, in tiles of 256 candidates
    int have = qn;
    while (have < 256 && cand < W) {
      const long long idx = cand + t;
      int pa = 0, pb = 0;
      bool active = false;
      if (idx < W) {
        int ai, bj;
        if (W < (1ll << 31)) {
          ai = int(unsigned(idx) / unsigned(S));
          bj = int(unsigned(idx) - unsigned(ai) * unsigned(S));
        } else {
          ai = int(idx / S);
          bj = int(idx - (long long)ai * S);
        }
        pa = a0 + ai;
        pb = st.at(bj);
        const long long dx = (long long)lx[pb] - lx[pa], dy = (long long)ly[pb] - ly[pa];
        active = pa != pb && (unsigned long long)(dx * dx + dy * dy) <= four_a2;
      }
      const unsigned long long mask = __ballot(active);
      int base = 0;
      if ((t & 63) == 0 && mask) base = atomicAdd(&qn, __popcll(mask));
      base = __shfl(base, 0);
      if (active) {
        const int at = base + __popcll(mask & ((1ull << (t & 63)) - 1ull));
        qa[at] = pa;
        qb[at] = pb;
      }
      cand += 256;
      __syncthreads();
      have = qn;
      __syncthreads();
    }
    if (have == 0) break;
    const int take = have < 256 ? have : 256;
    const bool mine = t < take;
    int pa = 0, pb = 0;
    double ax = 0, ay = 0, ex = 0, ey = 0;
    if (mine) {
      pa = qa[t];
      pb = qb[t];
      ax = double(lx[pa]);
      ay = double(ly[pa]);
      ex = double(lx[pb]) - ax;
      ey = double(ly[pb]) - ay;
    }
    double nl = 0, dl = 0, nr = 0, dr = 0;  // dl > 0: the left side has a point; dr < 0: the right side
    bool killed = false;
    for (int k0 = 0; k0 < S; k0 += kAlphaChunk) {
      const int cn = S - k0 < kAlphaChunk ? S - k0 : kAlphaChunk;
      if (!one_chunk) {
        __syncthreads();
        for (int j = t; j < cn; j += 256) {
          const int p = st.at(k0 + j);
          sx[j] = double(lx[p]);
          sy[j] = double(ly[p]);
        }
        __syncthreads();
      }
      if (!mine) continue;
      for (int j = 0; j < cn; ++j) {
        const double ux = sx[j] - ax, uy = sy[j] - ay;
        const double D = ex * uy - ey * ux;
        const double N = ux * (ux - ex) + uy * (uy - ey);
        if (D > 0) {
          bool better = !(dl > 0);
          if (!better) {  // t_p < tl  <=>  N dl < nl D   (D, dl > 0)
            const double lhs = N * dl, rhs = nl * D, diff = lhs - rhs;
            const double tol = (fabs(lhs) + fabs(rhs)) * 0x1p-50;
            if (diff < -tol) better = true;
            else if (!(diff > tol)) {
              ++my_exact;
              better = (__int128)(long long)N * (long long)dl < (__int128)(long long)nl * (long long)D;
            }
          }
          if (better) {
            nl = N;
            dl = D;
          }
        } else if (D < 0) {
          bool better = !(dr < 0);
          if (!better) {  // t_p > tr  <=>  N dr > nr D   (D, dr < 0)
            const double lhs = N * dr, rhs = nr * D, diff = lhs - rhs;
            const double tol = (fabs(lhs) + fabs(rhs)) * 0x1p-50;
            if (diff > tol) better = true;
            else if (!(diff < -tol)) {
              ++my_exact;
              better = (__int128)(long long)N * (long long)dr > (__int128)(long long)nr * (long long)D;
            }
          }
          if (better) {
            nr = N;
            dr = D;
          }
        } else if (N < 0) {
          killed = true;
        }
      }
    }
    if (mine) {
      my_tests += (unsigned long long)S;
      ++my_edges;
      const bool has_l = dl > 0, has_r = dr < 0;
      const long long NL = (long long)nl, DL = (long long)dl, NR = (long long)nr, DR = (long long)dr;
      // tr < tl  <=>  NR / DR < NL / DL  <=>  NR DL > NL DR   (DR DL < 0)
      const bool is_edge = !killed && (!has_l || !has_r || (__int128)NR * DL > (__int128)NL * DR);
      if (is_edge && has_l) {
        const unsigned __int128 e2 = (unsigned __int128)(unsigned long long)(long long)(ex * ex + ey * ey);
        const unsigned __int128 dl2 = (unsigned __int128)((__int128)DL * DL);
        const unsigned __int128 nl2 = (unsigned __int128)((__int128)NL * NL);
        if (e2 * (dl2 + nl2) <= (unsigned __int128)four_a2 * dl2) {  // the left cell is kept
          const long long bx = (long long)lx[pb], by = (long long)ly[pb];
          my_acc += (long long)lx[pa] * by - (long long)ly[pa] * bx;
          bool kept_r = false;
          if (has_r) {
            const unsigned __int128 dr2 = (unsigned __int128)((__int128)DR * DR);
            const unsigned __int128 nr2 = (unsigned __int128)((__int128)NR * NR);
            kept_r = e2 * (dr2 + nr2) <= (unsigned __int128)four_a2 * dr2;
          }
          if (!kept_r) {
            ++my_nb;
            if (ea) {
              const unsigned long long at = atomicAdd(cursor, 1ull);
              if ((long long)at < edge_cap) {
                ea[at] = lorig[pa];
                eb[at] = lorig[pb];
              }
            }
          }
        }
      }
    }
    // drop the served entries
    __syncthreads();
    const int rest = have - take;
    int ra = 0, rb = 0;
    if (t < rest) {
      ra = qa[take + t];
      rb = qb[take + t];
    }
    __syncthreads();
    if (t < rest) {
      qa[t] = ra;
      qb[t] = rb;
    }
    if (t == 0) qn = rest;
    __syncthreads();
  }
  if (my_acc) atomicAdd(&s_acc, (unsigned long long)my_acc);
  if (my_nb) atomicAdd(&s_nb, (unsigned long long)my_nb);
  if (my_tests) atomicAdd(&s_tests, my_tests);
  if (my_exact) atomicAdd(&s_exact, (unsigned long long)my_exact);
  if (my_edges) atomicAdd(&s_edges, (unsigned long long)my_edges);
  __syncthreads();
  if (t == 0) {
    if (s_acc) atomicAdd(&acc[s], s_acc);
    if (s_nb) atomicAdd(&nbound[s], s_nb);
    atomicAdd(&stats[0], s_tests);
    if (s_exact) atomicAdd(&stats[1], s_exact);
    atomicAdd(&stats[2], s_edges);
  }
}

__global__ __launch_bounds__(256) void k_alpha_edge_rows(int e, const int32_t* __restrict__ perm,
                                                         const int32_t* __restrict__ ea,
                                                         const int32_t* __restrict__ eb, int64_t* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= e) return;
  const int j = perm[i];
  out[2 * size_t(i)] = ea[j];
  out[2 * size_t(i) + 1] = eb[j];
}

// The live points of a segment the host settles (fewer than three points, or all on one line).
static int64_t alpha_host_live(const int32_t* ij, int64_t lo, int64_t hi) {
  std::vector<std::pair<int32_t, int32_t>> v;
  v.reserve(size_t(hi - lo));
  for (int64_t i = lo; i < hi; ++i) v.emplace_back(ij[2 * i], ij[2 * i + 1]);
  std::sort(v.begin(), v.end());
  return int64_t(std::unique(v.begin(), v.end()) - v.begin());
}

// true when every point of [lo, hi) lies on one line (or there are fewer than three distinct ones)
static bool alpha_collinear(const int32_t* ij, int64_t lo, int64_t hi) {
  const int64_t ax = ij[2 * lo], ay = ij[2 * lo + 1];
  int64_t i = lo + 1;
  while (i < hi && ij[2 * i] == ax && ij[2 * i + 1] == ay) ++i;
  if (i == hi) return true;
  const int64_t ex = ij[2 * i] - ax, ey = ij[2 * i + 1] - ay;  // |ex|, |ey| <= 2^20: the cross fits
  for (++i; i < hi; ++i)
    if (ex * (ij[2 * i + 1] - ay) - ey * (ij[2 * i] - ax) != 0) return false;
  return true;
}

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_alpha_area(const int32_t* ij, int64_t n, const int64_t* seg_start, int64_t n_seg, uint64_t a2,
                     int64_t max_tests, int32_t flags, int64_t* twice_area, int64_t* n_live, int64_t* n_boundary,
                     int64_t** edges, int64_t* stats, int32_t device) {
  PQ_API_RANGE("pyqsm_alpha_area");
  if (edges) *edges = nullptr;
  if (stats) std::fill(stats, stats + 5, int64_t(0));
  if (flags & ~PYQSM_ALPHA_BOUNDARY) return fail(PYQSM_EINVAL, "pyqsm_alpha_area: unknown flag");
  const bool want_edges = (flags & PYQSM_ALPHA_BOUNDARY) != 0;
  if (n < 0 || n_seg < 0) return fail(PYQSM_EINVAL, "negative size");
  if (!seg_start || (n > 0 && !ij) || (n_seg > 0 && (!twice_area || !n_live || !n_boundary)) ||
      (want_edges && !edges))
    return fail(PYQSM_EINVAL, "pyqsm_alpha_area: NULL pointer");
  if (seg_start[0] != 0 || seg_start[n_seg] != n)
    return fail(PYQSM_EINVAL, "seg_start must run from 0 to n");
  for (int64_t s = 0; s < n_seg; ++s)
    if (seg_start[s + 1] < seg_start[s]) return fail(PYQSM_EINVAL, "seg_start must not decrease");
  if (a2 > kAlphaMaxA2)
    return fail(PYQSM_EINVAL, "A2 = %llu exceeds 2^40 lattice units^2: use a coarser quantum",
                (unsigned long long)a2);
  if (n > 0x7FFFFF00LL || n_seg > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 points per call");
  if (max_tests <= 0) max_tests = kAlphaDefaultMaxTests;

  // the smallest cell edge with edge^2 >= 4 A2: 2 alpha, rounded up
  const uint64_t four_a2 = 4 * a2;
  int64_t edge0 = int64_t(std::sqrt(double(four_a2)));
  while (uint64_t(edge0) * uint64_t(edge0) < four_a2) ++edge0;
  while (edge0 > 1 && uint64_t(edge0 - 1) * uint64_t(edge0 - 1) >= four_a2) --edge0;
  if (edge0 < 1) edge0 = 1;

  std::vector<AlphaSeg> segs(size_t(n_seg) + 1);
  std::vector<int32_t> cell0(size_t(n_seg) + 1), seg_of(size_t(n), 0);
  int64_t ncell = 0, host_merged = 0;  // duplicates of the segments settled on the host
  bool any = false;
  for (int64_t s = 0; s < n_seg; ++s) {
    const int64_t lo = seg_start[s], hi = seg_start[s + 1];
    AlphaSeg g{0, 0, 1, 0, 0, 1};
    twice_area[s] = 0;
    n_boundary[s] = 0;
    n_live[s] = 0;
    cell0[size_t(s)] = int32_t(ncell);
    if (hi > lo) {
      int32_t x0 = ij[2 * lo], x1 = x0, y0 = ij[2 * lo + 1], y1 = y0;
      for (int64_t i = lo; i < hi; ++i) {
        x0 = std::min(x0, ij[2 * i]);
        x1 = std::max(x1, ij[2 * i]);
        y0 = std::min(y0, ij[2 * i + 1]);
        y1 = std::max(y1, ij[2 * i + 1]);
        seg_of[size_t(i)] = int32_t(s);
      }
      const int64_t wx = int64_t(x1) - x0, wy = int64_t(y1) - y0;
      if (wx > kAlphaMaxExtent || wy > kAlphaMaxExtent)
        return fail(PYQSM_EINVAL, "segment %lld spans %lld x %lld lattice units, more than 2^20: use a coarser quantum",
                    (long long)s, (long long)wx, (long long)wy);
      if (hi - lo < 3 || alpha_collinear(ij, lo, hi)) {
        n_live[s] = alpha_host_live(ij, lo, hi);
        host_merged += (hi - lo) - n_live[s];
      } else {
        int64_t edge = edge0;
        while ((wx / edge + 1) * (wy / edge + 1) > 4 * (hi - lo) + 16) edge *= 2;
        g = AlphaSeg{x0, y0, int32_t(edge), int32_t(wx / edge + 1), int32_t(wy / edge + 1), 0};
        ncell += int64_t(g.nx) * g.ny;
        if (ncell > kAlphaMaxCells) return fail(PYQSM_ERANGE, "more than 2^30 grid cells");
        any = true;
      }
    }
    segs[size_t(s)] = g;
  }
  cell0[size_t(n_seg)] = int32_t(ncell);
  if (stats) stats[4] = host_merged;
  if (!any) return 0;  // every segment is degenerate: no device work

  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  int32_t *d_ij, *d_seg_of, *d_cell0, *d_vals, *d_start, *d_flags, *d_lx, *d_ly, *d_lorig, *d_lstart, *d_blk;
  uint32_t* d_keys;
  AlphaSeg* d_segs;
  int64_t* d_seg_live;
  unsigned long long* d_counters;  // est[2], stats[3], cursor, then acc [n_seg], nbound [n_seg]
  PQ_TRY(c->arena.get(size_t(n) * 2, &d_ij));
  PQ_TRY(c->arena.get(size_t(n), &d_seg_of));
  PQ_TRY(c->arena.get(size_t(n_seg) + 1, &d_cell0));
  PQ_TRY(c->arena.get(size_t(n_seg) + 1, &d_segs));
  PQ_TRY(c->arena.get(size_t(n), &d_keys));
  PQ_TRY(c->arena.get(size_t(n), &d_vals));
  PQ_TRY(c->arena.get(size_t(ncell) + 1, &d_start));
  PQ_TRY(c->arena.get(size_t(ncell) + 1, &d_lstart));
  PQ_TRY(c->arena.get(size_t(ncell) + 1, &d_blk));
  PQ_TRY(c->arena.get(size_t(n) + 1, &d_flags));
  PQ_TRY(c->arena.get(size_t(n), &d_lx));
  PQ_TRY(c->arena.get(size_t(n), &d_ly));
  PQ_TRY(c->arena.get(size_t(n), &d_lorig));
  PQ_TRY(c->arena.get(size_t(n_seg), &d_seg_live));
  const size_t n_counters = 6 + 2 * size_t(n_seg);
  PQ_TRY(c->arena.get(n_counters, &d_counters));
  unsigned long long *d_est = d_counters, *d_stats = d_counters + 2, *d_cursor = d_counters + 5,
                     *d_acc = d_counters + 6, *d_nb = d_acc + n_seg;
  PQ_TRY(copy_in(c, d_ij, ij, size_t(n) * 2));
  PQ_TRY(copy_in(c, d_seg_of, seg_of.data(), size_t(n)));
  PQ_TRY(copy_in(c, d_cell0, cell0.data(), size_t(n_seg) + 1));
  PQ_TRY(copy_in(c, d_segs, segs.data(), size_t(n_seg) + 1));
  PQ_HIP(hipMemsetAsync(d_counters, 0, n_counters * 8, c->stream));

  const int nc = int(ncell);
  std::vector<int64_t> seg_live(size_t(n_seg), 0);
  unsigned long long est[2] = {0, 0};
  int32_t n_part = 0, total_live = 0, n_blocks = 0;
  {
    ProfScope ps(c, "alpha_bin");
    hipLaunchKernelGGL(k_alpha_keys, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, int(n), d_ij, d_seg_of, d_segs,
                       d_cell0, uint32_t(nc), d_keys, d_vals);
    PQ_HIP(hipGetLastError());
    PQ_TRY(stable_sort_pairs_u32(c, &d_keys, &d_vals, n, bit_length(uint64_t(nc))));
    hipLaunchKernelGGL(k_alpha_cell_start, dim3(ceil_div(nc + 1, 256)), dim3(256), 0, c->stream, nc,
                       static_cast<const uint32_t*>(d_keys), int(n), d_start);
    PQ_HIP(hipGetLastError());
    PQ_TRY(fetch(c, &n_part, d_start + nc));  // points of the segments that take part, a host-known number
    hipLaunchKernelGGL(k_alpha_live, dim3(ceil_div(n_part + 1, 256)), dim3(256), 0, c->stream, n_part,
                       static_cast<const int32_t*>(d_vals), static_cast<const uint32_t*>(d_keys),
                       static_cast<const int32_t*>(d_start), d_ij, d_flags);
    PQ_HIP(hipGetLastError());
    PQ_TRY(exclusive_scan_i32(c, d_flags, int64_t(n_part) + 1));
    hipLaunchKernelGGL(k_alpha_gather, dim3(ceil_div(n_part, 256)), dim3(256), 0, c->stream, n_part,
                       static_cast<const int32_t*>(d_flags), static_cast<const int32_t*>(d_vals), d_ij, d_seg_of,
                       d_segs, d_lx, d_ly, d_lorig);
    PQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_alpha_live_start, dim3(ceil_div(nc + 1, 256)), dim3(256), 0, c->stream, nc,
                       static_cast<const int32_t*>(d_start), static_cast<const int32_t*>(d_flags), d_lstart);
    PQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_alpha_seg_live, dim3(ceil_div(n_seg, 256)), dim3(256), 0, c->stream, int(n_seg), d_cell0,
                       static_cast<const int32_t*>(d_lstart), d_seg_live);
    PQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_alpha_estimate, dim3(ceil_div(nc, 256)), dim3(256), 0, c->stream, nc, int(n_seg), d_segs,
                       d_cell0, static_cast<const int32_t*>(d_lstart), d_est);
    PQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_alpha_blocks, dim3(ceil_div(nc + 1, 256)), dim3(256), 0, c->stream, nc,
                       static_cast<const int32_t*>(d_lstart), d_blk);
    PQ_HIP(hipGetLastError());
    PQ_TRY(exclusive_scan_i32(c, d_blk, int64_t(nc) + 1));
    PQ_TRY(download(c, &n_blocks, d_blk + nc, 1));
    PQ_TRY(download(c, seg_live.data(), d_seg_live, size_t(n_seg)));
    PQ_TRY(download(c, est, d_est, 2));
    PQ_TRY(download(c, &total_live, d_lstart + nc, 1));
    PQ_HIP(hipStreamSynchronize(c->stream));
  }
  for (int64_t s = 0; s < n_seg; ++s)
    if (!segs[size_t(s)].skip) n_live[s] = seg_live[size_t(s)];
  const unsigned __int128 est_all = ((unsigned __int128)est[1] << 32) + est[0];
  const int64_t est_tests = est_all > (unsigned __int128)INT64_MAX ? INT64_MAX : int64_t(est_all);
  if (stats) {
    stats[0] = est_tests;
    stats[4] = host_merged + int64_t(n_part) - total_live;
  }
  if (est_tests > max_tests)
    return fail(PYQSM_ERANGE,
                "pyqsm_alpha_area: an estimated %lld edge tests exceed max_tests = %lld (alpha spans many point "
                "spacings: down-sample the cloud, lower alpha or raise max_tests)",
                (long long)est_tests, (long long)max_tests);

  const int64_t edge_cap = want_edges ? 3 * int64_t(total_live) + 1 : 0;  // a planar graph has < 3 n edges
  int32_t *d_ea = nullptr, *d_eb = nullptr;
  if (want_edges) {
    PQ_TRY(c->arena.get(size_t(edge_cap), &d_ea));
    PQ_TRY(c->arena.get(size_t(edge_cap), &d_eb));
  }
  {
    ProfScope ps(c, "alpha_edges");
    if (n_blocks > 0)
      hipLaunchKernelGGL(k_alpha_edges, dim3(unsigned(n_blocks)), dim3(256), 0, c->stream, nc,
                       static_cast<const int32_t*>(d_blk), int(n_seg),
                       static_cast<const AlphaSeg*>(d_segs), static_cast<const int32_t*>(d_cell0),
                       static_cast<const int32_t*>(d_lstart), static_cast<const int32_t*>(d_lx),
                       static_cast<const int32_t*>(d_ly), static_cast<const int32_t*>(d_lorig),
                       (unsigned long long)four_a2, d_acc, d_nb, d_stats, (long long)edge_cap, d_ea, d_eb, d_cursor);
    PQ_HIP(hipGetLastError());
  }
  std::vector<unsigned long long> host(n_counters);
  PQ_TRY(fetch(c, host.data(), d_counters, n_counters));
  int64_t total_edges = 0;
  for (int64_t s = 0; s < n_seg; ++s) {
    twice_area[s] = int64_t(host[6 + size_t(s)]);
    n_boundary[s] = int64_t(host[6 + size_t(n_seg) + size_t(s)]);
    total_edges += n_boundary[s];
  }
  if (stats) {
    stats[1] = int64_t(host[2]);
    stats[2] = int64_t(host[3]);
    stats[3] = int64_t(host[4]);
  }
  if (!want_edges || total_edges == 0) return 0;
  if (int64_t(host[5]) != total_edges || total_edges > edge_cap)
    return fail(PYQSM_EHIP, "pyqsm_alpha_area: %lld boundary edges listed, %lld counted", (long long)host[5],
                (long long)total_edges);
  // ascending (a, b): a stable sort by b, then by a. Both indices belong to one segment and segments
  // are index ranges, so the rows are grouped by segment as well.
  const int e = int(total_edges), bits = bit_length(uint64_t(n));
  int64_t* d_rows;
  PQ_TRY(c->arena.get(size_t(e) * 2, &d_rows));
  {
    ProfScope ps(c, "alpha_boundary_sort");
    int32_t* perm = nullptr;
    PQ_TRY(refine_order_by_key(c, e, d_eb, &perm, bits));
    PQ_TRY(refine_order_by_key(c, e, d_ea, &perm, bits));
    hipLaunchKernelGGL(k_alpha_edge_rows, dim3(ceil_div(e, 256)), dim3(256), 0, c->stream, e,
                       static_cast<const int32_t*>(perm), static_cast<const int32_t*>(d_ea),
                       static_cast<const int32_t*>(d_eb), d_rows);
    PQ_HIP(hipGetLastError());
  }
  OutBufs out;
  int64_t* rows = out.get<int64_t>(size_t(e) * 2);
  if (!rows) return fail(PYQSM_ENOMEM, "pyqsm_alpha_area: no host memory for %d boundary edges", e);
  PQ_TRY(fetch(c, rows, d_rows, size_t(e) * 2));
  out.kept = true;
  *edges = rows;
  return 0;
}

}  // extern "C"
