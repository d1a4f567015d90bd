// knn.hip — exact k nearest neighbours of every point of a cloud on gfx950.
//
// Stands in for the neighbour search inside robust_laplacian.point_cloud_laplacian
// (pyQSM/geometry/skeletonize.py:253-255) and for scipy cKDTree.query
// (pyQSM/geometry/reconstruction.py:238-240).
//
// Method: points are counting-sorted into a uniform cell grid (grid.hip) whose
// edge is tuned so that an occupied cell holds about k/3 points. One lane per
// query walks Chebyshev shells of cells around its own cell (each shell row is
// one contiguous run of the sorted arrays) and keeps the best k candidates sorted in
// registers (k <= 32, k_knn_reg: by the distance alone in the first pass, ties detected and
// searched again exactly — see the kernel) or in a per-lane LDS column (element j of lane t
// at [j*T + t]: conflict-free, k_knn). A
// query is final once its k-th distance is no larger than the radius the
// visited cube is known to cover. The few queries that are not final after
// kMaxRing shells (isolated outliers) are retried, one wave per query, on a 4x coarser
// grid (binned from the points when the fine grid is large, else derived from it:
// grid.hip: coarsen_grid) with up to kWideRing shells, and on coarser ones still until the
// shells cover the whole grid. (If more than half of ALL queries are open after level 0 — coincident
// points met the planned occupancy — level 0 runs once more on the coarser grid first: knn_device.)
//
// (Measured alternative for level 0, MI355X, 1 M points, k = 20: a wave-tiled search like
// dbscan.hip's k_core_tiled — 64 consecutive queries, candidates broadcast from LDS, the K
// best per lane sorted in registers, branch-free insertion — took 9.0 ms against 5.1 ms for
// the per-lane walk below: almost every candidate beats SOME lane's current worst, so the
// ~300-instruction insertion step runs for nearly all of the tile's superset of candidates.)
//
// Distances are squared, fp64, ((dx*dx)+dy*dy)+dz*dz with separately rounded
// products — the accumulation order of scipy's cKDTree — and candidates are
// ordered by (d2, original index).
#include <atomic>

#include "grid.hpp"
#include "knn.hpp"

#include <cmath>
#include <string>
#include <type_traits>

namespace pyqsm {

static constexpr int kMaxRing = 3;
// The (wave-per-query) retries may walk this many shells: what is still open there are
// outliers, and one more 4x coarsening instead would make those next to a tree scan whole
// stems (a point 0.7 m from a trunk: 27 cells of 0.8 m; 4 such queries took 1.25 ms on the
// 1 M-point forest). From the first retry level on: 1.05 -> 0.83 ms for both levels with 8 shells.
// With 16 the first retry level finishes every outlier of the forest (1 % noise up to 5 m from a
// stem) and the second one — a coarsening of the grid and a launch whose duration is one long wave,
// 0.32 + 0.06 ms even for a single query — does not happen: retries 0.83 -> 0.38 ms. A query that
// does walk all 16 shells looks up 13 000 row segments (200 rounds of 64), about what a launch
// of the next level costs. PYQSM_KNN_WIDE overrides.
static constexpr int kWideRing = 16;

struct KnnGrid {
  int nx, ny, nz;
  double cell;
  double minx, miny, minz;  // origin of the interior cells (cell 1 starts here)
};

// sqdist3: grid.hpp

// T = threads per block (LDS holds T columns of k (d2, id) pairs).
template <int T, class CO>
__global__ __launch_bounds__(T) void k_knn(int n_query, const int32_t* __restrict__ query_list,
                                           const int32_t* __restrict__ pos_of /*orig->sorted*/,
                                           KnnGrid g, const int32_t* __restrict__ start,
                                           const int32_t* __restrict__ order,
                                           const int32_t* __restrict__ cell_of,
                                           CO co, int k,
                                           int exclude_self, int n_total, int last_level,
                                           int32_t* __restrict__ out_idx,
                                           double* __restrict__ out_d2,
                                           int32_t* __restrict__ fail_list,
                                           int32_t* __restrict__ fail_count) {
  extern __shared__ __align__(16) unsigned char smem[];
  double* bd = reinterpret_cast<double*>(smem);              // [k][T]
  int32_t* bi = reinterpret_cast<int32_t*>(bd + size_t(k) * T);  // [k][T]
  const int t = threadIdx.x;
  const int qi = blockIdx.x * T + t;
  if (qi >= n_query) return;
  // sorted position of this query
  const int p = query_list ? pos_of[query_list[qi]] : qi;
  const int self = order[p];
  double x, y, z;
  co.get(p, x, y, z);
  const int c = cell_of[p];
  const int cx = c % g.nx, cy = (c / g.nx) % g.ny, cz = c / (g.nx * g.ny);
  int have = 0;
  bool done = false;
  const int rmax_grid = max(g.nx, max(g.ny, g.nz));
  for (int r = 0; r <= kMaxRing && !done; ++r) {
    for (int dz = -r; dz <= r; ++dz) {
      const int zz = cz + dz;
      if (zz < 0 || zz >= g.nz) continue;
      for (int dy = -r; dy <= r; ++dy) {
        const int yy = cy + dy;
        if (yy < 0 || yy >= g.ny) continue;
        const int row = (zz * g.ny + yy) * g.nx;
        const bool full = (dz == -r || dz == r || dy == -r || dy == r);
        // full shell row: [cx-r, cx+r]; otherwise the two end cells only
        const int nseg = full ? 1 : (r > 0 ? 2 : 1);
        for (int s = 0; s < nseg; ++s) {
          int x0, x1;
          if (full) {
            x0 = cx - r;
            x1 = cx + r;
          } else {
            x0 = x1 = s == 0 ? cx - r : cx + r;
          }
          x0 = x0 < 0 ? 0 : x0;
          x1 = x1 >= g.nx ? g.nx - 1 : x1;
          if (x0 > x1) continue;
          const int qb = start[row + x0], qe = start[row + x1 + 1];
          for (int q = qb; q < qe; ++q) {
            if (exclude_self && q == p) continue;
            const double d = co.d2(q, x, y, z);
            const int id = order[q];
            if (have == k) {
              const double wd = bd[(k - 1) * T + t];
              if (d > wd || (d == wd && id > bi[(k - 1) * T + t])) continue;
            }
            int j = have < k ? have : k - 1;
            while (j > 0) {
              const double pd = bd[(j - 1) * T + t];
              const int pi = bi[(j - 1) * T + t];
              if (pd < d || (pd == d && pi < id)) break;
              bd[j * T + t] = pd;
              bi[j * T + t] = pi;
              --j;
            }
            bd[j * T + t] = d;
            bi[j * T + t] = id;
            if (have < k) ++have;
          }
        }
      }
    }
    // everything outside the visited cube is at least r cells away
    const double safe = double(r) * g.cell * 0.999999;
    if (have == k && bd[(k - 1) * T + t] <= safe * safe) done = true;
    if (r >= rmax_grid) done = true;  // the cube already covers the whole grid
  }
  if (!done && !last_level) {
    fail_list[atomicAdd(fail_count, 1)] = self;
    return;
  }
  for (int j = 0; j < k; ++j) {
    out_idx[size_t(self) * k + j] = j < have ? bi[j * T + t] : n_total;
    if (out_d2) out_d2[size_t(self) * k + j] = j < have ? bd[j * T + t] : __builtin_inf();
  }
}


// Level-0 search for k <= 32: the same per-lane shell walk, but the sorted best-K list lives
// in REGISTERS (K = k rounded up to a multiple of 4; unrolled, branch-free insertion) instead
// of a 12*k-byte LDS column per lane. At k = 20 the LDS columns allow two blocks per CU
// (two waves per SIMD) and the walk is a chain of dependent gathers: occupancy is what it
// needs. Slots beyond k only make the acceptance test slightly more generous.
// BUF > 0: accepted candidates are first pushed into a BUF-slot unsorted per-lane buffer; the
// sorted insertion (~11 instructions per list slot, executed by the whole wave as soon as ONE
// lane has a candidate to insert — which at 64 lanes is nearly every candidate) runs only when
// some lane's buffer is full, for all lanes and all their buffered candidates at once. The
// acceptance test then works with a slightly stale k-th distance (a superset is buffered);
// buffers are flushed before every "done" test, so the result is the same list. Measured on the
// 1 M-point forest, k = 20: see DESIGN.md (k_knn_reg).
// STRICT: the list is ordered by the distance ALONE (one fp64 compare per slot instead of two plus
// an index compare: 9 -> 7 vector instructions per slot, and the insertions are two thirds of this
// kernel: search 1.78 -> 1.25 ms per million points). Exactness is kept by detection, not by the
// comparison: equal distances INSIDE the list end up in arrival order and are put into index order
// by a pass at the end (a few instructions unless there are ties); a tie ACROSS the k-th place — a
// candidate dropped or evicted with the distance of the list's last entry — makes which index
// belongs to the result depend on what the comparison ignored, so that query is listed in
// `tie_list` and searched again by the exact variant (STRICT = false over `qlist`). Coordinates
// quantised to millimetres give a few per cent of such queries, a regular lattice nearly all
// (then the strict pass is wasted: 1.7x the exact kernel alone).
template <int K, int BUF, bool STRICT, class CO>
__global__ __launch_bounds__(256) void k_knn_reg(int n_query, KnnGrid g,
                                                 const int32_t* __restrict__ qlist /*sorted positions
                                                 to search, or null: all n_query*/,
                                                 const int32_t* __restrict__ qcount /*length of qlist,
                                                 on the device*/,
                                                 int q_min /*a list of at most this many is somebody
                                                 else's (k_knn_wave): nothing to do*/,
                                                 const int32_t* __restrict__ start,
                                                 const int32_t* __restrict__ order,
                                                 const int32_t* __restrict__ cell_of,
                                                 CO co, int k,
                                                 int exclude_self, int n_total, int last_level,
                                                 int32_t* __restrict__ out_idx,
                                                 double* __restrict__ out_d2,
                                                 int32_t* __restrict__ fail_list,
                                                 int32_t* __restrict__ fail_count,
                                                 int32_t* __restrict__ tie_list,
                                                 int32_t* __restrict__ tie_count) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  int p = gid;  // sorted position of this query
  if (qlist) {
    const int cnt = *qcount;
    if (cnt <= q_min || gid >= cnt) return;
    p = qlist[gid];
  } else if (p >= n_query) {
    return;
  }
  const int self = order[p];
  double x, y, z;
  co.get(p, x, y, z);
  const int c = cell_of[p];
  const int cx = c % g.nx, cy = (c / g.nx) % g.ny, cz = c / (g.nx * g.ny);
  double bd[K];
  int bi[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    bd[j] = __builtin_inf();
    bi[j] = 0x7FFFFFFF;
  }
  constexpr int NB = BUF > 0 ? BUF : 1;
  double fd[NB];  // buffered candidates, newest first; empty slots hold (inf, max)
  int fi[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    fd[j] = __builtin_inf();
    fi[j] = 0x7FFFFFFF;
  }
  int nbuf = 0;
  // STRICT: the smallest distance at which a candidate was dropped or evicted while equal to the
  // list's last entry; only if that is still the last entry's distance at the end does the result
  // depend on an index the comparison did not look at (earlier ties lie beyond the final k-th place)
  double tie_val = __builtin_inf();
  // sorted insertion of one candidate; (inf, max) is never smaller than a list entry: a no-op
  auto insert = [&](double d, int id) {
    if constexpr (STRICT) {
      const double last = bd[K - 1];
      bool lt_cur = d < last;
      const bool enters = lt_cur;
      tie_val = d == last && d < tie_val ? d : tie_val;  // dropped: as far as the list's last entry
#pragma unroll
      for (int t = K - 1; t > 0; --t) {
        const bool lt_prev = d < bd[t - 1];
        bd[t] = lt_prev ? bd[t - 1] : (lt_cur ? d : bd[t]);
        bi[t] = lt_prev ? bi[t - 1] : (lt_cur ? id : bi[t]);
        lt_cur = lt_prev;
      }
      bd[0] = lt_cur ? d : bd[0];
      bi[0] = lt_cur ? id : bi[0];
      tie_val = enters && last == bd[K - 1] && last < tie_val ? last : tie_val;  // evicted: as far as the new last
    } else {
      bool lt_cur = d < bd[K - 1] || (d == bd[K - 1] && id < bi[K - 1]);
#pragma unroll
      for (int t = K - 1; t > 0; --t) {
        const bool lt_prev = d < bd[t - 1] || (d == bd[t - 1] && id < bi[t - 1]);
        bd[t] = lt_prev ? bd[t - 1] : (lt_cur ? d : bd[t]);
        bi[t] = lt_prev ? bi[t - 1] : (lt_cur ? id : bi[t]);
        lt_cur = lt_prev;
      }
      bd[0] = lt_cur ? d : bd[0];
      bi[0] = lt_cur ? id : bi[0];
    }
  };
  auto flush = [&]() {
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      insert(fd[j], fi[j]);
      fd[j] = __builtin_inf();
      fi[j] = 0x7FFFFFFF;
    }
    nbuf = 0;
  };
  bool done = false;
  const int rmax_grid = max(g.nx, max(g.ny, g.nz));
  for (int r = 0; r <= kMaxRing && !done; ++r) {
    const int side = 2 * r + 1;
    for (int t = 0; t < side * side; ++t) {
      {
        // rows of the shell; for r = 1 nearest first — the centre row, the four rows that share a
        // face with it, the four corner rows (codes (dz+1)*3 + (dy+1), four bits each): the sooner
        // the list holds near points, the fewer of the later candidates pass the k-th-distance
        // test and have to be inserted. The result does not depend on the order.
        const int code = r == 1 ? int((0x862075134ull >> (4 * t)) & 15ull) : t;
        const int dz = code / side - r, dy = code % side - r;
        const int zz = cz + dz;
        if (zz < 0 || zz >= g.nz) continue;
        const int yy = cy + dy;
        if (yy < 0 || yy >= g.ny) continue;
        const int row = (zz * g.ny + yy) * g.nx;
        const bool full = (dz == -r || dz == r || dy == -r || dy == r);
        const int nseg = full ? 1 : (r > 0 ? 2 : 1);
        for (int s = 0; s < nseg; ++s) {
          int x0, x1;
          if (full) {
            x0 = cx - r;
            x1 = cx + r;
          } else {
            x0 = x1 = s == 0 ? cx - r : cx + r;
          }
          x0 = x0 < 0 ? 0 : x0;
          x1 = x1 >= g.nx ? g.nx - 1 : x1;
          if (x0 > x1) continue;
          const int qb = start[row + x0], qe = start[row + x1 + 1];
          for (int q = qb; q < qe; ++q) {
            if constexpr (BUF > 0) {
              // no early `continue`: every lane that is in this iteration reaches the ballot
              const double d = co.d2(q, x, y, z);
              bool acc = !(exclude_self && q == p) && (d < bd[K - 1] || d == bd[K - 1]);
              int id = 0x7FFFFFFF;
              if (acc) {
                id = order[q];
                if constexpr (!STRICT) acc = d < bd[K - 1] || (d == bd[K - 1] && id < bi[K - 1]);
              }
              if (acc) {
#pragma unroll
                for (int j = NB - 1; j > 0; --j) {  // push (static indices: registers, not scratch)
                  fd[j] = fd[j - 1];
                  fi[j] = fi[j - 1];
                }
                fd[0] = d;
                fi[0] = id;
                ++nbuf;
              }
              // one lane's buffer is full: EVERY lane of the iteration merges what it has
              if (__ballot(nbuf == NB) != 0ull) flush();
            } else {
              if (exclude_self && q == p) continue;
              const double d = co.d2(q, x, y, z);
              if (!(d < bd[K - 1] || d == bd[K - 1])) continue;  // cheap reject before the id load
              const int id = order[q];
              if (!(d < bd[K - 1] || (d == bd[K - 1] && id < bi[K - 1]))) continue;
              insert(d, id);
            }
          }
        }
      }
    }
    if constexpr (BUF > 0) flush();
    // everything outside the visited cube is at least r cells away
    double kth = __builtin_inf();
#pragma unroll
    for (int j = 0; j < K; ++j)
      if (j == k - 1) kth = bd[j];
    const double safe = double(r) * g.cell * 0.999999;
    if (kth <= safe * safe) done = true;
    if (r >= rmax_grid) done = true;  // the cube already covers the whole grid
  }
  bool tie = false;
  if constexpr (STRICT) {
    // a tie across the k-th place: with something outside the list (k = K) ...
    tie = k == K && tie_val == bd[K - 1] && tie_val < __builtin_inf();
    // ... or inside it (lists longer than k)
#pragma unroll
    for (int j = 1; j < K; ++j)
      if (j == k) tie |= bd[j] == bd[j - 1] && bd[j] < __builtin_inf();
    // equal distances inside the list: arrival order -> index order (bubble passes over the
    // indices of equal neighbours; no pass finds anything to do unless there are ties)
    for (int pass = 0; pass < K; ++pass) {
      bool sw = false;
#pragma unroll
      for (int t = 1; t < K; ++t) {
        const bool c = bd[t] == bd[t - 1] && bi[t] < bi[t - 1];
        const int lo = c ? bi[t] : bi[t - 1], hi = c ? bi[t - 1] : bi[t];
        bi[t - 1] = lo;
        bi[t] = hi;
        sw |= c;
      }
      if (__ballot(sw) == 0ull) break;
    }
  }
  // one atomic per wave for the queries that stay open (per lane it was ~10^4 atomics on one
  // address per million points)
  const bool open = !done && !last_level;
  const unsigned long long ob = __ballot(open);
  if (ob != 0) {
    const int lane = threadIdx.x & 63, lead = __ffsll(ob) - 1;
    int base = 0;
    if (lane == lead) base = atomicAdd(fail_count, __popcll(ob));
    base = __shfl(base, lead, 64);
    if (open) {
      fail_list[base + __popcll(ob & ((1ull << lane) - 1ull))] = self;
      return;
    }
  }
  if constexpr (STRICT) {  // the queries whose result hangs on a tie: again, by the exact variant
    const unsigned long long tb = __ballot(tie);
    if (tb != 0) {
      const int lane = threadIdx.x & 63, lead = __ffsll(tb) - 1;
      int base = 0;
      if (lane == lead) base = atomicAdd(tie_count, __popcll(tb));
      base = __shfl(base, lead, 64);
      if (tie) {
        tie_list[base + __popcll(tb & ((1ull << lane) - 1ull))] = p;
        return;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < K; ++j)
    if (j < k) {
      const bool have = bd[j] < __builtin_inf();
      out_idx[size_t(self) * k + j] = have ? bi[j] : n_total;
      if (out_d2) out_d2[size_t(self) * k + j] = bd[j];
    }
}

// Wave-per-query variant for the retry levels (k <= 64): there the cells are
// coarse and hold thousands of points, so the 64 lanes scan a run together.
// The sorted best-k list lives in registers, element j in lane j; an insertion
// is a ballot (position) plus one lane shift.
template <class CO>
__global__ __launch_bounds__(256) void k_knn_wave(int n_query,
                                                  const int32_t* __restrict__ n_ptr /*the number of
                                                  queries on the device, or null: n_query*/,
                                                  int n_max /*with n_ptr: more queries than this are
                                                  somebody else's (k_knn_reg over the list)*/,
                                                  const int32_t* __restrict__ query_list /*original
                                                  indices (pos_of given) or sorted positions*/,
                                                  const int32_t* __restrict__ pos_of, KnnGrid g,
                                                  const int32_t* __restrict__ start,
                                                  const int32_t* __restrict__ order,
                                                  const int32_t* __restrict__ cell_of,
                                                  CO co, int k,
                                                  int exclude_self, int n_total, int last_level,
                                                  int max_ring, int32_t* __restrict__ out_idx,
                                                  double* __restrict__ out_d2,
                                                  int32_t* __restrict__ fail_list,
                                                  int32_t* __restrict__ fail_count) {
  const int lane = threadIdx.x & 63;
  int nq = n_ptr ? *n_ptr : n_query;
  if (n_ptr && nq > n_max) nq = 0;
  const int wpb = int(blockDim.x) >> 6;  // waves per block
  for (int qi = blockIdx.x * wpb + (threadIdx.x >> 6); qi < nq; qi += gridDim.x * wpb) {  // whole waves
  const int p = query_list ? (pos_of ? pos_of[query_list[qi]] : query_list[qi]) : qi;
  const int self = order[p];
  double x, y, z;
  co.get(p, x, y, z);
  const int c = cell_of[p];
  const int cx = c % g.nx, cy = (c / g.nx) % g.ny, cz = c / (g.nx * g.ny);
  double bd = __builtin_inf();
  int bi = 0x7FFFFFFF;
  int have = 0;
  double tau_d = __builtin_inf();
  int tau_i = 0x7FFFFFFF;
  bool done = false;
  const int rmax_grid = max(g.nx, max(g.ny, g.nz));
  // A query clamped into the grid from far outside its box (a stray point; robust_box): everything
  // inside the box is further away than this level's rings reach, so the walk could only end on
  // other strays — it goes straight to the next level (in the end k_knn_brute) instead of scanning
  // the border cells' thousands of points.
  if (!last_level) {
    const double ox = fmax(fmax(g.minx - x, x - (g.minx + double(g.nx - 2) * g.cell)), 0.0);
    const double oy = fmax(fmax(g.miny - y, y - (g.miny + double(g.ny - 2) * g.cell)), 0.0);
    const double oz = fmax(fmax(g.minz - z, z - (g.minz + double(g.nz - 2) * g.cell)), 0.0);
    if (fmax(ox, fmax(oy, oz)) > double(max_ring) * g.cell) {
      if (lane == 0) fail_list[atomicAdd(fail_count, 1)] = self;
      continue;
    }
  }
  for (int r = 0; r <= max_ring && !done; ++r) {
    // The shell's row segments, 64 at a time: every lane looks one up (two loads), then the
    // wave scans the non-empty ones together. Around an isolated point nearly all of them
    // are empty, so a wide shell costs a few parallel lookups, not hundreds of serial ones.
    const int w = 2 * r + 1;
    const int nseg = 2 * w * w;  // two slots per row: [full row | -] or [left end | right end]
    for (int sbase = 0; sbase < nseg; sbase += 64) {
      const int sg = sbase + lane;
      int qb_l = 0, qe_l = 0;
      if (sg < nseg) {
        const int ri = sg >> 1, part = sg & 1;
        const int dz = ri / w - r, dy = ri % w - r;
        const int zz = cz + dz, yy = cy + dy;
        const bool full = (dz == -r || dz == r || dy == -r || dy == r);
        int x0 = 0, x1 = -1;
        if (full) {
          if (part == 0) {
            x0 = cx - r;
            x1 = cx + r;
          }
        } else if (r > 0) {
          x0 = x1 = part == 0 ? cx - r : cx + r;
        }
        x0 = x0 < 0 ? 0 : x0;
        x1 = x1 >= g.nx ? g.nx - 1 : x1;
        if (zz >= 0 && zz < g.nz && yy >= 0 && yy < g.ny && x0 <= x1) {
          const int row = (zz * g.ny + yy) * g.nx;
          qb_l = start[row + x0];
          qe_l = start[row + x1 + 1];
        }
      }
      unsigned long long segs = __ballot(qe_l > qb_l);
      while (segs) {
        const int sl = __ffsll(segs) - 1;
        segs &= segs - 1;
        const int qb = __shfl(qb_l, sl, 64), qe = __shfl(qe_l, sl, 64);
        for (int base = qb; base < qe; base += 64) {
          const int q = base + lane;
          const bool valid = q < qe && !(exclude_self && q == p);
          double d = __builtin_inf();
          int id = 0x7FFFFFFF;
          if (valid) {
            d = co.d2(q, x, y, z);
            id = order[q];
          }
          const bool cand = valid && (have < k || d < tau_d || (d == tau_d && id < tau_i));
          unsigned long long mask = __ballot(cand);
          while (mask) {
            const int l = __ffsll(mask) - 1;
            mask &= mask - 1;
            const double nd = __shfl(d, l, 64);
            const int ni = __shfl(id, l, 64);
            if (have == k && !(nd < tau_d || (nd == tau_d && ni < tau_i))) continue;
            const bool less = lane < have && (bd < nd || (bd == nd && bi < ni));
            const int pos = __popcll(__ballot(less));
            const double pd = __shfl_up(bd, 1, 64);
            const int pi = __shfl_up(bi, 1, 64);
            const int top = have < k ? have : k - 1;
            if (lane > pos && lane <= top) {
              bd = pd;
              bi = pi;
            }
            if (lane == pos) {
              bd = nd;
              bi = ni;
            }
            if (have < k) ++have;
            if (have == k) {
              tau_d = __shfl(bd, k - 1, 64);
              tau_i = __shfl(bi, k - 1, 64);
            }
          }
        }
      }
    }
    const double safe = double(r) * g.cell * 0.999999;
    if (have == k && tau_d <= safe * safe) done = true;
    if (r >= rmax_grid) done = true;
  }
  if (!done && !last_level) {
    if (lane == 0) fail_list[atomicAdd(fail_count, 1)] = self;
    continue;
  }
  if (lane < k) {
    out_idx[size_t(self) * k + lane] = lane < have ? bi : n_total;
    if (out_d2) out_d2[size_t(self) * k + lane] = lane < have ? bd : __builtin_inf();
  }
  }
}

// The last resort for a FEW isolated queries (stray points tens of metres outside the scan: their
// neighbours are further away than any affordable ring of cells, and every coarser retry level
// costs a grid build and a launch that lasts as long as its longest wave — 6-8 ms for a
// handful of them, 45 ms when the strays inflate the box until the grid hits its size cap): the
// whole cloud, same list, same comparison. A wave takes kBruteTile queries through one slice of
// the points (every loaded point is tested against all of them; the slices of one tile run on
// different waves, so that twenty queries still fill the chip), leaves its sorted partial lists in
// a scratch buffer, and k_knn_brute_merge folds a query's slices.
// queries it takes: what robust_box may leave outside its box. The cost is queries x points
// (1.4 ms for 2 000 of a million), the alternative a grid at its size cap (45 ms).
static int brute_max(int64_t n) { return int(std::min<int64_t>(8192, std::max<int64_t>(256, n / 256))); }
static constexpr int kBruteTile = 4;    // queries per wave

__device__ __forceinline__ void wave_list_insert(double nd, int ni, int k, int lane, double& bd, int& bi, int& have,
                                                 double& tau_d, int& tau_i) {
  if (have == k && !(nd < tau_d || (nd == tau_d && ni < tau_i))) return;
  const bool less = lane < have && (bd < nd || (bd == nd && bi < ni));
  const int pos = __popcll(__ballot(less));
  const double pd = __shfl_up(bd, 1, 64);
  const int pi = __shfl_up(bi, 1, 64);
  const int top = have < k ? have : k - 1;
  if (lane > pos && lane <= top) {
    bd = pd;
    bi = pi;
  }
  if (lane == pos) {
    bd = nd;
    bi = ni;
  }
  if (have < k) ++have;
  if (have == k) {
    tau_d = __shfl(bd, k - 1, 64);
    tau_i = __shfl(bi, k - 1, 64);
  }
}

__global__ __launch_bounds__(256) void k_knn_brute(int n_query, const int32_t* __restrict__ query_list,
                                                   const double* __restrict__ xyz, int n, int k,
                                                   int exclude_self, int n_slices,
                                                   double* __restrict__ part_d /*[tiles][slices][tile][k]*/,
                                                   int32_t* __restrict__ part_i) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);  // wave = (tile, slice)
  const int tile = w / n_slices, slice = w % n_slices;
  if (tile * kBruteTile >= n_query) return;  // whole waves
  int self[kBruteTile];
  double qx[kBruteTile], qy[kBruteTile], qz[kBruteTile];
  double bd[kBruteTile], tau_d[kBruteTile];
  int bi[kBruteTile], have[kBruteTile], tau_i[kBruteTile];
#pragma unroll
  for (int t = 0; t < kBruteTile; ++t) {
    const int qi = tile * kBruteTile + t;
    self[t] = qi < n_query ? query_list[qi] : -1;
    const size_t s0 = size_t(self[t] < 0 ? 0 : self[t]);
    qx[t] = xyz[3 * s0];
    qy[t] = xyz[3 * s0 + 1];
    qz[t] = xyz[3 * s0 + 2];
    bd[t] = tau_d[t] = __builtin_inf();
    bi[t] = tau_i[t] = 0x7FFFFFFF;
    have[t] = 0;
  }
  // slices of whole 64-point chunks
  const int chunks = (n + 63) / 64;
  const int per = (chunks + n_slices - 1) / n_slices;
  const int c_lo = slice * per, c_hi = min(chunks, c_lo + per);
  for (int ch = c_lo; ch < c_hi; ch += 2) {
    // two chunks' loads in flight before either is looked at
    double px[2], py[2], pz[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int q = (ch + u) * 64 + lane;
      const bool in = ch + u < c_hi && q < n;
      const size_t qq = size_t(in ? q : 0);
      px[u] = xyz[3 * qq];
      py[u] = xyz[3 * qq + 1];
      pz[u] = xyz[3 * qq + 2];
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int base = (ch + u) * 64;
      const int q = base + lane;
      const bool in = ch + u < c_hi && q < n;
#pragma unroll
      for (int t = 0; t < kBruteTile; ++t) {
        const bool valid = in && self[t] >= 0 && !(exclude_self && q == self[t]);
        const double d = valid ? sqdist3(qx[t], qy[t], qz[t], px[u], py[u], pz[u]) : __builtin_inf();
        const bool cand = valid && (have[t] < k || d < tau_d[t] || (d == tau_d[t] && q < tau_i[t]));
        unsigned long long mask = __ballot(cand);
        while (mask) {
          const int l = __ffsll(mask) - 1;
          mask &= mask - 1;
          wave_list_insert(__shfl(d, l, 64), base + l, k, lane, bd[t], bi[t], have[t], tau_d[t], tau_i[t]);
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < kBruteTile; ++t) {
    const size_t o = ((size_t(tile) * n_slices + slice) * kBruteTile + t) * size_t(k);
    if (lane < k) {
      part_d[o + lane] = lane < have[t] ? bd[t] : __builtin_inf();
      part_i[o + lane] = lane < have[t] ? bi[t] : 0x7FFFFFFF;
    }
  }
}

__global__ __launch_bounds__(256) void k_knn_brute_merge(int n_query, const int32_t* __restrict__ query_list,
                                                         int n, int k, int n_slices,
                                                         const double* __restrict__ part_d,
                                                         const int32_t* __restrict__ part_i,
                                                         int32_t* __restrict__ out_idx,
                                                         double* __restrict__ out_d2) {
  const int lane = threadIdx.x & 63;
  const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (qi >= n_query) return;
  const int self = query_list[qi];
  const int tile = qi / kBruteTile, t = qi % kBruteTile;
  double bd = __builtin_inf(), tau_d = __builtin_inf();
  int bi = 0x7FFFFFFF, tau_i = 0x7FFFFFFF, have = 0;
  // 64 / k slices per step, one entry per lane, the next step's loads issued before this step's
  // insertions (one slice at a time the loop was a chain of 256 memory round trips: 0.27 ms)
  const int per = 64 / k > 0 ? 64 / k : 1;
  const int sub = lane / k, e = lane % k;
  auto fetch = [&](int s0, double* d, int* id) {
    const int s = s0 + sub;
    const bool ok = sub < per && s < n_slices;
    const size_t o = ((size_t(tile) * n_slices + (ok ? s : 0)) * kBruteTile + t) * size_t(k) + e;
    *d = ok ? part_d[o] : __builtin_inf();
    *id = ok ? part_i[o] : 0x7FFFFFFF;
  };
  double dn;
  int idn;
  fetch(0, &dn, &idn);
  for (int s = 0; s < n_slices; s += per) {
    const double d = dn;
    const int id = idn;
    if (s + per < n_slices) fetch(s + per, &dn, &idn);
    const bool cand = id != 0x7FFFFFFF && (have < k || d < tau_d || (d == tau_d && id < tau_i));
    unsigned long long mask = __ballot(cand);
    while (mask) {
      const int l = __ffsll(mask) - 1;
      mask &= mask - 1;
      wave_list_insert(__shfl(d, l, 64), __shfl(id, l, 64), k, lane, bd, bi, have, tau_d, tau_i);
    }
  }
  if (lane < k) {
    out_idx[size_t(self) * k + lane] = lane < have ? bi : n;
    if (out_d2) out_d2[size_t(self) * k + lane] = lane < have ? bd : __builtin_inf();
  }
}

__global__ __launch_bounds__(256) void k_invert_order(int n, const int32_t* __restrict__ order,
                                                      int32_t* __restrict__ pos_of) {
  int p = blockIdx.x * 256 + threadIdx.x;
  if (p < n) pos_of[order[p]] = p;
}

// ---- the host side: switches, the kernel of a level, the steps of knn_device --------------------

struct KnnKnobs {
  // read once per process
  int buf;         // PYQSM_KNN_BUF=0: direct insertion (the round-1 kernel)
  bool strict;     // PYQSM_KNN_STRICT=0: the exact comparison in the first pass already
  double occ_div;  // PYQSM_KNN_OCC: points per occupied cell = k / this
  int wide;        // PYQSM_KNN_WIDE: shells a retry level may walk (kWideRing)
  // read on every call
  bool robust_box;  // PYQSM_KNN_ROBUST_BOX=0: grids over the full box
  bool trace;       // PYQSM_KNN_TRACE: what every level did, on stderr
};

static KnnKnobs read_knobs() {
  static const KnnKnobs once = [] {
    KnnKnobs kn{};
    const char* e = getenv("PYQSM_KNN_BUF");
    kn.buf = e ? atoi(e) : 4;
    e = getenv("PYQSM_KNN_STRICT");
    kn.strict = !(e && e[0] == '0');
    e = getenv("PYQSM_KNN_OCC");
    const double v = e ? atof(e) : 3.0;
    kn.occ_div = v > 0.25 && v < 64.0 ? v : 3.0;
    e = getenv("PYQSM_KNN_WIDE");
    kn.wide = e ? atoi(e) : kWideRing;
    return kn;
  }();
  KnnKnobs kn = once;
  const char* e = getenv("PYQSM_KNN_ROBUST_BOX");
  kn.robust_box = !(e && e[0] == '0');
  kn.trace = getenv("PYQSM_KNN_TRACE") != nullptr;
  return kn;
}

// The search kernel of one level: what the trace names and what is launched.
struct KnnKernel {
  enum Kind { Reg, Wave, Lds } kind;
  int width;  // Reg: the list length K; Lds: the block size T
  int buf;    // Reg: BUF
  bool strict;  // Reg: STRICT, followed by the two tie passes
};

static KnnKernel pick_kernel(int level, int k, const KnnKnobs& kn) {
  if (level == 0 && k <= 32) {
    // list length = k rounded up to a multiple of 4: every slot is ~11 instructions per
    // insertion, and slots beyond k loosen the acceptance test
    const int buf = kn.buf == 0 ? 0 : 4;
    return {KnnKernel::Reg, (k + 3) / 4 * 4, buf, buf != 0 && kn.strict};
  }
  if (level > 0 && k <= 64) return {KnnKernel::Wave, 0, 0, false};
  return {KnnKernel::Lds, k <= 48 ? 256 : k <= 96 ? 128 : 64, 0, false};
}

static std::string kernel_name(const KnnKernel& kk) {
  if (kk.kind == KnnKernel::Wave) return "k_knn_wave";
  char s[32];
  if (kk.kind == KnnKernel::Reg)
    snprintf(s, sizeof s, "k_knn_reg<%d,%d,%s>", kk.width, kk.buf, kk.strict ? "true" : "false");
  else
    snprintf(s, sizeof s, "k_knn<%d>", kk.width);
  return s;
}

// fn(std::integral_constant<int, W>) for the W among Ws that equals `width`; false: there is none.
template <int... Ws, class F>
static bool on_width(int width, F&& fn) {
  return ((width == Ws ? (fn(std::integral_constant<int, Ws>{}), true) : false) || ...);
}

// What every search launch of one level passes on: the grid, where the results go, and the list of
// the queries this level leaves open. Built once per level.
struct KnnArgs {
  KnnGrid g;
  const int32_t *start, *order, *cell_of;
  int k, exclude_self, n_total, last_level;
  int32_t* out_idx;
  double* out_d2;
  int32_t *fail_list, *fail_count;
};
static KnnArgs knn_args(const DevGrid& g, int k, int excl, int n_total, int last, int32_t* idx, double* d2,
                        int32_t* fail_list, int32_t* fail_count) {
  return KnnArgs{KnnGrid{g.nx, g.ny, g.nz, g.cell, g.minx, g.miny, g.minz}, g.start, g.order, g.cell_of, k, excl,
                 n_total, last, idx, d2, fail_list, fail_count};
}

template <class CO>
static void launch_wave(Ctx* c, unsigned blocks, const KnnArgs& a, CO co, int n_query, const int32_t* n_ptr, int n_max,
                        const int32_t* list, const int32_t* pos_of, int max_ring) {
  hipLaunchKernelGGL(k_knn_wave<CO>, dim3(blocks), dim3(256), 0, c->stream, n_query, n_ptr, n_max, list, pos_of, a.g,
                     a.start, a.order, a.cell_of, co, a.k, a.exclude_self, a.n_total, a.last_level, max_ring, a.out_idx,
                     a.out_d2, a.fail_list, a.fail_count);
}

// tie_list [n] / tie_count [1] (zeroed by the caller): scratch of the strict pass.
template <int K>
static int launch_knn_reg(Ctx* c, const KnnKernel& kk, const DevGrid& g, const KnnArgs& a, int n, int32_t* tie_list,
                          int32_t* tie_count) {
  const dim3 grid(ceil_div(n, 256)), blk(256);
  const int32_t* none = nullptr;
  bool known = true;
  on_coords(g, [&](auto co) {
    using CO = decltype(co);
    auto pass = [&](auto kernel, const int32_t* qlist, const int32_t* qcount, int q_min) {
      hipLaunchKernelGGL(kernel, grid, blk, 0, c->stream, n, a.g, qlist, qcount, q_min, a.start, a.order, a.cell_of, co,
                         a.k, a.exclude_self, a.n_total, a.last_level, a.out_idx, a.out_d2, a.fail_list, a.fail_count,
                         tie_list, tie_count);
    };
    if (kk.buf == 0 && !kk.strict) {
      pass(k_knn_reg<K, 0, false, CO>, none, none, 0);
    } else if (kk.buf == 4 && !kk.strict) {
      pass(k_knn_reg<K, 4, false, CO>, none, none, 0);
    } else if (kk.buf == 4) {
      pass(k_knn_reg<K, 4, true, CO>, none, none, 0);
      // The queries whose result hung on a tie, by the exact comparison: a WAVE per query (a lane per
      // query would be one long-running wave of 64 unrelated walks — 0.5 ms for 238 such queries of
      // a millimetre-quantised million points; this way they cost 20 us). Their number stays on the
      // device; the waves of a fixed grid stride over them. A cloud on a regular lattice ties nearly
      // everywhere (760 k of a million queries): past n / 16 the list goes to the per-lane kernel
      // with the exact comparison instead (both launches are issued, one of them finds nothing to do).
      const int many = n / 16;
      launch_wave(c, unsigned(std::min<int64_t>(ceil_div(n, 4), 8192)), a, co, n, tie_count, many, tie_list, none,
                  kMaxRing);
      pass(k_knn_reg<K, 4, false, CO>, tie_list, tie_count, many);
    } else {
      known = false;  // no such instantiation: pick_kernel and this table disagree
    }
  });
  return known ? 0 : fail(PYQSM_EINVAL, "knn: no kernel %s", kernel_name(kk).c_str());
}

template <int T>
static int launch_lds(Ctx* c, const DevGrid& g, const KnnArgs& a, int n_query, const int32_t* list,
                      const int32_t* pos_of) {
  const size_t smem = size_t(a.k) * T * 12;
  static std::atomic<uint64_t> attr_set{0};  // one bit per device (the attribute is per device)
  const uint64_t bit = 1ull << (c->device & 63);
  if (!(attr_set.load(std::memory_order_acquire) & bit)) {
    PQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_knn<T, CoordsF64>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    PQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_knn<T, CoordsF32>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set.fetch_or(bit, std::memory_order_release);
  }
  on_coords(g, [&](auto co) {
    hipLaunchKernelGGL((k_knn<T, decltype(co)>), dim3(ceil_div(n_query, T)), dim3(T), smem, c->stream, n_query, list,
                       pos_of, a.g, a.start, a.order, a.cell_of, co, a.k, a.exclude_self, a.n_total, a.last_level,
                       a.out_idx, a.out_d2, a.fail_list, a.fail_count);
  });
  return 0;
}

// The queries: every point in sorted order (list null: level 0), or the n_query original indices in
// `list`, whose sorted positions pos_of gives.
static int launch_kernel(Ctx* c, const KnnKernel& kk, const DevGrid& g, const KnnArgs& a, int n_query,
                         const int32_t* list, const int32_t* pos_of, int ring, int32_t* tie_list, int32_t* tie_count) {
  bool known = true;
  int rc = 0;
  switch (kk.kind) {
    case KnnKernel::Reg:
      known = on_width<4, 8, 12, 16, 20, 24, 28, 32>(kk.width, [&](auto w) {
        rc = launch_knn_reg<decltype(w)::value>(c, kk, g, a, n_query, tie_list, tie_count);
      });
      break;
    case KnnKernel::Wave:
      // (one or two waves per block instead of four: no difference — the launch lasts as long as its
      // longest waves, 0.34 ms for the forest's 9 864 outliers)
      on_coords(g, [&](auto co) {
        launch_wave(c, unsigned(ceil_div(n_query, 4)), a, co, n_query, nullptr, 0, list, pos_of, ring);
      });
      break;
    case KnnKernel::Lds:
      known = on_width<256, 128, 64>(
          kk.width, [&](auto w) { rc = launch_lds<decltype(w)::value>(c, g, a, n_query, list, pos_of); });
      break;
  }
  if (!known) return fail(PYQSM_EINVAL, "knn: no kernel %s", kernel_name(kk).c_str());
  PQ_TRY(rc);
  PQ_HIP(hipGetLastError());
  return 0;
}

// One level's search: the kernel picked once, named in the trace and launched. `made`: how the grid
// came about, if not planned for level 0 (trace only).
static int search_level(Ctx* c, const KnnKnobs& kn, int level, const DevGrid& g, const char* made, const KnnArgs& a,
                        int n_query, const int32_t* list, const int32_t* pos_of, int ring, int32_t* tie_list,
                        int32_t* tie_count) {
  const KnnKernel kk = pick_kernel(level, a.k, kn);
  if (kn.trace)  // printed for the last level too (knn_device's own lines are not)
    fprintf(stderr, "knn level %d: grid %d x %d x %d of cell %.4g%s, %s, %s, %d queries%s\n", level, g.nx, g.ny, g.nz,
            g.cell, made, g.p4 ? "fp32 records" : "fp64 arrays", kernel_name(kk).c_str(), n_query,
            a.last_level ? ", last level" : "");
  ProfScope ps(c, level == 0 ? "knn_search" : "knn_retry");
  return launch_kernel(c, kk, g, a, n_query, list, pos_of, ring, tie_list, tie_count);
}

// ---- level-0 cell edge: aim at ~k/3 points per occupied cell -----------
// Two count-only probes on coarse grids give the local density and how it
// scales with the edge (exponent ~2 for surfaces, ~3 for volumes); the edge
// for the target occupancy follows by extrapolation, and one corrective
// rebuild is allowed if the sorted grid misses the target by more than 2.5x.
static constexpr int64_t kMaxCells = int64_t(1) << 28;
struct KnnPlan {
  DevGrid g;             // the grid of the level at hand
  double box[6];         // what every grid of the call is built over
  bool all_f32 = false;  // every coordinate fp32-representable: the grids keep 16-byte fp32 records
};
static int plan_level0_grid(Ctx* c, const double* xyz, int64_t n, int k, const KnnKnobs& kn, KnnPlan* p) {
  ProfScope ps(c, "knn_bin");
  double* box = p->box;
  PQ_TRY(cloud_bbox(c, xyz, n, box, box + 3, &p->all_f32));
  // grids over the cloud without its sparse tails; what is given up is what k_knn_brute can take
  if (kn.robust_box && k <= 64) {
    int64_t outside = 0;
    PQ_TRY(robust_box(c, xyz, n, brute_max(n), box, &outside));
    if (outside && kn.trace)
      fprintf(stderr, "knn: grids over the box without its tails, at most %lld points outside\n", (long long)outside);
  }
  double ext = std::max(box[3] - box[0], std::max(box[4] - box[1], box[5] - box[2]));
  if (!(ext > 0)) ext = 1.0;
  const double target = std::max(2.0, double(k) / kn.occ_div);
  double c1, per1, c2, per2, dim = 2.0, cell;
  PQ_TRY(probe_occupancy(c, xyz, n, box, ext / 64.0, &c1, &per1));
  if (per1 <= 1.5 * target) {
    cell = c1 * (per1 < 0.5 * target ? 2.0 : 1.0);
  } else {
    PQ_TRY(probe_occupancy(c, xyz, n, box, c1 * 0.5, &c2, &per2));
    if (c2 < c1 && per2 > 0) dim = std::log2(std::max(per1 / per2, 1.0001)) / std::log2(c1 / c2);
    dim = std::min(3.0, std::max(1.0, dim));
    cell = c2 * std::pow(target / per2, 1.0 / dim);
  }
  cell = std::max(cell, ext / 4096.0);
  for (int it = 0; it < 2; ++it) {
    PQ_TRY(build_grid(c, xyz, n, cell, kMaxCells, &p->g, box, p->all_f32));
    if (it == 1) break;
    int64_t occ = 0;
    PQ_TRY(count_occupied(c, p->g, &occ));
    const double per = double(n) / double(occ > 0 ? occ : 1);
    if (per <= 2.5 * target && per >= 0.4 * target) break;
    if (per < target && p->g.nx <= 3 && p->g.ny <= 3 && p->g.nz <= 3) break;  // cannot coarsen further
    const double f = std::min(4.0, std::max(0.25, std::pow(target / per, 1.0 / dim)));
    if (f < 1.0 && p->g.cell > cell * 1.0000001) break;  // grid already at its size cap
    cell = p->g.cell * f;
  }
  return 0;
}

// A few isolated queries (`list`, original indices), one by one over the whole cloud.
static int brute_rest(Ctx* c, const double* xyz, int n, int k, int exclude_self, const int32_t* list, int n_query,
                      int32_t* idx, double* d2) {
  ProfScope pb(c, "knn_brute");
  const int tiles = ceil_div(n_query, kBruteTile);
  const int chunks = ceil_div(n, 64);
  // ~16 waves per CU over all tiles; a slice is at least 32 chunks long
  const int n_slices = std::max(1, std::min(std::min(256, ceil_div(chunks, 32)), ceil_div(c->cu_count * 16, tiles)));
  double* part_d = nullptr;
  int32_t* part_i = nullptr;
  const size_t slots = size_t(tiles) * n_slices * kBruteTile * size_t(k);
  PQ_TRY(c->arena.get(slots, &part_d));
  PQ_TRY(c->arena.get(slots, &part_i));
  hipLaunchKernelGGL(k_knn_brute, dim3(ceil_div(tiles * n_slices, 4)), dim3(256), 0, c->stream, n_query, list, xyz, n,
                     k, exclude_self, n_slices, part_d, part_i);
  hipLaunchKernelGGL(k_knn_brute_merge, dim3(ceil_div(n_query, 4)), dim3(256), 0, c->stream, n_query, list, n, k,
                     n_slices, static_cast<const double*>(part_d), static_cast<const int32_t*>(part_i), idx, d2);
  PQ_HIP(hipGetLastError());
  return 0;
}

// p->g = the grid of the next level, cells 4x larger; *made = how (trace only). pos_of (or null: the
// next level serves every point again) = the new grid's order, inverted.
static int next_grid(Ctx* c, const double* xyz, int64_t n, KnnPlan* p, const char** made, int32_t* pos_of) {
  ProfScope ps(c, "knn_bin");
  // Deriving the coarse grid from the fine one reads the fine grid's whole cell array (95 M
  // cells for a million points at k = 20: 0.22 ms); binning the points again at the coarse edge
  // touches 1.5 M cells (0.12 ms). The order inside a cell does not matter to a search. Small
  // fine grids (the later levels) keep the pyramid: no atomics, a few microseconds.
  DevGrid coarse;
  if (p->g.ncell > (int64_t(1) << 22)) {
    PQ_TRY(build_grid(c, xyz, n, p->g.cell * 4.0, kMaxCells, &coarse, p->box, p->all_f32));
    *made = " binned again";
  } else {
    PQ_TRY(coarsen_grid(c, p->g, n, 4, &coarse));
    *made = " coarsened";
  }
  p->g = coarse;
  if (pos_of) {
    hipLaunchKernelGGL(k_invert_order, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, int(n), p->g.order, pos_of);
    PQ_HIP(hipGetLastError());
  }
  return 0;
}

int knn_device(Ctx* c, const double* xyz, int64_t n, int32_t k, int32_t exclude_self,
               int32_t* idx, double* d2) {
  if (k <= 0 || k > kKnnMaxK) return fail(PYQSM_ERANGE, "k must be in [1, %d]", kKnnMaxK);
  if (n == 0) return 0;
  const int N = int(n);
  const KnnKnobs kn = read_knobs();
  KnnPlan plan;
  PQ_TRY(plan_level0_grid(c, xyz, n, k, kn, &plan));
  const DevGrid& g = plan.g;
  int32_t *pos_of = nullptr, *fail_a, *fail_b, *fail_count, *tie_list, *tie_count;
  PQ_TRY(c->arena.get(size_t(n), &fail_a));
  PQ_TRY(c->arena.get(size_t(n), &fail_b));
  PQ_TRY(c->arena.get(1, &fail_count));
  PQ_TRY(c->arena.get(size_t(n), &tie_list));
  PQ_TRY(c->arena.get(1, &tie_count));
  PQ_HIP(hipMemsetAsync(tie_count, 0, 4, c->stream));
  int n_query = N;
  const int32_t* list = nullptr;  // the queries of a retry level (original indices); null: every point
  const char* made = "";
  bool first_pass_again = false;  // level 0 has been run a second time (see below)
  for (int level = 0;;) {
    const int ring = level >= 1 && k <= 64 ? kn.wide : kMaxRing;
    const int last = (g.nx - 2 <= ring && g.ny - 2 <= ring && g.nz - 2 <= ring) ? 1 : 0;
    int32_t* open = (level & 1) ? fail_b : fail_a;  // the queries this level leaves open
    PQ_HIP(hipMemsetAsync(fail_count, 0, 4, c->stream));
    PQ_TRY(search_level(c, kn, level, g, made, knn_args(g, k, exclude_self, N, last, idx, d2, open, fail_count),
                        n_query, list, pos_of, ring, tie_list, tie_count));
    if (last) break;
    int32_t nf = 0;
    PQ_TRY(fetch(c, &nf, fail_count));
    if (kn.trace) {
      if (level == 0) {
        int32_t nt = 0;
        PQ_HIP(hipMemcpy(&nt, tie_count, 4, hipMemcpyDeviceToHost));
        fprintf(stderr, "knn level 0: %d queries searched again for a tie at the k-th place\n", nt);
      }
      fprintf(stderr, "knn level %d: %d of %d queries stay open (cell %.4g)\n", level, nf, n_query, g.cell);
    }
    if (nf == 0) break;
    if (level >= 1 && nf <= 2 * brute_max(n) && k <= 64) {
      PQ_TRY(brute_rest(c, xyz, N, k, exclude_self, open, nf, idx, d2));
      if (kn.trace) fprintf(stderr, "knn: %d isolated queries searched over the whole cloud\n", nf);
      break;
    }
    // More than half of ALL queries open after the register kernel's three rings: the occupancy the
    // cell edge was planned for came from coincident points (a contracted cloud, a lattice with several
    // points per node: 5.5 per node meet k / 3 at any edge below the lattice step), so the edge says
    // nothing about the spacing, level 0 answered (nearly) nobody, and a WAVE per query would now serve
    // the whole cloud. Level 0 once more instead, a lane per query with its tie passes, on the
    // coarser grid; what is still open after that is retried as usual.
    if (level == 0 && k <= 32 && !first_pass_again && nf > N / 2) {
      PQ_TRY(next_grid(c, xyz, n, &plan, &made, nullptr));
      if (kn.trace) fprintf(stderr, "knn: level 0 once more for every query, on the coarser grid\n");
      first_pass_again = true;
      PQ_HIP(hipMemsetAsync(tie_count, 0, 4, c->stream));
      continue;
    }
    // retry the stragglers on a 4x coarser grid
    if (!pos_of) PQ_TRY(c->arena.get(size_t(n), &pos_of));
    PQ_TRY(next_grid(c, xyz, n, &plan, &made, pos_of));
    list = open;
    n_query = nf;
    ++level;
  }
  return 0;
}

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_knn_dev(const double* xyz_dev, int64_t n, int32_t k, int32_t exclude_self,
                  int32_t* idx_dev, double* d2_dev, int32_t device) {
  PQ_API_RANGE("pyqsm_knn_dev");
  if (n < 0) return fail(PYQSM_EINVAL, "negative size");
  if (n > 0 && (!xyz_dev || !idx_dev || !d2_dev))
    return fail(PYQSM_EINVAL, "pyqsm_knn_dev: NULL pointer");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  ProfScope ps(c, "knn_total");
  return knn_device(c, xyz_dev, n, k, exclude_self, idx_dev, d2_dev);
}

int pyqsm_knn(const double* xyz, int64_t n, int32_t k, int32_t exclude_self, int32_t* idx,
              double* d2, int32_t device) {
  PQ_API_RANGE("pyqsm_knn");
  if (n < 0) return fail(PYQSM_EINVAL, "negative size");
  if (n == 0) return 0;
  if (!xyz || !idx || !d2) return fail(PYQSM_EINVAL, "pyqsm_knn: NULL pointer");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double *d_xyz, *d_d2;
  int32_t* d_idx;
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_xyz));
  PQ_TRY(c->arena.get(size_t(n) * size_t(k > 0 ? k : 1), &d_idx));
  PQ_TRY(c->arena.get(size_t(n) * size_t(k > 0 ? k : 1), &d_d2));
  PQ_TRY(copy_in(c, d_xyz, xyz, size_t(n) * 3));
  PQ_TRY(knn_device(c, d_xyz, n, k, exclude_self, d_idx, d_d2));
  PQ_TRY(download(c, idx, d_idx, size_t(n) * k));
  PQ_TRY(download(c, d2, d_d2, size_t(n) * k));
  PQ_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

}  // extern "C"
