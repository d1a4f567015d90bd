// grow.hip — region growing of seed clusters through a cloud, all cycles in HBM (SURVEY.md §8f
// rank 2): the loop of pyQSM/tree_isolation.py:98-262 (extend_seed_clusters, order_cutoff=None).
//
//   pyqsm_grow_clusters   Every cycle, every frontier point of every cluster that is still growing
//                         selects its (at most k nearest) source points within the radius — the rule
//                         of pyqsm_radius_mark, through the same walk (radius_walk.hpp). A free point
//                         goes to the smallest cluster index that selected it; what a cluster acquired
//                         is its next frontier; a cluster that acquired fewer than min_new points
//                         stops.
//
// The source, its grid, the ownership, the candidate words, the cycle stamps and the frontier stay
// on the device for the whole call; per cycle the host reads back one 64-bit word (the new
// frontier's size and how many of its points belong to clusters that go on) and launches:
//   grow_walk      one lane per frontier point: integer atomicMin of its cluster index into the
//                  candidate word of every selected point that is still free
//   grow_commit    one streaming pass over the points: candidate -> owner, cycle stamp, flag; new
//                  points per cluster counted with one integer atomicAdd per wave and cluster
//   grow_frontier  compact_flagged: the flagged positions, ascending — the next frontier, already in
//                  the order of the grid's cells; then one block that settles which clusters go on
// Everything lives in SORTED position space (the grid's cell order) and is scattered back through
// the grid's order array once at the end, so the walk gathers no order[q].
// Integer min / add atomics only, and no output depends on their arrival order: the minimum is
// order-free, the selection of a query depends on the grid alone, and the order of the frontier
// changes nothing but the order in which its points are served.
#include "radius_walk.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace pyqsm {

static constexpr int32_t kNoCand = 0x7FFFFFFF;  // above every cluster index

// owner in sorted position space; no candidate, no cycle yet
__global__ __launch_bounds__(256) void k_grow_init(int64_t n, const int32_t* __restrict__ order,
                                                   const int32_t* __restrict__ owner_in,
                                                   int32_t* __restrict__ owner, int32_t* __restrict__ cand,
                                                   int32_t* __restrict__ cycle) {
  const int64_t q = blockIdx.x * int64_t(256) + threadIdx.x;
  if (q >= n) return;
  owner[q] = owner_in[order[q]];
  cand[q] = kNoCand;
  cycle[q] = -1;
}

// Cycle 0: the frontier is the seed points themselves (coordinates that need not be source points).
template <class CO>
__global__ __launch_bounds__(256) void k_grow_walk_seeds(int m, const double* __restrict__ qry,
                                                         const int32_t* __restrict__ qlab,
                                                         const int32_t* __restrict__ perm /*may be null*/,
                                                         GridParams g, const int32_t* __restrict__ start, CO co,
                                                         double r2, int k, const int32_t* __restrict__ active,
                                                         const int32_t* __restrict__ owner,
                                                         int32_t* __restrict__ cand) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= m) return;
  const int i = perm ? perm[gid] : gid;
  const int lab = qlab[i];
  if (!active[lab]) return;
  const double x = qry[3 * i], y = qry[3 * i + 1], z = qry[3 * i + 2];
  (void)radius_select(g, start, co, x, y, z, r2, k, FreeMinSink{owner, cand, lab});
}

// Cycles >= 1: the frontier is a list of sorted positions, ascending; a point's cluster is its owner.
template <class CO>
__global__ __launch_bounds__(256) void k_grow_walk(int m, const int64_t* __restrict__ front, GridParams g,
                                                   const int32_t* __restrict__ start, CO co, double r2, int k,
                                                   const int32_t* __restrict__ active,
                                                   const int32_t* __restrict__ owner, int32_t* __restrict__ cand) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= m) return;
  const int q0 = int(front[gid]);
  const int lab = owner[q0];
  if (!active[lab]) return;  // its cluster has stopped
  double x, y, z;
  co.get(q0, x, y, z);
  (void)radius_select(g, start, co, x, y, z, r2, k, FreeMinSink{owner, cand, lab});
}

// n + 1 threads: flags[n] = 0 for compact_flagged. No early return: every lane takes part in the
// ballots.
__global__ __launch_bounds__(256) void k_grow_commit(int64_t n, int cyc, int32_t* __restrict__ cand,
                                                     int32_t* __restrict__ owner, int32_t* __restrict__ cycle,
                                                     int32_t* __restrict__ flags, int32_t* __restrict__ newcount) {
  const int64_t q = blockIdx.x * int64_t(256) + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int c = q < n ? cand[q] : kNoCand;
  const bool take = c != kNoCand;
  if (q <= n) flags[q] = take;
  if (take) {
    owner[q] = c;
    cycle[q] = cyc;
    cand[q] = kNoCand;
  }
  // one atomicAdd per wave and cluster: neighbours in cell order mostly share theirs
  unsigned long long left = __ballot(take);
  while (left) {
    const int leader = __ffsll(left) - 1;
    const int lc = __shfl(c, leader, 64);
    const unsigned long long same = __ballot(take && c == lc);
    if (lane == leader) atomicAdd(&newcount[lc], __popcll(same));
    left &= ~same;
  }
}

// One block. A cluster that was growing in cycle `cyc` and acquired fewer than min_new points
// stops (finished = the cycles it queried in); *rec = (new frontier's size << 32) | the frontier
// points of clusters that go on.
__global__ __launch_bounds__(256) void k_grow_settle(int n_clusters, int cyc, int min_new,
                                                     const int32_t* __restrict__ flags_n,
                                                     int32_t* __restrict__ active, int32_t* __restrict__ newcount,
                                                     int32_t* __restrict__ finished,
                                                     unsigned long long* __restrict__ rec) {
  __shared__ unsigned int served;
  if (threadIdx.x == 0) served = 0;
  __syncthreads();
  unsigned int mine = 0;
  for (int i = threadIdx.x; i < n_clusters; i += 256) {
    if (!active[i]) continue;
    const int cnt = newcount[i];
    newcount[i] = 0;
    if (cnt < min_new) {
      active[i] = 0;
      finished[i] = cyc + 1;
    } else {
      mine += unsigned(cnt);
    }
  }
  if (mine) atomicAdd(&served, mine);
  __syncthreads();
  if (threadIdx.x == 0) *rec = (uint64_t(uint32_t(*flags_n)) << 32) | served;
}

__global__ __launch_bounds__(256) void k_grow_scatter(int64_t n, const int32_t* __restrict__ order,
                                                      const int32_t* __restrict__ owner,
                                                      const int32_t* __restrict__ cycle,
                                                      int32_t* __restrict__ owner_out,
                                                      int32_t* __restrict__ cycle_out) {
  const int64_t q = blockIdx.x * int64_t(256) + threadIdx.x;
  if (q >= n) return;
  const int i = order[q];
  owner_out[i] = owner[q];
  cycle_out[i] = cycle[q];
}

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_grow_clusters(const double* src, int64_t n, const int32_t* owner_in, const double* seed_xyz,
                        const int32_t* seed_label, int64_t m, int32_t n_clusters, double radius, int32_t k_cap,
                        int32_t cycles, int32_t min_new, int32_t* owner_out, int32_t* cycle_out, int32_t* finished,
                        int64_t* stats, int32_t device) {
  PQ_API_RANGE("pyqsm_grow_clusters");
  if (n < 0 || m < 0 || n_clusters < 0) return fail(PYQSM_EINVAL, "negative size");
  if (n > 0 && (!src || !owner_in || !owner_out || !cycle_out))
    return fail(PYQSM_EINVAL, "pyqsm_grow_clusters: NULL pointer");
  if (m > 0 && (!seed_xyz || !seed_label)) return fail(PYQSM_EINVAL, "pyqsm_grow_clusters: NULL pointer");
  if (n_clusters > 0 && !finished) return fail(PYQSM_EINVAL, "pyqsm_grow_clusters: NULL pointer");
  if (!(radius > 0) || !std::isfinite(radius)) return fail(PYQSM_EINVAL, "radius must be positive");
  if (k_cap <= 0) return fail(PYQSM_EINVAL, "k must be positive");
  if (min_new < 1) return fail(PYQSM_EINVAL, "min_new must be at least 1");
  if (cycles < 0) return fail(PYQSM_EINVAL, "cycles must not be negative");
  if (n > 0x7FFFFF00LL || m > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 points per call");
  for (int64_t i = 0; i < n; ++i)
    if (owner_in[i] < -1 || owner_in[i] >= n_clusters)
      return fail(PYQSM_EINVAL, "owner_in[%lld] = %d is outside [-1, %d)", (long long)i, int(owner_in[i]),
                  int(n_clusters));
  std::vector<int32_t> active(size_t(n_clusters), 0);  // clusters with a seed point
  for (int64_t i = 0; i < m; ++i) {
    if (seed_label[i] < 0 || seed_label[i] >= n_clusters)
      return fail(PYQSM_EINVAL, "seed_label[%lld] = %d is outside [0, %d)", (long long)i, int(seed_label[i]),
                  int(n_clusters));
    active[size_t(seed_label[i])] = 1;
  }
  int64_t st[4] = {0, 0, 0, 0};  // cycles run, frontier queries served, points acquired, largest frontier
  if (n == 0 || m == 0 || cycles == 0) {
    // Nothing to walk. An empty source still answers the seeds' one cycle: nothing within reach.
    const bool one = m > 0 && cycles > 0;
    for (int64_t i = 0; i < n; ++i) {
      owner_out[i] = owner_in[i];
      cycle_out[i] = -1;
    }
    for (int32_t i = 0; i < n_clusters; ++i) finished[i] = active[size_t(i)] ? (one ? 1 : -1) : 0;
    if (one) {
      st[0] = 1;
      st[1] = st[3] = m;
    }
    if (stats) memcpy(stats, st, sizeof st);
    return 0;
  }
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double *d_src, *d_qry;
  int32_t *d_io, *d_qlab, *d_owner, *d_cand, *d_cycle, *d_flags, *d_active, *d_newcount, *d_finished;
  int64_t* d_front;
  unsigned long long* d_rec;
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_src));
  PQ_TRY(c->arena.get(size_t(m) * 3, &d_qry));
  PQ_TRY(c->arena.get(size_t(m), &d_qlab));
  PQ_TRY(c->arena.get(size_t(n) * 2, &d_io));  // owner_in on the way in; owner_out, cycle_out on the way out
  PQ_TRY(c->arena.get(size_t(n), &d_owner));
  PQ_TRY(c->arena.get(size_t(n), &d_cand));
  PQ_TRY(c->arena.get(size_t(n), &d_cycle));
  PQ_TRY(c->arena.get(size_t(n) + 1, &d_flags));
  PQ_TRY(c->arena.get(size_t(n), &d_front));
  PQ_TRY(c->arena.get(size_t(n_clusters), &d_active));
  PQ_TRY(c->arena.get(size_t(n_clusters), &d_newcount));
  PQ_TRY(c->arena.get(size_t(n_clusters), &d_finished));
  PQ_TRY(c->arena.get(1, &d_rec));
  PQ_TRY(copy_in(c, d_src, src, size_t(n) * 3));
  PQ_TRY(copy_in(c, d_qry, seed_xyz, size_t(m) * 3));
  PQ_TRY(copy_in(c, d_qlab, seed_label, size_t(m)));
  PQ_TRY(copy_in(c, d_io, owner_in, size_t(n)));
  PQ_TRY(copy_in(c, d_active, active.data(), size_t(n_clusters)));
  PQ_HIP(hipMemsetAsync(d_newcount, 0, size_t(n_clusters) * 4, c->stream));
  for (int32_t i = 0; i < n_clusters; ++i) finished[i] = active[size_t(i)] ? -1 : 0;
  PQ_TRY(copy_in(c, d_finished, finished, size_t(n_clusters)));
  DevGrid g;
  PQ_TRY(radius_grid(c, d_src, n, radius, &g));
  const GridParams rg = grid_params(g);
  const double r2 = radius * radius;
  hipLaunchKernelGGL(k_grow_init, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, n, g.order,
                     static_cast<const int32_t*>(d_io), d_owner, d_cand, d_cycle);
  PQ_HIP(hipGetLastError());
  int32_t* perm = nullptr;  // the seeds in cell order; later frontiers are born in it
  PQ_TRY(query_order(c, d_qry, m, rg, g.ncell, &perm));
  {
    // the scratch of compact_flagged's scan: taken once, handed back, so that the loop's
    // mark / rewind finds it in place and allocates nothing
    const Arena::Mark mk = c->arena.mark();
    int32_t* scratch;
    PQ_TRY(c->arena.get(size_t(n) / 1024 + 4096, &scratch));
    c->arena.rewind(mk);
  }
  int64_t fsize = m, served = m;
  for (int32_t cyc = 0; cyc < cycles && served > 0; ++cyc) {
    {
      ProfScope ps(c, "grow_walk");
      on_coords(g, [&](auto co) {
        if (cyc == 0)
          hipLaunchKernelGGL(k_grow_walk_seeds<decltype(co)>, dim3(ceil_div(fsize, 256)), dim3(256), 0, c->stream,
                             int(fsize), static_cast<const double*>(d_qry), static_cast<const int32_t*>(d_qlab),
                             static_cast<const int32_t*>(perm), rg, static_cast<const int32_t*>(g.start), co, r2,
                             k_cap, static_cast<const int32_t*>(d_active), static_cast<const int32_t*>(d_owner),
                             d_cand);
        else
          hipLaunchKernelGGL(k_grow_walk<decltype(co)>, dim3(ceil_div(fsize, 256)), dim3(256), 0, c->stream,
                             int(fsize), static_cast<const int64_t*>(d_front), rg,
                             static_cast<const int32_t*>(g.start), co, r2, k_cap,
                             static_cast<const int32_t*>(d_active), static_cast<const int32_t*>(d_owner), d_cand);
      });
      PQ_HIP(hipGetLastError());
    }
    {
      ProfScope ps(c, "grow_commit");
      hipLaunchKernelGGL(k_grow_commit, dim3(ceil_div(n + 1, 256)), dim3(256), 0, c->stream, n, int(cyc), d_cand,
                         d_owner, d_cycle, d_flags, d_newcount);
      PQ_HIP(hipGetLastError());
    }
    {
      ProfScope ps(c, "grow_frontier");
      const Arena::Mark mk = c->arena.mark();
      const int r = compact_flagged(c, d_flags, n, d_front);
      c->arena.rewind(mk);
      PQ_TRY(r);
      hipLaunchKernelGGL(k_grow_settle, dim3(1), dim3(256), 0, c->stream, int(n_clusters), int(cyc), int(min_new),
                         static_cast<const int32_t*>(d_flags + n), d_active, d_newcount, d_finished, d_rec);
      PQ_HIP(hipGetLastError());
    }
    unsigned long long rec = 0;  // the cycle's one read-back
    PQ_TRY(fetch(c, &rec, d_rec));
    st[0] += 1;
    st[1] += served;
    st[3] = std::max(st[3], served);
    fsize = int64_t(rec >> 32);
    served = int64_t(rec & 0xFFFFFFFFull);
    st[2] += fsize;
  }
  hipLaunchKernelGGL(k_grow_scatter, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, n, g.order,
                     static_cast<const int32_t*>(d_owner), static_cast<const int32_t*>(d_cycle), d_io, d_io + n);
  PQ_HIP(hipGetLastError());
  PQ_TRY(download(c, owner_out, d_io, size_t(n)));
  PQ_TRY(download(c, cycle_out, d_io + n, size_t(n)));
  PQ_TRY(download(c, finished, d_finished, size_t(n_clusters)));
  PQ_HIP(hipStreamSynchronize(c->stream));
  if (stats) memcpy(stats, st, sizeof st);
  return 0;
}

}  // extern "C"
