// adjacency.hip — which clusters touch, how closely and at how many point pairs, on gfx950.
//
//   pyqsm_cluster_adjacency   for labelled source and target points, every (source cluster a, target
//                       cluster b) with at least one point pair within `threshold`: the minimum
//                       squared distance, the number of point pairs within the threshold and, on
//                       request, the closest point pair. What the loop of
//                       tree_i.sparse_distance_matrix(tree_j, threshold)['v'].min() over all cluster
//                       pairs computes at pyQSM/cluster_joining.py:139-155 (determine_adjacency),
//                       in one grid pass over all points instead of S x T KD-tree pair queries.
// The targets are binned into cells of edge `threshold` (grid.hpp: radius_grid); one lane per source
// point, served in cell order, walks its 27 cells. A pair counts when d2 <= threshold * threshold
// (inclusive, like cKDTree), d2 = ((dx*dx)+dy*dy)+dz*dz in fp64. Results meet in a dense S x T table
// of 16-byte entries {~bits(min d2), pairs}: a 64-bit unsigned atomicMax on the complemented bit
// pattern (non-negative doubles order as their bit patterns, so the maximum of the complement is the
// minimum distance, and a table cleared to zero is an empty table: one memset) and a 64-bit integer
// atomicAdd, both on the same 16 bytes. Integer min and add commute: the table does not depend on
// the order in which the lanes arrive. A lane keeps the last kAdjCache target clusters it met in
// registers, so a run of candidates of one cluster costs one pair of atomics, not one per point pair.
#include "grid.hpp"

#include <algorithm>
#include <cmath>

namespace pyqsm {

static constexpr int kAdjCache = 4;                    // target clusters a lane accumulates in registers
static constexpr int64_t kAdjMaxTable = int64_t(1) << 26;  // S x T entries per call (1 GiB of table)

__global__ __launch_bounds__(256) void k_adj_sorted_labels(int m, const int32_t* __restrict__ order,
                                                           const int32_t* __restrict__ lab,
                                                           int32_t* __restrict__ out) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q < m) out[q] = lab[order[q]];
}

struct AdjEntry {
  unsigned long long inv_min;  // ~bits of the smallest d2 (0: no pair yet)
  unsigned long long pairs;
};

__device__ __forceinline__ void adj_flush(AdjEntry* __restrict__ table, size_t row, int b, unsigned long long bits,
                                          unsigned cnt) {
  AdjEntry* e = table + row + size_t(b);
  atomicMax(&e->inv_min, ~bits);
  atomicAdd(&e->pairs, (unsigned long long)cnt);
}

// SAME: sources and targets are one labelled cloud; a pair is taken from the side of the smaller
// label only (b > a), so every unordered point pair is seen once and equal labels cost no distance.
// CACHE false: every pair within the threshold goes to the table at once (the tool's comparison).
// stats (may be null): [0] += distance tests, [1] += pairs of atomics issued.
template <class CO, bool SAME, bool CACHE>
__global__ __launch_bounds__(256) void k_adj_accumulate(int n, const double* __restrict__ src,
                                                        const int32_t* __restrict__ slab,
                                                        const int32_t* __restrict__ perm /*may be null*/, GridParams g,
                                                        const int32_t* __restrict__ start,
                                                        const int32_t* __restrict__ tlab /*sorted order*/, CO co,
                                                        double r2, int T, AdjEntry* __restrict__ table,
                                                        unsigned long long* __restrict__ stats) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= n) return;
  const int i = perm ? perm[gid] : gid;
  const int a = slab[i];
  if (a < 0) return;
  const double x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
  const size_t row = size_t(a) * size_t(T);
  int c_lab[kAdjCache];
  unsigned long long c_min[kAdjCache];
  unsigned c_cnt[kAdjCache];
#pragma unroll
  for (int k = 0; k < kAdjCache; ++k) {
    c_lab[k] = -1;
    c_min[k] = 0;
    c_cnt[k] = 0;
  }
  int victim = 0;
  unsigned long long tests = 0, flushes = 0;
  int cx, cy, cz;
  clamped_cell(g, x, y, z, &cx, &cy, &cz);
  for (int dz = -1; dz <= 1; ++dz) {
    const int zz = cz + dz;
    if (zz < 0 || zz >= g.nz) continue;
    for (int dy = -1; dy <= 1; ++dy) {
      const int yy = cy + dy;
      if (yy < 0 || yy >= g.ny) continue;
      const int x0 = cx - 1 < 0 ? 0 : cx - 1, x1 = cx + 1 >= g.nx ? g.nx - 1 : cx + 1;
      const int cell_row = (zz * g.ny + yy) * g.nx;
      for (int q = start[cell_row + x0]; q < start[cell_row + x1 + 1]; ++q) {
        const int b = tlab[q];
        if (b < 0 || (SAME && b <= a)) continue;
        const double d = co.d2(q, x, y, z);
        ++tests;
        if (!(d <= r2)) continue;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(d);
        if (!CACHE) {
          adj_flush(table, row, b, bits, 1u);
          ++flushes;
          continue;
        }
        bool hit = false;
#pragma unroll
        for (int k = 0; k < kAdjCache; ++k)
          if (c_lab[k] == b) {
            c_min[k] = bits < c_min[k] ? bits : c_min[k];
            ++c_cnt[k];
            hit = true;
          }
        if (hit) continue;
        int v_lab = -1;
        unsigned long long v_min = 0;
        unsigned v_cnt = 0;
#pragma unroll
        for (int k = 0; k < kAdjCache; ++k)
          if (k == victim) {
            v_lab = c_lab[k];
            v_min = c_min[k];
            v_cnt = c_cnt[k];
            c_lab[k] = b;
            c_min[k] = bits;
            c_cnt[k] = 1;
          }
        victim = victim + 1 == kAdjCache ? 0 : victim + 1;
        if (v_lab >= 0) {
          adj_flush(table, row, v_lab, v_min, v_cnt);
          ++flushes;
        }
      }
    }
  }
  if (CACHE) {
#pragma unroll
    for (int k = 0; k < kAdjCache; ++k)
      if (c_lab[k] >= 0) {
        adj_flush(table, row, c_lab[k], c_min[k], c_cnt[k]);
        ++flushes;
      }
  }
  if (stats) {
    atomicAdd(&stats[0], tests);
    atomicAdd(&stats[1], flushes);
  }
}

// The closest point pair of every table entry: a second walk that compares d2 with the entry's final
// minimum and keeps the smallest (source index << 32 | target index) among the pairs that attain it,
// so ties go to the smallest source index, then the smallest target index. wit is preset to all ones.
template <class CO, bool SAME>
__global__ __launch_bounds__(256) void k_adj_witness(int n, const double* __restrict__ src,
                                                     const int32_t* __restrict__ slab,
                                                     const int32_t* __restrict__ perm, GridParams g,
                                                     const int32_t* __restrict__ start,
                                                     const int32_t* __restrict__ order,
                                                     const int32_t* __restrict__ tlab, CO co, double r2, int T,
                                                     const AdjEntry* __restrict__ table,
                                                     unsigned long long* __restrict__ wit) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= n) return;
  const int i = perm ? perm[gid] : gid;
  const int a = slab[i];
  if (a < 0) return;
  const double x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
  const size_t row = size_t(a) * size_t(T);
  int last = -1;                    // the target cluster whose minimum the lane holds
  unsigned long long last_min = 0;
  int cx, cy, cz;
  clamped_cell(g, x, y, z, &cx, &cy, &cz);
  for (int dz = -1; dz <= 1; ++dz) {
    const int zz = cz + dz;
    if (zz < 0 || zz >= g.nz) continue;
    for (int dy = -1; dy <= 1; ++dy) {
      const int yy = cy + dy;
      if (yy < 0 || yy >= g.ny) continue;
      const int x0 = cx - 1 < 0 ? 0 : cx - 1, x1 = cx + 1 >= g.nx ? g.nx - 1 : cx + 1;
      const int cell_row = (zz * g.ny + yy) * g.nx;
      for (int q = start[cell_row + x0]; q < start[cell_row + x1 + 1]; ++q) {
        const int b = tlab[q];
        if (b < 0 || (SAME && b <= a)) continue;
        const double d = co.d2(q, x, y, z);
        if (!(d <= r2)) continue;
        if (b != last) {
          last = b;
          last_min = ~table[row + size_t(b)].inv_min;
        }
        if ((unsigned long long)__double_as_longlong(d) == last_min)
          atomicMin(&wit[row + size_t(b)], ((unsigned long long)(unsigned)i << 32) | (unsigned)order[q]);
      }
    }
  }
}

// flags [entries + 1] for the scan: 1 where the entry holds a pair
__global__ __launch_bounds__(256) void k_adj_flags(int64_t entries, const AdjEntry* __restrict__ table,
                                                   int32_t* __restrict__ flags) {
  const int64_t e = blockIdx.x * int64_t(256) + threadIdx.x;
  if (e > entries) return;
  flags[e] = e < entries && table[e].pairs != 0;
}

// the non-empty entries in ascending (a, b), at most `cap` of them (pos = the scanned flags)
__global__ __launch_bounds__(256) void k_adj_rows(int64_t entries, int T, const int32_t* __restrict__ pos,
                                                  const AdjEntry* __restrict__ table,
                                                  const unsigned long long* __restrict__ wit /*may be null*/,
                                                  int64_t cap, int32_t* __restrict__ a, int32_t* __restrict__ b,
                                                  double* __restrict__ min_d2, int64_t* __restrict__ pairs,
                                                  int64_t* __restrict__ src_idx, int64_t* __restrict__ tgt_idx) {
  const int64_t e = blockIdx.x * int64_t(256) + threadIdx.x;
  if (e >= entries) return;
  const int64_t p = pos[e];
  if (pos[e + 1] == p || p >= cap) return;
  const AdjEntry t = table[e];
  a[p] = int32_t(e / T);
  b[p] = int32_t(e % T);
  min_d2[p] = __longlong_as_double((long long)~t.inv_min);
  pairs[p] = int64_t(t.pairs);
  if (wit) {
    const unsigned long long w = wit[e];
    src_idx[p] = int64_t(w >> 32);
    tgt_idx[p] = int64_t(w & 0xFFFFFFFFull);
  }
}

// Host-side screening of one side's input: PYQSM_EINVAL on a non-finite coordinate of a labelled
// point's cloud or a label >= n_labels; *any = some label is >= 0.
static int adj_screen(const char* side, const double* xyz, const int32_t* lab, int64_t n, int32_t n_labels,
                      bool* any) {
  *any = false;
  for (int64_t i = 0; i < n; ++i) {
    if (lab[i] >= n_labels) return fail(PYQSM_EINVAL, "%s label %d outside [0, %d)", side, lab[i], n_labels);
    if (lab[i] >= 0) *any = true;
    if (!std::isfinite(xyz[3 * i]) || !std::isfinite(xyz[3 * i + 1]) || !std::isfinite(xyz[3 * i + 2]))
      return fail(PYQSM_EINVAL, "point coordinates must be finite");
  }
  return 0;
}

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_cluster_adjacency(const double* src, const int32_t* src_label, int64_t n, int32_t n_src_labels,
                            const double* tgt, const int32_t* tgt_label, int64_t m, int32_t n_tgt_labels,
                            double threshold, int32_t flags, int64_t capacity, int32_t* a, int32_t* b,
                            double* min_d2, int64_t* pairs, int64_t* src_idx, int64_t* tgt_idx, int64_t* count,
                            int64_t* stats, int32_t device) {
  PQ_API_RANGE("pyqsm_cluster_adjacency");
  const bool same = (flags & PYQSM_ADJ_SAME_CLOUD) != 0, witness = (flags & PYQSM_ADJ_WITNESS) != 0;
  const bool cache = (flags & PYQSM_ADJ_NO_CACHE) == 0;
  if (flags & ~(PYQSM_ADJ_SAME_CLOUD | PYQSM_ADJ_WITNESS | PYQSM_ADJ_NO_CACHE))
    return fail(PYQSM_EINVAL, "pyqsm_cluster_adjacency: unknown flag");
  if (!count) return fail(PYQSM_EINVAL, "pyqsm_cluster_adjacency: NULL pointer");
  *count = 0;
  if (stats) stats[0] = stats[1] = 0;
  if (same) {
    tgt = src;
    tgt_label = src_label;
    m = n;
    n_tgt_labels = n_src_labels;
  }
  if (n < 0 || m < 0 || capacity < 0 || n_src_labels < 0 || n_tgt_labels < 0)
    return fail(PYQSM_EINVAL, "negative size");
  if (!(threshold > 0) || !std::isfinite(threshold)) return fail(PYQSM_EINVAL, "threshold must be positive");
  if ((n > 0 && (!src || !src_label)) || (m > 0 && (!tgt || !tgt_label)))
    return fail(PYQSM_EINVAL, "pyqsm_cluster_adjacency: NULL pointer");
  if (capacity > 0 && (!a || !b || !min_d2 || !pairs || (witness && (!src_idx || !tgt_idx))))
    return fail(PYQSM_EINVAL, "pyqsm_cluster_adjacency: NULL pointer");
  bool any_src = false, any_tgt = false;
  PQ_TRY(adj_screen("source", src, src_label, n, n_src_labels, &any_src));
  if (same)
    any_tgt = any_src;
  else
    PQ_TRY(adj_screen("target", tgt, tgt_label, m, n_tgt_labels, &any_tgt));
  if (!any_src || !any_tgt) return 0;  // nothing labelled on one side: no pair, no device
  if (n > 0x7FFFFF00LL || m > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 points per call");
  const int64_t entries = int64_t(n_src_labels) * int64_t(n_tgt_labels);
  if (entries > kAdjMaxTable)
    return fail(PYQSM_ERANGE, "%d x %d cluster pairs exceed the table of 2^26 entries: split the sources by label",
                n_src_labels, n_tgt_labels);
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  const int64_t cap = std::min(capacity, entries);
  double *d_src, *d_tgt, *d_min;
  int32_t *d_slab, *d_tlab, *d_tlab_sorted, *d_flags, *d_a, *d_b;
  int64_t *d_pairs, *d_si = nullptr, *d_ti = nullptr;
  AdjEntry* d_table;
  unsigned long long *d_wit = nullptr, *d_stats = nullptr;
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_src));
  PQ_TRY(c->arena.get(size_t(n), &d_slab));
  PQ_TRY(copy_in(c, d_src, src, size_t(n) * 3));
  PQ_TRY(copy_in(c, d_slab, src_label, size_t(n)));
  if (same) {
    d_tgt = d_src;
    d_tlab = d_slab;
  } else {
    PQ_TRY(c->arena.get(size_t(m) * 3, &d_tgt));
    PQ_TRY(c->arena.get(size_t(m), &d_tlab));
    PQ_TRY(copy_in(c, d_tgt, tgt, size_t(m) * 3));
    PQ_TRY(copy_in(c, d_tlab, tgt_label, size_t(m)));
  }
  PQ_TRY(c->arena.get(size_t(m), &d_tlab_sorted));
  PQ_TRY(c->arena.get(size_t(entries), &d_table));
  PQ_TRY(c->arena.get(size_t(entries) + 1, &d_flags));
  PQ_TRY(c->arena.get(size_t(cap) + 1, &d_a));
  PQ_TRY(c->arena.get(size_t(cap) + 1, &d_b));
  PQ_TRY(c->arena.get(size_t(cap) + 1, &d_min));
  PQ_TRY(c->arena.get(size_t(cap) + 1, &d_pairs));
  if (witness) {
    PQ_TRY(c->arena.get(size_t(entries), &d_wit));
    PQ_TRY(c->arena.get(size_t(cap) + 1, &d_si));
    PQ_TRY(c->arena.get(size_t(cap) + 1, &d_ti));
  }
  if (stats) {
    PQ_TRY(c->arena.get(2, &d_stats));
    PQ_HIP(hipMemsetAsync(d_stats, 0, 16, c->stream));
  }
  DevGrid g;
  PQ_TRY(radius_grid(c, d_tgt, m, threshold, &g));
  const GridParams rg = grid_params(g);
  const double r2 = threshold * threshold;
  const int T = n_tgt_labels;
  {
    ProfScope ps(c, "cluster_adjacency");
    hipLaunchKernelGGL(k_adj_sorted_labels, dim3(ceil_div(m, 256)), dim3(256), 0, c->stream, int(m), g.order, d_tlab,
                       d_tlab_sorted);
    PQ_HIP(hipGetLastError());
    PQ_HIP(hipMemsetAsync(d_table, 0, size_t(entries) * sizeof(AdjEntry), c->stream));
    int32_t* perm = nullptr;
    PQ_TRY(query_order(c, d_src, n, rg, g.ncell, &perm));
    const dim3 blocks(ceil_div(n, 256));
    on_coords(g, [&](auto co) {
      using CO = decltype(co);
      auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, blocks, dim3(256), 0, c->stream, int(n), d_src, d_slab,
                           static_cast<const int32_t*>(perm), rg, g.start, d_tlab_sorted, co, r2, T, d_table, d_stats);
      };
      if (same && cache) go(k_adj_accumulate<CO, true, true>);
      if (same && !cache) go(k_adj_accumulate<CO, true, false>);
      if (!same && cache) go(k_adj_accumulate<CO, false, true>);
      if (!same && !cache) go(k_adj_accumulate<CO, false, false>);
    });
    PQ_HIP(hipGetLastError());
    if (witness) {
      ProfScope pw(c, "cluster_adjacency_witness");
      PQ_HIP(hipMemsetAsync(d_wit, 0xFF, size_t(entries) * 8, c->stream));
      on_coords(g, [&](auto co) {
        using CO = decltype(co);
        auto go = [&](auto kern) {
          hipLaunchKernelGGL(kern, blocks, dim3(256), 0, c->stream, int(n), d_src, d_slab,
                             static_cast<const int32_t*>(perm), rg, g.start, g.order, d_tlab_sorted, co, r2, T,
                             static_cast<const AdjEntry*>(d_table), d_wit);
        };
        if (same) go(k_adj_witness<CO, true>);
        else go(k_adj_witness<CO, false>);
      });
      PQ_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_adj_flags, dim3(ceil_div(entries + 1, 256)), dim3(256), 0, c->stream, entries,
                       static_cast<const AdjEntry*>(d_table), d_flags);
    PQ_HIP(hipGetLastError());
    PQ_TRY(exclusive_scan_i32(c, d_flags, entries + 1));
    if (cap > 0) {
      hipLaunchKernelGGL(k_adj_rows, dim3(ceil_div(entries, 256)), dim3(256), 0, c->stream, entries, T,
                         static_cast<const int32_t*>(d_flags), static_cast<const AdjEntry*>(d_table),
                         static_cast<const unsigned long long*>(d_wit), cap, d_a, d_b, d_min, d_pairs, d_si, d_ti);
      PQ_HIP(hipGetLastError());
    }
  }
  int32_t total = 0;
  PQ_TRY(download(c, &total, d_flags + entries, 1));
  if (stats) PQ_TRY(download(c, reinterpret_cast<unsigned long long*>(stats), d_stats, 2));
  PQ_HIP(hipStreamSynchronize(c->stream));
  const size_t rows = size_t(std::min<int64_t>(total, cap));
  if (rows) {
    PQ_TRY(download(c, a, d_a, rows));
    PQ_TRY(download(c, b, d_b, rows));
    PQ_TRY(download(c, min_d2, d_min, rows));
    PQ_TRY(download(c, pairs, d_pairs, rows));
    if (witness) {
      PQ_TRY(download(c, src_idx, d_si, rows));
      PQ_TRY(download(c, tgt_idx, d_ti, rows));
    }
    PQ_HIP(hipStreamSynchronize(c->stream));
  }
  *count = total;
  return 0;
}

}  // extern "C"
