// grid.hip — bounding box, cell counting sort (see grid.hpp).
#include "grid.hpp"

#include "block_scan.hpp"

#include <atomic>
#include <cmath>
#include <type_traits>

namespace pyqsm {

// Order-preserving map double -> uint64 so that atomicMin/atomicMax work.
__device__ __forceinline__ unsigned long long ord_key(double x) {
  unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(x));
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ static inline double ord_val(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  double d;
  memcpy(&d, &b, 8);
  return d;
}

// ---- the shape rules every planner of a grid shares -----------------------------------------------
static constexpr int kBkMax = 16384;  // buckets (LDS histogram of the two-level sort's A passes: <= 64 KB)

// The two-level sort's buckets for a directory of ncell + 1 entries: 2^12 cells each, 2^13 beyond
// kBkMax of those; nbk = ceil((ncell + 1) / bucket). More than kBkMax buckets: no two-level sort.
struct BucketShape {
  int bits;
  int64_t nbk;
};
__host__ __device__ static inline BucketShape bucket_shape(int64_t ncell) {
  const int bits = ncell + 1 <= (int64_t(kBkMax) << 12) ? 12 : 13;
  return BucketShape{bits, (ncell + (int64_t(1) << bits)) >> bits};
}

// Interior slabs per axis of a grid of edge `cell` over the box [mn, mx] (raw[a]; 0 from the first
// axis on that has 2e9 or more) and *tot = the cells of that grid with `border` more slabs per axis,
// as a double. One function for the host and the device: where both plan the same box they do the
// same fp64 operations in the same order, and every point lands in the same cell.
__host__ __device__ static inline bool interior_slabs(const double* mn, const double* mx, double cell, double border,
                                                      int raw[3], double* tot) {
  bool ok = true;
  double t = 1.0;
  for (int a = 0; a < 3; ++a) {
    const double d = floor((mx[a] - mn[a]) / cell) + 1.0;
    if (!(d < 2.0e9)) ok = false;
    raw[a] = ok ? int(d) : 0;
    t *= d + border;
  }
  *tot = t;
  return ok;
}

// Stage 1: one (min, max) record per block, no atomics (94 k same-address atomics
// cost 0.56 ms in the first version of this kernel). Stage 2: one block folds the
// records.
// part[block][7]: min keys, max keys, and 1 if every coordinate the block saw is exactly
// representable in fp32 (double(float(v)) == v: true for PCD / LAS derived clouds), else 0.
// The kernel also clears `zero_n` ints for the caller, every block a slice (the bucket counters of the
// binning that follows: two memset launches less on the critical path; the one-block fold did it until it
// left DBSCAN's speculated step).
static constexpr int kBoxVals = 7;
// Two blocks per compute unit at most, 512 records on a MI355X: every block of k_bk_hist folds them all. (Four,
// as it was while one block folded: k_bbox 9.3 us instead of 8.4 on the 1 M-point forest, and k_bk_hist 0.8 us
// longer. A thread taking two or four points per sweep, their loads issued together: 7.9 and 8.2 us, less
// than the 1.5 us the launch varies by from step to step: not kept. profiles/plan_fold_bbox_variants.txt)
static int bbox_blocks(const Ctx* c, int64_t n) {
  return int(std::min<int64_t>(ceil_div(n, 256), int64_t(c->cu_count) * 2));
}
__global__ __launch_bounds__(256) void k_bbox(const double* __restrict__ xyz, int64_t n,
                                              unsigned long long* __restrict__ part /*[grid][7]*/,
                                              int32_t* __restrict__ zero_buf, int zero_n,
    unsigned long long* __restrict__ st /*stamps or null*/) {
  __shared__ unsigned long long red[4][6];
  __shared__ int red_f32[4];
  stamped(st, [&] {
  unsigned long long mn[3] = {~0ull, ~0ull, ~0ull}, mx[3] = {0, 0, 0};
  bool f32ok = true;
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += stride) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double v = xyz[3 * i + a];
      f32ok = f32ok && double(float(v)) == v;
      unsigned long long k = ord_key(v);
      mn[a] = k < mn[a] ? k : mn[a];
      mx[a] = k > mx[a] ? k : mx[a];
    }
  }
  for (int64_t q = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; q < zero_n; q += stride) zero_buf[q] = 0;
  const bool wave_ok = __all(f32ok);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      unsigned long long o1 = __shfl_down(mn[a], off, 64), o2 = __shfl_down(mx[a], off, 64);
      mn[a] = o1 < mn[a] ? o1 : mn[a];
      mx[a] = o2 > mx[a] ? o2 : mx[a];
    }
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      red[w][a] = mn[a];
      red[w][3 + a] = mx[a];
    }
    red_f32[w] = wave_ok;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    unsigned long long v = red[0][threadIdx.x];
    for (int q = 1; q < 4; ++q) {
      const unsigned long long o = red[q][threadIdx.x];
      v = threadIdx.x < 3 ? (o < v ? o : v) : (o > v ? o : v);
    }
    part[size_t(blockIdx.x) * kBoxVals + threadIdx.x] = v;
  }
  if (threadIdx.x == 6)
    part[size_t(blockIdx.x) * kBoxVals + 6] = (red_f32[0] && red_f32[1] && red_f32[2] && red_f32[3]) ? 1ull : 0ull;
  });
}

// (Folding in k_bbox itself — the block that counts itself last reads everybody's records — was tried
// in round 3 to save this launch: the agent-scope release every block needs before it counts itself
// writes its XCD's L2 back, and the binning went from 0.135 to 0.20 ms. DBSCAN's speculated step has no
// fold launch all the same: every block of k_bk_hist folds the records for itself, behind the kernel
// boundary, with no ticket and no fence: fold_box_records below.)
// One block folds the per-block records (the fp32 flag as a minimum: 0 wins).
// With `plan` (DBSCAN without a hint), the fold also writes the grid plan of edge `cell` (see
// plan_grid_device), and the same plan to `host` (host-mapped, coherent) with the sequence number `seq`
// stored last.
struct PlanIn {
  double cell;
  int64_t max_cells;
  PlanHint hint;
  GridPlan* host;
  unsigned seq;
};
__device__ GridPlan make_plan(const unsigned long long* box, const PlanIn& in);
__device__ void store_plan(GridPlan p, const PlanIn& in, GridPlan* __restrict__ plan);

// The records folded by a block of 256 threads into fin[kBoxVals] (shared), which the whole block may read
// on return. Minima and maxima: every block that folds the same records gets the same box, whatever
// the order. A thread issues the loads of two records, fourteen, before it waits for the first.
__device__ __forceinline__ void fold_box_records(const unsigned long long* __restrict__ part, int nblk,
                                                 unsigned long long (*red)[kBoxVals] /*[4], shared*/,
                                                 unsigned long long* fin /*[kBoxVals], shared*/) {
  const auto fold = [](int a, unsigned long long o, unsigned long long v) {
    return (a < 3 || a == 6) ? (o < v ? o : v) : (o > v ? o : v);
  };
  unsigned long long v[kBoxVals] = {~0ull, ~0ull, ~0ull, 0, 0, 0, ~0ull};
  for (int b0 = threadIdx.x; b0 < nblk; b0 += 512) {
    unsigned long long o[2][kBoxVals];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int b = b0 + 256 * u < nblk ? b0 + 256 * u : nblk - 1;  // (past the end: the last record twice)
#pragma unroll
      for (int a = 0; a < kBoxVals; ++a) o[u][a] = part[size_t(b) * kBoxVals + a];
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int a = 0; a < kBoxVals; ++a) v[a] = fold(a, o[u][a], v[a]);
  }
#pragma unroll
  for (int a = 0; a < kBoxVals; ++a)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[a] = fold(a, __shfl_down(v[a], off, 64), v[a]);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int a = 0; a < kBoxVals; ++a) red[threadIdx.x >> 6][a] = v[a];
  __syncthreads();
  if (threadIdx.x < kBoxVals) {
    unsigned long long r = red[0][threadIdx.x];
    for (int q = 1; q < 4; ++q) r = fold(int(threadIdx.x), red[q][threadIdx.x], r);
    fin[threadIdx.x] = r;
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void k_bbox_fold(const unsigned long long* __restrict__ part,
                                                   int nblk, unsigned long long* __restrict__ out,
                                                   PlanIn pin, GridPlan* __restrict__ plan) {
  __shared__ unsigned long long red[4][kBoxVals];
  __shared__ unsigned long long fin[kBoxVals];
  fold_box_records(part, nblk, red, fin);
  if (threadIdx.x < kBoxVals) out[threadIdx.x] = fin[threadIdx.x];
  if (plan && threadIdx.x == 0) store_plan(make_plan(fin, pin), pin, plan);  // (plan: kernel-uniform)
}

__global__ __launch_bounds__(256) void k_cell_count(const double* __restrict__ xyz, int64_t n,
                                                    GridParams g, int32_t* __restrict__ counts,
                                                    int32_t* __restrict__ cell_tmp,
                                                    int32_t* __restrict__ rank_tmp,
                                                    int32_t* __restrict__ occ_part /*[gridDim.x]*/) {
  __shared__ int wfirst[4];
  int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  bool first = false;
  if (i < n) {
    int c = cell_index(g, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    cell_tmp[i] = c;
    const int rank = atomicAdd(&counts[c], 1);
    rank_tmp[i] = rank;
    first = rank == 0;  // exactly one point per occupied cell sees an empty counter
  }
  const unsigned long long b = __ballot(first);
  if ((threadIdx.x & 63) == 0) wfirst[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) occ_part[blockIdx.x] = (wfirst[0] + wfirst[1]) + (wfirst[2] + wfirst[3]);
}

__global__ __launch_bounds__(256) void k_cell_scatter(const double* __restrict__ xyz, int64_t n,
                                                      const int32_t* __restrict__ start,
                                                      const int32_t* __restrict__ cell_tmp,
                                                      const int32_t* __restrict__ rank_tmp,
                                                      int32_t* __restrict__ order,
                                                      int32_t* __restrict__ cell_of,
                                                      double* __restrict__ sx,
                                                      double* __restrict__ sy,
                                                      double* __restrict__ sz) {
  const SortedStore out{order, cell_of, nullptr, nullptr, sx, sy, sz};
  int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (i >= n) return;
  int c = cell_tmp[i];
  out.put(start[c] + rank_tmp[i], int32_t(i), c, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
}

// wave sums -> one atomic per block (atomics on one address are served one at a time)
__device__ __forceinline__ void block_add_i32(int32_t local, int32_t* out) {
  __shared__ int32_t wsum[4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int32_t t = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    if (t) atomicAdd(out, t);
  }
}

__global__ __launch_bounds__(256) void k_count_occupied(const int32_t* __restrict__ start,
                                                        int64_t ncell, int32_t* __restrict__ out) {
  int32_t local = 0;
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < ncell;
       i += int64_t(gridDim.x) * blockDim.x)
    local += start[i + 1] > start[i];
  block_add_i32(local, out);
}

__global__ __launch_bounds__(256) void k_probe_count(const double* __restrict__ xyz, int64_t n,
                                                     GridParams g, int32_t* __restrict__ counts) {
  int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (i >= n) return;
  // only "occupied or not" is read afterwards: a plain store of 1 (racing stores of the same
  // value) instead of a counter — hundreds of points share a probe cell, and atomics on one
  // address are served one at a time
  counts[cell_index(g, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2])] = 1;
}

__global__ __launch_bounds__(256) void k_count_nonzero(const int32_t* __restrict__ counts,
                                                       int64_t ncell, int32_t* __restrict__ out) {
  int32_t local = 0;
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < ncell;
       i += int64_t(gridDim.x) * blockDim.x)
    local += counts[i] > 0;
  block_add_i32(local, out);
}

int probe_occupancy(Ctx* c, const double* xyz, int64_t n, const double box[6], double cell,
                    double* cell_used, double* per_cell) {
  int dims[3];
  for (;;) {
    double tot = 1.0;
    for (int a = 0; a < 3; ++a) {
      double d = std::floor((box[3 + a] - box[a]) / cell) + 3.0;
      dims[a] = d < 2.0e9 ? int(d) : 0x7FFFFFFF;
      tot *= d;
    }
    if (tot <= double(int64_t(1) << 22)) break;
    cell *= 2.0;
  }
  const int64_t ncell = int64_t(dims[0]) * dims[1] * dims[2];
  int32_t* counts;
  PQ_TRY(c->arena.get(size_t(ncell) + 1, &counts));
  PQ_HIP(hipMemsetAsync(counts, 0, (size_t(ncell) + 1) * 4, c->stream));
  GridParams gp{box[0], box[1], box[2], 1.0 / cell, dims[0], dims[1], dims[2]};
  hipLaunchKernelGGL(k_probe_count, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, xyz, n, gp,
                     counts);
  const int blocks = int(std::min<int64_t>(ceil_div(ncell, 256), int64_t(c->cu_count) * 8));
  hipLaunchKernelGGL(k_count_nonzero, dim3(blocks), dim3(256), 0, c->stream, counts, ncell,
                     counts + ncell);
  PQ_HIP(hipGetLastError());
  int32_t occ = 0;
  PQ_TRY(fetch(c, &occ, counts + ncell));
  *cell_used = cell;
  *per_cell = double(n) / double(occ > 0 ? occ : 1);
  return 0;
}

// ---- a box without the cloud's sparse tails --------------------------------------------
// A scan with a few stray returns tens of metres outside would have its search grids sized for
// mostly empty space (a million points at k = 20: up to 50 ms instead of 2.3). Binning CLAMPS into the
// outermost cells (cell_index), and a clamp moves no two points further apart, so a grid over a
// smaller box stays exact for searches that bound distances from below by cell rings; what it
// costs is that the clamped points themselves find their neighbours late. The box is therefore
// cut back only by as many points as the search can afford to treat one by one (`budget`).

static constexpr int kAxisBins = 64;
static constexpr int kAxisBlocks = 512;
static constexpr int kAxisSample = 4;

__global__ __launch_bounds__(256) void k_axis_hist(const double* __restrict__ xyz, int64_t n, double mnx,
                                                   double mny, double mnz, double ix, double iy, double iz,
                                                   int32_t* __restrict__ part /*[gridDim.x][3 * kAxisBins]*/) {
  __shared__ int32_t h[3 * kAxisBins];
  for (int t = threadIdx.x; t < 3 * kAxisBins; t += 256) h[t] = 0;
  __syncthreads();
  // every kAxisSample-th point (counted kAxisSample times): the LDS atomics of neighbouring points
  // land on the same bins and are served one at a time — all points cost 0.09 ms per million; a
  // stray the sample misses leaves its bin empty, which is what lets the cut pass it
  for (int64_t i = (blockIdx.x * 256ll + threadIdx.x) * kAxisSample; i < n;
       i += int64_t(gridDim.x) * 256 * kAxisSample) {
    const double bx = floor((xyz[3 * i] - mnx) * ix), by = floor((xyz[3 * i + 1] - mny) * iy),
                 bz = floor((xyz[3 * i + 2] - mnz) * iz);
    atomicAdd(&h[int(fmin(fmax(bx, 0.0), double(kAxisBins - 1)))], kAxisSample);
    atomicAdd(&h[kAxisBins + int(fmin(fmax(by, 0.0), double(kAxisBins - 1)))], kAxisSample);
    atomicAdd(&h[2 * kAxisBins + int(fmin(fmax(bz, 0.0), double(kAxisBins - 1)))], kAxisSample);
  }
  __syncthreads();
  for (int t = threadIdx.x; t < 3 * kAxisBins; t += 256) part[size_t(blockIdx.x) * 3 * kAxisBins + t] = h[t];
}

// one wave per bin
__global__ __launch_bounds__(64) void k_axis_fold(const int32_t* __restrict__ part, int nblk,
                                                  int32_t* __restrict__ out) {
  const int t = blockIdx.x;
  int32_t s = 0;
  for (int b = threadIdx.x; b < nblk; b += 64) s += part[size_t(b) * 3 * kAxisBins + t];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (threadIdx.x == 0) out[t] = s;
}

int robust_box(Ctx* c, const double* xyz, int64_t n, int budget, double box[6], int64_t* outside) {
  *outside = 0;
  if (budget <= 0 || n < 64) return 0;
  const int blocks = int(std::min<int64_t>(ceil_div(n, 256 * kAxisSample), kAxisBlocks));
  int32_t *d_part = nullptr, *d_hist = nullptr;
  PQ_TRY(c->arena.get(size_t(blocks) * 3 * kAxisBins, &d_part));
  PQ_TRY(c->arena.get(size_t(3 * kAxisBins), &d_hist));
  // points one side of one axis may lose: a stray in a corner is counted on three sides, strays
  // on one side of the scan on one — the union stays below 2 x budget, which is what the caller
  // accepts
  const int side = budget / 3;
  int64_t lost_axis[3] = {0, 0, 0};  // (a later cut counts the earlier one's points again: they sit in its end bins)
  for (int round = 0; round < 6; ++round) {
    double inv[3];
    for (int a = 0; a < 3; ++a) {
      const double e = box[3 + a] - box[a];
      inv[a] = e > 0 ? double(kAxisBins) / e : 0.0;
    }
    hipLaunchKernelGGL(k_axis_hist, dim3(blocks), dim3(256), 0, c->stream, xyz, n, box[0], box[1], box[2],
                       inv[0], inv[1], inv[2], d_part);
    hipLaunchKernelGGL(k_axis_fold, dim3(3 * kAxisBins), dim3(64), 0, c->stream, d_part, blocks, d_hist);
    PQ_HIP(hipGetLastError());
    int32_t h[3 * kAxisBins];
    PQ_TRY(fetch(c, h, d_hist, 3 * kAxisBins));
    bool cut = false;
    for (int a = 0; a < 3; ++a) {
      const int32_t* ha = h + a * kAxisBins;
      int lo = 0, hi = kAxisBins - 1;
      int64_t acc = 0;
      while (lo < hi && acc + ha[lo] <= side) acc += ha[lo++];
      int64_t lost_a = acc;
      acc = 0;
      while (hi > lo && acc + ha[hi] <= side) acc += ha[hi--];
      lost_a += acc;
      // worth it only when the axis loses a quarter of its length
      if (hi - lo + 1 > (3 * kAxisBins) / 4 || !(inv[a] > 0)) continue;
      const double w = (box[3 + a] - box[a]) / double(kAxisBins);
      const double mn = box[a];
      box[a] = mn + w * double(lo);
      box[3 + a] = mn + w * double(hi + 1);
      lost_axis[a] = lost_a;
      cut = true;
    }
    if (!cut) break;
    *outside = (lost_axis[0] + lost_axis[1]) + lost_axis[2];
  }
  return 0;
}

int cloud_bbox(Ctx* c, const double* xyz, int64_t n, double mn[3], double mx[3], bool* all_f32,
               int32_t* zero_buf, int zero_n) {
  if (n <= 0) return fail(PYQSM_EINVAL, "bounding box of an empty cloud");
  const int blocks = bbox_blocks(c, n);
  unsigned long long *d_box = nullptr, *d_part = nullptr;
  PQ_TRY(c->arena.get(kBoxVals, &d_box));
  PQ_TRY(c->arena.get(size_t(blocks) * kBoxVals, &d_part));
  hipLaunchKernelGGL(k_bbox, dim3(blocks), dim3(256), 0, c->stream, xyz, n, d_part, zero_buf, zero_n,
                     static_cast<unsigned long long*>(nullptr));
  hipLaunchKernelGGL(k_bbox_fold, dim3(1), dim3(256), 0, c->stream, d_part, blocks, d_box, PlanIn{},
                     static_cast<GridPlan*>(nullptr));
  PQ_HIP(hipGetLastError());
  unsigned long long h_box[kBoxVals];
  PQ_TRY(fetch(c, h_box, d_box, kBoxVals));
  if (all_f32) *all_f32 = h_box[6] != 0;
  for (int a = 0; a < 3; ++a) {
    mn[a] = ord_val(h_box[a]);
    mx[a] = ord_val(h_box[3 + a]);
    if (!std::isfinite(mn[a]) || !std::isfinite(mx[a]))
      return fail(PYQSM_EINVAL, "point coordinates must be finite");
  }
  return 0;
}

static int build_grid_bucketed(Ctx* c, const double* xyz, int64_t n, DevGrid* g);
static bool bucketed_fits(const DevGrid& g);

int build_grid(Ctx* c, const double* xyz, int64_t n, double min_cell, int64_t max_cells,
               DevGrid* g, const double* bbox, bool f32_records) {
  if (n <= 0) return fail(PYQSM_EINVAL, "build_grid: empty cloud");
  if (n > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 points per call");
  if (!(min_cell > 0) || !std::isfinite(min_cell))
    return fail(PYQSM_EINVAL, "cell edge must be positive and finite");
  double mn[3], mx[3];
  if (bbox) {
    for (int a = 0; a < 3; ++a) {
      mn[a] = bbox[a];
      mx[a] = bbox[3 + a];
    }
  } else {
    PQ_TRY(cloud_bbox(c, xyz, n, mn, mx));
  }
  double cell = min_cell;
  int dims[3];
  for (;;) {
    double tot;
    const bool ok = interior_slabs(mn, mx, cell, 2.0, dims, &tot);
    // (a grid that fits has far fewer than 2^52 slabs per axis: + 1 and + 2 are exact, the doubles those of
    // floor(...) + 3)
    if (ok && tot <= double(max_cells)) break;
    cell *= 2.0;
  }
  for (int a = 0; a < 3; ++a) dims[a] += 2;  // the border
  g->minx = mn[0];
  g->miny = mn[1];
  g->minz = mn[2];
  g->cell = cell;
  g->inv_cell = 1.0 / cell;
  g->nx = dims[0];
  g->ny = dims[1];
  g->nz = dims[2];
  g->ncell = int64_t(dims[0]) * dims[1] * dims[2];
  int32_t *cell_tmp, *rank_tmp;
  PQ_TRY(c->arena.get(size_t(g->ncell) + 1, &g->start));
  PQ_TRY(c->arena.get(size_t(n), &g->order));
  PQ_TRY(c->arena.get(size_t(n), &g->cell_of));
  // two-level counting sort: no scattered atomics, no memset and no scan of the directory; with
  // it, fp32 records instead of three fp64 arrays when the caller vouches for the input
  // (cloud_bbox's flag) and reads through on_coords()
  const bool bucketed = bucketed_fits(*g);
  g->p4 = nullptr;
  g->sx = g->sy = g->sz = nullptr;
  {
    const char* f32_env = getenv("PYQSM_COORD_F32");  // "0": keep fp64 storage (A/B comparisons)
    if (f32_env && !strcmp(f32_env, "0")) f32_records = false;
  }
  if (bucketed && f32_records) {
    PQ_TRY(c->arena.get(size_t(n), &g->p4));
  } else {
    PQ_TRY(c->arena.get(size_t(n), &g->sx));
    PQ_TRY(c->arena.get(size_t(n), &g->sy));
    PQ_TRY(c->arena.get(size_t(n), &g->sz));
  }
  if (bucketed) return build_grid_bucketed(c, xyz, n, g);
  PQ_TRY(c->arena.get(size_t(n), &cell_tmp));
  PQ_TRY(c->arena.get(size_t(n), &rank_tmp));
  PQ_HIP(hipMemsetAsync(g->start, 0, (size_t(g->ncell) + 1) * 4, c->stream));
  const GridParams gp = grid_params(*g);
  const dim3 grid(ceil_div(n, 256));
  g->occ_blocks = int(grid.x);
  PQ_TRY(c->arena.get(size_t(g->occ_blocks), &g->occ_part));
  hipLaunchKernelGGL(k_cell_count, grid, dim3(256), 0, c->stream, xyz, n, gp, g->start, cell_tmp,
                     rank_tmp, g->occ_part);
  PQ_HIP(hipGetLastError());
  PQ_TRY(exclusive_scan_i32(c, g->start, g->ncell + 1));
  hipLaunchKernelGGL(k_cell_scatter, grid, dim3(256), 0, c->stream, xyz, n, g->start, cell_tmp,
                     rank_tmp, g->order, g->cell_of, g->sx, g->sy, g->sz);
  PQ_HIP(hipGetLastError());
  return 0;
}


// ---- grid + octant sub-cells in one pass (DBSCAN's binning) ------------------------------

struct AxisMap {  // raw slab index -> compressed slab index (+1 for the border); null = identity
  const int32_t *x, *y, *z;
};

struct RawCell {
  int cx, cy, cz, oct;
};

// raw interior coordinates (0-based, clamped) and the octant inside the raw cell
__device__ __forceinline__ RawCell raw_cell(const GridParams& g, int rx, int ry, int rz, double x,
                                            double y, double z) {
  // positions in half cells; the cell is half of that, the octant its parity
  int hx = int(floor((x - g.minx) * (2.0 * g.inv_cell)));
  int hy = int(floor((y - g.miny) * (2.0 * g.inv_cell)));
  int hz = int(floor((z - g.minz) * (2.0 * g.inv_cell)));
  int cx = int(floor((x - g.minx) * g.inv_cell));
  int cy = int(floor((y - g.miny) * g.inv_cell));
  int cz = int(floor((z - g.minz) * g.inv_cell));
  cx = cx < 0 ? 0 : (cx > rx - 1 ? rx - 1 : cx);
  cy = cy < 0 ? 0 : (cy > ry - 1 ? ry - 1 : cy);
  cz = cz < 0 ? 0 : (cz > rz - 1 ? rz - 1 : cz);
  // octant relative to the cell the point was binned into (half cells past the cell's first: h - 2 c < 1 ? 0 : 1)
  const int ox = hx - 2 * cx < 1 ? 0 : 1, oy = hy - 2 * cy < 1 ? 0 : 1, oz = hz - 2 * cz < 1 ? 0 : 1;
  return RawCell{cx, cy, cz, ox | (oy << 1) | (oz << 2)};
}

// which raw slabs hold a point (plain stores of 1: racing stores of the same value)
__global__ __launch_bounds__(256) void k_axis_occ(const double* __restrict__ xyz, int64_t n,
                                                  GridParams g, int rx, int ry, int rz,
                                                  int32_t* __restrict__ ox, int32_t* __restrict__ oy,
                                                  int32_t* __restrict__ oz) {
  int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (i >= n) return;
  const RawCell r = raw_cell(g, rx, ry, rz, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
  ox[r.cx] = 1;
  oy[r.cy] = 1;
  oz[r.cz] = 1;
}

// keep[i] = slab i is occupied, or is the first empty slab after an occupied one
__global__ __launch_bounds__(256) void k_axis_keep(int m, const int32_t* __restrict__ occ,
                                                   int32_t* __restrict__ keep /*[m + 1]*/) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i > m) return;
  keep[i] = i < m ? ((occ[i] || (i > 0 && occ[i - 1])) ? 1 : 0) : 0;
}

// after the scan: compressed index of every raw slab, shifted by the border cell
__global__ __launch_bounds__(256) void k_axis_shift(int m, int32_t* __restrict__ map) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i < m) map[i] += 1;
}

template <bool MAPPED>
__global__ __launch_bounds__(256) void k_cell_count_oct(const double* __restrict__ xyz, int64_t n,
                                                        GridParams g, int rx, int ry, int rz, AxisMap am,
                                                        int32_t* __restrict__ counts,
                                                        int32_t* __restrict__ cell_tmp,
                                                        int32_t* __restrict__ rank_tmp) {
  int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (i >= n) return;
  const RawCell r = raw_cell(g, rx, ry, rz, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
  const int cx = MAPPED ? am.x[r.cx] : r.cx + 1, cy = MAPPED ? am.y[r.cy] : r.cy + 1,
            cz = MAPPED ? am.z[r.cz] : r.cz + 1;
  const int c = (cz * g.ny + cy) * g.nx + cx;
  cell_tmp[i] = c;
  rank_tmp[i] = (atomicAdd(&counts[c], 1) << 3) | r.oct;  // arrival rank in the cell, octant
}

// One 32-byte record per point to its cell-sorted position: coordinates, original index,
// cell * 8 + octant. (Scattering only (index, key) and gathering the coordinates in the ordering
// pass cost 13 + 51 us per million points: a million random 24-byte reads. With the coordinates
// in the record the ordering pass reads and writes whole lines.)
struct alignas(32) PointRec {
  double x, y, z;
  int32_t idx, key;
};

__global__ __launch_bounds__(256) void k_scatter_keys(const double* __restrict__ xyz, int64_t n,
                                                      const int32_t* __restrict__ start,
                                                      const int32_t* __restrict__ cell_tmp,
                                                      const int32_t* __restrict__ rank_tmp,
                                                      PointRec* __restrict__ keyed) {
  int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (i >= n) return;
  const int c = cell_tmp[i], ro = rank_tmp[i];
  PointRec r;
  r.x = xyz[3 * i];
  r.y = xyz[3 * i + 1];
  r.z = xyz[3 * i + 2];
  r.idx = int(i);
  r.key = (c << 3) | (ro & 7);
  keyed[start[c] + (ro >> 3)] = r;
}

static constexpr int kBigCell = 128;  // cells with more points are ordered by a block, not per point

// One thread per cell-sorted position p: the final position of its point inside the cell's run,
// ordered by octant (stable in arrival rank), from the octant bits of the run itself; the run's
// first thread also writes the eight sub-cell records. Cells with more than kBigCell points are
// listed for k_order_big (a per-point walk would be quadratic in the cell's size).
__global__ __launch_bounds__(256) void k_order_cells(int n, const int32_t* __restrict__ start,
                                                     const PointRec* __restrict__ keyed,
                                                     int32_t* __restrict__ order,
                                                     int32_t* __restrict__ cell_of,
                                                     int32_t* __restrict__ sub_of,
                                                     double* __restrict__ sx, double* __restrict__ sy,
                                                     double* __restrict__ sz,
                                                     int4* __restrict__ rec,
                                                     int32_t* __restrict__ big_list,
                                                     int32_t* __restrict__ big_cnt) {
  const SortedStore out{order, cell_of, sub_of, nullptr, sx, sy, sz};
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const PointRec me = keyed[p];
  const int c = me.key >> 3, o = me.key & 7;
  const int b = start[c], e = start[c + 1];
  if (e - b > kBigCell) {
    if (p == b) big_list[atomicAdd(big_cnt, 1)] = c;
    return;
  }
  int less = 0, same_before = 0;
  int cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool first = p == b;
  for (int q = b; q < e; ++q) {
    const int oq = keyed[q].key & 7;
    less += oq < o;
    same_before += (oq == o) & (q < p);
    if (first) {
#pragma unroll
      for (int k = 0; k < 8; ++k) cnt[k] += oq == k;
    }
  }
  out.put(b + less + same_before, me.idx, c, me.x, me.y, me.z, b * 8 + o);
  if (first) write_sub_records(rec, b, cnt);
}

// A block of W threads orders one run [b, e) of `keyed` (a cell's points in arrival order, key = cell * 8 +
// octant) by octant, stable in arrival order: octant totals, the cell's eight sub-cell records, then chunks
// of W in run order, ranked inside the chunk by ballots, with chunk bases that advance. tot, base and wcnt
// are the caller's LDS; whoever wrote the run has passed a barrier, and the call ends on one.
template <int W>
__device__ __forceinline__ void order_run_by_octant(const PointRec* __restrict__ keyed, int b, int e, int32_t (&tot)[8],
                                                    int32_t (&base)[8], int32_t (&wcnt)[W / 64][8],
                                                    const SortedStore& out, int4* __restrict__ rec) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  int loc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int q = b + t; q < e; q += W) {
    const int oq = keyed[q].key & 7;
#pragma unroll
    for (int k = 0; k < 8; ++k) loc[k] += oq == k;
  }
  if (t < 8) tot[t] = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    int cnt = loc[k];
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    if (lane == 0 && cnt) atomicAdd(&tot[k], cnt);  // LDS
  }
  __syncthreads();
  if (t == 0) {
    int r2 = b;
    for (int k = 0; k < 8; ++k) {
      base[k] = r2;
      r2 += tot[k];
    }
    write_sub_records(rec, b, tot);
  }
  __syncthreads();
  for (int q0 = b; q0 < e; q0 += W) {
    const int q = q0 + t;
    const bool live = q < e;
    PointRec pr;
    pr.key = 0;
    if (live) pr = keyed[q];
    const int o = pr.key & 7;
    int before = 0;  // same octant, earlier lane of this wave
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const unsigned long long m = __ballot(live && o == k);
      if (lane == 0) wcnt[w][k] = __popcll(m);
      if (o == k) before = __popcll(m & ((1ull << lane) - 1ull));
    }
    __syncthreads();
    if (live) {
      int f = base[o] + before;
      for (int ww = 0; ww < w; ++ww) f += wcnt[ww][o];
      out.put(f, pr.idx, pr.key >> 3, pr.x, pr.y, pr.z, b * 8 + o);
    }
    __syncthreads();
    if (t < 8) {
      int add = 0;
      for (int ww = 0; ww < W / 64; ++ww) add += wcnt[ww][t];
      base[t] += add;
    }
    __syncthreads();
  }
}

// A block per big cell of the atomic binning.
__global__ __launch_bounds__(256) void k_order_big(const int32_t* __restrict__ big_list,
                                                   const int32_t* __restrict__ big_cnt,
                                                   const int32_t* __restrict__ start,
                                                   const PointRec* __restrict__ keyed,
                                                   int32_t* __restrict__ order,
                                                   int32_t* __restrict__ cell_of,
                                                   int32_t* __restrict__ sub_of,
                                                   double* __restrict__ sx, double* __restrict__ sy,
                                                   double* __restrict__ sz, float4* __restrict__ p4,
                                                   int4* __restrict__ rec, const GridPlan* __restrict__ plan) {
  __shared__ int32_t tot[8], base[8], wcnt[4][8];
  const SortedStore out{order, cell_of, sub_of, p4, sx, sy, sz};
  if (!plan->ok) return;
  const int nbig = *big_cnt;  // usually 0: the launch is then a few idle blocks
  for (int bi = blockIdx.x; bi < nbig; bi += gridDim.x) {  // block-uniform
    const int c = big_list[bi];
    order_run_by_octant<256>(keyed, start[c], start[c + 1], tot, base, wcnt, out, rec);
  }
}

// ---- the same outputs without scattered global atomics and without a pass over the directory ----
// Round 2's binning above costs one returning atomic per point at 64 different lines per wave
// instruction (the chip's scattered-atomic rate: 51 us per million points), a memset and a
// three-phase scan of the dense directory (16 M cells: 65 us), a 32-byte record scattered and read
// back (20 + 48 us). This version splits the counting sort in two levels so that every atomic
// is either in LDS or lands, 64 lanes wide, on 64 CONSECUTIVE counters (4 memory requests instead of
// 64), and the directory is written exactly once, by the blocks that sort:
//   A1  k_bk_hist     cell and octant of every point; per block an LDS histogram over the BUCKETS
//                     (a bucket = 4096 or 8192 consecutive cell ids), flushed with one atomic per
//                     non-empty (block, bucket), lanes on consecutive buckets
//   A2  k_bk_scatter  every block scans the <= 16384 bucket totals itself (no one-block kernel between the
//                     passes); the same LDS histogram again, this time returning the rank inside the block;
//                     a block reserves its share of every bucket with one returning atomic
//                     (same shape) and writes the records bucket by bucket: 16 bytes (fp32-representable
//                     clouds) or 32, and the 4-byte key in an array of its own
//   B   k_bk_sort     one block per bucket, everything in LDS (bk_two_sweeps with the policy BkOctants): a
//                     count per cell (arrival rank) and eight 8-bit counts per cell packed in a u64 (rank
//                     inside the octant), a block scan of the bucket's cell counts -> the bucket's piece of
//                     the ranked directory (grid.hpp, CellDir: a word per 32 cells, a slot per occupied
//                     cell; a dense start[ncell + 1] was 60 MB per step for a forest's 0.4 % of occupied
//                     cells), written once; every point then goes straight to its final, octant-ordered
//                     place. Cells with more than 255 points (a packed count could overflow) are ordered
//                     by the same block afterwards (order_run_by_octant, as in k_order_big). A bucket of
//                     at most 64 points skips the counters: one wave ranks its points.
//       k_bk_sort_plain  the same two sweeps for build_grid (the policy BkPlain): cells only, the dense start
// Same arrays as the atomic binning leaves (the order inside a sub-cell is the arrival order of
// atomics in both versions, and nothing downstream depends on it).
static constexpr int kBkBig = 255;              // cells above this are ordered after k_bk_sort's sweep
static constexpr int kBkPer = 12;               // points of a bucket whose key and ranks a thread of k_bk_sort keeps
                                                // in registers, one word each: a bucket of up to 512 * 12 = 6144
                                                // points (8192-cell buckets: 12288) is sorted without a rank
                                                // leaving the registers

// Points per 256-thread block of the A passes. 1024 and 512 (two and four times the blocks) were measured
// against it on the forest: the step 0.366 and 0.389 ms against 0.360 at 1 M points, 1.63 and 1.71 ms
// against 1.60 at 5 M. What a block pays before its first point (LDS clear, the scan of the bucket
// totals, one reservation per bucket it touches) does not shrink with its share of the points.
static constexpr int kBkPts = 2048;

// The bucketed record of a point. Clouds whose coordinates are all fp32-representable (F32: the grid
// keeps float4 records) move 16 bytes, (x, y, z, index bits); the others three doubles, the index and
// the key. Both forms leave the key (cell * 8 + octant) in an array of its own as well, which is all
// that the sort's first sweep reads.
template <bool F32>
struct BkRec;
template <>
struct BkRec<true> {
  using type = float4;
};
template <>
struct BkRec<false> {
  using type = PointRec;
};

// DBSCAN's speculated step (MODE 0) has no plan in memory when k_bk_hist starts: the launch takes the fold's
// place. Every block folds k_bbox's records for itself and computes the plan in registers, all with the same
// fp64 operations in the same order (make_plan), so the blocks agree with each other and with the host; a
// block that finds ok == 0 leaves without a write. One block more than the histogram needs, the launch's
// last, folds once more and stores the plan (store_plan): the kernels behind the next kernel boundary read
// it from memory as they always did, and the host's slot is written earlier than the fold launch wrote it.
// (The fold launch was one block of 8.4 us between k_bbox and this kernel.)
struct PlanFold {
  const unsigned long long* part = nullptr;  // k_bbox's records, or null: no fold
  int nblk = 0;
  PlanIn in{};
  GridPlan* out = nullptr;
};

// MODE 0: cell and octant on the raw grid; 1: the same through the axis-compression maps;
// 2: cell only, clamped into the grid's box (build_grid: what kNN and the radius queries bin with)
template <int MODE>
__global__ __launch_bounds__(256) void k_bk_hist(const double* __restrict__ xyz, int64_t n, GridParams g,
                                                 int rx, int ry, int rz, AxisMap am, int nbk, int bits,
                                                 int32_t* __restrict__ key_tmp,
                                                 int32_t* __restrict__ tot, const GridPlan* __restrict__ plan,
                                                 PlanFold pf) {
  extern __shared__ __attribute__((aligned(16))) int32_t h[];
  __shared__ unsigned long long red[4][kBoxVals];  // (the fold's)
  __shared__ unsigned long long fin[kBoxVals];
  const bool folds = MODE == 0 && pf.part != nullptr;        // kernel-uniform
  const bool stores = folds && blockIdx.x + 1 == gridDim.x;  // block-uniform: the role behind the histogram's blocks
  // the block's points first (MODE 0: DBSCAN's raw grid): their loads are in flight during the fold. The other
  // modes load where they use, as they did.
  const int64_t base = int64_t(blockIdx.x) * kBkPts;
  double px[kBkPts / 256], py[kBkPts / 256], pz[kBkPts / 256];
#pragma unroll
  for (int k = 0; k < kBkPts / 256; ++k) {
    const int64_t i = base + k * 256 + threadIdx.x;
    px[k] = py[k] = pz[k] = 0.0;
    if (MODE == 0 && i < n) {
      px[k] = xyz[3 * i];
      py[k] = xyz[3 * i + 1];
      pz[k] = xyz[3 * i + 2];
    }
  }
  if (folds || plan) {  // DBSCAN: the grid comes from the plan (the LDS was sized for at least its nbk)
    GridPlan pl;
    if (folds) {
      fold_box_records(pf.part, pf.nblk, red, fin);
      pl = make_plan(fin, pf.in);
      if (stores) {
        if (threadIdx.x == 0) store_plan(pl, pf.in, pf.out);
        return;
      }
    } else {
      pl = *plan;
    }
    if (!pl.ok) return;
    g = GridParams{pl.mn[0], pl.mn[1], pl.mn[2], pl.inv_cell, pl.nx, pl.ny, pl.nz};
    rx = pl.rx;
    ry = pl.ry;
    rz = pl.rz;
    nbk = pl.nbk;
    bits = pl.bits;
  }
  for (int b = threadIdx.x; b < nbk; b += 256) h[b] = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kBkPts / 256; ++k) {
    const int64_t i = base + k * 256 + threadIdx.x;
    if (i < n) {
      int c, oct = 0;
      if (MODE != 0) px[k] = xyz[3 * i], py[k] = xyz[3 * i + 1], pz[k] = xyz[3 * i + 2];
      if (MODE == 2) {
        c = cell_index(g, px[k], py[k], pz[k]);
      } else {
        const RawCell r = raw_cell(g, rx, ry, rz, px[k], py[k], pz[k]);
        const int cx = MODE == 1 ? am.x[r.cx] : r.cx + 1, cy = MODE == 1 ? am.y[r.cy] : r.cy + 1,
                  cz = MODE == 1 ? am.z[r.cz] : r.cz + 1;
        c = (cz * g.ny + cy) * g.nx + cx;
        oct = r.oct;
      }
      key_tmp[i] = (c << 3) | oct;
      atomicAdd(&h[c >> bits], 1);  // LDS
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < nbk; b += 256) {
    const int v = h[b];
    if (v) atomicAdd(&tot[b], v);  // lanes on consecutive counters: 4 requests per wave instruction
  }
}

// one block: bstart[b] = points in buckets before b (bstart[nbk] = n). Used for directories of many
// buckets; up to kBkFusedScan buckets every block of k_bk_scatter scans the totals itself instead.
static constexpr int kBkFusedScan = 4096;
__global__ __launch_bounds__(1024) void k_bk_scan(int nbk, const int32_t* __restrict__ tot,
                                                  int32_t* __restrict__ bstart, const GridPlan* __restrict__ plan) {
  __shared__ int32_t wsum[16];
  if (plan) {
    if (!plan->ok) return;
    nbk = plan->nbk;
  }
  const int per = (nbk + 1023) / 1024;  // <= 16
  const int b0 = threadIdx.x * per;
  int32_t v[16], s = 0;
  for (int k = 0; k < per; ++k) {
    v[k] = b0 + k < nbk ? tot[b0 + k] : 0;
    s += v[k];
  }
  int32_t run = block_excl_scan<1024>(s, wsum);
  for (int k = 0; k < per; ++k) {
    if (b0 + k < nbk) bstart[b0 + k] = run;
    run += v[k];
  }
  if (threadIdx.x == 1023) bstart[nbk] = run;
}

template <bool F32>
__global__ __launch_bounds__(256) void k_bk_scatter(const double* __restrict__ xyz, int64_t n, int nbk,
                                                    int bits, const int32_t* __restrict__ key_tmp,
                                                    const int32_t* __restrict__ tot,
                                                    int32_t* __restrict__ cursor /*zeroed*/,
                                                    int32_t* __restrict__ bstart /*[nbk + 1]: written by block 0
                                                    (fused) or read (scanned by k_bk_scan)*/,
                                                    int fused,
                                                    typename BkRec<F32>::type* __restrict__ bucketed,
                                                    int32_t* __restrict__ keyb /*the keys in bucket order*/,
                                                    const GridPlan* __restrict__ plan) {
  extern __shared__ __attribute__((aligned(16))) int32_t h[];  // [nbk] ranks / shares (+ [nbk] bucket starts: fused)
  // the block's keys and coordinates first: their loads are in flight during the scan of the totals
  const int64_t base = int64_t(blockIdx.x) * kBkPts;
  using Coord = typename std::conditional<F32, float, double>::type;  // what the record keeps
  int key[kBkPts / 256], lr[kBkPts / 256];
  Coord px[kBkPts / 256], py[kBkPts / 256], pz[kBkPts / 256];
#pragma unroll
  for (int k = 0; k < kBkPts / 256; ++k) {
    const int64_t i = base + k * 256 + threadIdx.x;
    key[k] = -1;
    px[k] = py[k] = pz[k] = Coord(0);
    if (i < n) {
      key[k] = key_tmp[i];
      px[k] = Coord(xyz[3 * i]);
      py[k] = Coord(xyz[3 * i + 1]);
      pz[k] = Coord(xyz[3 * i + 2]);
    }
  }
  if (plan) {
    if (!plan->ok) return;
    nbk = plan->nbk;
    bits = plan->bits;
  }
  int32_t* pre = h + nbk;
  __shared__ int32_t wsum[4];
  for (int b = threadIdx.x; b < nbk; b += 256) h[b] = 0;
  // fused: every block scans the bucket totals itself (<= 16 KB out of L2: cheaper than a one-block
  // kernel of its own between the two passes): thread t owns kPer consecutive buckets, whose totals it
  // loads together and keeps in registers (as a loop of `nbk / 256` loads, each waited for, and run twice,
  // it was most of the 13 us that a launch of one block with 64 points took on the forest's 3 687 buckets)
  if (fused) {
    constexpr int kPer = kBkFusedScan / 256;
    const int b0 = threadIdx.x * kPer;
    int32_t v[kPer], s = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      v[k] = b0 + k < nbk ? tot[b0 + k] : 0;
      s += v[k];
    }
    int32_t run = block_excl_scan<256>(s, wsum);
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      if (b0 + k < nbk) {
        pre[b0 + k] = run;
        if (blockIdx.x == 0) bstart[b0 + k] = run;
      }
      run += v[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 255) bstart[nbk] = run;  // buckets past nbk count as empty
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kBkPts / 256; ++k) {
    lr[k] = key[k] >= 0 ? atomicAdd(&h[key[k] >> (3 + bits)], 1) : 0;  // rank inside this block's share
  }
  __syncthreads();
  // this block's share of every bucket it has points in: the reservations of sixteen buckets per thread
  // are issued before the first of them is waited for
  for (int bb = 0; bb < nbk; bb += 16 * 256) {
    int32_t v[16], a[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int b = bb + k * 256 + threadIdx.x;
      v[k] = b < nbk ? h[b] : 0;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      a[k] = 0;
      if (v[k]) a[k] = atomicAdd(&cursor[bb + k * 256 + threadIdx.x], v[k]);
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int b = bb + k * 256 + threadIdx.x;
      if (v[k]) h[b] = (fused ? pre[b] : bstart[b]) + a[k];
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kBkPts / 256; ++k) {
    if (key[k] < 0) continue;
    const int64_t i = base + k * 256 + threadIdx.x;
    const int pos = h[key[k] >> (3 + bits)] + lr[k];
    keyb[pos] = key[k];
    if constexpr (F32) {
      bucketed[pos] = make_float4(px[k], py[k], pz[k], __int_as_float(int(i)));
    } else {
      PointRec r;
      r.x = px[k];
      r.y = py[k];
      r.z = pz[k];
      r.idx = int(i);
      r.key = key[k];
      bucketed[pos] = r;
    }
  }
}

// records of a bucket that a thread of sweep 2 fetches together, one group ahead of the one it places:
// two of 16 bytes or one of 32 (more cost over 90 VGPRs, or scratch under the cap of 80 that keeps
// three blocks on a CU)
template <bool F32>
static constexpr int kBkGrp = F32 ? 2 : 1;

__device__ __forceinline__ int rec_idx(const float4& p) { return __float_as_int(p.w); }
__device__ __forceinline__ int rec_idx(const PointRec& p) { return p.idx; }

// ---- the second level: one block sorts one bucket, in two sweeps ---------------------------------------
// One block per bucket of 2^BITS cells, a thread per eight cells (BITS = 12: 512 threads, three blocks per
// CU; BITS = 13 for directories beyond 2^26 cells). Sweep 1 reads only the 4-byte keys and counts in LDS:
// P.rank_of packs what it learns of a point (its cell inside the bucket, its arrival rank, saturated) into
// one word, and the words of the bucket's first T * kBkPer points stay in registers between the sweeps (on
// the 1 M-point forest of the benchmark the largest of the 3 687 buckets holds 4 891 points: every bucket).
// Thread t then owns cells 8 t .. 8 t + 7: P.scan carries their counts across the block, P.directory writes
// the bucket's piece of the directory and leaves each cell's offset in the bucket where its count was.
// Sweep 2 fetches the records in unrolled groups, the next group's loads issued before the current one is
// placed (P.place). The block's chain of dependent memory round trips is bstart -> keys (and the first
// group of records) -> records -> stores. A bucket beyond the capacity takes further rounds of the same
// register tile, whose words alone go through word_tmp.
// A policy P supplies: cnt() (the LDS counts, [2^BITS]), clear(t), rank_of(key, j), scan(v, tot, t) -> the
// points in the cells before the thread's eight, directory(v, pre, t), place(rec, word, j).
template <int BITS, bool F32, class Policy>
__device__ __forceinline__ void bk_two_sweeps(Policy& P, int s, int e,
                                              const typename BkRec<F32>::type* __restrict__ bucketed,
                                              const int32_t* __restrict__ keyb, uint32_t* __restrict__ word_tmp) {
  constexpr int CELLS = 1 << BITS, T = CELLS / 8, CAP = T * kBkPer, G = kBkGrp<F32>;
  using Rec = typename BkRec<F32>::type;
  static_assert(kBkPer % G == 0, "whole groups");
  const int t = threadIdx.x;
  // the loads are issued before the LDS is cleared: the keys of the register tile (point k * T + t of
  // the bucket is thread t's k-th) and the first group of records
  uint32_t wd[kBkPer];
#pragma unroll
  for (int k = 0; k < kBkPer; ++k) {
    const int j = s + k * T + t;
    wd[k] = j < e ? uint32_t(keyb[j]) : 0u;
  }
  Rec cur[G] = {};
#pragma unroll
  for (int k = 0; k < G; ++k) {
    const int j = s + k * T + t;
    if (j < e) cur[k] = bucketed[j];
  }
  P.clear(t);
  __syncthreads();
  // sweep 1
#pragma unroll
  for (int k = 0; k < kBkPer; ++k) {
    const int j = s + k * T + t;
    if (j < e) wd[k] = P.rank_of(wd[k], j);
  }
  for (int base = s + CAP; base < e; base += CAP) {  // block-uniform: further rounds of the tile
    uint32_t kk[kBkPer];
#pragma unroll
    for (int k = 0; k < kBkPer; ++k) {
      const int j = base + k * T + t;
      kk[k] = j < e ? uint32_t(keyb[j]) : 0u;
    }
#pragma unroll
    for (int k = 0; k < kBkPer; ++k) {
      const int j = base + k * T + t;
      if (j < e) word_tmp[j] = P.rank_of(kk[k], j);
    }
  }
  __syncthreads();
  // the bucket's cells: thread t owns eight consecutive ones
  int32_t* const cnt = P.cnt();
  int32_t v[8], tot = 0;
  {
    const int4 a = *reinterpret_cast<const int4*>(&cnt[8 * t]);
    const int4 b = *reinterpret_cast<const int4*>(&cnt[8 * t + 4]);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
#pragma unroll
    for (int k = 0; k < 8; ++k) tot += v[k];
  }
  int32_t run = P.scan(v, tot, t);
  int32_t pre[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    pre[k] = run;
    run += v[k];
  }
  P.directory(v, pre, t);
  __syncthreads();
  // sweep 2: every point to its place
#pragma unroll
  for (int g = 0; g < kBkPer / G; ++g) {
    if (s + g * G * T >= e) break;  // block-uniform
    Rec nxt[G] = {};
    if (g + 1 < kBkPer / G) {
#pragma unroll
      for (int k = 0; k < G; ++k) {
        const int j = s + ((g + 1) * G + k) * T + t;
        if (j < e) nxt[k] = bucketed[j];
      }
    }
#pragma unroll
    for (int k = 0; k < G; ++k) {
      const int j = s + (g * G + k) * T + t;
      if (j < e) P.place(cur[k], wd[g * G + k], j);
    }
#pragma unroll
    for (int k = 0; k < G; ++k) cur[k] = nxt[k];
  }
  for (int base = s + CAP; base < e; base += CAP) {  // block-uniform
#pragma unroll
    for (int g = 0; g < kBkPer / G; ++g) {
      if (base + g * G * T >= e) break;
      Rec r[G] = {};
      uint32_t w[G];
#pragma unroll
      for (int k = 0; k < G; ++k) {
        const int j = base + (g * G + k) * T + t;
        w[k] = 0u;
        if (j < e) {
          r[k] = bucketed[j];
          w[k] = word_tmp[j];
        }
      }
#pragma unroll
      for (int k = 0; k < G; ++k) {
        const int j = base + (g * G + k) * T + t;
        if (j < e) P.place(r[k], w[k], j);
      }
    }
  }
}

// ---- DBSCAN's policy: cells AND octants, the ranked directory ------------------------------------------
// A count per cell (arrival rank) and eight 8-bit counts per cell packed in a u64 (rank inside the octant);
// the scan carries the occupied cells beside the points (their ranks are the directory's slots); every
// point goes straight to its final, octant-ordered place. Cells with more than kBkBig points (a packed
// count could overflow) go to their run of `keyed` in arrival order instead, and the block orders them
// after the sweeps.

// sum of the bytes of x below byte o (eight 8-bit counts packed in a u64)
__device__ __forceinline__ int bytes_below(unsigned long long x, int o) {
  x &= (1ull << (8 * o)) - 1ull;
  x = (x & 0x00FF00FF00FF00FFull) + ((x >> 8) & 0x00FF00FF00FF00FFull);
  x = (x & 0x0000FFFF0000FFFFull) + ((x >> 16) & 0x0000FFFF0000FFFFull);
  return int((x + (x >> 32)) & 0xFFFFull);
}

template <int BITS>
struct BkLds {
  unsigned long long oct[1 << BITS];  // eight 8-bit counts per cell
  int32_t cnt[1 << BITS];             // points per cell, then (in place) the cell's offset in the bucket
  uint32_t big[(1 << BITS) / 32];     // cells with more than kBkBig points
  int32_t wsum[16];
  int32_t osum[16];                   // per wave: occupied cells (the directory's slot ranks)
  int32_t any_big;                    // some cell of the bucket is in `big`
  int32_t btot[8], bbase[8];          // a big cell's octant totals and running bases
  int32_t bw[(1 << BITS) / 512][8];   // per wave: points of each octant in the current chunk
};

// What sweep 1 leaves of a point, in one word: the key inside the bucket (cell * 8 + octant, BITS + 3
// <= 16 bits), the arrival rank in the cell saturated at 255 and the arrival rank in the octant. A
// cell of at most kBkBig points has ranks below 255; a saturated rank belongs to a cell that the
// block orders afterwards, and its exact value goes through rank_tmp (the octant's rank is not read
// there).
__device__ __forceinline__ uint32_t bk_word(int lk, int rr, int r8) {
  return (uint32_t(lk) << 16) | (uint32_t(rr < 255 ? rr : 255) << 8) | uint32_t(r8);
}

template <int BITS, bool F32>
struct BkOctants {
  static constexpr int CELLS = 1 << BITS, T = CELLS / 8;
  using Rec = typename BkRec<F32>::type;
  BkLds<BITS>& L;
  const int s, e;         // the bucket's points
  const int64_t c0;       // its first cell
  DirWord* const wds;     // its piece of the ranked directory: the words, and the slots from sb
  int32_t* const slots;
  const uint32_t sb;
  int4* const rec;
  PointRec* const keyed;  // big cells' runs in arrival order
  int32_t* const rank_tmp;
  const SortedStore& out;
  uint32_t occ8;          // which of the thread's eight cells hold a point; how many; how many before them
  int nocc;
  int32_t orun;

  __device__ __forceinline__ int32_t* cnt() const { return L.cnt; }
  __device__ __forceinline__ void clear(int t) const {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      L.oct[k * T + t] = 0ull;
      L.cnt[k * T + t] = 0;
    }
    if (t < CELLS / 32) L.big[t] = 0u;
    if (t == 0) L.any_big = 0;
  }
  // arrival rank in the cell and in the octant
  __device__ __forceinline__ uint32_t rank_of(uint32_t ky, int j) const {
    const int lk = int(ky) & (8 * CELLS - 1), cl = lk >> 3, o = lk & 7;
    const int rr = atomicAdd(&L.cnt[cl], 1);
    const int r8 = int((atomicAdd(&L.oct[cl], 1ull << (8 * o)) >> (8 * o)) & 255ull);
    if (rr >= 255) rank_tmp[j] = rr;
    return bk_word(lk, rr, r8);
  }
  // (the same scan carries the number of occupied cells before the thread's eight: their slots)
  __device__ __forceinline__ int32_t scan(const int32_t (&v)[8], int32_t tot, int) {
    occ8 = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) occ8 |= v[k] ? 1u << k : 0u;
    nocc = __popc(occ8);
    int32_t run;
    block_excl_scan<T>(tot, nocc, L.wsum, L.osum, &run, &orun);
    return run;
  }
  __device__ __forceinline__ void directory(const int32_t (&v)[8], const int32_t (&pre)[8], int t) const {
    {
      // a directory word is four threads' cells: the first of the four collects the others' bits
      const uint32_t b1 = __shfl_down(occ8, 1, 64), b2 = __shfl_down(occ8, 2, 64), b3 = __shfl_down(occ8, 3, 64);
      if ((t & 3) == 0) wds[t >> 2] = DirWord{occ8 | (b1 << 8) | (b2 << 16) | (b3 << 24), sb + uint32_t(orun)};
      if (t == T - 1) slots[sb + uint32_t(orun + nocc)] = e;  // closes the bucket's slots
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int cl = 8 * t + k;
      L.cnt[cl] = pre[k];
      if (v[k] == 0) continue;
      const int b = s + pre[k];  // the cell's first sorted position: identifies its sub-cells
      slots[sb + uint32_t(orun) + __popc(occ8 & ((1u << k) - 1u))] = b;
      if (v[k] > kBkBig) {  // rare: the block orders the cell after sweep 2
        atomicOr(&L.big[cl >> 5], 1u << (cl & 31));
        L.any_big = 1;
        continue;
      }
      write_sub_records(rec, b, L.oct[cl]);
    }
  }
  // every point to its final place (big cells: to the cell's run of `keyed`, in arrival order)
  __device__ __forceinline__ void place(const Rec& p, uint32_t w, int j) const {
    const int lk = int(w >> 16), cl = lk >> 3, o = lk & 7, arr = int((w >> 8) & 255u);
    const int b = s + L.cnt[cl];
    if ((L.big[cl >> 5] >> (cl & 31)) & 1u) {
      PointRec q;
      q.x = p.x;
      q.y = p.y;
      q.z = p.z;
      q.key = int(c0 << 3) + lk;
      q.idx = rec_idx(p);
      keyed[b + (arr < 255 ? arr : rank_tmp[j])] = q;
      return;
    }
    out.put(b + bytes_below(L.oct[cl], o) + int(w & 255u), rec_idx(p), int(c0) + cl, p.x, p.y, p.z, b * 8 + o);
  }
};

// k_bk_sort: a bucket of DBSCAN's binning. A bucket of at most 64 points skips the counters: one wave
// ranks its points. Otherwise the two sweeps (BITS = 12: 49 KB of LDS), and after them the whole block
// orders each cell above kBkBig points, as k_order_big does for the atomic binning.
template <int BITS, bool F32>
__global__ __launch_bounds__((1 << BITS) / 8, BITS == 12 ? 6 : 4) void k_bk_sort(
    const int32_t* __restrict__ bstart,
    const typename BkRec<F32>::type* __restrict__ bucketed, const int32_t* __restrict__ keyb,
    uint32_t* __restrict__ word_tmp, int32_t* __restrict__ rank_tmp,
    DirWord* __restrict__ words /*[nbk << (BITS - 5)]*/, int32_t* __restrict__ slots /*[n + nbk + 1]*/,
    int32_t* __restrict__ order, int32_t* __restrict__ cell_of, int32_t* __restrict__ sub_of,
    double* __restrict__ sx, double* __restrict__ sy, double* __restrict__ sz,
    float4* __restrict__ p4 /*non-null: fp32 records instead of sx / sy / sz*/, int4* __restrict__ rec,
    PointRec* __restrict__ keyed /*big cells' runs in arrival order*/,
    const GridPlan* __restrict__ plan /*the number of buckets (the launch may have more blocks)*/,
    unsigned long long* __restrict__ st /*stamps or null*/) {
  constexpr int CELLS = 1 << BITS, T = CELLS / 8;
  using Rec = typename BkRec<F32>::type;
  __shared__ BkLds<BITS> L;
  stamped(st, [&] {
  const SortedStore out{order, cell_of, sub_of, F32 ? p4 : nullptr, sx, sy, sz};
  const int bk = blockIdx.x, t = threadIdx.x;
  if (!plan->ok || bk >= plan->nbk) return;
  const int s = bstart[bk], e = bstart[bk + 1];
  const int64_t c0 = int64_t(bk) << BITS;  // first cell (directory entry) of the bucket
  // The bucket's piece of the ranked directory (grid.hpp, CellDir): its WORDS words, and the begins of
  // its occupied cells in id order at slots[sb ...], closed by the next bucket's first point. A bucket
  // has at most as many occupied cells as points, so sb = s + bk leaves every bucket room for its
  // cells and the closing entry. Every word is written on every step (the arena is reused).
  constexpr int WORDS = CELLS / 32;
  DirWord* const wds = words + size_t(bk) * WORDS;
  const uint32_t sb = uint32_t(s) + uint32_t(bk);
  if (s == e) {  // nothing in the bucket: whatever is looked up in it reads "the next point is s"
    if (t < WORDS) wds[t] = DirWord{0u, sb};
    if (t == 0) slots[sb] = s;
    return;
  }
  if (e - s <= 64) {
    // A wave's worth of points (two buckets in three on a forest: the grid's box is mostly air): no
    // counters, no scan. Wave 0 ranks the points against each other, key by key, and places them; the
    // occupied cells are the distinct cells of those points, found in key order through LDS; a thread
    // per directory word then collects its bits and its base from that list. (3 642 buckets of the 1 M-point
    // forest's grid took 13.5 us when all were empty, 28.6 us with eleven points each through the
    // counters: what a block pays for the counters, not the bytes, was the cost of these buckets.)
    int32_t* const cells = L.cnt;       // [64] the points' cells in key order
    int32_t* const dcell = L.cnt + 64;  // [<= 64] the distinct ones, ascending
    const int m = e - s;
    if (t < 64) {
      const bool live = t < m;
      const int lk = live ? keyb[s + t] & (8 * CELLS - 1) : 0;
      Rec p = {};
      if (live) p = bucketed[s + t];
      int below_key = 0, below_cell = 0;
      unsigned long long oc = 0ull;  // the octant counts of this point's cell
      for (int q = 0; q < m; ++q) {  // wave-uniform
        const int kq = __builtin_amdgcn_readlane(lk, q);
        below_key += (kq < lk || (kq == lk && q < t)) ? 1 : 0;
        below_cell += (kq >> 3) < (lk >> 3) ? 1 : 0;
        if ((kq >> 3) == (lk >> 3)) oc += 1ull << (8 * (kq & 7));
      }
      if (live) {
        const int cl = lk >> 3, o = lk & 7, b = s + below_cell;
        cells[below_key] = cl;
        out.put(s + below_key, rec_idx(p), int(c0) + cl, p.x, p.y, p.z, b * 8 + o);
        // the first point of its cell: the cell's sub-cell records
        if (below_key == below_cell) write_sub_records(rec, b, oc);
      }
    }
    __syncthreads();
    if (t < 64) {
      const bool live = t < m;
      // lane i now looks at the i-th point in key order: a cell begins where the cell changes, at
      // sorted position s + i, and its rank among the bucket's occupied cells is a ballot away
      const int ci = live ? cells[t] : -1;
      const bool head = live && (t == 0 || cells[t - 1] != ci);
      const unsigned long long hm = __ballot(head);
      const int rk = __popcll(hm & ((1ull << t) - 1ull));
      if (head) {
        slots[sb + rk] = s + t;
        dcell[rk] = ci;
      }
      if (t == 0) {
        slots[sb + __popcll(hm)] = e;
        L.wsum[0] = __popcll(hm);
      }
    }
    __syncthreads();
    if (t < WORDS) {
      const int nd = L.wsum[0];
      uint32_t bits = 0u, before = 0u;
      for (int q = 0; q < nd; ++q) {
        const int c = dcell[q];  // the same address in every lane
        before += c < 32 * t ? 1u : 0u;
        bits |= (c >> 5) == t ? 1u << (c & 31) : 0u;
      }
      wds[t] = DirWord{bits, sb + before};
    }
    return;
  }
  BkOctants<BITS, F32> P{L, s, e, c0, wds, slots, sb, rec, keyed, rank_tmp, out, 0u, 0, 0};
  bk_two_sweeps<BITS, F32>(P, s, e, bucketed, keyb, word_tmp);
  // Cells above kBkBig points (none on a scan at eps ~ 10 x the point spacing). Without such a cell nothing
  // more runs, and no kernel is launched for them.
  __syncthreads();  // the big cells' runs of `keyed` are written, L.any_big is final
  if (!L.any_big) return;  // block-uniform
  for (int wd = 0; wd < CELLS / 32; ++wd) {
    for (uint32_t bm = L.big[wd]; bm; bm &= bm - 1u) {  // block-uniform
      const int cl = wd * 32 + __ffs(bm) - 1;
      order_run_by_octant<T>(keyed, s + L.cnt[cl], s + (cl + 1 < CELLS ? L.cnt[cl + 1] : e - s), L.btot, L.bbase,
                             L.bw, out, rec);
    }
  }
  });
}

// ---- build_grid's policy: cells only, the dense directory ----------------------------------------------
// A count per cell is all there is, so a bucket of 2^BITS cells needs 4 bytes of LDS per cell, the arrival
// rank IS the place inside the cell, and no cell is too big. A point's word: the cell inside the bucket in
// the top BITS bits, below it the arrival rank, saturated (the exact value of a rank that does not fit goes
// through rank_tmp). The directory is the dense `start`, written as int4 pairs; beside the points the
// block adds up its occupied cells: occ[bucket] (count_occupied adds them up).
template <int BITS>
struct BkPlainLds {
  int32_t cnt[1 << BITS];
  int32_t wsum[16], wocc[16];
};

template <int BITS, bool F32>
struct BkPlain {
  static constexpr int CELLS = 1 << BITS, T = CELLS / 8, RB = 32 - BITS, RMAX = (1 << RB) - 1;
  using Rec = typename BkRec<F32>::type;
  BkPlainLds<BITS>& L;
  const int s, bk;
  const int64_t c0, ncell1;
  int32_t* const start;
  int32_t* const occ;
  int32_t* const rank_tmp;
  const SortedStore& out;

  __device__ __forceinline__ int32_t* cnt() const { return L.cnt; }
  __device__ __forceinline__ void clear(int t) const {
#pragma unroll
    for (int k = 0; k < 8; ++k) L.cnt[k * T + t] = 0;
  }
  __device__ __forceinline__ uint32_t rank_of(uint32_t ky, int j) const {
    const int cl = int(ky >> 3) & (CELLS - 1);
    const int rr = atomicAdd(&L.cnt[cl], 1);
    if (rr >= RMAX) rank_tmp[j] = rr;
    return (uint32_t(cl) << RB) | uint32_t(rr < RMAX ? rr : RMAX);
  }
  __device__ __forceinline__ int32_t scan(const int32_t (&v)[8], int32_t tot, int t) const {
    int32_t nocc = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) nocc += v[k] > 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nocc += __shfl_down(nocc, off, 64);
    if ((t & 63) == 0) L.wocc[t >> 6] = nocc;
    const int32_t run = block_excl_scan<T>(tot, L.wsum);
    if (t == 0) {
      int o = 0;
      for (int q = 0; q < T / 64; ++q) o += L.wocc[q];
      occ[bk] = o;
    }
    return run;
  }
  __device__ __forceinline__ void directory(const int32_t (&)[8], const int32_t (&pre)[8], int t) const {
    const int64_t cidx = c0 + 8 * t;
    if (cidx + 7 < ncell1) {
      *reinterpret_cast<int4*>(start + cidx) = make_int4(s + pre[0], s + pre[1], s + pre[2], s + pre[3]);
      *reinterpret_cast<int4*>(start + cidx + 4) = make_int4(s + pre[4], s + pre[5], s + pre[6], s + pre[7]);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (cidx + k < ncell1) start[cidx + k] = s + pre[k];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) L.cnt[8 * t + k] = pre[k];
  }
  __device__ __forceinline__ void place(const Rec& p, uint32_t w, int j) const {
    const int cl = int(w >> RB), arr = int(w & uint32_t(RMAX));
    out.put(s + L.cnt[cl] + (arr < RMAX ? arr : rank_tmp[j]), rec_idx(p), int(c0) + cl, p.x, p.y, p.z);
  }
};

template <int BITS, bool F32>
__global__ __launch_bounds__((1 << BITS) / 8, BITS == 12 ? 6 : 4) void k_bk_sort_plain(
    int64_t ncell1, const int32_t* __restrict__ bstart, const typename BkRec<F32>::type* __restrict__ bucketed,
    const int32_t* __restrict__ keyb, uint32_t* __restrict__ word_tmp, int32_t* __restrict__ rank_tmp,
    int32_t* __restrict__ start, int32_t* __restrict__ order,
    int32_t* __restrict__ cell_of, double* __restrict__ sx, double* __restrict__ sy, double* __restrict__ sz,
    float4* __restrict__ p4 /*non-null: fp32 records instead of sx / sy / sz*/, int32_t* __restrict__ occ) {
  constexpr int T = (1 << BITS) / 8;
  __shared__ BkPlainLds<BITS> L;
  const SortedStore out{order, cell_of, nullptr, F32 ? p4 : nullptr, sx, sy, sz};
  const int bk = blockIdx.x, t = threadIdx.x;
  const int s = bstart[bk], e = bstart[bk + 1];
  const int64_t c0 = int64_t(bk) << BITS;
  if (s == e) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int64_t cidx = c0 + int64_t(k * T + t) * 4;
      if (cidx + 3 < ncell1) {
        *reinterpret_cast<int4*>(start + cidx) = make_int4(s, s, s, s);
      } else {
        for (int u = 0; u < 4; ++u)
          if (cidx + u < ncell1) start[cidx + u] = s;
      }
    }
    if (t == 0) occ[bk] = 0;
    return;
  }
  BkPlain<BITS, F32> P{L, s, bk, c0, ncell1, start, occ, rank_tmp, out};
  bk_two_sweeps<BITS, F32>(P, s, e, bucketed, keyb, word_tmp);
}

// build_grid through the two-level sort; returns false (nothing launched) when the directory has
// more buckets than the A passes' LDS histogram holds or PYQSM_GRID_BIN=atomic asks for the
// one-atomic-per-point path.
static bool bucketed_fits(const DevGrid& g) {
  const char* env = getenv("PYQSM_GRID_BIN");
  return bucket_shape(g.ncell).nbk <= kBkMax && !(env && !strcmp(env, "atomic"));
}

// launch(Sort<BITS, F32>{}) for the bucket size and the record form of a second-level launch
template <int BITS_, bool F32_>
struct Sort {
  static constexpr int BITS = BITS_;
  static constexpr bool F32 = F32_;
  using Rec = typename BkRec<F32_>::type;
};
template <class F>
static void on_sort_shape(int bits, bool f32, F&& launch) {
  if (bits == 12) {
    if (f32)
      launch(Sort<12, true>{});
    else
      launch(Sort<12, false>{});
  } else {
    if (f32)
      launch(Sort<13, true>{});
    else
      launch(Sort<13, false>{});
  }
}

// the A passes; `bucketed` holds float4 (f32) or PointRec records
static void enqueue_bk_a(Ctx* c, int mode, bool f32, const double* xyz, int64_t n, const GridParams& gp,
                         const int raw[3], AxisMap am, int64_t nbk, int bits, int32_t* key_tmp, int32_t* tot,
                         int32_t* cursor, int32_t* bstart, void* bucketed, int32_t* keyb, const GridPlan* d_plan,
                         const PlanFold& pf = PlanFold{}) {
  const dim3 ga(ceil_div(n, kBkPts)), blk(256);
  const dim3 gh(ga.x + (pf.part ? 1 : 0));  // (the block that stores the folded plan)
  const size_t lds = size_t(nbk) * 4;
  const int fused = nbk <= kBkFusedScan;
#define PQ_BK_HIST(MODE)                                                                                         \
  hipLaunchKernelGGL(k_bk_hist<MODE>, gh, blk, lds, c->stream, xyz, n, gp, raw[0], raw[1], raw[2], am, int(nbk), \
                     bits, key_tmp, tot, d_plan, pf)
  if (mode == 0)
    PQ_BK_HIST(0);
  else if (mode == 1)
    PQ_BK_HIST(1);
  else
    PQ_BK_HIST(2);
#undef PQ_BK_HIST
  if (!fused) hipLaunchKernelGGL(k_bk_scan, dim3(1), dim3(1024), 0, c->stream, int(nbk), tot, bstart, d_plan);
  if (f32)
    hipLaunchKernelGGL(k_bk_scatter<true>, ga, blk, fused ? 2 * lds : lds, c->stream, xyz, n, int(nbk), bits,
                       key_tmp, tot, cursor, bstart, fused, static_cast<float4*>(bucketed), keyb, d_plan);
  else
    hipLaunchKernelGGL(k_bk_scatter<false>, ga, blk, fused ? 2 * lds : lds, c->stream, xyz, n, int(nbk), bits,
                       key_tmp, tot, cursor, bstart, fused, static_cast<PointRec*>(bucketed), keyb, d_plan);
}

static int build_grid_bucketed(Ctx* c, const double* xyz, int64_t n, DevGrid* g) {
  const int bits = bucket_shape(g->ncell).bits;
  const int64_t nbk = bucket_shape(g->ncell).nbk;
  const bool f32 = g->p4 != nullptr;  // float4 records in, float4 records out
  int32_t *tot, *bstart, *cursor, *key_tmp, *keyb, *rank_tmp;
  uint32_t* word_tmp;
  void* bucketed;
  PQ_TRY(c->arena.get(size_t(nbk) * 2, &tot));  // totals, then the reservation cursors: one memset
  cursor = tot + nbk;
  PQ_TRY(c->arena.get(size_t(nbk) + 1, &bstart));
  PQ_TRY(c->arena.get(size_t(n), &key_tmp));
  PQ_TRY(c->arena.get(size_t(n), &keyb));
  PQ_TRY(c->arena.get(size_t(n), &word_tmp));
  PQ_TRY(c->arena.get(size_t(n), &rank_tmp));
  if (f32) {
    float4* b4;
    PQ_TRY(c->arena.get(size_t(n), &b4));
    bucketed = b4;
  } else {
    PointRec* b8;
    PQ_TRY(c->arena.get(size_t(n), &b8));
    bucketed = b8;
  }
  g->occ_blocks = int(nbk);
  PQ_TRY(c->arena.get(size_t(nbk), &g->occ_part));
  PQ_HIP(hipMemsetAsync(tot, 0, size_t(nbk) * 8, c->stream));
  const int raw[3] = {0, 0, 0};
  enqueue_bk_a(c, 2, f32, xyz, n, grid_params(*g), raw, AxisMap{nullptr, nullptr, nullptr}, nbk, bits, key_tmp, tot,
               cursor, bstart, bucketed, keyb, nullptr);
  on_sort_shape(bits, f32, [&](auto S) {
    using K = decltype(S);
    hipLaunchKernelGGL((k_bk_sort_plain<K::BITS, K::F32>), dim3(unsigned(nbk)), dim3((1 << K::BITS) / 8), 0, c->stream,
                       g->ncell + 1, bstart, static_cast<const typename K::Rec*>(bucketed), keyb, word_tmp, rank_tmp,
                       g->start, g->order, g->cell_of, g->sx, g->sy, g->sz, g->p4, g->occ_part);
  });
  PQ_HIP(hipGetLastError());
  return 0;
}

// ---- DBSCAN's grid plan ---------------------------------------------------------------------------

// bin_octants_host's first trial: interior_slabs and bucket_shape are the host's own, so that every
// point lands in the same cell
__device__ GridPlan make_plan(const unsigned long long* box, const PlanIn& in) {
  GridPlan p;
  bool ok = in.hint.valid != 0;
  for (int a = 0; a < 3; ++a) {
    p.mn[a] = ord_val(box[a]);
    p.mx[a] = ord_val(box[3 + a]);
    ok = ok && isfinite(p.mn[a]) && isfinite(p.mx[a]);
  }
  p.all_f32 = box[6] != 0 ? 1 : 0;
  ok = ok && p.all_f32;
  double tot;
  int raw[3];
  ok = interior_slabs(p.mn, p.mx, in.cell, 2.0, raw, &tot) && ok;
  ok = ok && tot <= double(in.max_cells);  // beyond: compressed axes or a doubled cell, which the host plans
  p.inv_cell = 1.0 / in.cell;
  p.rx = raw[0];
  p.ry = raw[1];
  p.rz = raw[2];
  p.nx = raw[0] + 2;
  p.ny = raw[1] + 2;
  p.nz = raw[2] + 2;
  const int64_t ncell = ok ? int64_t(p.nx) * p.ny * p.nz : 0;
  const BucketShape bs = bucket_shape(ncell);
  const int64_t nbk = bs.nbk;
  ok = ok && bs.bits == 12 && ncell <= in.hint.ncell && nbk <= in.hint.nbk &&
       (nbk <= kBkFusedScan) == (in.hint.fused != 0);
  p.ncell = ok ? int(ncell) : 0;
  p.nbk = ok ? int(nbk) : 0;
  p.bits = 12;
  p.ok = ok ? 1 : 0;
  p.seq = in.seq;
  return p;
}

// ... and where it goes: d_plan for the kernels behind the next kernel boundary, the host's slot for wait_plan
__device__ void store_plan(GridPlan p, const PlanIn& in, GridPlan* __restrict__ plan) {
  *plan = p;
  if (in.host) {
    // the host polls the sequence number: everything else first, visible to the host before it
    // (one system-scope release, by one thread of the one folding block)
    p.seq = 0;
    *in.host = p;
    __threadfence_system();
    *reinterpret_cast<volatile unsigned*>(&in.host->seq) = in.seq;
  }
}

int plan_grid_device(Ctx* c, const double* xyz, int64_t n, double cell, int64_t max_cells, const PlanHint& hint,
                     GridPlan* d_plan, GridPlan* h_plan, unsigned seq, int32_t* zero_buf, int zero_n,
                     PlanRecords* speculated) {
  if (n <= 0) return fail(PYQSM_EINVAL, "bounding box of an empty cloud");
  const int blocks = bbox_blocks(c, n);
  unsigned long long *d_box = nullptr, *d_part = nullptr;
  PQ_TRY(c->arena.get(kBoxVals, &d_box));
  PQ_TRY(c->arena.get(size_t(blocks) * kBoxVals, &d_part));
  hipLaunchKernelGGL(k_bbox, dim3(blocks), dim3(256), 0, c->stream, xyz, n, d_part, zero_buf, zero_n,
                     stamp_slots(c, blocks));
  if (speculated)
    *speculated = PlanRecords{d_part, blocks, max_cells, h_plan, seq};
  else
    hipLaunchKernelGGL(k_bbox_fold, dim3(1), dim3(256), 0, c->stream, d_part, blocks, d_box,
                       PlanIn{cell, max_cells, hint, h_plan, seq}, d_plan);
  PQ_HIP(hipGetLastError());
  return 0;
}

// layout: [kBkMax totals | kBkMax reservation cursors | big-cell counter | four zeros for the caller
// | kZeroedExtra more]
int octant_zeroed_ints() { return 2 * kBkMax + 5 + kZeroedExtra; }

// The output arrays of the octant binning and the two-level sort's launches, for a directory of at
// most ncell cells in nbk buckets (the plan's exact numbers, or the hint's bounds); the kernels
// read the grid itself from d_plan.
static int enqueue_bucketed(Ctx* c, const double* xyz, int64_t n, const GridParams& gp, const int raw[3],
                            AxisMap am, bool mapped, int64_t nbk, int bits, bool f32,
                            int32_t* zeroed, const GridPlan* d_plan, DevGrid* g, SubCells* sub,
                            const PlanFold& pf = PlanFold{}) {
  int32_t *cell_tmp, *keyb, *rank_tmp, *bstart;
  uint32_t* word_tmp;
  int32_t *tot = zeroed, *cursor = zeroed + kBkMax;
  PointRec* keyed;
  void* bucketed;
  g->p4 = nullptr;
  g->sx = g->sy = g->sz = nullptr;
  // the ranked directory (grid.hpp, CellDir) instead of a dense start[ncell + 1]: a word per 32 cells of
  // every bucket, and a slot per occupied cell plus one per bucket
  g->start = nullptr;
  PQ_TRY(c->arena.get(size_t(nbk) << (bits - 5), &g->dir_words));
  PQ_TRY(c->arena.get(size_t(n) + size_t(nbk) + 1, &g->dir_slots));
  PQ_TRY(c->arena.get(size_t(n), &g->order));
  PQ_TRY(c->arena.get(size_t(n), &g->cell_of));
  if (f32) {
    float4* b4;
    PQ_TRY(c->arena.get(size_t(n), &g->p4));
    PQ_TRY(c->arena.get(size_t(n), &b4));
    bucketed = b4;
  } else {
    PointRec* b8;
    PQ_TRY(c->arena.get(size_t(n), &g->sx));
    PQ_TRY(c->arena.get(size_t(n), &g->sy));
    PQ_TRY(c->arena.get(size_t(n), &g->sz));
    PQ_TRY(c->arena.get(size_t(n), &b8));
    bucketed = b8;
  }
  PQ_TRY(c->arena.get(size_t(n), &cell_tmp));
  PQ_TRY(c->arena.get(size_t(n), &keyb));
  PQ_TRY(c->arena.get(size_t(n), &word_tmp));
  PQ_TRY(c->arena.get(size_t(n), &rank_tmp));
  PQ_TRY(c->arena.get(size_t(n), &keyed));
  PQ_TRY(c->arena.get(size_t(n), &sub->sub_of));
  PQ_TRY(c->arena.get(size_t(n) * 8, &sub->rec));
  PQ_TRY(c->arena.get(size_t(nbk) + 1, &bstart));
  enqueue_bk_a(c, mapped ? 1 : 0, f32, xyz, n, gp, raw, am, nbk, bits, cell_tmp, tot, cursor, bstart, bucketed, keyb,
               d_plan, pf);
  on_sort_shape(bits, f32, [&](auto S) {
    using K = decltype(S);
    unsigned long long* const st_sort = stamp_slots(c, nbk);  // the binning's last kernel
    hipLaunchKernelGGL((k_bk_sort<K::BITS, K::F32>), dim3(unsigned(nbk)), dim3((1 << K::BITS) / 8), 0, c->stream,
                       bstart, static_cast<const typename K::Rec*>(bucketed), keyb, word_tmp, rank_tmp, g->dir_words,
                       g->dir_slots, g->order, g->cell_of, sub->sub_of, g->sx, g->sy, g->sz, g->p4, sub->rec, keyed,
                       d_plan, st_sort);
  });
  PQ_HIP(hipGetLastError());
  return 0;
}

// The ranked directory from a dense one (the atomic binning and grids beyond kBkMax buckets, which still
// count into start[ncell + 1]): the per-bucket rule of k_bk_sort applied per word. Word w owns the slots
// from start[32 w] + w: the begins of its occupied cells, then start[32 w + 32], the begin of whatever
// comes next. A word has at most as many occupied cells as points, so the ranges do not overlap, and no
// scan is needed. A thread per cell, two words per wave.
__global__ __launch_bounds__(256) void k_dir_from_dense(int64_t ncell, const int32_t* __restrict__ start,
                                                        DirWord* __restrict__ words, int32_t* __restrict__ slots) {
  const int64_t c = int64_t(blockIdx.x) * 256 + threadIdx.x;  // the launch covers whole words
  const int lane = threadIdx.x & 63, half = lane >> 5;
  const int a = start[c < ncell ? c : ncell];
  const int b = start[c + 1 < ncell ? c + 1 : ncell];
  const uint32_t bits = uint32_t(__ballot(b != a) >> (32 * half));
  const int64_t w = c >> 5;
  const uint32_t base = uint32_t(__shfl(a, half * 32, 64)) + uint32_t(w);
  if (w > (ncell >> 5)) return;  // (the launch's last block may reach past the last word)
  if (b != a) slots[base + __popc(bits & ((1u << (lane & 31)) - 1u))] = a;
  if ((lane & 31) == 31) slots[base + __popc(bits)] = b;
  if ((lane & 31) == 0) words[w] = DirWord{bits, base};
}

static int dir_from_dense(Ctx* c, int64_t n, DevGrid* g) {
  const int64_t nwords = (g->ncell >> 5) + 1;
  PQ_TRY(c->arena.get(size_t(nwords), &g->dir_words));
  PQ_TRY(c->arena.get(size_t(n) + size_t(nwords) + 1, &g->dir_slots));
  hipLaunchKernelGGL(k_dir_from_dense, dim3(unsigned(ceil_div(nwords * 32, 256))), dim3(256), 0, c->stream, g->ncell,
                     g->start, g->dir_words, g->dir_slots);
  PQ_HIP(hipGetLastError());
  return 0;
}

__global__ __launch_bounds__(256) void k_read_directory(int64_t ncell, const CellDir dir,
                                                        int32_t* __restrict__ out) {
  const int64_t c = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (c <= ncell) out[c] = dir.begin(int(c));
}

void read_directory(Ctx* c, const DevGrid& g, int64_t ncell, int32_t* begin_out) {
  hipLaunchKernelGGL(k_read_directory, dim3(unsigned(ceil_div(ncell + 1, 256))), dim3(256), 0, c->stream, ncell,
                     cell_dir(g), begin_out);
}

int bin_octants_planned(Ctx* c, const double* xyz, int64_t n, double cell, const PlanHint& hint,
                        const PlanRecords& rec, GridPlan* d_plan, int32_t* zeroed, DevGrid* g, SubCells* sub) {
  // the host knows the edge (never doubled on this path) and the bounds of the directory, not its shape
  g->minx = g->miny = g->minz = 0.0;
  g->cell = cell;
  g->inv_cell = 1.0 / cell;
  g->nx = g->ny = g->nz = 0;
  g->ncell = hint.ncell;
  sub->zeroed4 = zeroed + 2 * kBkMax + 1;
  const int raw[3] = {0, 0, 0};
  return enqueue_bucketed(c, xyz, n, GridParams{}, raw, AxisMap{nullptr, nullptr, nullptr}, false, hint.nbk, 12,
                          true, zeroed, d_plan, g, sub,
                          PlanFold{rec.part, rec.blocks, PlanIn{cell, rec.max_cells, hint, rec.h_plan, rec.seq}, d_plan});
}

static int upload_plan(Ctx* c, const GridPlan& p, GridPlan* h_up, GridPlan* d_plan) {
  *h_up = p;  // the previous call's upload has run: the host waited on an event recorded after it
  PQ_TRY(copy_in(c, d_plan, h_up, 1));
  return 0;
}

// Extents that would need more than `max_cells` cells of edge `min_cell` are first COMPRESSED
// per axis: runs of empty slabs collapse to one empty slab, which keeps exactly the adjacencies
// the 27-cell stencil and the sub-cell offsets use (two points in neighbouring slabs stay in
// neighbouring slabs, all others end up at least one empty slab apart). Only if the compressed
// grid is still too large is the edge doubled (g->cell > min_cell tells the caller).
int bin_octants_host(Ctx* c, const double* xyz, int64_t n, double min_cell, int64_t max_cells, const GridPlan& box,
                     int32_t* zeroed, GridPlan* h_up, GridPlan* d_plan, DevGrid* g, SubCells* sub,
                     PlanHint* hint_out) {
  *hint_out = PlanHint{};
  if (n <= 0) return fail(PYQSM_EINVAL, "build_grid_octants: empty cloud");
  if (n > (int64_t(1) << 27)) return fail(PYQSM_ERANGE, "octant sub-cells: more than 2^27 points");
  if (max_cells > (int64_t(1) << 28)) max_cells = int64_t(1) << 28;  // cell * 8 + octant in 31 bits
  if (!(min_cell > 0) || !std::isfinite(min_cell))
    return fail(PYQSM_EINVAL, "cell edge must be positive and finite");
  double mn[3], mx[3];
  for (int a = 0; a < 3; ++a) {
    mn[a] = box.mn[a];
    mx[a] = box.mx[a];
    if (!std::isfinite(mn[a]) || !std::isfinite(mx[a])) return fail(PYQSM_EINVAL, "point coordinates must be finite");
  }
  bool all_f32 = box.all_f32 != 0;
  sub->zeroed4 = zeroed + 2 * kBkMax + 1;
  GridPlan hp{};
  {
    const char* f32_env = getenv("PYQSM_COORD_F32");  // "0": keep fp64 storage (A/B comparisons)
    if (f32_env && !strcmp(f32_env, "0")) all_f32 = false;
  }
  const char* bin_env = getenv("PYQSM_DBSCAN_BIN");
  const dim3 grid(ceil_div(n, 256)), blk(256);
  double cell = min_cell;
  int raw[3], dims[3];
  AxisMap am{nullptr, nullptr, nullptr};
  bool mapped = false;
  for (;;) {
    double tot;
    const bool ok = interior_slabs(mn, mx, cell, 2.0, raw, &tot);
    for (int a = 0; a < 3; ++a) dims[a] = raw[a] + 2;
    if (ok && tot <= double(max_cells)) break;
    // too many cells of this edge: drop the empty slabs (per axis) before giving up on the edge
    const int64_t raw_sum = ok ? int64_t(raw[0]) + raw[1] + raw[2] : int64_t(1) << 40;
    if (raw_sum <= (int64_t(1) << 27)) {
      GridParams gp{mn[0], mn[1], mn[2], 1.0 / cell, 0, 0, 0};
      int32_t* occ[3];
      int32_t* map[3];
      for (int a = 0; a < 3; ++a) {
        PQ_TRY(c->arena.get(size_t(raw[a]) + 1, &occ[a]));
        PQ_TRY(c->arena.get(size_t(raw[a]) + 1, &map[a]));
        PQ_HIP(hipMemsetAsync(occ[a], 0, (size_t(raw[a]) + 1) * 4, c->stream));
      }
      hipLaunchKernelGGL(k_axis_occ, grid, blk, 0, c->stream, xyz, n, gp, raw[0], raw[1], raw[2], occ[0],
                         occ[1], occ[2]);
      double ctot = 1.0;
      for (int a = 0; a < 3; ++a) {
        hipLaunchKernelGGL(k_axis_keep, dim3(ceil_div(raw[a] + 1, 256)), blk, 0, c->stream, raw[a], occ[a],
                           map[a]);
        PQ_HIP(hipGetLastError());
        PQ_TRY(exclusive_scan_i32(c, map[a], int64_t(raw[a]) + 1));
        int32_t kept = 0;
        PQ_TRY(fetch(c, &kept, map[a] + raw[a]));
        hipLaunchKernelGGL(k_axis_shift, dim3(ceil_div(raw[a], 256)), blk, 0, c->stream, raw[a], map[a]);
        dims[a] = kept + 2;
        ctot *= double(dims[a]);
      }
      PQ_HIP(hipGetLastError());
      if (ctot <= double(max_cells)) {
        am = AxisMap{map[0], map[1], map[2]};
        mapped = true;
        break;
      }
    }
    cell *= 2.0;
  }
  g->minx = mn[0];
  g->miny = mn[1];
  g->minz = mn[2];
  g->cell = cell;
  g->inv_cell = 1.0 / cell;
  g->nx = dims[0];
  g->ny = dims[1];
  g->nz = dims[2];
  g->ncell = int64_t(dims[0]) * dims[1] * dims[2];
  // Two-level counting sort (k_bk_*): no scattered global atomics, the directory written once.
  // PYQSM_DBSCAN_BIN=atomic keeps round 2's one-atomic-per-point path (A/B comparisons); grids of
  // more than kBkMax buckets (2^27 cells) keep it too.
  const int bits = bucket_shape(g->ncell).bits;
  const int64_t nbk = bucket_shape(g->ncell).nbk;
  const bool bucketed_path = nbk <= kBkMax && !(bin_env && !strcmp(bin_env, "atomic"));
  for (int a = 0; a < 3; ++a) {
    hp.mn[a] = mn[a];
    hp.mx[a] = mx[a];
  }
  hp.inv_cell = g->inv_cell;
  hp.nx = dims[0];
  hp.ny = dims[1];
  hp.nz = dims[2];
  hp.rx = raw[0];
  hp.ry = raw[1];
  hp.rz = raw[2];
  hp.ncell = int(g->ncell);
  hp.nbk = int(nbk);
  hp.bits = bits;
  hp.all_f32 = all_f32 && bucketed_path;  // fp32 records (round 2's path keeps fp64 arrays)
  hp.ok = 1;
  PQ_TRY(upload_plan(c, hp, h_up, d_plan));
  const GridParams gp = grid_params(*g);
  if (bucketed_path) {
    PQ_TRY(enqueue_bucketed(c, xyz, n, gp, raw, am, mapped, nbk, bits, hp.all_f32, zeroed, d_plan, g, sub));
    // the kind of grid the bounding box's fold can plan: a hint with some headroom on the directory
    // (the same bucket size and the same side of the fused-scan threshold)
    if (!mapped && cell == min_cell && bits == 12 && hp.all_f32) {
      int64_t ncell_h = std::min<int64_t>(g->ncell + g->ncell / 16, (int64_t(kBkMax) << 12) - 1);
      if (nbk <= kBkFusedScan) ncell_h = std::min<int64_t>(ncell_h, (int64_t(kBkFusedScan) << 12) - 1);
      hint_out->valid = 1;
      hint_out->ncell = int(ncell_h);
      hint_out->nbk = int(bucket_shape(ncell_h).nbk);  // (bits = 12 for every ncell_h below the bound above)
      hint_out->fused = nbk <= kBkFusedScan;
    }
    return 0;
  }
  int32_t *cell_tmp, *rank_tmp, *big_list, *big_cnt = zeroed + 2 * kBkMax;
  PointRec* keyed;
  g->p4 = nullptr;
  PQ_TRY(c->arena.get(size_t(g->ncell) + 1, &g->start));
  PQ_TRY(c->arena.get(size_t(n), &g->order));
  PQ_TRY(c->arena.get(size_t(n), &g->cell_of));
  PQ_TRY(c->arena.get(size_t(n), &g->sx));
  PQ_TRY(c->arena.get(size_t(n), &g->sy));
  PQ_TRY(c->arena.get(size_t(n), &g->sz));
  PQ_TRY(c->arena.get(size_t(n), &cell_tmp));
  PQ_TRY(c->arena.get(size_t(n), &rank_tmp));
  PQ_TRY(c->arena.get(size_t(n), &keyed));
  PQ_TRY(c->arena.get(size_t(n), &sub->sub_of));
  PQ_TRY(c->arena.get(size_t(n) * 8, &sub->rec));
  PQ_TRY(c->arena.get(size_t(n) / kBigCell + 2, &big_list));
  PQ_HIP(hipMemsetAsync(g->start, 0, (size_t(g->ncell) + 1) * 4, c->stream));
  if (mapped)
    hipLaunchKernelGGL(k_cell_count_oct<true>, grid, blk, 0, c->stream, xyz, n, gp, raw[0], raw[1], raw[2],
                       am, g->start, cell_tmp, rank_tmp);
  else
    hipLaunchKernelGGL(k_cell_count_oct<false>, grid, blk, 0, c->stream, xyz, n, gp, raw[0], raw[1], raw[2],
                       am, g->start, cell_tmp, rank_tmp);
  PQ_HIP(hipGetLastError());
  PQ_TRY(exclusive_scan_i32(c, g->start, g->ncell + 1));
  hipLaunchKernelGGL(k_scatter_keys, grid, blk, 0, c->stream, xyz, n, g->start, cell_tmp, rank_tmp, keyed);
  hipLaunchKernelGGL(k_order_cells, grid, blk, 0, c->stream, int(n), g->start, keyed, g->order,
                     g->cell_of, sub->sub_of, g->sx, g->sy, g->sz, sub->rec, big_list, big_cnt);
  PQ_HIP(hipGetLastError());
  // cells with more than kBigCell points (none on a scan at eps ~ 10 x the point spacing): a fixed
  // grid reads their number on the device, so that no host round trip is needed
  hipLaunchKernelGGL(k_order_big, dim3(unsigned(std::min<int64_t>(n / kBigCell + 1, 2048))), blk, 0,
                     c->stream, big_list, big_cnt, g->start, keyed, g->order, g->cell_of, sub->sub_of,
                     g->sx, g->sy, g->sz, g->p4, sub->rec, d_plan);
  PQ_HIP(hipGetLastError());
  return dir_from_dense(c, n, g);
}

// ---- pyramid coarsening: a grid with cells `factor` times larger, without atomics ----
// Coarse cell C gathers the factor^3 fine cells of its block; their point runs are
// concatenated in (z, y, x) order, so a point's new position follows from its old one:
// coarse_start[C] + offset_of_its_fine_cell_in_C + (old position - fine_start[cell]).

struct Pyr {
  int fnx, fny, fnz, cnx, cny, cnz, factor;
};

__device__ __forceinline__ int coarse_of(const Pyr& P, int f) {
  const int fx = f % P.fnx, fy = (f / P.fnx) % P.fny, fz = f / (P.fnx * P.fny);
  // interior fine index i (1..n-2) holds coordinate i-1; borders stay borders
  auto m = [&](int i, int fn, int cn) {
    if (i <= 0) return 0;
    if (i >= fn - 1) return cn - 1;
    return (i - 1) / P.factor + 1;
  };
  const int cx = m(fx, P.fnx, P.cnx), cy = m(fy, P.fny, P.cny), cz = m(fz, P.fnz, P.cnz);
  return (cz * P.cny + cy) * P.cnx + cx;
}

__global__ __launch_bounds__(256) void k_pyr_counts(Pyr P, const int32_t* __restrict__ fstart,
                                                    int32_t* __restrict__ ccount,
                                                    int32_t* __restrict__ foff) {
  const int C = blockIdx.x * 256 + threadIdx.x;
  if (C >= P.cnx * P.cny * P.cnz) return;
  const int cx = C % P.cnx, cy = (C / P.cnx) % P.cny, cz = C / (P.cnx * P.cny);
  int run = 0;
  if (cx >= 1 && cy >= 1 && cz >= 1 && cx <= P.cnx - 2 && cy <= P.cny - 2 && cz <= P.cnz - 2) {
    const int x0 = (cx - 1) * P.factor + 1, y0 = (cy - 1) * P.factor + 1, z0 = (cz - 1) * P.factor + 1;
    if (P.factor == 4) {
      // the usual factor: the five run starts of a row of four fine cells are fetched together,
      // all sixteen rows' loads can be in flight at once (one cell at a time they were a chain of
      // 64 load-add-store steps: 0.36 ms for the 50 M-cell grid of a million points)
#pragma unroll
      for (int dz = 0; dz < 4; ++dz)
#pragma unroll
        for (int dy = 0; dy < 4; ++dy) {
          const int z = z0 + dz, y = y0 + dy;
          if (z > P.fnz - 2 || y > P.fny - 2) continue;
          const int f0 = (z * P.fny + y) * P.fnx + x0;
          const int nxr = min(4, P.fnx - 1 - x0);  // fine cells of this row inside the grid (>= 1)
          int s[5];
#pragma unroll
          for (int u = 0; u < 5; ++u) s[u] = fstart[f0 + min(u, nxr)];
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (u < nxr) foff[f0 + u] = run + (s[u] - s[0]);
          run += s[4] - s[0];  // s[4] = fstart[f0 + nxr]: the clamped index above
        }
    } else {
      for (int z = z0; z < z0 + P.factor && z <= P.fnz - 2; ++z)
        for (int y = y0; y < y0 + P.factor && y <= P.fny - 2; ++y)
          for (int x = x0; x < x0 + P.factor && x <= P.fnx - 2; ++x) {
            const int f = (z * P.fny + y) * P.fnx + x;
            foff[f] = run;
            run += fstart[f + 1] - fstart[f];
          }
    }
  }
  ccount[C] = run;
}

__global__ __launch_bounds__(256) void k_pyr_scatter(int n, Pyr P, const int32_t* __restrict__ fstart,
                                                     const int32_t* __restrict__ cstart,
                                                     const int32_t* __restrict__ foff,
                                                     const int32_t* __restrict__ f_cell_of,
                                                     const int32_t* __restrict__ f_order,
                                                     const double* __restrict__ fx,
                                                     const double* __restrict__ fy,
                                                     const double* __restrict__ fz,
                                                     const float4* __restrict__ fp4,
                                                     int32_t* __restrict__ order,
                                                     int32_t* __restrict__ cell_of,
                                                     double* __restrict__ sx,
                                                     double* __restrict__ sy,
                                                     double* __restrict__ sz, float4* __restrict__ p4) {
  const SortedStore out{order, cell_of, nullptr, p4, sx, sy, sz};
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int f = f_cell_of[p];
  const int C = coarse_of(P, f);
  const int q = cstart[C] + foff[f] + (p - fstart[f]);
  if (fp4) {
    const float4 v = fp4[p];  // (.w is 0 in every grid that is coarsened: build_grid's)
    out.put(q, f_order[p], C, v.x, v.y, v.z);
  } else {
    out.put(q, f_order[p], C, fx[p], fy[p], fz[p]);
  }
}

int coarsen_grid(Ctx* c, const DevGrid& fine, int64_t n, int factor, DevGrid* g) {
  if (factor < 2) return fail(PYQSM_EINVAL, "coarsen_grid: factor must be >= 2");
  Pyr P;
  P.factor = factor;
  P.fnx = fine.nx;
  P.fny = fine.ny;
  P.fnz = fine.nz;
  P.cnx = (fine.nx - 2 + factor - 1) / factor + 2;
  P.cny = (fine.ny - 2 + factor - 1) / factor + 2;
  P.cnz = (fine.nz - 2 + factor - 1) / factor + 2;
  *g = fine;
  g->occ_part = nullptr;  // the fine grid's occupancy does not describe this one
  g->occ_blocks = 0;
  g->nx = P.cnx;
  g->ny = P.cny;
  g->nz = P.cnz;
  g->cell = fine.cell * factor;
  g->inv_cell = 1.0 / g->cell;
  g->ncell = int64_t(P.cnx) * P.cny * P.cnz;
  int32_t* foff = nullptr;
  PQ_TRY(c->arena.get(size_t(fine.ncell) + 1, &foff));
  PQ_TRY(c->arena.get(size_t(g->ncell) + 1, &g->start));
  PQ_TRY(c->arena.get(size_t(n), &g->order));
  PQ_TRY(c->arena.get(size_t(n), &g->cell_of));
  if (fine.p4) {
    PQ_TRY(c->arena.get(size_t(n), &g->p4));
  } else {
    PQ_TRY(c->arena.get(size_t(n), &g->sx));
    PQ_TRY(c->arena.get(size_t(n), &g->sy));
    PQ_TRY(c->arena.get(size_t(n), &g->sz));
  }
  PQ_HIP(hipMemsetAsync(g->start + g->ncell, 0, 4, c->stream));
  hipLaunchKernelGGL(k_pyr_counts, dim3(ceil_div(g->ncell, 256)), dim3(256), 0, c->stream, P,
                     fine.start, g->start, foff);
  PQ_HIP(hipGetLastError());
  PQ_TRY(exclusive_scan_i32(c, g->start, g->ncell + 1));
  hipLaunchKernelGGL(k_pyr_scatter, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, int(n), P,
                     fine.start, g->start, foff, fine.cell_of, fine.order, fine.sx, fine.sy, fine.sz,
                     static_cast<const float4*>(fine.p4), g->order, g->cell_of, g->sx, g->sy, g->sz, g->p4);
  PQ_HIP(hipGetLastError());
  return 0;
}

int count_occupied(Ctx* c, const DevGrid& g, int64_t* occupied) {
  if (g.occ_part) {  // left by build_grid's counting pass
    std::vector<int32_t> h(size_t(g.occ_blocks));
    PQ_TRY(fetch(c, h.data(), g.occ_part, h.size()));
    int64_t t = 0;
    for (int32_t v : h) t += v;
    *occupied = t;
    return 0;
  }
  int32_t* d = nullptr;
  PQ_TRY(c->arena.get(1, &d));
  PQ_HIP(hipMemsetAsync(d, 0, 4, c->stream));
  const int blocks = int(std::min<int64_t>(ceil_div(g.ncell, 256), int64_t(c->cu_count) * 8));
  hipLaunchKernelGGL(k_count_occupied, dim3(blocks), dim3(256), 0, c->stream, g.start, g.ncell, d);
  PQ_HIP(hipGetLastError());
  int32_t h = 0;
  PQ_TRY(fetch(c, &h, d));
  *occupied = h;
  return 0;
}

// ---- what the fixed-radius kernels share (radius.hip, adjacency.hip) ---------------------------
// The grid of the source points: cells of the radius, over the cloud without its sparse tails (a few
// stray returns far outside would otherwise inflate the box until the dense grid cannot have cells
// of the radius any more — every doubling of the edge is 8x the points per cell).
// build_grid leaves the points of a cell in the order in which its binning's atomics arrived. A radius query
// that must choose among several points AT its k-th distance takes them in walk order, so that choice would
// differ from one grid build to the next (the region growing's host loop builds one per cycle). Here every
// cell's run is put in ascending ORIGINAL index: the stable radix sort (scan.hip, no global atomics) of
// (cell, index) pairs taken in index order. start and cell_of stay as they are; order and the coordinates
// are written again.
__global__ __launch_bounds__(256) void k_canon_keys(int n, const int32_t* __restrict__ order,
                                                    const int32_t* __restrict__ cell_of, uint32_t* __restrict__ key,
                                                    int32_t* __restrict__ ident) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  const int i = order[q];
  key[i] = uint32_t(cell_of[q]);
  ident[i] = i;
}

__global__ __launch_bounds__(256) void k_canon_gather(int n, const double* __restrict__ xyz,
                                                      const int32_t* __restrict__ sorted, int32_t* __restrict__ order,
                                                      double* __restrict__ sx, double* __restrict__ sy,
                                                      double* __restrict__ sz, float4* __restrict__ p4) {
  const SortedStore out{order, nullptr, nullptr, p4, sx, sy, sz};  // (start and cell_of stay as they are)
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  const int i = sorted[q];
  out.put(q, i, 0, xyz[3 * size_t(i)], xyz[3 * size_t(i) + 1], xyz[3 * size_t(i) + 2]);
}

static int canonical_cell_order(Ctx* c, const double* d_src, int64_t n, DevGrid* g) {
  uint32_t* key;
  int32_t* ident;
  PQ_TRY(c->arena.get(size_t(n), &key));
  PQ_TRY(c->arena.get(size_t(n), &ident));
  hipLaunchKernelGGL(k_canon_keys, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, int(n),
                     static_cast<const int32_t*>(g->order), static_cast<const int32_t*>(g->cell_of), key, ident);
  PQ_HIP(hipGetLastError());
  int bits = 1;
  while (bits < 32 && (int64_t(1) << bits) < g->ncell) ++bits;
  PQ_TRY(stable_sort_pairs_u32(c, &key, &ident, n, bits));
  hipLaunchKernelGGL(k_canon_gather, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, int(n), d_src,
                     static_cast<const int32_t*>(ident), g->order, g->sx, g->sy, g->sz, g->p4);
  PQ_HIP(hipGetLastError());
  return 0;
}

int ball_grid(Ctx* c, const double* d_src, int64_t n, double radius, DevGrid* g, double* cloud_box) {
  double box[6];
  bool all_f32 = false;  // every source coordinate fp32-representable: 16-byte fp32 records (grid.hpp: on_coords)
  PQ_TRY(cloud_bbox(c, d_src, n, box, box + 3, &all_f32));
  if (cloud_box)
    for (int a = 0; a < 6; ++a) cloud_box[a] = box[a];
  int64_t outside = 0;
  PQ_TRY(robust_box(c, d_src, n, int(std::min<int64_t>(8192, std::max<int64_t>(256, n / 256))), box, &outside));
  return build_grid(c, d_src, n, radius * (1.0 + 1.0 / 1048576.0), int64_t(1) << 28, g, box, all_f32);
}

int radius_grid(Ctx* c, const double* d_src, int64_t n, double radius, DevGrid* g) {
  PQ_TRY(ball_grid(c, d_src, n, radius, g));
  return canonical_cell_order(c, d_src, n, g);
}

// The queries in the order of the source grid's cells (round 3): a lane per query walks ~850 candidates of
// 27 cells, and 64 unrelated queries per wave are 64 unrelated walks — every load a gather of 64 lines.
// In cell order the lanes of a wave walk the same few runs and their loads fall on shared lines
// (100 k queries against 1 M sources: 4.8 -> 4.0 ms). Marks, labels (atomicMin) and the per-query
// counts do not depend on the order in which the queries are served.
__global__ __launch_bounds__(256) void k_query_keys(int m, const double* __restrict__ qry, GridParams g,
                                                    uint32_t* __restrict__ key, int32_t* __restrict__ ident) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  int cx, cy, cz;
  clamped_cell(g, qry[3 * i], qry[3 * i + 1], qry[3 * i + 2], &cx, &cy, &cz);
  key[i] = uint32_t((cz * g.ny + cy) * g.nx + cx);
  ident[i] = i;
}

int query_order(Ctx* c, const double* d_qry, int64_t m, const GridParams& rg, int64_t ncell, int32_t** perm) {
  *perm = nullptr;
  const char* e = getenv("PYQSM_RADIUS_SORT");  // "0": serve the queries in the caller's order
  if (m < 1024 || (e && e[0] == '0')) return 0;
  uint32_t* key;
  int32_t* ident;
  PQ_TRY(c->arena.get(size_t(m), &key));
  PQ_TRY(c->arena.get(size_t(m), &ident));
  hipLaunchKernelGGL(k_query_keys, dim3(ceil_div(m, 256)), dim3(256), 0, c->stream, int(m), d_qry, rg, key, ident);
  PQ_HIP(hipGetLastError());
  int bits = 1;
  while (bits < 32 && (int64_t(1) << bits) < ncell) ++bits;
  PQ_TRY(stable_sort_pairs_u32(c, &key, &ident, m, bits));
  *perm = ident;
  return 0;
}

}  // namespace pyqsm
