// pdist.hip — order statistics of the pairwise distances of a point set, without the distances.
//   pyqsm_pdist_select   for every segment (an independent cloud of 2-D or 3-D points) the elements
//                        of given ranks of the sorted scipy.spatial.distance.pdist, and the pair that
//                        attains the maximum: what pyQSM's canopy_metrics.width_at_height reads off
//                        np.percentile(pdist(slab[:, :2]), q). DESIGN.md section 21.
// A radix selection over keys that are recomputed from the points in every pass: the key of a pair
// is the bit pattern of d2 = (dx*dx) + (dy*dy) [+ (dz*dz)], a non-negative double, which orders as
// an unsigned 64-bit integer. Eight passes of eight bits, most significant first. A pass counts, for
// every group (the ranks of a segment whose keys so far share a prefix), the pairs whose key
// carries the group's prefix by their next digit; a one-wave kernel per segment then turns each
// histogram into the next prefix and the remaining rank and regroups the ranks, on the device. All
// counters are integers summed by integer atomics: the same bits on every run.
#include "reduce.hpp"  // k_radix_select_update: a histogram becomes the next prefix, the ranks regroup

#include <algorithm>
#include <cmath>

namespace pyqsm {

using u64 = unsigned long long;

constexpr int kPdTile = 256;      // points per tile edge = threads per block
constexpr int kPdBins = 256;      // eight bits per pass
constexpr int kPdPasses = 8;
constexpr int kPdMaxRanks = PYQSM_PDIST_MAX_RANKS;
// a block's LDS counters are 32 bits wide: it hands them on before this many tiles of 2^16 pairs
constexpr int kPdFlushTiles = 16384;
static constexpr int64_t kPdDefaultMaxPairs = PYQSM_PDIST_DEFAULT_MAX_PAIRS;

// what a pass does besides counting: the first finds every segment's largest key, the second the
// smallest pair (i, j) that attains it
enum { kPdMaxKey = 0, kPdMaxPair = 1, kPdPlain = 2 };

// The segment of global tile t: the last s with tile0[s] <= t (segments without tiles share their
// successor's offset and are never found).
__device__ __forceinline__ int pd_find_seg(const int64_t* __restrict__ tile0, int n_seg, int64_t t) {
  int lo = 0, hi = n_seg;  // tile0[lo] <= t < tile0[hi]
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (tile0[mid] <= t) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Tile t of a segment's upper triangle, column by column: t = b (b + 1) / 2 + a with a <= b.
__device__ __forceinline__ void pd_decode_tile(int64_t t, int* a, int* b) {
  int64_t c = int64_t((sqrt(8.0 * double(t) + 1.0) - 1.0) * 0.5);
  while ((c + 1) * (c + 2) / 2 <= t) ++c;
  while (c * (c + 1) / 2 > t) --c;
  *b = int(c);
  *a = int(t - c * (c + 1) / 2);
}

// One pass. A block walks tiles_per_block consecutive tiles; thread `tid` owns row point a * 256 + tid
// and walks the column tile's points, which lie in LDS (every lane reads the same one: a broadcast).
// The digit of consecutive pairs changes rarely in the passes over the exponent bits, where nearly all
// pairs fall into a few bins: a run of equal bins is counted in a register and handed to the LDS
// histogram when it ends. The LDS histogram goes to the global one when the block leaves a segment.
template <int MODE, int DIM>
__global__ __launch_bounds__(kPdTile) void k_pdist_hist(
    const double* __restrict__ pts, const int64_t* __restrict__ seg_start, const int64_t* __restrict__ tile0,
    int n_seg, int64_t total_tiles, int64_t tiles_per_block, int n_ranks, int pass,
    const int32_t* __restrict__ gcount, const u64* __restrict__ gprefix, u64* __restrict__ hist,
    u64* __restrict__ seg_maxkey, u64* __restrict__ seg_maxpair) {
  extern __shared__ uint32_t s_hist[];  // [n_ranks][256]
  __shared__ double s_x[kPdTile], s_y[kPdTile], s_z[kPdTile];
  __shared__ u64 s_gp[kPdMaxRanks];
  __shared__ u64 s_best;
  const int tid = threadIdx.x;
  const int64_t t_begin = int64_t(blockIdx.x) * tiles_per_block;
  const int64_t t_end = t_begin + tiles_per_block < total_tiles ? t_begin + tiles_per_block : total_tiles;
  const int pre_shift = 63 - 8 * pass;  // prefix = (key >> 1) >> pre_shift: the top 8 * pass bits
  const int dig_shift = 56 - 8 * pass;

  int seg = -1, groups = 0, since_flush = 0;
  int64_t p0 = 0, ns = 0, seg_tile0 = 0, seg_tile1 = 0;
  u64 seg_max = 0;            // MODE kPdMaxPair: the segment's largest key
  u64 best = MODE == kPdMaxKey ? 0 : ~u64(0);  // this thread's largest key / smallest pair of the segment

  auto flush = [&]() {  // block-uniform
    if (MODE == kPdMaxKey) atomicMax(&s_best, best);
    if (MODE == kPdMaxPair && best != ~u64(0)) atomicMin(&s_best, best);
    __syncthreads();
    u64* h = hist + size_t(seg) * n_ranks * kPdBins;
    for (int k = tid; k < groups * kPdBins; k += kPdTile) {
      const uint32_t v = s_hist[k];
      if (v) {
        atomicAdd(&h[k], u64(v));
        s_hist[k] = 0;
      }
    }
    if (tid == 0) {
      if (MODE == kPdMaxKey) atomicMax(&seg_maxkey[seg], s_best);
      if (MODE == kPdMaxPair && s_best != ~u64(0)) atomicMin(&seg_maxpair[seg], s_best);
    }
    __syncthreads();
    since_flush = 0;
  };

  for (int64_t t = t_begin; t < t_end; ++t) {
    if (seg < 0 || t >= seg_tile1 || since_flush >= kPdFlushTiles) {
      if (seg >= 0) flush();
      if (seg < 0 || t >= seg_tile1) {
        seg = pd_find_seg(tile0, n_seg, t);
        p0 = seg_start[seg];
        ns = seg_start[seg + 1] - p0;
        seg_tile0 = tile0[seg];
        seg_tile1 = tile0[seg + 1];
        groups = gcount[seg];
        if (MODE == kPdMaxPair) seg_max = seg_maxkey[seg];
        if (tid < groups) s_gp[tid] = gprefix[size_t(seg) * n_ranks + tid];
        for (int k = tid; k < groups * kPdBins; k += kPdTile) s_hist[k] = 0;
      }
      best = MODE == kPdMaxKey ? 0 : ~u64(0);
      if (tid == 0) s_best = best;
      __syncthreads();
    }
    ++since_flush;
    int ta, tb;
    pd_decode_tile(t - seg_tile0, &ta, &tb);
    const int64_t j0 = int64_t(tb) * kPdTile, i = int64_t(ta) * kPdTile + tid;
    const int cols = ns - j0 < kPdTile ? int(ns - j0) : kPdTile;
    if (tid < cols) {
      const double* q = pts + (p0 + j0 + tid) * DIM;
      s_x[tid] = q[0];
      s_y[tid] = q[1];
      if (DIM == 3) s_z[tid] = q[2];
    }
    __syncthreads();
    const bool row = i < ns;
    double xi = 0.0, yi = 0.0, zi = 0.0;
    if (row) {
      const double* q = pts + (p0 + i) * DIM;
      xi = q[0];
      yi = q[1];
      if (DIM == 3) zi = q[2];
    }
    const bool diag = ta == tb;
    // on the diagonal j > i: a wave starts behind its first lane's own point
    int run_bin = -1;
    uint32_t run = 0;
    for (int jj = diag ? (tid & ~63) + 1 : 0; jj < cols; ++jj) {
      const double dx = xi - s_x[jj], dy = yi - s_y[jj];
      double d2 = (dx * dx) + (dy * dy);
      if (DIM == 3) {
        const double dz = zi - s_z[jj];
        d2 = d2 + (dz * dz);
      }
      if (!row || (diag && jj <= tid)) continue;
      const u64 key = u64(__double_as_longlong(d2));
      if (MODE == kPdMaxKey && key > best) best = key;
      if (MODE == kPdMaxPair && key == seg_max) {  // tiles come column by column: a later one may hold a smaller i
        const u64 pair = (u64(i) << 32) | u64(j0 + jj);
        if (pair < best) best = pair;
      }
      const u64 pre = (key >> 1) >> pre_shift;
      int bin = -1;
      for (int g = 0; g < groups; ++g)
        if (pre == s_gp[g]) bin = g * kPdBins + int((key >> dig_shift) & 255);
      if (bin < 0) continue;
      if (bin != run_bin) {
        if (run) atomicAdd(&s_hist[run_bin], run);
        run_bin = bin;
        run = 0;
      }
      ++run;
    }
    if (run) atomicAdd(&s_hist[run_bin], run);
    __syncthreads();  // the column points are replaced by the next tile's
  }
  if (seg >= 0) flush();
}

template <int MODE>
static int pd_launch_hist(Ctx* c, int dim, int grid, size_t lds, const double* pts, const int64_t* seg_start,
                          const int64_t* tile0, int n_seg, int64_t total_tiles, int64_t tiles_per_block, int n_ranks,
                          int pass, const int32_t* gcount, const u64* gprefix, u64* hist, u64* maxkey, u64* maxpair) {
  if (dim == 2)
    hipLaunchKernelGGL((k_pdist_hist<MODE, 2>), dim3(grid), dim3(kPdTile), lds, c->stream, pts, seg_start, tile0, n_seg,
                       total_tiles, tiles_per_block, n_ranks, pass, gcount, gprefix, hist, maxkey, maxpair);
  else
    hipLaunchKernelGGL((k_pdist_hist<MODE, 3>), dim3(grid), dim3(kPdTile), lds, c->stream, pts, seg_start, tile0, n_seg,
                       total_tiles, tiles_per_block, n_ranks, pass, gcount, gprefix, hist, maxkey, maxpair);
  PQ_HIP(hipGetLastError());
  return 0;
}

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_pdist_select(const double* pts, int64_t n, int32_t dim, const int64_t* seg_start, int64_t n_seg,
                       const int64_t* ranks, int32_t n_ranks, int64_t max_pairs, double* values, int64_t* n_pairs,
                       int64_t* max_pair, int64_t* stats, int32_t device) {
  PQ_API_RANGE("pyqsm_pdist_select");
  if (stats) std::fill(stats, stats + 3, int64_t(0));
  if (n < 0 || n_seg < 0) return fail(PYQSM_EINVAL, "negative size");
  if (dim != 2 && dim != 3) return fail(PYQSM_EINVAL, "pyqsm_pdist_select: dim = %d, must be 2 or 3", int(dim));
  if (n_ranks < 0 || n_ranks > kPdMaxRanks)
    return fail(PYQSM_EINVAL, "pyqsm_pdist_select: %d ranks per segment, at most %d", int(n_ranks), kPdMaxRanks);
  if (!seg_start || (n > 0 && !pts) || (n_seg > 0 && !n_pairs) || (n_seg > 0 && n_ranks > 0 && (!ranks || !values)))
    return fail(PYQSM_EINVAL, "pyqsm_pdist_select: NULL pointer");
  if (seg_start[0] != 0 || seg_start[n_seg] != n) return fail(PYQSM_EINVAL, "seg_start must run from 0 to n");
  for (int64_t s = 0; s < n_seg; ++s)
    if (seg_start[s + 1] < seg_start[s]) return fail(PYQSM_EINVAL, "seg_start must not decrease");
  if (n > 0x7FFFFF00LL || n_seg > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 points per call");
  if (max_pairs <= 0) max_pairs = kPdDefaultMaxPairs;

  const int R = std::max<int>(n_ranks, 1);  // slots per segment in the device tables
  std::vector<int64_t> tile0(size_t(n_seg) + 1, 0);
  std::vector<u64> remaining(size_t(n_seg) * R, 0);
  std::vector<int32_t> group(size_t(n_seg) * R, -1), gcount(size_t(n_seg), 0);
  unsigned __int128 sum_pairs = 0;
  bool any_rank = false;
  for (int64_t s = 0; s < n_seg; ++s) {
    const int64_t ns = seg_start[s + 1] - seg_start[s];
    const int64_t m = ns * (ns - 1) / 2;  // ns < 2^31
    n_pairs[s] = m;
    sum_pairs += (unsigned __int128)m;
    const int64_t nt = m > 0 ? (ns + kPdTile - 1) / kPdTile : 0;
    tile0[size_t(s) + 1] = tile0[size_t(s)] + nt * (nt + 1) / 2;
    if (max_pair) max_pair[2 * s] = max_pair[2 * s + 1] = -1;
    for (int r = 0; r < n_ranks; ++r) {
      const int64_t k = ranks[s * n_ranks + r];
      values[s * n_ranks + r] = 0.0;
      if (k < 0) continue;
      if (k >= m)
        return fail(PYQSM_EINVAL, "pyqsm_pdist_select: rank %lld of segment %lld, which has %lld pairs", (long long)k,
                    (long long)s, (long long)m);
      remaining[size_t(s) * R + r] = u64(k);
      group[size_t(s) * R + r] = 0;
      gcount[size_t(s)] = 1;
      any_rank = true;
    }
  }
  if (sum_pairs > (unsigned __int128)max_pairs)
    return fail(PYQSM_ERANGE,
                "pyqsm_pdist_select: %.4g point pairs exceed max_pairs = %lld (split the call, thin the cloud or raise "
                "max_pairs)",
                double(sum_pairs), (long long)max_pairs);
  const int64_t total_pairs = int64_t(sum_pairs), total_tiles = tile0[size_t(n_seg)];
  if (stats) stats[0] = total_pairs;
  if (total_pairs == 0) return 0;  // no segment has a pair: no device work
  const int passes = any_rank ? kPdPasses : (max_pair ? 2 : 0);
  if (passes == 0) return 0;

  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  const int64_t want_blocks = std::min<int64_t>(total_tiles, int64_t(c->cu_count) * 8);
  const int64_t tiles_per_block = (total_tiles + want_blocks - 1) / want_blocks;
  const int grid = int((total_tiles + tiles_per_block - 1) / tiles_per_block);
  const size_t slots = size_t(n_seg) * R, lds = size_t(R) * kPdBins * sizeof(uint32_t);

  double* d_pts;
  int64_t *d_seg, *d_tile0;
  u64 *d_state, *d_rem;  // prefix [slots], gprefix [slots], maxkey [n_seg], histograms: cleared together
  int32_t *d_group, *d_gcount;
  PQ_TRY(upload(c, pts, size_t(n) * dim, &d_pts));
  PQ_TRY(upload(c, seg_start, size_t(n_seg) + 1, &d_seg));
  PQ_TRY(upload(c, tile0.data(), size_t(n_seg) + 1, &d_tile0));
  PQ_TRY(upload(c, remaining.data(), slots, &d_rem));
  PQ_TRY(upload(c, group.data(), slots, &d_group));
  PQ_TRY(upload(c, gcount.data(), size_t(n_seg), &d_gcount));
  const size_t n_state = 2 * slots + size_t(n_seg) + slots * kPdBins;
  PQ_TRY(c->arena.get(n_state + size_t(n_seg), &d_state));
  u64 *d_prefix = d_state, *d_gprefix = d_prefix + slots, *d_maxkey = d_gprefix + slots,
      *d_hist = d_maxkey + n_seg, *d_maxpair = d_state + n_state;
  PQ_HIP(hipMemsetAsync(d_state, 0, n_state * sizeof(u64), c->stream));
  PQ_HIP(hipMemsetAsync(d_maxpair, 0xFF, size_t(n_seg) * sizeof(u64), c->stream));

  auto run_pass = [&](int p) -> int {
    if (p == 0)
      PQ_TRY(pd_launch_hist<kPdMaxKey>(c, dim, grid, lds, d_pts, d_seg, d_tile0, int(n_seg), total_tiles,
                                       tiles_per_block, R, p, d_gcount, d_gprefix, d_hist, d_maxkey, d_maxpair));
    else if (p == 1)
      PQ_TRY(pd_launch_hist<kPdMaxPair>(c, dim, grid, lds, d_pts, d_seg, d_tile0, int(n_seg), total_tiles,
                                        tiles_per_block, R, p, d_gcount, d_gprefix, d_hist, d_maxkey, d_maxpair));
    else
      PQ_TRY(pd_launch_hist<kPdPlain>(c, dim, grid, lds, d_pts, d_seg, d_tile0, int(n_seg), total_tiles,
                                      tiles_per_block, R, p, d_gcount, d_gprefix, d_hist, d_maxkey, d_maxpair));
    if (!any_rank) return 0;
    hipLaunchKernelGGL((k_radix_select_update<kPdBins, kPdMaxRanks>), dim3(unsigned(n_seg)), dim3(64), 0, c->stream, R, d_hist, d_prefix, d_rem,
                       d_group, d_gcount, d_gprefix);
    PQ_HIP(hipGetLastError());
    return 0;
  };
  {
    ProfScope ps(c, "pdist_max_passes");  // the two passes that also find the farthest pair
    for (int p = 0; p < std::min(passes, 2); ++p) PQ_TRY(run_pass(p));
  }
  {
    ProfScope ps(c, "pdist_passes");
    for (int p = 2; p < passes; ++p) PQ_TRY(run_pass(p));
  }
  const size_t segs = size_t(n_seg);
  std::vector<u64> keys(slots), far(segs);
  PQ_TRY(download(c, keys.data(), d_prefix, slots));
  PQ_TRY(download(c, far.data(), d_maxpair, size_t(n_seg)));
  PQ_TRY(stream_sync(c));
  for (int64_t s = 0; s < n_seg; ++s) {
    for (int r = 0; r < n_ranks; ++r)
      if (group[size_t(s) * R + r] >= 0) {
        double d2;
        std::memcpy(&d2, &keys[size_t(s) * R + r], sizeof d2);
        values[s * n_ranks + r] = std::sqrt(d2);  // correctly rounded and monotone: the rank's distance
      }
    if (max_pair && n_pairs[s] > 0) {
      max_pair[2 * s] = int64_t(far[size_t(s)] >> 32);
      max_pair[2 * s + 1] = int64_t(far[size_t(s)] & 0xFFFFFFFFull);
    }
  }
  if (stats) {
    stats[1] = total_pairs * passes;  // every pass evaluates every pair once
    stats[2] = passes;
  }
  return 0;
}

}  // extern "C"
