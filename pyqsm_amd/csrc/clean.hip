// clean.hip — the cleaning step both of pyQSM's routes start with (pyQSM/geometry/
// point_cloud_processing.py:97-127 clean_cloud): Open3D's PointCloud.voxel_down_sample and
// remove_statistical_outlier, and the whole clean_cloud loop resident in HBM.
//
// Voxel step: cloud_bbox -> one key per point (IEEE fp64 division, no reciprocal) -> stable radix
// sort of (key, index) -> head flags and two scans (voxel id in key order, output row in input
// order) -> ordered segmented mean. Every sum runs over a voxel's members in ascending input index,
// from 0.0, one add at a time (Open3D's AccumulatedPoint): bit-exact and independent of the
// schedule. Statistical step: kNN with the point itself counted -> mean distance per point ->
// fixed-order two-level reductions (sparse.hpp) -> mask -> compaction by scan. No float atomics.
#include <algorithm>
#include <cmath>

#include "common.hpp"
#include "grid.hpp"
#include "knn.hpp"
#include "sparse.hpp"
#include "voxel.hpp"

namespace pyqsm {

static constexpr int kLaneMax = 64;         // voxels with at most this many members: one lane each
static constexpr int kWaveTile = 256;       // members a wave stages per step for a larger voxel
static constexpr int kTilePad = kWaveTile + 1;  // column stride in LDS: the six columns on distinct banks

struct VoxGeom {
  double vx, vy, vz, size;
  uint64_t nx, ny;
};

// ---- keys ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_voxel_keys(const double* __restrict__ xyz, int n, VoxGeom g,
                                                    uint64_t* __restrict__ key, uint32_t* __restrict__ lo,
                                                    int32_t* __restrict__ val) {
  const int i = int(blockIdx.x) * 256 + int(threadIdx.x);
  if (i >= n) return;
  const double* p = xyz + size_t(i) * 3;
  // floor((p - vmin) / size): a true division, as Open3D computes it (a reciprocal moves keys on faces)
  const uint64_t ix = uint64_t(floor((p[0] - g.vx) / g.size));
  const uint64_t iy = uint64_t(floor((p[1] - g.vy) / g.size));
  const uint64_t iz = uint64_t(floor((p[2] - g.vz) / g.size));
  const uint64_t k = ix + g.nx * (iy + g.ny * iz);
  key[i] = k;
  lo[i] = uint32_t(k);
  val[i] = i;
}

// high halves of the keys in the order of the first (low-half) sort
__global__ __launch_bounds__(256) void k_voxel_hi(const uint64_t* __restrict__ key, const int32_t* __restrict__ order,
                                                  int n, uint32_t* __restrict__ hi) {
  const int j = int(blockIdx.x) * 256 + int(threadIdx.x);
  if (j < n) hi[j] = uint32_t(key[order[j]] >> 32);
}

// ---- segments --------------------------------------------------------------------------------
// head[j] (key order) and first[i] (input order) = 1 where a voxel starts; the sort is stable, so the
// first member of a voxel in key order is its smallest input index. Entry n of both stays 0 so that
// the exclusive scans leave the voxel count there.
__global__ __launch_bounds__(256) void k_voxel_heads(const uint64_t* __restrict__ key, const int32_t* __restrict__ order,
                                                     int n, int32_t* __restrict__ head, int32_t* __restrict__ first) {
  const int j = int(blockIdx.x) * 256 + int(threadIdx.x);
  if (j >= n) {
    if (j == n) head[n] = first[n] = 0;
    return;
  }
  const int i = order[j];
  const int h = (j == 0 || key[i] != key[order[j - 1]]) ? 1 : 0;
  head[j] = h;
  first[i] = h;
}

// seg = scanned head, row = scanned first: offs[s] = first sorted position of voxel s, row_of[s] =
// its output row (rank of its smallest index among the voxels' smallest indices)
__global__ __launch_bounds__(256) void k_voxel_segs(const int32_t* __restrict__ order, const int32_t* __restrict__ seg,
                                                    const int32_t* __restrict__ row, int n, int32_t* __restrict__ offs,
                                                    int32_t* __restrict__ row_of) {
  const int j = int(blockIdx.x) * 256 + int(threadIdx.x);
  if (j >= n) return;
  const int s = seg[j];
  if (seg[j + 1] != s) {
    offs[s] = j;
    row_of[s] = row[order[j]];
  }
  if (j == n - 1) offs[seg[n]] = n;
}

// ---- ordered segmented mean ------------------------------------------------------------------
// Small voxels, one lane each; a larger one is listed for k_voxel_mean_wave (the list's order is
// the arrival order of an integer atomic, but every voxel is computed alone: the results are not).
__global__ __launch_bounds__(256) void k_voxel_mean_lane(const double* __restrict__ xyz, const double* __restrict__ rgb,
                                                         const int32_t* __restrict__ order,
                                                         const int32_t* __restrict__ offs,
                                                         const int32_t* __restrict__ row_of, int m,
                                                         double* __restrict__ out_xyz, double* __restrict__ out_rgb,
                                                         int32_t* __restrict__ big, int32_t* __restrict__ n_big) {
  const int s = int(blockIdx.x) * 256 + int(threadIdx.x);
  if (s >= m) return;
  const int b = offs[s], e = offs[s + 1];
  if (e - b > kLaneMax) {
    big[atomicAdd(n_big, 1)] = s;
    return;
  }
  const size_t r = size_t(row_of[s]) * 3;
  const double cnt = double(e - b);
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int q = b; q < e; ++q) {
    const double* p = xyz + size_t(order[q]) * 3;
    sx = sx + p[0];
    sy = sy + p[1];
    sz = sz + p[2];
  }
  out_xyz[r] = sx / cnt;
  out_xyz[r + 1] = sy / cnt;
  out_xyz[r + 2] = sz / cnt;
  if (rgb) {
    sx = sy = sz = 0.0;
    for (int q = b; q < e; ++q) {
      const double* p = rgb + size_t(order[q]) * 3;
      sx = sx + p[0];
      sy = sy + p[1];
      sz = sz + p[2];
    }
    out_rgb[r] = sx / cnt;
    out_rgb[r + 1] = sy / cnt;
    out_rgb[r + 2] = sz / cnt;
  }
}

// Larger voxels, one wave each (grid-stride over the list). The wave gathers kWaveTile members at a
// time (four per lane, the next tile's loads in flight while the current one is summed) into LDS,
// and lane c < 3 (6 with colours) adds column c in member order: one dependent add per member and
// column, as many gathers in flight as the wave can issue. A voxel that holds the whole cloud costs
// n / 256 steps instead of n dependent gathers on one lane.
__global__ __launch_bounds__(256) void k_voxel_mean_wave(const double* __restrict__ xyz, const double* __restrict__ rgb,
                                                         const int32_t* __restrict__ order,
                                                         const int32_t* __restrict__ offs,
                                                         const int32_t* __restrict__ row_of,
                                                         const int32_t* __restrict__ big,
                                                         const int32_t* __restrict__ n_big,
                                                         double* __restrict__ out_xyz, double* __restrict__ out_rgb) {
  __shared__ double tile[4][6 * kTilePad];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double* t = tile[w];
  const int ncol = rgb ? 6 : 3;
  const int nb = __builtin_amdgcn_readfirstlane(*n_big);
  const int waves = int(gridDim.x) * 4;
  for (int v = int(blockIdx.x) * 4 + w; v < nb; v += waves) {
    const int s = __builtin_amdgcn_readfirstlane(big[v]);
    const int b = __builtin_amdgcn_readfirstlane(offs[s]);
    const int e = __builtin_amdgcn_readfirstlane(offs[s + 1]);
    double reg[4][6] = {};
    auto load = [&](int base) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int q = base + u * 64 + lane;
        if (q < e) {
          const size_t i = size_t(order[q]) * 3;
          reg[u][0] = xyz[i];
          reg[u][1] = xyz[i + 1];
          reg[u][2] = xyz[i + 2];
          if (rgb) {
            reg[u][3] = rgb[i];
            reg[u][4] = rgb[i + 1];
            reg[u][5] = rgb[i + 2];
          }
        }
      }
    };
    load(b);
    double acc = 0.0;
    for (int base = b; base < e; base += kWaveTile) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        t[0 * kTilePad + u * 64 + lane] = reg[u][0];
        t[1 * kTilePad + u * 64 + lane] = reg[u][1];
        t[2 * kTilePad + u * 64 + lane] = reg[u][2];
        if (rgb) {
          t[3 * kTilePad + u * 64 + lane] = reg[u][3];
          t[4 * kTilePad + u * 64 + lane] = reg[u][4];
          t[5 * kTilePad + u * 64 + lane] = reg[u][5];
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (base + kWaveTile < e) load(base + kWaveTile);
      const int cnt = min(kWaveTile, e - base);
      if (lane < ncol) {
        const double* col = t + lane * kTilePad;
        for (int q = 0; q < cnt; ++q) acc = acc + col[q];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    const size_t r = size_t(row_of[s]) * 3;
    const double mean = acc / double(e - b);
    if (lane < 3)
      out_xyz[r + lane] = mean;
    else if (lane < ncol)
      out_rgb[r + lane - 3] = mean;
  }
}

// ---- trace -----------------------------------------------------------------------------------
// inverse[i] = output row of point i; cnt_row[row] = members of the voxel on that row
__global__ __launch_bounds__(256) void k_voxel_inverse(const int32_t* __restrict__ order, const int32_t* __restrict__ seg,
                                                       const int32_t* __restrict__ offs,
                                                       const int32_t* __restrict__ row_of, int n,
                                                       int64_t* __restrict__ inverse, int32_t* __restrict__ cnt_row) {
  const int j = int(blockIdx.x) * 256 + int(threadIdx.x);
  if (j >= n) {
    if (j == n) cnt_row[seg[n]] = 0;
    return;
  }
  const int s = seg[j + 1] - 1;  // seg is the exclusive scan of the heads: the voxel of j is one less than after it
  const int r = row_of[s];
  if (inverse) inverse[order[j]] = r;
  if (offs[s] == j) cnt_row[r] = offs[s + 1] - j;
}

// members in output-row order (ascending within a row: the key order is stable); offsets [m+1]
__global__ __launch_bounds__(256) void k_voxel_members(const int32_t* __restrict__ order, const int32_t* __restrict__ seg,
                                                       const int32_t* __restrict__ offs,
                                                       const int32_t* __restrict__ row_of,
                                                       const int32_t* __restrict__ row_start, int n,
                                                       int64_t* __restrict__ offsets, int64_t* __restrict__ members) {
  const int j = int(blockIdx.x) * 256 + int(threadIdx.x);
  if (j > n) return;
  if (j == n) {
    offsets[seg[n]] = n;
    return;
  }
  const int s = seg[j + 1] - 1;  // seg is the exclusive scan of the heads: the voxel of j is one less than after it
  const int r = row_of[s];
  const int pos = row_start[r] + (j - offs[s]);
  members[pos] = order[j];
  if (offs[s] == j) offsets[r] = row_start[r];
}

// ---- statistical outlier removal -------------------------------------------------------------
// avg[i] = (sum of sqrt(d2) over the k nearest, ascending, from 0.0) / k; partial sums of the
// positive averages into part (sparse.hpp: fixed order, no atomics)
__global__ __launch_bounds__(256) void k_stat_avg(const double* __restrict__ d2, int n, int k,
                                                  double* __restrict__ avg, double* __restrict__ part) {
  double pos = 0.0;
  for (int i = int(blockIdx.x) * 256 + int(threadIdx.x); i < n; i += int(gridDim.x) * 256) {
    const double* row = d2 + size_t(i) * k;
    double s = 0.0;
    for (int j = 0; j < k; ++j) s = s + sqrt(row[j]);
    const double a = s / double(k);
    avg[i] = a;
    if (a > 0) pos = pos + a;
  }
  reduce3_part(pos, 0.0, 0.0, part);
}

// stats[0] = mean = (sum of the positive averages) / n (Open3D divides by every point)
__global__ __launch_bounds__(256) void k_stat_mean(const double* __restrict__ part, int n, double* __restrict__ stats) {
  double tot[3];
  part_total3(part, tot);
  if (threadIdx.x == 0) stats[0] = tot[0] / double(n);
}

__global__ __launch_bounds__(256) void k_stat_sq(const double* __restrict__ avg, int n, const double* __restrict__ stats,
                                                 double* __restrict__ part) {
  const double mean = stats[0];
  double sq = 0.0;
  for (int i = int(blockIdx.x) * 256 + int(threadIdx.x); i < n; i += int(gridDim.x) * 256) {
    const double a = avg[i];
    if (a > 0) {
      const double t = a - mean;
      sq = sq + t * t;
    }
  }
  reduce3_part(sq, 0.0, 0.0, part);
}

// stats[1] = std = sqrt(sq / (n - 1)), stats[2] = thr = mean + ratio * std
__global__ __launch_bounds__(256) void k_stat_thr(const double* __restrict__ part, int n, double ratio,
                                                  double* __restrict__ stats) {
  double tot[3];
  part_total3(part, tot);
  if (threadIdx.x == 0) {
    const double sd = sqrt(tot[0] / double(n - 1));
    stats[1] = sd;
    stats[2] = stats[0] + ratio * sd;
  }
}

// keep[i] = avg > 0 && avg < thr; entry n = 0 (the scan leaves the kept count there)
__global__ __launch_bounds__(256) void k_stat_mask(const double* __restrict__ avg, int n, const double* __restrict__ stats,
                                                   int32_t* __restrict__ keep) {
  const int i = int(blockIdx.x) * 256 + int(threadIdx.x);
  if (i > n) return;
  if (i == n) {
    keep[n] = 0;
    return;
  }
  const double a = avg[i], thr = stats[2];
  keep[i] = (a > 0 && a < thr) ? 1 : 0;
}

// ---- device-resident steps -------------------------------------------------------------------
int voxel_keys_and_sort(Ctx* c, const double* xyz, int64_t n, double size, VoxelDev* v) {
  const int N = int(n);
  double mn[3], mx[3];
  {
    ProfScope ps(c, "clean_bbox");
    PQ_TRY(cloud_bbox(c, xyz, n, mn, mx));
  }
  VoxGeom g;
  double vmin[3];
  uint64_t dims[3];
  for (int a = 0; a < 3; ++a) {
    vmin[a] = mn[a] - size * 0.5;
    const double top = std::floor((mx[a] - vmin[a]) / size);
    if (!(top < 0x1p62)) return fail(PYQSM_ERANGE, "voxel_size too small for this cloud");
    dims[a] = uint64_t(top) + 1;
  }
  const unsigned __int128 lim = (unsigned __int128)1 << 62, xy = (unsigned __int128)dims[0] * dims[1];
  if (xy > lim || xy * dims[2] > lim) return fail(PYQSM_ERANGE, "voxel_size too small for this cloud");
  const unsigned __int128 cells = xy * dims[2];
  g.vx = vmin[0];
  g.vy = vmin[1];
  g.vz = vmin[2];
  g.size = size;
  g.nx = dims[0];
  g.ny = dims[1];
  for (int a = 0; a < 3; ++a) {
    v->vmin[a] = vmin[a];
    v->dims[a] = dims[a];
  }
  int bits = 0;
  while ((unsigned __int128)1 << bits < cells) ++bits;
  uint64_t* key;
  uint32_t* lo;
  int32_t* val;
  PQ_TRY(c->arena.get(size_t(n), &key));
  PQ_TRY(c->arena.get(size_t(n), &lo));
  PQ_TRY(c->arena.get(size_t(n), &val));
  {
    ProfScope ps(c, "clean_keys");
    hipLaunchKernelGGL(k_voxel_keys, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, xyz, N, g, key, lo, val);
    PQ_HIP(hipGetLastError());
  }
  {
    // LSD: the low 32 bits, then the high ones; both passes are stable, so members stay in index order
    ProfScope ps(c, "clean_sort");
    PQ_TRY(stable_sort_pairs_u32(c, &lo, &val, n, std::min(bits, 32)));
    if (bits > 32) {
      uint32_t* hi;
      PQ_TRY(c->arena.get(size_t(n), &hi));
      hipLaunchKernelGGL(k_voxel_hi, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, key, val, N, hi);
      PQ_HIP(hipGetLastError());
      PQ_TRY(stable_sort_pairs_u32(c, &hi, &val, n, bits - 32));
    }
  }
  v->order = val;
  v->key = key;
  int32_t *head, *first;
  PQ_TRY(c->arena.get(size_t(n) + 1, &head));
  PQ_TRY(c->arena.get(size_t(n) + 1, &first));
  {
    ProfScope ps(c, "clean_segments");
    hipLaunchKernelGGL(k_voxel_heads, dim3(ceil_div(n + 1, 256)), dim3(256), 0, c->stream, key, val, N, head, first);
    PQ_HIP(hipGetLastError());
    PQ_TRY(exclusive_scan_i32(c, head, n + 1));
    PQ_TRY(exclusive_scan_i32(c, first, n + 1));
    int32_t m = 0;
    PQ_TRY(fetch(c, &m, head + n));
    v->m = m;
    PQ_TRY(c->arena.get(size_t(m) + 1, &v->offs));
    PQ_TRY(c->arena.get(size_t(m), &v->row_of));
    hipLaunchKernelGGL(k_voxel_segs, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, val, head, first, N, v->offs,
                       v->row_of);
    PQ_HIP(hipGetLastError());
  }
  v->seg = head;
  return 0;
}

int voxel_means(Ctx* c, const double* xyz, const double* rgb, int64_t n, VoxelDev* v) {
  ProfScope ps(c, "clean_means");
  const int M = int(v->m);
  PQ_TRY(c->arena.get(size_t(M) * 3, &v->xyz));
  if (rgb) PQ_TRY(c->arena.get(size_t(M) * 3, &v->rgb));
  int32_t *big, *n_big;
  PQ_TRY(c->arena.get(size_t(n / (kLaneMax + 1)) + 1, &big));
  PQ_TRY(c->arena.get(1, &n_big));
  PQ_HIP(hipMemsetAsync(n_big, 0, 4, c->stream));
  hipLaunchKernelGGL(k_voxel_mean_lane, dim3(ceil_div(M, 256)), dim3(256), 0, c->stream, xyz, rgb, v->order, v->offs,
                     v->row_of, M, v->xyz, v->rgb, big, n_big);
  PQ_HIP(hipGetLastError());
  // at most n / 65 voxels are listed; waves past the list's length return at once
  const int waves = int(std::min<int64_t>(n / (kLaneMax + 1) + 1, int64_t(c->cu_count) * 16));
  hipLaunchKernelGGL(k_voxel_mean_wave, dim3(ceil_div(waves, 4)), dim3(256), 0, c->stream, xyz, rgb, v->order, v->offs,
                     v->row_of, big, n_big, v->xyz, v->rgb);
  PQ_HIP(hipGetLastError());
  return 0;
}

// Statistical outlier removal of the n points at xyz (device). Writes avg [n] (arena when null),
// stats [3] = (mean, std, thr), the kept indices ascending (keep, may be null), the kept points
// (out_xyz, may be null) and the scanned keep mask pos [n+1] (pos[n] = kept count).
static int stat_device(Ctx* c, const double* xyz, int64_t n, int32_t nb, double ratio, double* avg, double* stats,
                       int64_t* keep, double* out_xyz, int32_t** pos_out) {
  const int N = int(n);
  const int k = int(std::min<int64_t>(nb, n));
  if (k > kKnnMaxK) return fail(PYQSM_ERANGE, "nb_neighbors must be at most %d", kKnnMaxK);
  int32_t* idx;
  double* d2;
  PQ_TRY(c->arena.get(size_t(n) * k, &idx));
  PQ_TRY(c->arena.get(size_t(n) * k, &d2));
  if (!avg) PQ_TRY(c->arena.get(size_t(n), &avg));
  {
    ProfScope ps(c, "clean_knn");
    PQ_TRY(knn_device(c, xyz, n, k, 0, idx, d2));
  }
  double *part_a, *part_b;
  PQ_TRY(c->arena.get(size_t(3) * kPart, &part_a));
  PQ_TRY(c->arena.get(size_t(3) * kPart, &part_b));
  int32_t* pos;
  PQ_TRY(c->arena.get(size_t(n) + 1, &pos));
  {
    ProfScope ps(c, "clean_reduce");
    const unsigned grid = reduce_grid(n);
    hipLaunchKernelGGL(k_stat_avg, dim3(grid), dim3(256), 0, c->stream, d2, N, k, avg, part_a);
    hipLaunchKernelGGL(k_stat_mean, dim3(1), dim3(256), 0, c->stream, part_a, N, stats);
    hipLaunchKernelGGL(k_stat_sq, dim3(grid), dim3(256), 0, c->stream, avg, N, stats, part_b);
    hipLaunchKernelGGL(k_stat_thr, dim3(1), dim3(256), 0, c->stream, part_b, N, ratio, stats);
    PQ_HIP(hipGetLastError());
  }
  {
    ProfScope ps(c, "clean_compact");
    hipLaunchKernelGGL(k_stat_mask, dim3(ceil_div(n + 1, 256)), dim3(256), 0, c->stream, avg, N, stats, pos);
    PQ_HIP(hipGetLastError());
    PQ_TRY(compact_flagged(c, pos, n, keep, nullptr, xyz, out_xyz));
  }
  *pos_out = pos;
  return 0;
}

static int check_n(int64_t n) {
  if (n < 0) return fail(PYQSM_EINVAL, "negative size");
  if (n > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 points per call");
  return 0;
}

static bool bad_voxel(double size) { return !(size > 0) || !std::isfinite(size); }

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_voxel_down_sample(const double* xyz, int64_t n, const double* colors, double voxel_size, int64_t* m_out,
                            double** out_xyz, double** out_colors, int64_t* inverse, int64_t* offsets,
                            int64_t* members, int32_t device) {
  PQ_API_RANGE("pyqsm_voxel_down_sample");
  PQ_TRY(check_n(n));
  if (!m_out || !out_xyz || (colors && !out_colors)) return fail(PYQSM_EINVAL, "pyqsm_voxel_down_sample: NULL out-parameter");
  if (bool(offsets) != bool(members)) return fail(PYQSM_EINVAL, "offsets and members go together");
  *m_out = 0;
  *out_xyz = nullptr;
  if (out_colors) *out_colors = nullptr;
  if (bad_voxel(voxel_size)) return fail(PYQSM_EINVAL, "voxel_size must be positive and finite");
  if (n > 0 && !xyz) return fail(PYQSM_EINVAL, "pyqsm_voxel_down_sample: NULL pointer");
  Ctx* c = ctx_for(device);
  if (!c) return PYQSM_ENODEV;
  if (n == 0) {
    if (offsets) offsets[0] = 0;
    return 0;
  }
  Call call(c);
  double *d_xyz, *d_rgb = nullptr;
  PQ_TRY(upload(c, xyz, size_t(n) * 3, &d_xyz));
  if (colors) {
    PQ_TRY(upload(c, colors, size_t(n) * 3, &d_rgb));
  }
  VoxelDev v;
  PQ_TRY(voxel_keys_and_sort(c, d_xyz, n, voxel_size, &v));
  PQ_TRY(voxel_means(c, d_xyz, d_rgb, n, &v));
  const int M = int(v.m);
  int64_t *d_inv = nullptr, *d_offsets = nullptr, *d_members = nullptr;
  if (inverse || offsets) {
    int32_t *cnt_row;
    PQ_TRY(c->arena.get(size_t(M) + 1, &cnt_row));
    if (inverse) PQ_TRY(c->arena.get(size_t(n), &d_inv));
    hipLaunchKernelGGL(k_voxel_inverse, dim3(ceil_div(n + 1, 256)), dim3(256), 0, c->stream, v.order, v.seg, v.offs,
                       v.row_of, int(n), d_inv, cnt_row);
    PQ_HIP(hipGetLastError());
    if (offsets) {
      PQ_TRY(exclusive_scan_i32(c, cnt_row, int64_t(M) + 1));
      PQ_TRY(c->arena.get(size_t(M) + 1, &d_offsets));
      PQ_TRY(c->arena.get(size_t(n), &d_members));
      hipLaunchKernelGGL(k_voxel_members, dim3(ceil_div(n + 1, 256)), dim3(256), 0, c->stream, v.order, v.seg, v.offs,
                         v.row_of, cnt_row, int(n), d_offsets, d_members);
      PQ_HIP(hipGetLastError());
    }
  }
  OutBufs out;
  double* h_xyz = out.get<double>(size_t(M) * 3);
  double* h_rgb = colors ? out.get<double>(size_t(M) * 3) : nullptr;
  if (!h_xyz || (colors && !h_rgb)) return fail(PYQSM_ENOMEM, "host allocation failed");
  PQ_TRY(download(c, h_xyz, v.xyz, size_t(M) * 3));
  if (colors) PQ_TRY(download(c, h_rgb, v.rgb, size_t(M) * 3));
  if (inverse) PQ_TRY(download(c, inverse, d_inv, size_t(n)));
  if (offsets) {
    PQ_TRY(download(c, offsets, d_offsets, size_t(M) + 1));
    PQ_TRY(download(c, members, d_members, size_t(n)));
  }
  PQ_HIP(hipStreamSynchronize(c->stream));
  out.kept = true;
  *m_out = M;
  *out_xyz = h_xyz;
  if (colors) *out_colors = h_rgb;
  return 0;
}

int pyqsm_stat_outlier(const double* xyz, int64_t n, int32_t nb_neighbors, double std_ratio, int64_t* keep,
                       int64_t* n_keep, double* avg, double* stats, int32_t device) {
  PQ_API_RANGE("pyqsm_stat_outlier");
  PQ_TRY(check_n(n));
  if (!n_keep) return fail(PYQSM_EINVAL, "pyqsm_stat_outlier: NULL out-parameter");
  *n_keep = 0;
  if (nb_neighbors < 1) return fail(PYQSM_EINVAL, "nb_neighbors must be at least 1");
  if (!(std_ratio > 0)) return fail(PYQSM_EINVAL, "std_ratio must be positive");
  if (n > 0 && (!xyz || !keep)) return fail(PYQSM_EINVAL, "pyqsm_stat_outlier: NULL pointer");
  Ctx* c = ctx_for(device);
  if (!c) return PYQSM_ENODEV;
  if (n == 0) return 0;
  Call call(c);
  double *d_xyz, *d_avg = nullptr, *d_stats;
  int64_t* d_keep;
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_xyz));
  PQ_TRY(c->arena.get(size_t(n), &d_keep));
  PQ_TRY(c->arena.get(4, &d_stats));
  if (avg) PQ_TRY(c->arena.get(size_t(n), &d_avg));
  PQ_TRY(copy_in(c, d_xyz, xyz, size_t(n) * 3));
  int32_t* pos;
  PQ_TRY(stat_device(c, d_xyz, n, nb_neighbors, std_ratio, d_avg, d_stats, d_keep, nullptr, &pos));
  int32_t cnt = 0;
  PQ_TRY(download(c, &cnt, pos + n, 1));
  if (avg) PQ_TRY(download(c, avg, d_avg, size_t(n)));
  if (stats) PQ_TRY(download(c, stats, d_stats, 3));
  PQ_HIP(hipStreamSynchronize(c->stream));
  PQ_TRY(fetch(c, keep, d_keep, size_t(cnt)));
  *n_keep = cnt;
  return 0;
}

int pyqsm_clean_cloud(const double* xyz, int64_t n, double voxel_size, double neighbors, double ratio, int32_t iters,
                      int64_t* m_out, double** out_xyz, int32_t device) {
  PQ_API_RANGE("pyqsm_clean_cloud");
  PQ_TRY(check_n(n));
  if (!m_out || !out_xyz) return fail(PYQSM_EINVAL, "pyqsm_clean_cloud: NULL out-parameter");
  *m_out = 0;
  *out_xyz = nullptr;
  if (voxel_size != 0 && bad_voxel(voxel_size)) return fail(PYQSM_EINVAL, "voxel_size must be 0 (off) or positive and finite");
  if (iters < 0) return fail(PYQSM_EINVAL, "iters must be >= 0");
  if (iters > 0 && (!(neighbors >= 1) || !(ratio > 0))) return fail(PYQSM_EINVAL, "neighbors must be >= 1 and ratio > 0");
  if (iters > 0 && std::ldexp(neighbors, iters - 1) >= 2147483648.0)
    return fail(PYQSM_ERANGE, "neighbors doubled %d times exceeds int32", iters - 1);
  if (n > 0 && !xyz) return fail(PYQSM_EINVAL, "pyqsm_clean_cloud: NULL pointer");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  const double* cur = nullptr;
  int64_t m = n;
  if (n > 0) {
    double* d_xyz;
    PQ_TRY(upload(c, xyz, size_t(n) * 3, &d_xyz));
    cur = d_xyz;
    if (voxel_size > 0) {
      VoxelDev v;
      PQ_TRY(voxel_keys_and_sort(c, cur, n, voxel_size, &v));
      PQ_TRY(voxel_means(c, cur, nullptr, n, &v));
      cur = v.xyz;
      m = v.m;
    }
    // each round as pyQSM's loop runs it: int(neighbors), then neighbors *= 2 and ratio /= 1.5
    double nb = neighbors, r = ratio;
    for (int it = 0; it < iters && m > 0; ++it) {
      double* next;
      PQ_TRY(c->arena.get(size_t(m) * 3, &next));
      double* stats;
      PQ_TRY(c->arena.get(4, &stats));
      const Arena::Mark mk = c->arena.mark();
      int32_t* pos;
      PQ_TRY(stat_device(c, cur, m, int32_t(nb), r, nullptr, stats, nullptr, next, &pos));
      int32_t cnt = 0;
      PQ_TRY(fetch(c, &cnt, pos + m));
      c->arena.rewind(mk);
      cur = next;
      m = cnt;
      nb = nb * 2;
      r = r / 1.5;
    }
  }
  OutBufs out;
  double* h = out.get<double>(size_t(m) * 3);
  if (!h) return fail(PYQSM_ENOMEM, "host allocation failed");
  if (m > 0) PQ_TRY(fetch(c, h, cur, size_t(m) * 3));
  out.kept = true;
  *m_out = m;
  *out_xyz = h;
  return 0;
}

}  // extern "C"
