// boxes.hip — pyqsm_points_in_boxes: which points lie in which oriented boxes, as a CSR by box
// (OrientedBoundingBox.get_point_indices_within_bounding_box for up to 256 boxes per pass over the cloud;
// pyQSM's recover_original_details asks it of every cluster box against every tile of the scan).
//
// Point p is in box k iff |t_i| <= half_i for i = 0, 1, 2 with d = p - c and
// t_i = (d.x * R[0][i] + d.y * R[1][i]) + d.z * R[2][i]: fp64, in this order, no contraction.
//
// Two passes over the points, 24 B per point each: a wave owns 512 consecutive points (8 per lane, in
// registers) and counts, per box, its members by ballots; a scan over [box][wave] places every wave's
// members; the second pass repeats the tests and writes each member at its rank, so the indices ascend
// inside a box. No atomics.
#include "common.hpp"

namespace pyqsm {

static constexpr int kBoxMax = PYQSM_BOXES_MAX;
static constexpr int kBoxRounds = 8;                  // points per lane
static constexpr int kBoxWavePts = 64 * kBoxRounds;   // 512

__device__ __forceinline__ bool in_box(double px, double py, double pz, const double* __restrict__ b) {
  const double dx = px - b[0], dy = py - b[1], dz = pz - b[2];
  const double t0 = (dx * b[3] + dy * b[6]) + dz * b[9];
  const double t1 = (dx * b[4] + dy * b[7]) + dz * b[10];
  const double t2 = (dx * b[5] + dy * b[8]) + dz * b[11];
  return fabs(t0) <= b[12] && fabs(t1) <= b[13] && fabs(t2) <= b[14];
}

// FILL == false: counts[k * nw + wave] = members of box k among the wave's points.
// FILL == true: counts holds the scanned offsets; idx receives the members.
template <bool FILL>
__global__ __launch_bounds__(256) void k_boxes(const double* __restrict__ xyz, int64_t n,
                                               const double* __restrict__ boxes, int B, int64_t nw,
                                               int32_t* __restrict__ counts, int64_t* __restrict__ idx) {
  __shared__ double sb[kBoxMax * 15];
  for (int t = threadIdx.x; t < B * 15; t += 256) sb[t] = boxes[t];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t wave = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  const int64_t base = wave * kBoxWavePts;
  if (base >= n) return;
  double px[kBoxRounds], py[kBoxRounds], pz[kBoxRounds];
#pragma unroll
  for (int r = 0; r < kBoxRounds; ++r) {
    const int64_t i = base + r * 64 + lane;
    const bool ok = i < n;
    px[r] = ok ? xyz[3 * i] : __builtin_nan("");  // a NaN is in no box
    py[r] = ok ? xyz[3 * i + 1] : 0.0;
    pz[r] = ok ? xyz[3 * i + 2] : 0.0;
  }
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int k = 0; k < B; ++k) {
    const double* b = sb + 15 * k;
    int64_t off = FILL ? int64_t(counts[size_t(k) * nw + wave]) : 0;
#pragma unroll
    for (int r = 0; r < kBoxRounds; ++r) {
      const bool in = in_box(px[r], py[r], pz[r], b);
      const unsigned long long m = __ballot(in);
      if (FILL && in) idx[off + __popcll(m & below)] = base + r * 64 + lane;
      off += __popcll(m);
    }
    if (!FILL && lane == 0) counts[size_t(k) * nw + wave] = int32_t(off);
  }
}

__global__ __launch_bounds__(256) void k_boxes_ptr(int B, int64_t nw, const int32_t* __restrict__ counts,
                                                   int64_t* __restrict__ ptr) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k <= B) ptr[k] = counts[size_t(k) * nw];
}

static int boxes_run(Ctx* c, const double* d_xyz, int64_t n, const double* boxes, int32_t B, int64_t* ptr,
                     int64_t** idx) {
  const int64_t nw = (n + kBoxWavePts - 1) / kBoxWavePts;
  const unsigned blocks = unsigned((nw + 3) / 4);
  double* d_boxes;
  int32_t* d_counts;
  int64_t* d_ptr;
  PQ_TRY(upload(c, boxes, size_t(B) * 15, &d_boxes));
  PQ_TRY(c->arena.get(size_t(B) * nw + 1, &d_counts));
  PQ_TRY(c->arena.get(size_t(B) + 1, &d_ptr));
  PQ_HIP(hipMemsetAsync(d_counts + size_t(B) * nw, 0, 4, c->stream));
  {
    ProfScope ps(c, "boxes_count");
    hipLaunchKernelGGL(k_boxes<false>, dim3(blocks), dim3(256), 0, c->stream, d_xyz, n,
                       static_cast<const double*>(d_boxes), int(B), nw, d_counts, static_cast<int64_t*>(nullptr));
    PQ_HIP(hipGetLastError());
  }
  PQ_TRY(exclusive_scan_i32(c, d_counts, int64_t(B) * nw + 1));  // the last entry becomes the total
  hipLaunchKernelGGL(k_boxes_ptr, dim3(ceil_div(B + 1, 256)), dim3(256), 0, c->stream, int(B), nw,
                     static_cast<const int32_t*>(d_counts), d_ptr);
  PQ_HIP(hipGetLastError());
  PQ_TRY(fetch(c, ptr, d_ptr, size_t(B) + 1));
  const int64_t total = ptr[B];
  if (total == 0) return 0;
  int64_t* d_idx;
  PQ_TRY(c->arena.get(size_t(total), &d_idx));
  {
    ProfScope ps(c, "boxes_fill");
    hipLaunchKernelGGL(k_boxes<true>, dim3(blocks), dim3(256), 0, c->stream, d_xyz, n,
                       static_cast<const double*>(d_boxes), int(B), nw, d_counts, d_idx);
    PQ_HIP(hipGetLastError());
  }
  OutBufs out;
  int64_t* h = out.get<int64_t>(size_t(total));
  if (!h) return fail(PYQSM_ENOMEM, "pyqsm_points_in_boxes: no host memory for %lld indices", (long long)total);
  PQ_TRY(fetch(c, h, d_idx, size_t(total)));
  out.kept = true;
  *idx = h;
  return 0;
}

static int boxes_check(const void* xyz, int64_t n, const double* boxes, int32_t B, int64_t* ptr, int64_t** idx) {
  if (idx) *idx = nullptr;
  if (n < 0 || B < 0) return fail(PYQSM_EINVAL, "negative size");
  if (B > kBoxMax) return fail(PYQSM_EINVAL, "pyqsm_points_in_boxes: at most %d boxes per call", kBoxMax);
  if (!ptr || !idx || (n > 0 && !xyz) || (B > 0 && !boxes))
    return fail(PYQSM_EINVAL, "pyqsm_points_in_boxes: NULL pointer");
  for (int32_t k = 0; k <= B; ++k) ptr[k] = 0;
  // the member counts are scanned in 32 bits: n * B bounds their sum
  if (B > 0 && n > 0x7FFFFF00LL / B)
    return fail(PYQSM_ERANGE, "pyqsm_points_in_boxes: n * B above 2^31: pass fewer boxes per call");
  return 0;
}

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_points_in_boxes(const double* xyz, int64_t n, const double* boxes, int32_t B, int64_t* ptr,
                          int64_t** idx, int32_t device) {
  PQ_API_RANGE("pyqsm_points_in_boxes");
  PQ_TRY(boxes_check(xyz, n, boxes, B, ptr, idx));
  if (n == 0 || B == 0) return 0;
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double* d_xyz;
  PQ_TRY(upload(c, xyz, size_t(n) * 3, &d_xyz));
  return boxes_run(c, d_xyz, n, boxes, B, ptr, idx);
}

int pyqsm_points_in_boxes_dev(const double* xyz_dev, int64_t n, const double* boxes, int32_t B, int64_t* ptr,
                              int64_t** idx, int32_t device) {
  PQ_API_RANGE("pyqsm_points_in_boxes_dev");
  PQ_TRY(boxes_check(xyz_dev, n, boxes, B, ptr, idx));
  if (n == 0 || B == 0) return 0;
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  return boxes_run(c, xyz_dev, n, boxes, B, ptr, idx);
}

}  // extern "C"
