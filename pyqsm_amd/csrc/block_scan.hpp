// block_scan.hpp — prefix sums of one value per thread across a wave and across a block: shuffles
// inside the wave, the waves' totals through LDS that the caller owns (a kernel with an LDS struct of
// its own keeps the totals there and does not grow a second array).
#pragma once
#include "common.hpp"

namespace pyqsm {

__device__ __forceinline__ int32_t wave_incl_scan(int32_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    int32_t t = __shfl_up(v, off, 64);
    if (lane >= off) v += t;
  }
  return v;
}
// two values side by side
__device__ __forceinline__ void wave_incl_scan(int32_t& a, int32_t& b) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int32_t u = __shfl_up(a, off, 64), ub = __shfl_up(b, off, 64);
    if (lane >= off) {
      a += u;
      b += ub;
    }
  }
}

// Exclusive prefix of v across a block of THREADS threads; wsum: THREADS / 64 ints of LDS. One
// barrier; the caller puts another before wsum is written again.
template <int THREADS>
__device__ __forceinline__ int32_t block_excl_scan(int32_t v, int32_t* wsum) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int32_t incl = wave_incl_scan(v);
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  int32_t run = incl - v;
  for (int q = 0; q < w; ++q) run += wsum[q];
  return run;
}
// the same for two values behind the one barrier
template <int THREADS>
__device__ __forceinline__ void block_excl_scan(int32_t a, int32_t b, int32_t* wsum_a, int32_t* wsum_b, int32_t* run_a,
                                                int32_t* run_b) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int32_t ia = a, ib = b;
  wave_incl_scan(ia, ib);
  if (lane == 63) {
    wsum_a[w] = ia;
    wsum_b[w] = ib;
  }
  __syncthreads();
  int32_t ra = ia - a, rb = ib - b;
  for (int q = 0; q < w; ++q) {
    ra += wsum_a[q];
    rb += wsum_b[q];
  }
  *run_a = ra;
  *run_b = rb;
}
// The exclusive prefix and the block's total, wsum free again on return (a second barrier): for
// kernels that scan several values in a row.
template <int THREADS>
__device__ __forceinline__ int32_t block_excl_scan(int32_t v, int32_t* wsum, int32_t* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int32_t incl = wave_incl_scan(v);
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  int32_t base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < THREADS / 64; ++i) {
    if (i < w) base += wsum[i];
    tot += wsum[i];
  }
  *total = tot;
  __syncthreads();
  return base + incl - v;
}

}  // namespace pyqsm
