// reduce.hpp — the fixed-order pieces several translation units share: the chunk sum (kmeans.hip,
// epiphyte.hip) and the bookkeeping kernel of the radix selections (pdist.hip, epiphyte.hip).
#pragma once
#include "common.hpp"

namespace pyqsm {

// "Chunk sum": 256 consecutive values per chunk, lane l of a wave holding values 4l..4l+3 summed
// as ((v0 + v1) + v2) + v3, then an xor butterfly over the 64 lanes (pairs of neighbours first);
// the chunk totals are added one at a time from 0.0 in chunk order.
static constexpr int kChunk = 256;  // values per chunk-sum chunk (one wave)

__device__ __forceinline__ double chunk_wave_sum(double v0, double v1, double v2, double v3) {
  double s = ((v0 + v1) + v2) + v3;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) s = s + __shfl_xor(s, off, 64);
  return s;  // the same bits in every lane: a + b == b + a
}

// Between two passes of a radix selection (eight bits per pass, most significant first), one wave per
// segment, lane r for rank slot r: the bin of the group's histogram that holds the rank becomes the
// next digit of the slot's prefix, the keys in the bins before it leave the rank. Then the slots are
// regrouped by their new prefix (the first slot of a prefix leads its group, groups numbered in slot
// order) and the segment's histograms are cleared for the next pass. A template only so that the
// translation units that do not select carry no copy.
template <int BINS, int MAX_RANKS>
__global__ __launch_bounds__(64) void k_radix_select_update(int n_ranks, unsigned long long* __restrict__ hist,
                                                            unsigned long long* __restrict__ prefix,
                                                            unsigned long long* __restrict__ remaining,
                                                            int32_t* __restrict__ group, int32_t* __restrict__ gcount,
                                                            unsigned long long* __restrict__ gprefix) {
  using u64 = unsigned long long;
  __shared__ u64 s_pre[MAX_RANKS];
  __shared__ int s_lead[MAX_RANKS];
  const int s = blockIdx.x, r = threadIdx.x;
  const size_t slot = size_t(s) * n_ranks + r;
  const int old_groups = gcount[s];
  u64* h = hist + size_t(s) * n_ranks * BINS;
  const int g = r < n_ranks ? group[slot] : -1;
  u64 pre = 0;
  if (g >= 0) {
    const u64* hg = h + size_t(g) * BINS;
    u64 k = remaining[slot], before = 0;
    int bin = BINS - 1;
    for (int d = 0; d < BINS; ++d) {
      const u64 c = hg[d];
      if (k < before + c) {
        bin = d;
        break;
      }
      before += c;
    }
    remaining[slot] = k - before;
    pre = (prefix[slot] << 8) | u64(bin);
    prefix[slot] = pre;
  }
  if (r < MAX_RANKS) s_pre[r] = pre;
  __syncthreads();
  for (int k = r; k < old_groups * BINS; k += 64) h[k] = 0;
  int leader = -1;
  if (g >= 0) {
    for (int q = 0; q <= r; ++q)
      if (group[size_t(s) * n_ranks + q] >= 0 && s_pre[q] == pre) {
        leader = q;
        break;
      }
  }
  if (r < MAX_RANKS) s_lead[r] = leader == r;
  __syncthreads();  // every slot's group has been read
  if (g >= 0) {
    int id = 0;
    for (int q = 0; q < leader; ++q) id += s_lead[q];
    group[slot] = id;
    if (leader == r) gprefix[size_t(s) * n_ranks + id] = pre;
  }
  if (r == 0) {
    int n = 0;
    for (int q = 0; q < n_ranks; ++q) n += s_lead[q];
    gcount[s] = n;
  }
}

}  // namespace pyqsm
