// recon_grid.hpp — what the ball pivoting (recon.hip) and the 3-D alpha shape (alpha3.hip) share on the
// device besides the predicate of recon_exact.hpp: the 27-cell stencil of a cell of the shared grid as nine
// ranges of sorted positions, the plan of the triangle pass (blocks per cell, the estimate of the pair
// tests) and the split / permute kernels around the atomic-free radix sort of the rows.
#pragma once
#include "grid.hpp"

namespace pyqsm {

static __global__ __launch_bounds__(256) void k_recon_to_f64(int64_t n3, const int32_t* __restrict__ ijk,
                                                             double* __restrict__ xyz) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i < n3) xyz[i] = double(ijk[i]);
}

struct ReconStencil {
  int lo[9], n[9];  // the nine (y, z) rows of the 27 cells as ranges of sorted positions
  int total;
  __device__ __forceinline__ int at(int j) const {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (j < n[k]) return lo[k] + j;
      j -= n[k];
    }
    return lo[8] + j;
  }
};

// c is a cell that holds points, hence an interior one: the border cells make every row exist
__device__ __forceinline__ ReconStencil recon_stencil(int nx, int ny, int c, const int32_t* __restrict__ start) {
  ReconStencil st;
  const int cz = c / (nx * ny), r = c - cz * nx * ny, cy = r / nx, cx = r - cy * nx;
  st.total = 0;
  int k = 0;
  for (int dz = -1; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy, ++k) {
      const int row = ((cz + dz) * ny + cy + dy) * nx + cx;
      st.lo[k] = start[row - 1];
      st.n[k] = start[row + 2] - st.lo[k];
      st.total += st.n[k];
    }
  return st;
}

// nblk[c] = blocks of the triangle pass for cell c, kSlice points each, nblk[ncell] = 0 (scanned in place
// afterwards); est[0] += low 32 bits, est[1] += high bits of (points of the cell) * (stencil count)^2,
// clamped to 2^62 per cell; est[2] = the largest stencil, est[3] = the most points in one cell.
template <int kSlice>
__global__ __launch_bounds__(256) void k_recon_plan(int ncell, int nx, int ny, int nz,
                                                    const int32_t* __restrict__ start, int32_t* __restrict__ nblk,
                                                    unsigned long long* __restrict__ est) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c > ncell) return;
  const int m = c < ncell ? start[c + 1] - start[c] : 0;
  nblk[c] = (m + kSlice - 1) / kSlice;
  if (m == 0) return;
  const ReconStencil st = recon_stencil(nx, ny, c, start);
  unsigned __int128 v = (unsigned __int128)(unsigned)st.total * (unsigned)st.total * (unsigned)m;
  const unsigned __int128 cap = (unsigned __int128)1 << 62;
  const unsigned long long w = (unsigned long long)(v < cap ? v : cap);
  atomicAdd(&est[0], w & 0xFFFFFFFFull);
  atomicAdd(&est[1], w >> 32);
  atomicMax(&est[2], (unsigned long long)st.total);
  atomicMax(&est[3], (unsigned long long)m);
}

static __global__ __launch_bounds__(256) void k_recon_split_rows(int e, const int4* __restrict__ rows,
                                                                 int32_t* __restrict__ ka, int32_t* __restrict__ kb,
                                                                 int32_t* __restrict__ kc) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= e) return;
  const int4 r = rows[i];
  ka[i] = r.x;
  kb[i] = r.y;
  kc[i] = r.z;
}

static __global__ __launch_bounds__(256) void k_recon_permute_rows(int e, const int32_t* __restrict__ perm,
                                                                   const int4* __restrict__ rows,
                                                                   int4* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < e) out[i] = rows[perm[i]];
}

}  // namespace pyqsm
