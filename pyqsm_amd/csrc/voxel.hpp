// voxel.hpp — the voxel keying and the ordered member means of clean.hip, shared with
// voxelgrid.hip: a cloud's grid and its pyqsm_voxel_down_sample have the same voxels in the same
// row order because they are the same code.
#pragma once
#include "common.hpp"

namespace pyqsm {

struct VoxelDev {
  int64_t m = 0;                    // voxels (host)
  int32_t *order, *seg, *offs, *row_of;  // key order, voxel of each sorted position, voxel bounds, rows
  double *xyz = nullptr, *rgb = nullptr;  // [m,3] means, output-row order
  uint64_t* key = nullptr;          // [n] key of every point, input order: ix + dims[0] * (iy + dims[1] * iz)
  double vmin[3];                   // min bound - size / 2 (host)
  uint64_t dims[3];                 // largest index + 1 per axis (host)
};

// Keys of the n device points at xyz, their stable sort and the voxel segments (all in the arena).
int voxel_keys_and_sort(Ctx* c, const double* xyz, int64_t n, double size, VoxelDev* v);
// v->xyz (and v->rgb when rgb is given): each voxel's members added in ascending input index.
int voxel_means(Ctx* c, const double* xyz, const double* rgb, int64_t n, VoxelDev* v);

}  // namespace pyqsm
