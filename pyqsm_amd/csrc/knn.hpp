// knn.hpp — the exact k nearest neighbours (knn.hip) as the other kernels' host code calls it.
#pragma once
#include "common.hpp"

namespace pyqsm {

static constexpr int kKnnMaxK = 192;  // largest k of a search: the LDS lists of knn.hip and of its callers

// The k nearest of every one of the n points d_xyz (device) among them, ascending by (d2, index), into
// idx / d2 [n, k] (device); exclude_self != 0 leaves the point itself out. k in [1, kKnnMaxK].
int knn_device(Ctx* c, const double* xyz, int64_t n, int32_t k, int32_t exclude_self, int32_t* idx, double* d2);

}  // namespace pyqsm
