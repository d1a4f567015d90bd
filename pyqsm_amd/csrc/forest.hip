// forest.hip — inference of a fitted scikit-learn tree ensemble: the RandomForestClassifier pyQSM
// labels every point of a cloud as wood, leaf or epiphyte with (pyQSM/exploration.py:460-538
// random_forest_classification). Training stays on the host; this file walks the trees.
// tests/forest_restatement.py states the contract in NumPy; it is scikit-learn's
// own arithmetic (_tree.pyx _apply_dense, ForestClassifier.predict_proba) and is matched bit for bit.
//
// Layout. pyqsm_forest_create validates every tree on the host and re-lays its reachable nodes
// out breadth-first with the two children of a node adjacent. Every slot is 8 bytes:
//   internal  x = float32 threshold   y = [31] 0  [30] missing_go_to_left  [29:22] feature
//                                         [21:0] slot of the left child within the tree
//   leaf      x = row of the leaf in the value table   y = [31] 1
// The float32 threshold is the largest float32 not above the float64 one: for a float32 x,
// (double)x <= t and x <= t32 are the same predicate, so the narrowing is exact. Leaf distributions
// live in a separate f64 table, one row per leaf padded with zeros to the kernel's 2, 3, 8 or 32
// accumulators (the loads of a row need no branch), the leaves' original node numbers (for apply)
// in an i32 [leaves] table. Breadth-first order makes the first S slots of a tree its top levels.
//
// Kernel. k_forest_walk: RPL rows per lane (two up to 16 features and 8 classes, else one), 256
// lanes per workgroup. The block's rows sit in LDS, transposed ([feature][row]: every lane reads
// its own bank whatever feature its node asks for). A lane's two walks advance together, so their
// record loads are in flight at the same time. The trees are visited in estimator order, each lane adding the leaf's class fractions to its C
// float64 accumulators, so the sum has scikit-learn's order of additions by construction: no
// atomics, no partial sums. The first S = 256 * NPT slots of the current tree are read from LDS;
// the next tree's are loaded into registers before the walk and written to the other LDS buffer
// after it (one barrier per tree). A lane whose walk has reached its leaf leaves the loop: the wave
// issues loads only for the lanes still walking. At the end proba = acc / T (one IEEE division) and
// label = the first maximum of proba.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>

#include "common.hpp"

namespace pyqsm {

static constexpr int kForestRows = 256;                 // lanes per workgroup; each owns RPL rows
static constexpr int kForestMaxF = PYQSM_FOREST_MAX_FEATURES;
static constexpr int kForestMaxC = PYQSM_FOREST_MAX_CLASSES;
static constexpr uint32_t kForestMaxSlots = PYQSM_FOREST_MAX_TREE_NODES;  // 22-bit child slot
static constexpr int kForestTwoRowsMaxF = 16;           // two rows per lane up to this many features
static constexpr uint32_t kLeafBit = 0x80000000u;
static constexpr uint64_t kForestMagic = 0x70797173666f7265ull;

struct ForestDev {
  const uint2* nodes;          // [slots]
  const double* values;        // [leaves, CP], CP = class_pad(C): the columns beyond C are zero
  const int32_t* leaf_node;    // [leaves] node number within the tree, as the caller numbered it
  const uint32_t* tree_off;    // [T + 1] first slot of every tree
  int T, C, F;
};

struct Forest {
  uint64_t magic;
  int device;
  ForestDev d;
  int64_t slots, leaves, max_depth, bytes;
  int staged;
};

template <int CT, int NPT, int RPL>
__global__ __launch_bounds__(kForestRows) void k_forest_walk(ForestDev fd, const float* __restrict__ X, int64_t n,
                                                             double* __restrict__ proba,
                                                             int32_t* __restrict__ label,
                                                             int32_t* __restrict__ leaves) {
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int S = NPT * kForestRows;
  constexpr int BR = RPL * kForestRows;  // rows of the block; lane tid owns rows tid + r * 256
  float* xs = reinterpret_cast<float*>(smem);                            // [F][BR]
  uint2* st = reinterpret_cast<uint2*>(smem + size_t(fd.F) * BR * 4);    // [2][S]
  const int tid = threadIdx.x;
  const int64_t row0 = int64_t(blockIdx.x) * BR;
  const int nrow = int(n - row0 < BR ? n - row0 : BR);
  const int F = fd.F, C = fd.C, T = fd.T;
  const float* xb = X + row0 * F;
  for (int e = tid; e < nrow * F; e += kForestRows) {
    const int r = e / F, f = e - r * F;
    xs[f * BR + r] = xb[e];
  }
  if (NPT > 0) {
    const uint32_t cnt = fd.tree_off[1] - fd.tree_off[0];
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
      const uint32_t s = uint32_t(j * kForestRows + tid);
      if (s < cnt) st[s] = fd.nodes[fd.tree_off[0] + s];
    }
  }
  __syncthreads();
  double acc[RPL][CT];
  bool live[RPL];
#pragma unroll
  for (int r = 0; r < RPL; ++r) {
    live[r] = r * kForestRows + tid < nrow;
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[r][c] = 0.0;
  }
  const bool sum = proba != nullptr || label != nullptr;
  for (int t = 0; t < T; ++t) {
    const uint32_t base = fd.tree_off[t];
    uint2 pre[NPT > 0 ? NPT : 1];
    if (NPT > 0) {  // the next tree's top, in flight while this one is walked (the last tree: itself, unused)
      const int tn = t + 1 < T ? t + 1 : t;
      const uint32_t nb = fd.tree_off[tn], ncnt = fd.tree_off[tn + 1] - nb;
#pragma unroll
      for (int j = 0; j < NPT; ++j) {
        const uint32_t s = uint32_t(j * kForestRows + tid);
        pre[j] = s < ncnt ? fd.nodes[nb + s] : make_uint2(0u, 0u);
      }
    }
    const uint2* cur = st + (t & 1) * S;
    // the lane's RPL walks advance together: their record loads are in flight at the same time
    uint2 nd[RPL];
    bool any = false;
#pragma unroll
    for (int r = 0; r < RPL; ++r) {
      nd[r] = !live[r] ? make_uint2(0u, kLeafBit) : NPT > 0 ? cur[0] : fd.nodes[base];
      any = any || !(nd[r].y & kLeafBit);
    }
    while (any) {
      any = false;
#pragma unroll
      for (int r = 0; r < RPL; ++r)
        if (!(nd[r].y & kLeafBit)) {
          const float x = xs[((nd[r].y >> 22) & 0xFFu) * BR + r * kForestRows + tid];
          const bool left = x != x ? ((nd[r].y >> 30) & 1u) != 0u : x <= __uint_as_float(nd[r].x);
          const uint32_t s = (nd[r].y & 0x3FFFFFu) + (left ? 0u : 1u);
          if (NPT > 0 && s < uint32_t(S)) nd[r] = cur[s];
          else nd[r] = fd.nodes[base + s];
          any = true;  // a record just loaded is looked at in the next round
        }
    }
#pragma unroll
    for (int r = 0; r < RPL; ++r)
      if (live[r]) {
        const size_t lr = nd[r].x;
        if (leaves) leaves[size_t(row0 + r * kForestRows + tid) * T + t] = fd.leaf_node[lr];
        if (sum) {  // rows padded to CT columns (zeros): CT independent loads, no branch between them
          const double* v = fd.values + lr * CT;
          double w[CT];
#pragma unroll
          for (int c = 0; c < CT; ++c) w[c] = v[c];
#pragma unroll
          for (int c = 0; c < CT; ++c) acc[r][c] = acc[r][c] + w[c];
        }
      }
    if (NPT > 0) {
      uint2* nxt = st + ((t + 1) & 1) * S;
#pragma unroll
      for (int j = 0; j < NPT; ++j) nxt[j * kForestRows + tid] = pre[j];
      __syncthreads();  // the other buffer was last read in the walk of tree t - 1
    }
  }
  if (!sum) return;
  const double dT = double(T);
#pragma unroll
  for (int r = 0; r < RPL; ++r)
    if (live[r]) {
      const size_t row = size_t(row0 + r * kForestRows + tid);
      double best = 0.0;
      int bi = 0;
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (c < C) {
          const double p = acc[r][c] / dT;
          if (proba) proba[row * C + c] = p;
          if (c == 0 || p > best) {  // the first maximum
            best = p;
            bi = c;
          }
        }
      if (label) label[row] = bi;
    }
}

// The largest float32 not above t (t not NaN).
static float floor_f32(double t) {
  float f = float(t);
  if (double(f) > t) f = std::nextafterf(f, -std::numeric_limits<float>::infinity());
  return f;
}

// The columns of a row of the value table: the accumulators the kernel is instantiated with.
static int class_pad(int C) { return C <= 2 ? 2 : C <= 3 ? 3 : C <= 8 ? 8 : 32; }

static Forest* as_forest(const void* p) {
  Forest* f = const_cast<Forest*>(static_cast<const Forest*>(p));
  return f && f->magic == kForestMagic ? f : nullptr;
}

template <int CT, int NPT, int RPL>
static int launch_walk(Ctx* c, const Forest* f, const float* d_X, int64_t n, double* d_proba, int32_t* d_label,
                       int32_t* d_leaves) {
  const size_t lds = size_t(f->d.F) * RPL * kForestRows * 4 + size_t(2) * NPT * kForestRows * 8;
  if (lds > 65536)
    PQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_forest_walk<CT, NPT, RPL>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
  hipLaunchKernelGGL((k_forest_walk<CT, NPT, RPL>), dim3(ceil_div(n, RPL * kForestRows)), dim3(kForestRows), lds,
                     c->stream, f->d, d_X, n, d_proba, d_label, d_leaves);
  return 0;
}

template <int CT, int RPL>
static int launch_staged(Ctx* c, const Forest* f, const float* d_X, int64_t n, double* d_proba, int32_t* d_label,
                         int32_t* d_leaves) {
  switch (f->staged / kForestRows) {
    case 0: return launch_walk<CT, 0, RPL>(c, f, d_X, n, d_proba, d_label, d_leaves);
    case 2: return launch_walk<CT, 2, RPL>(c, f, d_X, n, d_proba, d_label, d_leaves);
    case 4: return launch_walk<CT, 4, RPL>(c, f, d_X, n, d_proba, d_label, d_leaves);
    default: return launch_walk<CT, 8, RPL>(c, f, d_X, n, d_proba, d_label, d_leaves);
  }
}

// Rows per lane: two walks in flight per lane where the block's rows still fit LDS comfortably
// and the accumulators the registers (PYQSM_FOREST_RPL=1|2 overrides, for measurements).
static int rows_per_lane(const Forest* f) {
  int rpl = f->d.F <= kForestTwoRowsMaxF && f->d.C <= 8 ? 2 : 1;
  if (const char* e = std::getenv("PYQSM_FOREST_RPL"))
    if ((e[0] == '1' || e[0] == '2') && e[1] == 0 && f->d.C <= 8 && f->d.F <= 32) rpl = e[0] - '0';
  return rpl;
}

template <int CT>
static int launch_rows(Ctx* c, const Forest* f, const float* d_X, int64_t n, double* d_proba, int32_t* d_label,
                       int32_t* d_leaves) {
  if (CT <= 8 && rows_per_lane(f) == 2) return launch_staged<CT, (CT <= 8 ? 2 : 1)>(c, f, d_X, n, d_proba, d_label, d_leaves);
  return launch_staged<CT, 1>(c, f, d_X, n, d_proba, d_label, d_leaves);
}

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_forest_create(const int64_t* tree_offsets, const int32_t* left, const int32_t* right,
                        const int32_t* feature, const double* threshold, const uint8_t* missing_left,
                        const double* value, int32_t T, int32_t C, int32_t F, int32_t device, void** forest) {
  PQ_API_RANGE("pyqsm_forest_create");
  if (!forest) return fail(PYQSM_EINVAL, "pyqsm_forest_create: forest is NULL");
  *forest = nullptr;
  if (!tree_offsets || !left || !right || !feature || !threshold || !missing_left || !value)
    return fail(PYQSM_EINVAL, "pyqsm_forest_create: NULL pointer");
  if (T < 1) return fail(PYQSM_EINVAL, "a forest needs at least one tree, got %d", int(T));
  if (C < 1 || F < 1) return fail(PYQSM_EINVAL, "classes and features must be positive, got C = %d, F = %d", int(C), int(F));
  if (C > kForestMaxC) return fail(PYQSM_ERANGE, "%d classes: the kernel keeps at most %d accumulators per row", int(C), kForestMaxC);
  if (F > kForestMaxF) return fail(PYQSM_ERANGE, "%d features: a block's rows fit LDS up to %d", int(F), kForestMaxF);
  if (tree_offsets[0] != 0) return fail(PYQSM_EINVAL, "tree_offsets must start at 0");
  for (int t = 0; t < T; ++t) {
    const int64_t m = tree_offsets[t + 1] - tree_offsets[t];
    if (m < 1) return fail(PYQSM_EINVAL, "tree %d has no nodes (tree_offsets must ascend)", t);
    if (m > int64_t(kForestMaxSlots))
      return fail(PYQSM_ERANGE, "tree %d has %lld nodes, the node record addresses %u per tree", t, (long long)m,
                  kForestMaxSlots);
  }
  if (tree_offsets[T] > 0x7FFFFFFFLL) return fail(PYQSM_ERANGE, "more than 2^31 - 1 nodes in the forest");
  // breadth-first re-layout of the reachable nodes, validated on the way: every child in range
  // and met once (a tree, so every path ends in a leaf), features in range, thresholds not NaN
  const int CP = class_pad(C);
  std::vector<uint2> nodes;
  std::vector<double> values;
  std::vector<int32_t> leaf_node;
  std::vector<uint32_t> off(size_t(T) + 1, 0u);
  nodes.reserve(size_t(tree_offsets[T]));
  std::vector<int32_t> queue, depth;
  std::vector<uint8_t> seen;
  int64_t max_depth = 0;
  for (int t = 0; t < T; ++t) {
    const int64_t o = tree_offsets[t];
    const int32_t m = int32_t(tree_offsets[t + 1] - o);
    off[t] = uint32_t(nodes.size());
    seen.assign(size_t(m), 0);
    queue.assign(1, 0);
    depth.assign(1, 0);
    seen[0] = 1;
    uint32_t next = 1;  // the next free slot of this tree
    for (size_t q = 0; q < queue.size(); ++q) {
      const int32_t i = queue[q];
      const int32_t l = left[o + i], r = right[o + i];
      max_depth = std::max<int64_t>(max_depth, depth[q]);
      if (l == -1) {
        if (r != -1) return fail(PYQSM_EINVAL, "tree %d node %d has one child", t, int(i));
        const double* v = value + size_t(o + i) * C;
        for (int c = 0; c < C; ++c)
          if (!std::isfinite(v[c])) return fail(PYQSM_EINVAL, "tree %d leaf %d: value is not finite", t, int(i));
        nodes.push_back(make_uint2(uint32_t(leaf_node.size()), kLeafBit));
        leaf_node.push_back(i);
        values.insert(values.end(), v, v + C);
        values.insert(values.end(), size_t(CP - C), 0.0);
        continue;
      }
      if (l < 0 || l >= m || r < 0 || r >= m)
        return fail(PYQSM_EINVAL, "tree %d node %d: child out of range (%d, %d; %d nodes)", t, int(i), int(l), int(r), int(m));
      if (seen[l] || seen[r] || l == r)
        return fail(PYQSM_EINVAL, "tree %d node %d: a child is reached twice (not a tree)", t, int(i));
      seen[l] = seen[r] = 1;
      const int32_t ft = feature[o + i];
      if (ft < 0 || ft >= F) return fail(PYQSM_EINVAL, "tree %d node %d: feature %d is not in [0, %d)", t, int(i), int(ft), int(F));
      const double th = threshold[o + i];
      if (th != th) return fail(PYQSM_EINVAL, "tree %d node %d: NaN threshold", t, int(i));
      const float t32 = floor_f32(th);
      uint32_t bits;
      std::memcpy(&bits, &t32, 4);
      nodes.push_back(make_uint2(bits, (missing_left[o + i] ? 0x40000000u : 0u) | (uint32_t(ft) << 22) | next));
      next += 2;
      queue.push_back(l);
      queue.push_back(r);
      depth.push_back(depth[q] + 1);
      depth.push_back(depth[q] + 1);
    }
  }
  off[T] = uint32_t(nodes.size());
  Ctx* c = ctx_for(device);
  if (!c) return PYQSM_ENODEV;
  Forest* f = new Forest();
  f->magic = kForestMagic;
  f->device = device;
  f->slots = int64_t(nodes.size());
  f->leaves = int64_t(leaf_node.size());
  f->max_depth = max_depth;
  f->d.T = T;
  f->d.C = C;
  f->d.F = F;
  const size_t bn = nodes.size() * 8, bv = values.size() * 8, bl = leaf_node.size() * 4, bo = off.size() * 4;
  f->bytes = int64_t(bn + bv + bl + bo);
  void *dn = nullptr, *dv = nullptr, *dl = nullptr, *dof = nullptr;
  hipError_t e = hipMalloc(&dn, bn);
  if (e == hipSuccess) e = hipMalloc(&dv, bv);
  if (e == hipSuccess) e = hipMalloc(&dl, bl);
  if (e == hipSuccess) e = hipMalloc(&dof, bo);
  if (e == hipSuccess) e = hipMemcpy(dn, nodes.data(), bn, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dv, values.data(), bv, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dl, leaf_node.data(), bl, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dof, off.data(), bo, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(dn);
    (void)hipFree(dv);
    (void)hipFree(dl);
    (void)hipFree(dof);
    delete f;
    return fail(e == hipErrorOutOfMemory ? PYQSM_ENOMEM : PYQSM_EHIP, "pyqsm_forest_create: %s", hipGetErrorString(e));
  }
  f->d.nodes = static_cast<const uint2*>(dn);
  f->d.values = static_cast<const double*>(dv);
  f->d.leaf_node = static_cast<const int32_t*>(dl);
  f->d.tree_off = static_cast<const uint32_t*>(dof);
  f->staged = rows_per_lane(f) == 2 ? 1024 : 512;  // the fastest measured for either shape
  *forest = f;
  return 0;
}

int pyqsm_forest_free(void* forest) {
  if (!forest) return 0;
  Forest* f = as_forest(forest);
  if (!f) return fail(PYQSM_EINVAL, "pyqsm_forest_free: not a forest");
  f->magic = 0;
  if (hipSetDevice(f->device) == hipSuccess) {
    (void)hipFree(const_cast<uint2*>(f->d.nodes));
    (void)hipFree(const_cast<double*>(f->d.values));
    (void)hipFree(const_cast<int32_t*>(f->d.leaf_node));
    (void)hipFree(const_cast<uint32_t*>(f->d.tree_off));
  }
  delete f;
  return 0;
}

int pyqsm_forest_info(const void* forest, int64_t info[8]) {
  const Forest* f = as_forest(forest);
  if (!f || !info) return fail(PYQSM_EINVAL, "pyqsm_forest_info: not a forest, or info is NULL");
  info[0] = f->d.T;
  info[1] = f->d.C;
  info[2] = f->d.F;
  info[3] = f->slots;
  info[4] = f->leaves;
  info[5] = f->max_depth;
  info[6] = f->bytes;
  info[7] = f->staged;
  return 0;
}

int pyqsm_forest_stage(void* forest, int32_t staged_nodes) {
  Forest* f = as_forest(forest);
  if (!f) return fail(PYQSM_EINVAL, "pyqsm_forest_stage: not a forest");
  if (staged_nodes != 0 && staged_nodes != 512 && staged_nodes != 1024 && staged_nodes != 2048)
    return fail(PYQSM_ERANGE, "staged_nodes must be 0, 512, 1024 or 2048, got %d", int(staged_nodes));
  f->staged = staged_nodes;
  return 0;
}

int pyqsm_forest_predict(const void* forest, const float* X, int64_t n, double* proba, int32_t* label,
                         int32_t* leaves) {
  PQ_API_RANGE("pyqsm_forest_predict");
  const Forest* f = as_forest(forest);
  if (!f) return fail(PYQSM_EINVAL, "pyqsm_forest_predict: not a forest");
  if (n < 0) return fail(PYQSM_EINVAL, "negative size");
  if (n > 0 && !X) return fail(PYQSM_EINVAL, "pyqsm_forest_predict: X is NULL");
  if (n == 0 || (!proba && !label && !leaves)) return 0;
  Call call(f->device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  const int T = f->d.T, C = f->d.C, F = f->d.F;
  // rows per chunk: about 256 MB of arena for the rows and everything asked for, whole blocks
  const size_t per_row = size_t(F) * 4 + (proba ? size_t(C) * 8 : 0) + (label ? 4 : 0) + (leaves ? size_t(T) * 4 : 0);
  int64_t chunk = int64_t((size_t(256) << 20) / per_row) / kForestRows * kForestRows;
  chunk = std::max<int64_t>(kForestRows, std::min<int64_t>(chunk, int64_t(1) << 23));
  chunk = std::min(chunk, n);
  float* d_X;
  double* d_proba = nullptr;
  int32_t *d_label = nullptr, *d_leaves = nullptr;
  PQ_TRY(c->arena.get(size_t(chunk) * F, &d_X));
  if (proba) PQ_TRY(c->arena.get(size_t(chunk) * C, &d_proba));
  if (label) PQ_TRY(c->arena.get(size_t(chunk), &d_label));
  if (leaves) PQ_TRY(c->arena.get(size_t(chunk) * T, &d_leaves));
  for (int64_t r0 = 0; r0 < n; r0 += chunk) {
    const int64_t m = std::min(chunk, n - r0);
    PQ_TRY(copy_in(c, d_X, X + size_t(r0) * F, size_t(m) * F));
    {
      ProfScope ps(c, "forest_walk");
      int rc;
      if (C <= 2) rc = launch_rows<2>(c, f, d_X, m, d_proba, d_label, d_leaves);
      else if (C <= 3) rc = launch_rows<3>(c, f, d_X, m, d_proba, d_label, d_leaves);
      else if (C <= 8) rc = launch_rows<8>(c, f, d_X, m, d_proba, d_label, d_leaves);
      else rc = launch_rows<32>(c, f, d_X, m, d_proba, d_label, d_leaves);
      PQ_TRY(rc);
      PQ_HIP(hipGetLastError());
    }
    if (proba) PQ_TRY(download(c, proba + size_t(r0) * C, d_proba, size_t(m) * C));
    if (label) PQ_TRY(download(c, label + size_t(r0), d_label, size_t(m)));
    if (leaves) PQ_TRY(download(c, leaves + size_t(r0) * T, d_leaves, size_t(m) * T));
  }
  PQ_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

}  // extern "C"
