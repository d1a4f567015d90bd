// voxelgrid.hip — a persistent voxel set on the device and tile-sized membership queries against it:
// Open3D's VoxelGrid.create_from_point_cloud + check_if_included, the step with which pyQSM goes
// back from a voxelised tree to the full-resolution tiles (pyQSM/geometry/reconstruction.py:266-355,
// tree_isolation.py:465-516). Recollected from Open3D, parity unpinned; tests/voxelgrid_restatement.py
// defines the contract; DESIGN.md section 14.
//
// Creation is clean.hip's keying (voxel.hpp): key per point with a true fp64 division, stable radix
// sort, segments, rows ordered by the smallest member index, colour means one add at a time. What
// stays on the device is an open-addressing table (load <= 0.5) of the occupied 4x4x4-voxel blocks:
// per block a 64-bit key, the 64-bit occupancy mask of its voxels and the place of its rows, so that
// row = perm[base + popcount(mask below the voxel's bit)]; beside it the rows' indices and colours.
// A query costs its 24 bytes, a box test in registers (most of a tile lies outside one tree's box
// and ends there) and, inside the box, one 16-byte slot in the common case: a miss ends at the mask.
// The block key is 64-bit throughout, so a grid of more than 2^32 cells takes the same path. A
// binary search over the sorted voxel keys was built first and measured against this (DESIGN.md
// section 14, profiles/detail_perf.jsonl); it lost where the lookup is reached and is gone.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "voxel.hpp"

namespace pyqsm {

static constexpr uint32_t kVoxMagic = 0x56784764u;
static constexpr int64_t kVoxChunk = int64_t(1) << 22;     // queries per pass of the host form
static constexpr int64_t kVoxChunkDev = int64_t(1) << 26;  // and of the resident form (its flags: 256 MB)

struct VoxQuery {
  double ox, oy, oz, size;
  double dx, dy, dz;  // dims as fp64 (at most 2^31 - 1: exact)
  uint64_t nx, ny;
};

struct VoxBlocks {
  uint64_t nbx, nby;  // blocks along x and y
};

struct VoxGrid {
  uint32_t magic = 0;
  int32_t device = 0;
  VoxQuery q{};
  int64_t dims[3] = {0, 0, 0};
  int64_t m = 0;        // voxels
  bool colored = false;
  int64_t bytes = 0;
  int32_t* gidx = nullptr;    // [m,3] voxel indices, row order
  double* colors = nullptr;   // [m,3] colour means, row order
  // the block table: open addressing over the occupied 4x4x4-voxel blocks, load <= 0.5
  ulonglong2* slots = nullptr;  // [cap] (block key + 1, or 0: free; occupancy mask of the block's 64 voxels)
  int32_t* base = nullptr;      // [cap] first position of the block's voxels in perm
  int32_t* perm = nullptr;      // [m] rows in (block, bit) order
  uint32_t cap_mask = 0;        // cap - 1, cap a power of two
  VoxBlocks bq{};
};

static VoxGrid* as_grid(const void* p) {
  VoxGrid* g = const_cast<VoxGrid*>(static_cast<const VoxGrid*>(p));
  return g && g->magic == kVoxMagic ? g : nullptr;
}

// One voxel per thread (s: its position in key order): its row and, from the key of its first
// member, its indices.
__global__ __launch_bounds__(256) void k_vox_pack(const uint64_t* __restrict__ key, const int32_t* __restrict__ order,
                                                  const int32_t* __restrict__ offs,
                                                  const int32_t* __restrict__ row_of, int m, uint64_t nx,
                                                  uint64_t ny, int32_t* __restrict__ rows,
                                                  int32_t* __restrict__ gidx) {
  const int s = int(blockIdx.x) * 256 + int(threadIdx.x);
  if (s >= m) return;
  const uint64_t k = key[order[offs[s]]];
  const int r = row_of[s];
  rows[s] = r;
  const uint64_t yz = k / nx;
  gidx[size_t(r) * 3] = int32_t(k - yz * nx);
  gidx[size_t(r) * 3 + 1] = int32_t(yz % ny);
  gidx[size_t(r) * 3 + 2] = int32_t(yz / ny);
}

// ---- the block table ---------------------------------------------------------------------------
// Block (ix >> 2, iy >> 2, iz >> 2) of a voxel and its bit (ix & 3) | (iy & 3) << 2 | (iz & 3) << 4.
__device__ __forceinline__ uint64_t block_key(uint32_t ix, uint32_t iy, uint32_t iz, const VoxBlocks& b) {
  return uint64_t(ix >> 2) + b.nbx * (uint64_t(iy >> 2) + b.nby * uint64_t(iz >> 2));
}
__device__ __forceinline__ int block_bit(uint32_t ix, uint32_t iy, uint32_t iz) {
  return int((ix & 3u) | ((iy & 3u) << 2) | ((iz & 3u) << 4));
}
__device__ __forceinline__ uint32_t block_hash(uint64_t k) {  // murmur3's 64-bit finaliser
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return uint32_t(k);
}

// per voxel (sorted-key position s): its block key and its bit, and val[s] = s for the sorts
__global__ __launch_bounds__(256) void k_vox_blocks(const int32_t* __restrict__ rows, const int32_t* __restrict__ gidx,
                                                    int m, VoxBlocks b, uint64_t* __restrict__ bkey,
                                                    uint32_t* __restrict__ bit, int32_t* __restrict__ val) {
  const int s = int(blockIdx.x) * 256 + int(threadIdx.x);
  if (s >= m) return;
  const int32_t* g = gidx + size_t(rows[s]) * 3;
  bkey[s] = block_key(uint32_t(g[0]), uint32_t(g[1]), uint32_t(g[2]), b);
  bit[s] = uint32_t(block_bit(uint32_t(g[0]), uint32_t(g[1]), uint32_t(g[2])));
  val[s] = s;
}

// one half of the block keys in the current order of the sort
__global__ __launch_bounds__(256) void k_vox_half(const uint64_t* __restrict__ bkey, const int32_t* __restrict__ order,
                                                  int m, int shift, uint32_t* __restrict__ out) {
  const int p = int(blockIdx.x) * 256 + int(threadIdx.x);
  if (p < m) out[p] = uint32_t(bkey[order[p]] >> shift);
}

// head[p] = 1 where a block starts in (block, bit) order (head[m] = 0 for the scan); perm[p] = row
__global__ __launch_bounds__(256) void k_vox_block_heads(const uint64_t* __restrict__ bkey,
                                                         const int32_t* __restrict__ order,
                                                         const int32_t* __restrict__ rows, int m,
                                                         int32_t* __restrict__ head, int32_t* __restrict__ perm) {
  const int p = int(blockIdx.x) * 256 + int(threadIdx.x);
  if (p > m) return;
  if (p == m) {
    head[m] = 0;
    return;
  }
  head[p] = (p == 0 || bkey[order[p]] != bkey[order[p - 1]]) ? 1 : 0;
  perm[p] = rows[order[p]];
}

// One thread per position; the first of a block gathers the block's mask (at most 64 voxels follow)
// and claims a slot by compare-and-swap on the key. Which slot of its probe sequence a block ends
// up in depends on the arrival order, what a lookup returns does not. Integer atomics only.
__global__ __launch_bounds__(256) void k_vox_insert(const uint64_t* __restrict__ bkey, const uint32_t* __restrict__ bit,
                                                    const int32_t* __restrict__ order, int m,
                                                    ulonglong2* __restrict__ slots, int32_t* __restrict__ base,
                                                    uint32_t cap_mask) {
  const int p = int(blockIdx.x) * 256 + int(threadIdx.x);
  if (p >= m) return;
  const uint64_t k = bkey[order[p]];
  if (p > 0 && bkey[order[p - 1]] == k) return;
  unsigned long long mask = 0;
  for (int q = p; q < m && q < p + 64 && bkey[order[q]] == k; ++q) mask |= 1ull << bit[order[q]];
  unsigned long long* words = reinterpret_cast<unsigned long long*>(slots);
  for (uint32_t h = block_hash(k) & cap_mask;; h = (h + 1) & cap_mask)
    if (atomicCAS(&words[2 * size_t(h)], 0ull, (unsigned long long)(k + 1)) == 0ull) {
      words[2 * size_t(h) + 1] = mask;
      base[h] = p;
      return;
    }
}

// One lane per query. The box test needs no memory beyond the query itself; NaN and +-inf fail it
// (every comparison with NaN is false, floor(+-inf) is +-inf). flags[i] = 1 where the query is to
// be listed (included, or not included when invert), flags[m] = 0 for the scan.
__global__ __launch_bounds__(256) void k_vox_query(const double* __restrict__ qry, int64_t m, VoxQuery g,
                                                   VoxBlocks bq, const ulonglong2* __restrict__ slots,
                                                   const int32_t* __restrict__ base,
                                                   const int32_t* __restrict__ perm, uint32_t cap_mask, int invert,
                                                   uint8_t* __restrict__ included, int32_t* __restrict__ row,
                                                   int32_t* __restrict__ flags) {
  const int64_t i = int64_t(blockIdx.x) * 256 + int64_t(threadIdx.x);
  if (i >= m) {
    if (i == m && flags) flags[m] = 0;
    return;
  }
  const double* p = qry + size_t(i) * 3;
  // floor((q - origin) / size): the division of k_voxel_keys, so a point of the cloud finds its own voxel
  const double fx = floor((p[0] - g.ox) / g.size);
  const double fy = floor((p[1] - g.oy) / g.size);
  const double fz = floor((p[2] - g.oz) / g.size);
  int r = -1;
  const bool in_box = fx >= 0.0 && fx < g.dx && fy >= 0.0 && fy < g.dy && fz >= 0.0 && fz < g.dz;
  if (in_box) {
    const uint32_t ix = uint32_t(fx), iy = uint32_t(fy), iz = uint32_t(fz);
    const unsigned long long want = block_key(ix, iy, iz, bq) + 1;
    const int b = block_bit(ix, iy, iz);
    for (uint32_t h = block_hash(want - 1) & cap_mask;; h = (h + 1) & cap_mask) {
      const ulonglong2 e = slots[h];
      if (e.x == want) {  // most in-box misses end here, at the mask
        if ((e.y >> b) & 1ull) r = perm[base[h] + __popcll(e.y & ((1ull << b) - 1ull))];
        break;
      }
      if (e.x == 0ull) break;
    }
  }
  if (included) included[i] = r >= 0;
  if (row) row[i] = r;
  if (flags) flags[i] = (r >= 0) != (invert != 0);
}

// idx[p] += base for the p < *count entries compact_flagged wrote for a chunk that starts at base
__global__ __launch_bounds__(256) void k_vox_shift(int64_t* __restrict__ idx, const int32_t* __restrict__ count,
                                                   int64_t cap, int64_t base) {
  const int64_t p = int64_t(blockIdx.x) * 256 + int64_t(threadIdx.x);
  if (p < cap && p < int64_t(*count)) idx[p] += base;
}

static int launch_query(Ctx* c, const VoxGrid* g, const double* d_qry, int64_t m, int invert, uint8_t* d_inc,
                        int32_t* d_row, int32_t* d_flags) {
  ProfScope ps(c, "voxgrid_query");
  hipLaunchKernelGGL(k_vox_query, dim3(unsigned(ceil_div(m + 1, 256))), dim3(256), 0, c->stream, d_qry, m, g->q, g->bq,
                     static_cast<const ulonglong2*>(g->slots), static_cast<const int32_t*>(g->base),
                     static_cast<const int32_t*>(g->perm), g->cap_mask, invert, d_inc, d_row, d_flags);
  PQ_HIP(hipGetLastError());
  return 0;
}

// The block table of a packed grid (rows [m] in key order, g->gidx): voxels sorted by (block, bit)
// with the stable radix sort, block heads counted by scan, one slot claimed per block.
static int build_table(Ctx* c, VoxGrid* g, const int32_t* rows) {
  ProfScope ps(c, "voxgrid_table");
  const int M = int(g->m);
  g->bq.nbx = uint64_t(g->dims[0] + 3) >> 2;
  g->bq.nby = uint64_t(g->dims[1] + 3) >> 2;
  const unsigned __int128 blocks = (unsigned __int128)g->bq.nbx * g->bq.nby * (uint64_t(g->dims[2] + 3) >> 2);
  int bits = 0;
  while (((unsigned __int128)1 << bits) < blocks) ++bits;
  uint64_t* bkey;
  uint32_t *bit, *half;
  int32_t *val, *head;
  PQ_TRY(c->arena.get(size_t(M), &bkey));
  PQ_TRY(c->arena.get(size_t(M), &bit));
  PQ_TRY(c->arena.get(size_t(M), &half));
  PQ_TRY(c->arena.get(size_t(M), &val));
  PQ_TRY(c->arena.get(size_t(M) + 1, &head));
  const dim3 grid(ceil_div(M, 256));
  hipLaunchKernelGGL(k_vox_blocks, grid, dim3(256), 0, c->stream, rows,
                     static_cast<const int32_t*>(g->gidx), M, g->bq, bkey, bit, val);
  PQ_HIP(hipGetLastError());
  // LSD: the bit, the block key's low half, its high half; the sort may hand back other buffers,
  // so the bits are read through the order afterwards (bit[] stays in voxel order)
  {
    uint32_t* kb;
    PQ_TRY(c->arena.get(size_t(M), &kb));
    PQ_HIP(hipMemcpyAsync(kb, bit, size_t(M) * 4, hipMemcpyDeviceToDevice, c->stream));
    PQ_TRY(stable_sort_pairs_u32(c, &kb, &val, M, 6));
  }
  for (int shift = 0; shift < bits; shift += 32) {
    uint32_t* kh = half;
    hipLaunchKernelGGL(k_vox_half, grid, dim3(256), 0, c->stream, static_cast<const uint64_t*>(bkey),
                       static_cast<const int32_t*>(val), M, shift, kh);
    PQ_HIP(hipGetLastError());
    PQ_TRY(stable_sort_pairs_u32(c, &kh, &val, M, std::min(32, bits - shift)));
  }
  PQ_HIP(hipMalloc(reinterpret_cast<void**>(&g->perm), size_t(M) * 4));
  hipLaunchKernelGGL(k_vox_block_heads, dim3(ceil_div(M + 1, 256)), dim3(256), 0, c->stream,
                     static_cast<const uint64_t*>(bkey), static_cast<const int32_t*>(val),
                     rows, M, head, g->perm);
  PQ_HIP(hipGetLastError());
  PQ_TRY(exclusive_scan_i32(c, head, int64_t(M) + 1));
  int32_t nb = 0;
  PQ_TRY(fetch(c, &nb, head + M));
  uint64_t cap = 64;  // nb <= M < 2^31: at most 2^32 slots, and the mask fits 32 bits
  while (cap < 2 * uint64_t(nb)) cap <<= 1;
  g->cap_mask = uint32_t(cap - 1);
  PQ_HIP(hipMalloc(reinterpret_cast<void**>(&g->slots), size_t(cap) * 16));
  PQ_HIP(hipMalloc(reinterpret_cast<void**>(&g->base), size_t(cap) * 4));
  PQ_HIP(hipMemsetAsync(g->slots, 0, size_t(cap) * 16, c->stream));
  PQ_HIP(hipMemsetAsync(g->base, 0, size_t(cap) * 4, c->stream));
  hipLaunchKernelGGL(k_vox_insert, grid, dim3(256), 0, c->stream, static_cast<const uint64_t*>(bkey),
                     static_cast<const uint32_t*>(bit), static_cast<const int32_t*>(val), M, g->slots, g->base,
                     g->cap_mask);
  PQ_HIP(hipGetLastError());
  g->bytes += int64_t(size_t(cap) * 20 + size_t(M) * 4);
  return 0;
}

// Queries per pass: PYQSM_VOX_CHUNK overrides (tests force several ragged passes with it).
static int64_t chunk_rows(int64_t dflt) {
  if (const char* e = std::getenv("PYQSM_VOX_CHUNK")) {
    const long long v = std::atoll(e);
    if (v >= 1 && v <= dflt) return int64_t(v);
  }
  return dflt;
}

static void free_grid(VoxGrid* g) {
  g->magic = 0;
  if (hipSetDevice(g->device) == hipSuccess) {
    (void)hipFree(g->gidx);
    (void)hipFree(g->colors);
    (void)hipFree(g->slots);
    (void)hipFree(g->base);
    (void)hipFree(g->perm);
  }
  delete g;
}

// The passes both forms of the query share. host: qry and the outputs are host arrays and go
// through arena buffers of one chunk; otherwise they are device arrays and are used in place.
static int query_impl(const VoxGrid* g, const double* qry, int64_t m, int32_t flags, uint8_t* included, int32_t* row,
                      int64_t* idx, int64_t* count, bool host) {
  if (m < 0) return fail(PYQSM_EINVAL, "negative size");
  if (flags & ~PYQSM_VOX_INVERT) return fail(PYQSM_EINVAL, "unknown flags 0x%x", unsigned(flags));
  if (m > 0 && !qry) return fail(PYQSM_EINVAL, "voxel grid query: qry is NULL");
  if (count) *count = 0;
  if (m == 0 || (!included && !row && !idx && !count)) return 0;
  Call call(g->device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  const int invert = (flags & PYQSM_VOX_INVERT) ? 1 : 0;
  const bool listing = idx || count;
  const int64_t chunk = std::min(m, chunk_rows(host ? kVoxChunk : kVoxChunkDev));
  double* d_q = nullptr;
  uint8_t* d_inc = nullptr;
  int32_t *d_row = nullptr, *d_flags = nullptr;
  int64_t* d_idx = nullptr;
  if (host) {
    PQ_TRY(c->arena.get(size_t(chunk) * 3, &d_q));
    if (included) PQ_TRY(c->arena.get(size_t(chunk), &d_inc));
    if (row) PQ_TRY(c->arena.get(size_t(chunk), &d_row));
    if (idx) PQ_TRY(c->arena.get(size_t(chunk), &d_idx));
  }
  if (listing) PQ_TRY(c->arena.get(size_t(chunk) + 1, &d_flags));
  const Arena::Mark mk = c->arena.mark();
  int64_t total = 0;
  for (int64_t r0 = 0; r0 < m; r0 += chunk) {
    const int64_t mc = std::min(chunk, m - r0);
    const double* q = qry + size_t(r0) * 3;
    if (host) {
      PQ_TRY(copy_in(c, d_q, q, size_t(mc) * 3));
      q = d_q;
    }
    uint8_t* inc = host ? d_inc : (included ? included + r0 : nullptr);
    int32_t* rw = host ? d_row : (row ? row + r0 : nullptr);
    PQ_TRY(launch_query(c, g, q, mc, invert, inc, rw, d_flags));
    if (host && included) PQ_TRY(download(c, included + r0, d_inc, size_t(mc)));
    if (host && row) PQ_TRY(download(c, row + r0, d_row, size_t(mc)));
    if (!listing) continue;
    // the chunk's listed queries, ascending; the running total places them (one 4-byte read-back per pass)
    int64_t* out = idx ? (host ? d_idx : idx + total) : nullptr;
    {
      ProfScope ps(c, "voxgrid_compact");
      PQ_TRY(compact_flagged(c, d_flags, mc, out));
      if (out && r0 > 0) {
        hipLaunchKernelGGL(k_vox_shift, dim3(ceil_div(mc, 256)), dim3(256), 0, c->stream, out,
                           static_cast<const int32_t*>(d_flags + mc), mc, r0);
        PQ_HIP(hipGetLastError());
      }
    }
    int32_t cnt = 0;
    PQ_TRY(fetch(c, &cnt, d_flags + mc));
    if (host && idx && cnt > 0)
      PQ_TRY(download(c, idx + total, d_idx, size_t(cnt)));
    total += cnt;
    c->arena.rewind(mk);  // the scan's block sums
  }
  PQ_HIP(hipStreamSynchronize(c->stream));
  if (count) *count = total;
  return 0;
}

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_voxel_grid_create(const double* xyz, int64_t n, const double* colors, double voxel_size, int32_t device,
                            void** grid) {
  PQ_API_RANGE("pyqsm_voxel_grid_create");
  if (!grid) return fail(PYQSM_EINVAL, "pyqsm_voxel_grid_create: grid is NULL");
  *grid = nullptr;
  if (n < 0) return fail(PYQSM_EINVAL, "negative size");
  if (!(voxel_size > 0) || !std::isfinite(voxel_size)) return fail(PYQSM_EINVAL, "voxel_size must be positive and finite");
  if (n > 0 && !xyz) return fail(PYQSM_EINVAL, "pyqsm_voxel_grid_create: NULL pointer");
  if (n > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 points per call");
  // the box on the host: non-finite coordinates and an oversized grid are reported before any device is touched
  double mn[3] = {0.0, 0.0, 0.0}, mx[3] = {0.0, 0.0, 0.0};
  for (int64_t i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) {
      const double v = xyz[3 * i + a];
      if (!std::isfinite(v)) return fail(PYQSM_EINVAL, "point %lld has a non-finite coordinate", (long long)i);
      if (i == 0 || v < mn[a]) mn[a] = v;
      if (i == 0 || v > mx[a]) mx[a] = v;
    }
  VoxGrid* g = new VoxGrid();
  g->device = device;
  g->colored = colors != nullptr;
  double origin[3];
  unsigned __int128 cells = 1;
  for (int a = 0; a < 3; ++a) {
    origin[a] = mn[a] - voxel_size * 0.5;
    const double top = n > 0 ? std::floor((mx[a] - origin[a]) / voxel_size) : -1.0;
    if (!(top < 2147483647.0)) {
      delete g;
      return fail(PYQSM_ERANGE, "voxel_size too small for this cloud: more than 2^31 - 1 voxels along an axis");
    }
    g->dims[a] = int64_t(top) + 1;
    cells *= (unsigned __int128)g->dims[a];
  }
  if (cells > ((unsigned __int128)1 << 62)) {
    delete g;
    return fail(PYQSM_ERANGE, "voxel_size too small for this cloud: more than 2^62 cells");
  }
  g->q = VoxQuery{origin[0], origin[1], origin[2], voxel_size, double(g->dims[0]), double(g->dims[1]),
                  double(g->dims[2]), uint64_t(g->dims[0]), uint64_t(g->dims[1])};
  Ctx* c = ctx_for(device);
  if (!c) {
    delete g;
    return PYQSM_ENODEV;
  }
  g->magic = kVoxMagic;
  if (n == 0) {
    *grid = g;
    return 0;
  }
  Call call(c);
  auto build = [&]() -> int {
    double *d_xyz, *d_rgb = nullptr;
    PQ_TRY(upload(c, xyz, size_t(n) * 3, &d_xyz));
    if (colors) {
      PQ_TRY(upload(c, colors, size_t(n) * 3, &d_rgb));
    }
    VoxelDev v;
    PQ_TRY(voxel_keys_and_sort(c, d_xyz, n, voxel_size, &v));
    for (int a = 0; a < 3; ++a)
      if (v.vmin[a] != origin[a] || int64_t(v.dims[a]) != g->dims[a])
        return fail(PYQSM_EHIP, "pyqsm_voxel_grid_create: the device's bounding box differs from the host's");
    if (colors) PQ_TRY(voxel_means(c, d_xyz, d_rgb, n, &v));
    const int64_t M = v.m;
    g->m = M;
    int32_t* rows;
    PQ_TRY(c->arena.get(size_t(M), &rows));
    PQ_HIP(hipMalloc(reinterpret_cast<void**>(&g->gidx), size_t(M) * 12));
    if (colors) PQ_HIP(hipMalloc(reinterpret_cast<void**>(&g->colors), size_t(M) * 24));
    g->bytes = int64_t(size_t(M) * 12 + (colors ? size_t(M) * 24 : 0));
    hipLaunchKernelGGL(k_vox_pack, dim3(ceil_div(M, 256)), dim3(256), 0, c->stream, v.key, v.order, v.offs, v.row_of,
                       int(M), g->q.nx, g->q.ny, rows, g->gidx);
    PQ_HIP(hipGetLastError());
    PQ_TRY(build_table(c, g, rows));
    if (colors) PQ_HIP(hipMemcpyAsync(g->colors, v.rgb, size_t(M) * 24, hipMemcpyDeviceToDevice, c->stream));
    PQ_HIP(hipStreamSynchronize(c->stream));
    return 0;
  };
  const int rc = build();
  if (rc != 0) {
    free_grid(g);
    return rc;
  }
  *grid = g;
  return 0;
}

int pyqsm_voxel_grid_free(void* grid) {
  if (!grid) return 0;
  VoxGrid* g = as_grid(grid);
  if (!g) return fail(PYQSM_EINVAL, "pyqsm_voxel_grid_free: not a voxel grid");
  free_grid(g);
  return 0;
}

int pyqsm_voxel_grid_info(const void* grid, double origin[3], double* voxel_size, int64_t dims[3], int64_t* n_voxels,
                          int64_t* device_bytes) {
  const VoxGrid* g = as_grid(grid);
  if (!g) return fail(PYQSM_EINVAL, "pyqsm_voxel_grid_info: not a voxel grid");
  if (origin) {
    origin[0] = g->q.ox;
    origin[1] = g->q.oy;
    origin[2] = g->q.oz;
  }
  if (voxel_size) *voxel_size = g->q.size;
  if (dims)
    for (int a = 0; a < 3; ++a) dims[a] = g->dims[a];
  if (n_voxels) *n_voxels = g->m;
  if (device_bytes) *device_bytes = g->bytes;
  return 0;
}

int pyqsm_voxel_grid_voxels(const void* grid, int32_t* grid_index, double* colors) {
  PQ_API_RANGE("pyqsm_voxel_grid_voxels");
  const VoxGrid* g = as_grid(grid);
  if (!g) return fail(PYQSM_EINVAL, "pyqsm_voxel_grid_voxels: not a voxel grid");
  if (colors && !g->colored) return fail(PYQSM_EINVAL, "pyqsm_voxel_grid_voxels: the grid was created without colours");
  if (g->m == 0 || (!grid_index && !colors)) return 0;
  Call call(g->device, Call::kKeepArena);  // copies only: no scratch
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  if (grid_index) PQ_TRY(download(c, grid_index, g->gidx, size_t(g->m) * 3));
  if (colors) PQ_TRY(download(c, colors, g->colors, size_t(g->m) * 3));
  PQ_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int pyqsm_voxel_grid_query(const void* grid, const double* qry, int64_t m, int32_t flags, uint8_t* included,
                           int32_t* row, int64_t* idx, int64_t* count) {
  PQ_API_RANGE("pyqsm_voxel_grid_query");
  const VoxGrid* g = as_grid(grid);
  if (!g) return fail(PYQSM_EINVAL, "pyqsm_voxel_grid_query: not a voxel grid");
  return query_impl(g, qry, m, flags, included, row, idx, count, true);
}

int pyqsm_voxel_grid_query_dev(const void* grid, const double* qry_dev, int64_t m, int32_t flags, uint8_t* included_dev,
                               int32_t* row_dev, int64_t* idx_dev, int64_t* count) {
  PQ_API_RANGE("pyqsm_voxel_grid_query_dev");
  const VoxGrid* g = as_grid(grid);
  if (!g) return fail(PYQSM_EINVAL, "pyqsm_voxel_grid_query_dev: not a voxel grid");
  return query_impl(g, qry_dev, m, flags, included_dev, row_dev, idx_dev, count, false);
}

}  // extern "C"
