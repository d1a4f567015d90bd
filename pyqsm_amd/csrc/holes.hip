// holes.hip — the boundary loops of a triangle mesh and their minimum-area patches:
// what pyQSM's geometry/surf_recon.py meshfix asks of pymeshfix's fill_small_boundaries, by a contract of
// its own with a fixed output order.
//
// The sorted half-edge table is mesh.hip's (mesh_halfedge.hpp); twins come from its runs. One thread per
// boundary half-edge rotates about its head vertex to its successor. The cycles of the successor are the
// loops: two pointer-doubling sweeps find every cycle's smallest member, then every member's rank from
// it, in O(log B) rounds each. The boundary half-edges are ordered by (tail vertex, h) beforehand, so the
// smallest member is the loop's start, the starts in ascending order number the loops, and a vertex
// that repeats inside a loop sits in adjacent positions. Loops are classed on the device and patched by
// one wave each (short) or one block each with the table in LDS (long); the arithmetic is holes_exact.hpp.
// Atomics: one 32-bit integer atomicAdd per triangle corner counts the fan sizes that cap the rotation;
// everything else is plain stores, scans and the atomic-free radix sort.
#include <algorithm>

#include "common.hpp"
#include "holes_exact.hpp"
#include "mesh_halfedge.hpp"

namespace pyqsm {

namespace {

constexpr int64_t kFillMaxTris = int64_t(1) << 29;  // 3T half-edges stay below 2^31
constexpr int kMaxLoop = PYQSM_FILL_MAX_LOOP;       // the longest loop that is patched
constexpr int kWaveMax = PYQSM_FILL_WAVE_MAX;       // the longest loop of the wave class
constexpr int kWaveTab = kWaveMax * (kWaveMax - 1) / 2;
constexpr int kLongTab = kMaxLoop * (kMaxLoop - 1) / 2;
// the long class's LDS: weights, points, splits
constexpr size_t kLongLds = size_t(kLongTab) * 8 + size_t(kMaxLoop) * 24 + size_t(kLongTab);
static_assert(kMaxLoop <= 128, "one thread per entry of a diagonal in a 128-thread block; splits are u8");
static_assert(kWaveMax <= 64 && kWaveMax >= 3 && kWaveMax < kMaxLoop, "a wave sweeps a short loop's diagonal");
static_assert(2 * kLongLds <= 160 * 1024, "two blocks of the long class per CU");

__device__ __forceinline__ int he_next(int h) {
  const int t = h / 3, k = h - 3 * t;
  return 3 * t + (k == 2 ? 0 : k + 1);
}

// One thread per sorted half-edge: twin[h] = the half-edge that runs the other way on an edge of exactly
// two triangles, -1 on a boundary edge (one triangle), -2 where a walk stops (more than two triangles,
// or two that run the same way). bflag [nh + 1]: 1 on boundary half-edges, bflag[nh] = 0.
__global__ __launch_bounds__(256) void k_fill_twins(int nh, const int32_t* __restrict__ tris,
                                                    const int32_t* __restrict__ hs, const int32_t* __restrict__ x,
                                                    const int32_t* __restrict__ first, int32_t* __restrict__ twin,
                                                    int32_t* __restrict__ bflag, int32_t* __restrict__ deg) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) bflag[nh] = 0;
  if (i >= nh) return;
  const int e = x[i + 1] - 1, f = first[e], cnt = first[e + 1] - f, h = hs[i];
  int tw = -2;
  if (cnt == 1) tw = -1;
  if (cnt == 2) {
    const int o = hs[i == f ? f + 1 : f];
    if (tris[o] != tris[h]) tw = o;  // different tails: opposite directions
  }
  twin[h] = tw;
  bflag[h] = cnt == 1;
  atomicAdd(&deg[tris[h]], 1);  // corners at the vertex: the size of its fan
}

// bscan: the exclusive scan of bflag. The boundary half-edges in ascending h, keyed by their tail vertex.
__global__ __launch_bounds__(256) void k_fill_boundary_list(int nh, const int32_t* __restrict__ bscan,
                                                            const int32_t* __restrict__ tris,
                                                            uint32_t* __restrict__ keys, int32_t* __restrict__ vals) {
  const int h = blockIdx.x * 256 + threadIdx.x;
  if (h >= nh) return;
  const int p = bscan[h];
  if (bscan[h + 1] != p) {
    keys[p] = uint32_t(tris[h]);
    vals[p] = h;
  }
}

__global__ __launch_bounds__(256) void k_fill_positions(int nb, const int32_t* __restrict__ bh,
                                                        int32_t* __restrict__ bpos) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < nb) bpos[bh[i]] = i;
}

// succ of boundary half-edge bh[i] = (a -> b): rotate about b from next(h) across twins until a boundary
// half-edge leaves b. nxt[i]: its position, or -1 where the walk meets an edge without a twin (an open
// chain). The half-edges visited all leave b and are distinct, so the fan size bounds the walk.
__global__ __launch_bounds__(256) void k_fill_successor(int nb, const int32_t* __restrict__ bh,
                                                        const int32_t* __restrict__ tris,
                                                        const int32_t* __restrict__ twin,
                                                        const int32_t* __restrict__ deg,
                                                        const int32_t* __restrict__ bpos, int32_t* __restrict__ nxt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nb) return;
  int g = he_next(bh[i]);
  const int cap = deg[tris[g]];
  int out = -1;
  for (int step = 0; step < cap; ++step) {
    const int tw = twin[g];
    if (tw == -1) {
      out = bpos[g];
      break;
    }
    if (tw < 0) break;
    g = he_next(tw);
  }
  nxt[i] = out;
}

__global__ __launch_bounds__(256) void k_fill_min_init(int nb, const int32_t* __restrict__ nxt,
                                                       int32_t* __restrict__ jump, int32_t* __restrict__ mn) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nb) return;
  jump[i] = nxt[i];
  mn[i] = i;
}

// One doubling round from (jump, mn) to (jump2, mn2): mn = the smallest position among the 2^r members
// from i on; a chain that ends keeps jump = -1.
__global__ __launch_bounds__(256) void k_fill_min_round(int nb, const int32_t* __restrict__ jump,
                                                        const int32_t* __restrict__ mn, int32_t* __restrict__ jump2,
                                                        int32_t* __restrict__ mn2) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nb) return;
  const int j = jump[i];
  jump2[i] = j < 0 ? -1 : jump[j];
  mn2[i] = j < 0 ? mn[i] : min(mn[i], mn[j]);
}

// After 2^r >= nb steps a member of a chain has run off its end (jump = -1): the others lie on cycles and
// mn is their cycle's smallest position, the loop's start. lab: that start, -1 off the loops. The cycle is
// cut in front of its start, so that dist can count the steps to its last member. sflag [nb + 1]: the starts.
__global__ __launch_bounds__(256) void k_fill_cut(int nb, const int32_t* __restrict__ nxt,
                                                  const int32_t* __restrict__ jump, const int32_t* __restrict__ mn,
                                                  int32_t* __restrict__ lab, int32_t* __restrict__ jump2,
                                                  int32_t* __restrict__ dist, int32_t* __restrict__ sflag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) sflag[nb] = 0;
  if (i >= nb) return;
  const bool on = jump[i] >= 0;
  const int s = on ? mn[i] : -1;
  const int n2 = (on && nxt[i] != s) ? nxt[i] : -1;
  lab[i] = s;
  jump2[i] = n2;
  dist[i] = n2 < 0 ? 0 : 1;
  sflag[i] = on && s == i;
}

__global__ __launch_bounds__(256) void k_fill_rank_round(int nb, const int32_t* __restrict__ jump,
                                                         const int32_t* __restrict__ dist,
                                                         int32_t* __restrict__ jump2, int32_t* __restrict__ dist2) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nb) return;
  const int j = jump[i];
  jump2[i] = j < 0 ? -1 : jump[j];
  dist2[i] = j < 0 ? dist[i] : dist[i] + dist[j];
}

// sscan: the exclusive scan of the starts, which numbers the loops. len [nb + 1] was zeroed.
__global__ __launch_bounds__(256) void k_fill_loop_len(int nb, const int32_t* __restrict__ sscan,
                                                       const int32_t* __restrict__ dist, int32_t* __restrict__ len) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nb) return;
  if (sscan[i + 1] != sscan[i]) len[sscan[i]] = dist[i] + 1;
}

// tail [nb] ascends: the members that share a vertex are neighbours. dup[l] = 1 when two of loop l do.
// Every writer stores the same value.
__global__ __launch_bounds__(256) void k_fill_repeats(int nb, const uint32_t* __restrict__ tail,
                                                      const int32_t* __restrict__ lab,
                                                      const int32_t* __restrict__ sscan, int32_t* __restrict__ dup) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nb) return;
  const int s = lab[i];
  if (s < 0) return;
  const uint32_t v = tail[i];
  for (int j = i + 1; j < nb && tail[j] == v; ++j)
    if (lab[j] == s) {
      dup[sscan[s]] = 1;
      break;
    }
}

// One thread per possible loop (l <= nb; those past the count stay empty). len still holds the lengths.
__global__ __launch_bounds__(256) void k_fill_loop_class(int nb, const int32_t* __restrict__ n_loops,
                                                         const int32_t* __restrict__ len,
                                                         const int32_t* __restrict__ dup, int max_edges,
                                                         uint8_t* __restrict__ flags, int32_t* __restrict__ rows,
                                                         int32_t* __restrict__ is_short, int32_t* __restrict__ is_long) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l > nb) return;
  int f = 0, r = 0, sh = 0, lo = 0;
  if (l < *n_loops) {
    const int L = len[l];
    f = (dup[l] ? 1 : 0) | (L > max_edges ? 2 : 0);
    if (f == 0) {
      r = L - 2;
      sh = L <= kWaveMax;
      lo = !sh;
    }
  }
  if (l < nb) flags[l] = uint8_t(f);
  rows[l] = r;
  is_short[l] = sh;
  is_long[l] = lo;
}

__global__ __launch_bounds__(256) void k_fill_class_lists(int nb, const int32_t* __restrict__ short_scan,
                                                          const int32_t* __restrict__ long_scan,
                                                          int32_t* __restrict__ short_list,
                                                          int32_t* __restrict__ long_list) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= nb) return;
  if (short_scan[l + 1] != short_scan[l]) short_list[short_scan[l]] = l;
  if (long_scan[l + 1] != long_scan[l]) long_list[long_scan[l]] = l;
}

// The member r steps after the start holds v_{(L - r) % L}: the loop is listed against its half-edges.
__global__ __launch_bounds__(256) void k_fill_loop_verts(int nb, const uint32_t* __restrict__ tail,
                                                         const int32_t* __restrict__ lab,
                                                         const int32_t* __restrict__ dist,
                                                         const int32_t* __restrict__ sscan,
                                                         const int32_t* __restrict__ ptr,
                                                         int32_t* __restrict__ loop_verts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nb) return;
  const int s = lab[i];
  if (s < 0) return;
  const int l = sscan[s], L = dist[s] + 1, r = dist[s] - dist[i];
  if (r < 0 || r >= L) return;  // cannot happen on a cycle
  loop_verts[ptr[l] + (r == 0 ? 0 : L - r)] = int32_t(tail[i]);
}

// The rows of loop l from its finished split table, one thread per row.
__device__ __forceinline__ void fill_emit(int L, const uint8_t* S, int q, const int32_t* __restrict__ lv, int l,
                                          int row0, int32_t* __restrict__ new_tris, int32_t* __restrict__ new_loop) {
  int i, j, k;
  fill_row(L, S, q, &i, &j, &k);
  const size_t r = size_t(row0) + size_t(q);
  new_tris[3 * r] = lv[i];
  new_tris[3 * r + 1] = lv[j];
  new_tris[3 * r + 2] = lv[k];
  new_loop[r] = l;
}

// The wave class: loops of at most kWaveMax edges, one wave each, four to a block. Lane i owns entry
// (i, i + d) of diagonal d. The four waves step through the diagonals together, up to the longest of
// their loops, with one block barrier per diagonal.
__global__ __launch_bounds__(256) void k_fill_patch_wave(const int32_t* __restrict__ n_short,
                                                         const int32_t* __restrict__ short_list,
                                                         const int32_t* __restrict__ ptr,
                                                         const int32_t* __restrict__ row_ptr,
                                                         const int32_t* __restrict__ loop_verts,
                                                         const double* __restrict__ verts, double* __restrict__ area,
                                                         int32_t* __restrict__ new_tris,
                                                         int32_t* __restrict__ new_loop) {
  __shared__ double s_w[4][kWaveTab];
  __shared__ double s_p[4][3 * kWaveMax];
  __shared__ uint8_t s_s[4][kWaveTab];
  __shared__ int s_len[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, idx = blockIdx.x * 4 + wave;
  int l = -1, L = 0, base = 0;
  if (idx < *n_short) {
    l = short_list[idx];
    base = ptr[l];
    L = ptr[l + 1] - base;
    if (L > kWaveMax) L = 0;  // cannot happen: the class was chosen by length
  }
  double* W = s_w[wave];
  double* P = s_p[wave];
  uint8_t* S = s_s[wave];
  if (lane == 0) s_len[wave] = L;
  if (lane < L) {
    const size_t v = size_t(loop_verts[base + lane]);
    P[3 * lane] = verts[3 * v];
    P[3 * lane + 1] = verts[3 * v + 1];
    P[3 * lane + 2] = verts[3 * v + 2];
  }
  if (lane + 1 < L) {
    W[fill_at(L, lane, lane + 1)] = 0.0;
    S[fill_at(L, lane, lane + 1)] = 0;
  }
  __syncthreads();
  const int max_len = max(max(s_len[0], s_len[1]), max(s_len[2], s_len[3]));
  for (int d = 2; d < max_len; ++d) {  // block-uniform
    if (lane + d < L) {
      double w;
      int j;
      fill_relax(L, P, W, lane, lane + d, &w, &j);
      W[fill_at(L, lane, lane + d)] = w;
      S[fill_at(L, lane, lane + d)] = uint8_t(j);
    }
    __syncthreads();
  }
  if (L < 3) return;
  if (lane == 0) area[l] = W[fill_at(L, 0, L - 1)];
  if (lane < L - 2) fill_emit(L, S, lane, loop_verts + base, l, row_ptr[l], new_tris, new_loop);
}

// The long class: one block of 128 threads per loop of kWaveMax + 1 .. kMaxLoop edges, the table in
// dynamic LDS (kLongLds bytes: two blocks per CU). Thread i owns entry (i, i + d); one barrier per diagonal.
__global__ __launch_bounds__(128) void k_fill_patch_block(const int32_t* __restrict__ long_list,
                                                          const int32_t* __restrict__ ptr,
                                                          const int32_t* __restrict__ row_ptr,
                                                          const int32_t* __restrict__ loop_verts,
                                                          const double* __restrict__ verts, double* __restrict__ area,
                                                          int32_t* __restrict__ new_tris,
                                                          int32_t* __restrict__ new_loop) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* W = reinterpret_cast<double*>(smem);
  double* P = W + kLongTab;
  uint8_t* S = reinterpret_cast<uint8_t*>(P + 3 * kMaxLoop);
  const int l = long_list[blockIdx.x], base = ptr[l], L = ptr[l + 1] - base, i = threadIdx.x;
  if (L < 3 || L > kMaxLoop) return;  // block-uniform; cannot happen: the class was chosen by length
  if (i < L) {
    const size_t v = size_t(loop_verts[base + i]);
    P[3 * i] = verts[3 * v];
    P[3 * i + 1] = verts[3 * v + 1];
    P[3 * i + 2] = verts[3 * v + 2];
  }
  if (i + 1 < L) {
    W[fill_at(L, i, i + 1)] = 0.0;
    S[fill_at(L, i, i + 1)] = 0;
  }
  __syncthreads();
  for (int d = 2; d < L; ++d) {
    if (i + d < L) {
      double w;
      int j;
      fill_relax(L, P, W, i, i + d, &w, &j);
      W[fill_at(L, i, i + d)] = w;
      S[fill_at(L, i, i + d)] = uint8_t(j);
    }
    __syncthreads();
  }
  if (i == 0) area[l] = W[fill_at(L, 0, L - 1)];
  if (i < L - 2) fill_emit(L, S, i, loop_verts + base, l, row_ptr[l], new_tris, new_loop);
}

// Per new row: zero[r] = its area is 0.0; diag[r] = its edge (first, last vertex) is a diagonal of the
// patch (every row but a loop's first) and an edge of the mesh, found by bisection of the sorted
// half-edges. Both [n + 1], scanned afterwards.
__global__ __launch_bounds__(256) void k_fill_row_stats(int n, const int32_t* __restrict__ new_tris,
                                                        const int32_t* __restrict__ new_loop,
                                                        const int32_t* __restrict__ row_ptr,
                                                        const double* __restrict__ verts, int nh,
                                                        const int32_t* __restrict__ tris,
                                                        const int32_t* __restrict__ hs, int32_t* __restrict__ zero,
                                                        int32_t* __restrict__ diag) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r > n) return;
  int z = 0, dg = 0;
  if (r < n) {
    const int a = new_tris[3 * size_t(r)], b = new_tris[3 * size_t(r) + 1], d = new_tris[3 * size_t(r) + 2];
    z = fill_area(verts + 3 * size_t(a), verts + 3 * size_t(b), verts + 3 * size_t(d)) == 0.0;
    if (r != row_ptr[new_loop[r]]) {
      const int lo_v = min(a, d), hi_v = max(a, d);
      int lo = 0, hi = nh;  // the first sorted half-edge whose (min, max) is not below (lo_v, hi_v)
      while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        int u, w;
        half_edge(tris, hs[mid], u, w);
        const int mu = min(u, w), mw = max(u, w);
        if (mu < lo_v || (mu == lo_v && mw < hi_v)) lo = mid + 1;
        else hi = mid;
      }
      if (lo < nh) {
        int u, w;
        half_edge(tris, hs[lo], u, w);
        dg = min(u, w) == lo_v && max(u, w) == hi_v;
      }
    }
  }
  zero[r] = z;
  diag[r] = dg;
}

#define PQ_LAUNCH(kernel, blocks, ...)                                               \
  do {                                                                               \
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, c->stream, __VA_ARGS__);  \
    PQ_HIP(hipGetLastError());                                                       \
  } while (0)

struct FillOut {
  int64_t* n_loops;
  int32_t **loop_ptr, **loop_verts;
  uint8_t** loop_flags;
  double** loop_area;
  int64_t* n_new;
  int32_t **new_tris, **new_loop;
};

// Both entry points. verts == nullptr: the loops only.
int fill_run(const char* who, const int32_t* tris, int64_t n_tris, int64_t n_verts, const double* verts,
             int32_t max_edges, const FillOut& o, int64_t* stats, int32_t device) {
  const bool patch = verts != nullptr;
  const int nt = int(n_tris), nh = 3 * nt, nv = int(n_verts);
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  int32_t *d_tris, *d_twin, *d_bflag, *d_deg, *d_hs, *d_x, *d_first;
  PQ_TRY(c->arena.get(size_t(nh), &d_tris));
  PQ_TRY(c->arena.get(size_t(nh), &d_twin));
  PQ_TRY(c->arena.get(size_t(nh) + 1, &d_bflag));
  PQ_TRY(c->arena.get(size_t(nv), &d_deg));
  PQ_TRY(copy_in(c, d_tris, tris, size_t(nh)));
  PQ_HIP(hipMemsetAsync(d_deg, 0, size_t(nv) * 4, c->stream));
  int32_t n_boundary = 0;
  {
    ProfScope ps(c, "fill_table");
    PQ_TRY(mesh_half_edge_runs(c, d_tris, nt, nv, &d_hs, &d_x, &d_first));
    PQ_LAUNCH(k_fill_twins, ceil_div(nh, 256), nh, static_cast<const int32_t*>(d_tris),
              static_cast<const int32_t*>(d_hs), static_cast<const int32_t*>(d_x),
              static_cast<const int32_t*>(d_first), d_twin, d_bflag, d_deg);
    PQ_TRY(exclusive_scan_i32(c, d_bflag, int64_t(nh) + 1));
    PQ_TRY(fetch(c, &n_boundary, d_bflag + nh));  // B sizes every array of the loop search
  }
  if (n_boundary < 0 || n_boundary > nh) return fail(PYQSM_EHIP, "%s: %d boundary half-edges counted", who, n_boundary);
  if (n_boundary == 0) return 0;  // a closed mesh
  const int nb = n_boundary, rounds = bit_length(uint64_t(nb));
  const int gb = ceil_div(nb, 256), gl = ceil_div(nb + 1, 256);

  uint32_t* d_tail;
  int32_t *d_bh, *d_bpos, *d_nxt, *d_ja, *d_jb, *d_va, *d_vb, *d_lab, *d_sflag;
  PQ_TRY(c->arena.get(size_t(nb), &d_tail));
  PQ_TRY(c->arena.get(size_t(nb), &d_bh));
  PQ_TRY(c->arena.get(size_t(nh), &d_bpos));
  PQ_TRY(c->arena.get(size_t(nb), &d_nxt));
  PQ_TRY(c->arena.get(size_t(nb), &d_ja));
  PQ_TRY(c->arena.get(size_t(nb), &d_jb));
  PQ_TRY(c->arena.get(size_t(nb), &d_va));
  PQ_TRY(c->arena.get(size_t(nb), &d_vb));
  PQ_TRY(c->arena.get(size_t(nb), &d_lab));
  PQ_TRY(c->arena.get(size_t(nb) + 1, &d_sflag));
  {
    ProfScope ps(c, "fill_successor");
    PQ_LAUNCH(k_fill_boundary_list, ceil_div(nh, 256), nh, static_cast<const int32_t*>(d_bflag),
              static_cast<const int32_t*>(d_tris), d_tail, d_bh);
    // ascending (tail, h): the list ascends in h, the sort by tail is stable
    PQ_TRY(stable_sort_pairs_u32(c, &d_tail, &d_bh, nb, bit_length(uint64_t(nv))));
    PQ_LAUNCH(k_fill_positions, gb, nb, static_cast<const int32_t*>(d_bh), d_bpos);
    PQ_LAUNCH(k_fill_successor, gb, nb, static_cast<const int32_t*>(d_bh), static_cast<const int32_t*>(d_tris),
              static_cast<const int32_t*>(d_twin), static_cast<const int32_t*>(d_deg),
              static_cast<const int32_t*>(d_bpos), d_nxt);
  }

  int32_t *d_len, *d_dup, *d_rows, *d_short, *d_long, *d_short_list, *d_long_list, *d_loop_verts;
  uint8_t* d_flags;
  PQ_TRY(c->arena.get(size_t(nb) + 1, &d_len));
  PQ_TRY(c->arena.get(size_t(nb) + 1, &d_dup));
  PQ_TRY(c->arena.get(size_t(nb) + 1, &d_rows));
  PQ_TRY(c->arena.get(size_t(nb) + 1, &d_short));
  PQ_TRY(c->arena.get(size_t(nb) + 1, &d_long));
  PQ_TRY(c->arena.get(size_t(nb), &d_short_list));
  PQ_TRY(c->arena.get(size_t(nb), &d_long_list));
  PQ_TRY(c->arena.get(size_t(nb), &d_loop_verts));
  PQ_TRY(c->arena.get(size_t(nb), &d_flags));
  int32_t counts[5] = {0, 0, 0, 0, 0};  // loops, loop vertices, new rows, short loops, long loops
  {
    ProfScope ps(c, "fill_loops");
    PQ_HIP(hipMemsetAsync(d_len, 0, (size_t(nb) + 1) * 4, c->stream));
    PQ_HIP(hipMemsetAsync(d_dup, 0, (size_t(nb) + 1) * 4, c->stream));
    PQ_LAUNCH(k_fill_min_init, gb, nb, static_cast<const int32_t*>(d_nxt), d_ja, d_va);
    for (int r = 0; r < rounds; ++r) {
      PQ_LAUNCH(k_fill_min_round, gb, nb, static_cast<const int32_t*>(d_ja), static_cast<const int32_t*>(d_va), d_jb,
                d_vb);
      std::swap(d_ja, d_jb);
      std::swap(d_va, d_vb);
    }
    PQ_LAUNCH(k_fill_cut, gl, nb, static_cast<const int32_t*>(d_nxt), static_cast<const int32_t*>(d_ja),
              static_cast<const int32_t*>(d_va), d_lab, d_jb, d_vb, d_sflag);
    std::swap(d_ja, d_jb);
    std::swap(d_va, d_vb);
    for (int r = 0; r < rounds; ++r) {
      PQ_LAUNCH(k_fill_rank_round, gb, nb, static_cast<const int32_t*>(d_ja), static_cast<const int32_t*>(d_va), d_jb,
                d_vb);
      std::swap(d_ja, d_jb);
      std::swap(d_va, d_vb);
    }
    const int32_t* d_dist = d_va;
    PQ_TRY(exclusive_scan_i32(c, d_sflag, int64_t(nb) + 1));  // d_sflag[nb]: the loops
    PQ_LAUNCH(k_fill_loop_len, gb, nb, static_cast<const int32_t*>(d_sflag), d_dist, d_len);
    PQ_LAUNCH(k_fill_repeats, gb, nb, static_cast<const uint32_t*>(d_tail), static_cast<const int32_t*>(d_lab),
              static_cast<const int32_t*>(d_sflag), d_dup);
    PQ_LAUNCH(k_fill_loop_class, gl, nb, static_cast<const int32_t*>(d_sflag + nb), static_cast<const int32_t*>(d_len),
              static_cast<const int32_t*>(d_dup), int(max_edges), d_flags, d_rows, d_short, d_long);
    PQ_TRY(exclusive_scan_i32(c, d_len, int64_t(nb) + 1));  // now loop_ptr
    PQ_TRY(exclusive_scan_i32(c, d_rows, int64_t(nb) + 1));
    PQ_TRY(exclusive_scan_i32(c, d_short, int64_t(nb) + 1));
    PQ_TRY(exclusive_scan_i32(c, d_long, int64_t(nb) + 1));
    PQ_LAUNCH(k_fill_class_lists, gb, nb, static_cast<const int32_t*>(d_short), static_cast<const int32_t*>(d_long),
              d_short_list, d_long_list);
    PQ_LAUNCH(k_fill_loop_verts, gb, nb, static_cast<const uint32_t*>(d_tail), static_cast<const int32_t*>(d_lab),
              d_dist, static_cast<const int32_t*>(d_sflag), static_cast<const int32_t*>(d_len), d_loop_verts);
    PQ_TRY(download(c, counts + 0, d_sflag + nb, 1));
    PQ_TRY(download(c, counts + 1, d_len + nb, 1));
    PQ_TRY(download(c, counts + 2, d_rows + nb, 1));
    PQ_TRY(download(c, counts + 3, d_short + nb, 1));
    PQ_TRY(download(c, counts + 4, d_long + nb, 1));
    PQ_TRY(stream_sync(c));  // the sizes of the outputs and of the two patch launches
  }
  const int nl = counts[0], n_lv = counts[1], n_new = patch ? counts[2] : 0;
  const int n_short = counts[3], n_long = counts[4];
  if (nl < 0 || 3 * int64_t(nl) > nb || n_lv < 3 * int64_t(nl) || n_lv > nb || n_new < 0 || n_new > nb ||
      n_short < 0 || n_long < 0 || n_short + n_long > nl)
    return fail(PYQSM_EHIP, "%s: %d loops of %d vertices and %d rows counted on %d boundary half-edges", who, nl, n_lv,
                counts[2], nb);
  stats[0] = nb;
  stats[1] = nl;
  stats[5] = nb - n_lv;
  if (nl == 0) return 0;

  double *d_verts = nullptr, *d_area = nullptr;
  int32_t *d_new_tris = nullptr, *d_new_loop = nullptr, *d_zero = nullptr, *d_diag = nullptr;
  if (patch) {
    ProfScope ps(c, "fill_patches");
    PQ_TRY(c->arena.get(size_t(nv) * 3, &d_verts));
    PQ_TRY(c->arena.get(size_t(nl), &d_area));
    PQ_TRY(c->arena.get(size_t(n_new) * 3 + 1, &d_new_tris));
    PQ_TRY(c->arena.get(size_t(n_new) + 1, &d_new_loop));
    PQ_TRY(c->arena.get(size_t(n_new) + 1, &d_zero));
    PQ_TRY(c->arena.get(size_t(n_new) + 1, &d_diag));
    PQ_TRY(copy_in(c, d_verts, verts, size_t(nv) * 3));
    PQ_HIP(hipMemsetAsync(d_area, 0, size_t(nl) * 8, c->stream));
    if (n_short > 0)
      PQ_LAUNCH(k_fill_patch_wave, ceil_div(n_short, 4), static_cast<const int32_t*>(d_short + nb),
                static_cast<const int32_t*>(d_short_list), static_cast<const int32_t*>(d_len),
                static_cast<const int32_t*>(d_rows), static_cast<const int32_t*>(d_loop_verts),
                static_cast<const double*>(d_verts), d_area, d_new_tris, d_new_loop);
    if (n_long > 0) {
      PQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_fill_patch_block),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, int(kLongLds)));
      hipLaunchKernelGGL(k_fill_patch_block, dim3(n_long), dim3(128), kLongLds, c->stream,
                         static_cast<const int32_t*>(d_long_list), static_cast<const int32_t*>(d_len),
                         static_cast<const int32_t*>(d_rows), static_cast<const int32_t*>(d_loop_verts),
                         static_cast<const double*>(d_verts), d_area, d_new_tris, d_new_loop);
      PQ_HIP(hipGetLastError());
    }
    PQ_LAUNCH(k_fill_row_stats, ceil_div(n_new + 1, 256), n_new, static_cast<const int32_t*>(d_new_tris),
              static_cast<const int32_t*>(d_new_loop), static_cast<const int32_t*>(d_rows),
              static_cast<const double*>(d_verts), nh, static_cast<const int32_t*>(d_tris),
              static_cast<const int32_t*>(d_hs), d_zero, d_diag);
    PQ_TRY(exclusive_scan_i32(c, d_zero, int64_t(n_new) + 1));
    PQ_TRY(exclusive_scan_i32(c, d_diag, int64_t(n_new) + 1));
  }

  OutBufs out;
  int32_t* h_ptr = out.get<int32_t>(size_t(nl) + 1);
  int32_t* h_lv = out.get<int32_t>(size_t(n_lv));
  uint8_t* h_flags = patch ? out.get<uint8_t>(size_t(nl)) : nullptr;
  double* h_area = patch ? out.get<double>(size_t(nl)) : nullptr;
  int32_t* h_new = n_new > 0 ? out.get<int32_t>(size_t(n_new) * 3) : nullptr;
  int32_t* h_new_loop = n_new > 0 ? out.get<int32_t>(size_t(n_new)) : nullptr;
  if (!h_ptr || !h_lv || (patch && (!h_flags || !h_area)) || (n_new > 0 && (!h_new || !h_new_loop)))
    return fail(PYQSM_ENOMEM, "%s: no host memory for %d loops and %d rows", who, nl, n_new);
  int32_t row_counts[2] = {0, 0};
  PQ_TRY(download(c, h_ptr, d_len, size_t(nl) + 1));
  PQ_TRY(download(c, h_lv, d_loop_verts, size_t(n_lv)));
  if (patch) {
    PQ_TRY(download(c, h_flags, d_flags, size_t(nl)));
    PQ_TRY(download(c, h_area, d_area, size_t(nl)));
    PQ_TRY(download(c, h_new, d_new_tris, size_t(n_new) * 3));
    PQ_TRY(download(c, h_new_loop, d_new_loop, size_t(n_new)));
    PQ_TRY(download(c, row_counts + 0, d_zero + n_new, 1));
    PQ_TRY(download(c, row_counts + 1, d_diag + n_new, 1));
  }
  PQ_TRY(stream_sync(c));
  if (patch) {
    for (int l = 0; l < nl; ++l) {
      stats[2] += h_flags[l] == 0;
      stats[3] += (h_flags[l] & 1) != 0;
      stats[4] += (h_flags[l] & 2) != 0;
    }
    stats[6] = row_counts[0];
    stats[7] = row_counts[1];
  }
  out.kept = true;
  *o.n_loops = nl;
  *o.loop_ptr = h_ptr;
  *o.loop_verts = h_lv;
  if (patch) {
    *o.loop_flags = h_flags;
    *o.loop_area = h_area;
    *o.n_new = n_new;
    *o.new_tris = h_new;
    *o.new_loop = h_new_loop;
  }
  return 0;
}

// The input checks of pyqsm_mesh_topology.
int fill_check(const char* who, const int32_t* tris, int64_t n_tris, int64_t n_verts) {
  if (n_tris < 0 || n_verts < 0) return fail(PYQSM_EINVAL, "negative size");
  if (n_tris > 0 && !tris) return fail(PYQSM_EINVAL, "%s: NULL pointer", who);
  if (n_tris >= kFillMaxTris) return fail(PYQSM_ERANGE, "%s: 2^29 triangles or more", who);
  if (n_verts > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "%s: more than 2^31 vertices", who);
  for (int64_t t = 0; t < n_tris; ++t) {
    const int32_t a = tris[3 * t], b = tris[3 * t + 1], d = tris[3 * t + 2];
    if (a < 0 || b < 0 || d < 0 || a >= n_verts || b >= n_verts || d >= n_verts)
      return fail(PYQSM_EINVAL, "triangle %lld has a vertex index outside [0, %lld)", (long long)t,
                  (long long)n_verts);
    if (a == b || b == d || a == d)
      return fail(PYQSM_EINVAL, "triangle %lld repeats a vertex index (remove degenerate triangles first)",
                  (long long)t);
  }
  return 0;
}

}  // namespace

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_mesh_boundary_loops(const int32_t* tris, int64_t n_tris, int64_t n_verts, int64_t* n_loops,
                              int32_t** loop_ptr, int32_t** loop_verts, int64_t* stats, int32_t device) {
  PQ_API_RANGE("pyqsm_mesh_boundary_loops");
  if (n_loops) *n_loops = 0;
  if (loop_ptr) *loop_ptr = nullptr;
  if (loop_verts) *loop_verts = nullptr;
  if (!n_loops || !loop_ptr || !loop_verts || !stats)
    return fail(PYQSM_EINVAL, "pyqsm_mesh_boundary_loops: NULL pointer");
  std::fill(stats, stats + 8, int64_t(0));
  PQ_TRY(fill_check("pyqsm_mesh_boundary_loops", tris, n_tris, n_verts));
  if (n_tris == 0) return 0;  // nothing to launch
  const FillOut o{n_loops, loop_ptr, loop_verts, nullptr, nullptr, nullptr, nullptr, nullptr};
  return fill_run("pyqsm_mesh_boundary_loops", tris, n_tris, n_verts, nullptr, kMaxLoop, o, stats, device);
}

int pyqsm_mesh_fill_holes(const int32_t* tris, int64_t n_tris, int64_t n_verts, const double* verts, int32_t max_edges,
                          int64_t* n_loops, int32_t** loop_ptr, int32_t** loop_verts, uint8_t** loop_flags,
                          double** loop_area, int64_t* n_new, int32_t** new_tris, int32_t** new_loop, int64_t* stats,
                          int32_t device) {
  PQ_API_RANGE("pyqsm_mesh_fill_holes");
  if (n_loops) *n_loops = 0;
  if (n_new) *n_new = 0;
  if (loop_ptr) *loop_ptr = nullptr;
  if (loop_verts) *loop_verts = nullptr;
  if (loop_flags) *loop_flags = nullptr;
  if (loop_area) *loop_area = nullptr;
  if (new_tris) *new_tris = nullptr;
  if (new_loop) *new_loop = nullptr;
  if (!n_loops || !loop_ptr || !loop_verts || !loop_flags || !loop_area || !n_new || !new_tris || !new_loop || !stats)
    return fail(PYQSM_EINVAL, "pyqsm_mesh_fill_holes: NULL pointer");
  std::fill(stats, stats + 8, int64_t(0));
  if (max_edges > kMaxLoop)
    return fail(PYQSM_EINVAL, "pyqsm_mesh_fill_holes: max_edges = %d is above PYQSM_FILL_MAX_LOOP = %d", int(max_edges),
                kMaxLoop);
  if (max_edges <= 0) max_edges = kMaxLoop;
  PQ_TRY(fill_check("pyqsm_mesh_fill_holes", tris, n_tris, n_verts));
  if (n_tris > 0 && !verts) return fail(PYQSM_EINVAL, "pyqsm_mesh_fill_holes: NULL pointer");
  if (n_tris == 0) return 0;  // nothing to launch
  const FillOut o{n_loops, loop_ptr, loop_verts, loop_flags, loop_area, n_new, new_tris, new_loop};
  return fill_run("pyqsm_mesh_fill_holes", tris, n_tris, n_verts, verts, max_edges, o, stats, device);
}

}  // extern "C"
