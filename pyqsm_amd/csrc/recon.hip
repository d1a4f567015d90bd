// recon.hip — surface reconstruction by exact ball pivoting of lattice points with normals, on gfx950.
//
//   pyqsm_ball_pivot    every oriented triangle (a, b, c) of cloud points a ball of radius rho can rest on
//                       from the normals' side: the alpha-exposed facets of the alpha shape, alpha = rho,
//                       in place of the traversal-ordered front of Open3D's
//                       create_from_point_cloud_ball_pivoting.
//
// A triple is emitted iff (1) with n = (b - a) x (c - a) the three vertex normals all have a strictly
// positive dot product with n (the triple is oriented so that they do, and dropped if neither
// orientation does) and (2) the ball of radius rho through a, b, c whose centre lies on the +n side
// holds no other cloud point strictly inside. With e1 = b - a, e2 = c - a, e3 = e2 - e1, u = p - a,
// n2 = |n|^2, E = |e1|^2 |e2|^2 |e3|^2, H = 4 rho^2 n2 - E (the ball exists iff H >= 0),
// w = |e1|^2 (e2 x n) + |e2|^2 (n x e1), D = n.u and N = |u|^2 n2 - w.u the centre is
// a + w / (2 n2) + sqrt(H) n / (2 n2), and p is strictly inside iff N < sqrt(H) D, on the ball iff equal.
//
// Exactness. Everything within the ball lies within L = 2 rho of a, so stencil points with |u| > L are
// skipped and every triangle edge is at most L. rho^2 <= 2^22 lattice units^2 (the entry point refuses
// more), hence L <= 2^12 and
//   |n_i| <= L^2 = 2^24, n2 <= L^4 = 2^48, |D| <= |n| |u| <= L^3 = 2^36: exact in fp64 and in int64;
//   |w_i| <= |e1|^2 |e2| |n| + |e2|^2 |n| |e1| <= 2 L^5 = 2^61: int64;
//   E <= L^6 = 2^72, 4 rho^2 n2 <= L^6: H < 2^73, |N| <= |u|^2 n2 + |w| |u| <= 3 L^6 < 2^74: __int128;
//   N^2 < 2^148 against D^2 H <= 2^72 * 2^72 = 2^144: four 64-bit limbs (recon_exact.hpp).
// int64 w is what sets the bound: L = 2^13 would need 2^66 there.
// The filter (recon_filter in recon_exact.hpp, so that the host can run it). Each test first runs in fp64: D exactly; Nf = fl(u2 n2 - w.u) from four products with
// M = |u2 n2| + sum |w_i u_i| (w_i rounded once to fp64, each product once, three additions:
// |Nf - N| <= 2^-50 M); sH = fl(sqrt(fl(H))) and rhs = fl(sH D) with |rhs - sqrt(H) D| <= 2^-49 |rhs|
// (H is put together from two halves, two roundings, halved by the root; a root within two units of
// the last place; one product). The sign of diff = fl(Nf - rhs) is taken only when
// |diff| > 2^-46 (M + |rhs|), eight times the sum of those bounds; everything else, every exact tie
// among it, is classified by the integers. Decisions per triangle are integer comparisons only.
//
// Ties. A point exactly on the ball does not block. If every tie point of a surviving triple lies in
// its plane (D = 0; they are concyclic with it) the triple is kept iff its smallest index is the
// smallest among the ties too and no tie point lies strictly beyond the edge opposite that vertex:
// the fan from the smallest index of a cocircular polygon. With a tie point off the plane the triple
// is kept and counted (n_unresolved_ties).
//
// Locality. Cells of the shared grid (grid.hpp) have an integer edge >= 2 rho + 1: the 27-cell stencil
// of a's cell holds every point within 2 rho of a, also when a point exactly on a cell face is binned
// one cell low by the rounding of the reciprocal edge.
//
// Shape. a is the smallest index of its triple, so each unordered triple is met once. One block serves
// up to kReconSlice points of one cell: the index pairs (b, c) of the stencil with all three edges <= 2 rho,
// H >= 0 and agreeing normals are ballot-compacted into an LDS queue, one lane owns one candidate and
// tests it against the stencil, whose coordinates are staged in LDS in chunks of kReconChunk and read as
// broadcasts; a wave skips a chunk once all its lanes are blocked. Survivors are appended through one
// 64-bit integer atomicAdd and sorted by their unique (a, b, c) at the end: the bytes that leave the
// library do not depend on the order of the appends.
//
// Several radii, ascending. Level 0 emits every triangle above. After a level the directed half-edges
// of all triangles so far are sorted by (u, v); a vertex is INNER when it has triangles and every
// incident half-edge has its reverse. A triple exposed at a later level is accepted iff none of its
// vertices is inner and none of its three half-edges is in the table; all of a level at once.
#include "grid.hpp"
#include "recon_exact.hpp"
#include "recon_grid.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace pyqsm {

static constexpr int kReconChunk = PYQSM_RECON_CHUNK;  // stencil points staged at a time (24 KiB)
static constexpr int kReconSlice = PYQSM_RECON_SLICE;  // points of a cell one block serves
static constexpr uint64_t kReconMaxRho2 = PYQSM_RECON_MAX_RHO2;
// ten seconds of the triangle pass at the 1.1e11 estimated pair tests per second measured on one MI355X
// (profiles/recon_perf.jsonl)
static constexpr int64_t kReconDefaultMaxTests = PYQSM_RECON_DEFAULT_MAX_TESTS;

struct alignas(8) Normal16 {
  int16_t x, y, z, pad;
};

// the points in the grid's order: coordinates relative to the cloud's corner, normals as one 8-byte record
__global__ __launch_bounds__(256) void k_recon_gather(int n, const int32_t* __restrict__ order,
                                                      const int32_t* __restrict__ ijk,
                                                      const int16_t* __restrict__ nrm, int x0, int y0, int z0,
                                                      int32_t* __restrict__ lx, int32_t* __restrict__ ly,
                                                      int32_t* __restrict__ lz, Normal16* __restrict__ ln) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const size_t i = size_t(order[p]);
  lx[p] = int32_t(int64_t(ijk[3 * i]) - x0);
  ly[p] = int32_t(int64_t(ijk[3 * i + 1]) - y0);
  lz[p] = int32_t(int64_t(ijk[3 * i + 2]) - z0);
  ln[p] = Normal16{nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2], 0};
}

// is the directed half-edge (u, v) in the table sorted by (u, v)?
__device__ __forceinline__ bool recon_has_half_edge(int n, const int32_t* __restrict__ hu,
                                                    const int32_t* __restrict__ hv, int u, int v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const int mu = hu[mid];
    if (mu < u || (mu == u && hv[mid] < v)) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && hu[lo] == u && hv[lo] == v;
}

// 0: no candidate; 1: (a, b, c) as given; 2: (a, c, b)
__device__ __forceinline__ int recon_pair(const int32_t* __restrict__ lx, const int32_t* __restrict__ ly,
                                          const int32_t* __restrict__ lz, const Normal16* __restrict__ ln,
                                          const int32_t* __restrict__ lorig, const int32_t* __restrict__ state,
                                          int pa, int oa, int pb, int pc, uint64_t four_r2) {
  const int64_t ax = lx[pa], ay = ly[pa], az = lz[pa];
  const int64_t b0 = lx[pb] - ax, b1 = ly[pb] - ay, b2 = lz[pb] - az;  // below 2^27 inside a stencil
  if (uint64_t(b0 * b0 + b1 * b1 + b2 * b2) > four_r2) return 0;
  const int ob = lorig[pb];
  if (ob <= oa) return 0;
  const int64_t c0 = lx[pc] - ax, c1 = ly[pc] - ay, c2 = lz[pc] - az;
  if (uint64_t(c0 * c0 + c1 * c1 + c2 * c2) > four_r2) return 0;
  const int oc = lorig[pc];
  if (oc <= oa) return 0;
  if (state && (state[ob] == 1 || state[oc] == 1)) return 0;  // an inner vertex takes no new triangle
  const int64_t a[3] = {0, 0, 0}, b[3] = {b0, b1, b2}, c[3] = {c0, c1, c2};
  ReconTri t;
  if (!recon_setup(a, b, c, four_r2, &t)) return 0;
  const Normal16 na = ln[pa], nb = ln[pb], nc = ln[pc];
  const int64_t da = t.n[0] * na.x + t.n[1] * na.y + t.n[2] * na.z;
  const int64_t db = t.n[0] * nb.x + t.n[1] * nb.y + t.n[2] * nb.z;
  const int64_t dc = t.n[0] * nc.x + t.n[1] * nc.y + t.n[2] * nc.z;
  if (da > 0 && db > 0 && dc > 0) return 1;
  if (da < 0 && db < 0 && dc < 0) return 2;
  return 0;
}

// The rare path, kept out of line so that its wide integers do not cost the scan its registers:
// 1 = p is strictly inside the ball of (pa, pb, pc), 2 = on it and off the plane, 4 = on it, in the plane,
// and either of a lower index than a or strictly beyond the edge opposite a.
__device__ __noinline__ int recon_exact_test(const int32_t* __restrict__ lx, const int32_t* __restrict__ ly,
                                             const int32_t* __restrict__ lz, const int32_t* __restrict__ lorig,
                                             int pa, int pb, int pc, int p, uint64_t four_r2) {
  const int64_t a[3] = {lx[pa], ly[pa], lz[pa]}, b[3] = {lx[pb], ly[pb], lz[pb]}, c[3] = {lx[pc], ly[pc], lz[pc]};
  ReconTri tri;
  recon_setup(a, b, c, four_r2, &tri);  // a candidate: recon_pair said so
  const int64_t u[3] = {lx[p] - a[0], ly[p] - a[1], lz[p] - a[2]};
  const int where = recon_classify(tri, u);
  if (where == kReconInside) return 1;
  if (where == kReconTieOffPlane) return 2;
  if (where == kReconTieCoplanar && (lorig[p] < lorig[pa] || recon_beyond_bc(tri, u))) return 4;
  return 0;
}

// stats: [0] ball tests, [1] tests classified by the integers, [2] candidates, [3] triangles kept with a
// tie point off their plane. state (level > 0): 1 = inner vertex, by original index; hu / hv: the
// half-edges of the earlier levels. rows: (a, b, c, level) appended at *cursor while below tri_cap.
__global__ __launch_bounds__(256) void k_recon_tris(
    int ncell, const int32_t* __restrict__ blk_start, int nx, int ny, const int32_t* __restrict__ start,
    const int32_t* __restrict__ lx, const int32_t* __restrict__ ly, const int32_t* __restrict__ lz,
    const Normal16* __restrict__ ln, const int32_t* __restrict__ lorig, unsigned long long four_r2, int level,
    const int32_t* __restrict__ state, int n_he, const int32_t* __restrict__ hu, const int32_t* __restrict__ hv,
    long long tri_cap, int4* __restrict__ rows, unsigned long long* __restrict__ cursor,
    unsigned long long* __restrict__ stats) {
  __shared__ double sx[kReconChunk], sy[kReconChunk], sz[kReconChunk];
  __shared__ int qa[512], qb[512], qc[512];
  __shared__ int qn, s_cell;
  __shared__ unsigned long long s_tests, s_exact, s_cand, s_unres;
  const int t = threadIdx.x;
  if (t == 0) {
    int lo = 0, hi = ncell;  // the cell c with blk_start[c] <= blockIdx.x < blk_start[c + 1]
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (blk_start[mid + 1] <= int(blockIdx.x)) lo = mid + 1;
      else hi = mid;
    }
    s_cell = lo;
    qn = 0;
    s_tests = s_exact = s_cand = s_unres = 0;
  }
  __syncthreads();
  const int c = s_cell;
  if (c >= ncell) return;  // block-uniform; cannot happen for a block inside the scanned total
  const int a0 = start[c] + (int(blockIdx.x) - blk_start[c]) * kReconSlice;  // this block's points of the cell
  const int m = min(kReconSlice, start[c + 1] - a0);
  if (m <= 0) return;
  const ReconStencil st = recon_stencil(nx, ny, c, start);
  const int S = st.total;
  const unsigned long long SS = (unsigned long long)S * (unsigned long long)S;
  const bool one_chunk = S <= kReconChunk;
  if (one_chunk) {
    for (int j = t; j < S; j += 256) {
      const int p = st.at(j);
      sx[j] = double(lx[p]);
      sy[j] = double(ly[p]);
      sz[j] = double(lz[p]);
    }
    __syncthreads();
  }
  const double four_r2d = double(four_r2);
  unsigned my_exact = 0, my_cand = 0, my_unres = 0;
  unsigned long long my_tests = 0;
  int cur_a = 0;                // both block-uniform: the point whose pairs are being listed, and how far
  unsigned long long cand = 0;
  for (;;) {
    // fill the queue with candidate triples, 256 index pairs (bj, cj) of the current point at a time
    int have = qn;
    __syncthreads();  // every wave has read qn before the first of them adds to it
    while (have < 256 && cur_a < m) {
      const int pa = a0 + cur_a, oa = lorig[pa];
      if (state && state[oa] == 1) {  // an inner vertex
        ++cur_a;
        cand = 0;
        continue;
      }
      const unsigned long long idx = cand + (unsigned)t;
      int pb = 0, pc = 0, how = 0;
      if (idx < SS) {
        int bj, cj;
        if (SS < (1ull << 32)) {
          bj = int(unsigned(idx) / unsigned(S));
          cj = int(unsigned(idx) - unsigned(bj) * unsigned(S));
        } else {
          bj = int(idx / (unsigned long long)S);
          cj = int(idx - (unsigned long long)bj * (unsigned long long)S);
        }
        if (bj < cj) {
          pb = st.at(bj);
          pc = st.at(cj);
          how = recon_pair(lx, ly, lz, ln, lorig, state, pa, oa, pb, pc, four_r2);
        }
      }
      const bool active = how != 0;
      const unsigned long long mask = __ballot(active);
      int base = 0;
      if ((t & 63) == 0 && mask) base = atomicAdd(&qn, __popcll(mask));
      base = __shfl(base, 0);
      if (active) {
        const int at = base + __popcll(mask & ((1ull << (t & 63)) - 1ull));
        qa[at] = pa;
        qb[at] = how == 1 ? pb : pc;
        qc[at] = how == 1 ? pc : pb;
      }
      cand += 256;
      if (cand >= SS) {
        ++cur_a;
        cand = 0;
      }
      __syncthreads();
      have = qn;
      __syncthreads();
    }
    if (have == 0) break;
    const int take = have < 256 ? have : 256;
    const bool mine = t < take;
    int pa = 0, pb = 0, pc = 0;
    double ax = 0, ay = 0, az = 0;
    ReconFilterTri ft = {{0, 0, 0}, {0, 0, 0}, 0, 0};
    if (mine) {
      pa = qa[t];
      pb = qb[t];
      pc = qc[t];
      const int64_t a[3] = {lx[pa], ly[pa], lz[pa]}, b[3] = {lx[pb], ly[pb], lz[pb]}, cc[3] = {lx[pc], ly[pc], lz[pc]};
      ReconTri tri;
      recon_setup(a, b, cc, four_r2, &tri);  // a candidate: recon_pair said so
      ax = double(a[0]);
      ay = double(a[1]);
      az = double(a[2]);
      ft = recon_filter_setup(tri);
    }
    bool blocked = !mine, unresolved = false, tie_drop = false;
    for (int k0 = 0; k0 < S; k0 += kReconChunk) {
      const int cn = S - k0 < kReconChunk ? S - k0 : kReconChunk;
      if (!one_chunk) {
        __syncthreads();
        for (int j = t; j < cn; j += 256) {
          const int p = st.at(k0 + j);
          sx[j] = double(lx[p]);
          sy[j] = double(ly[p]);
          sz[j] = double(lz[p]);
        }
        __syncthreads();
      }
      if (__ballot(!blocked) == 0) continue;  // the whole wave is done with this tile of candidates
      for (int j = 0; j < cn && !blocked; ++j) {
        const double ux = sx[j] - ax, uy = sy[j] - ay, uz = sz[j] - az;
        const double u2 = (ux * ux + uy * uy) + uz * uz;
        if (u2 > four_r2d) continue;  // beyond 2 rho of a: outside every ball through a
        const int side = recon_filter(ft, ux, uy, uz);  // recon_exact.hpp: the host checks the same function
        if (side == kReconFilterOutside) continue;
        if (side == kReconFilterInside) {
          blocked = true;
          break;
        }
        const int p = st.at(k0 + j);
        if (p == pa || p == pb || p == pc) continue;
        ++my_exact;
        const int where = recon_exact_test(lx, ly, lz, lorig, pa, pb, pc, p, four_r2);
        blocked = (where & 1) != 0;
        unresolved = unresolved || (where & 2) != 0;
        tie_drop = tie_drop || (where & 4) != 0;
      }
    }
    if (mine) {
      my_tests += (unsigned long long)S;
      ++my_cand;
      if (!blocked && (unresolved || !tie_drop)) {
        const int oa = lorig[pa], ob = lorig[pb], oc = lorig[pc];
        bool ok = true;
        if (n_he > 0)
          ok = !recon_has_half_edge(n_he, hu, hv, oa, ob) && !recon_has_half_edge(n_he, hu, hv, ob, oc) &&
               !recon_has_half_edge(n_he, hu, hv, oc, oa);
        if (ok) {
          if (unresolved) ++my_unres;
          const unsigned long long at = atomicAdd(cursor, 1ull);
          if ((long long)at < tri_cap) rows[at] = make_int4(oa, ob, oc, level);
        }
      }
    }
    // drop the served entries
    __syncthreads();
    const int rest = have - take;
    int ra = 0, rb = 0, rc = 0;
    if (t < rest) {
      ra = qa[take + t];
      rb = qb[take + t];
      rc = qc[take + t];
    }
    __syncthreads();
    if (t < rest) {
      qa[t] = ra;
      qb[t] = rb;
      qc[t] = rc;
    }
    if (t == 0) qn = rest;
    __syncthreads();
  }
  if (my_tests) atomicAdd(&s_tests, my_tests);
  if (my_exact) atomicAdd(&s_exact, (unsigned long long)my_exact);
  if (my_cand) atomicAdd(&s_cand, (unsigned long long)my_cand);
  if (my_unres) atomicAdd(&s_unres, (unsigned long long)my_unres);
  __syncthreads();
  if (t == 0) {
    atomicAdd(&stats[0], s_tests);
    if (s_exact) atomicAdd(&stats[1], s_exact);
    if (s_cand) atomicAdd(&stats[2], s_cand);
    if (s_unres) atomicAdd(&stats[3], s_unres);
  }
}

// ---- the half-edge table and the inner vertices --------------------------------------------------
// half-edge h = 3 t + k of triangle t: (v_k, v_{k+1})
__global__ __launch_bounds__(256) void k_recon_half_edges(int n_he, const int4* __restrict__ rows,
                                                          int32_t* __restrict__ eu, int32_t* __restrict__ ev) {
  const int h = blockIdx.x * 256 + threadIdx.x;
  if (h >= n_he) return;
  const int4 r = rows[h / 3];
  const int k = h % 3;
  eu[h] = k == 0 ? r.x : k == 1 ? r.y : r.z;
  ev[h] = k == 0 ? r.y : k == 1 ? r.z : r.x;
}

__global__ __launch_bounds__(256) void k_recon_permute2(int e, const int32_t* __restrict__ perm,
                                                        const int32_t* __restrict__ eu,
                                                        const int32_t* __restrict__ ev, int32_t* __restrict__ hu,
                                                        int32_t* __restrict__ hv) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= e) return;
  hu[i] = eu[perm[i]];
  hv[i] = ev[perm[i]];
}

// state[v] |= 1: v has a triangle; |= 2: a half-edge at v lacks its reverse. Inner: state == 1.
__global__ __launch_bounds__(256) void k_recon_vertex_state(int n_he, const int32_t* __restrict__ hu,
                                                            const int32_t* __restrict__ hv,
                                                            int32_t* __restrict__ state) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_he) return;
  const int u = hu[i], v = hv[i];
  const int bits = recon_has_half_edge(n_he, hu, hv, v, u) ? 1 : 3;
  atomicOr(&state[u], bits);
  atomicOr(&state[v], bits);
}

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_ball_pivot(const int32_t* ijk, const int16_t* normals, int64_t n, const uint64_t* rho2, int32_t n_levels,
                     int64_t max_tests, int64_t* n_tris, int32_t** tris, int64_t* stats, int32_t device) {
  PQ_API_RANGE("pyqsm_ball_pivot");
  if (tris) *tris = nullptr;
  if (n_tris) *n_tris = 0;
  if (stats) std::fill(stats, stats + 8, int64_t(0));
  if (n < 0 || n_levels < 1) return fail(PYQSM_EINVAL, "pyqsm_ball_pivot: negative size or no radius");
  if (!rho2 || !n_tris || !tris || (n > 0 && (!ijk || !normals)))
    return fail(PYQSM_EINVAL, "pyqsm_ball_pivot: NULL pointer");
  for (int32_t k = 0; k < n_levels; ++k) {
    if (rho2[k] == 0) return fail(PYQSM_EINVAL, "pyqsm_ball_pivot: rho^2 must be positive");
    if (k > 0 && rho2[k] < rho2[k - 1]) return fail(PYQSM_EINVAL, "pyqsm_ball_pivot: the radii must ascend");
    if (rho2[k] > kReconMaxRho2) {
      int shift = 1;
      while ((rho2[k] >> (2 * shift)) > kReconMaxRho2) ++shift;
      return fail(PYQSM_EINVAL,
                  "pyqsm_ball_pivot: rho^2 = %llu exceeds 2^22 lattice units^2 (rho <= 2048): a quantum 2^%d times "
                  "as large would fit",
                  (unsigned long long)rho2[k], shift);
    }
  }
  if (n > (int64_t(1) << 26))  // 3 (8 n + 1024) half-edges are counted in 32 bits
    return fail(PYQSM_ERANGE, "pyqsm_ball_pivot: more than 2^26 points per call");
  if (max_tests <= 0) max_tests = kReconDefaultMaxTests;
  if (n < 3) return 0;  // no triple: no device work

  int32_t mn[3], mx[3];
  for (int a = 0; a < 3; ++a) mn[a] = mx[a] = ijk[a];
  for (int64_t i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) {
      mn[a] = std::min(mn[a], ijk[3 * i + a]);
      mx[a] = std::max(mx[a], ijk[3 * i + a]);
    }
  for (int a = 0; a < 3; ++a)
    if (int64_t(mx[a]) - mn[a] > 0x7FFFFFFFLL)
      return fail(PYQSM_EINVAL, "pyqsm_ball_pivot: the cloud spans more than 2^31 lattice units");
  const double bbox[6] = {double(mn[0]), double(mn[1]), double(mn[2]), double(mx[0]), double(mx[1]), double(mx[2])};

  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  const int N = int(n);
  const int64_t tri_cap = 8 * n + 1024;
  int32_t *d_ijk, *d_state = nullptr, *d_lx, *d_ly, *d_lz;
  int16_t* d_nrm;
  Normal16* d_ln;
  double* d_xyz;
  int4* d_rows;
  unsigned long long* d_counters;  // cursor, stats[4], then est[4] of the level being planned
  const size_t n_counters = 9;
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_ijk));
  PQ_TRY(c->arena.get(size_t(n) * 3 + 1, &d_nrm));
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_xyz));
  PQ_TRY(c->arena.get(size_t(n), &d_lx));
  PQ_TRY(c->arena.get(size_t(n), &d_ly));
  PQ_TRY(c->arena.get(size_t(n), &d_lz));
  PQ_TRY(c->arena.get(size_t(n), &d_ln));
  PQ_TRY(c->arena.get(size_t(tri_cap), &d_rows));
  PQ_TRY(c->arena.get(n_counters, &d_counters));
  if (n_levels > 1) PQ_TRY(c->arena.get(size_t(n), &d_state));
  PQ_TRY(copy_in(c, d_ijk, ijk, size_t(n) * 3));
  PQ_TRY(copy_in(c, d_nrm, normals, size_t(n) * 3));
  PQ_HIP(hipMemsetAsync(d_counters, 0, n_counters * 8, c->stream));
  hipLaunchKernelGGL(k_recon_to_f64, dim3(ceil_div(3 * n, 256)), dim3(256), 0, c->stream, 3 * n,
                     static_cast<const int32_t*>(d_ijk), d_xyz);
  PQ_HIP(hipGetLastError());

  if (d_state) PQ_HIP(hipMemsetAsync(d_state, 0, size_t(n) * 4, c->stream));  // no vertex is inner yet

  // Everything a level takes from the arena (its grid, its block map, the sort's temporaries) is given
  // back when the level is done: the call holds one level's scratch, however many radii there are.
  const Arena::Mark base = c->arena.mark();
  struct LevelPlan {
    uint64_t four_r2;
    DevGrid g;
    int32_t* d_blk;
    int32_t n_blocks;
    int64_t est_tests, max_stencil, max_cell;
  };
  // The grid of a level, the block map of its triangle pass and the estimate of its pair tests
  // (synchronises); with `gather` also the points in the grid's order, which the triangle pass reads.
  auto plan_level = [&](int32_t level, bool gather, LevelPlan* lp) -> int {
    ProfScope ps(c, "recon_bin");
    // the smallest integer edge >= 2 rho, and one more (see Locality)
    lp->four_r2 = 4 * rho2[level];
    int64_t edge = int64_t(std::sqrt(double(lp->four_r2)));
    while (uint64_t(edge) * uint64_t(edge) < lp->four_r2) ++edge;
    while (edge > 1 && uint64_t(edge - 1) * uint64_t(edge - 1) >= lp->four_r2) --edge;
    edge += 1;
    unsigned long long est[4] = {0, 0, 0, 0};
    unsigned long long* d_est = d_counters + 5;
    const int64_t max_cells = std::min<int64_t>(int64_t(1) << 28, std::max<int64_t>(int64_t(1) << 22, 64 * n));
    PQ_TRY(build_grid(c, d_xyz, n, double(edge), max_cells, &lp->g, bbox, false));
    const int nc = int(lp->g.ncell);
    PQ_TRY(c->arena.get(size_t(nc) + 1, &lp->d_blk));
    if (gather) {
      hipLaunchKernelGGL(k_recon_gather, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, N,
                         static_cast<const int32_t*>(lp->g.order), static_cast<const int32_t*>(d_ijk),
                         static_cast<const int16_t*>(d_nrm), mn[0], mn[1], mn[2], d_lx, d_ly, d_lz, d_ln);
      PQ_HIP(hipGetLastError());
    }
    PQ_HIP(hipMemsetAsync(d_est, 0, 32, c->stream));
    hipLaunchKernelGGL(k_recon_plan<kReconSlice>, dim3(ceil_div(nc + 1, 256)), dim3(256), 0, c->stream, nc, lp->g.nx, lp->g.ny,
                       lp->g.nz, static_cast<const int32_t*>(lp->g.start), lp->d_blk, d_est);
    PQ_HIP(hipGetLastError());
    PQ_TRY(exclusive_scan_i32(c, lp->d_blk, int64_t(nc) + 1));
    PQ_TRY(download(c, &lp->n_blocks, lp->d_blk + nc, 1));
    PQ_TRY(download(c, est, d_est, 4));
    PQ_HIP(hipStreamSynchronize(c->stream));
    const unsigned __int128 est_all = ((unsigned __int128)est[1] << 32) + est[0];
    lp->est_tests = est_all > (unsigned __int128)INT64_MAX ? INT64_MAX : int64_t(est_all);
    lp->max_stencil = int64_t(est[2]);
    lp->max_cell = int64_t(est[3]);
    return 0;
  };
  int64_t est_sum = 0, max_stencil = 0, max_cell = 0, blocks_sum = 0;
  // the estimate of a level into the statistics, and the refusal when it exceeds the cap
  auto account = [&](int32_t level, const LevelPlan& lp) -> int {
    est_sum = lp.est_tests > INT64_MAX - est_sum ? INT64_MAX : est_sum + lp.est_tests;
    max_stencil = std::max(max_stencil, lp.max_stencil);
    max_cell = std::max(max_cell, lp.max_cell);
    if (stats) {
      stats[0] = est_sum;
      stats[5] = max_stencil;
      stats[6] = max_cell;
    }
    if (lp.est_tests > max_tests)
      return fail(PYQSM_ERANGE,
                  "pyqsm_ball_pivot: an estimated %lld pair tests at rho^2 = %llu exceed max_tests = %lld (rho spans "
                  "many point spacings: down-sample the cloud, lower the radius or raise max_tests)",
                  (long long)lp.est_tests, (unsigned long long)rho2[level], (long long)max_tests);
    return 0;
  };
  // With several radii every level is binned and estimated before the first triangle pass, so that a
  // refusal costs binning only, whichever level it is about.
  if (n_levels > 1) {
    for (int32_t level = 0; level < n_levels; ++level) {
      LevelPlan lp;
      PQ_TRY(plan_level(level, false, &lp));
      c->arena.rewind(base);
      PQ_TRY(account(level, lp));
    }
    est_sum = max_stencil = max_cell = 0;  // counted again below, level by level
  }

  const int id_bits = bit_length(uint64_t(n));
  int64_t total = 0;  // triangles so far
  int n_he = 0;
  int32_t *d_hu = nullptr, *d_hv = nullptr;
  for (int32_t level = 0; level < n_levels; ++level) {
    LevelPlan lp;
    PQ_TRY(plan_level(level, true, &lp));
    PQ_TRY(account(level, lp));
    {
      ProfScope ps(c, "recon_tris");
      if (lp.n_blocks > 0)
        hipLaunchKernelGGL(k_recon_tris, dim3(unsigned(lp.n_blocks)), dim3(256), 0, c->stream, int(lp.g.ncell),
                           static_cast<const int32_t*>(lp.d_blk), lp.g.nx, lp.g.ny,
                           static_cast<const int32_t*>(lp.g.start), static_cast<const int32_t*>(d_lx),
                           static_cast<const int32_t*>(d_ly), static_cast<const int32_t*>(d_lz),
                           static_cast<const Normal16*>(d_ln), static_cast<const int32_t*>(lp.g.order),
                           (unsigned long long)lp.four_r2, int(level),
                           static_cast<const int32_t*>(level > 0 ? d_state : nullptr), n_he,
                           static_cast<const int32_t*>(d_hu), static_cast<const int32_t*>(d_hv), (long long)tri_cap,
                           d_rows, d_counters, d_counters + 1);
      PQ_HIP(hipGetLastError());
    }
    blocks_sum += lp.n_blocks;
    unsigned long long cursor = 0;
    PQ_TRY(fetch(c, &cursor, d_counters));
    // the pass is over: its grid and the table of the levels before go back (the table is built anew
    // from all rows; until then n_he = 0 says that there is none)
    c->arena.rewind(base);
    n_he = 0;
    d_hu = d_hv = nullptr;
    if (int64_t(cursor) > tri_cap)
      return fail(PYQSM_ERANGE, "pyqsm_ball_pivot: %lld triangles, more than 8 n + 1024 = %lld",
                  (long long)cursor, (long long)tri_cap);
    total = int64_t(cursor);
    if (level + 1 == n_levels || total == 0) continue;  // d_state is all zero while there is no triangle
    // the half-edge table of everything so far, sorted by (u, v), and the state of every vertex
    ProfScope ps(c, "recon_half_edges");
    n_he = int(3 * total);
    int32_t *d_eu, *d_ev, *perm = nullptr;
    PQ_TRY(c->arena.get(size_t(n_he), &d_hu));
    PQ_TRY(c->arena.get(size_t(n_he), &d_hv));
    const Arena::Mark table = c->arena.mark();  // what follows is scratch of the sort
    PQ_TRY(c->arena.get(size_t(n_he), &d_eu));
    PQ_TRY(c->arena.get(size_t(n_he), &d_ev));
    hipLaunchKernelGGL(k_recon_half_edges, dim3(ceil_div(n_he, 256)), dim3(256), 0, c->stream, n_he,
                       static_cast<const int4*>(d_rows), d_eu, d_ev);
    PQ_HIP(hipGetLastError());
    PQ_TRY(refine_order_by_key(c, n_he, d_ev, &perm, id_bits));
    PQ_TRY(refine_order_by_key(c, n_he, d_eu, &perm, id_bits));
    hipLaunchKernelGGL(k_recon_permute2, dim3(ceil_div(n_he, 256)), dim3(256), 0, c->stream, n_he,
                       static_cast<const int32_t*>(perm), static_cast<const int32_t*>(d_eu),
                       static_cast<const int32_t*>(d_ev), d_hu, d_hv);
    PQ_HIP(hipGetLastError());
    PQ_HIP(hipMemsetAsync(d_state, 0, size_t(n) * 4, c->stream));
    hipLaunchKernelGGL(k_recon_vertex_state, dim3(ceil_div(n_he, 256)), dim3(256), 0, c->stream, n_he,
                       static_cast<const int32_t*>(d_hu), static_cast<const int32_t*>(d_hv), d_state);
    PQ_HIP(hipGetLastError());
    c->arena.rewind(table);  // the stream orders the next level's writes behind these kernels
  }
  unsigned long long host[5];
  PQ_TRY(fetch(c, host, d_counters, 5));
  if (stats) {
    stats[1] = int64_t(host[1]);
    stats[2] = int64_t(host[2]);
    stats[3] = int64_t(host[3]);
    stats[4] = int64_t(host[4]);
    stats[7] = blocks_sum;
  }
  if (total == 0) return 0;
  // ascending (a, b, c), a unique key: stable sorts by c, then b, then a
  const int e = int(total);
  int32_t *d_ka, *d_kb, *d_kc, *perm = nullptr;
  int4* d_sorted;
  PQ_TRY(c->arena.get(size_t(e), &d_ka));
  PQ_TRY(c->arena.get(size_t(e), &d_kb));
  PQ_TRY(c->arena.get(size_t(e), &d_kc));
  PQ_TRY(c->arena.get(size_t(e), &d_sorted));
  {
    ProfScope ps(c, "recon_sort");
    hipLaunchKernelGGL(k_recon_split_rows, dim3(ceil_div(e, 256)), dim3(256), 0, c->stream, e,
                       static_cast<const int4*>(d_rows), d_ka, d_kb, d_kc);
    PQ_HIP(hipGetLastError());
    PQ_TRY(refine_order_by_key(c, e, d_kc, &perm, id_bits));
    PQ_TRY(refine_order_by_key(c, e, d_kb, &perm, id_bits));
    PQ_TRY(refine_order_by_key(c, e, d_ka, &perm, id_bits));
    hipLaunchKernelGGL(k_recon_permute_rows, dim3(ceil_div(e, 256)), dim3(256), 0, c->stream, e,
                       static_cast<const int32_t*>(perm), static_cast<const int4*>(d_rows), d_sorted);
    PQ_HIP(hipGetLastError());
  }
  OutBufs out;
  int32_t* rows = out.get<int32_t>(size_t(e) * 4);
  if (!rows) return fail(PYQSM_ENOMEM, "pyqsm_ball_pivot: no host memory for %d triangles", e);
  PQ_TRY(fetch(c, reinterpret_cast<int4*>(rows), d_sorted, size_t(e)));  // (a, b, c, level) per row
  out.kept = true;
  *tris = rows;
  *n_tris = total;
  return 0;
}

}  // extern "C"
