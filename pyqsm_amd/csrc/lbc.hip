// lbc.hip — the Laplacian-contraction solve of pyQSM/geometry/skeletonize.py:148-180
// (least_squares_sparse) on gfx950, plus the per-point clamp of :291-296.
//
// The reference stacks A = [L*W_L ; W_H], forms A'A and factorises it three
// times with SuperLU (once per coordinate). Here the normal equations
//     (W_L L' L W_L + W_H^2) x = W_H^2 p
// are solved matrix-free; the three coordinates ride every sparse pass together (one
// read of L serves x, y and z). L'L is never formed. L must be symmetric (it is: the
// point-cloud Laplacian is), so L' x is computed as L x.
//
// Uniform W_L = c I (what extract_skeleton always passes): flexible CG on A preconditioned
// by B^-2, B = c L + W_H — with Riccati-corrected weights while W_H is rough, in two phases
// (k_riccati_f) — each B-solve a CG preconditioned by one aggregation-multigrid cycle
// (amg.hip), on spatially sorted unknowns — see lbc_solve_core / lbc_solve_device below and
// DESIGN.md section 6. Per-point W_L: Jacobi-preconditioned CG on A.
//
// HBM traffic of one sparse pass (fp64, CSR with 32-bit indices): 12*nnz + 52*n bytes
// (SURVEY.md §8 d-roofline); the scalars of the inner CGs (alpha, beta, dot products) stay
// on the device as per-block partial sums that are added up in a fixed order (sparse.hpp: no
// floating-point atomics, the same bits on every run), and the host looks at a residual only
// between bursts of iterations.
#include "grid.hpp"
#include "sparse.hpp"

namespace pyqsm {

static constexpr int kBurst = 24;  // CG iterations per graph replay / residual check
static constexpr double kInnerRtolDefault = 3e-2;  // B-solves inside the preconditioner (flexible CG outside); round 3: 1e-2 -> 3e-2
static constexpr int kInnerMaxIt = 200000;
static constexpr int kOuterMaxIt = 600;
static constexpr int kOuterStall = 12;
static constexpr int kAmgMaxIt = 400;   // multigrid-preconditioned CG iterations per B-solve
static constexpr int kF32MaxIt = 96;    // ... per fp32 B-solve: one that needs more has lost its digits (fp64 then)
static constexpr int kRiccatiMaxIt = 8;            // Newton steps on the preconditioner's weights
static constexpr double kRiccatiTol = 2e-3;        // |F| / |w^2| at which they are good enough (1e-2: the
                                                   // hardest contraction takes twice the outer steps)
// The Riccati weights are worth their Newton solves only while W_H is rough: the measure is the
// fraction of points at which the potential c (L w)_i of B^2 cancels more than half of w_i^2
// (1 M-point forest, c = 3: 0.53, 0.40, 0.29, 0.13, 0.03, < 0.005 ... over the contractions, with
// 57, 76, 34, 19, 14, 13 ... outer steps of the plain preconditioner; c = 7: 0.52, 0.35, 0.10, 0.01)
static constexpr double kRiccatiFrac = 0.2;
static constexpr int kRiccatiStall = 3;            // phase-1 steps without a better estimate before phase 2
static constexpr double kRiccatiInnerRtol = 1e-2;  // the Newton systems, like every B-solve
static constexpr int kRiccatiInnerMaxIt = 100;
static constexpr int kStallIters = 1500;
// CG residuals are not monotone, so stagnation only counts once the solve is
// close to its attainable accuracy
static constexpr double kStallBelow = 1e-8;

static constexpr int kRowChunk = 4;

// y = L (s .* x)   three columns; one lane per row (rows hold ~7 entries).
__global__ __launch_bounds__(256) void k_spmv3(int n, const int32_t* __restrict__ indptr,
                                               const int32_t* __restrict__ indices,
                                               const double* __restrict__ vals,
                                               const double* __restrict__ s /*may be null*/,
                                               const double* __restrict__ x,
                                               double* __restrict__ y) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  const int b = indptr[i], e = indptr[i + 1];
  // four entries at a time, their loads issued side by side (amg.hip: kRowUnroll); entries
  // past the row's end read the row itself with weight 0
  for (int j = b; j < e; j += kRowChunk) {
    int col[kRowChunk];
    double v[kRowChunk], x0[kRowChunk], x1[kRowChunk], x2[kRowChunk];
#pragma unroll
    for (int u = 0; u < kRowChunk; ++u) {
      const bool ok = j + u < e;
      col[u] = ok ? indices[j + u] : i;
      v[u] = ok ? vals[j + u] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kRowChunk; ++u) {
      if (s) v[u] *= s[col[u]];
      x0[u] = x[3 * col[u]];
      x1[u] = x[3 * col[u] + 1];
      x2[u] = x[3 * col[u] + 2];
    }
#pragma unroll
    for (int u = 0; u < kRowChunk; ++u) {
      a0 += v[u] * x0[u];
      a1 += v[u] * x1[u];
      a2 += v[u] * x2[u];
    }
  }
  y[3 * i] = a0;
  y[3 * i + 1] = a1;
  y[3 * i + 2] = a2;
}

// diag(A)_i = wl_i^2 * sum_j L_ji^2 + wh_i^2 ; symmetric L: column norm = row norm
__global__ __launch_bounds__(256) void k_diag(int n, const int32_t* __restrict__ indptr,
                                              const double* __restrict__ vals,
                                              const double* __restrict__ wl,
                                              const double* __restrict__ wh,
                                              double* __restrict__ minv) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int j = indptr[i]; j < indptr[i + 1]; ++j) s += vals[j] * vals[j];
  const double d = wl[i] * wl[i] * s + wh[i] * wh[i];
  minv[i] = d > 0.0 ? 1.0 / d : 1.0;
}

// Scalars of the fused CG loops, kept on the device as partial arrays (sparse.hpp:
// reduce3_part / part_total3 — no atomics, reproducible bits). Two slots alternate with the
// iteration parity p: rz[p] is the current r.z, rz[p^1] receives the next one; a producer
// overwrites its array completely, so an iteration is four launches with no bookkeeping kernel.
struct Scal {
  double rz[2][3 * kPart], pq[2][3 * kPart], rr[2][3 * kPart], bb[3 * kPart];
  // fp32 loop only: the totals of rz[p], stored by the first kernel that adds them up (block 0)
  // for the two later kernels that need them again
  double rz_tot[2][4];
};

enum Op { OP_A = 0, OP_B = 1 };  // A = wl L L wl + wh^2 ; B = wl L + wh (wl constant along the edges of L)

// r = b - q (q = Op(x0), or absent when x0 = 0); z = Minv r; dir = z; rz, rr, bb.
__global__ __launch_bounds__(256) void k_init(int n, const double* __restrict__ q /*may be null*/,
                                              const double* __restrict__ b,
                                              const double* __restrict__ minv,
                                              double* __restrict__ r, double* __restrict__ dir,
                                              Scal* __restrict__ sc) {
  double rz[3] = {0, 0, 0}, rr[3] = {0, 0, 0}, bb[3] = {0, 0, 0};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {  // reduce_grid
    const double mi = minv[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double bi = b[3 * i + k];
      const double ri = q ? bi - q[3 * i + k] : bi;
      const double zi = mi * ri;
      r[3 * i + k] = ri;
      dir[3 * i + k] = zi;
      rz[k] += ri * zi;
      rr[k] += ri * ri;
      bb[k] += bi * bi;
    }
  }
  reduce3_part(rz[0], rz[1], rz[2], sc->rz[0]);
  __syncthreads();
  reduce3_part(rr[0], rr[1], rr[2], sc->rr[1]);
  __syncthreads();
  reduce3_part(bb[0], bb[1], bb[2], sc->bb);
}

// Sparse pass fused with the operator tail: t = L v for row i, then
//   OP_A: q_i = wl_i * t + wh_i^2 * v_i    (v here is L(wl .* dir), `dirv` the CG direction)
//   OP_B: q_i = wl_i * t + wh_i * v_i
// and pq += dirv_i * q_i. Saves one launch and one 3-column stream per iteration.
template <int OP>
__global__ __launch_bounds__(256) void k_spmv3_tail(int n, const int32_t* __restrict__ indptr,
                                                    const int32_t* __restrict__ indices,
                                                    const double* __restrict__ vals,
                                                    const double* __restrict__ x /*gathered*/,
                                                    const double* __restrict__ wl,
                                                    const double* __restrict__ wh,
                                                    const double* __restrict__ dirv,
                                                    double* __restrict__ q, Scal* __restrict__ sc,
                                                    int par) {
  double pq[3] = {0, 0, 0};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {  // reduce_grid when sc
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    const int b = indptr[i], e = indptr[i + 1];
    for (int j = b; j < e; j += kRowChunk) {
      int col[kRowChunk];
      double v[kRowChunk], x0[kRowChunk], x1[kRowChunk], x2[kRowChunk];
#pragma unroll
      for (int u = 0; u < kRowChunk; ++u) {
        const bool ok = j + u < e;
        col[u] = ok ? indices[j + u] : i;
        v[u] = ok ? vals[j + u] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kRowChunk; ++u) {
        x0[u] = x[3 * col[u]];
        x1[u] = x[3 * col[u] + 1];
        x2[u] = x[3 * col[u] + 2];
      }
#pragma unroll
      for (int u = 0; u < kRowChunk; ++u) {
        a0 += v[u] * x0[u];
        a1 += v[u] * x1[u];
        a2 += v[u] * x2[u];
      }
    }
    const double a = wl[i];
    const double h = OP == OP_A ? wh[i] * wh[i] : wh[i];
    const double t[3] = {a0, a1, a2};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double d = dirv[3 * i + k];
      const double qi = a * t[k] + h * d;
      q[3 * i + k] = qi;
      pq[k] += d * qi;
    }
  }
  if (sc) reduce3_part(pq[0], pq[1], pq[2], sc->pq[par]);
}

// alpha = rz/pq ; x += alpha dir ; r -= alpha q ; z = Minv r ; rz_new += r.z ; rr += r.r
__global__ __launch_bounds__(256) void k_update(int n, const double* __restrict__ dir,
                                                const double* __restrict__ q,
                                                const double* __restrict__ minv,
                                                double* __restrict__ x, double* __restrict__ r,
                                                double* __restrict__ z, Scal* __restrict__ sc,
                                                int par) {
  double rz[3] = {0, 0, 0}, rr[3] = {0, 0, 0}, pqt[3], rzt[3], alpha[3];
  part_total3(sc->pq[par], pqt);
  part_total3(sc->rz[par], rzt);
#pragma unroll
  for (int k = 0; k < 3; ++k) alpha[k] = pqt[k] != 0.0 ? rzt[k] / pqt[k] : 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {  // reduce_grid
    const double mi = minv[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      x[3 * i + k] += alpha[k] * dir[3 * i + k];
      const double ri = r[3 * i + k] - alpha[k] * q[3 * i + k];
      const double zi = mi * ri;
      r[3 * i + k] = ri;
      z[3 * i + k] = zi;
      rz[k] += ri * zi;
      rr[k] += ri * ri;
    }
  }
  __syncthreads();
  reduce3_part(rz[0], rz[1], rz[2], sc->rz[par ^ 1]);
  __syncthreads();
  reduce3_part(rr[0], rr[1], rr[2], sc->rr[par]);
}

// beta = rz_new/rz ; dir = z + beta dir
__global__ __launch_bounds__(256) void k_direction(int n, const double* __restrict__ z,
                                                   double* __restrict__ dir,
                                                   Scal* __restrict__ sc, int par) {
  int i = blockIdx.x * 256 + threadIdx.x;
  double rzo[3], rzn[3];
  part_total3(sc->rz[par], rzo);
  part_total3(sc->rz[par ^ 1], rzn);
  if (i >= n) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double beta = rzo[k] != 0.0 ? rzn[k] / rzo[k] : 0.0;
    dir[3 * i + k] = z[3 * i + k] + beta * dir[3 * i + k];
  }
}

// 1 / diag(B),  B = wl L + wh
__global__ __launch_bounds__(256) void k_diag_b(int n, const int32_t* __restrict__ indptr,
                                                const int32_t* __restrict__ indices,
                                                const double* __restrict__ vals,
                                                const double* __restrict__ wl,
                                                const double* __restrict__ wh,
                                                double* __restrict__ minv) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double lii = 0.0;
  for (int j = indptr[i]; j < indptr[i + 1]; ++j)
    if (indices[j] == i) lii += vals[j];
  const double d = wl[i] * lii + wh[i];
  minv[i] = d > 0.0 ? 1.0 / d : 1.0;
}

// ---- small vector kernels of the outer iteration (scalars come from the host) -------

struct S3 {
  double v[3];
};

__global__ __launch_bounds__(256) void k_dot3(int n, const double* __restrict__ a,
                                              const double* __restrict__ b,
                                              double* __restrict__ out /*[3][kPart]*/) {
  double d[3] = {0, 0, 0};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {  // reduce_grid
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] += a[3 * i + k] * b[3 * i + k];
  }
  reduce3_part(d[0], d[1], d[2], out);
}

// y += s .* x (per column)
__global__ __launch_bounds__(256) void k_axpy3(int n, S3 s, const double* __restrict__ x,
                                               double* __restrict__ y) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) y[3 * i + k] += s.v[k] * x[3 * i + k];
}

// y = x + s .* y (per column)
__global__ __launch_bounds__(256) void k_xpay3(int n, S3 s, const double* __restrict__ x,
                                               double* __restrict__ y) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) y[3 * i + k] = x[3 * i + k] + s.v[k] * y[3 * i + k];
}

// b = wh^2 .* p
__global__ __launch_bounds__(256) void k_rhs(int n, const double* __restrict__ wh,
                                             const double* __restrict__ p,
                                             double* __restrict__ b) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double h2 = wh[i] * wh[i];
#pragma unroll
  for (int k = 0; k < 3; ++k) b[3 * i + k] = h2 * p[3 * i + k];
}

__global__ __launch_bounds__(256) void k_sub3(int n, const double* __restrict__ a,
                                              const double* __restrict__ b,
                                              double* __restrict__ out) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) out[3 * i + k] = a[3 * i + k] - b[3 * i + k];
}

__global__ __launch_bounds__(256) void k_clamp(int64_t n3, double* __restrict__ pts, double lo0,
                                               double lo1, double lo2, double hi0, double hi1,
                                               double hi2) {
  int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (i >= n3) return;
  const int a = int(i % 3);
  const double lo = a == 0 ? lo0 : (a == 1 ? lo1 : lo2);
  const double hi = a == 0 ? hi0 : (a == 1 ? hi1 : hi2);
  double v = pts[i];
  // skeletonize.py:293-296: if v < lo: v = lo ; if v > hi: v = hi  (NaN stays NaN)
  if (v < lo) v = lo;
  if (v > hi) v = hi;
  pts[i] = v;
}

static int upload_csr(Ctx* c, const int32_t* indptr, const int32_t* indices, const double* vals,
                      int64_t n, DevCsr* d, int64_t* nnz_out) {
  if (n > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 rows");
  const int64_t nnz = indptr[n];
  if (nnz < 0 || indptr[0] != 0) return fail(PYQSM_EINVAL, "malformed CSR indptr");
  PQ_TRY(c->arena.get(size_t(n) + 1, &d->indptr));
  PQ_TRY(c->arena.get(size_t(nnz) + 1, &d->indices));
  PQ_TRY(c->arena.get(size_t(nnz) + 1, &d->vals));
  PQ_TRY(copy_in(c, d->indptr, indptr, size_t(n) + 1));
  if (nnz) {
    PQ_TRY(copy_in(c, d->indices, indices, size_t(nnz)));
    PQ_TRY(copy_in(c, d->vals, vals, size_t(nnz)));
  }
  *nnz_out = nnz;
  return 0;
}

// The operator and the vectors one Jacobi-PCG run works on.
struct System {
  DevCsr L;
  int n;
  Op op;
  const double* wl;  // per-point Laplacian weights (OP_B: constant along every edge of L)
  const double* wh;
  const double* minv;
};

struct Work {  // scratch of one Jacobi-PCG level
  double *t1, *t2, *r, *z, *dir, *q, *x_best;
  Scal* sc;
};

static int alloc_work(Ctx* c, int64_t n, Work* w) {
  PQ_TRY(c->arena.get(size_t(n) * 3, &w->t1));
  PQ_TRY(c->arena.get(size_t(n) * 3, &w->t2));
  PQ_TRY(c->arena.get(size_t(n) * 3, &w->r));
  PQ_TRY(c->arena.get(size_t(n) * 3, &w->z));
  PQ_TRY(c->arena.get(size_t(n) * 3, &w->dir));
  PQ_TRY(c->arena.get(size_t(n) * 3, &w->q));
  PQ_TRY(c->arena.get(size_t(n) * 3, &w->x_best));
  PQ_TRY(c->arena.get(1, &w->sc));
  return 0;
}

// q = Op(v) (+ pq accumulation when sc != null)
static void apply_op(Ctx* c, const System& S, const Work& w, const double* v, double* q,
                     Scal* sc, int par = 0) {
  const dim3 grid(ceil_div(S.n, 256)), block(256);
  const dim3 tgrid = sc ? dim3(reduce_grid(S.n)) : grid;
  if (S.op == OP_A) {
    hipLaunchKernelGGL(k_spmv3, grid, block, 0, c->stream, S.n, S.L.indptr, S.L.indices, S.L.vals,
                       S.wl, v, w.t1);
    hipLaunchKernelGGL(k_spmv3_tail<OP_A>, tgrid, block, 0, c->stream, S.n, S.L.indptr, S.L.indices,
                       S.L.vals, w.t1, S.wl, S.wh, v, q, sc, par);
  } else {
    hipLaunchKernelGGL(k_spmv3_tail<OP_B>, tgrid, block, 0, c->stream, S.n, S.L.indptr, S.L.indices,
                       S.L.vals, v, S.wl, S.wh, v, q, sc, par);
  }
}

// Plain launches instead of graph replays when PYQSM_NO_GRAPH is set. The library never looks
// at the profiler's environment, and the profile scripts (tools/profile_r0*.sh) keep graphs ON:
// what they measure is the shipped path. PYQSM_NO_GRAPH=1 is an explicit switch for whoever
// wants a profile of plain launches.
static bool graphs_enabled() { return !getenv("PYQSM_NO_GRAPH"); }

// The multigrid-CG bursts are plain launches unless PYQSM_AMG_GRAPH is set: their graphs hold
// 30-150 kernel nodes, are instantiated anew for every B-solve pair and replayed ~5 times, and
// measured against plain launches they lose at every size on this ROCm (20 contractions:
// 1 M points 5.28 vs 5.07 s, 50 k 0.82 vs 0.77 s, 5 k 0.61 vs 0.55 s). They paid off for
// the round's first solver — 24-iteration bursts of four tiny kernels — which keeps them.
static bool amg_graphs_enabled() { return getenv("PYQSM_AMG_GRAPH") && graphs_enabled(); }

// A burst of kBurst CG iterations recorded once as a hipGraph and replayed: at a
// few thousand points an iteration is four ~5 us launches, and replaying a graph
// costs about a third of launching them one by one.
struct BurstGraph {
  const void *b, *x;
  int op;
  hipGraphExec_t exec;
};
struct GraphCache {
  std::vector<BurstGraph> items;
  ~GraphCache() {
    for (auto& g : items) (void)hipGraphExecDestroy(g.exec);
  }
};

static void launch_iteration(Ctx* c, const System& S, const Work& w, double* x, int par) {
  const dim3 grid(ceil_div(S.n, 256)), block(256);
  apply_op(c, S, w, w.dir, w.q, w.sc, par);
  hipLaunchKernelGGL(k_update, dim3(reduce_grid(S.n)), block, 0, c->stream, S.n, w.dir, w.q, S.minv, x,
                     w.r, w.z, w.sc, par);
  hipLaunchKernelGGL(k_direction, grid, block, 0, c->stream, S.n, w.z, w.dir, w.sc, par);
}

// Jacobi-preconditioned CG on Op x = b for three columns. x holds the start
// vector (zero_start: it is taken as 0 and overwritten). Scalars stay on the
// device; the host reads the residual once per burst. Returns 0 when
// |r|/|b| <= rtol for all columns, PYQSM_ENOCONV otherwise (best iterate in x).
static int jacobi_pcg(Ctx* c, const System& S, const Work& w, const double* b, double* x,
                      bool zero_start, double rtol, int32_t max_it, const char* prof_name,
                      GraphCache* cache, int32_t* iters, double resid[3]) {
  const int64_t n = S.n;
  const dim3 grid(ceil_div(n, 256)), block(256);
  PQ_HIP(hipMemsetAsync(w.sc, 0, sizeof(Scal), c->stream));
  if (zero_start) {
    PQ_HIP(hipMemsetAsync(x, 0, size_t(n) * 24, c->stream));
    hipLaunchKernelGGL(k_init, dim3(reduce_grid(n)), block, 0, c->stream, S.n,
                       static_cast<const double*>(nullptr), b, S.minv, w.r, w.dir, w.sc);
  } else {
    apply_op(c, S, w, x, w.q, nullptr);
    hipLaunchKernelGGL(k_init, dim3(reduce_grid(n)), block, 0, c->stream, S.n, w.q, b, S.minv, w.r,
                       w.dir, w.sc);
  }
  PQ_HIP(hipGetLastError());
  double h0[2][3];  // |r|^2, |b|^2
  {
    const double* parts[2] = {w.sc->rr[1], w.sc->bb};
    PQ_TRY(part_totals_host(c, parts, 2, h0));
  }
  double bnorm[3];
  bool done = true;
  for (int k = 0; k < 3; ++k) {
    bnorm[k] = std::sqrt(h0[1][k]);
    resid[k] = bnorm[k] > 0 ? std::sqrt(h0[0][k]) / bnorm[k] : 0.0;
    if (resid[k] > rtol) done = false;
  }
  // Past the attainable accuracy (about cond * 1e-16) the recurrences drift and
  // the residual grows again, so the best iterate is kept and the loop stops once
  // a nearly converged residual has not improved for kStallIters iterations.
  PQ_HIP(hipMemcpyAsync(w.x_best, x, size_t(n) * 24, hipMemcpyDeviceToDevice, c->stream));
  double best = std::max(resid[0], std::max(resid[1], resid[2]));
  double best_res[3] = {resid[0], resid[1], resid[2]};
  int it = 0, best_it = 0;
  bool broke = false;
  hipGraphExec_t exec = nullptr;
  if (!graphs_enabled()) cache = nullptr;
  while (!done && it < max_it) {
    // bursts have an even length so that each one starts at parity 0
    int burst = std::min<int>(kBurst, max_it - it);
    if (burst < kBurst) burst += burst & 1;
    {
      ProfScope ps(c, prof_name, burst);
      if (burst == kBurst && cache) {
        if (!exec) {
          for (auto& g : cache->items)
            if (g.b == b && g.x == x && g.op == int(S.op)) exec = g.exec;
        }
        if (!exec) {
          hipGraph_t graph = nullptr;
          PQ_HIP(hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed));
          for (int bi = 0; bi < burst; ++bi) launch_iteration(c, S, w, x, bi & 1);
          PQ_HIP(hipStreamEndCapture(c->stream, &graph));
          PQ_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
          (void)hipGraphDestroy(graph);
          cache->items.push_back({b, x, int(S.op), exec});
        }
        PQ_HIP(hipGraphLaunch(exec, c->stream));
      } else {
        for (int bi = 0; bi < burst; ++bi) launch_iteration(c, S, w, x, bi & 1);
        PQ_HIP(hipGetLastError());
      }
    }
    it += burst;
    double rr[3];
    {
      const double* parts[1] = {w.sc->rr[1]};
      PQ_TRY(part_totals_host(c, parts, 1, &rr));
    }
    done = true;
    double worst = 0.0;
    for (int k = 0; k < 3; ++k) {
      resid[k] = bnorm[k] > 0 ? std::sqrt(rr[k]) / bnorm[k] : 0.0;
      if (!(resid[k] <= rtol)) done = false;
      if (!std::isfinite(resid[k])) broke = true;
      worst = std::max(worst, resid[k]);
    }
    if (broke) break;
    if (worst < best) {
      best = worst;
      best_it = it;
      for (int k = 0; k < 3; ++k) best_res[k] = resid[k];
      PQ_HIP(hipMemcpyAsync(w.x_best, x, size_t(n) * 24, hipMemcpyDeviceToDevice, c->stream));
    } else if (best < kStallBelow && it - best_it >= kStallIters) {
      break;  // converged as far as fp64 allows; the recurrences are drifting now
    }
  }
  *iters = it;
  if (!done) {
    PQ_HIP(hipMemcpyAsync(x, w.x_best, size_t(n) * 24, hipMemcpyDeviceToDevice, c->stream));
    for (int k = 0; k < 3; ++k) resid[k] = best_res[k];
    return fail(PYQSM_ENOCONV, "CG stopped after %d iterations (%s); best residual %.3e at %d", it,
                broke ? "breakdown" : (it >= max_it ? "max_it" : "stagnation"), best, best_it);
  }
  return 0;
}

// d_tmp: a partial array [3][kPart]
static int dot3_host(Ctx* c, int n, const double* a, const double* b, double* d_tmp,
                     double out[3]) {
  hipLaunchKernelGGL(k_dot3, dim3(reduce_grid(n)), dim3(256), 0, c->stream, n, a, b, d_tmp);
  PQ_HIP(hipGetLastError());
  const double* parts[1] = {d_tmp};
  double t[1][3];
  PQ_TRY(part_totals_host(c, parts, 1, t));
  for (int k = 0; k < 3; ++k) out[k] = t[0][k];
  return 0;
}

int part_totals_host(Ctx* c, const double* const* parts, int m, double (*out)[3]) {
  std::vector<double> h(size_t(m) * 3 * kPart);
  for (int a = 0; a < m; ++a)
    PQ_TRY(download(c, h.data() + size_t(a) * 3 * kPart, parts[a], kPart * 3));
  PQ_HIP(hipStreamSynchronize(c->stream));
  for (int a = 0; a < m; ++a)
    for (int k = 0; k < 3; ++k) {
      const double* p = h.data() + (size_t(a) * 3 + size_t(k)) * kPart;
      double s[4] = {0, 0, 0, 0};  // four interleaved chains, then pairwise: fixed order
      for (int i = 0; i < kPart; i += 4) {
        s[0] += p[i];
        s[1] += p[i + 1];
        s[2] += p[i + 2];
        s[3] += p[i + 3];
      }
      out[a][k] = (s[0] + s[1]) + (s[2] + s[3]);
    }
  return 0;
}


// alpha = rz/pq ; x += alpha dir ; r -= alpha q ; rr += r.r   (the multigrid cycle follows)
__global__ __launch_bounds__(256) void k_update_r(int n, const double* __restrict__ dir,
                                                  const double* __restrict__ q,
                                                  double* __restrict__ x, double* __restrict__ r,
                                                  Scal* __restrict__ sc, int par) {
  double rr[3] = {0, 0, 0}, pqt[3], rzt[3], alpha[3];
  part_total3(sc->pq[par], pqt);
  part_total3(sc->rz[par], rzt);
#pragma unroll
  for (int k = 0; k < 3; ++k) alpha[k] = pqt[k] != 0.0 ? rzt[k] / pqt[k] : 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {  // reduce_grid
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      x[3 * i + k] += alpha[k] * dir[3 * i + k];
      const double ri = r[3 * i + k] - alpha[k] * q[3 * i + k];
      r[3 * i + k] = ri;
      rr[k] += ri * ri;
    }
  }
  __syncthreads();
  reduce3_part(rr[0], rr[1], rr[2], sc->rr[par]);
}

// PYQSM_AMG_FIXED=m: every B-solve runs exactly m multigrid-CG iterations (experiment knob)
static int amg_fixed_iterations() {
  static const int v = [] {
    const char* e = getenv("PYQSM_AMG_FIXED");
    return e ? std::max(0, atoi(e)) : 0;
  }();
  return v;
}

static constexpr int kAmgFirstBurst = 8;  // a 1e-2 solve takes 10-14 iterations: no look before 8
static constexpr int kAmgBurst = 2;       // then a residual check every 2
static int amg_next_burst() {  // PYQSM_AMG_BURST: iterations between two looks after the first (even, 2-16)
  static const int v = [] {
    const char* e = getenv("PYQSM_AMG_BURST");
    const int b = e ? atoi(e) : kAmgBurst;
    return b >= 2 && b <= 16 ? (b & ~1) : kAmgBurst;
  }();
  return v;
}
static int amg_first_burst() {
  static const int v = [] {
    const char* e = getenv("PYQSM_AMG_FIRST_BURST");
    const int b = e ? atoi(e) : kAmgFirstBurst;
    return b >= 2 && b <= 64 ? (b & ~1) : kAmgFirstBurst;
  }();
  return v;
}

// CG on B y = rhs preconditioned by one multigrid V-cycle (amg.hip). Same device-side
// scalar protocol as jacobi_pcg: an iteration is the sparse pass, the update, the cycle
// (its last kernel also accumulates r.z) and the direction update, replayed as graphs of 8
// and then 2 iterations; the host only reads |b|^2 and |r|^2 between replays (each look
// costs a stream drain, which is what small systems are bound by). y starts at 0.
static int amg_pcg(Ctx* c, const System& S, const Work& w, AmgHierarchy* H, const double* rhs,
                   double* y, double rtol, int32_t max_it, GraphCache* cache, int32_t* iters,
                   double resid[3]) {
  const int N = S.n;
  const dim3 grid(ceil_div(N, 256)), block(256);
  PQ_HIP(hipMemsetAsync(w.sc, 0, sizeof(Scal), c->stream));
  PQ_HIP(hipMemsetAsync(y, 0, size_t(N) * 24, c->stream));
  PQ_HIP(hipMemcpyAsync(w.r, rhs, size_t(N) * 24, hipMemcpyDeviceToDevice, c->stream));
  const dim3 rgrid(reduce_grid(N));
  hipLaunchKernelGGL(k_dot3, rgrid, block, 0, c->stream, N, rhs, rhs, w.sc->bb);
  PQ_TRY(amg_vcycle(c, H, w.r, w.z, w.sc->rz[0]));
  PQ_HIP(hipMemcpyAsync(w.dir, w.z, size_t(N) * 24, hipMemcpyDeviceToDevice, c->stream));
  for (int k = 0; k < 3; ++k) resid[k] = 1.0;
  *iters = 0;
  auto iteration = [&](int par) -> int {
    hipLaunchKernelGGL(k_spmv3_tail<OP_B>, rgrid, block, 0, c->stream, N, S.L.indptr, S.L.indices,
                       S.L.vals, w.dir, S.wl, S.wh, w.dir, w.q,
                       w.sc, par);
    hipLaunchKernelGGL(k_update_r, rgrid, block, 0, c->stream, N, w.dir, w.q, y, w.r, w.sc, par);
    PQ_TRY(amg_vcycle(c, H, w.r, w.z, w.sc->rz[par ^ 1]));
    hipLaunchKernelGGL(k_direction, grid, block, 0, c->stream, N, w.z, w.dir, w.sc, par);
    return 0;
  };
  if (!amg_graphs_enabled()) cache = nullptr;
  // graphs are keyed by (hierarchy, target vector, burst length)
  auto run_burst = [&](int len) -> int {
    hipGraphExec_t exec = nullptr;
    if (cache)
      for (auto& g : cache->items)
        if (g.b == static_cast<const void*>(H) && g.x == y && g.op == 100 + len) exec = g.exec;
    if (cache && !exec) {
      hipGraph_t graph = nullptr;
      PQ_HIP(hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed));
      int rc = 0;
      for (int bi = 0; bi < len && rc == 0; ++bi) rc = iteration(bi & 1);
      PQ_HIP(hipStreamEndCapture(c->stream, &graph));
      if (rc != 0) return rc;
      PQ_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
      (void)hipGraphDestroy(graph);
      cache->items.push_back({static_cast<const void*>(H), y, 100 + len, exec});
    }
    if (exec) {
      PQ_HIP(hipGraphLaunch(exec, c->stream));
    } else {
      for (int bi = 0; bi < len; ++bi) PQ_TRY(iteration(bi & 1));
    }
    return 0;
  };
  int it = 0;
  bool done = false;
  while (!done && it < max_it) {
    int len = it == 0 ? amg_first_burst() : amg_next_burst();
    if (len > max_it - it) len = std::max(2, (max_it - it + 1) & ~1);  // even: bursts start at parity 0
    {
      ProfScope ps(c, "lbc_amg_iter", len);
      PQ_TRY(run_burst(len));
    }
    it += len;
    double h[2][3];
    {
      const double* parts[2] = {w.sc->rr[1], w.sc->bb};
      PQ_TRY(part_totals_host(c, parts, 2, h));
    }
    const double* rr = h[0];
    const double* bb = h[1];
    if (bb[0] == 0.0 && bb[1] == 0.0 && bb[2] == 0.0) {  // zero right-hand side: y = 0
      for (int k = 0; k < 3; ++k) resid[k] = 0.0;
      *iters = it;
      return 0;
    }
    done = true;
    for (int k = 0; k < 3; ++k) {
      resid[k] = bb[k] > 0 ? std::sqrt(rr[k] / bb[k]) : 0.0;
      if (!(resid[k] <= rtol)) done = false;
      if (!std::isfinite(resid[k])) {
        *iters = it;
        return fail(PYQSM_ENOCONV, "multigrid CG broke down after %d iterations", it);
      }
    }
  }
  PQ_HIP(hipGetLastError());
  *iters = it;
  return done ? 0 : fail(PYQSM_ENOCONV, "multigrid CG reached %d iterations, residual %.3e", it,
                         std::max(resid[0], std::max(resid[1], resid[2])));
}

// ---- the same CG in fp32 ------------------------------------------------------------------
// The B-solves are asked for two digits and sit inside a flexible outer CG, so they run in
// fp32 altogether: B as the multigrid's fp32 level-0 matrix, float vectors, the cycle without
// its conversion pass; dot products are still accumulated in fp64. Half the bytes per sparse
// pass and vector update.
// PYQSM_REDUCE_BLOCKS: grid cap of the reducing kernels of this loop below kPart (tuning knob)
static unsigned reduce_grid_f(int64_t n) {
  static const int cap = [] {
    const char* e = getenv("PYQSM_REDUCE_BLOCKS");
    const int v = e ? atoi(e) : 0;
    return v > 0 ? std::min(v, kPart) : kPart;
  }();
  return std::min<unsigned>(reduce_grid(n), unsigned(cap));
}

struct WorkF {
  float *r, *z, *dir, *q;
  Scal* sc;
};

__device__ __forceinline__ float4 ld4(const float* v, int i) {
  return reinterpret_cast<const float4*>(v)[i];
}
__device__ __forceinline__ void st4(float* v, int i, float a, float b, float c) {
  reinterpret_cast<float4*>(v)[i] = make_float4(a, b, c, 0.f);
}

static constexpr int kU = 8;

__global__ __launch_bounds__(256) void k_bspmv_f(int n, const int32_t* __restrict__ indptr,
                                                 const int32_t* __restrict__ indices,
                                                 const float* __restrict__ vals,
                                                 const float* __restrict__ p, float* __restrict__ q,
                                                 Scal* __restrict__ sc, int par) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  double pq[3] = {0, 0, 0};
  for (int i = gid; i < n; i += gridDim.x * 256) {  // reduce_grid
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    const int e = indptr[i + 1];
    for (int j = indptr[i]; j < e; j += kU) {  // kU entries' loads side by side (amg.hip: kRowUnroll)
      int col[kU];
      float v[kU];
      float4 pc[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const bool ok = j + u < e;
        col[u] = ok ? indices[j + u] : i;
        v[u] = ok ? vals[j + u] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) pc[u] = ld4(p, col[u]);
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        a0 += v[u] * pc[u].x;
        a1 += v[u] * pc[u].y;
        a2 += v[u] * pc[u].z;
      }
    }
    st4(q, i, a0, a1, a2);
    const float4 pi = ld4(p, i);
    pq[0] += double(pi.x) * a0;
    pq[1] += double(pi.y) * a1;
    pq[2] += double(pi.z) * a2;
  }
  reduce3_part(pq[0], pq[1], pq[2], sc->pq[par]);
}

__global__ __launch_bounds__(256) void k_update_r_f(int n, const float* __restrict__ dir,
                                                    const float* __restrict__ q,
                                                    float* __restrict__ x, float* __restrict__ r,
                                                    Scal* __restrict__ sc, int par) {
  double rr[3] = {0, 0, 0}, pqt[3];
  float alpha[3];
  part_total3(sc->pq[par], pqt);
#pragma unroll
  for (int k = 0; k < 3; ++k) alpha[k] = float(pqt[k] != 0.0 ? sc->rz_tot[par][k] / pqt[k] : 0.0);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float4 d = ld4(dir, i), qi = ld4(q, i), xi = ld4(x, i), ri = ld4(r, i);
    st4(x, i, xi.x + alpha[0] * d.x, xi.y + alpha[1] * d.y, xi.z + alpha[2] * d.z);
    const float r0 = ri.x - alpha[0] * qi.x, r1 = ri.y - alpha[1] * qi.y, r2 = ri.z - alpha[2] * qi.z;
    st4(r, i, r0, r1, r2);
    rr[0] += double(r0) * r0;
    rr[1] += double(r1) * r1;
    rr[2] += double(r2) * r2;
  }
  __syncthreads();
  reduce3_part(rr[0], rr[1], rr[2], sc->rr[par]);
}

__global__ __launch_bounds__(256) void k_direction_f(int n, const float* __restrict__ z,
                                                     float* __restrict__ dir, Scal* __restrict__ sc,
                                                     int par) {
  double rzn[3];
  part_total3(sc->rz[par ^ 1], rzn);  // the cycle's r.z: first use, kept for the next iteration
  float beta[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double rzo = sc->rz_tot[par][k];
    beta[k] = float(rzo != 0.0 ? rzn[k] / rzo : 0.0);
  }
  if (blockIdx.x == 0 && threadIdx.x < 3) sc->rz_tot[par ^ 1][threadIdx.x] = rzn[threadIdx.x];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {  // reduce_grid
    const float4 zi = ld4(z, i), d = ld4(dir, i);
    st4(dir, i, zi.x + beta[0] * d.x, zi.y + beta[1] * d.y, zi.z + beta[2] * d.z);
  }
}

// totals of a partial array into tot[0..2] (one block; the start of a solve)
__global__ __launch_bounds__(256) void k_part_final(const double* __restrict__ part,
                                                    double* __restrict__ tot) {
  double t[3];
  part_total3(part, t);
  if (threadIdx.x < 3) tot[threadIdx.x] = t[threadIdx.x];
}

__global__ __launch_bounds__(256) void k_dot3_f(int n, const float* __restrict__ a,
                                                double* __restrict__ out /*[3][kPart]*/) {
  double d[3] = {0, 0, 0};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float4 t = ld4(a, i);
    d[0] += double(t.x) * t.x;
    d[1] += double(t.y) * t.y;
    d[2] += double(t.z) * t.z;
  }
  reduce3_part(d[0], d[1], d[2], out);
}

// fp64 [n,3] <-> fp32 rows of kVecStride floats
__global__ __launch_bounds__(256) void k_cvt_d2f(int n, const double* __restrict__ a,
                                                 float* __restrict__ out) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) st4(out, i, float(a[3 * i]), float(a[3 * i + 1]), float(a[3 * i + 2]));
}

__global__ __launch_bounds__(256) void k_cvt_f2d(int n, const float* __restrict__ a,
                                                 double* __restrict__ out) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 t = ld4(a, i);
  out[3 * i] = double(t.x);
  out[3 * i + 1] = double(t.y);
  out[3 * i + 2] = double(t.z);
}

// y = B^-1 rhs to rtol, everything fp32 (rhs and y are float [n,3]); y starts at 0.
static int amg_pcg_f32(Ctx* c, int N, const WorkF& w, AmgHierarchy* H, const float* rhs, float* y,
                       double rtol, int32_t max_it, GraphCache* cache, int32_t* iters,
                       double resid[3]) {
  const dim3 grid(ceil_div(N, 256)), block(256);
  const int32_t *ip, *ix;
  const float* bv;
  amg_fine_matrix(H, &ip, &ix, &bv);
  PQ_HIP(hipMemsetAsync(w.sc, 0, sizeof(Scal), c->stream));
  PQ_HIP(hipMemsetAsync(y, 0, size_t(N) * kVecStride * 4, c->stream));
  PQ_HIP(hipMemcpyAsync(w.r, rhs, size_t(N) * kVecStride * 4, hipMemcpyDeviceToDevice, c->stream));
  const dim3 rgrid(reduce_grid_f(N));  // kernels that end in a reduction
  hipLaunchKernelGGL(k_dot3_f, rgrid, block, 0, c->stream, N, rhs, w.sc->bb);
  PQ_TRY(amg_vcycle_f32(c, H, w.r, w.z, w.sc->rz[0]));
  hipLaunchKernelGGL(k_part_final, dim3(1), block, 0, c->stream, w.sc->rz[0], w.sc->rz_tot[0]);
  PQ_HIP(hipMemcpyAsync(w.dir, w.z, size_t(N) * kVecStride * 4, hipMemcpyDeviceToDevice, c->stream));
  for (int k = 0; k < 3; ++k) resid[k] = 1.0;
  *iters = 0;
  auto iteration = [&](int par) -> int {
    {
      ProfScope pk(c, "k_bspmv_f", 1, 2);
      hipLaunchKernelGGL(k_bspmv_f, rgrid, block, 0, c->stream, N, ip, ix, bv, w.dir, w.q, w.sc, par);
    }
    hipLaunchKernelGGL(k_update_r_f, rgrid, block, 0, c->stream, N, w.dir, w.q, y, w.r, w.sc, par);
    PQ_TRY(amg_vcycle_f32(c, H, w.r, w.z, w.sc->rz[par ^ 1]));
    hipLaunchKernelGGL(k_direction_f, rgrid, block, 0, c->stream, N, w.z, w.dir, w.sc, par);
    return 0;
  };
  if (!amg_graphs_enabled()) cache = nullptr;
  auto run_burst = [&](int len) -> int {
    hipGraphExec_t exec = nullptr;
    if (cache)
      for (auto& g : cache->items)
        if (g.b == static_cast<const void*>(H) && g.x == y && g.op == 200 + len) exec = g.exec;
    if (cache && !exec) {
      hipGraph_t graph = nullptr;
      PQ_HIP(hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed));
      int rc = 0;
      for (int bi = 0; bi < len && rc == 0; ++bi) rc = iteration(bi & 1);
      PQ_HIP(hipStreamEndCapture(c->stream, &graph));
      if (rc != 0) return rc;
      PQ_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
      (void)hipGraphDestroy(graph);
      cache->items.push_back({static_cast<const void*>(H), y, 200 + len, exec});
    }
    if (exec) {
      PQ_HIP(hipGraphLaunch(exec, c->stream));
    } else {
      for (int bi = 0; bi < len; ++bi) PQ_TRY(iteration(bi & 1));
    }
    return 0;
  };
  int it = 0;
  bool done = false;
  if (const int fixed = amg_fixed_iterations()) {
    // a fixed, even number of iterations and no look at the residual: no host round trip in
    // the whole B-solve (the outer CG is flexible, an inexact B^-1 costs it a few steps)
    const int len = std::min<int>((fixed + 1) & ~1, std::max(2, max_it & ~1));
    {
      ProfScope ps(c, "lbc_amg_iter", len);
      PQ_TRY(run_burst(len));
    }
    PQ_HIP(hipGetLastError());
    *iters = len;
    for (int k = 0; k < 3; ++k) resid[k] = 0.0;
    return 0;
  }
  while (!done && it < max_it) {
    int len = it == 0 ? amg_first_burst() : amg_next_burst();
    if (len > max_it - it) len = std::max(2, (max_it - it + 1) & ~1);
    {
      ProfScope ps(c, "lbc_amg_iter", len);
      PQ_TRY(run_burst(len));
    }
    it += len;
    double h[2][3];
    {
      const double* parts[2] = {w.sc->rr[1], w.sc->bb};
      PQ_TRY(part_totals_host(c, parts, 2, h));
    }
    const double* rr = h[0];
    const double* bb = h[1];
    if (bb[0] == 0.0 && bb[1] == 0.0 && bb[2] == 0.0) {
      for (int k = 0; k < 3; ++k) resid[k] = 0.0;
      *iters = it;
      return 0;
    }
    done = true;
    for (int k = 0; k < 3; ++k) {
      resid[k] = bb[k] > 0 ? std::sqrt(rr[k] / bb[k]) : 0.0;
      if (!(resid[k] <= rtol)) done = false;
      if (!std::isfinite(resid[k])) {
        *iters = it;
        return fail(PYQSM_ENOCONV, "multigrid CG (fp32) broke down after %d iterations", it);
      }
    }
    // CG on an SPD system does not leave the residual ten times above the right-hand side for
    // long: this one is diverging (see `diverged` in lbc_solve_core), no point in going to max_it
    if (!done && it >= 16 && std::max(resid[0], std::max(resid[1], resid[2])) > 10.0) {
      *iters = it;
      return fail(PYQSM_ENOCONV, "multigrid CG (fp32) is diverging after %d iterations, residual %.3e", it,
                  std::max(resid[0], std::max(resid[1], resid[2])));
    }
  }
  PQ_HIP(hipGetLastError());
  *iters = it;
  return done ? 0 : fail(PYQSM_ENOCONV, "multigrid CG (fp32) reached %d iterations, residual %.3e", it,
                         std::max(resid[0], std::max(resid[1], resid[2])));
}

// ---- Riccati weights for the preconditioner ----------------------------------------------------
// B^2 = (c L + W)^2 = c^2 L^2 + c (L W + W L) + W^2, and as a quadratic form
//   x'(L W + W L)x = sum_ij w_ij (w_i + w_j)/2 (x_i - x_j)^2  +  sum_i (L w)_i x_i^2
// (w_ij >= 0 the edge weights of L): a gradient term, which is harmless, and a POTENTIAL (L w)_i that
// is negative wherever w has a local minimum. With the rough per-point W_H of the contractions after
// the second (0.7 ... 1000 between neighbours) that potential cancels most of w_i^2 on small plateaus
// around the minima: B^2 << A there, B^-2 A gets a tail of eigenvalues up to ~11 (measured with exact
// solves on 20 k points) and the outer CG needs 60-80 steps instead of 10-20.
// The preconditioner is therefore built from weights w~ that solve the discrete Riccati equation
//   w~_i^2 + c (L w~)_i = w_i^2,
// for which (c L + W~)^2 = A + c * (gradient term) >= A: no eigenvalue above 1 is left. Newton's
// method on F(w~) = w~^2 + c L w~ - w^2: the Jacobian c L + 2 W~ is a matrix of B's kind, solved by
// the multigrid CG that is there anyway (the hierarchy of B as its preconditioner).

// F (column 0 of an [n,3] vector, columns 1-2 zero) and its negative as the right-hand side
__global__ __launch_bounds__(256) void k_riccati_f(int n, const int32_t* __restrict__ indptr,
                                                   const int32_t* __restrict__ indices,
                                                   const double* __restrict__ vals,
                                                   const double* __restrict__ wl,
                                                   const double* __restrict__ wt,
                                                   const double* __restrict__ wh,
                                                   double* __restrict__ negf, double* __restrict__ w2,
                                                   int mark /* column 1 := (-F_i > w_i^2 / 2), see
                                                   kRiccatiFrac; 0: a right-hand side, column 1 zero */) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double a = 0.0;
  for (int j = indptr[i]; j < indptr[i + 1]; ++j) a += vals[j] * wt[indices[j]];
  const double f = wt[i] * wt[i] + wl[i] * a - wh[i] * wh[i];
  negf[3 * i] = -f;
  negf[3 * i + 1] = mark && -f > 0.5 * wh[i] * wh[i] ? 1.0 : 0.0;
  negf[3 * i + 2] = 0.0;
  w2[3 * i] = wh[i] * wh[i];
  w2[3 * i + 1] = 0.0;
  w2[3 * i + 2] = 0.0;
}

// w~ += delta (column 0), never below a quarter of its value (Newton from above stays positive in
// exact arithmetic; the inexact solves get this guard); wj = 2 w~ for the next Jacobian
__global__ __launch_bounds__(256) void k_riccati_step(int n, const double* __restrict__ delta,
                                                      double* __restrict__ wt, double* __restrict__ wj) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double w = wt[i];
  double v = w + delta[3 * i];
  if (!(v >= 0.25 * w)) v = 0.25 * w;
  wt[i] = v;
  wj[i] = 2.0 * v;
}

__global__ __launch_bounds__(256) void k_scale2(int n, const double* __restrict__ a, double* __restrict__ out) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = 2.0 * a[i];
}

// PYQSM_RICCATI=0: the preconditioner keeps W_H itself; 2: Riccati weights whenever W_H varies;
// default 1: while W_H is rough (kRiccatiFrac). Read per solve, so that a test can compare the modes.
static int riccati_mode() {
  const char* e = getenv("PYQSM_RICCATI");
  return e ? atoi(e) : 1;
}

// Device-resident contraction solve.
//
// Uniform Laplacian weight c (what extract_skeleton always passes): the system
// A = c^2 L^2 + W_H^2 is preconditioned by B^2 with B = c L + W_H, which is
// symmetric positive definite and spectrally within a small factor of A
// ((c l + h)^2 / (c^2 l^2 + h^2) lies in [1, 2] for every eigenvalue l >= 0 when
// W_H = h I). cond(B) ~ sqrt(cond(A)), so the outer flexible CG needs a few dozen
// steps and each step two Jacobi-PCG solves with B. cond(A) reaches 1e13 on
// contracted clouds: far beyond what Jacobi-PCG on A itself can do.
// Non-uniform wl: plain Jacobi-PCG on A.
static int lbc_solve_core(Ctx* c, const DevCsr& L, int64_t n, const double* wl, bool wl_edge_const,
                          const double* wh, const double* pts, double rtol, int32_t max_it, double* x,
                          int32_t* iters, double resid[3]) {
  const int N = int(n);
  const dim3 grid(ceil_div(n, 256)), block(256);
  double *b, *minv_a, *d_tmp;
  PQ_TRY(c->arena.get(size_t(n) * 3, &b));
  PQ_TRY(c->arena.get(size_t(n), &minv_a));
  PQ_TRY(c->arena.get(size_t(3) * kPart, &d_tmp));
  double* d_parts[5];  // the outer iteration's dot products of one step: launched one after the other, read in ONE look
  for (int a = 0; a < 5; ++a) PQ_TRY(c->arena.get(size_t(3) * kPart, &d_parts[a]));
  hipLaunchKernelGGL(k_rhs, grid, block, 0, c->stream, N, wh, pts, b);
  PQ_HIP(hipMemcpyAsync(x, pts, size_t(n) * 24, hipMemcpyDeviceToDevice, c->stream));
  Work wa;
  PQ_TRY(alloc_work(c, n, &wa));
  System SA{L, N, OP_A, wl, wh, minv_a};
  if (!wl_edge_const) {
    hipLaunchKernelGGL(k_diag, grid, block, 0, c->stream, N, L.indptr, L.vals, wl, wh, minv_a);
    GraphCache cache;
    return jacobi_pcg(c, SA, wa, b, x, false, rtol, max_it, "lbc_cg_iter", &cache, iters, resid);
  }
  // ---- B^2-preconditioned flexible CG ------------------------------------------
  double *minv_b, *r, *z, *z_old, *dir, *q, *y, *x_best;
  PQ_TRY(c->arena.get(size_t(n), &minv_b));
  PQ_TRY(c->arena.get(size_t(n) * 3, &r));
  PQ_TRY(c->arena.get(size_t(n) * 3, &z));
  PQ_TRY(c->arena.get(size_t(n) * 3, &z_old));
  PQ_TRY(c->arena.get(size_t(n) * 3, &dir));
  PQ_TRY(c->arena.get(size_t(n) * 3, &q));
  PQ_TRY(c->arena.get(size_t(n) * 3, &y));
  PQ_TRY(c->arena.get(size_t(n) * 3, &x_best));
  Work wb;
  PQ_TRY(alloc_work(c, n, &wb));
  hipLaunchKernelGGL(k_diag_b, grid, block, 0, c->stream, N, L.indptr, L.indices, L.vals,
                     wl, wh, minv_b);
  System SB{L, N, OP_B, wl, wh, minv_b};
  // Multilevel preconditioner for the B-solves (amg.hip): 12-17 cycles per solve where
  // Jacobi-PCG needs 200-700 sparse passes. PYQSM_AMG=0 selects Jacobi-PCG; it is also
  // the fallback when no hierarchy can be built (tiny or fully decoupled systems).
  AmgHierarchy* amg = nullptr;
  const char* amg_env = getenv("PYQSM_AMG");
  if (!(amg_env && amg_env[0] == '0')) {
    ProfScope ps(c, "lbc_amg_build");
    if (amg_build(c, L, N, wl, wh, &amg) != 0 || amg_levels(amg) < 2) {
      amg_destroy(amg);
      amg = nullptr;
    }
  }
  struct AmgGuard {
    AmgHierarchy* h;
    ~AmgGuard() { amg_destroy(h); }
  } amg_guard{amg};
  int32_t total_inner = 0;
  GraphCache cache;
  // Two-phase outer iteration when the Riccati weights are in use (see k_riccati_f): phase 1 with
  // (c L + W~)^-2, whose spectrum has no upper tail; its error estimate |z| / |x| UNDER-weights the
  // few modes in which the lifted weights make B~^2 >> A (eigenvalues down to 0.03 measured), so
  // when it reports convergence the iteration is restarted with the plain B^-2 — whose estimate
  // is the one the tolerance was calibrated on (spectrum >= 1/2) — and runs until that one agrees.
  AmgHierarchy *amg_r = nullptr, *amg_b = nullptr;
  AmgGuard amg_r_guard{nullptr};
  const double* wh_r = nullptr;
  int phase = 0;
  double kInnerRtol = kInnerRtolDefault;
  if (const char* e = getenv("PYQSM_INNER_RTOL")) {  // tuning knob
    const double v = atof(e);
    if (v > 0.0 && v < 1.0) kInnerRtol = v;
  }
  // fp32 B-solves when they are asked for no more than four digits (the default asks for two);
  // PYQSM_LBC_F32=0 keeps them in fp64
  const char* f32e = getenv("PYQSM_LBC_F32");
  const bool use_f32 = amg && kInnerRtol >= 1e-4 && !(f32e && f32e[0] == '0');
  WorkF wf{nullptr, nullptr, nullptr, nullptr, nullptr};
  float *f_rhs = nullptr, *f_y = nullptr, *f_out = nullptr;
  if (use_f32) {
    PQ_TRY(c->arena.get(size_t(n) * kVecStride, &wf.r));
    PQ_TRY(c->arena.get(size_t(n) * kVecStride, &wf.z));
    PQ_TRY(c->arena.get(size_t(n) * kVecStride, &wf.dir));
    PQ_TRY(c->arena.get(size_t(n) * kVecStride, &wf.q));
    PQ_TRY(c->arena.get(size_t(n) * kVecStride, &f_rhs));
    PQ_TRY(c->arena.get(size_t(n) * kVecStride, &f_y));
    PQ_TRY(c->arena.get(size_t(n) * kVecStride, &f_out));
    wf.sc = wb.sc;
  }
  const bool trace = getenv("PYQSM_LBC_TRACE") != nullptr;
  // ---- Riccati weights for B (k_riccati_f) -------------------------------------------------------
  int riccati_its = 0;
  if (amg && riccati_mode() != 0) {
    ProfScope psr(c, "lbc_riccati");
    double *wt, *wj, *negf, *w2, *delta;
    PQ_TRY(c->arena.get(size_t(n), &wt));
    PQ_TRY(c->arena.get(size_t(n), &wj));
    PQ_TRY(c->arena.get(size_t(n) * 3, &negf));
    PQ_TRY(c->arena.get(size_t(n) * 3, &w2));
    PQ_TRY(c->arena.get(size_t(n) * 3, &delta));
    PQ_HIP(hipMemcpyAsync(wt, wh, size_t(n) * 8, hipMemcpyDeviceToDevice, c->stream));
    hipLaunchKernelGGL(k_scale2, grid, block, 0, c->stream, N, wh, wj);
    double wnorm = 0.0;
    static const double ric_tol = [] {  // PYQSM_RICCATI_TOL: tuning knob for kRiccatiTol
      const char* e = getenv("PYQSM_RICCATI_TOL");
      const double v = e ? atof(e) : -1.0;
      return v > 0.0 && v < 1.0 ? v : kRiccatiTol;
    }();
    static const double frac_min = [] {  // PYQSM_RICCATI_FRAC: tuning knob for kRiccatiFrac
      const char* e = getenv("PYQSM_RICCATI_FRAC");
      const double v = e ? atof(e) : -1.0;
      return v >= 0.0 && v <= 1.0 ? v : kRiccatiFrac;
    }();
    for (int k = 0; k <= kRiccatiMaxIt; ++k) {
      hipLaunchKernelGGL(k_riccati_f, grid, block, 0, c->stream, N, L.indptr, L.indices, L.vals, wl, wt, wh,
                         negf, w2, k == 0 ? 1 : 0);
      PQ_HIP(hipGetLastError());
      double ff[3], ww[3];
      PQ_TRY(dot3_host(c, N, negf, negf, d_tmp, ff));
      if (k == 0) {
        PQ_TRY(dot3_host(c, N, w2, w2, d_tmp, ww));
        wnorm = ww[0];
      }
      const double rel = wnorm > 0 ? std::sqrt(ff[0] / wnorm) : 0.0;
      if (trace)
        fprintf(stderr, "riccati %d: |F|/|w^2| = %.3e%s\n", k, rel,
                k == 0 ? (" cancelled fraction " + std::to_string(ff[1] / double(N))).c_str() : "");
      // Newton gone wrong (it never did on the clouds tried): the plain preconditioner is always valid
      if (!std::isfinite(rel) || (k == kRiccatiMaxIt && rel > 10.0 * ric_tol)) {
        riccati_its = 0;
        break;
      }
      // uniform W_H solves the equation itself (the first two contractions): rel = 0 at k = 0
      if (rel <= ric_tol || k == kRiccatiMaxIt) break;
      if (k == 0) {
        if (riccati_mode() == 1 && ff[1] < frac_min * double(N)) break;  // W_H smooth enough for plain B
        hipLaunchKernelGGL(k_riccati_f, grid, block, 0, c->stream, N, L.indptr, L.indices, L.vals, wl, wt,
                           wh, negf, w2, 0);  // the same F as a right-hand side
      }
      if (max_it - total_inner < 4 * kRiccatiInnerMaxIt) {  // not on a caller's tight iteration budget
        riccati_its = 0;
        break;
      }
      System SJ{L, N, OP_B, wl, wj, minv_b};
      int32_t itj = 0;
      double rsj[3];
      const int rcj = amg_pcg(c, SJ, wb, amg, negf, delta, kRiccatiInnerRtol, kRiccatiInnerMaxIt, &cache,
                              &itj, rsj);
      if (rcj != 0 && rcj != PYQSM_ENOCONV) return rcj;
      total_inner += itj;
      hipLaunchKernelGGL(k_riccati_step, grid, block, 0, c->stream, N, delta, wt, wj);
      ++riccati_its;
    }
    if (riccati_its > 0) {  // phase 1 of the outer iteration runs with (c L + W~)^-2
      ProfScope ps(c, "lbc_amg_build");
      if (amg_build(c, L, N, wl, wt, &amg_r) != 0 || amg_levels(amg_r) < 2) {
        amg_destroy(amg_r);
        amg_r = nullptr;
      }
      amg_r_guard.h = amg_r;
      if (amg_r) {
        wh_r = wt;
        amg_b = amg;
        amg = amg_r;
        SB.wh = wh_r;
        phase = 1;
      }
    }
  }
  // max_it caps the total number of inner (sparse-pass) iterations
  auto budget = [&]() { return std::max<int32_t>(1, std::min<int32_t>(kInnerMaxIt, max_it - total_inner)); };
  // B-solves that break down: the fp32 multigrid CG loses its digits on the collapsed clouds of
  // late contractions — cot weights of degenerate triangles put c L_ii at 1e12 where W_H is 1e3,
  // below fp32's resolution of a row, and B^-1 r (the right-hand side of the second solve) is
  // dominated by smooth modes whose residual fp32 cannot evaluate. Seen: one solve of a perturbed
  // 20-contraction run spent 11 000 iterations feeding garbage to the outer iteration; a system
  // with 30x the usual W_L took 1 753 iterations where the fp64 operator takes 376. An fp32 solve
  // that diverges (amg_pcg_f32 returns after 16 iterations) or needs more than kF32MaxIt
  // iterations is therefore repeated one rung down — fp64 operator with the same cycle — and
  // the solve stays there; an fp64 solve that DIVERGES goes on to Jacobi-PCG.
  // (CG's residual is not monotone: a solve cut short by the caller's max_it after a few
  // iterations may stand above 1 without diverging, and an exhausted budget is not spent again.)
  auto diverged = [&](int rc, int32_t its, const double rs[3]) {
    if (rc == 0 || total_inner >= max_it) return false;
    const double w = std::max(rs[0], std::max(rs[1], rs[2]));
    return !std::isfinite(w) || (its >= 16 && w > 1.0);
  };
  int rung = 0;  // 0: fp32 multigrid CG, 1: fp64 operator, 2: Jacobi-PCG
  auto precond = [&](const double* rhs, double* out) -> int {  // out = B^-1 B^-1 rhs
    int32_t it1 = 0, it2 = 0;
    double rs[3];
    if (amg && use_f32 && rung == 0) {
      hipLaunchKernelGGL(k_cvt_d2f, grid, block, 0, c->stream, N, rhs, f_rhs);
      int rc = amg_pcg_f32(c, N, wf, amg, f_rhs, f_y, kInnerRtol, std::min(budget(), kF32MaxIt), &cache, &it1,
                           rs);
      if (rc != 0 && rc != PYQSM_ENOCONV) return rc;
      total_inner += it1;
      bool bad = rc != 0 && total_inner < max_it;  // fp32: stalling counts as well
      if (!bad) {
        rc = amg_pcg_f32(c, N, wf, amg, f_y, f_out, kInnerRtol, std::min(budget(), kF32MaxIt), &cache, &it2, rs);
        if (rc != 0 && rc != PYQSM_ENOCONV) return rc;
        total_inner += it2;
        bad = rc != 0 && total_inner < max_it;
      }
      if (!bad) {
        hipLaunchKernelGGL(k_cvt_f2d, grid, block, 0, c->stream, N, f_out, out);
        return 0;
      }
      rung = 1;
      if (trace)
        fprintf(stderr, "  fp32 B-solve gave up after %d + %d iterations (%.3e %.3e %.3e): fp64 operator from here\n",
                it1, it2, rs[0], rs[1], rs[2]);
      it1 = it2 = 0;
    }
    if (amg && rung <= 1) {
      int rc = amg_pcg(c, SB, wb, amg, rhs, y, kInnerRtol, std::min(budget(), kAmgMaxIt), &cache, &it1, rs);
      if (rc != 0 && rc != PYQSM_ENOCONV) return rc;
      total_inner += it1;
      bool bad = diverged(rc, it1, rs);
      if (!bad) {
        rc = amg_pcg(c, SB, wb, amg, y, out, kInnerRtol, std::min(budget(), kAmgMaxIt), &cache, &it2, rs);
        if (rc != 0 && rc != PYQSM_ENOCONV) return rc;
        total_inner += it2;
        bad = diverged(rc, it2, rs);
      }
      if (!bad) return 0;
      rung = 2;
      if (trace)
        fprintf(stderr, "  multigrid B-solve diverged after %d + %d iterations (%.3e %.3e %.3e): Jacobi-PCG from here\n",
                it1, it2, rs[0], rs[1], rs[2]);
      it1 = it2 = 0;
    }
    int rc = jacobi_pcg(c, SB, wb, rhs, y, true, kInnerRtol, budget(), "lbc_inner_iter", &cache, &it1,
                        rs);
    if (rc != 0 && rc != PYQSM_ENOCONV) return rc;
    total_inner += it1;
    rc = jacobi_pcg(c, SB, wb, y, out, true, kInnerRtol, budget(), "lbc_inner_iter", &cache, &it2, rs);
    if (rc != 0 && rc != PYQSM_ENOCONV) return rc;
    total_inner += it2;
    return 0;
  };
  // r = b - A x0
  apply_op(c, SA, wa, x, q, nullptr);
  hipLaunchKernelGGL(k_sub3, grid, block, 0, c->stream, N, b, q, r);
  double bb[3], rr[3], rz[3];
  PQ_TRY(dot3_host(c, N, b, b, d_tmp, bb));
  PQ_TRY(dot3_host(c, N, r, r, d_tmp, rr));
  auto rel = [&](const double v[3], double out[3]) {
    double worst = 0.0;
    for (int k = 0; k < 3; ++k) {
      out[k] = bb[k] > 0 ? std::sqrt(v[k] / bb[k]) : 0.0;
      worst = std::max(worst, out[k]);
    }
    return worst;
  };
  // Convergence is judged on z = B^-2 r: B^-2 A has its spectrum in [1/2, 1] for uniform
  // W_H (a modest interval otherwise), so |z| / |x| estimates the relative ERROR of x, which
  // is what the caller's 1e-5 position tolerance is about. The true residual |r| / |b| is
  // tracked as well (and reported), but with cond(A) up to 1e10 it is neither monotone
  // under CG nor a usable measure of the error.
  rel(rr, resid);
  double cur_res[3] = {resid[0], resid[1], resid[2]};
  double best = HUGE_VAL;
  double best_res[3] = {resid[0], resid[1], resid[2]};
  PQ_HIP(hipMemcpyAsync(x_best, x, size_t(n) * 24, hipMemcpyDeviceToDevice, c->stream));
  int outer = 0, best_outer = 0;
  bool done = std::max(resid[0], std::max(resid[1], resid[2])) <= rtol;
  // after every preconditioner application: error estimate of the current x
  auto dot_launch = [&](const double* a, const double* bvec, double* part) {
    hipLaunchKernelGGL(k_dot3, dim3(reduce_grid(N)), dim3(256), 0, c->stream, N, a, bvec, part);
  };
  auto judge = [&](const double zz[3], const double xx[3]) -> int {
    double est = 0.0;
    for (int k = 0; k < 3; ++k) est = std::max(est, xx[k] > 0 ? std::sqrt(zz[k] / xx[k]) : 0.0);
    if (trace)
      fprintf(stderr, "lbc outer %d inner %d resid %.3e est %.3e\n", outer, total_inner,
              std::max(cur_res[0], std::max(cur_res[1], cur_res[2])), est);
    if (!std::isfinite(est)) return 1;
    if (est < best) {
      best = est;
      best_outer = outer;
      for (int k = 0; k < 3; ++k) best_res[k] = cur_res[k];
      PQ_HIP(hipMemcpyAsync(x_best, x, size_t(n) * 24, hipMemcpyDeviceToDevice, c->stream));
    }
    if (est <= rtol) done = true;
    return 0;
  };
  // (re)start of the CG with the current preconditioner: z = M^-1 r, dir = z
  auto restart = [&]() -> int {
    PQ_TRY(precond(r, z));
    PQ_HIP(hipMemcpyAsync(dir, z, size_t(n) * 24, hipMemcpyDeviceToDevice, c->stream));
    dot_launch(r, z, d_parts[0]);
    dot_launch(z, z, d_parts[1]);
    dot_launch(x, x, d_parts[2]);
    PQ_HIP(hipGetLastError());
    double t[3][3];
    PQ_TRY(part_totals_host(c, d_parts, 3, t));
    for (int k = 0; k < 3; ++k) rz[k] = t[0][k];
    if (judge(t[1], t[2]) != 0) return fail(PYQSM_EHIP, "contraction solve: non-finite preconditioned residual");
    return 0;
  };
  if (!done) {
    ProfScope ps0(c, "lbc_first_precond");
    PQ_TRY(restart());
  }
  for (;;) {
  while (!done && outer < kOuterMaxIt && total_inner < max_it) {
    ProfScope ps(c, "lbc_outer_iter");
    apply_op(c, SA, wa, dir, q, nullptr);
    double pq[3];
    PQ_TRY(dot3_host(c, N, dir, q, d_tmp, pq));
    S3 alpha, nalpha;
    for (int k = 0; k < 3; ++k) {
      alpha.v[k] = pq[k] != 0.0 ? rz[k] / pq[k] : 0.0;
      nalpha.v[k] = -alpha.v[k];
    }
    hipLaunchKernelGGL(k_axpy3, grid, block, 0, c->stream, N, alpha, dir, x);
    hipLaunchKernelGGL(k_axpy3, grid, block, 0, c->stream, N, nalpha, q, r);
    ++outer;
    PQ_HIP(hipMemcpyAsync(z_old, z, size_t(n) * 24, hipMemcpyDeviceToDevice, c->stream));
    PQ_TRY(precond(r, z));
    // the five dot products of the step in one look (each look is a round trip; they used to be
    // five, plus the one for alpha above: 0.2 ms per outer step). |r|^2 is only needed for the
    // report and the breakdown test, so it waits for the others.
    dot_launch(r, r, d_parts[0]);
    dot_launch(z, z, d_parts[1]);
    dot_launch(x, x, d_parts[2]);
    dot_launch(r, z, d_parts[3]);
    dot_launch(r, z_old, d_parts[4]);
    PQ_HIP(hipGetLastError());
    double t5[5][3];
    PQ_TRY(part_totals_host(c, d_parts, 5, t5));
    for (int k = 0; k < 3; ++k) rr[k] = t5[0][k];
    const double worst = rel(rr, cur_res);
    if (!std::isfinite(worst)) break;
    const int jr = judge(t5[1], t5[2]);
    if (jr < 0) return jr;
    if (jr > 0 || done) break;
    // attainable accuracy reached. Phase 1 leaves much sooner: its estimate flattens once what is
    // left sits in the modes the Riccati weights over-weight (measured: 1.7e-8 after 23 steps, no
    // better after 35), and those are the plain preconditioner's to finish.
    static const int ric_stall = [] {  // PYQSM_RICCATI_STALL: tuning knob for kRiccatiStall
      const char* e = getenv("PYQSM_RICCATI_STALL");
      const int v = e ? atoi(e) : 0;
      return v > 0 ? v : kRiccatiStall;
    }();
    if (outer - best_outer >= (phase == 1 ? ric_stall : kOuterStall)) break;
    // flexible (Polak-Ribiere) beta: the inner solves are not exact
    const double* rz_new = t5[3];
    const double* rzo = t5[4];
    S3 beta;
    for (int k = 0; k < 3; ++k) {
      beta.v[k] = rz[k] != 0.0 ? (rz_new[k] - rzo[k]) / rz[k] : 0.0;
      if (!(beta.v[k] > 0.0)) beta.v[k] = 0.0;
      rz[k] = rz_new[k];
    }
    hipLaunchKernelGGL(k_xpay3, grid, block, 0, c->stream, N, beta, z, dir);
  }
  if (phase == 1 && outer < kOuterMaxIt && total_inner < max_it) {
    // converged (or stalled) by the Riccati-preconditioned estimate: go on with the plain B^-2
    // from the best iterate, until ITS estimate agrees
    phase = 0;
    amg = amg_b;
    SB.wh = wh;
    if (trace) fprintf(stderr, "lbc outer %d: phase 2 (plain B)\n", outer);
    PQ_HIP(hipMemcpyAsync(x, x_best, size_t(n) * 24, hipMemcpyDeviceToDevice, c->stream));
    apply_op(c, SA, wa, x, q, nullptr);
    hipLaunchKernelGGL(k_sub3, grid, block, 0, c->stream, N, b, q, r);
    PQ_TRY(dot3_host(c, N, r, r, d_tmp, rr));
    rel(rr, cur_res);
    done = false;
    best = HUGE_VAL;
    best_outer = outer;
    PQ_TRY(restart());
    continue;
  }
  break;
  }
  PQ_HIP(hipGetLastError());
  *iters = total_inner + outer;
  PQ_HIP(hipMemcpyAsync(x, x_best, size_t(n) * 24, hipMemcpyDeviceToDevice, c->stream));
  for (int k = 0; k < 3; ++k) resid[k] = best_res[k];
  if (!done)
    return fail(PYQSM_ENOCONV,
                "contraction solve stopped after %d outer / %d inner iterations; best error "
                "estimate %.3e", outer, total_inner, best);
  return 0;
}

// flag = 1 when the Laplacian weight differs across some edge of L (then B = W_L L + W_H would
// not be symmetric and the solve takes the plain path)
__global__ __launch_bounds__(256) void k_edge_const(int n, const int32_t* __restrict__ indptr,
                                                    const int32_t* __restrict__ indices,
                                                    const double* __restrict__ wl,
                                                    int32_t* __restrict__ flag) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double w = wl[i];
  bool differs = false;
  for (int j = indptr[i]; j < indptr[i + 1]; ++j) differs |= wl[indices[j]] != w;
  if (differs) *flag = 1;  // racing stores of the same value
}

// ---- spatially sorted unknowns -----------------------------------------------------------
// Every sparse pass gathers 24-byte rows of a vector at the columns of a matrix row, i.e. at
// the point's mesh neighbours. In the caller's point order those are anywhere in the
// array; sorted by grid cell they sit within a few cache lines of each other. The solve
// therefore runs on P L P', P w, P p and un-permutes the result (measured on the 1 M-point
// forest: -22 % per multigrid-CG iteration; the permutation costs ~1 ms per solve).
// key of every point = its grid cell, value = its index: the input of the stable sort
__global__ __launch_bounds__(256) void k_perm_keys(int n, const int32_t* __restrict__ gorder,
                                                   const int32_t* __restrict__ cell_of,
                                                   uint32_t* __restrict__ keys,
                                                   int32_t* __restrict__ vals) {
  int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= n) return;
  keys[gorder[f]] = uint32_t(cell_of[f]);
  vals[f] = f;
}

__global__ __launch_bounds__(256) void k_perm_invert(int n, const int32_t* __restrict__ order,
                                                     int32_t* __restrict__ pos_of) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) pos_of[order[i]] = i;
}

__global__ __launch_bounds__(256) void k_perm_rowlen(int n, const int32_t* __restrict__ order,
                                                     const int32_t* __restrict__ indptr,
                                                     int32_t* __restrict__ new_indptr) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  new_indptr[i] = i < n ? indptr[order[i] + 1] - indptr[order[i]] : 0;
}

__global__ __launch_bounds__(256) void k_perm_fill(int n, const int32_t* __restrict__ order,
                                                   const int32_t* __restrict__ pos_of,
                                                   const int32_t* __restrict__ indptr,
                                                   const int32_t* __restrict__ indices,
                                                   const double* __restrict__ vals,
                                                   const int32_t* __restrict__ new_indptr,
                                                   int32_t* __restrict__ new_indices,
                                                   double* __restrict__ new_vals,
                                                   const double* __restrict__ wh,
                                                   const double* __restrict__ wl,
                                                   const double* __restrict__ pts,
                                                   double* __restrict__ wh_p,
                                                   double* __restrict__ wl_p,
                                                   double* __restrict__ pts_p) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int o = order[i];
  int w = new_indptr[i];
  for (int j = indptr[o]; j < indptr[o + 1]; ++j, ++w) {
    new_indices[w] = pos_of[indices[j]];
    new_vals[w] = vals[j];
  }
  wh_p[i] = wh[o];
  wl_p[i] = wl[o];
  pts_p[3 * i] = pts[3 * o];
  pts_p[3 * i + 1] = pts[3 * o + 1];
  pts_p[3 * i + 2] = pts[3 * o + 2];
}

__global__ __launch_bounds__(256) void k_perm_back(int n, const int32_t* __restrict__ order,
                                                   const double* __restrict__ x_p,
                                                   double* __restrict__ x) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int o = order[i];
  x[3 * o] = x_p[3 * i];
  x[3 * o + 1] = x_p[3 * i + 1];
  x[3 * o + 2] = x_p[3 * i + 2];
}

int lbc_solve_device(Ctx* c, const DevCsr& L, int64_t n, const double* wl, bool wl_edge_const,
                     const double* wh, const double* pts, double rtol, int32_t max_it, double* x,
                     int32_t* iters, double resid[3]) {
  ProfScope pst(c, "lbc_solve_total");
  const char* pe = getenv("PYQSM_LBC_SORT");
  if (!wl_edge_const || n < 4096 || (pe && pe[0] == '0'))
    return lbc_solve_core(c, L, n, wl, wl_edge_const, wh, pts, rtol, max_it, x, iters, resid);
  const int N = int(n);
  const dim3 grid(ceil_div(n, 256)), grid1(ceil_div(n + 1, 256)), block(256);
  // cells of ~1/512 of the extent (the dense grid is capped at 2^24 cells; the edge doubles to
  // fit). Finer cells = neighbours closer in memory: 1/128 -> 1/512 took 10 % off an iteration;
  // numbering the cells block by block (8^3) instead of row by row changed nothing, and so did
  // staging the CSR segments of 64 rows through LDS — what is left is the gathers themselves.
  double mn[3], mx[3];
  PQ_TRY(cloud_bbox(c, pts, n, mn, mx));
  double ext = std::max(mx[0] - mn[0], std::max(mx[1] - mn[1], mx[2] - mn[2]));
  if (!(ext > 0.0) || !std::isfinite(ext))
    return lbc_solve_core(c, L, n, wl, wl_edge_const, wh, pts, rtol, max_it, x, iters, resid);
  double box[6] = {mn[0], mn[1], mn[2], mx[0], mx[1], mx[2]};
  DevGrid g;
  PQ_TRY(build_grid(c, pts, n, ext / 512.0, int64_t(1) << 24, &g, box));
  // The grid's own order inside a cell is the arrival order of atomics. The unknowns are
  // numbered by (cell, original index) instead — a stable sort — so that the same system is
  // the same numbering, the same aggregates and the same rounding on every run.
  uint32_t* keys = nullptr;
  int32_t* order = nullptr;
  PQ_TRY(c->arena.get(size_t(n), &keys));
  PQ_TRY(c->arena.get(size_t(n), &order));
  hipLaunchKernelGGL(k_perm_keys, grid, block, 0, c->stream, N, g.order, g.cell_of, keys, order);
  PQ_HIP(hipGetLastError());
  int bits = 1;
  while (bits < 32 && (int64_t(1) << bits) < g.ncell) ++bits;
  PQ_TRY(stable_sort_pairs_u32(c, &keys, &order, n, bits));
  int32_t nnz = 0;
  PQ_TRY(fetch(c, &nnz, L.indptr + n));
  int32_t* pos_of;
  DevCsr Lp;
  double *wh_p, *wl_p, *pts_p, *x_p;
  PQ_TRY(c->arena.get(size_t(n), &pos_of));
  PQ_TRY(c->arena.get(size_t(n) + 1, &Lp.indptr));
  PQ_TRY(c->arena.get(size_t(nnz) + 1, &Lp.indices));
  PQ_TRY(c->arena.get(size_t(nnz) + 1, &Lp.vals));
  PQ_TRY(c->arena.get(size_t(n), &wh_p));
  PQ_TRY(c->arena.get(size_t(n), &wl_p));
  PQ_TRY(c->arena.get(size_t(n) * 3, &pts_p));
  PQ_TRY(c->arena.get(size_t(n) * 3, &x_p));
  hipLaunchKernelGGL(k_perm_invert, grid, block, 0, c->stream, N, order, pos_of);
  hipLaunchKernelGGL(k_perm_rowlen, grid1, block, 0, c->stream, N, order, L.indptr, Lp.indptr);
  PQ_TRY(exclusive_scan_i32(c, Lp.indptr, n + 1));
  hipLaunchKernelGGL(k_perm_fill, grid, block, 0, c->stream, N, order, pos_of, L.indptr, L.indices,
                     L.vals, Lp.indptr, Lp.indices, Lp.vals, wh, wl, pts, wh_p, wl_p, pts_p);
  PQ_HIP(hipGetLastError());
  const int rc = lbc_solve_core(c, Lp, n, wl_p, wl_edge_const, wh_p, pts_p, rtol, max_it, x_p, iters, resid);
  if (rc != 0 && rc != PYQSM_ENOCONV) return rc;
  hipLaunchKernelGGL(k_perm_back, grid, block, 0, c->stream, N, order, x_p, x);
  PQ_HIP(hipGetLastError());
  return rc;
}

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_spmv3(const int32_t* indptr, const int32_t* indices, const double* vals, int64_t n,
                const double* x, double* y, int32_t device) {
  PQ_API_RANGE("pyqsm_spmv3");
  if (n < 0) return fail(PYQSM_EINVAL, "negative size");
  if (n == 0) return 0;
  if (!indptr || !x || !y) return fail(PYQSM_EINVAL, "pyqsm_spmv3: NULL pointer");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  DevCsr L;
  int64_t nnz;
  PQ_TRY(upload_csr(c, indptr, indices, vals, n, &L, &nnz));
  double *dx, *dy;
  PQ_TRY(c->arena.get(size_t(n) * 3, &dx));
  PQ_TRY(c->arena.get(size_t(n) * 3, &dy));
  PQ_TRY(copy_in(c, dx, x, size_t(n) * 3));
  {
    ProfScope ps(c, "spmv3");
    hipLaunchKernelGGL(k_spmv3, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, int(n), L.indptr,
                       L.indices, L.vals, static_cast<const double*>(nullptr), dx, dy);
    PQ_HIP(hipGetLastError());
  }
  PQ_TRY(fetch(c, y, dy, size_t(n) * 3));
  return 0;
}

int pyqsm_lbc_solve(const int32_t* indptr, const int32_t* indices, const double* vals, int64_t n,
                    const double* wl, const double* wh, const double* pts, double rtol,
                    int32_t max_it, double* out, int32_t* iters, double* resid, int32_t device) {
  PQ_API_RANGE("pyqsm_lbc_solve");
  if (n < 0) return fail(PYQSM_EINVAL, "negative size");
  if (iters) *iters = 0;
  if (n == 0) return 0;
  if (!indptr || !wl || !wh || !pts || !out)
    return fail(PYQSM_EINVAL, "pyqsm_lbc_solve: NULL pointer");
  if (!(rtol > 0)) return fail(PYQSM_EINVAL, "rtol must be positive");
  // extract_skeleton always passes a uniform Laplacian weight (skeletonize.py:265,329,334);
  // the fast path only needs it constant along every edge of L (checked on the device below):
  // several clouds stacked into one block-diagonal system may each bring their own
  bool wl_uniform = true, wl_positive = true;
  for (int64_t i = 0; i < n; ++i) {
    if (wl[i] != wl[0]) wl_uniform = false;
    if (!(wl[i] > 0.0) || !std::isfinite(wl[i])) wl_positive = false;
  }
  for (int64_t i = 0; i < n; ++i)
    if (!(wh[i] > 0.0) || !std::isfinite(wh[i]))
      return fail(PYQSM_EINVAL, "positional weights must be positive and finite");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  DevCsr L;
  int64_t nnz;
  PQ_TRY(upload_csr(c, indptr, indices, vals, n, &L, &nnz));
  double *d_wl, *d_wh, *d_pts, *d_x;
  PQ_TRY(c->arena.get(size_t(n), &d_wl));
  PQ_TRY(c->arena.get(size_t(n), &d_wh));
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_pts));
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_x));
  PQ_TRY(copy_in(c, d_wl, wl, size_t(n)));
  PQ_TRY(copy_in(c, d_wh, wh, size_t(n)));
  PQ_TRY(copy_in(c, d_pts, pts, size_t(n) * 3));
  int32_t it = 0;
  double rs[3] = {0, 0, 0};
  bool wl_edge_const = wl_positive;
  if (wl_positive && !wl_uniform) {
    int32_t* d_flag;
    PQ_TRY(c->arena.get(1, &d_flag));
    PQ_HIP(hipMemsetAsync(d_flag, 0, 4, c->stream));
    hipLaunchKernelGGL(k_edge_const, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, int(n), L.indptr,
                       L.indices, d_wl, d_flag);
    int32_t h_flag = 0;
    PQ_TRY(fetch(c, &h_flag, d_flag));
    wl_edge_const = h_flag == 0;
  }
  int rc = lbc_solve_device(c, L, n, d_wl, wl_edge_const, d_wh, d_pts, rtol, max_it, d_x, &it, rs);
  if (iters) *iters = it;
  if (resid) {
    resid[0] = rs[0];
    resid[1] = rs[1];
    resid[2] = rs[2];
  }
  if (rc != 0 && rc != PYQSM_ENOCONV) return rc;
  PQ_TRY(fetch(c, out, d_x, size_t(n) * 3));
  return rc;
}

int pyqsm_clamp(double* pts, int64_t n, const double lo[3], const double hi[3], int32_t device) {
  PQ_API_RANGE("pyqsm_clamp");
  if (n < 0) return fail(PYQSM_EINVAL, "negative size");
  if (n == 0) return 0;
  if (!pts || !lo || !hi) return fail(PYQSM_EINVAL, "pyqsm_clamp: NULL pointer");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double* d;
  PQ_TRY(upload(c, pts, size_t(n) * 3, &d));
  {
    ProfScope ps(c, "clamp");
    hipLaunchKernelGGL(k_clamp, dim3(ceil_div(n * 3, 256)), dim3(256), 0, c->stream, n * 3, d,
                       lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
    PQ_HIP(hipGetLastError());
  }
  PQ_TRY(fetch(c, pts, d, size_t(n) * 3));
  return 0;
}

}  // extern "C"
