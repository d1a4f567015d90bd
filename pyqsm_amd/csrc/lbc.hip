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
#include <climits>

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

// ---- environment knobs ----------------------------------------------------------------------
// Every switch of this file goes through these four readers (INTEGRATION.md has the table). A
// value outside its range counts as not set. Switches that tests flip between two solves are
// read where a solve uses them; the tuning knobs sit in a function-local static and are read
// once per process, on first use.
static const char* knob_text(const char* name) { return getenv(name); }
static bool knob_set(const char* name) { return knob_text(name) != nullptr; }  // present, whatever it says
static bool knob_off(const char* name) {                                         // "0...": a default-on path off
  const char* e = knob_text(name);
  return e && e[0] == '0';
}
static int knob_int(const char* name, int lo, int hi, int dflt) {
  const char* e = knob_text(name);
  if (!e) return dflt;
  const int v = atoi(e);
  return v >= lo && v <= hi ? v : dflt;
}
// closed: [lo, hi], otherwise (lo, hi)
static double knob_real(const char* name, double lo, double hi, bool closed, double dflt) {
  const char* e = knob_text(name);
  if (!e) return dflt;
  const double v = atof(e);
  return (closed ? v >= lo && v <= hi : v > lo && v < hi) ? v : dflt;
}

// Plain launches instead of graph replays when PYQSM_NO_GRAPH is set. The library never looks
// at the profiler's environment, and the profile scripts (tools/profile_r0*.sh) keep graphs ON:
// what they measure is the shipped path. PYQSM_NO_GRAPH=1 is an explicit switch for whoever
// wants a profile of plain launches.
static bool graphs_enabled() { return !knob_set("PYQSM_NO_GRAPH"); }

// The multigrid-CG bursts are plain launches unless PYQSM_AMG_GRAPH is set: their graphs hold
// 30-150 kernel nodes, are instantiated anew for every B-solve pair and replayed ~5 times, and
// measured against plain launches they lose at every size on this ROCm (20 contractions:
// 1 M points 5.28 vs 5.07 s, 50 k 0.82 vs 0.77 s, 5 k 0.61 vs 0.55 s). They paid off for
// the round's first solver — 24-iteration bursts of four tiny kernels — which keeps them.
static bool amg_graphs_enabled() { return knob_set("PYQSM_AMG_GRAPH") && graphs_enabled(); }

// ---- bursts of CG iterations ------------------------------------------------------------------
// A burst recorded once as a hipGraph and replayed: at a few thousand points an iteration is
// four ~5 us launches, and replaying a graph costs about a third of launching them one by one.
enum class Loop { Jacobi, MultigridF64, MultigridF32 };
// What a recorded burst depends on: the operator it applies (`owner`: the weight vector of a
// Jacobi-PCG system, the hierarchy of a multigrid one — each fixes the scratch vectors too), the
// vector it updates, the loop that issued it and its length.
struct BurstKey {
  const void *owner, *x;
  Loop loop;
  int len;
  bool operator==(const BurstKey& o) const { return owner == o.owner && x == o.x && loop == o.loop && len == o.len; }
};
struct GraphCache {  // lives as long as one lbc_solve_core call
  std::vector<std::pair<BurstKey, hipGraphExec_t>> items;
  ~GraphCache() {
    for (auto& g : items) (void)hipGraphExecDestroy(g.second);
  }
};

// key.len iterations with the parities 0, 1, 0, ... (an even length, so that the next burst starts
// at parity 0 again). `iteration(par)` enqueues one iteration on c->stream and returns 0 or an
// error. With a cache the burst is a graph: captured and instantiated on first use, replayed
// from then on; without one (nullptr) it is plain launches. The capture is closed and the
// captured graph destroyed on every way out; an iteration's error is returned after that.
template <typename Iteration>
static int run_burst(Ctx* c, GraphCache* cache, const BurstKey& key, Iteration&& iteration) {
  if (!cache) {
    for (int bi = 0; bi < key.len; ++bi) PQ_TRY(iteration(bi & 1));
    return 0;
  }
  hipGraphExec_t exec = nullptr;
  for (auto& g : cache->items)
    if (g.first == key) exec = g.second;
  if (!exec) {
    PQ_HIP(hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed));
    int rc = 0;
    for (int bi = 0; bi < key.len && rc == 0; ++bi) rc = iteration(bi & 1);
    hipGraph_t graph = nullptr;
    const hipError_t ended = hipStreamEndCapture(c->stream, &graph);
    hipError_t made = hipSuccess;
    if (rc == 0 && ended == hipSuccess) made = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (graph) (void)hipGraphDestroy(graph);
    if (rc != 0) return rc;
    PQ_HIP(ended);
    PQ_HIP(made);
    cache->items.push_back({key, exec});
  }
  PQ_HIP(hipGraphLaunch(exec, c->stream));
  return 0;
}

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
  const dim3 block(256);
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
  if (!graphs_enabled()) cache = nullptr;
  const auto iteration = [&](int par) {
    launch_iteration(c, S, w, x, par);
    return 0;
  };
  while (!done && it < max_it) {
    // bursts have an even length so that each one starts at parity 0
    int burst = std::min<int>(kBurst, max_it - it);
    if (burst < kBurst) burst += burst & 1;
    {
      ProfScope ps(c, prof_name, burst);
      // only the full burst is worth a graph; the short one at the end of a budget runs once
      PQ_TRY(run_burst(c, burst == kBurst ? cache : nullptr, {S.wh, x, Loop::Jacobi, burst}, iteration));
      PQ_HIP(hipGetLastError());
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

// ---- the same kernels in fp32 ---------------------------------------------------------------
// The B-solves are asked for two digits and sit inside a flexible outer CG, so they run in
// fp32 altogether: B as the multigrid's fp32 level-0 matrix, float vectors (ld4 / st4,
// sparse.hpp), the cycle without its conversion pass; dot products are still accumulated in
// fp64. Half the bytes per sparse pass and vector update.
struct WorkF {
  float *r, *z, *dir, *q;
  Scal* sc;
};

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

// ---- CG on B y = rhs preconditioned by one multigrid V-cycle (amg.hip) -------------------------
// Same device-side scalar protocol as jacobi_pcg: an iteration is the sparse pass, the update,
// the cycle (its last kernel also accumulates r.z) and the direction update, issued as bursts of
// 8 and then 2 iterations; the host only reads |b|^2 and |r|^2 between bursts (each look costs a
// stream drain, which is what small systems are bound by). y starts at 0.
// One loop (mg_pcg) serves fp64 and fp32 vectors. What the two do differently is spelled out,
// member by member, in the policies MgF64 and MgF32, so that each difference is a decision.

// PYQSM_AMG_FIXED=m: every fp32 B-solve runs exactly m multigrid-CG iterations (experiment knob)
static int amg_fixed_iterations() {
  static const int v = knob_int("PYQSM_AMG_FIXED", 0, INT_MAX, 0);
  return v;
}
static constexpr int kAmgFirstBurst = 8;  // a 1e-2 solve takes 10-14 iterations: no look before 8
static constexpr int kAmgBurst = 2;       // then a residual check every 2
static int amg_next_burst() {  // PYQSM_AMG_BURST: iterations between two looks after the first (even, 2-16)
  static const int v = knob_int("PYQSM_AMG_BURST", 2, 16, kAmgBurst) & ~1;
  return v;
}
static int amg_first_burst() {  // PYQSM_AMG_FIRST_BURST (even, 2-64)
  static const int v = knob_int("PYQSM_AMG_FIRST_BURST", 2, 64, kAmgFirstBurst) & ~1;
  return v;
}
// PYQSM_REDUCE_BLOCKS: grid cap of the reducing kernels of the fp32 loop below kPart (tuning knob)
static unsigned reduce_grid_f(int64_t n) {
  static const int cap = std::min(knob_int("PYQSM_REDUCE_BLOCKS", 1, INT_MAX, kPart), kPart);
  return std::min<unsigned>(reduce_grid(n), unsigned(cap));
}

// fp64: vectors [n,3], B = wl L + wh applied from the Laplacian (the Newton systems of the Riccati
// weights, which bring their own wh, and rung 1 of the ladder).
struct MgF64 {
  using Vec = double;
  static constexpr int kStride = 3;  // values per row of a vector
  static constexpr Loop kLoop = Loop::MultigridF64;
  static constexpr const char* kName = "multigrid CG";  // in the failure messages
  static constexpr bool kFixedMode = false;       // PYQSM_AMG_FIXED is an experiment on the default path only
  static constexpr bool kStopsDiverging = false;  // left to the ladder (BSolve::diverged), which asks for less: > 1
  const System& S;
  const Work& w;  // r, z, dir, q, sc: the names mg_pcg uses
  static unsigned reduce_blocks(int n) { return reduce_grid(n); }
  void rhs_norm(Ctx* c, dim3 rgrid, int n, const Vec* rhs) const {
    hipLaunchKernelGGL(k_dot3, rgrid, dim3(256), 0, c->stream, n, rhs, rhs, w.sc->bb);
  }
  int cycle(Ctx* c, AmgHierarchy* H, double* dot) const { return amg_vcycle(c, H, w.r, w.z, dot); }
  void keep_first_rz(Ctx*) const {}  // k_update_r and k_direction add the partials up themselves
  void sparse_pass(Ctx* c, dim3 rgrid, int n, int par) const {
    hipLaunchKernelGGL(k_spmv3_tail<OP_B>, rgrid, dim3(256), 0, c->stream, n, S.L.indptr, S.L.indices,
                       S.L.vals, w.dir, S.wl, S.wh, w.dir, w.q, w.sc, par);
  }
  void update(Ctx* c, dim3 rgrid, int n, Vec* y, int par) const {
    hipLaunchKernelGGL(k_update_r, rgrid, dim3(256), 0, c->stream, n, w.dir, w.q, y, w.r, w.sc, par);
  }
  void direction(Ctx* c, int n, int par) const {  // a thread per row: the full grid
    hipLaunchKernelGGL(k_direction, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, n, w.z, w.dir, w.sc, par);
  }
};

// fp32: vectors of kVecStride floats per row, B as the hierarchy's fp32 level-0 matrix (rung 0).
struct MgF32 {
  using Vec = float;
  static constexpr int kStride = kVecStride;
  static constexpr Loop kLoop = Loop::MultigridF32;
  static constexpr const char* kName = "multigrid CG (fp32)";
  static constexpr bool kFixedMode = true;
  // CG on an SPD system does not leave the residual ten times above the right-hand side for
  // long: an fp32 solve that does is diverging (BSolve::apply), no point in going to max_it
  static constexpr bool kStopsDiverging = true;
  const WorkF& w;  // r, z, dir, q, sc
  const int32_t *ip, *ix;
  const float* bv;
  MgF32(const WorkF& work, const AmgHierarchy* H) : w(work) { amg_fine_matrix(H, &ip, &ix, &bv); }
  static unsigned reduce_blocks(int n) { return reduce_grid_f(n); }  // every kernel of this loop strides by its grid
  void rhs_norm(Ctx* c, dim3 rgrid, int n, const Vec* rhs) const {
    hipLaunchKernelGGL(k_dot3_f, rgrid, dim3(256), 0, c->stream, n, rhs, w.sc->bb);
  }
  int cycle(Ctx* c, AmgHierarchy* H, double* dot) const { return amg_vcycle_f32(c, H, w.r, w.z, dot); }
  void keep_first_rz(Ctx* c) const {  // rz_tot[0]: the totals k_update_r_f and k_direction_f read
    hipLaunchKernelGGL(k_part_final, dim3(1), dim3(256), 0, c->stream, w.sc->rz[0], w.sc->rz_tot[0]);
  }
  void sparse_pass(Ctx* c, dim3 rgrid, int n, int par) const {
    ProfScope pk(c, "k_bspmv_f", 1, 2);
    hipLaunchKernelGGL(k_bspmv_f, rgrid, dim3(256), 0, c->stream, n, ip, ix, bv, w.dir, w.q, w.sc, par);
  }
  void update(Ctx* c, dim3 rgrid, int n, Vec* y, int par) const {
    hipLaunchKernelGGL(k_update_r_f, rgrid, dim3(256), 0, c->stream, n, w.dir, w.q, y, w.r, w.sc, par);
  }
  void direction(Ctx* c, int n, int par) const {  // strides by its grid: the capped one
    hipLaunchKernelGGL(k_direction_f, dim3(reduce_grid_f(n)), dim3(256), 0, c->stream, n, w.z, w.dir, w.sc, par);
  }
};

static double max3(const double v[3]) { return std::max(v[0], std::max(v[1], v[2])); }

// y = B^-1 rhs to rtol; y starts at 0. Returns 0, PYQSM_ENOCONV (y is what the loop reached) or an error.
template <typename P>
static int mg_pcg(Ctx* c, int N, const P& p, AmgHierarchy* H, const typename P::Vec* rhs,
                  typename P::Vec* y, double rtol, int32_t max_it, GraphCache* cache, int32_t* iters,
                  double resid[3]) {
  const size_t bytes = size_t(N) * P::kStride * sizeof(typename P::Vec);
  Scal* sc = p.w.sc;
  PQ_HIP(hipMemsetAsync(sc, 0, sizeof(Scal), c->stream));
  PQ_HIP(hipMemsetAsync(y, 0, bytes, c->stream));
  PQ_HIP(hipMemcpyAsync(p.w.r, rhs, bytes, hipMemcpyDeviceToDevice, c->stream));
  const dim3 rgrid(P::reduce_blocks(N));  // kernels that end in a reduction
  p.rhs_norm(c, rgrid, N, rhs);
  PQ_TRY(p.cycle(c, H, sc->rz[0]));
  p.keep_first_rz(c);
  PQ_HIP(hipMemcpyAsync(p.w.dir, p.w.z, bytes, hipMemcpyDeviceToDevice, c->stream));
  for (int k = 0; k < 3; ++k) resid[k] = 1.0;
  *iters = 0;
  const auto iteration = [&](int par) -> int {
    p.sparse_pass(c, rgrid, N, par);
    p.update(c, rgrid, N, y, par);
    PQ_TRY(p.cycle(c, H, sc->rz[par ^ 1]));
    p.direction(c, N, par);
    return 0;
  };
  if (!amg_graphs_enabled()) cache = nullptr;
  const auto burst = [&](int len) -> int {
    ProfScope ps(c, "lbc_amg_iter", len);
    return run_burst(c, cache, {H, y, P::kLoop, len}, iteration);
  };
  if (P::kFixedMode) {
    if (const int fixed = amg_fixed_iterations()) {
      // a fixed, even number of iterations and no look at the residual: no host round trip in
      // the whole B-solve (the outer CG is flexible, an inexact B^-1 costs it a few steps)
      const int len = std::min<int>((fixed + 1) & ~1, std::max(2, max_it & ~1));
      PQ_TRY(burst(len));
      PQ_HIP(hipGetLastError());
      *iters = len;
      for (int k = 0; k < 3; ++k) resid[k] = 0.0;
      return 0;
    }
  }
  int it = 0;
  bool done = false;
  while (!done && it < max_it) {
    int len = it == 0 ? amg_first_burst() : amg_next_burst();
    if (len > max_it - it) len = std::max(2, (max_it - it + 1) & ~1);  // even: bursts start at parity 0
    PQ_TRY(burst(len));
    it += len;
    *iters = it;
    double h[2][3];
    {
      const double* parts[2] = {sc->rr[1], sc->bb};
      PQ_TRY(part_totals_host(c, parts, 2, h));
    }
    const double* rr = h[0];
    const double* bb = h[1];
    if (bb[0] == 0.0 && bb[1] == 0.0 && bb[2] == 0.0) {  // zero right-hand side: y = 0
      for (int k = 0; k < 3; ++k) resid[k] = 0.0;
      return 0;
    }
    done = true;
    for (int k = 0; k < 3; ++k) {
      resid[k] = bb[k] > 0 ? std::sqrt(rr[k] / bb[k]) : 0.0;
      if (!(resid[k] <= rtol)) done = false;
      if (!std::isfinite(resid[k])) return fail(PYQSM_ENOCONV, "%s broke down after %d iterations", P::kName, it);
    }
    if (P::kStopsDiverging && !done && it >= 16 && max3(resid) > 10.0)
      return fail(PYQSM_ENOCONV, "%s is diverging after %d iterations, residual %.3e", P::kName, it, max3(resid));
  }
  PQ_HIP(hipGetLastError());
  return done ? 0 : fail(PYQSM_ENOCONV, "%s reached %d iterations, residual %.3e", P::kName, it, max3(resid));
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
static int riccati_mode() { return knob_int("PYQSM_RICCATI", INT_MIN, INT_MAX, 1); }
static double riccati_tol() {  // PYQSM_RICCATI_TOL: tuning knob for kRiccatiTol
  static const double v = knob_real("PYQSM_RICCATI_TOL", 0.0, 1.0, false, kRiccatiTol);
  return v;
}
static double riccati_frac() {  // PYQSM_RICCATI_FRAC: tuning knob for kRiccatiFrac
  static const double v = knob_real("PYQSM_RICCATI_FRAC", 0.0, 1.0, true, kRiccatiFrac);
  return v;
}
static int riccati_stall() {  // PYQSM_RICCATI_STALL: tuning knob for kRiccatiStall
  static const int v = knob_int("PYQSM_RICCATI_STALL", 1, INT_MAX, kRiccatiStall);
  return v;
}

// ---- the device-resident contraction solve ---------------------------------------------------
// Uniform Laplacian weight c (what extract_skeleton always passes): the system
// A = c^2 L^2 + W_H^2 is preconditioned by B^2 with B = c L + W_H, which is
// symmetric positive definite and spectrally within a small factor of A
// ((c l + h)^2 / (c^2 l^2 + h^2) lies in [1, 2] for every eigenvalue l >= 0 when
// W_H = h I). cond(B) ~ sqrt(cond(A)), so the outer flexible CG (OuterFcg) needs a few dozen
// steps and each step two solves with B (BSolve). cond(A) reaches 1e13 on
// contracted clouds: far beyond what Jacobi-PCG on A itself can do.
// Non-uniform wl: plain Jacobi-PCG on A.

// What the pieces of one lbc_solve_core call share.
struct Solve {
  Ctx* c;
  DevCsr L;
  int N;
  const double *wl, *wh;
  int32_t max_it;           // caps the total number of inner (sparse-pass) iterations
  int32_t total_inner = 0;  // ... spent so far, by every B-solve and Newton solve
  bool trace = false;       // PYQSM_LBC_TRACE
  double *b, *d_tmp;
  double* d_parts[5];  // the outer iteration's dot products of one step: launched one after the other, read in ONE look
  System SA;           // A, and its scratch
  Work wa;
  GraphCache cache;
  dim3 grid() const { return dim3(ceil_div(N, 256)); }  // a thread per row
  size_t bytes() const { return size_t(N) * 24; }       // of an [n,3] vector
};

struct AmgGuard {
  AmgHierarchy* h;
  ~AmgGuard() { amg_destroy(h); }
};

// The multigrid hierarchy of B = wl L + wh; null when none can be built (tiny or fully decoupled
// systems).
static AmgHierarchy* build_hierarchy(Solve& s, const double* wh) {
  ProfScope ps(s.c, "lbc_amg_build");
  AmgHierarchy* h = nullptr;
  if (amg_build(s.c, s.L, s.N, s.wl, wh, &h) != 0 || amg_levels(h) < 2) {
    amg_destroy(h);
    h = nullptr;
  }
  return h;
}

// out = B^-1 B^-1 rhs, the preconditioner of the outer iteration, as a ladder of three rungs.
// B-solves that break down: the fp32 multigrid CG loses its digits on the collapsed clouds of
// late contractions — cot weights of degenerate triangles put c L_ii at 1e12 where W_H is 1e3,
// below fp32's resolution of a row, and B^-1 r (the right-hand side of the second solve) is
// dominated by smooth modes whose residual fp32 cannot evaluate. Seen: one solve of a perturbed
// 20-contraction run spent 11 000 iterations feeding garbage to the outer iteration; a system
// with 30x the usual W_L took 1 753 iterations where the fp64 operator takes 376. An fp32 solve
// that diverges (MgF32::kStopsDiverging: mg_pcg returns after 16 iterations) or needs more than
// kF32MaxIt iterations is therefore repeated one rung down — fp64 operator with the same cycle —
// and the solve stays there; an fp64 solve that DIVERGES goes on to Jacobi-PCG.
// Invariant of every rung's verdict: an exhausted budget (total_inner >= max_it) is never a
// reason to step down, so it is not spent again. (CG's residual is not monotone: a solve cut
// short by the caller's max_it after a few iterations may stand above 1 without diverging.)
struct BSolve {
  Solve& s;
  System SB;          // B with the weights of the current phase
  Work wb;
  AmgHierarchy* amg;  // of the current phase; null: Jacobi-PCG only
  double* y;          // B^-1 rhs, between the two solves
  double inner_rtol;
  bool use_f32;
  WorkF wf;
  float *f_rhs, *f_y, *f_out;
  int rung = 0;  // 0: fp32 multigrid CG, 1: fp64 operator, 2: Jacobi-PCG

  void use(AmgHierarchy* h, const double* wh) {  // the preconditioner's weights: W~ (phase 1) or W_H
    amg = h;
    SB.wh = wh;
  }
  int32_t budget() const { return std::max<int32_t>(1, std::min<int32_t>(kInnerMaxIt, s.max_it - s.total_inner)); }
  bool exhausted() const { return s.total_inner >= s.max_it; }
  bool diverged(int rc, int32_t its, const double rs[3]) const {
    if (rc == 0 || exhausted()) return false;
    const double w = max3(rs);
    return !std::isfinite(w) || (its >= 16 && w > 1.0);
  }

  // One rung: two runs of solve(rhs, x, &its, rs), rhs -> mid -> out, each booked on the budget.
  // *gave_up: gives_up(rc, its, rs) held for one of them (a first one's keeps the second from running).
  template <typename V, typename SolveFn, typename Verdict>
  int twice(SolveFn&& solve, Verdict&& gives_up, const V* rhs, V* mid, V* out, int32_t its[2], double rs[3],
            bool* gave_up) {
    const V* from[2] = {rhs, mid};
    V* to[2] = {mid, out};
    its[0] = its[1] = 0;
    *gave_up = false;
    for (int k = 0; k < 2 && !*gave_up; ++k) {
      const int rc = solve(from[k], to[k], &its[k], rs);
      if (rc != 0 && rc != PYQSM_ENOCONV) return rc;
      s.total_inner += its[k];
      *gave_up = gives_up(rc, its[k], rs);
    }
    return 0;
  }

  int apply(const double* rhs, double* out) {
    Ctx* c = s.c;
    const int N = s.N;
    int32_t its[2];
    double rs[3];
    bool gave_up = false;
    if (amg && use_f32 && rung == 0) {
      hipLaunchKernelGGL(k_cvt_d2f, s.grid(), dim3(256), 0, c->stream, N, rhs, f_rhs);
      const MgF32 p(wf, amg);
      PQ_TRY(twice([&](const float* b, float* x, int32_t* it, double* r) {
                     return mg_pcg(c, N, p, amg, b, x, inner_rtol, std::min(budget(), kF32MaxIt), &s.cache, it, r);
                   },
                   [&](int rc, int32_t, const double*) { return rc != 0 && !exhausted(); },  // fp32: stalling counts as well
                   f_rhs, f_y, f_out, its, rs, &gave_up));
      if (!gave_up) {
        hipLaunchKernelGGL(k_cvt_f2d, s.grid(), dim3(256), 0, c->stream, N, f_out, out);
        return 0;
      }
      rung = 1;
      if (s.trace)
        fprintf(stderr, "  fp32 B-solve gave up after %d + %d iterations (%.3e %.3e %.3e): fp64 operator from here\n",
                its[0], its[1], rs[0], rs[1], rs[2]);
    }
    if (amg && rung <= 1) {
      const MgF64 p{SB, wb};
      PQ_TRY(twice([&](const double* b, double* x, int32_t* it, double* r) {
                     return mg_pcg(c, N, p, amg, b, x, inner_rtol, std::min(budget(), kAmgMaxIt), &s.cache, it, r);
                   },
                   [&](int rc, int32_t n_it, const double* r) { return diverged(rc, n_it, r); }, rhs, y, out, its, rs,
                   &gave_up));
      if (!gave_up) return 0;
      rung = 2;
      if (s.trace)
        fprintf(stderr, "  multigrid B-solve diverged after %d + %d iterations (%.3e %.3e %.3e): Jacobi-PCG from here\n",
                its[0], its[1], rs[0], rs[1], rs[2]);
    }
    return twice([&](const double* b, double* x, int32_t* it, double* r) {
                   return jacobi_pcg(c, SB, wb, b, x, true, inner_rtol, budget(), "lbc_inner_iter", &s.cache, it, r);
                 },
                 [](int, int32_t, const double*) { return false; },  // the last rung: what it reaches is what there is
                 rhs, y, out, its, rs, &gave_up);
  }
};

// ---- Riccati weights for B (k_riccati_f) ---------------------------------------------------------
// Newton's method on the weights, each step a multigrid-CG solve with B's hierarchy, and the
// hierarchy of (c L + W~) when the steps were worth taking. *wt and *amg_r stay null when the plain
// preconditioner is to be used: W_H smooth enough (mode 1), Newton gone wrong, the caller's
// iteration budget too tight, or no second hierarchy.
static int riccati_weights(Solve& s, BSolve& B, int mode, const double** wt_out, AmgHierarchy** amg_r) {
  Ctx* c = s.c;
  const int N = s.N;
  const DevCsr& L = s.L;
  const dim3 grid = s.grid(), block(256);
  ProfScope psr(c, "lbc_riccati");
  double *wt, *wj, *negf, *w2, *delta;
  PQ_TRY(c->arena.get(size_t(N), &wt));
  PQ_TRY(c->arena.get(size_t(N), &wj));
  PQ_TRY(c->arena.get(size_t(N) * 3, &negf));
  PQ_TRY(c->arena.get(size_t(N) * 3, &w2));
  PQ_TRY(c->arena.get(size_t(N) * 3, &delta));
  PQ_HIP(hipMemcpyAsync(wt, s.wh, size_t(N) * 8, hipMemcpyDeviceToDevice, c->stream));
  hipLaunchKernelGGL(k_scale2, grid, block, 0, c->stream, N, s.wh, wj);
  double wnorm = 0.0;
  const double ric_tol = riccati_tol(), frac_min = riccati_frac();
  int steps = 0;
  for (int k = 0; k <= kRiccatiMaxIt; ++k) {
    hipLaunchKernelGGL(k_riccati_f, grid, block, 0, c->stream, N, L.indptr, L.indices, L.vals, s.wl, wt, s.wh,
                       negf, w2, k == 0 ? 1 : 0);
    PQ_HIP(hipGetLastError());
    double ff[3], ww[3];
    PQ_TRY(dot3_host(c, N, negf, negf, s.d_tmp, ff));
    if (k == 0) {
      PQ_TRY(dot3_host(c, N, w2, w2, s.d_tmp, ww));
      wnorm = ww[0];
    }
    const double rel = wnorm > 0 ? std::sqrt(ff[0] / wnorm) : 0.0;
    if (s.trace)
      fprintf(stderr, "riccati %d: |F|/|w^2| = %.3e%s\n", k, rel,
              k == 0 ? (" cancelled fraction " + std::to_string(ff[1] / double(N))).c_str() : "");
    // Newton gone wrong (it never did on the clouds tried): the plain preconditioner is always valid
    if (!std::isfinite(rel) || (k == kRiccatiMaxIt && rel > 10.0 * ric_tol)) {
      steps = 0;
      break;
    }
    // uniform W_H solves the equation itself (the first two contractions): rel = 0 at k = 0
    if (rel <= ric_tol || k == kRiccatiMaxIt) break;
    if (k == 0) {
      if (mode == 1 && ff[1] < frac_min * double(N)) break;  // W_H smooth enough for plain B
      hipLaunchKernelGGL(k_riccati_f, grid, block, 0, c->stream, N, L.indptr, L.indices, L.vals, s.wl, wt,
                         s.wh, negf, w2, 0);  // the same F as a right-hand side
    }
    if (s.max_it - s.total_inner < 4 * kRiccatiInnerMaxIt) {  // not on a caller's tight iteration budget
      steps = 0;
      break;
    }
    const System SJ{L, N, OP_B, s.wl, wj, B.SB.minv};  // the Jacobian c L + 2 W~
    int32_t itj = 0;
    double rsj[3];
    const int rcj = mg_pcg(c, N, MgF64{SJ, B.wb}, B.amg, negf, delta, kRiccatiInnerRtol, kRiccatiInnerMaxIt,
                           &s.cache, &itj, rsj);
    if (rcj != 0 && rcj != PYQSM_ENOCONV) return rcj;
    s.total_inner += itj;
    hipLaunchKernelGGL(k_riccati_step, grid, block, 0, c->stream, N, delta, wt, wj);
    ++steps;
  }
  if (steps > 0 && (*amg_r = build_hierarchy(s, wt)) != nullptr) *wt_out = wt;
  return 0;
}

// ---- the outer iteration: flexible CG on A x = b preconditioned by BSolve ----------------------
// Convergence is judged on z = B^-2 r: B^-2 A has its spectrum in [1/2, 1] for uniform
// W_H (a modest interval otherwise), so |z| / |x| estimates the relative ERROR of x, which
// is what the caller's 1e-5 position tolerance is about. The true residual |r| / |b| is
// tracked as well (and reported), but with cond(A) up to 1e10 it is neither monotone
// under CG nor a usable measure of the error.
struct OuterFcg {
  Solve& s;
  BSolve& B;
  double rtol;
  double* x;
  double *r, *z, *z_old, *dir, *q, *x_best;
  double bb[3], rr[3], rz[3];
  double cur_res[3], best_res[3];  // |r| / |b| of x and of x_best
  double best = HUGE_VAL;          // error estimate of x_best
  int outer = 0, best_outer = 0;
  bool done = false;

  double rel(const double v[3], double out[3]) const {
    for (int k = 0; k < 3; ++k) out[k] = bb[k] > 0 ? std::sqrt(v[k] / bb[k]) : 0.0;
    return max3(out);
  }
  void dot_launch(const double* a, const double* bvec, double* part) const {
    hipLaunchKernelGGL(k_dot3, dim3(reduce_grid(s.N)), dim3(256), 0, s.c->stream, s.N, a, bvec, part);
  }
  void residual() {  // r = b - A x
    apply_op(s.c, s.SA, s.wa, x, q, nullptr);
    hipLaunchKernelGGL(k_sub3, s.grid(), dim3(256), 0, s.c->stream, s.N, s.b, q, r);
  }
  // r = b - A x0 and what the first estimate is compared with
  int start() {
    residual();
    PQ_TRY(dot3_host(s.c, s.N, s.b, s.b, s.d_tmp, bb));
    PQ_TRY(dot3_host(s.c, s.N, r, r, s.d_tmp, rr));
    rel(rr, cur_res);
    for (int k = 0; k < 3; ++k) best_res[k] = cur_res[k];
    PQ_HIP(hipMemcpyAsync(x_best, x, s.bytes(), hipMemcpyDeviceToDevice, s.c->stream));
    done = max3(cur_res) <= rtol;
    return 0;
  }
  // after every preconditioner application: the error estimate of the current x; keeps the best x
  int judge(const double zz[3], const double xx[3], bool* finite) {
    double est = 0.0;
    for (int k = 0; k < 3; ++k) est = std::max(est, xx[k] > 0 ? std::sqrt(zz[k] / xx[k]) : 0.0);
    if (s.trace)
      fprintf(stderr, "lbc outer %d inner %d resid %.3e est %.3e\n", outer, s.total_inner, max3(cur_res), est);
    *finite = std::isfinite(est);
    if (!*finite) return 0;
    if (est < best) {
      best = est;
      best_outer = outer;
      for (int k = 0; k < 3; ++k) best_res[k] = cur_res[k];
      PQ_HIP(hipMemcpyAsync(x_best, x, s.bytes(), hipMemcpyDeviceToDevice, s.c->stream));
    }
    if (est <= rtol) done = true;
    return 0;
  }
  // (re)start of the CG with the current preconditioner: z = M^-1 r, dir = z
  int restart() {
    PQ_TRY(B.apply(r, z));
    PQ_HIP(hipMemcpyAsync(dir, z, s.bytes(), hipMemcpyDeviceToDevice, s.c->stream));
    dot_launch(r, z, s.d_parts[0]);
    dot_launch(z, z, s.d_parts[1]);
    dot_launch(x, x, s.d_parts[2]);
    PQ_HIP(hipGetLastError());
    double t[3][3];
    PQ_TRY(part_totals_host(s.c, s.d_parts, 3, t));
    for (int k = 0; k < 3; ++k) rz[k] = t[0][k];
    bool finite;
    PQ_TRY(judge(t[1], t[2], &finite));
    if (!finite) return fail(PYQSM_EHIP, "contraction solve: non-finite preconditioned residual");
    return 0;
  }
  // the second phase: from the best iterate, its estimate forgotten
  int reroot() {
    PQ_HIP(hipMemcpyAsync(x, x_best, s.bytes(), hipMemcpyDeviceToDevice, s.c->stream));
    residual();
    PQ_TRY(dot3_host(s.c, s.N, r, r, s.d_tmp, rr));
    rel(rr, cur_res);
    done = false;
    best = HUGE_VAL;
    best_outer = outer;
    return restart();
  }
  // Steps until the estimate meets rtol, stalls, breaks down, or a budget ends.
  int run(bool riccati_phase) {
    Ctx* c = s.c;
    const int N = s.N;
    const dim3 grid = s.grid(), block(256);
    while (!done && outer < kOuterMaxIt && s.total_inner < s.max_it) {
      ProfScope ps(c, "lbc_outer_iter");
      apply_op(c, s.SA, s.wa, dir, q, nullptr);
      double pq[3];
      PQ_TRY(dot3_host(c, N, dir, q, s.d_tmp, pq));
      S3 alpha, nalpha;
      for (int k = 0; k < 3; ++k) {
        alpha.v[k] = pq[k] != 0.0 ? rz[k] / pq[k] : 0.0;
        nalpha.v[k] = -alpha.v[k];
      }
      hipLaunchKernelGGL(k_axpy3, grid, block, 0, c->stream, N, alpha, dir, x);
      hipLaunchKernelGGL(k_axpy3, grid, block, 0, c->stream, N, nalpha, q, r);
      ++outer;
      PQ_HIP(hipMemcpyAsync(z_old, z, s.bytes(), hipMemcpyDeviceToDevice, c->stream));
      PQ_TRY(B.apply(r, z));
      // the five dot products of the step in one look (each look is a round trip; they used to be
      // five, plus the one for alpha above: 0.2 ms per outer step). |r|^2 is only needed for the
      // report and the breakdown test, so it waits for the others.
      dot_launch(r, r, s.d_parts[0]);
      dot_launch(z, z, s.d_parts[1]);
      dot_launch(x, x, s.d_parts[2]);
      dot_launch(r, z, s.d_parts[3]);
      dot_launch(r, z_old, s.d_parts[4]);
      PQ_HIP(hipGetLastError());
      double t5[5][3];
      PQ_TRY(part_totals_host(c, s.d_parts, 5, t5));
      for (int k = 0; k < 3; ++k) rr[k] = t5[0][k];
      if (!std::isfinite(rel(rr, cur_res))) break;
      bool finite;
      PQ_TRY(judge(t5[1], t5[2], &finite));
      if (!finite || done) break;
      // attainable accuracy reached. Phase 1 leaves much sooner: its estimate flattens once what is
      // left sits in the modes the Riccati weights over-weight (measured: 1.7e-8 after 23 steps, no
      // better after 35), and those are the plain preconditioner's to finish.
      const int ric_stall = riccati_stall();
      if (outer - best_outer >= (riccati_phase ? ric_stall : kOuterStall)) break;
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
    return 0;
  }
  // the best iterate and its figures to the caller
  int finish(int32_t* iters, double resid[3]) {
    PQ_HIP(hipGetLastError());
    *iters = s.total_inner + outer;
    PQ_HIP(hipMemcpyAsync(x, x_best, s.bytes(), hipMemcpyDeviceToDevice, s.c->stream));
    for (int k = 0; k < 3; ++k) resid[k] = best_res[k];
    if (!done)
      return fail(PYQSM_ENOCONV,
                  "contraction solve stopped after %d outer / %d inner iterations; best error "
                  "estimate %.3e", outer, s.total_inner, best);
    return 0;
  }
};

// The B^2-preconditioned solve: buffers, hierarchies, Riccati weights, then the outer iteration in
// one or two phases.
// Two phases when the Riccati weights are in use (see k_riccati_f): phase 1 with
// (c L + W~)^-2, whose spectrum has no upper tail; its error estimate |z| / |x| UNDER-weights the
// few modes in which the lifted weights make B~^2 >> A (eigenvalues down to 0.03 measured), so
// when it reports convergence the iteration is restarted with the plain B^-2 — whose estimate
// is the one the tolerance was calibrated on (spectrum >= 1/2) — and runs until that one agrees.
static int solve_preconditioned(Solve& s, double rtol, double* x, int32_t* iters, double resid[3]) {
  Ctx* c = s.c;
  const size_t n = size_t(s.N);
  BSolve B{s};
  OuterFcg O{s, B, rtol, x};
  double* minv_b;
  PQ_TRY(c->arena.get(n, &minv_b));
  PQ_TRY(c->arena.get(n * 3, &O.r));
  PQ_TRY(c->arena.get(n * 3, &O.z));
  PQ_TRY(c->arena.get(n * 3, &O.z_old));
  PQ_TRY(c->arena.get(n * 3, &O.dir));
  PQ_TRY(c->arena.get(n * 3, &O.q));
  PQ_TRY(c->arena.get(n * 3, &B.y));
  PQ_TRY(c->arena.get(n * 3, &O.x_best));
  PQ_TRY(alloc_work(c, s.N, &B.wb));
  hipLaunchKernelGGL(k_diag_b, s.grid(), dim3(256), 0, c->stream, s.N, s.L.indptr, s.L.indices, s.L.vals,
                     s.wl, s.wh, minv_b);
  B.SB = System{s.L, s.N, OP_B, s.wl, s.wh, minv_b};
  // Multilevel preconditioner for the B-solves (amg.hip): 12-17 cycles per solve where
  // Jacobi-PCG needs 200-700 sparse passes. PYQSM_AMG=0 selects Jacobi-PCG; it is also
  // the fallback when no hierarchy can be built.
  AmgHierarchy* const amg_b = knob_off("PYQSM_AMG") ? nullptr : build_hierarchy(s, s.wh);
  AmgGuard guard_b{amg_b};
  B.amg = amg_b;
  B.inner_rtol = knob_real("PYQSM_INNER_RTOL", 0.0, 1.0, false, kInnerRtolDefault);  // tuning knob
  // fp32 B-solves when they are asked for no more than four digits (the default asks for two);
  // PYQSM_LBC_F32=0 keeps them in fp64
  B.use_f32 = amg_b && B.inner_rtol >= 1e-4 && !knob_off("PYQSM_LBC_F32");
  B.wf = WorkF{nullptr, nullptr, nullptr, nullptr, nullptr};
  B.f_rhs = B.f_y = B.f_out = nullptr;
  if (B.use_f32) {
    PQ_TRY(c->arena.get(n * kVecStride, &B.wf.r));
    PQ_TRY(c->arena.get(n * kVecStride, &B.wf.z));
    PQ_TRY(c->arena.get(n * kVecStride, &B.wf.dir));
    PQ_TRY(c->arena.get(n * kVecStride, &B.wf.q));
    PQ_TRY(c->arena.get(n * kVecStride, &B.f_rhs));
    PQ_TRY(c->arena.get(n * kVecStride, &B.f_y));
    PQ_TRY(c->arena.get(n * kVecStride, &B.f_out));
    B.wf.sc = B.wb.sc;
  }
  s.trace = knob_set("PYQSM_LBC_TRACE");
  const double* wt = nullptr;
  AmgHierarchy* amg_r = nullptr;
  if (amg_b) {
    const int mode = riccati_mode();
    if (mode != 0) PQ_TRY(riccati_weights(s, B, mode, &wt, &amg_r));
  }
  AmgGuard guard_r{amg_r};
  const bool two_phases = amg_r != nullptr;
  if (two_phases) B.use(amg_r, wt);
  PQ_TRY(O.start());
  if (!O.done) {
    ProfScope ps0(c, "lbc_first_precond");
    PQ_TRY(O.restart());
  }
  PQ_TRY(O.run(two_phases));
  if (two_phases && O.outer < kOuterMaxIt && s.total_inner < s.max_it) {
    // converged (or stalled) by the Riccati-preconditioned estimate: go on with the plain B^-2
    // from the best iterate, until ITS estimate agrees
    B.use(amg_b, s.wh);
    if (s.trace) fprintf(stderr, "lbc outer %d: phase 2 (plain B)\n", O.outer);
    PQ_TRY(O.reroot());
    PQ_TRY(O.run(false));
  }
  return O.finish(iters, resid);
}

static int lbc_solve_core(Ctx* c, const DevCsr& L, int64_t n, const double* wl, bool wl_edge_const,
                          const double* wh, const double* pts, double rtol, int32_t max_it, double* x,
                          int32_t* iters, double resid[3]) {
  Solve s;
  s.c = c;
  s.L = L;
  s.N = int(n);
  s.wl = wl;
  s.wh = wh;
  s.max_it = max_it;
  double* minv_a;
  PQ_TRY(c->arena.get(size_t(n) * 3, &s.b));
  PQ_TRY(c->arena.get(size_t(n), &minv_a));
  PQ_TRY(c->arena.get(size_t(3) * kPart, &s.d_tmp));
  for (int a = 0; a < 5; ++a) PQ_TRY(c->arena.get(size_t(3) * kPart, &s.d_parts[a]));
  hipLaunchKernelGGL(k_rhs, s.grid(), dim3(256), 0, c->stream, s.N, wh, pts, s.b);
  PQ_HIP(hipMemcpyAsync(x, pts, s.bytes(), hipMemcpyDeviceToDevice, c->stream));
  PQ_TRY(alloc_work(c, n, &s.wa));
  s.SA = System{L, s.N, OP_A, wl, wh, minv_a};
  if (!wl_edge_const) {
    hipLaunchKernelGGL(k_diag, s.grid(), dim3(256), 0, c->stream, s.N, L.indptr, L.vals, wl, wh, minv_a);
    return jacobi_pcg(c, s.SA, s.wa, s.b, x, false, rtol, max_it, "lbc_cg_iter", &s.cache, iters, resid);
  }
  return solve_preconditioned(s, rtol, x, iters, resid);
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
  if (!wl_edge_const || n < 4096 || knob_off("PYQSM_LBC_SORT"))
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

int pyqsm_amg_probe(const int32_t* indptr, const int32_t* indices, const double* vals, int64_t n,
                    const double* cw, const double* wh, const double* rhs, int64_t m, int64_t* meta,
                    int32_t* ibuf, int64_t icap, double* dbuf, int64_t dcap, float* fbuf, int64_t fcap,
                    double* x64, float* x32, double* dots, int32_t device) {
  PQ_API_RANGE("pyqsm_amg_probe");
  if (n <= 0 || m < 0) return fail(PYQSM_EINVAL, "pyqsm_amg_probe: empty system or negative count");
  if (!indptr || !indices || !vals || !cw || !wh || !meta)
    return fail(PYQSM_EINVAL, "pyqsm_amg_probe: NULL pointer");
  if (m > 0 && (!rhs || !x64 || !x32 || !dots)) return fail(PYQSM_EINVAL, "pyqsm_amg_probe: NULL pointer");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  DevCsr L;
  int64_t nnz;
  PQ_TRY(upload_csr(c, indptr, indices, vals, n, &L, &nnz));
  double *d_cw, *d_wh;
  PQ_TRY(upload(c, cw, size_t(n), &d_cw));
  PQ_TRY(upload(c, wh, size_t(n), &d_wh));
  AmgHierarchy* h = nullptr;
  PQ_TRY(amg_build(c, L, int(n), d_cw, d_wh, &h));  // as build_hierarchy does
  AmgGuard guard{h};
  PQ_TRY(amg_readout(c, h, meta, ibuf, icap, dbuf, dcap, fbuf, fcap));
  // a single level is no hierarchy (build_hierarchy refuses it: the cycle has no level-0 xb), and a
  // caller whose buffers were too small comes again
  if (amg_levels(h) < 2 || meta[7] == 0 || m == 0) return 0;
  double *d_b, *d_x, *d_dot;
  float *d_bf, *d_xf;
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_b));
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_x));
  PQ_TRY(c->arena.get(size_t(3) * kPart, &d_dot));
  PQ_TRY(c->arena.get(size_t(n) * kVecStride, &d_bf));
  PQ_TRY(c->arena.get(size_t(n) * kVecStride, &d_xf));
  std::vector<float> hb(size_t(n) * kVecStride, 0.f), hx(size_t(n) * kVecStride);
  const double* parts[1] = {d_dot};
  double t[1][3];
  for (int64_t r = 0; r < m; ++r) {
    const double* b = rhs + size_t(r) * size_t(n) * 3;
    double* dr = dots + size_t(r) * 6;
    PQ_TRY(copy_in(c, d_b, b, size_t(n) * 3));
    PQ_TRY(amg_vcycle(c, h, d_b, d_x, d_dot));
    PQ_TRY(part_totals_host(c, parts, 1, t));
    for (int k = 0; k < 3; ++k) dr[k] = t[0][k];
    PQ_TRY(fetch(c, x64 + size_t(r) * size_t(n) * 3, d_x, size_t(n) * 3));
    for (int64_t i = 0; i < n; ++i)
      for (int k = 0; k < 3; ++k) hb[size_t(i) * kVecStride + k] = float(b[3 * i + k]);
    PQ_TRY(copy_in(c, d_bf, hb.data(), hb.size()));
    PQ_TRY(amg_vcycle_f32(c, h, d_bf, d_xf, d_dot));
    PQ_TRY(part_totals_host(c, parts, 1, t));
    for (int k = 0; k < 3; ++k) dr[3 + k] = t[0][k];
    PQ_TRY(fetch(c, hx.data(), d_xf, hx.size()));
    float* xr = x32 + size_t(r) * size_t(n) * 3;
    for (int64_t i = 0; i < n; ++i)
      for (int k = 0; k < 3; ++k) xr[3 * i + k] = hx[size_t(i) * kVecStride + k];
  }
  return 0;
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
