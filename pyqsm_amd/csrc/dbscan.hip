// dbscan.hip — eps-neighbourhood clustering on gfx950, bit-exact with
// scikit-learn's DBSCAN (pyQSM/math_utils/fit.py:223) and usable for Open3D's
// cluster_dbscan call sites (pyQSM/geometry/point_cloud_processing.py:185,209).
//
// Parallel formulation of the sequential reference:
//   1. bin points into cells of edge eps, then by octant inside each cell (grid.hip)
//   2. core(i)  <=> #{ j in 27-cell stencil : d2(i,j) <= eps^2 } >= min_pts
//      (wave tiles with an early exit; stragglers in a wave-per-point pass)
//   3. connected components of the core points on the graph of octant sub-cells:
//      a hook pass without union-find, path compression, then lock-free union-find
//      (randomised linking, agent-scope atomics) for what is left; per-point
//      union-find when the grid had to be coarsened
//   4. cluster number = rank of the component's smallest ORIGINAL core index
//      (what the index-order seeding of the sequential algorithm produces)
//   5. border point -> smallest cluster number among its core neighbours
//      (a wave per non-core point)
// The distance predicate is evaluated in fp64 exactly as scikit-learn does:
// d2 = ((dx*dx) + dy*dy) + dz*dz with separately rounded products, compared
// with fl(eps*eps). The library is compiled with -ffp-contract=off.
// (The core pass over fp32 records decides in fp32 the pairs that fp32 can decide, the others in that same
// fp64 form: core_band. The verdicts are the fp64 predicate's, pair by pair.)
#include "grid.hpp"

#include <atomic>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <optional>
#include <type_traits>
#include <vector>

namespace pyqsm {

static constexpr int kNoRoot = 0x7FFFFFFF;

__device__ __forceinline__ double sqdist(double ax, double ay, double az, double bx, double by,
                                         double bz) {
  double t0 = ax - bx, t1 = ay - by, t2 = az - bz;
  double d = t0 * t0;
  d = d + t1 * t1;
  d = d + t2 * t2;
  return d;
}


// Visit every sorted position q in the 27-cell stencil of cell c:
// nine contiguous runs (x-1..x+1 for each of the 3x3 (y,z) rows).
#define FOR_STENCIL(c, st, dir, q, body)                           \
  for (int dz__ = -1; dz__ <= 1; ++dz__)                           \
    for (int dy__ = -1; dy__ <= 1; ++dy__) {                       \
      const int row__ = (c) + dy__ * (st).nx + dz__ * (st).nxy;    \
      const int qb__ = (dir).begin(row__ - 1), qe__ = (dir).begin(row__ + 2); \
      for (int q = qb__; q < qe__; ++q) {                          \
        body                                                       \
      }                                                            \
    }

struct TileLds {
  double x[4][64], y[4][64], z[4][64];  // the current chunk of candidates, per wave
};
// ... and as floats, for the fp32 decision (k_core_tiled<CoordsF32, true>): read two candidates at a time
struct TileLdsF32 {
  alignas(16) float x[4][64], y[4][64], z[4][64];
};
typedef float float2v __attribute__((ext_vector_type(2)));
typedef float float4v __attribute__((ext_vector_type(4)));

// The two thresholds of the fp32 decision of the core pass. A CoordsF32 grid exists only when every input
// coordinate IS an fp32 value, so the fp32 chain
//     d = fl(dx*dx), d = fma(dy, dy, d), d = fma(dz, dz, d)      with dx = fl(x - cx), ...
// differs from the true squared distance D by a relative (1 + u)^5 - 1 < 5.0001 u, u = 2^-24: one rounding on
// each difference, doubled by the squaring; one on the product, one on each fma; the partial sums are sums
// of non-negative terms, so no error is amplified by cancellation. The fp64 chain of the exact predicate is
// within 2^-50 of D. The margin is 2^-20 = 16 u, more than three times the bound:
//     d <= lo <= r2 (1 - 16 u)  =>  D <= d / (1 - 5.0001 u) < r2 (1 - 10 u)  =>  the fp64 chain says "in",
//     d >  hi >= r2 (1 + 16 u)  =>  D >= d / (1 + 5.0001 u) > r2 (1 + 10 u)  =>  the fp64 chain says "out",
// and only lo < d <= hi is left to fp64 (k_core_rest). Underflow: a difference is exact when it is
// subnormal, and a flushed difference or a product below 2^-126 moves d by less than 3 * 2^-126 in all,
// which with lo > 2^-100 is less than 0.75 u of r2: inside the margin (smaller eps: the fp64 kernel).
// Overflow: a difference or a sum that overflows gives d = +inf > hi, "out", and the true D is then above
// 2^128 (1 - 6 u) > FLT_MAX / (1 + 16 u) >= r2: the verdict is right (hi not finite: the fp64 kernel).
// +inf never turns into NaN in the chain (finite coordinates: no inf - inf, no 0 * inf), which is also what
// makes (+inf, 0, 0) the padding candidate that counts on neither side.
struct CoreBand {
  float lo, hi;  // the largest float <= r2 (1 - 2^-20), the smallest float >= r2 (1 + 2^-20)
  bool usable() const { return lo > 0x1p-100f && std::isfinite(hi); }
};
static CoreBand core_band(double r2) {
  const double a = r2 * (1.0 - 0x1p-20), b = r2 * (1.0 + 0x1p-20);
  CoreBand t{0.0f, INFINITY};
  if (!(a > 0.0) || !(b <= double(FLT_MAX))) return t;  // (also NaN)
  t.lo = float(a);
  if (double(t.lo) > a) t.lo = nextafterf(t.lo, -INFINITY);
  t.hi = float(b);
  if (double(t.hi) < b) t.hi = nextafterf(t.hi, INFINITY);
  return t;
}

// The fp32 decision COUNTS with two clamped ramps instead of two compares and two integer adds: per
// candidate pair one packed fma with the clamp modifier and one packed add for each side,
//     s_in = sat(fma(d, -K, A)),  acc_in += s_in        s_hi = sat(fma(d, -K, B)),  acc_hi += s_hi,
// with K a power of two, 1/K in [r2 2^-20, r2 2^-19) (scaling by it is exact), A the largest float
// <= K lo and B the smallest float >= 1 + K hi. The fma rounds once, and a rounding neither changes a
// sign nor carries a value >= 1 below 1, so
//     s_in(d) > 0   =>  K d < A <= K lo         =>  d < lo:   only a certainly-inside candidate adds to
//                                                             acc_in, and at most 1;
//     d <= hi       =>  B - K d >= B - K hi >= 1 =>  s_hi = 1: every possibly-inside candidate adds
//                                                             exactly 1 to acc_hi
// (a flushed result only turns a positive s_in into 0). Fractions arise for d in [lo - 1/K, hi + 1/K] only,
// inside r2 (1 +- 3 * 2^-20) up to a rounding: that is the zone k_core_rest may be asked about, three times
// as wide as the band. The sums need no error bound, only that round-to-nearest is monotone and that
// integers below 2^24 are floats. Induction over the additions: if acc_in <= k, k the number of positive
// terms so far, then fl(acc_in + s) <= fl(k + 1) = k + 1 for a term 0 < s <= 1, and adding 0 changes
// nothing: acc_in never exceeds the count of d <= lo. If acc_hi >= k, k the number of terms equal to 1
// so far, then fl(acc_hi + 1) >= fl(k + 1) = k + 1, and a term >= 0 never lowers a sum: acc_hi is never
// below the count of d <= hi. Adding the two halves keeps both (the same step with integers on one side).
// A tile holds at most kTileMax = 16384 candidates, so every integer involved stays below 2^24. Hence
//     acc_in.x + acc_in.y >= float(min_pts)  =>  at least min_pts candidates certainly within: core,
//     tile done and acc_hi.x + acc_hi.y < float(min_pts)  =>  fewer than min_pts possibly within: not core,
// and every other lane goes to k_core_rest, which decides in fp64. NaN: none arises (finite coordinates; the
// padding candidate gives d = +inf and fma(+inf, -K, .) = -inf, clamped to 0 on both ramps).
struct CoreRamp {
  float lo, hi;   // core_band(r2)
  float K, A, B;  // 0 where the band is not usable
  // ... and the constants are normal floats, min_pts is a float far below 2^24: anything else runs the fp64 kernel
  bool usable(int min_pts = 1) const {
    return CoreBand{lo, hi}.usable() && std::isnormal(K) && std::isnormal(A) && std::isnormal(B) &&
           min_pts <= (1 << 20);
  }
};
static CoreRamp core_ramp(double r2) {
  const CoreBand cb = core_band(r2);
  CoreRamp t{cb.lo, cb.hi, 0.0f, 0.0f, 0.0f};
  if (!cb.usable()) return t;
  int x;
  const double m = frexp(r2, &x);  // r2 = m 2^x, 0.5 <= m < 1: the power of two in [m 2^(x-20), m 2^(x-19))
  const int e = m == 0.5 ? x - 21 : x - 20;
  if (e < -126 || e > 126) return t;
  t.K = float(ldexp(1.0, -e));
  const double a = ldexp(double(cb.lo), -e), b = 1.0 + ldexp(double(cb.hi), -e);  // exact in fp64
  t.A = float(a);
  if (double(t.A) > a) t.A = nextafterf(t.A, -INFINITY);
  t.B = float(b);
  if (double(t.B) < b) t.B = nextafterf(t.B, INFINITY);
  return t;
}
// (the compiler folds no clamp into a packed fp32 fma: min(max(fma, 0), 1) becomes the fma and one
// v_max_f32 ... clamp per element)
__device__ __forceinline__ float2v core_ramp_sat(float2v d, float2v neg_k, float2v c) {
  float2v s;
  asm("v_pk_fma_f32 %0, %1, %2, %3 clamp" : "=v"(s) : "v"(d), "v"(neg_k), "v"(c));
  return s;
}

// The two ramps of n squared distances, pair by pair as the core pass forms them (pyqsm_core_ramp_probe).
__global__ __launch_bounds__(256) void k_core_ramp_probe(const float* __restrict__ d, int64_t n, float neg_k,
                                                         float ramp_a, float ramp_b, float* __restrict__ s_in,
                                                         float* __restrict__ s_hi) {
  const int64_t i = 2 * (int64_t(blockIdx.x) * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const bool two = i + 1 < n;
  const float2v v = {d[i], two ? d[i + 1] : INFINITY};  // (the padding candidate)
  const float2v a = core_ramp_sat(v, float2v{neg_k, neg_k}, float2v{ramp_a, ramp_a});
  const float2v b = core_ramp_sat(v, float2v{neg_k, neg_k}, float2v{ramp_b, ramp_b});
  s_in[i] = a.x, s_hi[i] = b.x;
  if (two) s_in[i + 1] = a.y, s_hi[i + 1] = b.y;
}

// (Measured alternatives, MI355X, 1 M-point forest: per-lane gathers 0.72 ms; this
// LDS-broadcast fp64 loop 0.48 ms; the same with a rigorous fp32 pre-filter and the
// chunk held in registers / broadcast by v_readlane 0.71 ms — issue-stall bound, see
// profiles/r01_dbscan_sq_counters.csv. The simplest form won. That pre-filter still ran fp64 on whatever
// passed; the fp32 DECISION of k_core_tiled<CoordsF32, true> keeps the LDS broadcast and runs no fp64 at all:
// 51.9 -> 36.9 us per launch, 19.2 -> 12.8 M vector instructions, profiles/core_f32_bench_ab.txt. The same
// with the band lanes kept as a wave mask in scalar registers instead of the second count: one vector
// instruction per candidate fewer and 1.3 us slower.)
//
// Only "at least min_pts" matters, so the wave stops as soon as (almost) all of its
// points have seen enough neighbours: the runs are visited centre row first, and once
// at most kStragglers lanes are still short they are put on a list for k_core_rest and
// the wave leaves. In a dense cloud that is after 2-4 of the ~13 chunks; without the
// straggler list one noise point would hold its whole wave to the end.
static constexpr int kStragglers = 6;
// ... and after kMaxChunks chunks everybody still short goes there, whatever their number: a
// tile can hold 5000 candidates (80 chunks) and a wave that cannot leave early was the tail
// that set the kernel's duration (average wave 21 us, kernel 300 us). (6 until the end of round 3; with
// k_core_rest taking a point's stencil as one sequence the balance moved: 10 / 6 / 4 / 3 / 2 / 1 chunks ->
// core phase 0.104 / 0.091 / 0.083 / 0.079 / 0.079 / 0.188 ms per million points at min_pts = 10.)
static constexpr int kMaxChunks = 3;  // for min_pts <= 10; more neighbours asked for, more chunks (core_max_chunks)
static constexpr int kRestSegs = 64;  // segments (and counters) of the straggler list
// centre, same-z rows, same-y rows, corners (compile-time: the run bounds stay in SGPRs)
__device__ constexpr int kRunOrder[9] = {4, 3, 5, 1, 7, 0, 2, 6, 8};

// The nine runs [qb[r], qe[r]) of the 27-cell stencil of cell c, in kRunOrder: the eighteen directory
// words are loaded side by side, then the eighteen slots.
__device__ __forceinline__ void stencil_bounds(int c, Stencil st, const CellDir& dir, int (&qb)[9], int (&qe)[9]) {
  int cells[18], q[18];
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const int row = c + (kRunOrder[r] % 3 - 1) * st.nx + (kRunOrder[r] / 3 - 1) * st.nxy;
    cells[2 * r] = row - 1;
    cells[2 * r + 1] = row + 2;
  }
  dir.begins(cells, q);
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    qb[r] = q[2 * r];
    qe[r] = q[2 * r + 1];
  }
}

// F32 (CoordsF32 only; core_band and core_ramp above): the tiled path decides in packed fp32 against the two
// thresholds and counts twice with the clamped ramps, acc_in (d <= lo: certainly within, never too many) and
// acc_hi (d <= hi: possibly within, never too few), two halves each; cnt below means their sums. acc_in takes
// the place of the exact count everywhere: a lane is core once it reaches min_pts, the early exit and the
// hand-off go by it. A lane is non-core when the whole tile was visited and acc_hi < min_pts; a lane that still
// straddles then joins the stragglers, and k_core_rest decides it in fp64.
// Two candidates per step: three v_pk_add_f32, one v_pk_mul_f32 and two v_pk_fma_f32 for the distances, two
// v_pk_fma_f32 with clamp and two v_pk_add_f32 for the counts, no conversion on staging and half the LDS
// bytes. The per-cell path of the oversized tiles stays fp64.
template <class CO, bool F32>
__global__ __launch_bounds__(256) void k_core_tiled(int n, const GridPlan* __restrict__ plan,
                                                    const DirWord* __restrict__ dwords,
                                                    const int32_t* __restrict__ dslots,
                                                    const int32_t* __restrict__ cell_of, CO co, double r2,
                                                    float neg_k, float ramp_a, float ramp_b /*F32: core_ramp(r2)*/,
                                                    int min_pts, uint8_t* __restrict__ core,
                                                    int32_t* __restrict__ rest,
                                                    int32_t* __restrict__ rest_cnt /*[kRestSegs]*/, int seg_cap,
                                                    int* __restrict__ parent, int* __restrict__ min_orig,
                                                    uint32_t* __restrict__ bits /*[n / 32 + 2]*/,
                                                    int32_t* __restrict__ seam /*[seam_cap]*/, int seam_cap,
                                                    int max_chunks,
                                                    unsigned long long* __restrict__ tests /*may be null:
                                                    [256] slots, candidates staged per wave (x 64 lanes
                                                    = lane-tests executed), then [256] slots, lanes handed
                                                    on with a distance in the band (F32)*/,
    unsigned long long* __restrict__ st /*stamps or null*/) {
  __shared__ TileLds L;
  __shared__ TileLdsF32 LF;  // (F32 only: an unused array takes no LDS)
  stamped(st, [&] {
  const CellDir dir{dwords, dslots};
  // wave-uniform quantities are forced into SGPRs so that the loops below are scalar
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int p0 = (blockIdx.x * 4 + w) * 64;
  if (p0 >= n || !plan->ok) return;  // whole wave
  const Stencil st = plan_stencil(plan);
  const int ncell = plan->ncell;
  const int p = p0 + lane;
  const bool live = p < n;
  double x = 0.0, y = 0.0, z = 0.0;
  float fx = 0.0f, fy = 0.0f, fz = 0.0f;  // F32: the same point as it is stored
  if constexpr (F32) {
    if (live) {
      const float4 v = co.p[p];
      fx = v.x, fy = v.y, fz = v.z;
    }
  } else {
    if (live) co.get(p, x, y, z);
  }
  const Tile t = wave_tile(p0, n, st, ncell, dir, cell_of);
  int cnt = 0;  // (starting lanes of sub-cells with >= min_pts points as "decided" gained nothing)
  float2v acc_in = {0.0f, 0.0f}, acc_hi = {0.0f, 0.0f};  // F32, the tiled path: the ramps' sums (cnt stays 0)
  const float fmin_pts = float(min_pts);
  bool deferred = false;
  int chunks = 0;
  int staged = 0;  // wave-uniform: candidates this wave tested its 64 lanes against
  int band = 0;    // wave-uniform, F32: lanes handed on that had a distance in the band (acc_in < acc_hi): all
                   // that fp32 alone might have decided otherwise
  // The lanes of `und` (short of min_pts) restart on their own in k_core_rest. A wave comes here once.
  const auto hand_on = [&](unsigned long long und) {
    if (und != 0) {
      int slot = 0;
      const int lead = __ffsll(und) - 1;
      // kRestSegs counters, a block's stragglers go to segment blockIdx % kRestSegs of the list
      // (capacity seg_cap: a block has at most 256): thousands of waves adding to ONE counter were
      // served one at a time (~10 ns each), and every one of them waited for its turn
      const int seg = blockIdx.x % kRestSegs;
      if (lane == lead) slot = atomicAdd(rest_cnt + seg, __popcll(und));
      slot = __shfl(slot, lead, 64);
      const bool mine = (und >> lane) & 1ull;
      if constexpr (F32) band += __popcll(__ballot(mine && acc_hi.x + acc_hi.y > acc_in.x + acc_in.y));
      if (mine) {
        rest[size_t(seg) * seg_cap + slot + __popcll(und & ((1ull << lane) - 1ull))] = p;
        cnt = -1;
      }
    }
    deferred = true;
  };
  const bool ramped = F32 && t.total <= kTileMax;  // wave-uniform: the verdict is acc_in's, not cnt's
  if (t.total > kTileMax) {
    // The wave's points straddle distant cells (end of one grid layer, start of the next):
    // the linear intervals would sweep whole layers. Take the distinct cells of the wave
    // one at a time instead — exact 27-cell stencil, candidates still staged through LDS,
    // only the lanes of that cell count. (A per-lane walk here made these few waves the
    // 0.25 ms tail of the whole kernel: ~850 dependent gathers per lane.)
    if constexpr (F32) x = double(fx), y = double(fy), z = double(fz);
    const int mycell = live ? cell_of[p] : -1;
    unsigned long long todo = __ballot(live);
    while (todo) {
      const int lead = __ffsll(todo) - 1;
      const int c = __builtin_amdgcn_readlane(mycell, lead);
      const bool mine = mycell == c;
      todo &= ~__ballot(mine);
      int rqb[9], rqe[9];  // the cell's nine runs (in kRunOrder: every candidate counts, the order is free)
      stencil_bounds(c, st, dir, rqb, rqe);
#pragma unroll
      for (int r = 0; r < 9; ++r) {
        const int qb = __builtin_amdgcn_readfirstlane(rqb[r]);
        const int qe = __builtin_amdgcn_readfirstlane(rqe[r]);
        for (int base = qb; base < qe; base += 64) {
          const int q = base + lane;
          const int m = qe - base < 64 ? qe - base : 64;
          if (q < qe) co.get(q, L.x[w][lane], L.y[w][lane], L.z[w][lane]);
          __builtin_amdgcn_wave_barrier();
          staged += m;
          if (mine)
            for (int j = 0; j < m; ++j)
              cnt += sqdist(x, y, z, L.x[w][j], L.y[w][j], L.z[w][j]) <= r2;
          __builtin_amdgcn_wave_barrier();
        }
      }
    }
  } else {
    const float2v X = {fx, fx}, Y = {fy, fy}, Z = {fz, fz};  // (F32)
    const float2v NK = {neg_k, neg_k}, RA = {ramp_a, ramp_a}, RB = {ramp_b, ramp_b};
#pragma unroll
    for (int ri = 0; ri < 9; ++ri) {
      const int r = kRunOrder[ri];
      for (int base = t.qb[r]; base < t.qe[r] && !deferred; base += 64) {
        const int q = base + lane;
        const int m = t.qe[r] - base < 64 ? t.qe[r] - base : 64;
        if constexpr (F32) {
          // every lane stores: its candidate, or the padding (d = +inf) that makes an odd count even
          float4 v = make_float4(INFINITY, 0.0f, 0.0f, 0.0f);
          if (q < t.qe[r]) v = co.p[q];
          LF.x[w][lane] = v.x, LF.y[w][lane] = v.y, LF.z[w][lane] = v.z;
          __builtin_amdgcn_wave_barrier();
          const auto pair = [&](float2v cx, float2v cy, float2v cz) {
            const float2v dx = X - cx, dy = Y - cy, dz = Z - cz;
            float2v d = dx * dx;
            d = __builtin_elementwise_fma(dy, dy, d);
            d = __builtin_elementwise_fma(dz, dz, d);
            acc_in += core_ramp_sat(d, NK, RA);
            acc_hi += core_ramp_sat(d, NK, RB);
          };
          // Four pairs a step and the rest pair by pair, by hand: an asm statement counts as convergent, and a
          // loop that holds one is not unrolled with a remainder. The step reads 16 bytes at a time
          // (ds_read_b128; left to itself the compiler pairs the 8-byte reads into ds_read2_b64, which costs the
          // LDS four times the cycles per byte and made it, not the vector pipe, the loop's limit).
          int j = 0;
          for (; j + 8 <= m; j += 8) {
            const float4v* const lx = reinterpret_cast<const float4v*>(&LF.x[w][j]);
            const float4v* const ly = reinterpret_cast<const float4v*>(&LF.y[w][j]);
            const float4v* const lz = reinterpret_cast<const float4v*>(&LF.z[w][j]);
            const float4v x0 = lx[0], x1 = lx[1], y0 = ly[0], y1 = ly[1], z0 = lz[0], z1 = lz[1];
            pair(x0.lo, y0.lo, z0.lo);
            pair(x0.hi, y0.hi, z0.hi);
            pair(x1.lo, y1.lo, z1.lo);
            pair(x1.hi, y1.hi, z1.hi);
          }
          for (; j < m; j += 2)
            pair(*reinterpret_cast<const float2v*>(&LF.x[w][j]), *reinterpret_cast<const float2v*>(&LF.y[w][j]),
                 *reinterpret_cast<const float2v*>(&LF.z[w][j]));
        } else {
          if (q < t.qe[r]) co.get(q, L.x[w][lane], L.y[w][lane], L.z[w][lane]);
          __builtin_amdgcn_wave_barrier();
#pragma unroll 4
          for (int j = 0; j < m; ++j)
            cnt += sqdist(x, y, z, L.x[w][j], L.y[w][j], L.z[w][j]) <= r2;
        }
        staged += m;
        __builtin_amdgcn_wave_barrier();
        const unsigned long long und =
            F32 ? __ballot(live && acc_in.x + acc_in.y < fmin_pts) : __ballot(live && cnt < min_pts);
        ++chunks;
        // (the tile's last chunk: whoever is still short has seen everything)
        if ((__popcll(und) <= kStragglers || chunks >= max_chunks) &&
            !(ri == 8 && base + 64 >= t.qe[r])) {
          hand_on(und);  // the few lanes still short
          break;
        }
      }
    }
    // F32, the whole tile visited (through its last chunk or through empty trailing runs): a lane short
    // of min_pts by acc_in is non-core only if acc_hi is short too
    if constexpr (F32) {
      if (!deferred)
        hand_on(__ballot(live && acc_in.x + acc_in.y < fmin_pts && acc_hi.x + acc_hi.y >= fmin_pts));
    }
  }
  if (live && cnt >= 0) {  // (not handed on)
    const bool is_core = ramped ? acc_in.x + acc_in.y >= fmin_pts : cnt >= min_pts;
    core[p] = is_core;
    co.mark_core(p, is_core);
  }
  // the start of the union phase rides along (it was a launch of its own, ~5 us): every point its own
  // parent, no smallest index yet, k_number's bitmap (n / 32 + 1 words: nothing reads more of it) and the
  // cells' seam words empty (k_flatten_reps; a word per directory slot, n of them and a few per bucket
  // more: the n live threads stride over them), no pre-root listed (the count lies behind the bitmap)
  if (live) {
    parent[p] = p;
    min_orig[p] = 0x7F7F7F7F;  // > any index
    if (p <= n / 32) bits[p] = 0u;
    if (p == 0) bits[n / 32 + 1] = 0u;
    for (int i = p; i < seam_cap; i += n) seam[i] = 0;
  }
  if (tests && lane == 0) {
    atomicAdd(tests + (blockIdx.x & 255), static_cast<unsigned long long>(staged));
    if (band) atomicAdd(tests + 256 + (blockIdx.x & 255), static_cast<unsigned long long>(band));
  }
  });
}

// The 27-cell stencil of one point as ONE sequence of candidates: the nine runs' bounds are loaded side
// by side (they used to be fetched row by row, a dependent round trip each before the row's candidates
// could be asked for), and candidate g of the sequence is found by a chain of selects. Wave-uniform.
// The runs come in kRunOrder, centre row first, as k_core_tiled visits them: a point's near neighbours
// are among the first candidates, so a walk that stops at min_pts (k_core_rest) stops steps earlier.
struct Runs9 {
  int qb[9];
  int pre[10];  // pre[r] = candidates before run r, pre[9] = all
  __device__ __forceinline__ int at(int g) const {  // sorted position of candidate g < pre[9]
    int q = qb[0] + g;
#pragma unroll
    for (int r = 1; r < 9; ++r) q = g >= pre[r] ? qb[r] + (g - pre[r]) : q;
    return q;
  }
};
// The runs of kRunBatch points per wave at once. With the ranked directory a bound is two dependent
// loads (word, slot), and a wave that takes one point per step pays that chain, on top of the point's
// own (list entry -> cell -> bounds -> candidates), once per point: k_core_rest went from 16.5 to
// 25.7 us on the benchmark forest with the bounds fetched per point by scalar loads. So lane
// 18 k + j looks up bound j of the wave's k-th point (j = 2 r: begin of run r in kRunOrder, 2 r + 1:
// its end): one gather of words and one of slots serve three points, whose chains overlap.
static constexpr int kRunBatch = 3;
__device__ __forceinline__ int lane_bound(bool act, int c, int j, Stencil st, const CellDir& dir) {
  const int r = int((0x862071534ull >> (4 * (j >> 1))) & 15ull);  // kRunOrder[j >> 1], without a table in memory
  const int cell = c + (r % 3 - 1) * st.nx + (r / 3 - 1) * st.nxy + ((j & 1) ? 2 : -1);
  int b = 0;
  if (act) {
    const DirWord w = dir.words[cell >> 5];
    b = dir.slots[CellDir::slot_of(w, cell)];
  }
  return b;
}
// the k-th point's runs out of the lanes' bounds (k is a constant: unrolled loops)
__device__ __forceinline__ Runs9 runs_of_lanes(int bound, int k) {
  Runs9 t;
  t.pre[0] = 0;
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    t.qb[r] = __builtin_amdgcn_readlane(bound, 18 * k + 2 * r);
    t.pre[r + 1] = t.pre[r] + (__builtin_amdgcn_readlane(bound, 18 * k + 2 * r + 1) - t.qb[r]);
  }
  return t;
}

// The stragglers of k_core_tiled, one WAVE each: 64 candidates of the stencil per step,
// stop at min_pts. (One lane each was 0.13 ms per million points: a noise point walks
// ~850 candidates one dependent load at a time.) A wave takes kRunBatch stragglers per step and
// looks their bounds up together (lane_bound), then walks them one after the other.
template <class CO>
__global__ __launch_bounds__(256) void k_core_rest(const int32_t* __restrict__ rest,
                                                   const int32_t* __restrict__ rest_cnt /*[kRestSegs]*/,
                                                   int seg_cap, const GridPlan* __restrict__ plan,
                                                   const DirWord* __restrict__ dwords,
                                                   const int32_t* __restrict__ dslots,
                                                   const int32_t* __restrict__ cell_of, CO co, double r2,
                                                   int min_pts, uint8_t* __restrict__ core,
    unsigned long long* __restrict__ st /*stamps or null*/) {
  stamped(st, [&] {
  const CellDir dir{dwords, dslots};
  if (!plan->ok) return;
  const Stencil st = plan_stencil(plan);
  const int lane = threadIdx.x & 63;
  // the list is kRestSegs segments: lane s holds segment s's count, an inclusive scan numbers the entries
  const int mine = rest_cnt[lane];
  int incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(incl, off, 64);
    if (lane >= off) incl += v;
  }
  const int m = __shfl(incl, 63, 64);
  const int grp = lane / 18, j = lane % 18;  // (lanes 54 .. 63 look nothing up)
  for (int i0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * kRunBatch; i0 < m; i0 += gridDim.x * 4 * kRunBatch) {  // wave-uniform
    int p = 0;
#pragma unroll
    for (int k = 0; k < kRunBatch; ++k) {
      if (i0 + k >= m) break;  // wave-uniform
      const int seg = __popcll(__ballot(incl <= i0 + k));  // the first segment whose running total exceeds the entry
      const int before = __shfl(incl - mine, seg, 64);
      const int pk = rest[size_t(seg) * seg_cap + (i0 + k - before)];
      p = grp == k ? pk : p;
    }
    const bool act = grp < kRunBatch && i0 + grp < m;
    double x = 0.0, y = 0.0, z = 0.0;
    int c = 0;
    if (act) {
      co.get(p, x, y, z);
      c = cell_of[p];
    }
    const int bound = lane_bound(act, c, j, st, dir);
#pragma unroll
    for (int k = 0; k < kRunBatch; ++k) {
      if (i0 + k >= m) break;  // wave-uniform
      const Runs9 t = runs_of_lanes(bound, k);
      const int pk = __builtin_amdgcn_readlane(p, 18 * k);
      const double xk = __shfl(x, 18 * k, 64), yk = __shfl(y, 18 * k, 64), zk = __shfl(z, 18 * k, 64);
      int cnt = 0;
      for (int g0 = 0; g0 < t.pre[9] && cnt < min_pts; g0 += 64) {
        const int g = g0 + lane;
        const bool hit = g < t.pre[9] && co.d2(t.at(g), xk, yk, zk) <= r2;
        cnt += __popcll(__ballot(hit));
      }
      if (lane == 0) {
        core[pk] = cnt >= min_pts;
        co.mark_core(pk, cnt >= min_pts);
      }
    }
  }
  });
}

// ---- union-find --------------------------------------------------------------

__device__ __forceinline__ int ld_parent(const int* parent, int i) {
  return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_parent(int* parent, int i, int v) {
  __hip_atomic_store(parent + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Linking order. Hooking "larger index under smaller" on spatially sorted indices builds
// chains (neighbours in space are neighbours in index), and every find then walks
// hundreds of dependent loads. A bijective hash of the index as the priority is
// randomised linking: expected depth O(log n). A root is hooked under a root of smaller
// priority, so priorities strictly decrease towards the root: every pointer names an
// ancestor, halving a path is always safe, and there are no cycles.
__device__ __forceinline__ unsigned link_prio(int x) { return unsigned(x) * 0x9E3779B1u; }

__device__ __forceinline__ int find_root(int* parent, int x) {
  int cur = ld_parent(parent, x);
  if (cur != x) {
    int prev = x, next;
    while (cur != (next = ld_parent(parent, cur))) {
      st_parent(parent, prev, next);
      prev = cur;
      cur = next;
    }
  }
  return cur;
}

__device__ __forceinline__ void unite(int* parent, int a, int b) {
  int ra = find_root(parent, a), rb = find_root(parent, b);
  while (ra != rb) {
    if (link_prio(ra) < link_prio(rb)) {
      int t = ra;
      ra = rb;
      rb = t;
    }
    // hook the root of larger priority under the other one
    const int old = atomicCAS(parent + ra, ra, rb);
    if (old == ra) break;
    // lost the race: ra has a parent now. Climb with loads, not with failing CAS
    // operations (atomics on one address are served one at a time).
    ra = find_root(parent, old);
    rb = find_root(parent, rb);
  }
}

// ---- union phase over octant sub-cells -------------------------------------------------
// Cells have an edge of eps (a hair more), so two points of the same octant sub-cell
// (half a cell per axis) are at most 0.87 eps apart: the core points of a sub-cell are one
// component without any test. What remains is to find, for every pair of sub-cells at
// most two sub-cells apart per axis, ONE core-core pair within eps — and not even that
// once the two are known to be in the same tree. The first version walked all ~850
// candidates of every core point and chased a parent pointer for each of its ~40 core
// neighbours (1.15 ms per million points, 91 % memory waits); this one looks at
// 62 neighbour sub-cells per sub-cell, most of them empty or already joined.

// A thread per sorted point, a wave per 64 consecutive points: sub-cell runs are contiguous, so "which core
// point of my run comes first" is a ballot over the wave's core flags. The representative (the run's first
// core point) takes the run's minimum of original indices, a segmented min over the wave's lanes plus, for the
// one run that goes on past the wave, the rest of it 64 points per step; it fills in the record and lists the
// sub-cell. Core points hang themselves under it. A run that began in an earlier wave is looked up from its
// start, 64 core flags per load. Everything a wave needs besides the run records, the 64 points before and
// after it included, is loaded up front side by side, so that only runs longer than that loop. (The first
// version let each run's first thread walk the run alone with byte loads: 24 us per million points, the
// longest run of a wave setting the wave's time; this one 18.6 us. Neither the loads one after the other
// (18.9) nor four rounds of 1024 points per block with one append (17.5; k_labels the same way 18.3 -> 20.5)
// moved it much: it is not bound by one wave's chain of loads nor by the list's atomic.)
__global__ __launch_bounds__(1024) void k_sub_rep(int n, const int32_t* __restrict__ sub_of,
                                                 const uint8_t* __restrict__ core,
                                                 const int32_t* __restrict__ order,
                                                 int* __restrict__ parent,
                                                 const int32_t* __restrict__ cell_of,
                                                 int4* __restrict__ rec,
                                                 int* __restrict__ run_min,
                                                 int4* __restrict__ list,
                                                 int32_t* __restrict__ list_cnt, const GridPlan* __restrict__ plan,
                                                 int4* __restrict__ list_xyz,
                                                 const DirWord* __restrict__ dwords,
    unsigned long long* __restrict__ st /*stamps or null*/) {
  stamped(st, [&] {
  if (!plan->ok) return;
  const int nx = plan->nx, ny = plan->ny;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int base = blockIdx.x * 1024 + w * 64;  // the wave's first position
  const int p = base + lane;
  const bool live = p < n;
  int sid = 0, s = n, e = n, ord = 0x7FFFFFFF, cell = 0;  // sub-cell, run [s, e), original index, cell
  bool c = false;
  // the wave before and the wave after: their core flags, and the next one's original indices
  const bool c_prev = base >= 64 && p - 64 < n && core[p - 64];
  const bool c_next = p + 64 < n && core[p + 64];
  const int o_next = c_next ? order[p + 64] : 0x7FFFFFFF;
  if (live) {
    sid = sub_of[p];
    c = core[p];
    if (c) ord = order[p];
    cell = cell_of[p];
    const int2 run = *reinterpret_cast<const int2*>(rec + sid);  // (first position, points)
    s = run.x;
    e = run.x + run.y;
  }
  const unsigned long long cb = __ballot(c);
  // the run of lane 0 may have begun in an earlier wave: its first core point there, if any (wave-uniform)
  int lead = -1;
  const int s0 = __shfl(s, 0, 64);
  if (s0 < base && s0 >= base - 64) {  // within the wave before
    const unsigned long long f = __ballot(c_prev && base - 64 + lane >= s0);
    if (f) lead = base - 64 + __ffsll(f) - 1;
  } else {
    for (int q0 = s0; q0 < base; q0 += 64) {
      const int q = q0 + lane;
      const unsigned long long f = __ballot(q < base && core[q]);
      if (f) {
        lead = q0 + __ffsll(f) - 1;
        break;
      }
    }
  }
  int rep = -1;
  if (c) {
    if (s < base && lead >= 0) {
      rep = lead;
    } else {  // the first core lane of my run in this wave (lane itself at the latest)
      const int lo = s > base ? s - base : 0;
      rep = base + __ffsll(cb & (~0ull << lo)) - 1;
    }
    parent[p] = rep;
  }
  const bool is_rep = c && rep == p;
  // smallest original index of the core points from each lane to its run's end within the wave
  int mn = ord;
  const int seg_end = e - base < 64 ? e - base : 64;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_down(mn, off, 64);
    if (lane + off < seg_end) mn = o < mn ? o : mn;
  }
  // ... and beyond it, for the representative whose run goes on past the wave (at most one)
  const unsigned long long tail = __ballot(is_rep && e > base + 64);
  if (tail) {
    const int t = __ffsll(tail) - 1;
    const int et = __shfl(e, t, 64);
    int m2 = base + 64 + lane < et ? o_next : 0x7FFFFFFF;
    for (int q = base + 128 + lane; q < et; q += 64)
      if (core[q]) m2 = min(m2, order[q]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const int o = __shfl_xor(m2, off, 64);
      m2 = o < m2 ? o : m2;
    }
    if (lane == t) mn = min(mn, m2);
  }
  if (is_rep) {
    rec[sid].z = rep;
    run_min[rep] = mn;  // smallest original index among the run's core points
  }
  // block-aggregated append of the representatives: one atomic per block of 1024 threads
  // (atomics on a single address are served one at a time: one per wave cost 0.16 ms per
  // million points, one per 256 threads still 0.04 ms)
  __shared__ int wcount[16], wbase[16];
  const unsigned long long b = __ballot(is_rep);
  if (lane == 0) wcount[w] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int k = 0; k < 16; ++k) tot += wcount[k];
    int base2 = tot ? atomicAdd(list_cnt, tot) : 0;
    for (int k = 0; k < 16; ++k) {
      wbase[k] = base2;
      base2 += wcount[k];
    }
  }
  __syncthreads();
  // list record: representative, its cell, its cell's directory slot (where the cell's seam word lies,
  // k_flatten_reps: the directory word is looked up HERE, where the neighbouring lanes ask for the same
  // one), points from it to the run's end
  // ... and, for k_hook_sub, its cell's grid coordinates and its octant: the two integer divisions by the
  // grid's dimensions happen HERE, once per sub-cell — in the hook pass every wave did twelve of them per
  // four sub-cells (~40 instructions each; the pass's look-ups were 48 us of its 81, a third of that this)
  if (is_rep) {
    const int slot = wbase[w] + __popcll(b & ((1ull << lane) - 1ull));
    const int c1 = cell;
    list[slot] = make_int4(rep, c1, CellDir::slot_of(dwords[c1 >> 5], c1), e - rep);
    list_xyz[slot] = make_int4(c1 % nx, (c1 / nx) % ny, c1 / (nx * ny), sid & 7);
  }
  });
}

// The 62 lexicographically positive (dz, dy, dx) offsets in [-2,2]^3 as (dx, dy, dz): the 13
// of max-norm 1 first, then the 49 of max-norm 2.
__constant__ signed char kSubOffsets[62][3] = {{1,0,0}, {-1,1,0}, {0,1,0}, {1,1,0}, {-1,-1,1}, {0,-1,1}, {1,-1,1}, {-1,0,1}, {0,0,1}, {1,0,1}, {-1,1,1}, {0,1,1}, {1,1,1}, {2,0,0}, {-2,1,0}, {2,1,0}, {-2,2,0}, {-1,2,0}, {0,2,0}, {1,2,0}, {2,2,0}, {-2,-2,1}, {-1,-2,1}, {0,-2,1}, {1,-2,1}, {2,-2,1}, {-2,-1,1}, {2,-1,1}, {-2,0,1}, {2,0,1}, {-2,1,1}, {2,1,1}, {-2,2,1}, {-1,2,1}, {0,2,1}, {1,2,1}, {2,2,1}, {-2,-2,2}, {-1,-2,2}, {0,-2,2}, {1,-2,2}, {2,-2,2}, {-2,-1,2}, {-1,-1,2}, {0,-1,2}, {1,-1,2}, {2,-1,2}, {-2,0,2}, {-1,0,2}, {0,0,2}, {1,0,2}, {2,0,2}, {-2,1,2}, {-1,1,2}, {0,1,2}, {1,1,2}, {2,1,2}, {-2,2,2}, {-1,2,2}, {0,2,2}, {1,2,2}, {2,2,2}};

// Block-aggregated append of the flagged threads' values to list[*cnt]: one atomic per block (atomics on one
// address are served one at a time). Every thread of the block calls it.
template <int kThreads>
__device__ __forceinline__ void block_append(bool take, int value, int32_t* __restrict__ list,
                                             int32_t* __restrict__ cnt) {
  constexpr int kWaves = kThreads / 64;
  __shared__ int wcount[kWaves], wbase[kWaves];
  const unsigned long long b = __ballot(take);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) wcount[w] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int k = 0; k < kWaves; ++k) tot += wcount[k];
    int base = tot ? atomicAdd(cnt, tot) : 0;
    for (int k = 0; k < kWaves; ++k) {
      wbase[k] = base;
      base += wcount[k];
    }
  }
  __syncthreads();
  if (take) list[wbase[w] + __popcll(b & ((1ull << lane) - 1ull))] = value;
}

// The list of the non-core points for the label pass (`rest`, reused from the core pass: after k_core_rest),
// from the final core flags. Block b of the role takes the sorted positions [b * kFlagsPerBlock,
// (b + 1) * kFlagsPerBlock), sixteen per thread, their loads side by side, and appends its non-core ones with ONE
// atomic as block_append does (the counter is one address and its atomics are served one at a time, so few
// large blocks). Every thread of a block of kFlagsThreads calls it; it runs as extra blocks of a launch of the
// union phase whose own blocks leave most wave slots empty (k_flatten_reps).
static constexpr int kFlagsThreads = 256, kFlagsPer = 16, kFlagsPerBlock = kFlagsThreads * kFlagsPer;
__device__ __forceinline__ void flags_role(int b, int n, const uint8_t* __restrict__ core,
                                           int32_t* __restrict__ rest, int32_t* __restrict__ rest_cnt) {
  constexpr int kWaves = kFlagsThreads / 64;
  __shared__ int fcount[kWaves], fbase[kWaves];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int p0 = b * kFlagsPerBlock + threadIdx.x;
  unsigned take = 0;  // bit k: position p0 + k * kFlagsThreads is a non-core point
#pragma unroll
  for (int k = 0; k < kFlagsPer; ++k) {
    const int p = p0 + k * kFlagsThreads;
    take |= unsigned(p < n && !core[p]) << k;
  }
  // the wave's count by a butterfly: sixteen ballots kept across the barriers cost the launch a wave per SIMD in
  // scalar registers
  int mine = __popc(take);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
  if (lane == 0) fcount[w] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int k = 0; k < kWaves; ++k) tot += fcount[k];
    int base = tot ? atomicAdd(rest_cnt, tot) : 0;
    for (int k = 0; k < kWaves; ++k) {
      fbase[k] = base;
      base += fcount[k];
    }
  }
  __syncthreads();
  int at = fbase[w];
#pragma unroll
  for (int k = 0; k < kFlagsPer; ++k) {
    const bool t = (take >> k) & 1u;
    const unsigned long long bal = __ballot(t);
    if (t) rest[at + __popcll(bal & ((1ull << lane) - 1ull))] = p0 + k * kFlagsThreads;
    at += __popcll(bal);
  }
}

// Full path compression for the listed representatives (plain accesses: the kernel
// boundary makes the unions of the previous launch visible, and any value another lane
// writes meanwhile is an ancestor too).
// Several launches of one kernel, by mode:
//   kFlattenJump   moves every pointer `max_steps` links up (a hundred and more dependent loads per
//                  thread, all threads starting together, was 35 us per million points); the launch
//                  after it then reaches the root in depth / max_steps hops over the pointers it left.
//   kFlattenLink   reaches the root r of the sub-cell and, side by side (both sets of loads in flight
//                  together), the root r2 of its SECOND LINK (k_hook_sub), and unites the two where they
//                  differ. The hook pass follows the first connected neighbour only, which leaves thin
//                  basins side by side along every stem (386 trees for the 20 clusters of the benchmark
//                  forest, and 37 k sub-cells on their seams for k_union_sub); the second links cross
//                  nearly all of those boundaries (23 trees, 86 seam sub-cells), and only the few thousand
//                  that join two different trees cost a union.
//   kFlattenWords  chases the one to three links those unions left and folds the root into the cell's word.
//   kFlattenRoots  the sequence without second links (PYQSM_DBSCAN_LINK2=0): root and word in one launch.
// kFlattenLink runs concurrently with its own CAS hooks on roots, so no mode stores a pointer that is
// unchanged: `parent[p] = p` could overwrite the hook another thread has just installed on the root p.
// A sub-cell that is not a root is never the target of a CAS, and whatever is stored there is an ancestor.
// Plain reads that race with the unions still name ancestors (trees only merge).
// The launch that knows every listed sub-cell's root r (the WORDS launch: kFlattenWords, or kFlattenRoots
// without second links; no union runs while it does, so r is exact) does two things with it.
// It folds r into ONE WORD PER CELL, seam[slot]: a table of its own indexed by the cell's slot in the
// ranked directory (CellDir::slot_of, which k_sub_rep left in the list entry), so that the words of
// x-neighbouring occupied cells share a line (k_core_tiled zeroes it):
//   0      no sub-cell with core points seen yet
//   r + 1  every such sub-cell of the cell seen so far has root r
//   -1     mixed
// The first to arrive installs r + 1; whoever finds another root there stores -1. Whatever the order of
// arrival, the word ends as r + 1 exactly when all of the cell's listed sub-cells have root r.
// k_union_sub decides "same tree" per CELL from it.
// And it lists the PRE-ROOTS, the sub-cells that are their own root now. From here on every representative
// points at a pre-root: k_union_sub's unions only hook pre-roots under pre-roots, and the path halving of
// their finds moves a pointer to another ancestor, a pre-root again. The smallest indices are folded into
// the pre-roots beside the seams (fold_role) and k_fold_roots settles the pre-roots after them; a launch
// over all representatives (k_rep_root, 16.8 us per million points for the benchmark forest's 23
// pre-roots) is not needed for it.
// The hosting launch (kFlattenLink, or kFlattenRoots without second links) also carries flags_role in the
// blocks behind its own: its threads spend their time waiting on chains of dependent loads.
enum FlattenMode { kFlattenJump, kFlattenRoots, kFlattenLink, kFlattenWords };

// The minimum of v over the active lanes that share a root r, for every root of the wave: returned in the
// root's first lane, 0x7FFFFFFF in every other lane. One root at a time, shuffles only.
__device__ __forceinline__ int wave_fold_by_root(bool active, int r, int v) {
  const int lane = threadIdx.x & 63;
  int fold = 0x7FFFFFFF;
  unsigned long long rem = __ballot(active);
  while (rem) {
    const int lead = __ffsll(rem) - 1;
    const int r0 = __shfl(r, lead, 64);
    const bool mine = active && r == r0;
    int mn = mine ? v : 0x7FFFFFFF;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const int o = __shfl_xor(mn, off, 64);
      mn = o < mn ? o : mn;
    }
    if (lane == lead) fold = mn;
    rem &= ~__ballot(mine);
  }
  return fold;
}

// The components' smallest original core indices, folded from the per-run minima of the representatives
// (run_min, k_sub_rep: 5x fewer values than points) into min_orig of the pre-root each representative
// points at. It runs as extra blocks of k_union_sub's launch, entry s of the list per thread: that launch's own
// blocks leave the chip nearly empty (a few waves on the seams), and this role is what cost k_rep_root its
// time — a wave of representatives spans a dozen clusters (grid rows run across the whole scene), and
// folding them one root at a time is some four hundred cycles per root. The unions of the same launch only
// move a representative's pointer to another pre-root above it, and k_fold_roots hands every pre-root's
// minimum on to its final root afterwards, so whichever pre-root the plain read names will do.
// Each group of four waves puts its (root, minimum) pairs together in LDS, the group's first wave folds
// those the same way, and only what is left goes to min_orig, behind a plain pre-check: an atomic only if it
// can still lower the stored minimum. (Atomics on one address are served one at a time; folding all core
// points with them cost 0.23 ms per million points.) Every thread of a block of kThreads calls it.
static constexpr int kFoldSlots = 64;  // pairs of a group of four waves: what one wave folds
static constexpr int kFoldRuns = 24;   // runs of equal roots in a wave beyond which it does not fold
template <int kThreads>
__device__ __forceinline__ void fold_role(int s, int m, const int4* __restrict__ list, const int* parent,
                                          const int* __restrict__ run_min, int* min_orig) {
  constexpr int kGroups = kThreads / 256;
  __shared__ int f_root[kGroups][kFoldSlots], f_min[kGroups][kFoldSlots], f_cnt[kGroups];
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 8;
  if ((threadIdx.x & 255) == 0) f_cnt[grp] = 0;
  const bool active = s < m;
  int r = -1, v = 0x7FFFFFFF;
  if (active) {
    const int p = list[s].x;
    v = run_min[p];
    r = parent[p];
  }
  __syncthreads();
  const volatile int* vmin = min_orig;  // a stale value only costs an atomic
  // Where nearly every sub-cell is its own tree (a sparse cloud with min_pts = 1) there is nothing to fold and
  // no address is hot: a wave with more than kFoldRuns runs of equal roots sends every value straight to its root.
  const int before = __shfl_up(r, 1, 64);
  const bool many = __popcll(__ballot(lane == 0 || before != r)) > kFoldRuns;  // wave-uniform
  if (many && active && v < vmin[r]) atomicMin(min_orig + r, v);
  const int fold = many ? 0x7FFFFFFF : wave_fold_by_root(active, r, v);
  const bool has = fold != 0x7FFFFFFF;
  const unsigned long long hb = __ballot(has);
  int at = 0;
  if (lane == 0 && hb) at = atomicAdd(&f_cnt[grp], __popcll(hb));
  at = __shfl(at, 0, 64) + __popcll(hb & ((1ull << lane) - 1ull));
  if (has) {
    if (at < kFoldSlots) {
      f_root[grp][at] = r;
      f_min[grp][at] = fold;
    } else if (fold < vmin[r]) {  // (more roots in the group than slots: straight to the root)
      atomicMin(min_orig + r, fold);
    }
  }
  __syncthreads();
  if ((threadIdx.x & 255) < 64) {
    const bool mine = lane < min(f_cnt[grp], kFoldSlots);
    const int r1 = mine ? f_root[grp][lane] : -1;
    const int fold1 = wave_fold_by_root(mine, r1, mine ? f_min[grp][lane] : 0x7FFFFFFF);
    if (fold1 != 0x7FFFFFFF && fold1 < vmin[r1]) atomicMin(min_orig + r1, fold1);
  }
}

template <FlattenMode MODE>
__global__ __launch_bounds__(kFlagsThreads) void k_flatten_reps(const int4* __restrict__ list,
                                                      const int32_t* __restrict__ m_ptr,
                                                      int* parent, int max_steps /*kFlattenJump*/,
                                                      const int32_t* __restrict__ link2 /*kFlattenLink*/,
                                                      int32_t* __restrict__ seam /*the words launch, as below*/,
                                                      int32_t* __restrict__ pre, int32_t* __restrict__ pre_cnt,
                                                      int rep_blocks /*the hosting launch, as below*/, int n,
                                                      const uint8_t* __restrict__ core,
                                                      int32_t* __restrict__ rest, int32_t* __restrict__ rest_cnt,
                                                      const GridPlan* __restrict__ plan) {
  constexpr int kThreads = kFlagsThreads;
  static_assert(kThreads == 256, "the list is cut in 256s");
  if constexpr (MODE == kFlattenLink || MODE == kFlattenRoots) {
    // Two roles, by block index and independent of each other. The representatives' blocks come first, so
    // that their chains of dependent loads start at once; the blocks behind them do the flags role.
    if (int(blockIdx.x) >= rep_blocks) {
      if (plan->ok) flags_role(blockIdx.x - rep_blocks, n, core, rest, rest_cnt);
      return;
    }
  }
  const int m = *m_ptr;  // number of listed sub-cells, left on the device by k_sub_rep
  const int s = blockIdx.x * kThreads + threadIdx.x;
  const bool active = s < m;
  if constexpr (MODE == kFlattenJump || MODE == kFlattenLink) {
    if (!active) return;
  }
  int p = -1, r = -1, slot = -1;  // (slot: of the sub-cell's cell in the directory)
  if (active) {
    const int4 me = list[s];
    p = r = me.x;
    slot = me.z;
  }
  if constexpr (MODE == kFlattenJump) {
    int steps = 0;
    for (int nx = parent[r]; nx != r && steps < max_steps; nx = parent[r], ++steps) r = nx;
    if (r != p) parent[p] = r;
  } else if constexpr (MODE == kFlattenLink) {
    const int l = link2[s];
    int r2 = l >= 0 ? l : p;  // (no second link: the same chain twice, the second from the cache)
    for (;;) {
      const int a = parent[r], b = parent[r2];
      if (a == r && b == r2) break;
      r = a;
      r2 = b;
    }
    if (r != p) parent[p] = r;
    if (r2 != r) unite(parent, r, r2);
  } else {
    if (active) {
      for (int nx = parent[r]; nx != r; nx = parent[r]) r = nx;
      if (r != p) parent[p] = r;
    }
    const int lane = threadIdx.x & 63;
    // The list follows the sorted order within a block of k_sub_rep, so the sub-cells of a cell mostly sit
    // in neighbouring lanes: a lane whose predecessor brings the same root to the same word leaves the
    // atomic to it (the word depends only on the SET of roots folded into it).
    const int pc = __shfl_up(slot, 1, 64), pr = __shfl_up(r, 1, 64);
    const bool dup = lane != 0 && pc == slot && pr == r;
    if (active && !dup) {
      int* const word = seam + slot;
      const int old = atomicCAS(word, 0, r + 1);
      if (old != 0 && old != r + 1 && old != -1) *word = -1;
    }
    block_append<kThreads>(active && r == p, p, pre, pre_cnt);
  }
}

// Four sub-cells per wave in the two passes below, side by side in 16-lane groups: a wave per sub-cell
// (200 k waves of a few hundred cycles each per million points) was bound by the rate at which waves
// START (resident waves: 13-21 % of the slots), not by what they did.
static constexpr int kSubPerWave = 4;

// The sub-cell at half-cell offset -(dx, dy, dz) of the sub-cell (cx, cy, cz, octant) = at: its run
// [q0, q0 + n2) and its representative; rep < 0 where the lane is idle, the cell is empty or the
// sub-cell has no core point. Three dependent gathers (the directory word, the cell's slot, the
// record); a lane whose neighbour cell is empty stops after the word, whose bit says so.
// (What these kernels cost is the number of cache LINES their gathers touch — one per
// neighbouring cell and table, taken by the L1 a line at a time.)
struct SubNbr {
  int q0, n2, rep;
};
__device__ __forceinline__ SubNbr sub_neighbour(bool active, const int4 at, int dx, int dy, int dz, int nx, int ny,
                                                const CellDir& dir, const int4* __restrict__ rec) {
  // half-cell coordinates (cell 1 is the first interior cell; borders are empty)
  const int gx = 2 * (at.x - 1) + (at.w & 1) - dx, gy = 2 * (at.y - 1) + ((at.w >> 1) & 1) - dy,
            gz = 2 * (at.z - 1) + ((at.w >> 2) & 1) - dz;
  const int c2 = (((gz >> 1) + 1) * ny + ((gy >> 1) + 1)) * nx + ((gx >> 1) + 1);
  const int oct = (gx & 1) | ((gy & 1) << 1) | ((gz & 1) << 2);
  SubNbr out{0, 0, -1};
  DirWord w{0u, 0u};
  if (active) w = dir.words[c2 >> 5];
  if ((w.bits >> (c2 & 31)) & 1u) {
    const int b2 = dir.slots[CellDir::slot_of(w, c2)];
    const int4 r = rec[b2 * 8 + oct];
    if (r.y > 0) {
      out.q0 = r.x;
      out.n2 = r.y;
      out.rep = r.z;
    }
  }
  return out;
}

// Pass 1 of the union phase, without union-find: every sub-cell hangs itself under the
// first neighbour it is connected to among the 13 lexicographically NEGATIVE offsets of
// max-norm 1 (the first 13 of kSubOffsets). Pointers only go to lexicographically smaller
// sub-cells, so there is no cycle, and every sub-cell writes its own pointer only (plain store,
// no atomics, no chasing). A sub-cell that finds no such neighbour stays its own root: the pass
// only has to leave FEW trees, completeness is k_union_sub's business. What remains after
// compression is a few trees per cluster.
// Lane t < 13 of a group takes offset t, so one set of gathers serves the wave's four
// sub-cells; each group then tests its current candidate's point pairs 16 per step (the loop is
// wave-wide, the ballots are read per group), moves on when a candidate is exhausted and stops
// at the first hit: the hook.
// LINK2: the group then goes on through its remaining candidates in the same order to the next one that
// is connected as well, and records that one's representative as the sub-cell's second link (-1: none) for
// k_flatten_reps to unite across. Nothing is chased or united here: the chains are hundreds of links long
// while this pass runs.
// (Until this form the pass looked up all 62 offsets per sub-cell, four sub-cells one after the other,
// and wrote the neighbours found as a 256-byte row per sub-cell for pass 2: 197 002 candidates were
// tested for 196 884 sub-cells of the benchmark forest — the first one nearly always connects — and
// the table was the step's largest single piece of traffic.)
template <class CO, bool LINK2>
__global__ __launch_bounds__(256) void k_hook_sub(const int4* __restrict__ list,
                                                  const int4* __restrict__ list_xyz,
                                                  const int32_t* __restrict__ m_ptr,
                                                  const GridPlan* __restrict__ plan,
                                                  const DirWord* __restrict__ dwords,
                                                  const int32_t* __restrict__ dslots,
                                                  const int4* __restrict__ rec, CO co, double r2,
                                                  const uint8_t* __restrict__ core,
                                                  int* __restrict__ parent,
                                                  int32_t* __restrict__ link2 /*[m], LINK2 only*/,
    unsigned long long* __restrict__ st /*stamps or null*/) {
  stamped(st, [&] {
  const CellDir dir{dwords, dslots};
  if (!plan->ok) return;
  const int nx = plan->nx, ny = plan->ny;
  const int m = *m_ptr;
  const int k = threadIdx.x & 63;
  const int t = k & 15, grp = k >> 4;  // offset and sub-cell of the lane
  const int o_dx = t < 13 ? kSubOffsets[t][0] : 0, o_dy = t < 13 ? kSubOffsets[t][1] : 0,
            o_dz = t < 13 ? kSubOffsets[t][2] : 0;
  // resident waves stride over the list (wave-uniform bounds): the launch is sized for the chip, not
  // for the upper bound n of m — four waves in five of such a grid found nothing to do and still
  // had to be started (SQ_WAVES 250 k per million points for 49 k with work)
  for (int s0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * kSubPerWave; s0 < m; s0 += gridDim.x * 4 * kSubPerWave) {
    const bool live = s0 + grp < m;
    const int4 me = list[min(s0 + grp, m - 1)], at = list_xyz[min(s0 + grp, m - 1)];
    const SubNbr nb2 = sub_neighbour(live && t < 13, at, o_dx, o_dy, o_dz, nx, ny, dir, rec);
    const int p = me.x, n1 = me.w;
    // the group's candidates, nearest first; `base`: the pairs of the current one already tested
    unsigned todo = unsigned(__ballot(nb2.rep >= 0) >> (16 * grp)) & 0xFFFFu;
    int base = 0, hooked = -1, second = -1;
    while (__ballot(todo != 0)) {
      const int src = (k & 48) + (todo ? __ffs(todo) - 1 : 0);
      const int qb = __shfl(nb2.q0, src, 64), nb = __shfl(nb2.n2, src, 64), rb = __shfl(nb2.rep, src, 64);
      // pair (i, j) of the two runs sits at index (i << sh) | j, sh = bits of nb - 1: no division by a
      // run length per lane and step (~40 instructions), at the price of idle lanes where nb is no power of two
      const int sh = nb > 1 ? 32 - __clz(nb - 1) : 0;
      const int pairs = n1 << sh;
      const int idx = base + t;
      const int j = idx & ((1 << sh) - 1);
      bool hit = false;
      if (todo && idx < pairs && j < nb) hit = co.core_pair_within(p + (idx >> sh), qb + j, core, r2);
      const bool found = ((__ballot(hit) >> (16 * grp)) & 0xFFFFull) != 0;
      if (found) {
        if (LINK2 && hooked < 0) {  // on to the next candidate, for the second link
          hooked = rb;
          todo &= todo - 1;
          base = 0;
        } else {
          if (LINK2) second = rb; else hooked = rb;
          todo = 0;
        }
      } else if (todo) {
        base += 16;
        if (base >= pairs) {
          todo &= todo - 1;
          base = 0;
        }
      }
    }
    // Hang under the neighbour's own pointer rather than under the neighbour: sub-cells are
    // listed in spatial order, the smaller neighbour's wave has usually finished, and what
    // it points to is an ancestor still smaller than this sub-cell (no cycles). Chains come
    // out a few links long instead of as long as a trunk is tall in sub-cells.
    // (The chains are nevertheless long — 80 % of the benchmark forest's sub-cells sit more than 64
    // links from their root, PYQSM_DBSCAN_TRACE prints the histogram: a third of the list is in flight
    // at once, so most neighbours have not hooked yet when their pointer is read, and agent-scope
    // accesses here change nothing. k_flatten_reps deals with them in two passes.)
    if (hooked >= 0 && t == 0) parent[p] = parent[hooked];
    if (LINK2 && live && t == 0) link2[s0 + grp] = second;  // every slot below m, every call: the arena is reused
  }
  });
}

// All |S1| x |S2| point pairs of two runs, 64 per wave step: is one core-core pair within eps?
template <class CO>
__device__ __forceinline__ bool wave_pair_within(const CO& co, int p, int n1, int qb, int nb, int k,
                                                 const uint8_t* __restrict__ core, double r2) {
  const int sh = nb > 1 ? 32 - __clz(nb - 1) : 0;  // (as in k_hook_sub: shift and mask, no division)
  const int pairs = n1 << sh;
  bool found = false;
  for (int base = 0; base < pairs && !found; base += 64) {
    const int idx = base + k;
    const int j = idx & ((1 << sh) - 1);
    bool hit = false;
    if (idx < pairs && j < nb) hit = co.core_pair_within(p + (idx >> sh), qb + j, core, r2);
    found = __ballot(hit) != 0;
  }
  return found;
}

// The full treatment of ONE sub-cell by a wave: lane k looks up the neighbour at the k-th of the 62
// lexicographically negative offsets and decides whether it still has to be tested (two plain loads
// showing the same root say no); the wave then takes the ones that do one at a time and tests all
// |S1| x |S2| point pairs at once, 64 per step. (A lane per pair of sub-cells running the pair loop
// itself was 3x slower: ~25 dependent iterations per lane, and a wave lasts as long as its slowest lane.)
template <class CO>
__device__ __forceinline__ void seam_unite(const int4 me, const int4 at, int k, int o_dx, int o_dy, int o_dz,
                                           int nx, int ny, const CellDir& dir,
                                           const int4* __restrict__ rec, const CO& co, double r2,
                                           const uint8_t* __restrict__ core, int* parent) {
  const SubNbr nb2 = sub_neighbour(k < 62, at, o_dx, o_dy, o_dz, nx, ny, dir, rec);
  const int p = me.x, n1 = me.w, rep2 = nb2.rep;
  // A plain (cached, possibly stale) read names an ancestor; equal ancestors prove
  // "same tree" (trees only merge). The coherent chase is for the rest.
  const int* vparent = parent;
  int a1 = 0, a2 = 0;
  if (rep2 >= 0) {
    a1 = vparent[p];
    a2 = vparent[rep2];
  }
  bool need = rep2 >= 0 && !(a1 == a2 || a2 == p || a1 == rep2);
  int root2 = -1;  // the neighbour's tree, as the coherent look found it
  if (need) {
    // The coherent look: both chains at once, starting from the ancestors the plain reads named (after
    // the compression those are the roots unless this launch has hooked them since) — four dependent
    // agent-scope loads per doubtful pair became one or two.
    int ra = a1, rb = a2;
    for (;;) {
      const int pa = ld_parent(parent, ra), pb = ld_parent(parent, rb);
      if (pa == ra && pb == rb) break;
      ra = pa;
      rb = pb;
    }
    need = ra != rb;
    root2 = rb;
  }
  unsigned long long todo = __ballot(need);
  while (todo) {
    const int src = __ffsll(todo) - 1;
    todo &= todo - 1;
    const int qb = __shfl(nb2.q0, src, 64), nb = __shfl(nb2.n2, src, 64), rb = __shfl(rep2, src, 64);
    const int tree = __shfl(root2, src, 64);
    if (wave_pair_within(co, p, n1, qb, nb, k, core, r2)) {
      if (k == 0) unite(parent, p, rb);
      // this sub-cell now hangs together with that whole tree: its other doubtful neighbours in the same
      // tree need no test and no union (a sub-cell on the seam of two trees has ~7 of them, and a wave
      // went through them one after the other — test, two coherent finds, a CAS on the same hot root)
      todo &= ~__ballot(root2 == tree);
    }
  }
}

// Pass 2 joins the trees the hook pass left, and it is what makes the union phase COMPLETE: every
// unordered pair of neighbouring sub-cells sits at a lexicographically negative offset (dz, dy, dx; at
// most two half-cells per axis) of exactly one of the two. The sub-cells at the negative offsets of s lie
// in the 18 cells of s's own z-layer and the layer below: dz >= 0 keeps them out of the layer above, and
// with dz = 1 inside the own layer dy and dx are free. (NOT in "the cell and its 13 lexicographically
// smaller neighbours": offset (0, -2, 1) of an upper octant leads to the cell at y + 1 of the same layer.)
// Every listed sub-cell of a cell C looks at the SAME 18 cells, C among them, so whether its pairs can
// need a test is decided once per CELL, from the seam words alone (k_flatten_reps): when C's own word names
// a root r and each of the 18 words is 0 or names r too, every core sub-cell of those cells, C's own
// included, is in the tree r and no pair of C's sub-cells needs a test. C is a SEAM cell when its own word
// is mixed (-1) or one of the 18 names something else; every listed sub-cell of a seam cell gets
// seam_unite's 62 offsets, one sub-cell per wave step. The words are a snapshot taken at a kernel boundary
// and trees only merge: two sub-cells the snapshot shows in one tree stay in one tree, whatever this launch
// does meanwhile, and nothing but the snapshot enters the decision (no pointer that this launch moves).
// A wave takes 64 consecutive list entries. A cell's listed sub-cells are consecutive in the list (it
// follows the sorted order within a block of k_sub_rep), so the wave filters the LEADERS only, the entries
// whose predecessor has another cell, seven per step: nine lanes per leader, a lane per (x, y) column in
// both layers, two dependent gathers each (directory word, then the seam word at the cell's slot; a lane
// whose cell is empty stops after the first). The first entry of a wave's stretch always counts as a
// leader, and so does the first one after the end of a k_sub_rep block: a cell cut in two there or at a
// stretch's end is filtered twice with the same answer, and each of its entries belongs to exactly one run.
// (Until this form the filter ran per sub-cell, 197 k times for the benchmark forest's ~60 k cells, with
// three dependent gathers per cell — the last one into the sub-cell records, a line of its own per cell —
// and a gather of the sub-cell's pointer: 19.9 us for 86 seam sub-cells. Before that every sub-cell put
// all its neighbours, 6 million pairs on the benchmark forest, through two parent gathers each, from the
// table the hook pass wrote: 21 of the pass's 32 us, for 15 800 doubtful pairs in 2 200 sub-cells.)
// The seam entries a block's waves find go on a list in LDS, and the block's sixteen waves then take them in
// turn: seam cells lie side by side, a seam sub-cell is a chain of some twenty dependent memory accesses, and
// with every wave treating what it had found itself the one whose stretch held a seam's cells set the
// launch's time (filter alone 6.4 us on the benchmark forest, with its 86 seam sub-cells 18 us).
static constexpr int kSeamStretch = 64;   // list entries per wave step
static constexpr int kSeamThreads = 1024;  // ... and per block step
template <class CO>
__global__ __launch_bounds__(kSeamThreads) void k_union_sub(const int4* __restrict__ list,
                                                   const int4* __restrict__ list_xyz,
                                                   const int32_t* __restrict__ m_ptr,
                                                   const GridPlan* __restrict__ plan,
                                                   const DirWord* __restrict__ dwords,
                                                   const int32_t* __restrict__ dslots,
                                                   const int32_t* __restrict__ seam,
                                                   const int4* __restrict__ rec, CO co, double r2,
                                                   const uint8_t* __restrict__ core, int* parent,
                                                   int seam_blocks, const int* __restrict__ run_min,
                                                   int* min_orig,
                                                   unsigned long long* __restrict__ seam_cnt /*trace or null*/,
    unsigned long long* __restrict__ st /*stamps or null*/) {
  __shared__ int todo_list[kSeamThreads], todo_cnt;
  stamped(st, [&] {
  const CellDir dir{dwords, dslots};
  if (!plan->ok) return;
  const int nx = plan->nx, ny = plan->ny;
  const int m = *m_ptr;
  // Two roles, by block index and independent of each other: the seams' blocks first, so that their chains
  // of dependent accesses start at once; the blocks behind them fold the smallest indices (fold_role).
  if (int(blockIdx.x) >= seam_blocks) {
    fold_role<kSeamThreads>((blockIdx.x - seam_blocks) * kSeamThreads + threadIdx.x, m, list, parent, run_min,
                            min_orig);
    return;
  }
  const int k = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int o_dx = k < 62 ? kSubOffsets[k][0] : 0, o_dy = k < 62 ? kSubOffsets[k][1] : 0,
            o_dz = k < 62 ? kSubOffsets[k][2] : 0;
  // the filter's groups: lane j of group g9 < 7 takes the column (j % 3 - 1, j / 3 - 1) of the group's cell,
  // in the own layer and the one below (lane 63 idles there)
  const int g9 = k / 9, j = k % 9;
  const int c_off = (j % 3 - 1) + (j / 3 - 1) * nx;
  const int layer = nx * ny;
  for (int b0 = blockIdx.x * kSeamThreads; b0 < m; b0 += seam_blocks * kSeamThreads) {  // block-uniform
    if (threadIdx.x == 0) todo_cnt = 0;
    __syncthreads();
    const int s0 = b0 + wv * kSeamStretch;
    const bool live = s0 + k < m;
    const int cell = live ? list[s0 + k].y : -1;
    const int before = __shfl_up(cell, 1, 64);
    const unsigned long long leaders = __ballot(live && (k == 0 || before != cell));
    unsigned long long rem = leaders, seam_leaders = 0;
    while (rem) {  // wave-uniform: the next seven leaders
      unsigned long long mine = rem;  // ... the g9-th of them for this lane
#pragma unroll
      for (int i = 0; i < 6; ++i)
        if (i < g9) mine &= mine - 1;
      const bool act = g9 < 7 && mine != 0;
      const int src = act ? __ffsll(mine) - 1 : 0;
      const int c2 = __shfl(cell, src, 64) + c_off;  // (cells have a border of empty cells all round: c2 - layer - 1 >= 0)
      int word[2] = {0, 0};
      DirWord dw[2] = {{0u, 0u}, {0u, 0u}};
      if (act) {
#pragma unroll
        for (int l = 0; l < 2; ++l) dw[l] = dir.words[(c2 - l * layer) >> 5];
      }
#pragma unroll
      for (int l = 0; l < 2; ++l)
        if ((dw[l].bits >> ((c2 - l * layer) & 31)) & 1u) word[l] = seam[CellDir::slot_of(dw[l], c2 - l * layer)];
      const int own = __shfl(word[0], g9 * 9 + 4, 64);  // the group's cell itself: column (0, 0), own layer
      const unsigned long long bad = __ballot(
          act && (own == -1 || (word[0] != 0 && word[0] != own) || (word[1] != 0 && word[1] != own)));
#pragma unroll
      for (int g = 0; g < 7; ++g) {
        if ((bad >> (9 * g)) & 0x1FFull) seam_leaders |= rem & (~rem + 1ull);  // the g-th leader of this step
        rem &= rem - 1;
      }
    }
    if (seam_leaders) {  // wave-uniform
      // the entries of the seam cells' runs: a lane's leader is the last one at or before it (lane 0 is one)
      const int leader = 63 - __clzll(leaders & (~0ull >> (63 - k)));
      const bool take = live && ((seam_leaders >> leader) & 1ull);
      const unsigned long long todo = __ballot(take);
      int at = 0;
      if (k == 0) at = atomicAdd(&todo_cnt, __popcll(todo));
      at = __shfl(at, 0, 64);
      if (take) todo_list[at + __popcll(todo & ((1ull << k) - 1ull))] = s0 + k;
    }
    __syncthreads();
    const int cnt = todo_cnt;
    if (seam_cnt && threadIdx.x == 0 && cnt) atomicAdd(seam_cnt, static_cast<unsigned long long>(cnt));
    for (int i = wv; i < cnt; i += kSeamThreads / 64) {  // wave-uniform
      const int s = __builtin_amdgcn_readfirstlane(todo_list[i]);
      seam_unite(list[s], list_xyz[s], k, o_dx, o_dy, o_dz, nx, ny, dir, rec, co, r2, core, parent);
    }
    __syncthreads();  // the list is rewritten in the next step
  }
  });
}

// ---- fallback for coarsened grids ----------------------------------------------------
// When the cloud's extent would need more than 2^28 cells of edge eps, grid.hip doubles the
// edge; a sub-cell is then wider than eps and says nothing about connectivity. Such clouds
// take the per-point union-find of the first version (same results, ~3x slower union phase).
template <class CO>
__global__ __launch_bounds__(256) void k_union_points(int n, Stencil st,
                                                      const DirWord* __restrict__ dwords,
                                                      const int32_t* __restrict__ dslots,
                                                      const int32_t* __restrict__ cell_of, CO co, double r2,
                                                      const uint8_t* __restrict__ core, int* parent) {
  const CellDir dir{dwords, dslots};
  int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n || !core[p]) return;
  double x, y, z;
  co.get(p, x, y, z);
  const int c = cell_of[p];
  const volatile int* vparent = parent;
  int rp = find_root(parent, p);
  FOR_STENCIL(c, st, dir, q, {
    // each unordered pair once; a plain read equal to p's root proves "same tree"
    if (q < p && core[q] && co.d2(q, x, y, z) <= r2) {
      if (vparent[q] != rp) {
        unite(parent, p, q);
        rp = find_root(parent, p);
      }
    }
  })
}

// parent[p] = root for every core point (the per-point union-find's trees)
__global__ __launch_bounds__(256) void k_flatten(int n, const uint8_t* __restrict__ core,
                                                 int* __restrict__ parent, const GridPlan* __restrict__ plan) {
  int p = blockIdx.x * 256 + threadIdx.x;
  if (!plan->ok || p >= n || !core[p]) return;
  int r = p;
  for (int nx = parent[r]; nx != r; nx = parent[r]) r = nx;
  parent[p] = r;  // benign: r is still an ancestor for concurrent readers
}

// The same as a launch of its own: the per-point union-find's path.
__global__ __launch_bounds__(kFlagsThreads) void k_noncore_list(int n, const uint8_t* __restrict__ core,
                                                                int32_t* __restrict__ rest,
                                                                int32_t* __restrict__ rest_cnt,
                                                                const GridPlan* __restrict__ plan) {
  if (!plan->ok) return;  // block-uniform
  flags_role(blockIdx.x, n, core, rest, rest_cnt);
}

// k_flatten ran: parent[p] is the root. Folds the components' smallest original indices and lists the roots.
__global__ __launch_bounds__(256) void k_point_min(int n, const uint8_t* __restrict__ core,
                                                   const int* __restrict__ parent,
                                                   const int32_t* __restrict__ order,
                                                   int* __restrict__ min_orig,
                                                   int32_t* __restrict__ roots,
                                                   int32_t* __restrict__ roots_cnt,
                                                   const GridPlan* __restrict__ plan) {
  int p = blockIdx.x * 256 + threadIdx.x;
  const bool is_c = plan->ok && p < n && core[p];
  if (is_c) atomicMin(min_orig + parent[p], order[p]);
  block_append<256>(is_c && parent[p] == p, p, roots, roots_cnt);
}

// After the seams: only the PRE-ROOTS (k_flatten_reps) can have got a parent since the words launch knew
// every representative's root, so only they are chased again — 23 on the benchmark forest, where a launch
// over all 197 k representatives did this before (k_rep_root). A pre-root q that is still its own root is a
// component: it goes on the list of roots that k_number and the cluster count read. One that k_union_sub
// hooked hands the smallest index folded into it on to its final root f and points straight at f. Nobody
// folds into a pre-root that is not final (every chase ends at a final one), so the value read there is
// stable; the pointers written name ancestors. Every core point then reaches its component's smallest
// index in THREE hops: point -> representative -> pre-root -> root (a root points at itself), k_labels.
// Resident blocks stride over the list; its length is read here, nothing is sized by it on the host.
static constexpr int kFoldThreads = 256;
__global__ __launch_bounds__(kFoldThreads) void k_fold_roots(const int32_t* __restrict__ pre,
                                                             const int32_t* __restrict__ pre_cnt,
                                                             int* parent, int* min_orig,
                                                             int32_t* __restrict__ roots,
                                                             int32_t* __restrict__ roots_cnt,
                                                             const GridPlan* __restrict__ plan) {
  if (!plan->ok) return;  // block-uniform
  const int m = *pre_cnt;
  for (int i0 = blockIdx.x * kFoldThreads; i0 < m; i0 += gridDim.x * kFoldThreads) {  // block-uniform
    const int i = i0 + threadIdx.x;
    int q = -1, f = -1;
    if (i < m) {
      q = f = pre[i];
      for (int nx = parent[f]; nx != f; nx = parent[f]) f = nx;
      if (f != q) {
        atomicMin(min_orig + f, min_orig[q]);
        parent[q] = f;
      }
    }
    block_append<kFoldThreads>(i < m && f == q, q, roots, roots_cnt);
  }
}

// Cluster number = rank of the component's smallest original index among all components'. Up to kRankCap
// components (the forest has 20) one workgroup sorts the roots by that index in LDS and overwrites each
// root's min_orig with its number. Beyond it the numbering must not depend on the count of components: every
// block marks its share of the smallest indices in a bitmap of n bits, and the last block to finish writes
// the exclusive prefix of the bitmap's word popcounts; a number is then that prefix plus a popcount within the
// word (cluster_number). Which of the two is decided here on the device, from the root count, and the label
// passes read the same count. (It replaces a flag per point and a three-launch scan over n + 1 words.)
static constexpr int kRankCap = 4096;
static constexpr int kNumberThreads = 1024;

__global__ __launch_bounds__(kNumberThreads) void k_number(int n, const int32_t* __restrict__ roots,
                                                           const int32_t* __restrict__ roots_cnt,
                                                           int* __restrict__ min_orig,
                                                           uint32_t* __restrict__ bits /*zeroed, n / 32 + 1*/,
                                                           int32_t* __restrict__ wpre /*n / 32 + 1*/,
                                                           int32_t* __restrict__ done /*zeroed*/,
                                                           const GridPlan* __restrict__ plan,
    unsigned long long* __restrict__ st /*stamps or null*/) {
  stamped(st, [&] {
  if (!plan->ok) return;
  const int R = *roots_cnt;
  const int t = threadIdx.x;
  if (R <= kRankCap) {
    if (blockIdx.x != 0) return;
    __shared__ unsigned long long key[kRankCap];
    int P = 2;
    while (P < R) P <<= 1;
    for (int i = t; i < P; i += kNumberThreads) {
      unsigned long long k = ~0ull;
      if (i < R) {
        const int r = roots[i];
        k = (static_cast<unsigned long long>(min_orig[r]) << 32) | static_cast<uint32_t>(r);
      }
      key[i] = k;
    }
    __syncthreads();
    // bitonic sort of P keys (the smallest indices are distinct: so are the keys)
    for (int k = 2; k <= P; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = t; i < P; i += kNumberThreads) {
          const int l = i ^ j;
          if (l > i) {
            const unsigned long long a = key[i], b = key[l];
            if ((a > b) == ((i & k) == 0)) {
              key[i] = b;
              key[l] = a;
            }
          }
        }
        __syncthreads();
      }
    for (int i = t; i < R; i += kNumberThreads) min_orig[static_cast<uint32_t>(key[i])] = i;
    return;
  }
  for (int i = blockIdx.x * kNumberThreads + t; i < R; i += gridDim.x * kNumberThreads) {
    const int v = min_orig[roots[i]];
    __hip_atomic_fetch_or(bits + (v >> 5), 1u << (v & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // the last block to get here sees every mark
  __shared__ int last;
  __threadfence();
  __syncthreads();
  if (t == 0) last = atomicAdd(done, 1) == int(gridDim.x) - 1;
  __syncthreads();
  if (!last) return;
  __threadfence();
  // exclusive prefix of the words' popcounts, 16 consecutive words per thread and round
  __shared__ int wsum[kNumberThreads / 64];
  const int lane = t & 63, wv = t >> 6;
  const int nw = n / 32 + 1;
  int carry = 0;
  for (int w0 = 0; w0 < nw; w0 += 16 * kNumberThreads) {
    const int i0 = w0 + 16 * t;
    int cnt[16], sum = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      cnt[k] = i0 + k < nw ? __popc(__hip_atomic_load(bits + i0 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) : 0;
      sum += cnt[k];
    }
    int incl = sum;  // inclusive scan over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int before = carry, total = 0;
    for (int k = 0; k < kNumberThreads / 64; ++k) {
      before += k < wv ? wsum[k] : 0;
      total += wsum[k];
    }
    int run = before + incl - sum;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (i0 + k < nw) {
        wpre[i0 + k] = run;
        run += cnt[k];
      }
    carry += total;
    __syncthreads();  // wsum is rewritten next round
  }
  });
}

// The cluster number of a component from what k_number left in min_orig[root] (or the smallest index of the
// component's points among its neighbours, for the border pass: the numbering keeps the order of the indices).
__device__ __forceinline__ int cluster_number(int v, int n_roots, const uint32_t* __restrict__ bits,
                                              const int32_t* __restrict__ wpre) {
  if (n_roots <= kRankCap) return v;  // already the number
  return wpre[v >> 5] + __popc(bits[v >> 5] & ((1u << (v & 31)) - 1u));
}

// The label pass, two roles in one launch. Core points copy their cluster number (point -> representative ->
// pre-root -> root, k_fold_roots; the per-point union-find's points name their root at once, and a root
// names itself, so three hops serve every path): a thread each, one scattered store, and every point's core flag goes out in the caller's order beside
// it. Then every wave takes the entries wave, wave + waves of the grid, ... of the list of non-core points
// (flags_role): a WAVE per point (kRunBatch points' bounds looked up together, as in k_core_rest), the smallest
// cluster number among the core neighbours in its stencil, or -1.
// The roles do not wait on each other and cannot race: the first writes the labels of core points only, the
// second those of non-core points only, and both only read core / parent / min_orig. (DESIGN section 4 has the
// forms measured and dropped.)
static constexpr int kLabelThreads = 256;
template <class CO>
__global__ __launch_bounds__(kLabelThreads) void k_labels(int n, const int32_t* __restrict__ rest,
                                                          const int32_t* __restrict__ rest_cnt,
                                                          const GridPlan* __restrict__ plan,
                                                          const DirWord* __restrict__ dwords,
                                                          const int32_t* __restrict__ dslots,
                                                          const int32_t* __restrict__ cell_of, CO co, double r2,
                                                          const uint8_t* __restrict__ core,
                                                          const int* __restrict__ parent,
                                                          const int* __restrict__ min_orig,
                                                          const int32_t* __restrict__ roots_cnt,
                                                          const uint32_t* __restrict__ bits,
                                                          const int32_t* __restrict__ wpre,
                                                          const int32_t* __restrict__ order,
                                                          int64_t* __restrict__ labels,
                                                          uint8_t* __restrict__ is_core,
    unsigned long long* __restrict__ st /*stamps or null*/) {
  stamped(st, [&] {
  const CellDir dir{dwords, dslots};
  if (!plan->ok) return;  // block-uniform
  constexpr int kWaves = kLabelThreads / 64;
  const int n_roots = *roots_cnt;
  const int lane = threadIdx.x & 63;
  {
    const int p = blockIdx.x * kLabelThreads + threadIdx.x;
    const bool is_c = p < n && core[p];
    if (is_c) {
      const int v = min_orig[parent[parent[parent[p]]]];
      labels[order[p]] = int64_t(cluster_number(v, n_roots, bits, wpre));
    }
    if (p < n && is_core) is_core[order[p]] = is_c;
  }
  const int m = *rest_cnt;
  const Stencil sten = plan_stencil(plan);
  const int first = (blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * kRunBatch;
  const int grp = lane / 18, j = lane % 18;  // (as k_core_rest: three points' bounds per gather)
  for (int i0 = first; i0 < m; i0 += gridDim.x * kWaves * kRunBatch) {  // wave-uniform
    const bool act = grp < kRunBatch && i0 + grp < m;
    double x = 0.0, y = 0.0, z = 0.0;
    int p = 0, c = 0;
    if (act) {
      p = rest[i0 + grp];
      co.get(p, x, y, z);
      c = cell_of[p];
    }
    const int bound = lane_bound(act, c, j, sten, dir);
#pragma unroll
    for (int k = 0; k < kRunBatch; ++k) {
      if (i0 + k >= m) break;  // wave-uniform
      const Runs9 t = runs_of_lanes(bound, k);
      const int pk = __builtin_amdgcn_readlane(p, 18 * k);
      const double xk = __shfl(x, 18 * k, 64), yk = __shfl(y, 18 * k, 64), zk = __shfl(z, 18 * k, 64);
      int best = kNoRoot;
      for (int g0 = 0; g0 < t.pre[9]; g0 += 64) {
        const int g = g0 + lane;
        if (g < t.pre[9]) {
          const int q = t.at(g);
          if (core[q] && co.d2(q, xk, yk, zk) <= r2) {
            const int mo = min_orig[parent[parent[parent[q]]]];
            best = mo < best ? mo : best;
          }
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(best, off, 64);
        best = o < best ? o : best;
      }
      if (lane == 0)
        labels[order[pk]] = best == kNoRoot ? int64_t(-1) : int64_t(cluster_number(best, n_roots, bits, wpre));
    }
  }
  });
}

// The squared radius every kernel compares with (cluster_binned says why the strict rule is this one).
static double dbscan_r2(double eps, bool radius_inclusive) {
  return radius_inclusive ? eps * eps : nextafter(eps * eps, 0.0);
}

// Core flags, union-find and labels over a binned cloud. The kernels read the grid from d_plan.
// *count_out: where the number of clusters lies on the device once the step has run.
static int cluster_binned(Ctx* c, int64_t n, double eps, int32_t min_pts, bool radius_inclusive, const DevGrid& g,
                          const SubCells& sub, const GridPlan* d_plan, int64_t* labels, uint8_t* is_core,
                          const int32_t** count_out) {
  // the sub-cell shortcuts need cells of edge eps (not doubled to fit the dense grid)
  const bool fine = g.cell <= eps * (1.0 + 1.0 / 524288.0);
  const int N = int(n);
  const dim3 grid(ceil_div(n, 256)), block(256);
  const Stencil st{g.nx, g.nx * g.ny};  // (host-planned grids only: k_union_points)
  const CellDir dir = cell_dir(g);
  // Every kernel tests d2 <= r2. The STRICT neighbourhood d2 < eps^2 (radius_inclusive = 0: what
  // Open3D's cluster_dbscan computes if nanoflann's radius search compares strictly; SURVEY.md
  // §8 a2) is the same test against the double just below eps^2 — no fp64 value lies between
  // the two, so d2 < r2 <=> d2 <= pred(r2) exactly, and the kernels need no second form.
  const double r2 = dbscan_r2(eps, radius_inclusive);
  uint8_t* core;
  int *parent, *min_orig;
  // [n / 32 + 1] the bitmap of k_number's large-count numbering, [1] the number of pre-roots (k_flatten_reps,
  // k_fold_roots): zeroed by k_core_tiled
  uint32_t* bits;
  PQ_TRY(c->arena.get(size_t(n), &core));
  PQ_TRY(c->arena.get(size_t(n), &parent));
  PQ_TRY(c->arena.get(size_t(n), &min_orig));
  PQ_TRY(c->arena.get(size_t(n / 32) + 2, &bits));
  int32_t* const pre_cnt = reinterpret_cast<int32_t*>(bits + n / 32 + 1);
  // The cells' seam words (k_flatten_reps), one per slot of the ranked directory: a slot index stays below
  // n + buckets + 1 from the two-level sort (a bucket has at least 2^12 cells) and below n + words + 1 of a
  // directory made from a dense one (grid.hip). k_core_tiled zeroes the first kind, n stores and a few
  // more; the second, the rare paths' with up to 2^23 words, takes a memset.
  // (The per-point union-find of a doubled grid has no use for them.)
  const size_t seam_cap = fine ? size_t(n) + size_t(g.start ? g.ncell >> 5 : g.ncell >> 12) + 3 : 0;
  int32_t *seam, *pre;  // ... and the list of the pre-roots
  PQ_TRY(c->arena.get(seam_cap, &seam));
  PQ_TRY(c->arena.get(size_t(n), &pre));
  if (fine && g.start) PQ_HIP(hipMemsetAsync(seam, 0, seam_cap * 4, c->stream));
  int32_t *roots, *wpre;  // the components' roots; k_number's word prefix (n / 32 + 1)
  PQ_TRY(c->arena.get(size_t(n), &roots));
  PQ_TRY(c->arena.get(size_t(n / 32) + 1, &wpre));
  int4* list;
  int32_t* list_cnt;
  int* run_min;
  PQ_TRY(c->arena.get(size_t(n), &run_min));
  PQ_TRY(c->arena.get(size_t(n), &list));
  int4* list_xyz;  // [n] grid coordinates and octant of every listed sub-cell
  PQ_TRY(c->arena.get(size_t(n), &list_xyz));
  int32_t* link2;  // [n] second link of every listed sub-cell (k_hook_sub), indexed like list
  PQ_TRY(c->arena.get(size_t(n), &link2));
  // [0] listed sub-cells, [1] roots (= clusters), [2] blocks k_number has seen finish, [3] non-core
  // points of the label pass. The binning leaves four zeroed ints behind for this (no memset launches).
  list_cnt = sub.zeroed4;
  int32_t* const roots_cnt = list_cnt + 1;
  int32_t* rest;
  // (the core pass's stragglers come in kRestSegs segments of seg_cap entries; the label pass reuses the
  // array as one list of at most n)
  const int core_blocks = int(ceil_div(n, 256));
  const int seg_cap = ceil_div(core_blocks, kRestSegs) * 256;
  PQ_TRY(c->arena.get(std::max<size_t>(size_t(n), size_t(seg_cap) * kRestSegs), &rest));
  int32_t* const rest_segs = list_cnt + 4;  // kRestSegs zeroed counters
  {
    StampScope ps(c, "dbscan_core");
    unsigned long long* d_tests = nullptr;
    if (c->prof >= 2) {
      PQ_TRY(c->arena.get(512, &d_tests));  // [256] candidates staged, [256] lanes handed on out of the band
      PQ_HIP(hipMemsetAsync(d_tests, 0, 512 * 8, c->stream));
    }
    // chunks of 64 candidates a wave of the tiled pass looks at before it hands its short lanes on: three
    // serve min_pts = 10, and in proportion beyond
    const int max_chunks = std::min(32, std::max(kMaxChunks, (kMaxChunks * min_pts + 9) / 10));
    {
      const StampKernel pk(c, "k_core_tiled", grid.x);
      // fp32 records and an eps whose band neither underflows nor overflows: decide in fp32, fp64 only in the
      // band (core_band), counted with the ramps (core_ramp); anything else runs the fp64 kernel
      const CoreRamp cr = core_ramp(r2);
      const bool f32 = cr.usable(min_pts);
      on_coords(g, [&](auto co) {
        const auto launch = [&](auto kernel) {
          hipLaunchKernelGGL(kernel, grid, block, 0, c->stream, N, d_plan, dir.words, dir.slots, g.cell_of, co, r2, -cr.K,
                             cr.A, cr.B, min_pts, core, rest, rest_segs, seg_cap, parent, min_orig, bits, seam,
                             g.start ? 0 : int(seam_cap), max_chunks, d_tests, pk.slots);
        };
        if constexpr (std::is_same_v<decltype(co), CoordsF32>) {
          if (f32) return launch(k_core_tiled<CoordsF32, true>);
        }
        launch(k_core_tiled<decltype(co), false>);
      });
    }
    if (d_tests) {  // profiling level 2 only: read the counters back (synchronises)
      unsigned long long h[512];
      PQ_TRY(fetch(c, h, d_tests, 512));
      unsigned long long tot = 0, band = 0;
      for (int i = 0; i < 256; ++i) tot += h[i], band += h[256 + i];
      c->timers["core_pair_tests"].launches += int64_t(tot) * 64;  // lane-tests executed
      c->timers["core_band_lanes"].launches += int64_t(band);      // lanes handed to fp64 with a distance in the band
    }
    const dim3 gr(std::min<int64_t>(8192, ceil_div(n, 64)));
    unsigned long long* const st_rest = stamp_slots(c, gr.x);
    on_coords(g, [&](auto co) {
      hipLaunchKernelGGL(k_core_rest<decltype(co)>, gr, block, 0, c->stream, rest, rest_segs, seg_cap, d_plan, dir.words, dir.slots,
                         g.cell_of, co, r2, min_pts, core, st_rest);
    });
    PQ_HIP(hipGetLastError());
    if (getenv("PYQSM_DBSCAN_TRACE")) {  // how many points did the tiled pass hand on?
      int32_t h[kRestSegs];
      PQ_TRY(fetch(c, h, rest_segs, kRestSegs));
      long long tot = 0;
      for (int32_t v : h) tot += v;
      fprintf(stderr, "core pass: %lld stragglers\n", tot);
    }
  }
  {
    StampScope ps(c, "dbscan_union");
    const dim3 gf(ceil_div(n, kFlagsPerBlock));  // blocks of flags_role
    // (parent / min_orig / bits / seam / pre_cnt were initialised by k_core_tiled; list_cnt[0..2] are still
    // the zeros the binning left)
    if (fine) {
      hipLaunchKernelGGL(k_sub_rep, dim3(ceil_div(n, 1024)), dim3(1024), 0, c->stream, N, sub.sub_of, core,
                         g.order, parent, g.cell_of, sub.rec, run_min, list, list_cnt, d_plan, list_xyz, dir.words,
                         stamp_slots(c, ceil_div(n, 1024)));
      // The number m of listed sub-cells stays on the device: the passes below are launched for the
      // upper bound n (a sub-cell holds at least one point, in practice ~5) and read m themselves —
      // waves beyond it leave at once — which spares the host round trip in the middle of the step
      // (~15 us of an 0.7 ms step). Nothing in the phase is sized by m any more.
      {
        // PYQSM_DBSCAN_LINK2=0: the sequence without second links (no second search in the hook pass, two
        // compression launches, the words written by the second)
        static const bool use_link2 = [] {
          const char* e = getenv("PYQSM_DBSCAN_LINK2");
          return e ? atoi(e) != 0 : true;
        }();
        // the two wave-per-four-sub-cells passes: resident waves striding over the list, 8 (hook; 16 without
        // the second search) and 32 (union) blocks per CU (PYQSM_UNION_BLOCKS_PER_CU=<hook>,<union>; 0 = a
        // block per 16 rows of the bound n, which starts four waves in five for nothing). Eight blocks are what
        // a CU holds of either kernel: the hook pass with its second search is shortest when no wave waits for
        // a slot (30.5 us against 32.8 with 16 and 36.3 with 6); the union pass, mostly its filter, was the
        // same 20-22 us with 8, 16, 32 and 64 when it filtered per sub-cell. (It takes kSeamThreads list
        // entries per block step now, so its bound grid is a block per kSeamThreads rows of n.)
        int per_cu[2] = {use_link2 ? 8 : 16, 32};
        if (const char* e_cu = getenv("PYQSM_UNION_BLOCKS_PER_CU")) {
          per_cu[0] = per_cu[1] = atoi(e_cu);
          if (const char* comma = strchr(e_cu, ',')) per_cu[1] = atoi(comma + 1);
        }
        const int64_t full = ceil_div(n, 4 * kSubPerWave), full_u = ceil_div(n, kSeamThreads);
        const int64_t cu_u = std::max(1, per_cu[1] * 256 / kSeamThreads);  // (the figure counts blocks of 256 threads)
        const dim3 gh(per_cu[0] > 0 ? std::min<int64_t>(full, int64_t(c->cu_count) * per_cu[0]) : full),
            gu(per_cu[1] > 0 ? std::min<int64_t>(full_u, int64_t(c->cu_count) * cu_u) : full_u);
        const bool trace = getenv("PYQSM_DBSCAN_TRACE") != nullptr;
        {
          const StampKernel pk(c, "k_hook_sub", gh.x);
          on_coords(g, [&](auto co) {
            if (use_link2)
              hipLaunchKernelGGL((k_hook_sub<decltype(co), true>), gh, block, 0, c->stream, list, list_xyz, list_cnt,
                                 d_plan, dir.words, dir.slots, sub.rec, co, r2, core, parent, link2, pk.slots);
            else
              hipLaunchKernelGGL((k_hook_sub<decltype(co), false>), gh, block, 0, c->stream, list, list_xyz, list_cnt,
                                 d_plan, dir.words, dir.slots, sub.rec, co, r2, core, parent, link2, pk.slots);
          });
        }
        // trace only: the list and the pointers on the host, every listed sub-cell's root and depth
        int32_t tm = 0;
        std::vector<int32_t> hp, root_of;
        std::vector<int4> hl;
        const auto snapshot = [&](std::vector<int64_t>* hist) -> int {
          PQ_TRY(fetch(c, &tm, list_cnt));
          hp.assign(static_cast<size_t>(n), 0);
          hl.assign(static_cast<size_t>(tm), make_int4(0, 0, 0, 0));
          PQ_HIP(hipMemcpy(hp.data(), parent, size_t(n) * 4, hipMemcpyDeviceToHost));
          PQ_HIP(hipMemcpy(hl.data(), list, size_t(tm) * 16, hipMemcpyDeviceToHost));
          root_of.assign(static_cast<size_t>(n), -1);
          for (int32_t s2 = 0; s2 < tm; ++s2) {
            int d = 0, r = hl[size_t(s2)].x;
            while (hp[size_t(r)] != r) {
              r = hp[size_t(r)];
              ++d;
            }
            root_of[size_t(hl[size_t(s2)].x)] = r;
            if (hist) (*hist)[size_t(std::min(d, 65))]++;
          }
          return 0;
        };
        const auto count_roots = [&] {
          int64_t roots = 0;
          for (int32_t s2 = 0; s2 < tm; ++s2) roots += root_of[size_t(hl[size_t(s2)].x)] == hl[size_t(s2)].x;
          return roots;
        };
        int64_t links = 0, crossing = 0;
        if (trace) {  // how deep are the chains the hook pass leaves?
          std::vector<int64_t> hist(66, 0);
          PQ_TRY(snapshot(&hist));
          fprintf(stderr, "hook pass: %d sub-cells, %lld roots; chain depth histogram:", tm, (long long)count_roots());
          for (int d = 0; d < 66; ++d)
            if (hist[size_t(d)]) fprintf(stderr, " %d:%lld", d, (long long)hist[size_t(d)]);
          fprintf(stderr, "\n");
          if (use_link2) {  // second links, and how many of them lead into another of the hook pass's trees
            std::vector<int32_t> h2(static_cast<size_t>(tm), -1);
            PQ_HIP(hipMemcpy(h2.data(), link2, size_t(tm) * 4, hipMemcpyDeviceToHost));
            for (int32_t s2 = 0; s2 < tm; ++s2) {
              if (h2[size_t(s2)] < 0) continue;
              ++links;
              crossing += root_of[size_t(h2[size_t(s2)])] != root_of[size_t(hl[size_t(s2)].x)];
            }
          }
        }
        static const int jump = [] {  // PYQSM_FLATTEN_JUMP: links of the first pass (0: one pass, the earlier form)
          const char* e = getenv("PYQSM_FLATTEN_JUMP");
          return e ? atoi(e) : 12;
        }();
        // one launch of k_flatten_reps; `host_flags`: with the label pass's list of non-core points in gf
        // blocks behind its own (flags_role)
        const auto flatten = [&](auto mode, int max_steps, bool host_flags) {
          constexpr int threads = kFlagsThreads;
          const int rep_blocks = int(ceil_div(n, threads));
          hipLaunchKernelGGL(k_flatten_reps<decltype(mode)::value>, dim3(rep_blocks + (host_flags ? gf.x : 0)),
                             dim3(threads), 0, c->stream, list, list_cnt, parent, max_steps, link2, seam,
                             pre, pre_cnt, rep_blocks, N, core, rest, list_cnt + 3, d_plan);
        };
        if (jump > 0) flatten(std::integral_constant<FlattenMode, kFlattenJump>{}, jump, false);
        if (use_link2) {
          // the pass that reaches the roots unites across the second links; a short third one then writes
          // the cells' seam words, folds the smallest indices and lists the pre-roots
          flatten(std::integral_constant<FlattenMode, kFlattenLink>{}, 0, true);
          if (trace) {
            PQ_TRY(snapshot(nullptr));
            fprintf(stderr, "link pass: %lld recorded, %lld crossed trees, %lld roots left\n", (long long)links,
                    (long long)crossing, (long long)count_roots());
          }
          flatten(std::integral_constant<FlattenMode, kFlattenWords>{}, 0, false);
        } else {
          // (the pass that reaches the roots is the words launch as well)
          flatten(std::integral_constant<FlattenMode, kFlattenRoots>{}, 0, true);
        }
        // what is left: joining the few trees per cluster along their seams
        unsigned long long* d_seams = nullptr;  // trace only: sub-cells that took the 62-offset path
        if (trace) {
          PQ_TRY(c->arena.get(1, &d_seams));
          PQ_HIP(hipMemsetAsync(d_seams, 0, 8, c->stream));
        }
        {
          const int fold_blocks = int(ceil_div(n, kSeamThreads));  // (fold_role behind the seams' blocks)
          const StampKernel pk(c, "k_union_sub", gu.x + fold_blocks);
          on_coords(g, [&](auto co) {
            hipLaunchKernelGGL(k_union_sub<decltype(co)>, dim3(gu.x + fold_blocks), dim3(kSeamThreads), 0, c->stream, list,
                               list_xyz, list_cnt, d_plan, dir.words, dir.slots, seam, sub.rec, co, r2, core, parent,
                               int(gu.x), run_min, min_orig, d_seams, pk.slots);
          });
        }
        if (trace) {
          unsigned long long h = 0;
          PQ_TRY(fetch(c, &h, d_seams));
          fprintf(stderr, "seam union: %llu sub-cells took the 62-offset path\n", h);
        }
        // the pre-roots the seams hooked hand their smallest index on; the others are the components
        const dim3 gp(std::min<int64_t>(ceil_div(n, kFoldThreads), int64_t(c->cu_count) * 8));
        hipLaunchKernelGGL(k_fold_roots, gp, dim3(kFoldThreads), 0, c->stream, pre, pre_cnt, parent, min_orig, roots,
                           roots_cnt, d_plan);
      }
      PQ_HIP(hipGetLastError());
    } else {
      PQ_TRY(stamp_mark(c));  // (the per-point union-find is not stamped itself)
      on_coords(g, [&](auto co) {
        hipLaunchKernelGGL(k_union_points<decltype(co)>, grid, block, 0, c->stream, N, st, dir.words, dir.slots, g.cell_of, co,
                           r2, core, parent);
      });
      hipLaunchKernelGGL(k_flatten, grid, block, 0, c->stream, N, core, parent, d_plan);
      hipLaunchKernelGGL(k_point_min, grid, block, 0, c->stream, N, core, parent, g.order, min_orig, roots,
                         roots_cnt, d_plan);
      hipLaunchKernelGGL(k_noncore_list, gf, dim3(kFlagsThreads), 0, c->stream, N, core, rest,
                         list_cnt + 3, d_plan);
    }
    // one workgroup numbers up to kRankCap clusters; more take the bitmap, a block per CU at most
    const dim3 gn(std::min<int64_t>(ceil_div(n, kNumberThreads), c->cu_count));
    hipLaunchKernelGGL(k_number, gn, dim3(kNumberThreads), 0, c->stream, N, roots, roots_cnt, min_orig, bits, wpre,
                       list_cnt + 2, d_plan, stamp_slots(c, gn.x));
    PQ_HIP(hipGetLastError());
  }
  {
    StampScope ps(c, "dbscan_label");
    const dim3 gb(ceil_div(n, kLabelThreads));
    unsigned long long* const st_labels = stamp_slots(c, gb.x);
    on_coords(g, [&](auto co) {
      hipLaunchKernelGGL(k_labels<decltype(co)>, gb, dim3(kLabelThreads), 0, c->stream, N, rest, list_cnt + 3, d_plan,
                         dir.words, dir.slots, g.cell_of, co, r2, core, parent, min_orig, roots_cnt, bits, wpre, g.order, labels,
                         is_core, st_labels);
    });
    PQ_HIP(hipGetLastError());
    if (getenv("PYQSM_DBSCAN_TRACE")) {
      int32_t h = 0;
      PQ_TRY(fetch(c, &h, list_cnt + 3));
      fprintf(stderr, "label pass: %d non-core points listed\n", h);
    }
  }
  *count_out = roots_cnt;
  return 0;
}


// The fold's plan in the host-mapped slot: a bounded poll of its sequence number (the fold runs within
// microseconds of the call unless the stream holds earlier work), then, when the bound runs out, the
// stream's synchronisation (which waits for the speculative step too).
static constexpr double kPlanPollMs = 20.0;
static int wait_plan(Ctx* c, const GridPlan* h_plan, unsigned seq) {
  const volatile unsigned* const s = &h_plan->seq;
  const auto t0 = std::chrono::steady_clock::now();
  while (*s != seq) {
    if (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > kPlanPollMs) {
      PQ_HIP(hipStreamSynchronize(c->stream));
      if (*s != seq) return fail(PYQSM_EHIP, "DBSCAN: the grid plan was not written (sequence %u)", seq);
      break;
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return 0;
}

// The bounding box's fold plans the grid on the device. With a shape hint (the last host-planned call
// of this context) the whole step is enqueued at once behind it, and the host waits only for the
// plan's read-back: when the plan fits the hint (ok) the call returns with the step queued and
// nothing synchronised. Otherwise the enqueued kernels leave without a write, and the step is
// planned on the host from the box already read back (what every call did before), which also
// covers axis-compressed and doubled grids, fp64 records, bits = 13 and non-finite input.
// PYQSM_DBSCAN_PLAN=host: the host plans every call (A/B comparisons). A missed speculation records
// its (empty) profiling scopes as well.
// `readout` (pyqsm_octant_directory): plan and bin as every call does, then, instead of clustering, hand
// back the grid's dims and the directory's begin(c) for c = 0 .. ncell as the device evaluates it.
struct DirReadout {
  int64_t cap;       // entries begin_host has room for
  int32_t* begin_host;
  int32_t dims[3];
};
static int dbscan_device(Ctx* c, const double* xyz, int64_t n, double eps, int32_t min_pts,
                         bool radius_inclusive, int64_t* labels, uint8_t* is_core, int64_t* n_clusters,
                         DirReadout* readout = nullptr) {
  if (!(eps > 0) || !std::isfinite(eps)) return fail(PYQSM_EINVAL, "eps must be positive");
  if (n == 0) {
    if (n_clusters) *n_clusters = 0;
    return 0;
  }
  // a hair wider than eps: rounding of the cell index can then never put two
  // points that are within eps of each other two cells apart
  const double cell = eps * (1.0 + 1.0 / 1048576.0);
  const int64_t max_cells = int64_t(1) << 28;
  if (!c->plan_pinned) {
    PQ_HIP(hipHostMalloc(&c->plan_pinned, 2 * sizeof(GridPlan), hipHostMallocMapped | hipHostMallocCoherent));
    memset(c->plan_pinned, 0, 2 * sizeof(GridPlan));
  }
  GridPlan* const h_plan = static_cast<GridPlan*>(c->plan_pinned);  // [0] read-back, [1] upload
  GridPlan* h_plan_dev;  // the read-back slot as the fold writes it
  PQ_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&h_plan_dev), c->plan_pinned, 0));
  if (++c->plan_seq == 0) c->plan_seq = 1;  // 0: the slot's value while the fold writes it
  const unsigned seq = c->plan_seq;
  GridPlan* d_plan;  // [0] the fold's, [1] the host's
  int32_t* zeroed;
  PQ_TRY(c->arena.get(2, &d_plan));
  PQ_TRY(c->arena.get(size_t(octant_zeroed_ints()), &zeroed));
  const char* plan_env = getenv("PYQSM_DBSCAN_PLAN");
  const char* bin_env = getenv("PYQSM_DBSCAN_BIN");
  const char* f32_env = getenv("PYQSM_COORD_F32");
  // (clouds beyond 2^25 points read the sub-cell count back in the union phase: planned on the host)
  const bool speculate = c->plan_hint.valid && !(plan_env && !strcmp(plan_env, "host")) && !bin_env &&
                         !(f32_env && !strcmp(f32_env, "0")) && n <= (int64_t(1) << 25);
  const PlanHint hint = speculate ? c->plan_hint : PlanHint{};
  DevGrid g;
  SubCells sub;
  const int32_t* count = nullptr;
  std::optional<StampScope> bin_scope(std::in_place, c, "dbscan_bin");
  // (speculated: no fold launch; the binning's first kernel plans from the box records and stores the plan)
  PlanRecords rec{};
  PQ_TRY(plan_grid_device(c, xyz, n, cell, max_cells, hint, d_plan, h_plan_dev, seq, zeroed, octant_zeroed_ints(),
                          speculate ? &rec : nullptr));
  const Arena::Mark mark = c->arena.mark();
  if (speculate) {
    PQ_TRY(bin_octants_planned(c, xyz, n, cell, hint, rec, d_plan, zeroed, &g, &sub));
    bin_scope.reset();
    if (!readout)
      PQ_TRY(cluster_binned(c, n, eps, min_pts, radius_inclusive, g, sub, d_plan, labels, is_core, &count));
  }
  PQ_TRY(wait_plan(c, h_plan, seq));
  const bool hit = speculate && h_plan[0].ok;
  if (!hit) {
    // planned on the host; the kernels enqueued above (if any) left without a write, so their
    // scratch memory can be handed out again
    c->arena.rewind(mark);
    PlanHint next;
    if (!bin_scope) bin_scope.emplace(c, "dbscan_bin");
    PQ_TRY(stamp_mark(c));  // (the host-planned binning's first and last kernels vary with the grid)
    PQ_TRY(bin_octants_host(c, xyz, n, cell, max_cells, h_plan[0], zeroed, &h_plan[1], d_plan + 1, &g, &sub, &next));
    PQ_TRY(stamp_mark(c));
    bin_scope.reset();
    if (next.valid) c->plan_hint = next;  // (a grid of another kind keeps the hint there is)
    if (!readout)
      PQ_TRY(cluster_binned(c, n, eps, min_pts, radius_inclusive, g, sub, d_plan + 1, labels, is_core, &count));
  }
  if (c->prof >= 1) {
    c->timers["dbscan_f32_records"].launches += g.p4 ? 1 : 0;  // which storage form ran
    c->timers[hit ? "dbscan_plan_hit" : "dbscan_plan_miss"].launches += 1;  // which planning ran
  }
  if (readout) {
    const GridPlan& pl = hit ? h_plan[0] : h_plan[1];  // the fold's plan, or the one the host uploaded
    readout->dims[0] = pl.nx;
    readout->dims[1] = pl.ny;
    readout->dims[2] = pl.nz;
    const int64_t entries = int64_t(pl.ncell) + 1;
    if (entries > readout->cap)
      return fail(PYQSM_ERANGE, "octant directory: %lld entries, room for %lld", (long long)entries,
                  (long long)readout->cap);
    int32_t* d_begin;
    PQ_TRY(c->arena.get(size_t(entries), &d_begin));
    read_directory(c, g, pl.ncell, d_begin);
    PQ_HIP(hipGetLastError());
    PQ_TRY(fetch(c, readout->begin_host, d_begin, size_t(entries)));
    return 0;
  }
  if (n_clusters) {
    int32_t h = 0;
    PQ_TRY(fetch(c, &h, count));
    *n_clusters = h;
  }
  return 0;
}

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_dbscan_dev_ex(const double* xyz_dev, int64_t n, double eps, int32_t min_pts,
                        int32_t radius_inclusive, int64_t* labels_dev, uint8_t* is_core_dev,
                        int64_t* n_clusters, int32_t device) {
  PQ_API_RANGE("pyqsm_dbscan_dev");
  if (n < 0) return fail(PYQSM_EINVAL, "negative size");
  if (n > 0 && (!xyz_dev || !labels_dev)) return fail(PYQSM_EINVAL, "pyqsm_dbscan_dev: NULL pointer");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  StampScope ps(c, "dbscan_total");
  return dbscan_device(c, xyz_dev, n, eps, min_pts, radius_inclusive != 0, labels_dev, is_core_dev,
                       n_clusters);
}

int pyqsm_dbscan_dev(const double* xyz_dev, int64_t n, double eps, int32_t min_pts,
                     int64_t* labels_dev, uint8_t* is_core_dev, int64_t* n_clusters,
                     int32_t device) {
  return pyqsm_dbscan_dev_ex(xyz_dev, n, eps, min_pts, 1, labels_dev, is_core_dev, n_clusters, device);
}

int pyqsm_dbscan(const double* xyz, int64_t n, double eps, int32_t min_pts, int64_t* labels,
                 uint8_t* is_core, int32_t device) {
  return pyqsm_dbscan_ex(xyz, n, eps, min_pts, 1, labels, is_core, device);
}

int pyqsm_dbscan_ex(const double* xyz, int64_t n, double eps, int32_t min_pts, int32_t radius_inclusive,
                    int64_t* labels, uint8_t* is_core, int32_t device) {
  PQ_API_RANGE("pyqsm_dbscan");
  if (n < 0) return fail(PYQSM_EINVAL, "negative size");
  if (n == 0) return 0;
  if (!xyz || !labels) return fail(PYQSM_EINVAL, "pyqsm_dbscan: NULL pointer");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double* d_xyz;
  int64_t* d_lab;
  uint8_t* d_core;
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_xyz));
  PQ_TRY(c->arena.get(size_t(n), &d_lab));
  PQ_TRY(c->arena.get(size_t(n), &d_core));
  PQ_TRY(copy_in(c, d_xyz, xyz, size_t(n) * 3));
  PQ_TRY(dbscan_device(c, d_xyz, n, eps, min_pts, radius_inclusive != 0, d_lab, d_core, nullptr));
  PQ_TRY(download(c, labels, d_lab, size_t(n)));
  if (is_core) PQ_TRY(download(c, is_core, d_core, size_t(n)));
  PQ_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int pyqsm_octant_directory(const double* xyz, int64_t n, double eps, int32_t* dims_out, int32_t* begin_out,
                           int64_t cap, int32_t device) {
  PQ_API_RANGE("pyqsm_octant_directory");
  if (n <= 0) return fail(PYQSM_EINVAL, "pyqsm_octant_directory: empty cloud");
  if (!xyz || !dims_out || !begin_out) return fail(PYQSM_EINVAL, "pyqsm_octant_directory: NULL pointer");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double* d_xyz;
  PQ_TRY(upload(c, xyz, size_t(n) * 3, &d_xyz));
  DirReadout ro{cap, begin_out, {0, 0, 0}};
  PQ_TRY(dbscan_device(c, d_xyz, n, eps, 1, true, nullptr, nullptr, nullptr, &ro));
  for (int a = 0; a < 3; ++a) dims_out[a] = ro.dims[a];
  return 0;
}

int pyqsm_core_ramp_constants(double eps, int32_t radius_inclusive, float* out) {
  if (!out) return fail(PYQSM_EINVAL, "pyqsm_core_ramp_constants: NULL pointer");
  const CoreRamp cr = core_ramp(dbscan_r2(eps, radius_inclusive != 0));
  out[0] = cr.lo, out[1] = cr.hi, out[2] = cr.K, out[3] = cr.A, out[4] = cr.B;
  out[5] = cr.usable() ? 1.0f : 0.0f;
  return 0;
}

int pyqsm_core_ramp_probe(const float* d, int64_t n, double eps, int32_t radius_inclusive, float* s_in_out,
                          float* s_hi_out, int32_t device) {
  PQ_API_RANGE("pyqsm_core_ramp_probe");
  if (n < 0) return fail(PYQSM_EINVAL, "negative size");
  const CoreRamp cr = core_ramp(dbscan_r2(eps, radius_inclusive != 0));
  if (!cr.usable()) return fail(PYQSM_EINVAL, "pyqsm_core_ramp_probe: no ramp form at this eps");
  if (n == 0) return 0;
  if (!d || !s_in_out || !s_hi_out) return fail(PYQSM_EINVAL, "pyqsm_core_ramp_probe: NULL pointer");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  float *d_d, *d_in, *d_hi;
  PQ_TRY(upload(c, d, size_t(n), &d_d));
  PQ_TRY(c->arena.get(size_t(n), &d_in));
  PQ_TRY(c->arena.get(size_t(n), &d_hi));
  hipLaunchKernelGGL(k_core_ramp_probe, dim3(ceil_div(ceil_div(n, 2), 256)), dim3(256), 0, c->stream, d_d, n, -cr.K,
                     cr.A, cr.B, d_in, d_hi);
  PQ_HIP(hipGetLastError());
  PQ_TRY(fetch(c, s_in_out, d_in, size_t(n)));
  PQ_TRY(fetch(c, s_hi_out, d_hi, size_t(n)));
  return 0;
}

}  // extern "C"
