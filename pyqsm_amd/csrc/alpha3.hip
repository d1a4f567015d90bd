// alpha3.hip — the 3-D alpha shape of lattice points on gfx950: exact boundary triangles and volume.
//
//   pyqsm_alpha_shape3   every triple of points of one segment with exactly one empty ball of radius rho
//                        through it (regular, oriented out of the solid), on request also the triples with
//                        two (singular), and six times the enclosed volume per segment as an exact integer:
//                        what Open3D's create_from_point_cloud_alpha_shape extracts from the Delaunay
//                        tetrahedra, by a contract of its own.
//
// The predicate is ball pivoting's (recon.hip, recon_exact.hpp): with n = (b - a) x (c - a), u = p - a,
// D = n.u and N = |u|^2 n2 - w.u a point is strictly inside the ball B+ on the +n side iff N < sqrt(H) D and
// strictly inside B- iff N < -sqrt(H) D (alpha3_exact.hpp: one evaluation, both answers, the fp64 filter in
// front for +D and -D). The bounds on every quantity are §19's; -D is no larger than D.
//
// Kinds. A ball is empty when no point of the segment is strictly inside. Exactly one empty ball and H > 0:
// regular, the row oriented so that its normal points to the empty ball. Both empty and H > 0: singular,
// written with b < c. Ties as in §19: a point on a ball does not block; a tie in the plane (on both balls)
// drops the triple when its index is below a's or it lies strictly beyond the edge opposite a, unless a
// point off the plane lies exactly on an empty ball, in which case the triple is kept and counted.
//
// Shape. a is the smallest index of its triple. A block serves kAlpha3Slice points of one cell, one after
// the other. For the point a it compacts the 27-cell stencil ONCE to the points of a's segment within
// 2 rho of a: their positions go to a block-private list in global memory (L2), the first kAlpha3Chunk of
// them, as u = p - a in fp64, straight into LDS; the higher-indexed among them go to a second list. Pairs
// (b, c) are formed from the second list only, a candidate is a pair with |b - c| <= 2 rho, n != 0 and H >= 0,
// and one lane owns one candidate and sweeps the first list, read from LDS as broadcasts, deciding both balls
// from one N and D; it stops when both are blocked, and a wave skips a chunk when all its lanes are done.
// Lists longer than one chunk are staged chunk by chunk from the global list. Blocks are resident and
// stride over the work items, so the private lists are (blocks in flight) x (largest stencil), not
// (work items) x (largest stencil).
//
// Rows are appended through one 64-bit integer atomicAdd and sorted by their unique (a, b, c) with the
// atomic-free radix sort. The volume is the sum of det(a - o, b - o, c - o) over the regular rows, o the
// segment's first point, each determinant a 128-bit integer cut into four 32-bit limbs that are added into
// four 64-bit integer accumulators per segment: integer sums, the same bytes whatever the arrival order.
#include "alpha3_exact.hpp"
#include "grid.hpp"
#include "recon_grid.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace pyqsm {

static constexpr int kAlpha3Chunk = PYQSM_ALPHA3_CHUNK;  // neighbours staged in LDS at a time (24 KiB)
static constexpr int kAlpha3Slice = PYQSM_ALPHA3_SLICE;  // points of a cell one work item serves
static constexpr uint64_t kAlpha3MaxRho2 = PYQSM_RECON_MAX_RHO2;
// ten seconds of the triangle pass at the 4.1e11 estimated pair tests per second measured on one MI355X
// (profiles/alpha3_perf.jsonl)
static constexpr int64_t kAlpha3DefaultMaxTests = PYQSM_ALPHA3_DEFAULT_MAX_TESTS;
static constexpr int kAlpha3MaxBlocks = 2048;                    // resident blocks of the triangle pass
static constexpr int64_t kAlpha3ScratchInts = int64_t(1) << 27;  // 512 MiB of neighbour lists at the most

// the points in the grid's order: coordinates relative to the cloud's corner and the segment of each
__global__ __launch_bounds__(256) void k_alpha3_gather(int n, const int32_t* __restrict__ order,
                                                       const int32_t* __restrict__ ijk,
                                                       const int32_t* __restrict__ seg, int x0, int y0, int z0,
                                                       int32_t* __restrict__ lx, int32_t* __restrict__ ly,
                                                       int32_t* __restrict__ lz, int32_t* __restrict__ lseg) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const size_t i = size_t(order[p]);
  lx[p] = int32_t(int64_t(ijk[3 * i]) - x0);
  ly[p] = int32_t(int64_t(ijk[3 * i + 1]) - y0);
  lz[p] = int32_t(int64_t(ijk[3 * i + 2]) - z0);
  lseg[p] = seg[i];
}

// is (pa, pb, pc), pb and pc within 2 rho of pa, a candidate: third edge, n != 0, circumradius <= rho
__device__ __forceinline__ bool alpha3_pair(const int32_t* __restrict__ lx, const int32_t* __restrict__ ly,
                                            const int32_t* __restrict__ lz, int pa, int pb, int pc,
                                            uint64_t four_r2) {
  const int64_t a[3] = {lx[pa], ly[pa], lz[pa]}, b[3] = {lx[pb], ly[pb], lz[pb]}, c[3] = {lx[pc], ly[pc], lz[pc]};
  ReconTri t;
  return recon_setup(a, b, c, four_r2, &t);
}

// The rare path, out of line so that its wide integers do not cost the sweep its registers. Bits: 1 = p is
// strictly inside B+, 2 = on B+ and off the plane, 8 / 16 the same for B-, 4 = on both in the plane and
// either of a lower index than a or strictly beyond the edge opposite a.
__device__ __noinline__ int alpha3_exact_test(const int32_t* __restrict__ lx, const int32_t* __restrict__ ly,
                                              const int32_t* __restrict__ lz, const int32_t* __restrict__ lorig,
                                              int pa, int pb, int pc, int p, uint64_t four_r2) {
  const int64_t a[3] = {lx[pa], ly[pa], lz[pa]}, b[3] = {lx[pb], ly[pb], lz[pb]}, c[3] = {lx[pc], ly[pc], lz[pc]};
  ReconTri tri;
  recon_setup(a, b, c, four_r2, &tri);  // a candidate: alpha3_pair said so
  const int64_t u[3] = {lx[p] - a[0], ly[p] - a[1], lz[p] - a[2]};
  const Alpha3Sides s = alpha3_classify(tri, u);
  int bits = 0;
  if (s.plus == kReconInside) bits |= 1;
  if (s.plus == kReconTieOffPlane) bits |= 2;
  if (s.minus == kReconInside) bits |= 8;
  if (s.minus == kReconTieOffPlane) bits |= 16;
  if (s.plus == kReconTieCoplanar && (lorig[p] < lorig[pa] || recon_beyond_bc(tri, u))) bits |= 4;
  return bits;
}

// stats: [0] ball tests, [1] tests classified by the integers, [2] candidates, [3] rows kept with a tie point
// off their plane on an empty ball. lists: 2 * list_stride ints per block. rows: (a, b, c, kind) appended at
// *cursor while below row_cap.
__global__ __launch_bounds__(256) void k_alpha3_tris(
    int n_work, int ncell, const int32_t* __restrict__ blk_start, int nx, int ny, const int32_t* __restrict__ start,
    const int32_t* __restrict__ lx, const int32_t* __restrict__ ly, const int32_t* __restrict__ lz,
    const int32_t* __restrict__ lorig, const int32_t* __restrict__ lseg, unsigned long long four_r2, int faces_all,
    int32_t* lists, long long list_stride, long long row_cap, int4* __restrict__ rows,
    unsigned long long* __restrict__ cursor, unsigned long long* __restrict__ stats) {
  __shared__ double sx[kAlpha3Chunk], sy[kAlpha3Chunk], sz[kAlpha3Chunk];
  __shared__ int qb[512], qc[512];
  __shared__ int qn, s_cell, s_k, s_kh;
  __shared__ unsigned long long s_tests, s_exact, s_cand, s_unres;
  const int t = threadIdx.x;
  int32_t* const gl = lists + size_t(blockIdx.x) * 2 * size_t(list_stride);  // a's neighbours
  int32_t* const gh = gl + list_stride;                                      // the higher-indexed among them
  if (t == 0) s_tests = s_exact = s_cand = s_unres = 0;
  unsigned my_exact = 0, my_cand = 0, my_unres = 0;
  unsigned long long my_tests = 0;
  for (int work = blockIdx.x; work < n_work; work += gridDim.x) {
    __syncthreads();
    if (t == 0) {
      int lo = 0, hi = ncell;  // the cell c with blk_start[c] <= work < blk_start[c + 1]
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (blk_start[mid + 1] <= work) lo = mid + 1;
        else hi = mid;
      }
      s_cell = lo;
    }
    __syncthreads();
    const int c = s_cell;
    if (c >= ncell) continue;  // block-uniform; cannot happen for a work item inside the scanned total
    const int a0 = start[c] + (work - blk_start[c]) * kAlpha3Slice;  // this item's points of the cell
    const int m = min(kAlpha3Slice, start[c + 1] - a0);
    const ReconStencil st = recon_stencil(nx, ny, c, start);
    const int S = st.total;
    for (int ia = 0; ia < m; ++ia) {
      const int pa = a0 + ia, oa = lorig[pa], sa = lseg[pa];
      const int ax = lx[pa], ay = ly[pa], az = lz[pa];
      __syncthreads();  // the point before is done with the lists, the queue and the staged chunk
      if (t == 0) s_k = s_kh = qn = 0;
      __syncthreads();
      // the stencil, once: a's neighbours within 2 rho in its segment, and the higher-indexed among them
      for (int j0 = 0; j0 < S; j0 += 256) {
        const int j = j0 + t;
        bool near = false, high = false;
        int p = 0, ux = 0, uy = 0, uz = 0;
        if (j < S) {
          p = st.at(j);
          if (p != pa && lseg[p] == sa) {
            ux = lx[p] - ax;  // below 2^27 inside a stencil
            uy = ly[p] - ay;
            uz = lz[p] - az;
            near = uint64_t(int64_t(ux) * ux + int64_t(uy) * uy + int64_t(uz) * uz) <= four_r2;
            high = near && lorig[p] > oa;
          }
        }
        const unsigned long long mask = __ballot(near), mask_h = __ballot(high);
        const unsigned long long below = (1ull << (t & 63)) - 1ull;
        int base = 0, base_h = 0;
        if ((t & 63) == 0) {
          if (mask) base = atomicAdd(&s_k, __popcll(mask));
          if (mask_h) base_h = atomicAdd(&s_kh, __popcll(mask_h));
        }
        base = __shfl(base, 0);
        base_h = __shfl(base_h, 0);
        if (near) {
          const int at = base + __popcll(mask & below);  // below S <= list_stride
          gl[at] = p;
          if (at < kAlpha3Chunk) {
            sx[at] = double(ux);
            sy[at] = double(uy);
            sz[at] = double(uz);
          }
        }
        if (high) gh[base_h + __popcll(mask_h & below)] = p;
      }
      __syncthreads();
      const int K = s_k, KH = s_kh;
      if (KH < 2) continue;  // block-uniform
      const bool one_chunk = K <= kAlpha3Chunk;
      const unsigned long long KK = (unsigned long long)KH * (unsigned long long)KH;
      unsigned long long cand = 0;  // block-uniform: how far the index pairs of gh are listed
      for (;;) {
        // fill the queue with candidate pairs, 256 index pairs (bj, cj) at a time
        int have = qn;
        __syncthreads();  // every wave has read qn before the first of them adds to it
        while (have < 256 && cand < KK) {
          const unsigned long long idx = cand + (unsigned)t;
          int pb = 0, pc = 0;
          bool active = false;
          if (idx < KK) {
            int bj, cj;
            if (KK < (1ull << 32)) {
              bj = int(unsigned(idx) / unsigned(KH));
              cj = int(unsigned(idx) - unsigned(bj) * unsigned(KH));
            } else {
              bj = int(idx / (unsigned long long)KH);
              cj = int(idx - (unsigned long long)bj * (unsigned long long)KH);
            }
            if (bj < cj) {
              pb = gh[bj];
              pc = gh[cj];
              active = alpha3_pair(lx, ly, lz, pa, pb, pc, four_r2);
            }
          }
          const unsigned long long mask = __ballot(active);
          int base = 0;
          if ((t & 63) == 0 && mask) base = atomicAdd(&qn, __popcll(mask));
          base = __shfl(base, 0);
          if (active) {
            const int at = base + __popcll(mask & ((1ull << (t & 63)) - 1ull));  // below 256 + 256
            qb[at] = pb;
            qc[at] = pc;
          }
          cand += 256;
          __syncthreads();
          have = qn;
          __syncthreads();
        }
        if (have == 0) break;
        const int take = have < 256 ? have : 256;
        const bool mine = t < take;
        int pb = 0, pc = 0;
        bool h_zero = false;
        ReconFilterTri ft = {{0, 0, 0}, {0, 0, 0}, 0, 0};
        if (mine) {
          pb = qb[t];
          pc = qc[t];
          const int64_t a[3] = {ax, ay, az}, b[3] = {lx[pb], ly[pb], lz[pb]}, cc[3] = {lx[pc], ly[pc], lz[pc]};
          ReconTri tri;
          recon_setup(a, b, cc, four_r2, &tri);  // a candidate: alpha3_pair said so
          h_zero = tri.H == 0;
          ft = recon_filter_setup(tri);
        }
        bool blocked_p = !mine, blocked_m = !mine, off_p = false, off_m = false, tie_drop = false;
        for (int k0 = 0; k0 < K; k0 += kAlpha3Chunk) {
          const int cn = K - k0 < kAlpha3Chunk ? K - k0 : kAlpha3Chunk;
          if (!one_chunk) {
            __syncthreads();
            for (int j = t; j < cn; j += 256) {
              const int p = gl[k0 + j];
              sx[j] = double(lx[p] - ax);
              sy[j] = double(ly[p] - ay);
              sz[j] = double(lz[p] - az);
            }
            __syncthreads();
          }
          if (__ballot(!(blocked_p && blocked_m)) == 0) continue;  // the whole wave is done with this tile
          for (int j = 0; j < cn && !(blocked_p && blocked_m); ++j) {
            const Alpha3Sides side = alpha3_filter(ft, sx[j], sy[j], sz[j]);  // the host checks the same function
            bool ask_p = !blocked_p && side.plus != kReconFilterOutside;
            bool ask_m = !blocked_m && side.minus != kReconFilterOutside;
            if (!ask_p && !ask_m) continue;
            if (ask_p && side.plus == kReconFilterInside) {
              blocked_p = true;
              ask_p = false;
            }
            if (ask_m && side.minus == kReconFilterInside) {
              blocked_m = true;
              ask_m = false;
            }
            if (!ask_p && !ask_m) continue;
            const int p = gl[k0 + j];
            if (p == pb || p == pc) continue;
            ++my_exact;
            const int where = alpha3_exact_test(lx, ly, lz, lorig, pa, pb, pc, p, four_r2);
            if (ask_p) {
              blocked_p = (where & 1) != 0;
              off_p = off_p || (where & 2) != 0;
            }
            if (ask_m) {
              blocked_m = (where & 8) != 0;
              off_m = off_m || (where & 16) != 0;
            }
            tie_drop = tie_drop || (where & 4) != 0;
          }
        }
        if (mine) {
          my_tests += (unsigned long long)K;
          ++my_cand;
          const bool unresolved = (!blocked_p && off_p) || (!blocked_m && off_m);
          bool flip;
          const int kind = alpha3_kind(!blocked_p, !blocked_m, unresolved, tie_drop, h_zero, &flip);
          if (kind == kAlpha3Regular || (kind == kAlpha3Singular && faces_all)) {
            int ob = lorig[pb], oc = lorig[pc];
            if (kind == kAlpha3Singular) flip = ob > oc;
            if (flip) {
              const int tmp = ob;
              ob = oc;
              oc = tmp;
            }
            if (unresolved) ++my_unres;
            const unsigned long long at = atomicAdd(cursor, 1ull);
            if ((long long)at < row_cap) rows[at] = make_int4(oa, ob, oc, kind);
          }
        }
        // drop the served entries
        __syncthreads();
        const int rest = have - take;
        int rb = 0, rc = 0;
        if (t < rest) {
          rb = qb[take + t];
          rc = qc[take + t];
        }
        __syncthreads();
        if (t < rest) {
          qb[t] = rb;
          qc[t] = rc;
        }
        if (t == 0) qn = rest;
        __syncthreads();
      }
    }
  }
  __syncthreads();
  if (my_tests) atomicAdd(&s_tests, my_tests);
  if (my_exact) atomicAdd(&s_exact, (unsigned long long)my_exact);
  if (my_cand) atomicAdd(&s_cand, (unsigned long long)my_cand);
  if (my_unres) atomicAdd(&s_unres, (unsigned long long)my_unres);
  __syncthreads();
  if (t == 0) {
    if (s_tests) atomicAdd(&stats[0], s_tests);
    if (s_exact) atomicAdd(&stats[1], s_exact);
    if (s_cand) atomicAdd(&stats[2], s_cand);
    if (s_unres) atomicAdd(&stats[3], s_unres);
  }
}

// acc[4 s + k] += limb k (32 bits) of det(a - o, b - o, c - o) as a 128-bit two's complement, for every
// regular row of segment s, o the segment's first point: the sum of the four accumulators, shifted, is
// six times the volume modulo 2^128. Differences are below 2^32, a determinant below 6 * 2^96.
__global__ __launch_bounds__(256) void k_alpha3_volume(long long n_rows, const int4* __restrict__ rows,
                                                       const int32_t* __restrict__ ijk,
                                                       const int32_t* __restrict__ seg,
                                                       const long long* __restrict__ seg_start,
                                                       unsigned long long* __restrict__ acc) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  int s = -1;
  unsigned long long limb[4] = {0, 0, 0, 0};
  if (i < n_rows) {
    const int4 r = rows[i];
    if (r.w == kAlpha3Regular) {
      s = seg[r.x];
      const size_t o = size_t(seg_start[s]);
      int64_t v[3][3];
      const int idx[3] = {r.x, r.y, r.z};
      for (int k = 0; k < 3; ++k)
        for (int d = 0; d < 3; ++d) v[k][d] = int64_t(ijk[3 * size_t(idx[k]) + d]) - int64_t(ijk[3 * o + d]);
      const i128 cx = i128(v[1][1]) * v[2][2] - i128(v[1][2]) * v[2][1];
      const i128 cy = i128(v[1][2]) * v[2][0] - i128(v[1][0]) * v[2][2];
      const i128 cz = i128(v[1][0]) * v[2][1] - i128(v[1][1]) * v[2][0];
      const u128 det = u128(cx * v[0][0] + cy * v[0][1] + cz * v[0][2]);
      for (int k = 0; k < 4; ++k) limb[k] = (unsigned long long)(uint32_t(det >> (32 * k)));
    }
  }
  const int s0 = __shfl(s, 0);
  if (__ballot(s != s0) == 0) {  // one segment in the whole wave (or no row at all): one lane adds
    if (s0 < 0) return;
    for (int k = 0; k < 4; ++k) {
      unsigned long long v = limb[k];
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
      if ((threadIdx.x & 63) == 0) atomicAdd(&acc[4 * size_t(s0) + k], v);
    }
  } else if (s >= 0) {
    for (int k = 0; k < 4; ++k) atomicAdd(&acc[4 * size_t(s) + k], limb[k]);
  }
}

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_alpha_shape3(const int32_t* ijk, int64_t n, const int64_t* seg_start, int64_t n_seg, uint64_t rho2,
                       int32_t faces, int64_t max_tests, int64_t* n_rows, int32_t** rows, uint64_t* vol6,
                       int64_t* stats, int32_t device) {
  PQ_API_RANGE("pyqsm_alpha_shape3");
  if (rows) *rows = nullptr;
  if (n_rows) *n_rows = 0;
  if (stats) std::fill(stats, stats + 8, int64_t(0));
  if (!seg_start) n_seg = 1;
  if (vol6 && n_seg > 0) std::fill(vol6, vol6 + 2 * n_seg, uint64_t(0));
  if (n < 0 || n_seg < 0) return fail(PYQSM_EINVAL, "pyqsm_alpha_shape3: negative size");
  if (!n_rows || !rows || (n_seg > 0 && !vol6) || (n > 0 && !ijk))
    return fail(PYQSM_EINVAL, "pyqsm_alpha_shape3: NULL pointer");
  if (faces != PYQSM_ALPHA3_REGULAR && faces != PYQSM_ALPHA3_ALL)
    return fail(PYQSM_EINVAL, "pyqsm_alpha_shape3: faces must be PYQSM_ALPHA3_REGULAR or PYQSM_ALPHA3_ALL");
  if (rho2 == 0) return fail(PYQSM_EINVAL, "pyqsm_alpha_shape3: rho^2 must be positive");
  if (rho2 > kAlpha3MaxRho2) {
    int shift = 1;
    while ((rho2 >> (2 * shift)) > kAlpha3MaxRho2) ++shift;
    return fail(PYQSM_EINVAL,
                "pyqsm_alpha_shape3: rho^2 = %llu exceeds 2^22 lattice units^2 (rho <= 2048): a quantum 2^%d times "
                "as large would fit",
                (unsigned long long)rho2, shift);
  }
  if (seg_start) {
    if (seg_start[0] != 0 || seg_start[n_seg] != n)
      return fail(PYQSM_EINVAL, "pyqsm_alpha_shape3: seg_start must run from 0 to n");
    for (int64_t s = 0; s < n_seg; ++s)
      if (seg_start[s + 1] < seg_start[s]) return fail(PYQSM_EINVAL, "pyqsm_alpha_shape3: seg_start must ascend");
  }
  if (n > (int64_t(1) << 26))  // 16 n + 1024 rows are counted in 32 bits
    return fail(PYQSM_ERANGE, "pyqsm_alpha_shape3: more than 2^26 points per call");
  if (max_tests <= 0) max_tests = kAlpha3DefaultMaxTests;
  int64_t largest = seg_start ? 0 : n;
  for (int64_t s = 0; seg_start && s < n_seg; ++s) largest = std::max(largest, seg_start[s + 1] - seg_start[s]);
  if (largest < 3) return 0;  // no triple inside a segment: no device work

  int32_t mn[3], mx[3];
  for (int a = 0; a < 3; ++a) mn[a] = mx[a] = ijk[a];
  for (int64_t i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) {
      mn[a] = std::min(mn[a], ijk[3 * i + a]);
      mx[a] = std::max(mx[a], ijk[3 * i + a]);
    }
  for (int a = 0; a < 3; ++a)
    if (int64_t(mx[a]) - mn[a] > 0x7FFFFFFFLL)
      return fail(PYQSM_EINVAL, "pyqsm_alpha_shape3: the cloud spans more than 2^31 lattice units");
  const double bbox[6] = {double(mn[0]), double(mn[1]), double(mn[2]), double(mx[0]), double(mx[1]), double(mx[2])};
  std::vector<int32_t> seg(size_t(n), 0);
  std::vector<long long> first(size_t(n_seg) + 1, 0);
  first[size_t(n_seg)] = n;
  if (seg_start)
    for (int64_t s = 0; s < n_seg; ++s) {
      first[size_t(s)] = seg_start[s];
      std::fill(seg.begin() + seg_start[s], seg.begin() + seg_start[s + 1], int32_t(s));
    }

  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  const int N = int(n);
  const int64_t row_cap = 16 * n + 1024;
  int32_t *d_ijk, *d_seg, *d_lx, *d_ly, *d_lz, *d_lseg, *d_blk;
  long long* d_first;
  double* d_xyz;
  unsigned long long *d_counters, *d_acc;  // cursor, stats[4], est[4]
  const size_t n_counters = 9;
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_ijk));
  PQ_TRY(c->arena.get(size_t(n), &d_seg));
  PQ_TRY(c->arena.get(size_t(n_seg) + 1, &d_first));
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_xyz));
  PQ_TRY(c->arena.get(size_t(n), &d_lx));
  PQ_TRY(c->arena.get(size_t(n), &d_ly));
  PQ_TRY(c->arena.get(size_t(n), &d_lz));
  PQ_TRY(c->arena.get(size_t(n), &d_lseg));
  PQ_TRY(c->arena.get(n_counters, &d_counters));
  PQ_TRY(c->arena.get(size_t(n_seg) * 4, &d_acc));
  PQ_TRY(copy_in(c, d_ijk, ijk, size_t(n) * 3));
  PQ_TRY(copy_in(c, d_seg, seg.data(), size_t(n)));
  PQ_TRY(copy_in(c, d_first, first.data(), size_t(n_seg) + 1));
  PQ_HIP(hipMemsetAsync(d_counters, 0, n_counters * 8, c->stream));
  PQ_HIP(hipMemsetAsync(d_acc, 0, size_t(n_seg) * 32, c->stream));
  hipLaunchKernelGGL(k_recon_to_f64, dim3(ceil_div(3 * n, 256)), dim3(256), 0, c->stream, 3 * n,
                     static_cast<const int32_t*>(d_ijk), d_xyz);
  PQ_HIP(hipGetLastError());

  // the grid (cells of the smallest integer edge >= 2 rho, and one more: recon.hip, "Locality"), the work
  // items of the triangle pass and the estimate of its pair tests
  const uint64_t four_r2 = 4 * rho2;
  DevGrid g;
  int32_t n_work = 0;
  unsigned long long est[4] = {0, 0, 0, 0};
  {
    ProfScope ps(c, "alpha3_bin");
    int64_t edge = int64_t(std::sqrt(double(four_r2)));
    while (uint64_t(edge) * uint64_t(edge) < four_r2) ++edge;
    while (edge > 1 && uint64_t(edge - 1) * uint64_t(edge - 1) >= four_r2) --edge;
    edge += 1;
    unsigned long long* d_est = d_counters + 5;
    const int64_t max_cells = std::min<int64_t>(int64_t(1) << 28, std::max<int64_t>(int64_t(1) << 22, 64 * n));
    PQ_TRY(build_grid(c, d_xyz, n, double(edge), max_cells, &g, bbox, false));
    const int nc = int(g.ncell);
    PQ_TRY(c->arena.get(size_t(nc) + 1, &d_blk));
    hipLaunchKernelGGL(k_alpha3_gather, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, N,
                       static_cast<const int32_t*>(g.order), static_cast<const int32_t*>(d_ijk),
                       static_cast<const int32_t*>(d_seg), mn[0], mn[1], mn[2], d_lx, d_ly, d_lz, d_lseg);
    PQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_recon_plan<kAlpha3Slice>, dim3(ceil_div(nc + 1, 256)), dim3(256), 0, c->stream, nc, g.nx,
                       g.ny, g.nz, static_cast<const int32_t*>(g.start), d_blk, d_est);
    PQ_HIP(hipGetLastError());
    PQ_TRY(exclusive_scan_i32(c, d_blk, int64_t(nc) + 1));
    PQ_TRY(download(c, &n_work, d_blk + nc, 1));
    PQ_TRY(download(c, est, d_est, 4));
    PQ_HIP(hipStreamSynchronize(c->stream));
  }
  const unsigned __int128 est_all = ((unsigned __int128)est[1] << 32) + est[0];
  const int64_t est_tests = est_all > (unsigned __int128)INT64_MAX ? INT64_MAX : int64_t(est_all);
  if (stats) {
    stats[0] = est_tests;
    stats[5] = int64_t(est[2]);
    stats[6] = int64_t(est[3]);
    stats[7] = n_work;
  }
  if (est_tests > max_tests)
    return fail(PYQSM_ERANGE,
                "pyqsm_alpha_shape3: an estimated %lld pair tests at rho^2 = %llu exceed max_tests = %lld (rho spans "
                "many point spacings: down-sample the cloud, lower the radius or raise max_tests)",
                (long long)est_tests, (unsigned long long)rho2, (long long)max_tests);

  // resident blocks, each with two private lists of one stencil's length
  const int64_t list_stride = std::max<int64_t>(int64_t(est[2]), 1);
  const int64_t fit = std::max<int64_t>(1, kAlpha3ScratchInts / (2 * list_stride));
  const int n_blocks = int(std::min<int64_t>(std::min<int64_t>(n_work, kAlpha3MaxBlocks), fit));
  int32_t* d_lists;
  int4* d_rows;
  PQ_TRY(c->arena.get(size_t(row_cap), &d_rows));
  PQ_TRY(c->arena.get(size_t(std::max(n_blocks, 1)) * 2 * size_t(list_stride), &d_lists));
  {
    ProfScope ps(c, "alpha3_tris");
    if (n_blocks > 0)
      hipLaunchKernelGGL(k_alpha3_tris, dim3(unsigned(n_blocks)), dim3(256), 0, c->stream, int(n_work),
                         int(g.ncell), static_cast<const int32_t*>(d_blk), g.nx, g.ny,
                         static_cast<const int32_t*>(g.start), static_cast<const int32_t*>(d_lx),
                         static_cast<const int32_t*>(d_ly), static_cast<const int32_t*>(d_lz),
                         static_cast<const int32_t*>(g.order), static_cast<const int32_t*>(d_lseg),
                         (unsigned long long)four_r2, int(faces == PYQSM_ALPHA3_ALL), d_lists, (long long)list_stride,
                         (long long)row_cap, d_rows, d_counters, d_counters + 1);
    PQ_HIP(hipGetLastError());
  }
  unsigned long long host[5];
  PQ_TRY(fetch(c, host, d_counters, 5));
  if (stats) {
    stats[1] = int64_t(host[1]);
    stats[2] = int64_t(host[2]);
    stats[3] = int64_t(host[3]);
    stats[4] = int64_t(host[4]);
  }
  const int64_t total = int64_t(host[0]);
  if (total > row_cap)
    return fail(PYQSM_ERANGE, "pyqsm_alpha_shape3: %lld rows, more than 16 n + 1024 = %lld (a cospherical set?)",
                (long long)total, (long long)row_cap);
  if (total == 0) return 0;
  const int e = int(total);
  {
    ProfScope ps(c, "alpha3_volume");
    hipLaunchKernelGGL(k_alpha3_volume, dim3(ceil_div(e, 256)), dim3(256), 0, c->stream, (long long)total,
                       static_cast<const int4*>(d_rows), static_cast<const int32_t*>(d_ijk),
                       static_cast<const int32_t*>(d_seg), static_cast<const long long*>(d_first), d_acc);
    PQ_HIP(hipGetLastError());
  }
  // ascending (a, b, c), a unique key: stable sorts by c, then b, then a
  const int id_bits = bit_length(uint64_t(n));
  int32_t *d_ka, *d_kb, *d_kc, *perm = nullptr;
  int4* d_sorted;
  PQ_TRY(c->arena.get(size_t(e), &d_ka));
  PQ_TRY(c->arena.get(size_t(e), &d_kb));
  PQ_TRY(c->arena.get(size_t(e), &d_kc));
  PQ_TRY(c->arena.get(size_t(e), &d_sorted));
  {
    ProfScope ps(c, "alpha3_sort");
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
  std::vector<unsigned long long> acc(size_t(n_seg) * 4);
  PQ_TRY(fetch(c, acc.data(), d_acc, acc.size()));
  OutBufs out;
  int32_t* host_rows = out.get<int32_t>(size_t(e) * 4);
  if (!host_rows) return fail(PYQSM_ENOMEM, "pyqsm_alpha_shape3: no host memory for %d rows", e);
  PQ_TRY(fetch(c, reinterpret_cast<int4*>(host_rows), d_sorted, size_t(e)));  // (a, b, c, kind) per row
  for (int64_t s = 0; s < n_seg; ++s) {
    u128 v = 0;
    for (int k = 0; k < 4; ++k) v += u128(acc[size_t(4 * s + k)]) << (32 * k);
    vol6[2 * s] = uint64_t(v);
    vol6[2 * s + 1] = uint64_t(v >> 64);
  }
  out.kept = true;
  *rows = host_rows;
  *n_rows = total;
  return 0;
}

}  // extern "C"
