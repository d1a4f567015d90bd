// meshdist.hip — distance from query points to a triangle mesh on gfx950.
//
// Stands in for open3d RaycastingScene.compute_distance / compute_signed_distance as used
// by `mri` (pyQSM/viz/ray_casting.py:237-260): N random points and a 64^3 grid of query
// points against the scene's mesh. Brute force like the ray sweep: one lane per query, the
// expanded triangle records arrive by scalar loads (the triangle index is wave-uniform), the
// closest point on each triangle follows Ericson's region walk (Real-Time Collision
// Detection, 5.1.5) in fp32 with separately rounded products — the CPU oracle
// (orc_point_mesh_distance) repeats the same operation sequence, so distances and the
// index of the closest triangle (lowest index on ties) are bit-identical.
// FP32-VALU bound: ~60 flop per point-triangle pair.
//
// Thin triangles do not go through the walk. Its va, vb, vc and 1 / (va + vb + vc) are differences
// of fp32 products of size |ap|^2 |edge|^2 that have to resolve (height * base)^2: on a sliver they
// are rounding noise, the region comes out wrong and the interior formula lands far from the
// triangle (measured against an fp64 evaluation: distances off by up to 37 %, from
// height / longest edge = 3e-3 downwards). k_dist_tris classifies every triangle ONCE, in fp64
// from the fp32 edge vectors:
//   kind 0  |ab x ac|^2 >  THIN_REL2 * (longest edge^2)^2: the walk;
//   kind 1  thinner, but with a normal: unit normal and the three unit in-plane edge normals are
//           prepared per triangle; a query inside the three edge half-planes is at its
//           plane distance, any other at the nearest of the three segments;
//   kind 2  no normal at all (ab x ac == 0 exactly: collinear or repeated vertices): the nearest
//           of the three segments.
// The pair loop over all T records stays the walk alone, without a branch (a scalar branch on the
// kind inside it cost 2 %: the loop runs at less than one wave per SIMD and lives on the scalar
// loads of the next record overlapping the arithmetic of this one). Instead k_dist_tris MOVES a thin
// triangle out: its record goes to a compact list (DThin, appended by an integer atomic; the order
// does not matter, see below) and its slot in the T records is filled with NaN, which the walk
// turns into a NaN distance that `d < best` rejects. A second loop over the list evaluates the thin
// triangles and merges by (distance, index), so the result is the lowest index among the closest
// triangles whatever the order of the list — the same as the oracle's single loop. Neither thin
// path can produce a NaN from finite input (a zero-length segment is a point), so no triangle of
// the list drops out.
#include "common.hpp"

namespace pyqsm {

#define PYQSM_THIN_REL2 4e-4  // (height / longest edge)^2 ~ (2 %)^2; the walk is accurate to 2.5e-7 above it

struct alignas(16) DTri {  // 48 bytes: a, ab, ac (what raycast.hip calls TriRec)
  float ax, ay, az, abx, aby, abz, acx, acy, acz, pad0, pad1, pad2;
};

struct alignas(16) DThin {  // 96 bytes: a thin triangle, its index and kind; for kind 1 the unit normal
                            // n and the inward unit edge normals of ab, bc, ca
  float ax, ay, az, abx, aby, abz, acx, acy, acz;
  uint32_t idx, kind, pad;
  float nx, ny, nz, mabx, maby, mabz, mbcx, mbcy, mbcz, mcax, mcay, mcaz;
};

__device__ __forceinline__ float dot3f(float ax, float ay, float az, float bx, float by, float bz) {
  float d = ax * bx;
  d = d + ay * by;
  d = d + az * bz;
  return d;
}

// m = unit(n x e); false if e has no length in fp32
__device__ __forceinline__ bool edge_normal(float nx, float ny, float nz, float ex, float ey, float ez,
                                            float* mx, float* my, float* mz) {
  const float cx = ny * ez - nz * ey, cy = nz * ex - nx * ez, cz = nx * ey - ny * ex;
  const float l2 = dot3f(cx, cy, cz, cx, cy, cz);
  if (!(l2 > 0.f) || l2 == __builtin_inff()) return false;
  const float inv = 1.f / sqrtf(l2);
  *mx = cx * inv; *my = cy * inv; *mz = cz * inv;
  return true;
}

__global__ void k_dist_tris(const float* __restrict__ verts, int64_t V,
                            const int32_t* __restrict__ tris, int64_t T, DTri* __restrict__ out,
                            DThin* __restrict__ thin, int* __restrict__ flags) {  // flags: bad, n_thin
  int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (i >= T) return;
  const int a = tris[3 * i], b = tris[3 * i + 1], c = tris[3 * i + 2];
  if (a < 0 || b < 0 || c < 0 || a >= V || b >= V || c >= V) {
    flags[0] = 1;
    return;
  }
  const float ax = verts[3 * a], ay = verts[3 * a + 1], az = verts[3 * a + 2];
  const float abx = verts[3 * b] - ax, aby = verts[3 * b + 1] - ay, abz = verts[3 * b + 2] - az;
  const float acx = verts[3 * c] - ax, acy = verts[3 * c + 1] - ay, acz = verts[3 * c + 2] - az;
  const float bcx = acx - abx, bcy = acy - aby, bcz = acz - abz;
  // the normal and the thinness in fp64 (add, multiply, divide, compare: the oracle's bits)
  const double nx = double(aby) * double(acz) - double(abz) * double(acy);
  const double ny = double(abz) * double(acx) - double(abx) * double(acz);
  const double nz = double(abx) * double(acy) - double(aby) * double(acx);
  const double nn = (nx * nx + ny * ny) + nz * nz;
  const double lab = (double(abx) * double(abx) + double(aby) * double(aby)) + double(abz) * double(abz);
  const double lac = (double(acx) * double(acx) + double(acy) * double(acy)) + double(acz) * double(acz);
  const double lbc = (double(bcx) * double(bcx) + double(bcy) * double(bcy)) + double(bcz) * double(bcz);
  double l2 = lab > lac ? lab : lac;
  l2 = lbc > l2 ? lbc : l2;
  double nmax = fabs(nx) > fabs(ny) ? fabs(nx) : fabs(ny);
  nmax = fabs(nz) > nmax ? fabs(nz) : nmax;
  uint32_t kind = 0;
  DThin h = {};
  if (!(nmax > 0.0)) {
    kind = 2;
  } else if (!(nn > PYQSM_THIN_REL2 * (l2 * l2))) {
    kind = 2;  // unless every normal below has a length
    const float ux = float(nx / nmax), uy = float(ny / nmax), uz = float(nz / nmax);
    const float inv = 1.f / sqrtf(dot3f(ux, uy, uz, ux, uy, uz));
    h.nx = ux * inv; h.ny = uy * inv; h.nz = uz * inv;
    if (edge_normal(h.nx, h.ny, h.nz, abx, aby, abz, &h.mabx, &h.maby, &h.mabz) &&
        edge_normal(h.nx, h.ny, h.nz, bcx, bcy, bcz, &h.mbcx, &h.mbcy, &h.mbcz) &&
        edge_normal(h.nx, h.ny, h.nz, -acx, -acy, -acz, &h.mcax, &h.mcay, &h.mcaz))
      kind = 1;
  }
  if (kind == 0) {
    out[i] = DTri{ax, ay, az, abx, aby, abz, acx, acy, acz, 0.f, 0.f, 0.f};
    return;
  }
  h.ax = ax; h.ay = ay; h.az = az; h.abx = abx; h.aby = aby; h.abz = abz;
  h.acx = acx; h.acy = acy; h.acz = acz;
  h.idx = uint32_t(i); h.kind = kind; h.pad = 0;
  thin[atomicAdd(&flags[1], 1)] = h;  // at most T appends into T slots
  const float nan = __builtin_nanf("");
  out[i] = DTri{nan, nan, nan, nan, nan, nan, nan, nan, nan, 0.f, 0.f, 0.f};  // the walk passes it over
}

// squared distance from w = p - u to the segment u .. u + e
__device__ __forceinline__ float seg_dist2(float ex, float ey, float ez, float wx, float wy, float wz) {
  const float ee = dot3f(ex, ey, ez, ex, ey, ez);
  float s = ee > 0.f ? dot3f(wx, wy, wz, ex, ey, ez) / ee : 0.f;
  s = s < 0.f ? 0.f : (s > 1.f ? 1.f : s);
  const float rx = wx - s * ex, ry = wy - s * ey, rz = wz - s * ez;
  return dot3f(rx, ry, rz, rx, ry, rz);
}

// squared distance from p to a thin triangle (kind 1: normals valid; kind 2: segments only)
__device__ __forceinline__ float thin_dist2(const DThin& t, float px, float py, float pz) {
  const float apx = px - t.ax, apy = py - t.ay, apz = pz - t.az;
  const float bpx = apx - t.abx, bpy = apy - t.aby, bpz = apz - t.abz;
  float d = seg_dist2(t.abx, t.aby, t.abz, apx, apy, apz);
  const float dac = seg_dist2(t.acx, t.acy, t.acz, apx, apy, apz);
  const float dbc = seg_dist2(t.acx - t.abx, t.acy - t.aby, t.acz - t.abz, bpx, bpy, bpz);
  d = dac < d ? dac : d;
  d = dbc < d ? dbc : d;
  if (t.kind == 1) {
    const DThin& m = t;
    const float sab = dot3f(m.mabx, m.maby, m.mabz, apx, apy, apz);
    const float sbc = dot3f(m.mbcx, m.mbcy, m.mbcz, bpx, bpy, bpz);
    const float sca = dot3f(m.mcax, m.mcay, m.mcaz, apx, apy, apz);
    if (sab >= 0.f && sbc >= 0.f && sca >= 0.f) {
      const float s = dot3f(m.nx, m.ny, m.nz, apx, apy, apz);
      d = s * s;
    }
  }
  return d;
}

// squared distance from p to the triangle (a, a + ab, a + ac)
__device__ __forceinline__ float tri_dist2(const DTri& t, float px, float py, float pz) {
  const float apx = px - t.ax, apy = py - t.ay, apz = pz - t.az;
  const float d1 = dot3f(t.abx, t.aby, t.abz, apx, apy, apz);
  const float d2 = dot3f(t.acx, t.acy, t.acz, apx, apy, apz);
  float cx, cy, cz;  // closest point minus a
  const float bpx = apx - t.abx, bpy = apy - t.aby, bpz = apz - t.abz;
  const float d3 = dot3f(t.abx, t.aby, t.abz, bpx, bpy, bpz);
  const float d4 = dot3f(t.acx, t.acy, t.acz, bpx, bpy, bpz);
  const float cpx = apx - t.acx, cpy = apy - t.acy, cpz = apz - t.acz;
  const float d5 = dot3f(t.abx, t.aby, t.abz, cpx, cpy, cpz);
  const float d6 = dot3f(t.acx, t.acy, t.acz, cpx, cpy, cpz);
  const float vc = d1 * d4 - d3 * d2;
  const float vb = d5 * d2 - d1 * d6;
  const float va = d3 * d6 - d5 * d4;
  if (d1 <= 0.f && d2 <= 0.f) {  // vertex a
    cx = cy = cz = 0.f;
  } else if (d3 >= 0.f && d4 <= d3) {  // vertex b
    cx = t.abx; cy = t.aby; cz = t.abz;
  } else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {  // edge ab
    const float v = d1 / (d1 - d3);
    cx = v * t.abx; cy = v * t.aby; cz = v * t.abz;
  } else if (d6 >= 0.f && d5 <= d6) {  // vertex c
    cx = t.acx; cy = t.acy; cz = t.acz;
  } else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {  // edge ac
    const float w = d2 / (d2 - d6);
    cx = w * t.acx; cy = w * t.acy; cz = w * t.acz;
  } else if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {  // edge bc
    const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    cx = t.abx + w * (t.acx - t.abx);
    cy = t.aby + w * (t.acy - t.aby);
    cz = t.abz + w * (t.acz - t.abz);
  } else {  // interior
    const float denom = 1.f / (va + vb + vc);
    const float v = vb * denom, w = vc * denom;
    cx = t.abx * v + t.acx * w;
    cy = t.aby * v + t.acy * w;
    cz = t.abz * v + t.acz * w;
  }
  const float ex = apx - cx, ey = apy - cy, ez = apz - cz;
  return dot3f(ex, ey, ez, ex, ey, ez);
}

__global__ __launch_bounds__(256) void k_point_mesh_dist(const DTri* __restrict__ tri,
                                                         const DThin* __restrict__ thin, int n_thin,
                                                         int T,
                                                         const float* __restrict__ qry, int64_t Q,
                                                         float* __restrict__ dist,
                                                         uint32_t* __restrict__ prim) {
  const int64_t i = blockIdx.x * int64_t(256) + threadIdx.x;
  const bool live = i < Q;
  const float px = live ? qry[3 * i] : 0.f, py = live ? qry[3 * i + 1] : 0.f,
              pz = live ? qry[3 * i + 2] : 0.f;
  float best = __builtin_inff();
  uint32_t bp = PYQSM_MISS_PRIM;
  for (int j = 0; j < T; ++j) {
    const DTri t = tri[j];  // wave-uniform address: scalar loads
    const float d = tri_dist2(t, px, py, pz);  // NaN for a slot whose triangle is in the thin list
    if (d < best) {
      best = d;
      bp = uint32_t(j);
    }
  }
  for (int k = 0; k < n_thin; ++k) {
    const DThin t = thin[k];  // wave-uniform address: scalar loads
    const float d = thin_dist2(t, px, py, pz);
    if (d < best || (d == best && t.idx < bp)) {
      best = d;
      bp = t.idx;
    }
  }
  if (live) {
    dist[i] = sqrtf(best);
    prim[i] = bp;
  }
}

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_point_mesh_distance(const float* verts, int64_t V, const int32_t* tris, int64_t T,
                              const float* qry, int64_t Q, float* dist, uint32_t* prim,
                              int32_t device) {
  PQ_API_RANGE("pyqsm_point_mesh_distance");
  if (V < 0 || T < 0 || Q < 0) return fail(PYQSM_EINVAL, "negative size");
  if (Q == 0) return 0;
  if (!qry || !dist || !prim) return fail(PYQSM_EINVAL, "pyqsm_point_mesh_distance: NULL pointer");
  if (T > 0 && (!verts || !tris)) return fail(PYQSM_EINVAL, "pyqsm_point_mesh_distance: NULL pointer");
  if (T > 0x7FFFFF00LL || V > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "mesh too large");
  if (T == 0) {  // no surface: infinitely far
    for (int64_t i = 0; i < Q; ++i) {
      dist[i] = HUGE_VALF;
      prim[i] = PYQSM_MISS_PRIM;
    }
    return 0;
  }
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  float *d_v, *d_q, *d_dist;
  int32_t* d_t;
  uint32_t* d_prim;
  DTri* d_rec;
  DThin* d_thin;
  int* d_flags;
  PQ_TRY(c->arena.get(size_t(V) * 3 + 1, &d_v));
  PQ_TRY(c->arena.get(size_t(T) * 3, &d_t));
  PQ_TRY(c->arena.get(size_t(Q) * 3, &d_q));
  PQ_TRY(c->arena.get(size_t(Q), &d_dist));
  PQ_TRY(c->arena.get(size_t(Q), &d_prim));
  PQ_TRY(c->arena.get(size_t(T), &d_rec));
  PQ_TRY(c->arena.get(size_t(T), &d_thin));
  PQ_TRY(c->arena.get(2, &d_flags));
  PQ_TRY(copy_in(c, d_v, verts, size_t(V) * 3));
  PQ_TRY(copy_in(c, d_t, tris, size_t(T) * 3));
  PQ_TRY(copy_in(c, d_q, qry, size_t(Q) * 3));
  PQ_HIP(hipMemsetAsync(d_flags, 0, 8, c->stream));
  hipLaunchKernelGGL(k_dist_tris, dim3(ceil_div(T, 256)), dim3(256), 0, c->stream, d_v, V, d_t, T, d_rec,
                     d_thin, d_flags);
  int flags[2] = {0, 0};  // a triangle index out of range; the length of the thin list
  PQ_TRY(fetch(c, flags, d_flags, 2));
  if (flags[0]) return fail(PYQSM_EINVAL, "triangle index outside the vertex array");
  {
    ProfScope ps(c, "point_mesh_distance");
    hipLaunchKernelGGL(k_point_mesh_dist, dim3(ceil_div(Q, 256)), dim3(256), 0, c->stream, d_rec, d_thin,
                       flags[1], int(T), d_q, Q, d_dist, d_prim);
    PQ_HIP(hipGetLastError());
  }
  PQ_TRY(download(c, dist, d_dist, size_t(Q)));
  PQ_TRY(download(c, prim, d_prim, size_t(Q)));
  PQ_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

}  // extern "C"
