/* meshdist_f64.c — INDEPENDENT double-precision references for point-to-mesh distance and for
 * inside/outside of a closed mesh (test infrastructure; the counterpart of ray_f64.c for
 * pyqsm_amd/csrc/meshdist.hip and RaycastingScene.compute_occupancy).
 *
 * Neither shares a formulation with the code under test:
 *  - distance: the fp32 inputs are taken as exact doubles. A triangle with a non-zero normal n is
 *    met by projecting the query onto its plane; if the query lies inside the three edge
 *    half-planes (((v - u) x (p - u)) . n >= 0 for the edges u -> v) the distance is the plane
 *    distance |(p - a) . n| / |n|, otherwise (and for a zero normal) it is the smallest of the
 *    three point-to-segment distances. No d1...d6 region walk, no barycentric weights.
 *  - inside/outside: the winding number, the sum over all triangles of the solid angle they
 *    subtend at the query (Van Oosterom & Strackee 1983: tan(W/2) = a.(b x c) /
 *    (|a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|)) divided by 4 pi. No ray is cast. */
#include <math.h>
#include <stdint.h>

static inline double dot3(const double* a, const double* b) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

static inline void sub3(const double* a, const double* b, double* o) {
  o[0] = a[0] - b[0]; o[1] = a[1] - b[1]; o[2] = a[2] - b[2];
}

static inline void cross3(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

static double seg_d2(const double* p, const double* u, const double* v) {
  double e[3], w[3];
  sub3(v, u, e);
  sub3(p, u, w);
  const double ee = dot3(e, e);
  double s = ee > 0.0 ? dot3(w, e) / ee : 0.0;
  s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
  const double r[3] = {w[0] - s * e[0], w[1] - s * e[1], w[2] - s * e[2]};
  return dot3(r, r);
}

static double tri_d2(const double* p, const double* a, const double* b, const double* c) {
  double ab[3], ac[3], n[3];
  sub3(b, a, ab);
  sub3(c, a, ac);
  cross3(ab, ac, n);
  const double nn = dot3(n, n);
  if (nn > 0.0) {
    const double* u[3] = {a, b, c};
    int inside = 1;
    for (int k = 0; k < 3 && inside; ++k) {
      double e[3], w[3], x[3];
      sub3(u[(k + 1) % 3], u[k], e);
      sub3(p, u[k], w);
      cross3(e, w, x);
      inside = dot3(x, n) >= 0.0;
    }
    if (inside) {
      double w[3];
      sub3(p, a, w);
      const double s = dot3(w, n);
      return s * s / nn;
    }
  }
  const double d0 = seg_d2(p, a, b), d1 = seg_d2(p, b, c), d2 = seg_d2(p, c, a);
  return fmin(d0, fmin(d1, d2));
}

static void load3(const float* v, int32_t i, double* o) {
  o[0] = v[3 * (int64_t)i]; o[1] = v[3 * (int64_t)i + 1]; o[2] = v[3 * (int64_t)i + 2];
}

/* dist [Q] and the closest triangle (lowest index on exact fp64 ties; -1 when T == 0). */
int orc_point_mesh_distance_f64(const float* verts, const int32_t* tris, int64_t T,
                                const float* qry, int64_t Q, double* dist, int64_t* prim) {
#pragma omp parallel for schedule(static)
  for (int64_t i = 0; i < Q; ++i) {
    const double p[3] = {qry[3 * i], qry[3 * i + 1], qry[3 * i + 2]};
    double best = INFINITY;
    int64_t bp = -1;
    for (int64_t j = 0; j < T; ++j) {
      double a[3], b[3], c[3];
      load3(verts, tris[3 * j], a);
      load3(verts, tris[3 * j + 1], b);
      load3(verts, tris[3 * j + 2], c);
      const double d = tri_d2(p, a, b, c);
      if (d < best) {
        best = d;
        bp = j;
      }
    }
    dist[i] = sqrt(best);
    prim[i] = bp;
  }
  return 0;
}

/* Distance of query i to the ONE triangle prim[i] (NaN where prim[i] is outside [0, T)). */
int orc_point_tri_pairs_f64(const float* verts, const int32_t* tris, int64_t T, const float* qry,
                            int64_t Q, const int64_t* prim, double* dist) {
#pragma omp parallel for schedule(static)
  for (int64_t i = 0; i < Q; ++i) {
    const int64_t j = prim[i];
    if (j < 0 || j >= T) {
      dist[i] = NAN;
      continue;
    }
    const double p[3] = {qry[3 * i], qry[3 * i + 1], qry[3 * i + 2]};
    double a[3], b[3], c[3];
    load3(verts, tris[3 * j], a);
    load3(verts, tris[3 * j + 1], b);
    load3(verts, tris[3 * j + 2], c);
    dist[i] = sqrt(tri_d2(p, a, b, c));
  }
  return 0;
}

/* Winding number of the mesh about every query: +-1 inside a closed, consistently oriented
 * surface, 0 outside; undefined on the surface itself. */
int orc_winding_number_f64(const float* verts, const int32_t* tris, int64_t T, const float* qry,
                           int64_t Q, double* wn) {
#pragma omp parallel for schedule(static)
  for (int64_t i = 0; i < Q; ++i) {
    const double p[3] = {qry[3 * i], qry[3 * i + 1], qry[3 * i + 2]};
    double sum = 0.0;
    for (int64_t j = 0; j < T; ++j) {
      double a[3], b[3], c[3], bc[3];
      load3(verts, tris[3 * j], a);
      load3(verts, tris[3 * j + 1], b);
      load3(verts, tris[3 * j + 2], c);
      sub3(a, p, a);
      sub3(b, p, b);
      sub3(c, p, c);
      const double la = sqrt(dot3(a, a)), lb = sqrt(dot3(b, b)), lc = sqrt(dot3(c, c));
      cross3(b, c, bc);
      const double num = dot3(a, bc);
      const double den = la * lb * lc + dot3(a, b) * lc + dot3(b, c) * la + dot3(c, a) * lb;
      sum += 2.0 * atan2(num, den);
    }
    wn[i] = sum / (4.0 * M_PI);
  }
  return 0;
}
