// pca.hpp — the symmetric 3x3 eigen solve shared by the point-cloud Laplacian (laplacian.hip:
// k_tangent_planes) and normal estimation (normals.hip). Host and device: the restatements and the
// CPU oracle repeat the same operations in the same order.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace pyqsm {

// ---- symmetric 3x3 eigen decomposition (cyclic Jacobi, fixed sweep count) ------

struct Sym3 {
  double a00, a01, a02, a11, a12, a22;
};

// Returns the unit eigenvector of the smallest eigenvalue of A.
__host__ __device__ inline void smallest_eigvec(Sym3 A, double n[3]) {
  double a[3][3] = {{A.a00, A.a01, A.a02}, {A.a01, A.a11, A.a12}, {A.a02, A.a12, A.a22}};
  double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < 12; ++sweep) {
    for (int pi = 0; pi < 3; ++pi) {
      const int p = pi == 2 ? 1 : 0, q = pi == 0 ? 1 : 2;  // (0,1), (0,2), (1,2)
      const double apq = a[p][q];
      if (apq == 0.0) continue;
      const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
      const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
      const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
      for (int r = 0; r < 3; ++r) {  // A <- A J
        const double arp = a[r][p], arq = a[r][q];
        a[r][p] = cs * arp - sn * arq;
        a[r][q] = sn * arp + cs * arq;
      }
      for (int r = 0; r < 3; ++r) {  // A <- J' A
        const double apr = a[p][r], aqr = a[q][r];
        a[p][r] = cs * apr - sn * aqr;
        a[q][r] = sn * apr + cs * aqr;
      }
      for (int r = 0; r < 3; ++r) {  // V <- V J
        const double vrp = v[r][p], vrq = v[r][q];
        v[r][p] = cs * vrp - sn * vrq;
        v[r][q] = sn * vrp + cs * vrq;
      }
    }
  }
  int m = 0;
  if (a[1][1] < a[m][m]) m = 1;
  if (a[2][2] < a[m][m]) m = 2;
  const double len = sqrt((v[0][m] * v[0][m] + v[1][m] * v[1][m]) + v[2][m] * v[2][m]);
  n[0] = v[0][m] / len;
  n[1] = v[1][m] / len;
  n[2] = v[2][m] / len;
}

// The full decomposition for the geometric features (features.hip): the same cyclic Jacobi
// (12 sweeps), then lam[0] >= lam[1] >= lam[2] (the rotated diagonal, sorted, ties keep the lower
// column first) and e3 the unit eigenvector of lam[2]. smallest_eigvec above stays as it is: the
// Laplacian and the normals promise bit-identical results through it.
__host__ __device__ inline void sym3_eigh_desc(Sym3 A, double lam[3], double e3[3]) {
  double a[3][3] = {{A.a00, A.a01, A.a02}, {A.a01, A.a11, A.a12}, {A.a02, A.a12, A.a22}};
  double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < 12; ++sweep) {
    for (int pi = 0; pi < 3; ++pi) {
      const int p = pi == 2 ? 1 : 0, q = pi == 0 ? 1 : 2;
      const double apq = a[p][q];
      if (apq == 0.0) continue;
      const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
      const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
      const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
      for (int r = 0; r < 3; ++r) {
        const double arp = a[r][p], arq = a[r][q];
        a[r][p] = cs * arp - sn * arq;
        a[r][q] = sn * arp + cs * arq;
      }
      for (int r = 0; r < 3; ++r) {
        const double apr = a[p][r], aqr = a[q][r];
        a[p][r] = cs * apr - sn * aqr;
        a[q][r] = sn * apr + cs * aqr;
      }
      for (int r = 0; r < 3; ++r) {
        const double vrp = v[r][p], vrq = v[r][q];
        v[r][p] = cs * vrp - sn * vrq;
        v[r][q] = sn * vrp + cs * vrq;
      }
    }
  }
  int o[3] = {0, 1, 2};  // columns by descending eigenvalue (insertion sort, stable)
  for (int s = 1; s < 3; ++s)
    for (int u = s; u > 0 && a[o[u]][o[u]] > a[o[u - 1]][o[u - 1]]; --u) {
      const int tmp = o[u];
      o[u] = o[u - 1];
      o[u - 1] = tmp;
    }
  for (int s = 0; s < 3; ++s) lam[s] = a[o[s]][o[s]];
  const int m = o[2];
  const double len = sqrt((v[0][m] * v[0][m] + v[1][m] * v[1][m]) + v[2][m] * v[2][m]);
  e3[0] = v[0][m] / len;
  e3[1] = v[1][m] / len;
  e3[2] = v[2][m] / len;
}

}  // namespace pyqsm
