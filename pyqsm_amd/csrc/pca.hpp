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

}  // namespace pyqsm
