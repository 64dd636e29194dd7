// Smallest-eigenvalue eigenvector of a symmetric 3x3 in fp64 (cyclic Jacobi), shared by the PCA
// normals of the local triangulation (operators.hip) and of estimate_normals (icp.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace pk_eig {

// a is overwritten by its (nearly) diagonal form; v is a unit vector up to rounding
__device__ inline void min_eigvec3(double a[3][3], double v[3]) {
  double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < 20; ++sweep) {
    const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
    if (off < 1e-30 * (a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2]) + 1e-300) break;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = p + 1; q < 3; ++q) {
        const double apq = a[p][q];
        if (apq == 0.0) continue;
        const double th = (a[q][q] - a[p][p]) / (2.0 * apq);
        const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double arp = a[r][p], arq = a[r][q];
          a[r][p] = c * arp - s * arq;
          a[r][q] = s * arp + c * arq;
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double apr = a[p][r], aqr = a[q][r];
          a[p][r] = c * apr - s * aqr;
          a[q][r] = s * apr + c * aqr;
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double vrp = V[r][p], vrq = V[r][q];
          V[r][p] = c * vrp - s * vrq;
          V[r][q] = s * vrp + c * vrq;
        }
      }
  }
  int m = 0;
  double best = a[0][0];
  if (a[1][1] < best) {
    best = a[1][1];
    m = 1;
  }
  if (a[2][2] < best) m = 2;
#pragma unroll
  for (int r = 0; r < 3; ++r) v[r] = m == 0 ? V[r][0] : (m == 1 ? V[r][1] : V[r][2]);
}

}  // namespace pk_eig
