// (f1) Gradient operators on the device: upstream diffusion-net geometry.build_grad /
// build_grad_point_cloud / edge_tangent_vectors (the gradX / gradY of compute_operators), for a
// packed batch in one launch.
//
//   pk_grad_build   per point i with outgoing neighbours j_1..j_m (a fixed-width table, -1 = empty):
//                   the edges projected on i's tangent basis a_t = ((p_j - p_i) . X_i, (p_j - p_i) . Y_i),
//                   the 2 x 2 normal matrix M = sum a_t a_t^T + 1e-5 I, the least-squares rows
//                   c_t = M^-1 a_t and the diagonal c_0 = -sum c_t. fp64, one thread per point, every
//                   sum in slot order (-ffp-contract=off: each product and sum rounded on its own, so
//                   a host restatement in the same order agrees to the last few bits).
//
// The rows keep the table's width: slot 0 is the point itself, slot t the table's entry t - 1, so
// the layer kernels (csrc/gradfeat.hip) read 31 x 2 values and 31 indices per point, no CSR.
// Parity unpinned (the upstream package is absent); tests/_gradfeat_ref.py restates it.
#include "common.hpp"
#include "posekern.h"

namespace {

// grid ceil(B nmax / 256)
__global__ __launch_bounds__(256) void grad_build_kernel(const double* __restrict__ pts, const int64_t* __restrict__ off,
                                                         int B, int nmax, const double* __restrict__ frames,
                                                         const int32_t* __restrict__ nbr, int W,
                                                         int32_t* __restrict__ idx, double* __restrict__ val) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (int64_t)B * nmax) return;
  const int b = (int)(g / nmax), i = (int)(g - (int64_t)b * nmax);
  const int64_t p0 = off[b];
  const int n = (int)(off[b + 1] - p0);
  int32_t* oi = idx + g * W;
  double* ov = val + g * W * 2;
  if (i >= n) {  // past the crop: an empty row
    for (int s = 0; s < W; ++s) {
      oi[s] = -1;
      ov[2 * s] = 0.0;
      ov[2 * s + 1] = 0.0;
    }
    return;
  }
  const double* P = pts + 3 * p0;
  const double* F = frames + 9 * (p0 + i);
  const int32_t* nb = nbr + (p0 + i) * (int64_t)(W - 1);
  const double px = P[3 * i], py = P[3 * i + 1], pz = P[3 * i + 2];
  const double bx0 = F[0], bx1 = F[1], bx2 = F[2], by0 = F[3], by1 = F[4], by2 = F[5];
  // pass 1: M = sum a a^T in slot order (the edge coordinates are recomputed in pass 2: the same
  // arithmetic, the same bits)
  double m00 = 0.0, m01 = 0.0, m11 = 0.0;
  for (int t = 0; t < W - 1; ++t) {
    const int j = nb[t];
    if (j < 0 || j >= n || j == i) continue;
    const double ex = P[3 * j] - px, ey = P[3 * j + 1] - py, ez = P[3 * j + 2] - pz;
    const double ax = (ex * bx0 + ey * bx1) + ez * bx2;
    const double ay = (ex * by0 + ey * by1) + ez * by2;
    m00 += ax * ax;
    m01 += ax * ay;
    m11 += ay * ay;
  }
  m00 += 1e-5;
  m11 += 1e-5;
  const double det = m00 * m11 - m01 * m01;
  double s0 = 0.0, s1 = 0.0;
  for (int t = 0; t < W - 1; ++t) {
    const int j = nb[t];
    double c0 = 0.0, c1 = 0.0;
    int jj = -1;
    if (!(j < 0 || j >= n || j == i)) {
      const double ex = P[3 * j] - px, ey = P[3 * j + 1] - py, ez = P[3 * j + 2] - pz;
      const double ax = (ex * bx0 + ey * bx1) + ez * bx2;
      const double ay = (ex * by0 + ey * by1) + ez * by2;
      c0 = (m11 * ax - m01 * ay) / det;
      c1 = (m00 * ay - m01 * ax) / det;
      s0 += c0;
      s1 += c1;
      jj = j;
    }
    oi[t + 1] = jj;
    ov[2 * (t + 1)] = c0;
    ov[2 * (t + 1) + 1] = c1;
  }
  oi[0] = i;
  ov[0] = -s0;
  ov[1] = -s1;
}

}  // namespace

extern "C" int pk_grad_build(const double* pts, const int64_t* off, int B, int nmax, const double* frames,
                             const int32_t* nbr, int W, int32_t* idx, double* val, void* stream) {
  PK_REQUIRE(B >= 0 && nmax >= 0 && W >= 2);
  if (B == 0 || nmax == 0) return PK_OK;
  PK_REQUIRE(pts && off && frames && nbr && idx && val);
  const int64_t total = (int64_t)B * nmax;
  PK_REQUIRE((total + 255) / 256 <= (int64_t)INT32_MAX);
  hipLaunchKernelGGL(grad_build_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, pk::as_stream(stream), pts,
                     off, B, nmax, frames, nbr, W, idx, val);
  PK_CHECK_LAUNCH();
  return PK_OK;
}
