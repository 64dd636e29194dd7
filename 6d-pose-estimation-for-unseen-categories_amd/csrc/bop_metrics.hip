// BOP pose errors with object symmetry sets, batched over crops, fp64 (absent in the reference;
// restated from bop_toolkit pose_error.py mssd / mspd / adi and misc.get_symmetry_transformations,
// which builds the sets this file consumes — dataset/formats.py symmetry_transformations).
//
//   MSSD = min_S max_x ||T_est x - T_gt S x||
//   MSPD = min_S max_x ||proj(K, T_est x) - proj(K, T_gt S x)||,  proj(K, p) = (K p)_{0,1} / (K p)_2
//   ADI  = mean_x min_y ||T_est x - T_gt y||        (the ADD-S of the papers; no symmetry set)
//
// Four launches, no host read, no floating-point atomic; every reduction has a fixed order:
//   bop_prep_kernel    T_gt y for every vertex, once, into the work buffer as [B, 3, nmax] (SoA).
//   bop_adi_kernel     grid (ceil(nmax / kQB), B), 256 threads x 2 queries = kQB queries T_est x per
//                      workgroup. The crop's transformed targets stream through LDS in tiles of kTT;
//                      every lane reads the same two targets (one 16-byte broadcast read per
//                      coordinate) and updates the running minimum of the squared distance of its two
//                      queries: 3 subtractions, 1 multiply, 2 FMAs and 1 min per pair, all fp64 VALU.
//                      One sqrt per query at the end; the per-query minima go to the work buffer.
//   bop_sym_kernel     grid (ceil(smax / kSC), B): T_gt S composed once per symmetry of the chunk
//                      (kSC of them, in LDS), then every point is transformed once by T_est and kSC
//                      times by T_gt S; per-thread running maxima of the squared 3-D and pixel
//                      distances, block max, sqrt, one value per symmetry into the work buffer.
//   bop_finish_kernel  grid (B): the ADI mean (256 strided partial sums, xor-shuffle tree, 4 wave sums
//                      in order) and the min / first-argmin over the crop's symmetries.
// A crop that is not evaluated (0 points, more than nmax, non-finite T_est) is skipped by the first
// three kernels and written as NaN / -1 by the last.
#include "common.hpp"
#include "posekern.h"

namespace {

constexpr int kQB = PK_BOP_QUERY_BLOCK;  // queries per ADI workgroup (256 threads x 2)
constexpr int kTT = PK_BOP_TARGET_TILE;  // transformed targets per LDS tile (3 x 8 KiB)
constexpr int kSC = PK_BOP_SYM_CHUNK;    // symmetries per MSSD / MSPD workgroup
static_assert(kQB == 512 && kTT % 2 == 0, "two queries per thread, two targets per LDS read");

__device__ __forceinline__ double row(const double* T, int r, double x, double y, double z) {
  return fma(T[4 * r], x, fma(T[4 * r + 1], y, fma(T[4 * r + 2], z, T[4 * r + 3])));
}

// the crop's point count and first row; false when the crop is not evaluated
__device__ __forceinline__ bool crop_ok(const int64_t* __restrict__ off, const double* __restrict__ Te, int b,
                                        int nmax, int& n, int64_t& o) {
  o = off[b];
  const int64_t c = off[b + 1] - o;
  n = 0;
  if (c < 1 || c > (int64_t)nmax) return false;
  n = (int)c;
  bool fin = true;
  for (int k = 0; k < 16; ++k) fin = fin && isfinite(Te[16 * b + k]);
  return fin;
}

// grid (ceil(nmax/256), B)
__global__ __launch_bounds__(256) void bop_prep_kernel(const double* __restrict__ cad, const int64_t* __restrict__ off,
                                                       const double* __restrict__ Te, const double* __restrict__ Tg,
                                                       int nmax, double* __restrict__ tg /*[B,3,nmax]*/) {
  const int b = blockIdx.y;
  int n;
  int64_t o;
  if (!crop_ok(off, Te, b, nmax, n, o)) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double* p = cad + 3 * (o + i);
  const double x = p[0], y = p[1], z = p[2];
  const double* T = Tg + 16 * b;
  double* g = tg + (int64_t)b * 3 * nmax;
  g[i] = row(T, 0, x, y, z);
  g[(int64_t)nmax + i] = row(T, 1, x, y, z);
  g[2 * (int64_t)nmax + i] = row(T, 2, x, y, z);
}

__device__ __forceinline__ double dist2(double qx, double qy, double qz, double tx, double ty, double tz) {
  const double dx = qx - tx, dy = qy - ty, dz = qz - tz;
  return fma(dz, dz, fma(dy, dy, dx * dx));
}

// grid (ceil(nmax/kQB), B)
__global__ __launch_bounds__(256) void bop_adi_kernel(const double* __restrict__ cad, const int64_t* __restrict__ off,
                                                      const double* __restrict__ Te, const double* __restrict__ tg,
                                                      int nmax, double* __restrict__ qmin /*[B,nmax]*/) {
  __shared__ __attribute__((aligned(16))) double tile[3][kTT];
  const int b = blockIdx.y;
  int n;
  int64_t o;
  if (!crop_ok(off, Te, b, nmax, n, o)) return;
  const int q0 = blockIdx.x * kQB;
  if (q0 >= n) return;
  const int i0 = q0 + threadIdx.x, i1 = i0 + 256;
  const double* T = Te + 16 * b;
  // a thread past the crop's end works on point 0 and stores nothing
  const double* p0 = cad + 3 * (o + (i0 < n ? i0 : 0));
  const double* p1 = cad + 3 * (o + (i1 < n ? i1 : 0));
  const double ax = row(T, 0, p0[0], p0[1], p0[2]), ay = row(T, 1, p0[0], p0[1], p0[2]),
               az = row(T, 2, p0[0], p0[1], p0[2]);
  const double bx = row(T, 0, p1[0], p1[1], p1[2]), by = row(T, 1, p1[0], p1[1], p1[2]),
               bz = row(T, 2, p1[0], p1[1], p1[2]);
  double besta = __builtin_huge_val(), bestb = __builtin_huge_val();
  const double* g = tg + (int64_t)b * 3 * nmax;
  for (int t0 = 0; t0 < n; t0 += kTT) {
    const int tn = min(kTT, n - t0);
    const int tp = (tn + 1) & ~1;  // an odd tile repeats its first target in the last slot
    __syncthreads();
    for (int k = threadIdx.x; k < tp; k += 256) {
      const int src = t0 + (k < tn ? k : 0);
      tile[0][k] = g[src];
      tile[1][k] = g[(int64_t)nmax + src];
      tile[2][k] = g[2 * (int64_t)nmax + src];
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < tp; k += 2) {
      const double2 tx = *reinterpret_cast<const double2*>(&tile[0][k]);
      const double2 ty = *reinterpret_cast<const double2*>(&tile[1][k]);
      const double2 tz = *reinterpret_cast<const double2*>(&tile[2][k]);
      besta = fmin(besta, dist2(ax, ay, az, tx.x, ty.x, tz.x));
      bestb = fmin(bestb, dist2(bx, by, bz, tx.x, ty.x, tz.x));
      besta = fmin(besta, dist2(ax, ay, az, tx.y, ty.y, tz.y));
      bestb = fmin(bestb, dist2(bx, by, bz, tx.y, ty.y, tz.y));
    }
  }
  if (i0 < n) qmin[(int64_t)b * nmax + i0] = sqrt(besta);
  if (i1 < n) qmin[(int64_t)b * nmax + i1] = sqrt(bestb);
}

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// grid (ceil(smax/kSC), B)
__global__ __launch_bounds__(256) void bop_sym_kernel(const double* __restrict__ cad, const int64_t* __restrict__ off,
                                                      const double* __restrict__ Te, const double* __restrict__ Tg,
                                                      const double* __restrict__ K, const double* __restrict__ sym,
                                                      const int64_t* __restrict__ sym_off, int nmax, int smax,
                                                      double* __restrict__ symmax /*[B,smax,2]*/) {
  __shared__ double M[kSC][12];      // rows 0..2 of T_gt S
  __shared__ double red[4][2 * kSC];
  const int b = blockIdx.y;
  int n;
  int64_t o;
  if (!crop_ok(off, Te, b, nmax, n, o)) return;
  const int64_t so = sym ? sym_off[b] : 0;
  const int64_t nsl = sym ? sym_off[b + 1] - so : 1;
  if (nsl < 1 || nsl > (int64_t)smax) return;
  const int ns = (int)nsl;
  const int s0 = blockIdx.x * kSC;
  if (s0 >= ns) return;
  const int sc = min(kSC, ns - s0);
  if ((int)threadIdx.x < sc) {
    const double* G = Tg + 16 * b;
    double* m = M[threadIdx.x];
    if (sym) {  // T_gt S: R = R_gt R_s, t = R_gt t_s + t_gt
      const double* S = sym + 16 * (so + s0 + threadIdx.x);
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) m[4 * r + c] = fma(G[4 * r], S[c], fma(G[4 * r + 1], S[4 + c], G[4 * r + 2] * S[8 + c]));
        m[4 * r + 3] = row(G, r, S[3], S[7], S[11]);
      }
    } else {
      for (int k = 0; k < 12; ++k) m[k] = G[k];
    }
  }
  __syncthreads();
  const double* T = Te + 16 * b;
  const double* Kb = K ? K + 9 * b : nullptr;
  double m3[kSC], m2[kSC];
#pragma unroll
  for (int s = 0; s < kSC; ++s) m3[s] = m2[s] = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double* p = cad + 3 * (o + i);
    const double x = p[0], y = p[1], z = p[2];
    const double ex = row(T, 0, x, y, z), ey = row(T, 1, x, y, z), ez = row(T, 2, x, y, z);
    double eu = 0.0, ev = 0.0;
    if (Kb) {
      const double w = fma(Kb[6], ex, fma(Kb[7], ey, Kb[8] * ez));
      eu = fma(Kb[0], ex, fma(Kb[1], ey, Kb[2] * ez)) / w;
      ev = fma(Kb[3], ex, fma(Kb[4], ey, Kb[5] * ez)) / w;
    }
#pragma unroll
    for (int s = 0; s < kSC; ++s) {
      if (s < sc) {
        const double gx = row(M[s], 0, x, y, z), gy = row(M[s], 1, x, y, z), gz = row(M[s], 2, x, y, z);
        m3[s] = fmax(m3[s], dist2(ex, ey, ez, gx, gy, gz));
        if (Kb) {
          const double w = fma(Kb[6], gx, fma(Kb[7], gy, Kb[8] * gz));
          const double du = eu - fma(Kb[0], gx, fma(Kb[1], gy, Kb[2] * gz)) / w;
          const double dv = ev - fma(Kb[3], gx, fma(Kb[4], gy, Kb[5] * gz)) / w;
          m2[s] = fmax(m2[s], fma(dv, dv, du * du));
        }
      }
    }
  }
#pragma unroll
  for (int s = 0; s < kSC; ++s) {
    const double a = wave_max_f64(m3[s]), c = wave_max_f64(m2[s]);
    if (pk::lane_id() == 0) {
      red[pk::wave_id()][2 * s] = a;
      red[pk::wave_id()][2 * s + 1] = c;
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < 2 * sc && (Kb || (t & 1) == 0)) {
    const double v = fmax(fmax(red[0][t], red[1][t]), fmax(red[2][t], red[3][t]));
    symmax[((int64_t)b * smax + s0) * 2 + t] = sqrt(v);
  }
}

// (value, index) pairs ordered by value, then index: the first minimum
__device__ __forceinline__ void take_min(double& v, int& i, double ov, int oi) {
  if (ov < v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

// grid (B)
__global__ __launch_bounds__(256) void bop_finish_kernel(const int64_t* __restrict__ off, const double* __restrict__ Te,
                                                         const double* __restrict__ K, const double* __restrict__ sym,
                                                         const int64_t* __restrict__ sym_off, int nmax, int smax,
                                                         const double* __restrict__ qmin,
                                                         const double* __restrict__ symmax, double* __restrict__ out,
                                                         int32_t* __restrict__ best) {
  __shared__ double ws[4];
  __shared__ double wv[2][4];
  __shared__ int wi[2][4];
  const int b = blockIdx.x;
  const double nan = __builtin_nan("");
  int n;
  int64_t o;
  if (!crop_ok(off, Te, b, nmax, n, o)) {
    if (threadIdx.x == 0) {
      out[3 * b] = out[3 * b + 1] = out[3 * b + 2] = nan;
      best[2 * b] = best[2 * b + 1] = -1;
    }
    return;
  }
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += qmin[(int64_t)b * nmax + i];
  s = pk::wave_sum_f64(s);
  if (pk::lane_id() == 0) ws[pk::wave_id()] = s;
  const int64_t nsl = sym ? sym_off[b + 1] - sym_off[b] : 1;
  const int ns = (nsl < 1 || nsl > (int64_t)smax) ? 0 : (int)nsl;
  for (int c = 0; c < 2; ++c) {
    double v = __builtin_huge_val();
    int idx = 0x7fffffff;
    if (c == 0 || K) {
      for (int k = threadIdx.x; k < ns; k += 256) take_min(v, idx, symmax[((int64_t)b * smax + k) * 2 + c], k);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const double ov = __shfl_xor(v, m);
      const int oi = __shfl_xor(idx, m);
      take_min(v, idx, ov, oi);
    }
    if (pk::lane_id() == 0) {
      wv[c][pk::wave_id()] = v;
      wi[c][pk::wave_id()] = idx;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    out[3 * b + 2] = ((ws[0] + ws[1]) + (ws[2] + ws[3])) / (double)n;
    for (int c = 0; c < 2; ++c) {
      double v = wv[c][0];
      int idx = wi[c][0];
      for (int w = 1; w < 4; ++w) take_min(v, idx, wv[c][w], wi[c][w]);
      const bool found = idx != 0x7fffffff;
      out[3 * b + c] = found ? v : nan;
      best[2 * b + c] = found ? idx : -1;
    }
  }
}

}  // namespace

extern "C" int pk_bop_errors(const double* cad, const int64_t* off, int B, int nmax, const double* T_est,
                             const double* T_gt, const double* K, const double* sym, const int64_t* sym_off,
                             int smax, double* work, double* out, int32_t* best, void* stream) {
  PK_REQUIRE(B >= 0 && nmax >= 0);
  if (B == 0 || nmax == 0) return PK_OK;
  PK_REQUIRE(cad && off && T_est && T_gt && work && out && best);
  if (sym) {
    PK_REQUIRE(sym_off && smax >= 1);
  } else {
    smax = 1;
  }
  PK_REQUIRE(B <= 65535);  // crops ride on gridDim.y
  hipStream_t s = pk::as_stream(stream);
  double* tg = work;                               // [B, 3, nmax]
  double* qmin = tg + (int64_t)B * 3 * nmax;       // [B, nmax]
  double* symmax = qmin + (int64_t)B * nmax;       // [B, smax, 2]
  hipLaunchKernelGGL(bop_prep_kernel, dim3((nmax + 255) / 256, B), dim3(256), 0, s, cad, off, T_est, T_gt, nmax, tg);
  PK_CHECK_LAUNCH();
  hipLaunchKernelGGL(bop_adi_kernel, dim3((nmax + kQB - 1) / kQB, B), dim3(256), 0, s, cad, off, T_est, tg, nmax, qmin);
  PK_CHECK_LAUNCH();
  hipLaunchKernelGGL(bop_sym_kernel, dim3((smax + kSC - 1) / kSC, B), dim3(256), 0, s, cad, off, T_est, T_gt, K, sym,
                     sym_off, nmax, smax, symmax);
  PK_CHECK_LAUNCH();
  hipLaunchKernelGGL(bop_finish_kernel, dim3(B), dim3(256), 0, s, off, T_est, K, sym, sym_off, nmax, smax, qmin,
                     symmax, out, best);
  PK_CHECK_LAUNCH();
  return PK_OK;
}
