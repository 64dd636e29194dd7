// DiffusionNet gradient features (upstream diffusion-net layers.py SpatialGradientFeatures and the
// block that consumes them), f32, C = 64, on the fixed-width gradient operator of csrc/gradop.hip
// (idx int32 [B,N,W], val f32 [B,N,W,2]: slot s of row i names a source point and its gradX / gradY
// coefficient; -1 = empty).
//
//   pk_grad_apply     v = [gradX x | gradY x]: per point a gather of <= W rows of 256 B. 16 lanes x
//                     float4 own one point (4 points per wave), the W coefficient pairs and indices
//                     are broadcast loads. A crop's x (<= 512 KB at 2048 points) is re-read ~W times:
//                     the grid is renumbered (pk::xcd_block3) so that a crop's workgroups share one
//                     XCD's L2. Bound by that L2 gather (W x 256 B per point); algorithmic (HBM)
//                     bytes = x in + v out + the operator. Loading 8 slots' rows before summing any
//                     did not shorten it (and lengthened the transpose by a tenth): the plain loop stays.
//   pk_grad_apply_t   dx = gradX^T dvX + gradY^T dvY through the inverted index (per destination, its
//                     (row, slot) contributions in ascending order): a gather again, no atomics, the
//                     order of every sum fixed -> bitwise reproducible. The loop length is the
//                     destination's in-degree (skewed: up to ~2x the out-degree W on a kNN graph);
//                     nothing is sized by W, a 16-lane group simply runs its own list.
//   pk_gradfeat_fwd   g = tanh(vX . B_re + vY . B_im), [B_re | B_im] = [vX | vY] x the stacked
//                     128 x 128 rotation weight [[A_re^T, A_im^T], [-A_im^T, A_re^T]] on
//                     v_mfma_f32_32x32x2_f32: one wave = 32 points x 128 outputs (four 32 x 32
//                     accumulators); the lane halves split the contraction as in linear_fwd.hip — half 0
//                     holds the point's vX row, half 1 its vY row, so MFMA step s contracts the pair
//                     (vX[s], vY[s]) against rows (A_re[:, s], -A_im[:, s]) / (A_im[:, s], A_re[:, s])
//                     read from one LDS copy of A_re and A_im (the stacked matrix is never built).
//                     Without rotations A_im = 0 (the block-diagonal weight).
//   pk_gradfeat_bwd   recomputes B the same way, scales it by ds = dg (1 - g^2) (the ds . B terms
//                     of dv) and adds [P | Q] x the transposed stacked weight in a second MFMA pass
//                     (P = ds . vX, Q = ds . vY, formed in place in the operand registers and written
//                     out as the weight gradients' operands).
//   pk_linear192_fwd  the block's first MLP layer on 192 inputs (pk_linear_ex stops at 128): the
//                     same 32-points-per-wave product with 96 contraction steps per lane half.
#include "common.hpp"
#include "mfma_tile.hpp"
#include "posekern.h"

namespace {

using pk::f32x16;
using pk::al16;
using pk::al8;

constexpr int kGfC = 64;
constexpr int kGfST = kGfC + 1;          // LDS row stride of a 64 x 64 weight (odd: conflict-free both ways)
constexpr int kGfW = kGfC * kGfST;       // floats of one weight copy
constexpr int kPtsPerBlock = 16;         // grad_apply / grad_apply_t: 16 lanes per point, 256 threads

// grid (ceil(N / 16), B): logical block (x, b) after the XCD renumbering
__global__ __launch_bounds__(256) void grad_apply_kernel(const float* __restrict__ x, int64_t ldx,
                                                         const int32_t* __restrict__ idx,
                                                         const float* __restrict__ val, int N, int W,
                                                         float* __restrict__ v) {
  const int3 lb = pk::xcd_block3();
  const int b = lb.y;
  const int i = lb.x * kPtsPerBlock + (threadIdx.x >> 4);
  const int c4 = (threadIdx.x & 15) * 4;
  if (i >= N) return;
  const int64_t row = (int64_t)b * N + i;
  const int32_t* ii = idx + row * W;
  const float2* cc = reinterpret_cast<const float2*>(val) + row * W;
  const float* xb = x + (int64_t)b * N * ldx + c4;
  float4 ax = make_float4(0.f, 0.f, 0.f, 0.f), ay = ax;
  for (int s = 0; s < W; ++s) {
    const int j = ii[s];
    if (j < 0 || j >= N) continue;
    const float2 c = cc[s];
    const float4 xr = *reinterpret_cast<const float4*>(xb + (int64_t)j * ldx);
    ax.x = fmaf(c.x, xr.x, ax.x);
    ax.y = fmaf(c.x, xr.y, ax.y);
    ax.z = fmaf(c.x, xr.z, ax.z);
    ax.w = fmaf(c.x, xr.w, ax.w);
    ay.x = fmaf(c.y, xr.x, ay.x);
    ay.y = fmaf(c.y, xr.y, ay.y);
    ay.z = fmaf(c.y, xr.z, ay.z);
    ay.w = fmaf(c.y, xr.w, ay.w);
  }
  float* o = v + row * (2 * kGfC) + c4;
  *reinterpret_cast<float4*>(o) = ax;
  *reinterpret_cast<float4*>(o + kGfC) = ay;
}

// grid (ceil(N / 16), B)
__global__ __launch_bounds__(256) void grad_apply_t_kernel(const float* __restrict__ dv,
                                                           const int32_t* __restrict__ tptr,
                                                           const int32_t* __restrict__ tsrc,
                                                           const float* __restrict__ val, int N, int W,
                                                           float* __restrict__ dx, int64_t lddx, int accumulate) {
  const int3 lb = pk::xcd_block3();
  const int b = lb.y;
  const int j = lb.x * kPtsPerBlock + (threadIdx.x >> 4);
  const int c4 = (threadIdx.x & 15) * 4;
  if (j >= N) return;
  const int NW = N * W;
  int p0 = tptr[(int64_t)b * (N + 1) + j], p1 = tptr[(int64_t)b * (N + 1) + j + 1];
  p0 = max(p0, 0);
  p1 = min(p1, NW);
  const int32_t* src = tsrc + (int64_t)b * NW;
  const float2* cc = reinterpret_cast<const float2*>(val) + (int64_t)b * NW;
  const float* db = dv + (int64_t)b * N * (2 * kGfC) + c4;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int p = p0; p < p1; ++p) {
    const int e = src[p];
    if (e < 0 || e >= NW) continue;
    const float2 c = cc[e];
    const float* r = db + (int64_t)(e / W) * (2 * kGfC);
    const float4 gx = *reinterpret_cast<const float4*>(r);
    const float4 gy = *reinterpret_cast<const float4*>(r + kGfC);
    a.x = fmaf(c.y, gy.x, fmaf(c.x, gx.x, a.x));
    a.y = fmaf(c.y, gy.y, fmaf(c.x, gx.y, a.y));
    a.z = fmaf(c.y, gy.z, fmaf(c.x, gx.z, a.z));
    a.w = fmaf(c.y, gy.w, fmaf(c.x, gx.w, a.w));
  }
  float4* o = reinterpret_cast<float4*>(dx + ((int64_t)b * N + j) * lddx + c4);
  if (accumulate) {
    const float4 old = *o;
    a.x += old.x;
    a.y += old.y;
    a.z += old.z;
    a.w += old.w;
  }
  *o = a;
}

// A_re and A_im (zeros when absent) as S[0 .. kGfW) and S[kGfW .. 2 kGfW), rows of stride kGfST
__device__ __forceinline__ void gf_load_weights(const float* __restrict__ A_re, const float* __restrict__ A_im,
                                                float* S) {
  for (int e = threadIdx.x; e < kGfC * kGfC; e += 256) {
    const int o = e >> 6, k = e & 63;
    S[o * kGfST + k] = A_re[e];
    S[kGfW + o * kGfST + k] = A_im != nullptr ? A_im[e] : 0.f;
  }
}

// this lane's half row (64 floats at p, or zeros)
__device__ __forceinline__ void gf_load_half(const float* p, bool ok, float (&xa)[kGfC]) {
#pragma unroll
  for (int q = 0; q < kGfC / 4; ++q) {
    const float4 t = ok ? reinterpret_cast<const float4*>(p)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    xa[4 * q] = t.x;
    xa[4 * q + 1] = t.y;
    xa[4 * q + 2] = t.z;
    xa[4 * q + 3] = t.w;
  }
}

// acc[t] += [a0 | a1] x stacked weight, a0 / a1 = the half rows held by lane halves 0 / 1 (xa):
//   TRANS = false (forward):  columns of acc[0..1] = a0 A_re^T - a1 A_im^T, acc[2..3] = a0 A_im^T + a1 A_re^T
//   TRANS = true  (backward): columns of acc[0..1] = a0 A_re + a1 A_im,     acc[2..3] = -a0 A_im + a1 A_re
// Lane half h reads A_re or A_im by an offset and a sign of its own: one LDS read per MFMA.
template <bool TRANS>
__device__ __forceinline__ void gf_product(const float (&xa)[kGfC], const float* S, int m, int h, f32x16 (&acc)[4]) {
  const int base01 = h ? kGfW : 0, base23 = h ? 0 : kGfW;
  const float sg01 = (!TRANS && h) ? -1.f : 1.f;
  const float sg23 = (TRANS && !h) ? -1.f : 1.f;
#pragma unroll
  for (int s = 0; s < kGfC; ++s) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int o = (t & 1) * 32 + m;
      const int a = TRANS ? s * kGfST + o : o * kGfST + s;
      const float wv = t < 2 ? sg01 * S[base01 + a] : sg23 * S[base23 + a];
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[s], wv, acc[t], 0, 0, 0);
    }
  }
}

// D element e of a 32 x 32 accumulator: row 8 (e / 4) + 4 h + e % 4, column m
__device__ __forceinline__ int gf_row(int e, int h) { return 8 * (e >> 2) + 4 * h + (e & 3); }

// grid ceil(R / 128), 4 waves x 32 points
__global__ __launch_bounds__(256) void gradfeat_fwd_kernel(const float* __restrict__ v, const float* __restrict__ A_re,
                                                           const float* __restrict__ A_im, int64_t R,
                                                           float* __restrict__ g, int64_t ldg) {
  __shared__ float S[2 * kGfW];
  gf_load_weights(A_re, A_im, S);
  __syncthreads();
  const int lane = pk::lane_id(), wave = pk::wave_id();
  const int m = lane & 31, h = lane >> 5;
  const int64_t r0 = ((int64_t)blockIdx.x * 4 + wave) * 32;
  if (r0 >= R) return;
  const int64_t r = r0 + m;
  float xa[kGfC];
  gf_load_half(v + r * (2 * kGfC) + h * kGfC, r < R, xa);
  f32x16 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
  gf_product<false>(xa, S, m, h, acc);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int64_t pr = r0 + gf_row(e, h);
      const int c = t * 32 + m;
      if (pr < R) {
        const float vx = v[pr * (2 * kGfC) + c], vy = v[pr * (2 * kGfC) + kGfC + c];
        g[pr * ldg + c] = tanhf(vx * acc[t][e] + vy * acc[t + 2][e]);
      }
    }
  }
}

__global__ __launch_bounds__(256) void gradfeat_bwd_kernel(const float* __restrict__ dg, int64_t lddg,
                                                           const float* __restrict__ g, int64_t ldg,
                                                           const float* __restrict__ v, const float* __restrict__ A_re,
                                                           const float* __restrict__ A_im, int64_t R,
                                                           float* __restrict__ dv, float* __restrict__ pq) {
  __shared__ float S[2 * kGfW];
  gf_load_weights(A_re, A_im, S);
  __syncthreads();
  const int lane = pk::lane_id(), wave = pk::wave_id();
  const int m = lane & 31, h = lane >> 5;
  const int64_t r0 = ((int64_t)blockIdx.x * 4 + wave) * 32;
  if (r0 >= R) return;
  const int64_t r = r0 + m;
  const bool ok = r < R;
  float xa[kGfC];
  gf_load_half(v + r * (2 * kGfC) + h * kGfC, ok, xa);
  f32x16 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
  gf_product<false>(xa, S, m, h, acc);  // B_re | B_im
  // dv starts from ds . B
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int64_t pr = r0 + gf_row(e, h);
      const int c = t * 32 + m;
      float ds = 0.f;
      if (pr < R) {
        const float gg = g[pr * ldg + c];
        ds = dg[pr * lddg + c] * (1.f - gg * gg);
      }
      acc[t][e] *= ds;
      acc[t + 2][e] *= ds;
    }
  }
  // P = ds . vX (half 0) / Q = ds . vY (half 1) in place of the operand row, and out to pq [2, R, 64]
  {
    const float4* dgr = reinterpret_cast<const float4*>(dg + r * lddg);
    const float4* gr = reinterpret_cast<const float4*>(g + r * ldg);
    float4* out = reinterpret_cast<float4*>(pq + ((int64_t)h * R + r) * kGfC);
#pragma unroll
    for (int q = 0; q < kGfC / 4; ++q) {
      if (ok) {
        const float4 d4 = dgr[q], g4 = gr[q];
        float4 p;
        p.x = xa[4 * q] = d4.x * (1.f - g4.x * g4.x) * xa[4 * q];
        p.y = xa[4 * q + 1] = d4.y * (1.f - g4.y * g4.y) * xa[4 * q + 1];
        p.z = xa[4 * q + 2] = d4.z * (1.f - g4.z * g4.z) * xa[4 * q + 2];
        p.w = xa[4 * q + 3] = d4.w * (1.f - g4.w * g4.w) * xa[4 * q + 3];
        out[q] = p;
      }
    }
  }
  gf_product<true>(xa, S, m, h, acc);  // + P A_re + Q A_im | - P A_im + Q A_re
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int64_t pr = r0 + gf_row(e, h);
      if (pr < R) dv[pr * (2 * kGfC) + (t >> 1) * kGfC + (t & 1) * 32 + m] = acc[t][e];
    }
  }
}

constexpr int kL192In = 192;
constexpr int kL192ST = kL192In + 1;

// y [R, 64] = act(x W^T + b), x rows of 192 at stride ldx; grid ceil(R / 128)
__global__ __launch_bounds__(256) void linear192_kernel(const float* __restrict__ x, int64_t ldx,
                                                        const float* __restrict__ w, const float* __restrict__ bias,
                                                        int64_t R, int relu, float* __restrict__ y) {
  __shared__ float Ws[kGfC * kL192ST];
  for (int e = threadIdx.x; e < kGfC * kL192In; e += 256) {
    const int o = e / kL192In, k = e - o * kL192In;
    Ws[o * kL192ST + k] = w[e];
  }
  __syncthreads();
  const int lane = pk::lane_id(), wave = pk::wave_id();
  const int m = lane & 31, h = lane >> 5;
  const int64_t r0 = ((int64_t)blockIdx.x * 4 + wave) * 32;
  if (r0 >= R) return;
  const int64_t r = r0 + m;
  const bool ok = r < R;
  constexpr int KH = kL192In / 2;
  float xa[KH];
  {
    const float4* p = reinterpret_cast<const float4*>(x + r * ldx + h * KH);
#pragma unroll
    for (int q = 0; q < KH / 4; ++q) {
      const float4 t = ok ? p[q] : make_float4(0.f, 0.f, 0.f, 0.f);
      xa[4 * q] = t.x;
      xa[4 * q + 1] = t.y;
      xa[4 * q + 2] = t.z;
      xa[4 * q + 3] = t.w;
    }
  }
  f32x16 acc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
#pragma unroll
  for (int s = 0; s < KH; ++s) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[s], Ws[(t * 32 + m) * kL192ST + h * KH + s], acc[t], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int o = t * 32 + m;
    const float bv = bias != nullptr ? bias[o] : 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int64_t pr = r0 + gf_row(e, h);
      if (pr < R) {
        float val = acc[t][e] + bv;
        if (relu) val = fmaxf(val, 0.f);
        y[pr * kGfC + o] = val;
      }
    }
  }
}

}  // namespace

extern "C" int pk_grad_apply(const float* x, int64_t ldx, const int32_t* idx, const float* val, int B, int N, int W,
                             int C, float* v, void* stream) {
  PK_REQUIRE(C == kGfC && B >= 0 && N >= 0 && W >= 1 && B <= 65535);
  if (B == 0 || N == 0) return PK_OK;
  PK_REQUIRE(x && idx && val && v && ldx >= C && ldx % 4 == 0 && al16(x) && al16(v) && al8(val));
  PK_REQUIRE((int64_t)N * W <= (int64_t)INT32_MAX);
  hipLaunchKernelGGL(grad_apply_kernel, dim3((N + kPtsPerBlock - 1) / kPtsPerBlock, B), dim3(256), 0,
                     pk::as_stream(stream), x, ldx, idx, val, N, W, v);
  PK_CHECK_LAUNCH();
  return PK_OK;
}

extern "C" int pk_grad_apply_t(const float* dv, const int32_t* tptr, const int32_t* tsrc, const float* val, int B, int N,
                               int W, int C, float* dx, int64_t lddx, int accumulate, void* stream) {
  PK_REQUIRE(C == kGfC && B >= 0 && N >= 0 && W >= 1 && B <= 65535);
  if (B == 0 || N == 0) return PK_OK;
  PK_REQUIRE(dv && tptr && tsrc && val && dx && lddx >= C && lddx % 4 == 0 && al16(dv) && al16(dx) && al8(val));
  PK_REQUIRE((int64_t)N * W <= (int64_t)INT32_MAX);
  hipLaunchKernelGGL(grad_apply_t_kernel, dim3((N + kPtsPerBlock - 1) / kPtsPerBlock, B), dim3(256), 0,
                     pk::as_stream(stream), dv, tptr, tsrc, val, N, W, dx, lddx, accumulate);
  PK_CHECK_LAUNCH();
  return PK_OK;
}

extern "C" int pk_gradfeat_fwd(const float* v, const float* A_re, const float* A_im, int64_t R, int C, float* g,
                               int64_t ldg, void* stream) {
  PK_REQUIRE(C == kGfC && R >= 0);
  if (R == 0) return PK_OK;
  PK_REQUIRE(v && A_re && g && ldg >= C && al16(v));
  PK_REQUIRE((R + 127) / 128 <= (int64_t)INT32_MAX);
  hipLaunchKernelGGL(gradfeat_fwd_kernel, dim3((unsigned)((R + 127) / 128)), dim3(256), 0, pk::as_stream(stream), v,
                     A_re, A_im, R, g, ldg);
  PK_CHECK_LAUNCH();
  return PK_OK;
}

extern "C" int pk_gradfeat_bwd(const float* dg, int64_t lddg, const float* g, int64_t ldg, const float* v,
                               const float* A_re, const float* A_im, int64_t R, int C, float* dv, float* pq,
                               void* stream) {
  PK_REQUIRE(C == kGfC && R >= 0);
  if (R == 0) return PK_OK;
  PK_REQUIRE(dg && g && v && A_re && dv && pq && lddg >= C && ldg >= C && lddg % 4 == 0 && ldg % 4 == 0);
  PK_REQUIRE(al16(dg) && al16(g) && al16(v) && al16(pq));
  PK_REQUIRE((R + 127) / 128 <= (int64_t)INT32_MAX);
  hipLaunchKernelGGL(gradfeat_bwd_kernel, dim3((unsigned)((R + 127) / 128)), dim3(256), 0, pk::as_stream(stream), dg,
                     lddg, g, ldg, v, A_re, A_im, R, dv, pq);
  PK_CHECK_LAUNCH();
  return PK_OK;
}

extern "C" int pk_linear192_fwd(const float* x, int64_t ldx, const float* w, const float* bias, int64_t R, int relu,
                                float* y, void* stream) {
  PK_REQUIRE(R >= 0);
  if (R == 0) return PK_OK;
  PK_REQUIRE(x && w && y && ldx >= kL192In && ldx % 4 == 0 && al16(x));
  PK_REQUIRE((R + 127) / 128 <= (int64_t)INT32_MAX);
  hipLaunchKernelGGL(linear192_kernel, dim3((unsigned)((R + 127) / 128)), dim3(256), 0, pk::as_stream(stream), x, ldx, w,
                     bias, R, relu, y);
  PK_CHECK_LAUNCH();
  return PK_OK;
}
