// ---- DiffusionNet block MLP as one chain per direction (pk_mlp3_fwd / pk_mlp3_bwd) ----
// The block's three per-point layers (128 -> 64 -> 64 -> 64, upstream DiffusionNetBlock.forward,
// models/dpfm.py:22-30) on the pipeline of linear_glds_rows_kernel, one launch per direction:
//   forward  h1 = relu(cat W1^T + b1), h2 = relu(h1 W2^T + b2), y = (h2 W3^T + b3) + x_in
//   backward d2 = mask(dy W3, h2), d1 = mask(d2 W2, h1), dcat = d1 W1 -> dX = dcat[:, :64] + dy,
//            dD = dcat[:, 64:]
// The weight is the A operand and the points are the B operand, so a layer's result D[out][point]
// leaves lane (m, g) with outputs 16 t + 4 g + r of point m in acc[t][r] — and the next layer's B
// operand at step (q, i) is feature 16 q + 4 g + i of point m on the same lane: acc[t][r] of one
// layer IS xv[q = t][i = r] of the next. The activation stays in the wave's registers (no LDS
// transpose); it is stored once because the weight gradient reads it. All three weights sit in
// registers (128 + 64 + 64 per lane, one wave per SIMD); the slot holds the tile's input rows
// (forward: x_in | x_diffuse, also the residual; backward: dy | h2 | h1, also the masks and the
// residual's dy). Step order (q, i), k-slot assignment and every epilogue expression are those of
// linear_glds_rows_kernel, so each output is bit-identical to the three per-layer launches.
#include "mfma_tile.hpp"
#include "../../include/posekern.h"

using namespace pk;  // the tile helpers of mfma_tile.hpp

namespace {

constexpr int kMlpC = 64;  // C_width
constexpr int kFwdSlot = 2 * 16 * kMlpC;  // ring slot (floats) of the forward: x_in rows, then x_diffuse rows
constexpr int kBwdSlot = 3 * 16 * kMlpC;  // and of the backward: dy rows, h2 rows, h1 rows

template <bool SAVE>  // SAVE: h1 / h2 are written (the backward's operands)
__global__ __launch_bounds__(256, 1) void mlp3_fwd_chain_kernel(
    const float* __restrict__ xin, int64_t sxi, const float* __restrict__ xdf, int64_t sxd,
    const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
    const float* __restrict__ b2, const float* __restrict__ w3, const float* __restrict__ b3, int64_t R,
    float* __restrict__ h1, float* __restrict__ h2, float* __restrict__ y, int64_t sy) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int C = kMlpC, SLOT = kFwdSlot, G = 8, D = ring_depth(SLOT);
  const int lane = pk::lane_id(), wv = pk::wave_id(), m = lane & 15, g = lane >> 4;
  // weights -> VGPRs through the (not yet used) ring
  float* Ws1 = lds;
  float* Ws2 = Ws1 + C * (2 * C + 4);
  float* Ws3 = Ws2 + C * (C + 4);
  lr_stage<8, 4>(w1, C, 0, Ws1, w1, 1 << 30);
  lr_stage<4, 4>(w2, C, 0, Ws2, w2, 1 << 30);
  lr_stage<4, 4>(w3, C, 0, Ws3, w3, 1 << 30);
  __syncthreads();
  f32x4 W1[4][8], W2[4][4], W3[4][4];
  chain_wfrag<8, 4>(Ws1, m, g, W1);
  chain_wfrag<4, 4>(Ws2, m, g, W2);
  chain_wfrag<4, 4>(Ws3, m, g, W3);
  f32x4 bv1[4], bv2[4], bv3[4];  // biases of outputs 16 t + 4 g + r
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      bv1[t][r] = b1[16 * t + 4 * g + r];
      bv2[t][r] = b2[16 * t + 4 * g + r];
      bv3[t][r] = b3[16 * t + 4 * g + r];
    }
  __syncthreads();  // every wave holds its weights: the ring may now overwrite the stage
  float* ring = lds + (int64_t)wv * D * SLOT;
  const int64_t T = (R + 15) >> 4, stride = (int64_t)gridDim.x * 4;
  const int64_t t0 = (int64_t)blockIdx.x * 4 + wv;
  if (t0 >= T) return;
  const int64_t nt = (T - 1 - t0) / stride + 1;  // tiles of this wave
  int offi[4], offd[4];
  glds_rows_off<C>(sxi, C, lane, offi);
  glds_rows_off<C>(sxd, C, lane, offd);
  auto issue = [&](int64_t k) {  // glds of this wave's k-th tile (clamped: constant op count)
    const int64_t tile = t0 + min(k, nt - 1) * stride;
    float* s = ring + (k % D) * SLOT;
    const int64_t r0 = tile * 16;
    if (r0 + 16 <= R) {  // (wave-uniform) every row in range
      glds_issue<4, 16>(xin + r0 * sxi, offi, s);
      glds_issue<4, 16>(xdf + r0 * sxd, offd, s + 16 * C);
    } else {
      glds_rows<C>(xin, sxi, r0, R, C, s, lane);
      glds_rows<C>(xdf, sxd, r0, R, C, s + 16 * C, lane);
    }
  };
#pragma unroll
  for (int k = 0; k < D - 1; ++k) issue(k);
  for (int64_t k = 0; k < nt; ++k) {
    issue(k + D - 1);
    vm_wait<(D - 1) * G>();  // tile k landed (see linear_glds_rows_kernel)
    const float* s = ring + (k % D) * SLOT;
    const int64_t pr = (t0 + k * stride) * 16 + m;
    f32x4 acc[4], a[4];
    {  // layer 1: point m's features 16 q + 4 g .. + 3 of [x_in | x_diffuse]
      f32x4 xv[8];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        xv[q] = lds_chunk<C>(s, m, 4 * q + g);
        xv[4 + q] = lds_chunk<C>(s + 16 * C, m, 4 * q + g);
      }
      chain_mma<8, 4>(W1, xv, acc);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) a[t][r] = fmaxf(acc[t][r] + bv1[t][r], 0.f);
      if (SAVE && pr < R) *reinterpret_cast<f32x4*>(&h1[pr * C + 16 * t + 4 * g]) = a[t];
    }
    chain_mma<4, 4>(W2, a, acc);  // layer 2: h1 from the registers it was computed in
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) a[t][r] = fmaxf(acc[t][r] + bv2[t][r], 0.f);
      if (SAVE && pr < R) *reinterpret_cast<f32x4*>(&h2[pr * C + 16 * t + 4 * g]) = a[t];
    }
    chain_mma<4, 4>(W3, a, acc);  // layer 3 + the residual (x_in: the slot's first region)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const f32x4 ad = lds_chunk<C>(s, m, 4 * t + g);
      f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = (acc[t][r] + bv3[t][r]) + ad[r];
      if (pr < R) *reinterpret_cast<f32x4*>(&y[pr * sy + 16 * t + 4 * g]) = v;
    }
  }
  vm_wait<0>();
}

__global__ __launch_bounds__(256, 1) void mlp3_bwd_chain_kernel(
    const float* __restrict__ dy, const float* __restrict__ h2, const float* __restrict__ h1,
    const float* __restrict__ w3, const float* __restrict__ w2, const float* __restrict__ w1, int64_t R,
    float* __restrict__ d2, float* __restrict__ d1, float* __restrict__ dX, float* __restrict__ dD) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int C = kMlpC, SLOT = kBwdSlot, G = 12, D = ring_depth(SLOT);
  const int lane = pk::lane_id(), wv = pk::wave_id(), m = lane & 15, g = lane >> 4;
  // transposed weights (the dgrad's Ws[o = input channel][k = output channel]) -> VGPRs
  float* Ws3 = lds;
  float* Ws2 = Ws3 + C * (C + 4);
  float* Ws1 = Ws2 + C * (C + 4);
  lr_stage<4, 4>(w3, C, 1, Ws3, w3, 1 << 30);
  lr_stage<4, 4>(w2, C, 1, Ws2, w2, 1 << 30);
  lr_stage<4, 8>(w1, 2 * C, 1, Ws1, w1, 1 << 30);
  __syncthreads();
  f32x4 W3[4][4], W2[4][4], W1[8][4];
  chain_wfrag<4, 4>(Ws3, m, g, W3);
  chain_wfrag<4, 4>(Ws2, m, g, W2);
  chain_wfrag<4, 8>(Ws1, m, g, W1);
  __syncthreads();
  float* ring = lds + (int64_t)wv * D * SLOT;
  const int64_t T = (R + 15) >> 4, stride = (int64_t)gridDim.x * 4;
  const int64_t t0 = (int64_t)blockIdx.x * 4 + wv;
  if (t0 >= T) return;
  const int64_t nt = (T - 1 - t0) / stride + 1;
  int off[4];  // dy, h2, h1 are contiguous [R, 64]: one offset set
  glds_rows_off<C>(C, C, lane, off);
  auto issue = [&](int64_t k) {
    const int64_t tile = t0 + min(k, nt - 1) * stride;
    float* s = ring + (k % D) * SLOT;
    const int64_t r0 = tile * 16;
    if (r0 + 16 <= R) {
      glds_issue<4, 16>(dy + r0 * C, off, s);
      glds_issue<4, 16>(h2 + r0 * C, off, s + 16 * C);
      glds_issue<4, 16>(h1 + r0 * C, off, s + 32 * C);
    } else {
      glds_rows<C>(dy, C, r0, R, C, s, lane);
      glds_rows<C>(h2, C, r0, R, C, s + 16 * C, lane);
      glds_rows<C>(h1, C, r0, R, C, s + 32 * C, lane);
    }
  };
#pragma unroll
  for (int k = 0; k < D - 1; ++k) issue(k);
  for (int64_t k = 0; k < nt; ++k) {
    issue(k + D - 1);
    vm_wait<(D - 1) * G>();
    const float* s = ring + (k % D) * SLOT;
    const int64_t pr = (t0 + k * stride) * 16 + m;
    f32x4 acc[4], a[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = lds_chunk<C>(s, m, 4 * q + g);
    chain_mma<4, 4>(W3, a, acc);  // d2 = mask(dy W3, h2)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const f32x4 mk = lds_chunk<C>(s + 16 * C, m, 4 * t + g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float u = acc[t][r] + 0.f;  // (the per-layer call's null bias)
        a[t][r] = mk[r] <= 0.f ? 0.f : u;
      }
      if (pr < R) *reinterpret_cast<f32x4*>(&d2[pr * C + 16 * t + 4 * g]) = a[t];
    }
    chain_mma<4, 4>(W2, a, acc);  // d1 = mask(d2 W2, h1)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const f32x4 mk = lds_chunk<C>(s + 32 * C, m, 4 * t + g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float u = acc[t][r] + 0.f;
        a[t][r] = mk[r] <= 0.f ? 0.f : u;
      }
      if (pr < R) *reinterpret_cast<f32x4*>(&d1[pr * C + 16 * t + 4 * g]) = a[t];
    }
    f32x4 acc8[8];
    chain_mma<4, 8>(W1, a, acc8);  // dcat = d1 W1: columns < 64 (+ dy) -> dX, the rest -> dD
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      f32x4 ad = {0.f, 0.f, 0.f, 0.f};  // (past the residual's columns the per-layer epilogue adds 0)
      if (t < 4) ad = lds_chunk<C>(s, m, 4 * t + g);
      f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = (acc8[t][r] + 0.f) + ad[r];
      if (pr < R) {
        if (t < 4) *reinterpret_cast<f32x4*>(&dX[pr * C + 16 * t + 4 * g]) = v;
        else *reinterpret_cast<f32x4*>(&dD[pr * C + 16 * (t - 4) + 4 * g]) = v;
      }
    }
  }
  vm_wait<0>();
}

}  // namespace

// grid of the block-MLP chains: 4 tiles per block, at most max_blocks (0: the persistent grid)
static unsigned mlp3_blocks(int64_t R, int max_blocks) {
  const int64_t tiles = (R + 15) / 16;
  return (unsigned)std::min<int64_t>((tiles + 3) / 4, max_blocks > 0 ? max_blocks : kRowsPersistCUs);
}

extern "C" int pk_mlp3_fwd(const float* x_in, int64_t ld_in, const float* x_diff, int64_t ld_diff, const float* w1,
                           const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                           int64_t R, int C, float* h1, float* h2, float* y, int64_t ldy, int max_blocks,
                           void* stream) {
  PK_REQUIRE(R >= 0 && C == kMlpC && max_blocks >= 0);
  if (R == 0) return PK_OK;
  const int64_t sxi = ld_in ? ld_in : C, sxd = ld_diff ? ld_diff : C, sy = ldy ? ldy : C;
  PK_REQUIRE(x_in && x_diff && w1 && b1 && w2 && b2 && w3 && b3 && y && (h1 != nullptr) == (h2 != nullptr));
  PK_REQUIRE(sxi >= C && sxd >= C && sy >= C && sxi % 4 == 0 && sxd % 4 == 0 && sy % 4 == 0 && sxi <= (1 << 24) &&
             sxd <= (1 << 24));
  PK_REQUIRE(al16(x_in) && al16(x_diff) && al16(w1) && al16(w2) && al16(w3) && al16(y) && al16(h1) && al16(h2));
  const size_t lds = sizeof(float) * ring_depth(kFwdSlot) * 4 * kFwdSlot;  // the ring (the weight stage fits inside)
  const dim3 grid(mlp3_blocks(R, max_blocks));
  if (h1 != nullptr)
    hipLaunchKernelGGL(mlp3_fwd_chain_kernel<true>, grid, dim3(256), lds, pk::as_stream(stream), x_in, sxi, x_diff,
                       sxd, w1, b1, w2, b2, w3, b3, R, h1, h2, y, sy);
  else
    hipLaunchKernelGGL(mlp3_fwd_chain_kernel<false>, grid, dim3(256), lds, pk::as_stream(stream), x_in, sxi, x_diff,
                       sxd, w1, b1, w2, b2, w3, b3, R, h1, h2, y, sy);
  PK_CHECK_LAUNCH();
  return PK_OK;
}

extern "C" int pk_mlp3_bwd(const float* dy, const float* h2, const float* h1, const float* w3, const float* w2,
                           const float* w1, int64_t R, int C, float* d2, float* d1, float* dx, float* dd,
                           int max_blocks, void* stream) {
  PK_REQUIRE(R >= 0 && C == kMlpC && max_blocks >= 0);
  if (R == 0) return PK_OK;
  PK_REQUIRE(dy && h2 && h1 && w3 && w2 && w1 && d2 && d1 && dx && dd);
  PK_REQUIRE(al16(dy) && al16(h2) && al16(h1) && al16(d2) && al16(d1) && al16(dx) && al16(dd));
  const size_t lds = sizeof(float) * std::max(ring_depth(kBwdSlot) * 4 * kBwdSlot, 4 * kMlpC * (kMlpC + 4));
  hipLaunchKernelGGL(mlp3_bwd_chain_kernel, dim3(mlp3_blocks(R, max_blocks)), dim3(256), lds, pk::as_stream(stream),
                     dy, h2, h1, w3, w2, w1, R, d2, d1, dx, dd);
  PK_CHECK_LAUNCH();
  return PK_OK;
}
