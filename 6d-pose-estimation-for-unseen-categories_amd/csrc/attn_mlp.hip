// The MLP around the cross-attention of one AttentionalPropagation call (modeling/dpfm.py:45-82,
// C = 32 channels, channels-first [B, C, N] activations) in three or four launches instead of eight:
//     message = Wm a + bm;  hc = cat(x, message);  h1 = W0 hc + b0;  h1n = relu(instnorm(h1))
//   pk_attn_mlp_fwd       x, a -> hc, h1, h1n, mean, invstd  (the concatenation copy, the merge,
//                         mlp.0 and InstanceNorm + ReLU: one launch when hc / h1 are not stored,
//                         else a per-point chain launch and the norm launch on h1)
//   pk_attn_mlp_bwd_norm  dout -> dh1  (mlp.3^T and the InstanceNorm / ReLU backward; dh1n, the
//                         gradient in between, lives only in LDS)
//   pk_attn_mlp_bwd_in    dh1 -> dhc, da  (mlp.0^T, then merge^T on dhc[:, C:] from the registers
//                         it was computed in)
// InstanceNorm's statistics run over all N points of a (crop, channel) row, but mlp.0's output
// channels are independent of each other: a workgroup that owns (crop b, 16 of the 2C channels)
// computes those 16 complete rows into LDS (16 x N floats) and normalises them there. The backward
// mirrors it: mlp.3^T gives complete dh1n rows per (crop, 16 channels) for the norm backward.
//
// Every element is bit-identical to the per-layer launches (linear_cf_body in linear_fwd.hip and
// instnorm_relu_*_kernel in norm.hip): the products run on v_mfma_f32_16x16x4f32 with the weight
// as the A operand and the points as the B operand, contraction channel 16 q + 4 g + i on lane
// group g at step (q outer, i inner), the bias added after the accumulation (a null bias adds
// 0.f, as there); the norm reads its row in the lane + 64 k layout, sums k ascending per lane, then
// pk::wave_sum_f32, with the same two-pass variance and the same PER (8 / 16 / 32 values per lane
// for N <= 512 / 1024 / 2048).
//
// A layer's result D[out][point] leaves lane (m, g) with outputs 16 t + 4 g + r of point m in
// acc[t][r], and the next layer's B operand at step (q, i) is channel 16 q + 4 g + i of point m on
// the same lane: acc[t][r] of one layer IS the operand [q = t][i = r] of the next (no shuffle).
// Point tiles are 16 SUB consecutive points of one crop: lane (m, g) holds points SUB m + u as one
// vector per channel (SUB > 1 needs N % (16 SUB) == 0; with SUB = 1 a crop's last tile may be
// ragged: its columns past N compute on a clamped point and are not stored).
#include "common.hpp"
#include "mfma_tile.hpp"
#include "../../include/posekern.h"

namespace {

using pk::f32x2;
using pk::f32x4;
using pk::PtVec;  // SUB points of one channel per lane
using pk::al16;

constexpr int kC = 32;          // channels of the refinement (heads x 16)
constexpr int kMaxN = 2048;     // the norm's register tile (64 lanes x 32), 16 rows = 128 KB of LDS
constexpr int kRowWaves = 8;    // waves of a row-owning workgroup (2 of its 16 rows each in the norm)

template <int SUB>
__device__ __forceinline__ float vget(const typename PtVec<SUB>::T& v, int u) {
  if constexpr (SUB == 1) return v; else return v[u];
}
template <int SUB>
__device__ __forceinline__ void vset(typename PtVec<SUB>::T& v, int u, float z) {
  if constexpr (SUB == 1) v = z; else v[u] = z;
}

// LDS row stride of the 16 owned rows: 4 (mod 16), so the four row groups 4 g of one store land on
// different banks
__host__ __device__ constexpr int row_ld(int N) { return ((N + 15) & ~15) + 4; }

// Q x 4 channel rows (16 q + 4 g + i) of the tile's points, one vector per row
template <int SUB, int Q>
__device__ __forceinline__ void load_tile(const float* __restrict__ p, int N, int g, int off,
                                          typename PtVec<SUB>::T (&v)[Q][4]) {
  using V = typename PtVec<SUB>::T;
#pragma unroll
  for (int q = 0; q < Q; ++q)
#pragma unroll
    for (int i = 0; i < 4; ++i) v[q][i] = *reinterpret_cast<const V*>(p + (int64_t)(16 * q + 4 * g + i) * N + off);
}

// acc[t][u] += sum over (q, i) of A[t][q][i] x B[q][i][u], in linear_cf_body's order
template <int SUB, int Q, int TO>
__device__ __forceinline__ void tile_mma(const f32x4 (&wf)[TO][Q], const typename PtVec<SUB>::T (&xv)[Q][4],
                                         f32x4 (&acc)[TO][SUB]) {
#pragma unroll
  for (int t = 0; t < TO; ++t)
#pragma unroll
    for (int u = 0; u < SUB; ++u) acc[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < Q; ++q)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int u = 0; u < SUB; ++u)
#pragma unroll
        for (int t = 0; t < TO; ++t)
          acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[t][q][i], vget<SUB>(xv[q][i], u), acc[t][u], 0, 0, 0);
}

// One workgroup per (crop b, channel group cg: mlp.0 outputs 16 cg .. 16 cg + 15); its 8 waves walk
// the crop's point tiles (the next tile's loads in flight behind the current tile's MFMAs), then
// each normalises two of the 16 rows held in LDS. hc's 16 channels 16 cg .. are written by group cg
// (groups 0, 1: the copy of x; groups 2, 3: the message, which every group computes for its own
// mlp.0 operand). hc == nullptr / h1 == nullptr: not stored (no backward will read them).
template <int SUB, int PER>
__global__ __launch_bounds__(64 * kRowWaves) void attn_mlp_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ a, const float* __restrict__ wm,
    const float* __restrict__ bm, const float* __restrict__ w0, const float* __restrict__ b0, int N, float eps,
    float* __restrict__ hc, float* __restrict__ h1, float* __restrict__ h1n, float* __restrict__ mean_out,
    float* __restrict__ invstd_out) {
  using V = typename PtVec<SUB>::T;
  extern __shared__ __attribute__((aligned(16))) float rows[];  // [16][row_ld(N)]
  constexpr int C = kC, P = 16 * SUB;
  const int b = blockIdx.x >> 2, cg = blockIdx.x & 3;
  const int lane = pk::lane_id(), wv = pk::wave_id(), m = lane & 15, g = lane >> 4;
  const int LD = row_ld(N);
  const int tpc = (N + P - 1) / P;
  const float* __restrict__ xb = x + (int64_t)b * C * N;
  const float* __restrict__ ab = a + (int64_t)b * C * N;
  V cx[2][4], ca[2][4], nx[2][4], na[2][4];
  auto tile_off = [&](int tile) { return tile * P + ((SUB > 1 || tile * P + m < N) ? SUB * m : 0); };
  int tile = wv;
  if (tile < tpc) {  // the first tile's operands are in flight while the weights are fetched
    load_tile<SUB, 2>(xb, N, g, tile_off(tile), cx);
    load_tile<SUB, 2>(ab, N, g, tile_off(tile), ca);
  }
  // weight fragments (A operands) straight from memory: lane (m, g) holds W[16 t + m][16 q + 4 g ..]
  f32x4 wmf[2][2], w0f[1][4];
  f32x4 bmv[2], b0v;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int q = 0; q < 2; ++q) wmf[t][q] = *reinterpret_cast<const f32x4*>(wm + (16 * t + m) * C + 16 * q + 4 * g);
    bmv[t] = *reinterpret_cast<const f32x4*>(bm + 16 * t + 4 * g);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
    w0f[0][q] = *reinterpret_cast<const f32x4*>(w0 + (16 * cg + m) * 2 * C + 16 * q + 4 * g);
  b0v = *reinterpret_cast<const f32x4*>(b0 + 16 * cg + 4 * g);
  for (; tile < tpc; tile += kRowWaves) {
    const int tn = tile + kRowWaves;
    if (tn < tpc) {
      load_tile<SUB, 2>(xb, N, g, tile_off(tn), nx);
      load_tile<SUB, 2>(ab, N, g, tile_off(tn), na);
    }
    const bool live = SUB > 1 || tile * P + m < N;
    const int off = tile_off(tile);
    // the merge: message channels 16 t + 4 g + r of the lane's points
    f32x4 am[2][SUB];
    tile_mma<SUB, 2, 2>(wmf, ca, am);
    V hv[4][4];  // cat(x, message): mlp.0's B operand
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        hv[q][i] = cx[q][i];
#pragma unroll
        for (int u = 0; u < SUB; ++u) vset<SUB>(hv[2 + q][i], u, am[q][u][i] + bmv[q][i]);
      }
    f32x4 acc[1][SUB];
    tile_mma<SUB, 4, 1>(w0f, hv, acc);
    if (live) {
      if (hc != nullptr) {
        float* __restrict__ hb = hc + ((int64_t)b * 2 * C + 16 * cg + 4 * g) * N + off;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (q == cg) {
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<V*>(hb + (int64_t)i * N) = hv[q][i];
          }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        V v;
#pragma unroll
        for (int u = 0; u < SUB; ++u) vset<SUB>(v, u, acc[0][u][r] + b0v[r]);
        *reinterpret_cast<V*>(&rows[(4 * g + r) * LD + off]) = v;
        if (h1 != nullptr) *reinterpret_cast<V*>(h1 + ((int64_t)b * 2 * C + 16 * cg + 4 * g + r) * N + off) = v;
      }
    }
    if (tn < tpc) {
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          cx[q][i] = nx[q][i];
          ca[q][i] = na[q][i];
        }
    }
  }
  __syncthreads();
  // InstanceNorm + ReLU on the rows in LDS: instnorm_relu_fwd_kernel<PER>'s arithmetic
#pragma unroll
  for (int j = 0; j < 16 / kRowWaves; ++j) {
    const int row = wv + kRowWaves * j;
    const float* xr = rows + row * LD;
    float v[PER];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int n = lane + 64 * k;
      v[k] = n < N ? xr[n] : 0.f;
      s += v[k];
    }
    const float mean = pk::wave_sum_f32(s) / (float)N;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int n = lane + 64 * k;
      const float d = v[k] - mean;
      q += n < N ? d * d : 0.f;
    }
    const float var = pk::wave_sum_f32(q) / (float)N;
    const float invstd = 1.f / sqrtf(var + eps);
    const int64_t r = (int64_t)b * 2 * C + 16 * cg + row;
    float* __restrict__ yr = h1n + r * N;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int n = lane + 64 * k;
      if (n < N) yr[n] = fmaxf((v[k] - mean) * invstd, 0.f);
    }
    if (lane == 0) {
      mean_out[r] = mean;
      invstd_out[r] = invstd;
    }
  }
}

// The forward without the norm, per point (one wave per point tile, 4 per workgroup, every CU busy
// and the merge computed once): hc = cat(x, Wm a + bm) and h1 = W0 hc + b0. The training forward
// runs this and then instnorm_relu_fwd_kernel on h1, which it has to store anyway: on the device
// that pair is faster than the row-owning kernel above, whose 4 workgroups per crop each repeat the
// merge (half of its MFMA time) on half of the CUs. Weight fragments come straight from memory.
template <int SUB>
__global__ __launch_bounds__(256) void attn_mlp_fwd_chain_kernel(
    const float* __restrict__ x, const float* __restrict__ a, const float* __restrict__ wm,
    const float* __restrict__ bm, const float* __restrict__ w0, const float* __restrict__ b0, int N, int tpc, int T,
    float* __restrict__ hc, float* __restrict__ h1) {
  using V = typename PtVec<SUB>::T;
  constexpr int C = kC, P = 16 * SUB;
  const int lane = pk::lane_id(), m = lane & 15, g = lane >> 4;
  const int tile = blockIdx.x * 4 + pk::wave_id();
  if (tile >= T) return;
  const int b = tile / tpc, n0 = (tile - b * tpc) * P;
  const bool live = SUB > 1 || n0 + m < N;
  const int off = n0 + (live ? SUB * m : 0);
  V cx[2][4], ca[2][4];
  load_tile<SUB, 2>(x + (int64_t)b * C * N, N, g, off, cx);
  load_tile<SUB, 2>(a + (int64_t)b * C * N, N, g, off, ca);
  f32x4 wmf[2][2], w0f[4][4], bmv[2], b0v[4];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int q = 0; q < 2; ++q) wmf[t][q] = *reinterpret_cast<const f32x4*>(wm + (16 * t + m) * C + 16 * q + 4 * g);
    bmv[t] = *reinterpret_cast<const f32x4*>(bm + 16 * t + 4 * g);
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      w0f[t][q] = *reinterpret_cast<const f32x4*>(w0 + (16 * t + m) * 2 * C + 16 * q + 4 * g);
    b0v[t] = *reinterpret_cast<const f32x4*>(b0 + 16 * t + 4 * g);
  }
  f32x4 am[2][SUB];
  tile_mma<SUB, 2, 2>(wmf, ca, am);
  V hv[4][4];  // cat(x, message): stored as hc and mlp.0's B operand
  float* __restrict__ hb = hc + ((int64_t)b * 2 * C + 4 * g) * N + off;
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      hv[q][i] = cx[q][i];
#pragma unroll
      for (int u = 0; u < SUB; ++u) vset<SUB>(hv[2 + q][i], u, am[q][u][i] + bmv[q][i]);
    }
  if (live) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) *reinterpret_cast<V*>(hb + (int64_t)(16 * q + i) * N) = hv[q][i];
  }
  f32x4 acc[4][SUB];
  tile_mma<SUB, 4, 4>(w0f, hv, acc);
  float* __restrict__ ob = h1 + ((int64_t)b * 2 * C + 4 * g) * N + off;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      V v;
#pragma unroll
      for (int u = 0; u < SUB; ++u) vset<SUB>(v, u, acc[t][u][r] + b0v[t][r]);
      if (live) *reinterpret_cast<V*>(ob + (int64_t)(16 * t + r) * N) = v;
    }
}

// Same ownership: (crop b, dh1n channels 16 cg .. 16 cg + 15). dh1n = W3^T dout goes into LDS row
// by row tile; each wave then runs instnorm_relu_bwd_kernel<PER>'s arithmetic on two rows, with the
// rows' h1 values (loaded before the tile loop: they do not depend on it) and writes dh1.
template <int SUB, int PER>
__global__ __launch_bounds__(64 * kRowWaves) void attn_mlp_bwd_norm_kernel(
    const float* __restrict__ dout, const float* __restrict__ w3, const float* __restrict__ h1,
    const float* __restrict__ mean_in, const float* __restrict__ invstd_in, int N, float* __restrict__ dh1) {
  using V = typename PtVec<SUB>::T;
  extern __shared__ __attribute__((aligned(16))) float rows[];  // [16][row_ld(N)]
  constexpr int C = kC, P = 16 * SUB, RJ = 16 / kRowWaves;
  const int b = blockIdx.x >> 2, cg = blockIdx.x & 3;
  const int lane = pk::lane_id(), wv = pk::wave_id(), m = lane & 15, g = lane >> 4;
  const int LD = row_ld(N);
  const int tpc = (N + P - 1) / P;
  const float* __restrict__ db = dout + (int64_t)b * C * N;
  V cd[2][4], nd[2][4];
  auto tile_off = [&](int tile) { return tile * P + ((SUB > 1 || tile * P + m < N) ? SUB * m : 0); };
  int tile = wv;
  if (tile < tpc) load_tile<SUB, 2>(db, N, g, tile_off(tile), cd);
  // W3 [C, 2 C] read transposed: A[o = 16 cg + m][k = 16 q + 4 g + i] = W3[k][o]
  f32x4 w3f[1][2];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int i = 0; i < 4; ++i) w3f[0][q][i] = w3[(16 * q + 4 * g + i) * 2 * C + 16 * cg + m];
  float xv[RJ][PER];
#pragma unroll
  for (int j = 0; j < RJ; ++j) {
    const float* __restrict__ xr = h1 + ((int64_t)b * 2 * C + 16 * cg + wv + kRowWaves * j) * N;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int n = lane + 64 * k;
      xv[j][k] = n < N ? xr[n] : 0.f;
    }
  }
  for (; tile < tpc; tile += kRowWaves) {
    const int tn = tile + kRowWaves;
    if (tn < tpc) load_tile<SUB, 2>(db, N, g, tile_off(tn), nd);
    const bool live = SUB > 1 || tile * P + m < N;
    const int off = tile_off(tile);
    f32x4 acc[1][SUB];
    tile_mma<SUB, 2, 1>(w3f, cd, acc);
    if (live) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        V v;
#pragma unroll
        for (int u = 0; u < SUB; ++u) vset<SUB>(v, u, acc[0][u][r] + 0.f);  // (the per-layer call's null bias)
        *reinterpret_cast<V*>(&rows[(4 * g + r) * LD + off]) = v;
      }
    }
    if (tn < tpc) {
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i) cd[q][i] = nd[q][i];
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < RJ; ++j) {
    const int row = wv + kRowWaves * j;
    const int64_t r = (int64_t)b * 2 * C + 16 * cg + row;
    const float mean = mean_in[r], invstd = invstd_in[r];
    const float* gr = rows + row * LD;
    float xh[PER], gk[PER];
    float sg = 0.f, sgx = 0.f;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int n = lane + 64 * k;
      const float gv = n < N ? gr[n] : 0.f;
      xh[k] = (xv[j][k] - mean) * invstd;
      gk[k] = xh[k] > 0.f ? gv : 0.f;
      sg += gk[k];
      sgx += gk[k] * xh[k];
    }
    const float mg = pk::wave_sum_f32(sg) / (float)N;
    const float mgx = pk::wave_sum_f32(sgx) / (float)N;
    float* __restrict__ dr = dh1 + r * N;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int n = lane + 64 * k;
      if (n < N) dr[n] = invstd * ((gk[k] - mg) - xh[k] * mgx);
    }
  }
}

// Per-point chain, tiled like linear_cf_body (one wave per point tile, 4 per workgroup, the
// transposed weights staged in LDS as Ws[o][k], row stride K + 4): dhc = W0^T dh1 (all 2 C rows
// stored), then da = Wm^T dhc[:, C:] from the accumulators.
template <int SUB>
__global__ __launch_bounds__(256) void attn_mlp_bwd_in_kernel(const float* __restrict__ dh1,
                                                              const float* __restrict__ w0,
                                                              const float* __restrict__ wm, int N, int tpc,
                                                              int T, float* __restrict__ dhc,
                                                              float* __restrict__ da) {
  using V = typename PtVec<SUB>::T;
  constexpr int C = kC, P = 16 * SUB, ST0 = 2 * C + 4, STM = C + 4;
  __shared__ __attribute__((aligned(16))) float Ws0[2 * C * ST0];
  __shared__ __attribute__((aligned(16))) float Wsm[C * STM];
  const int lane = pk::lane_id(), m = lane & 15, g = lane >> 4;
  const int tile = blockIdx.x * 4 + pk::wave_id();
  V xv[4][4];
  int b = 0, off = 0;
  bool live = true;
  if (tile < T) {  // the tile's operands are in flight while the weights are staged
    b = tile / tpc;
    const int n0 = (tile - b * tpc) * P;
    if (SUB == 1) live = n0 + m < N;
    off = n0 + (live ? SUB * m : 0);
    load_tile<SUB, 4>(dh1 + (int64_t)b * 2 * C * N, N, g, off, xv);
  }
  {  // Ws0[o][k] = W0[k][o], Wsm[o][k] = Wm[k][o]: reads along o, all issued before the LDS writes
    float v0[16], vm[4];
#pragma unroll
    for (int i = 0; i < 16; ++i) v0[i] = w0[threadIdx.x + 256 * i];
#pragma unroll
    for (int i = 0; i < 4; ++i) vm[i] = wm[threadIdx.x + 256 * i];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int e = threadIdx.x + 256 * i, k = e / (2 * C), o = e - k * 2 * C;
      Ws0[o * ST0 + k] = v0[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = threadIdx.x + 256 * i, k = e / C, o = e - k * C;
      Wsm[o * STM + k] = vm[i];
    }
  }
  __syncthreads();
  if (tile >= T) return;
  f32x4 acc[4][SUB];
  {
    f32x4 wf[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) wf[t][q] = *reinterpret_cast<const f32x4*>(&Ws0[(16 * t + m) * ST0 + 16 * q + 4 * g]);
    tile_mma<SUB, 4, 4>(wf, xv, acc);
  }
  V dv[2][4];  // dhc[:, C:] of the lane's points: merge^T's B operand
  float* __restrict__ hb = dhc + (int64_t)b * 2 * C * N + off;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      V v;
#pragma unroll
      for (int u = 0; u < SUB; ++u) vset<SUB>(v, u, acc[t][u][r] + 0.f);  // (the per-layer call's null bias)
      if (t >= 2) dv[t - 2][r] = v;
      if (live) *reinterpret_cast<V*>(hb + (int64_t)(16 * t + 4 * g + r) * N) = v;
    }
  f32x4 acc2[2][SUB];
  {
    f32x4 wf[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int q = 0; q < 2; ++q) wf[t][q] = *reinterpret_cast<const f32x4*>(&Wsm[(16 * t + m) * STM + 16 * q + 4 * g]);
    tile_mma<SUB, 2, 2>(wf, dv, acc2);
  }
  float* __restrict__ ob = da + (int64_t)b * C * N + off;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      V v;
#pragma unroll
      for (int u = 0; u < SUB; ++u) vset<SUB>(v, u, acc2[t][u][r] + 0.f);
      if (live) *reinterpret_cast<V*>(ob + (int64_t)(16 * t + 4 * g + r) * N) = v;
    }
}

}  // namespace

extern "C" int pk_attn_mlp_fwd(const float* x, const float* a, const float* wm, const float* bm, const float* w0,
                               const float* b0, int B, int C, int N, float eps, float* hc, float* h1, float* h1n,
                               float* mean, float* invstd, void* stream) {
  PK_REQUIRE(B >= 0 && C == kC && N > 0 && N <= kMaxN && (int64_t)B * ((N + 15) / 16) < (1ll << 31));
  if (B == 0) return PK_OK;
  PK_REQUIRE(x && a && wm && bm && w0 && b0 && h1n && mean && invstd);
  PK_REQUIRE(al16(wm) && al16(bm) && al16(w0) && al16(b0));
  // 32-point tiles (8-B vectors): with the next tile prefetched, 64-point tiles spill
  const bool v2 = N % 32 == 0 && al16(x) && al16(a) && al16(hc) && al16(h1);
  hipStream_t s = pk::as_stream(stream);
  if (hc != nullptr && h1 != nullptr) {  // the training forward: the per-point chain, then the norm on h1
    const int P = v2 ? 32 : 16;
    const int tpc = (N + P - 1) / P, T = B * tpc;
    const dim3 cgrid((unsigned)((T + 3) / 4));
    if (v2)
      hipLaunchKernelGGL(attn_mlp_fwd_chain_kernel<2>, cgrid, dim3(256), 0, s, x, a, wm, bm, w0, b0, N, tpc, T, hc, h1);
    else
      hipLaunchKernelGGL(attn_mlp_fwd_chain_kernel<1>, cgrid, dim3(256), 0, s, x, a, wm, bm, w0, b0, N, tpc, T, hc, h1);
    PK_CHECK_LAUNCH();
    return pk_instnorm_relu_fwd(h1, (int64_t)B * 2 * C, N, eps, h1n, mean, invstd, stream);
  }
  const dim3 grid((unsigned)B * 4), block(64 * kRowWaves);
  const size_t lds = sizeof(float) * 16 * row_ld(N);
#define PK_AM_FWD(SUB, PER)                                                                                      \
  hipLaunchKernelGGL((attn_mlp_fwd_kernel<SUB, PER>), grid, block, lds, s, x, a, wm, bm, w0, b0, N, eps, hc, h1, \
                     h1n, mean, invstd)
  if (v2) {
    if (N <= 512) PK_AM_FWD(2, 8); else if (N <= 1024) PK_AM_FWD(2, 16); else PK_AM_FWD(2, 32);
  } else {
    if (N <= 512) PK_AM_FWD(1, 8); else if (N <= 1024) PK_AM_FWD(1, 16); else PK_AM_FWD(1, 32);
  }
#undef PK_AM_FWD
  PK_CHECK_LAUNCH();
  return PK_OK;
}

extern "C" int pk_attn_mlp_bwd_norm(const float* dout, const float* w3, const float* h1, const float* mean,
                                    const float* invstd, int B, int C, int N, float* dh1, void* stream) {
  PK_REQUIRE(B >= 0 && C == kC && N > 0 && N <= kMaxN);
  if (B == 0) return PK_OK;
  PK_REQUIRE(dout && w3 && h1 && mean && invstd && dh1);
  const bool v4 = N % 64 == 0 && al16(dout);
  const dim3 grid((unsigned)B * 4), block(64 * kRowWaves);
  const size_t lds = sizeof(float) * 16 * row_ld(N);
  hipStream_t s = pk::as_stream(stream);
#define PK_AM_BWN(SUB, PER)                                                                                       \
  hipLaunchKernelGGL((attn_mlp_bwd_norm_kernel<SUB, PER>), grid, block, lds, s, dout, w3, h1, mean, invstd, N, dh1)
  if (v4) {
    if (N <= 512) PK_AM_BWN(4, 8); else if (N <= 1024) PK_AM_BWN(4, 16); else PK_AM_BWN(4, 32);
  } else {
    if (N <= 512) PK_AM_BWN(1, 8); else if (N <= 1024) PK_AM_BWN(1, 16); else PK_AM_BWN(1, 32);
  }
#undef PK_AM_BWN
  PK_CHECK_LAUNCH();
  return PK_OK;
}

extern "C" int pk_attn_mlp_bwd_in(const float* dh1, const float* w0, const float* wm, int B, int C, int N, float* dhc,
                                  float* da, void* stream) {
  PK_REQUIRE(B >= 0 && C == kC && N > 0 && (int64_t)B * ((N + 15) / 16) < (1ll << 31));
  if (B == 0) return PK_OK;
  PK_REQUIRE(dh1 && w0 && wm && dhc && da);
  // 32-point tiles (8-B vectors) where the rows allow: twice the waves of 64-point tiles at the
  // refinement's 32 x 1024 points, one per SIMD of the device
  const bool v2 = N % 32 == 0 && al16(dh1) && al16(dhc) && al16(da);
  const int P = v2 ? 32 : 16;
  const int tpc = (N + P - 1) / P, T = B * tpc;
  const dim3 grid((unsigned)((T + 3) / 4));
  hipStream_t s = pk::as_stream(stream);
  if (v2) hipLaunchKernelGGL(attn_mlp_bwd_in_kernel<2>, grid, dim3(256), 0, s, dh1, w0, wm, N, tpc, T, dhc, da);
  else hipLaunchKernelGGL(attn_mlp_bwd_in_kernel<1>, grid, dim3(256), 0, s, dh1, w0, wm, N, tpc, T, dhc, da);
  PK_CHECK_LAUNCH();
  return PK_OK;
}
