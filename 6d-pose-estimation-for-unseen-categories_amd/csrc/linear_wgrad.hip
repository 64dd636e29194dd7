// Weight / bias gradients of the per-point layers of H7 / H8 (DiffusionNet MiniMLP and
// first/last_lin, models/dpfm.py:22-30; refinement Conv1d(k=1) projections and MLPs,
// modeling/dpfm.py:16-26, 45-54, 63, 82-95, 120-130):
//     dW[o, i] = sum_r dY[r, o] X[r, i],   db[o] = sum_r dY[r, o]
// over every point of every crop (r = B * N rows, 32768-65536 per call) into a tiny
// [O <= 128, I <= 128] result. A library GEMM tiles the output (a handful of tiles) and
// walks all rows serially; here the rows are split into slices of at least 128 rows, one
// workgroup per slice, each contracting its slice on the f32 MFMA (exact f32 products, f32
// accumulation) into a partial [O, I]; a second pass sums the partials in slice order
// (deterministic).
//
// Layouts: 0 = rows x channels ([R, C] row-major, nn.Linear), 1 = channels-first
// ([Bn, C, N], Conv1d with kernel 1; row r = (r / N, r % N)).
#include "mfma_tile.hpp"
#include "../../include/posekern.h"

#include <vector>

using namespace pk;  // the tile helpers of mfma_tile.hpp

namespace {

constexpr int kSlice = 128;         // least rows per workgroup
constexpr int kMaxC = 128;          // I, O <= 128
constexpr int kMaxTilesPerWave = 8;  // O * I <= 128 * 64

// dw[e] = sum_s part[s, e] (e < O*I), db[o] = sum_s partb[s, o]. Block = 64 outputs x
// 16 slice groups (two interleaved chains each), combined by a fixed pairwise tree:
// deterministic, and 16 loads in flight per output instead of a serial walk over S.
constexpr int kRedGroups = 16;
__global__ __launch_bounds__(64 * kRedGroups) void wgrad_reduce_kernel(const float* __restrict__ part,
                                                                       const float* __restrict__ partb, int S,
                                                                       int OI, int O, float* __restrict__ dw,
                                                                       float* __restrict__ db, int accumulate) {
  __shared__ float red[kRedGroups][64];
  const int e = blockIdx.x * 64 + (threadIdx.x & 63);
  const int grp = threadIdx.x >> 6;
  const bool is_w = e < OI;
  const bool is_b = !is_w && e < OI + O && db != nullptr;
  float v = 0.f;
  if (is_w || is_b) {
    const float* p = is_w ? part + e : partb + (e - OI);
    const int64_t st = is_w ? OI : O;
    const int s0 = (S * grp) / kRedGroups, s1 = (S * (grp + 1)) / kRedGroups;
    float a0 = 0.f, a1 = 0.f;
    int s = s0;
    for (; s + 2 <= s1; s += 2) {
      a0 += p[(int64_t)s * st];
      a1 += p[(int64_t)(s + 1) * st];
    }
    if (s < s1) a0 += p[(int64_t)s * st];
    v = a0 + a1;
  }
  red[grp][threadIdx.x & 63] = v;
  __syncthreads();
#pragma unroll
  for (int half = kRedGroups / 2; half >= 1; half >>= 1) {
    if (grp < half) red[grp][threadIdx.x & 63] += red[grp + half][threadIdx.x & 63];
    __syncthreads();
  }
  if (grp == 0 && (is_w || is_b)) {
    const float r = red[0][threadIdx.x & 63];
    float* dst = is_w ? dw + e : db + (e - OI);
    *dst = accumulate ? *dst + r : r;  // += : a weight used by several layers' calls
  }
}

// ---------------------------------------------------------------------------------
// Direct-load variant (the default): v_mfma_f32_32x32x2_f32 takes its operands straight
// from global memory, no LDS staging and no barriers in the row loop.
//   A[m][k] = dY[row k][o0 + m], B[k][n] = X[row k][i0 + n]  ->  D = dW tile [32 x 32]
// Lane l supplies A[l & 31][l >> 5] and B[l >> 5][l & 31], i.e. one value of row
// r(step, h = l >> 5) at channel (l & 31). Rows are taken in batches of 16 (8 k-steps):
//   layout 0 ([R, C]): r = rb + 2 s + h       (32 lanes read 128 contiguous bytes)
//   layout 1 ([Bn, C, N]): r = rb + 8 h + s  (a lane's 8 rows are 8 consecutive n of one
//            channel: two 16-byte loads when N % 16 == 0, else 8 scalar loads with the tail
//            rows past the slice end read as 0)
// Both operands use the same r(s, h), so the contraction is the same sum over rows.
// Workgroup = one row slice; its 4 waves split the 32x32 output tiles (T = To * Ti <= 16)
// and, when there are fewer than 4 tiles, the slice's batches; wave row groups are
// combined through LDS in a fixed order (deterministic). Bias = row sums of the A values
// of the tiles with ti == 0.

template <int LAYOUT>
__device__ __forceinline__ void load8(const float* __restrict__ p, int C, int c, int N, int64_t rb, int64_t r1,
                                      int h, float (&v)[8], int64_t sb) {
  if (LAYOUT == 0) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int64_t r = rb + 2 * s + h;
      v[s] = (c < C && r < r1) ? p[r * C + c] : 0.f;
    }
  } else if (N & 15) {  // ragged items (N % 16 != 0): a 16-row batch may straddle two items
    const int64_t cs = sb ? sb : (int64_t)C * N;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int64_t r = rb + 8 * h + s;
      const int64_t b = r / N;
      v[s] = (c < C && r < r1) ? p[b * cs + (int64_t)c * N + (r - b * N)] : 0.f;
    }
  } else {
    if (c < C) {  // batch stride sb (0: dense C N)
      const int64_t b = rb / N;
      const int64_t n = rb - b * N + 8 * h;
      const float4* q = reinterpret_cast<const float4*>(p + b * (sb ? sb : (int64_t)C * N) + (int64_t)c * N + n);
      const float4 u = q[0], w = q[1];
      v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
      v[4] = w.x; v[5] = w.y; v[6] = w.z; v[7] = w.w;
    } else {
#pragma unroll
      for (int s = 0; s < 8; ++s) v[s] = 0.f;
    }
  }
}

// Operands of one 16-row batch for a wave's J tiles.
template <int J>
struct WgradBatch {
  float a[J][8], b[J][8];
};

template <int LAYOUT, int J>
__device__ __forceinline__ void wgrad_load(WgradBatch<J>& B, const float* __restrict__ x, const float* __restrict__ dy,
                                           int I, int O, int N, int Ti, int T, int tw, int WT, int m, int h,
                                           int64_t rb, int64_t r1, int64_t sbx, int64_t sbdy) {
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int t = tw + WT * j;
    if (t < T) {
      const int to = t / Ti, ti = t - to * Ti;
      load8<LAYOUT>(dy, O, to * 32 + m, N, rb, r1, h, B.a[j], sbdy);
      load8<LAYOUT>(x, I, ti * 32 + m, N, rb, r1, h, B.b[j], sbx);
    }
  }
}

template <int J>
__device__ __forceinline__ void wgrad_mma(const WgradBatch<J>& B, f32x16 (&acc)[J], float (&bs)[J], int Ti, int T,
                                          int tw, int WT) {
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int t = tw + WT * j;
    if (t < T) {
#pragma unroll
      for (int st = 0; st < 8; ++st) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(B.a[j][st], B.b[j][st], acc[j], 0, 0, 0);
      if (t % Ti == 0) {
#pragma unroll
        for (int st = 0; st < 8; ++st) bs[j] += B.a[j][st];
      }
    }
  }
}

// 8 waves per workgroup: WT = min(T, 8) tile lanes x WR = 8 / WT row groups; J tiles per
// wave (J = 2 only for T = 16). The next batch's loads are issued before the current
// batch's MFMAs (two register buffers, statically indexed).
constexpr int kV2Waves = 8;

// Slice s of one problem; comb / combb: the workgroup's [kV2Waves][16 * 64] / [kV2Waves][64]
// LDS (declared by the calling kernel, so a kernel instantiating both layouts allocates it once).
template <int LAYOUT, int J>
__device__ __forceinline__ void wgrad_v2_body(const float* __restrict__ x, const float* __restrict__ dy, int64_t R,
                                              int I, int O, int N, int SL, float* __restrict__ part,
                                              float* __restrict__ partb, int s, float (*comb)[16 * 64],
                                              float (*combb)[64], int64_t sbx, int64_t sbdy) {
  const int lane = pk::lane_id(), w = pk::wave_id();
  const int m = lane & 31, h = lane >> 5;
  const int To = (O + 31) >> 5, Ti = (I + 31) >> 5, T = To * Ti;
  const int WT = T < kV2Waves ? T : kV2Waves;
  const int WR = kV2Waves / WT;
  const int tw = w % WT, g = w / WT;
  const bool active = g < WR;
  f32x16 acc[J];
  float bs[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    bs[j] = 0.f;
  }
  const int64_t r0 = (int64_t)s * SL;
  const int64_t r1 = r0 + SL < R ? r0 + SL : R;
  const int nb = (int)((r1 - r0 + 15) / 16);
  if (active) {
    WgradBatch<J> b0, b1;
    int q = g;
    if (q < nb) wgrad_load<LAYOUT, J>(b0, x, dy, I, O, N, Ti, T, tw, WT, m, h, r0 + 16ll * q, r1, sbx, sbdy);
    for (; q < nb; q += 2 * WR) {
      const bool has1 = q + WR < nb;
      if (has1) wgrad_load<LAYOUT, J>(b1, x, dy, I, O, N, Ti, T, tw, WT, m, h, r0 + 16ll * (q + WR), r1, sbx, sbdy);
      wgrad_mma<J>(b0, acc, bs, Ti, T, tw, WT);
      if (has1) {
        if (q + 2 * WR < nb)
          wgrad_load<LAYOUT, J>(b0, x, dy, I, O, N, Ti, T, tw, WT, m, h, r0 + 16ll * (q + 2 * WR), r1, sbx, sbdy);
        wgrad_mma<J>(b1, acc, bs, Ti, T, tw, WT);
      }
    }
  }
  // combine row groups (only when WT < 8, i.e. one tile per wave) in group order
  if (WR > 1) {
    if (active) {
#pragma unroll
      for (int e = 0; e < 16; ++e) comb[w][e * 64 + lane] = acc[0][e];
      combb[w][lane] = bs[0];
    }
    __syncthreads();
    if (!active || g != 0) return;
    for (int gg = 1; gg < WR; ++gg) {
      const int src = tw + WT * gg;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[0][e] += comb[src][e * 64 + lane];
      bs[0] += combb[src][lane];
    }
  }
  if (!active) return;
  float* __restrict__ ps = part + (int64_t)s * O * I;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int t = tw + WT * j;
    if (t < T) {
      const int to = t / Ti, ti = t - to * Ti;
      const int i = ti * 32 + m;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int o = to * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (o < O && i < I) ps[(int64_t)o * I + i] = acc[j][e];
      }
      if (ti == 0) {
        const float tot = bs[j] + __shfl_xor(bs[j], 32);  // the two row halves
        const int o = to * 32 + m;
        if (h == 0 && o < O) partb[(int64_t)s * O + o] = tot;
      }
    }
  }
}

template <int LAYOUT, int J>
__global__ __launch_bounds__(64 * kV2Waves) void wgrad_v2_kernel(const float* __restrict__ x,
                                                                 const float* __restrict__ dy, int64_t R, int I,
                                                                 int O, int N, int SL, float* __restrict__ part,
                                                                 float* __restrict__ partb) {
  __shared__ float comb[kV2Waves][16 * 64];
  __shared__ float combb[kV2Waves][64];
  wgrad_v2_body<LAYOUT, J>(x, dy, R, I, O, N, SL, part, partb, blockIdx.x, comb, combb, 0, 0);
}

// ---------------------------------------------------------------------------------
// Grouped weight gradients: every per-point layer of a backward pass in two launches
// (partials, then reduction) instead of two launches per layer. The problem tables travel
// as kernel arguments (captured into a HIP graph node by value). Block b belongs to the
// problem whose [blk0, blk0 + S) holds b; each problem runs the same slice body as
// pk_linear_wgrad. An output fed by two calls of one forward (a shared layer) reduces both
// partial sets, first call first: r = reduce(seg 0) + reduce(seg 1), the same rounding as
// autograd's grad = grad_0 + grad_1.
constexpr int kGroupMax = 32;

struct WgradProblem {
  const float* x;
  const float* dy;
  float* part;   // S * O * I weight partials, then S * O bias partials
  int64_t R;
  int I, O, N, layout, SL, S, blk0, pad;  // pad: unused (0); keeps the 8-byte members aligned
  int64_t sbx, sbdy;  // channels-first batch strides (0: dense)
};
struct WgradProblems {
  int G;
  WgradProblem p[kGroupMax];
};

__global__ __launch_bounds__(64 * kV2Waves) void wgrad_grouped_kernel(const WgradProblems tab) {
  __shared__ float comb[kV2Waves][16 * 64];
  __shared__ float combb[kV2Waves][64];
  const int b = blockIdx.x;
  int g = 0;
  while (g + 1 < tab.G && b >= tab.p[g + 1].blk0) ++g;  // block-uniform scan (G <= 32)
  const WgradProblem& P = tab.p[g];
  const int s = b - P.blk0;
  float* partb = P.part + (int64_t)P.S * P.O * P.I;
  if (P.layout == 0) wgrad_v2_body<0, 1>(P.x, P.dy, P.R, P.I, P.O, P.N, P.SL, P.part, partb, s, comb, combb, 0, 0);
  else wgrad_v2_body<1, 1>(P.x, P.dy, P.R, P.I, P.O, P.N, P.SL, P.part, partb, s, comb, combb, P.sbx, P.sbdy);
}

struct WgradOut {
  const float* part[2];  // partial sets of the (up to two) calls feeding this output
  float* dw;
  float* db;
  int S[2];
  int nseg, OI, O, blk0;
};
struct WgradOuts {
  int G;
  WgradOut p[kGroupMax];
};

// The tree of wgrad_reduce_kernel for output element e of one partial set (all threads of
// the block call it; red = the block's [kRedGroups][64] LDS).
__device__ __forceinline__ float wgrad_tree(const float* __restrict__ part, int S, int OI, int O, int e,
                                            float (*red)[64]) {
  const int grp = threadIdx.x >> 6;
  const bool is_w = e < OI, is_b = !is_w && e < OI + O;
  float v = 0.f;
  if (is_w || is_b) {
    const float* p = is_w ? part + e : part + (int64_t)S * OI + (e - OI);
    const int64_t st = is_w ? OI : O;
    const int s0 = (S * grp) / kRedGroups, s1 = (S * (grp + 1)) / kRedGroups;
    float a0 = 0.f, a1 = 0.f;
    int s = s0;
    for (; s + 2 <= s1; s += 2) {
      a0 += p[(int64_t)s * st];
      a1 += p[(int64_t)(s + 1) * st];
    }
    if (s < s1) a0 += p[(int64_t)s * st];
    v = a0 + a1;
  }
  __syncthreads();  // red reused across calls
  red[grp][threadIdx.x & 63] = v;
  __syncthreads();
#pragma unroll
  for (int half = kRedGroups / 2; half >= 1; half >>= 1) {
    if (grp < half) red[grp][threadIdx.x & 63] += red[grp + half][threadIdx.x & 63];
    __syncthreads();
  }
  return red[0][threadIdx.x & 63];
}

__global__ __launch_bounds__(64 * kRedGroups) void wgrad_grouped_reduce_kernel(const WgradOuts tab) {
  __shared__ float red[kRedGroups][64];
  const int b = blockIdx.x;
  int g = 0;
  while (g + 1 < tab.G && b >= tab.p[g + 1].blk0) ++g;
  const WgradOut& P = tab.p[g];
  const int e = (b - P.blk0) * 64 + (threadIdx.x & 63);
  float r = wgrad_tree(P.part[0], P.S[0], P.OI, P.O, e, red);
  if (P.nseg > 1) r = r + wgrad_tree(P.part[1], P.S[1], P.OI, P.O, e, red);
  if ((threadIdx.x >> 6) == 0 && e < P.OI + P.O) {
    if (e < P.OI) P.dw[e] = r;
    else if (P.db) P.db[e - P.OI] = r;
  }
}

// Rows per slice of a grouped problem: ~kGroupSlices slices (whole 16-row batches, >= 128
// rows); the group supplies the parallelism the single-layer launch gets from ~320 slices.
constexpr int kGroupSlices = 64;
inline int64_t grouped_slice_rows(int64_t R) {
  int64_t SL = (R + kGroupSlices - 1) / kGroupSlices;
  SL = (SL + 15) / 16 * 16;
  return SL < kSlice ? kSlice : SL;
}

// ---- Weight gradients on the LDS-DMA pipeline (round 4, the grouped path's default) ----
// Round 3's wgrad_v2_body gave each of 8 waves one 32 x 32 output tile and had every wave load
// its own columns of x and dy straight into VGPRs: each row was fetched by To + Ti waves and
// only two 16-row batches were in flight per wave (0.20 ms/step at 0.2 of the f32 MFMA rate and
// 0.3 of HBM). Here a block is 4 waves, one per SIMD, over one slice of one problem's rows; wave
// w walks the slice's 16-row tiles w, w + 4, ... through a ring of D LDS slots filled by
// global_load_lds_dwordx4 (x rows, then dy rows: each byte fetched once, D - 1 tiles in flight
// at no VGPR cost), and holds the WHOLE [O, I] gradient as TO x TI 16 x 16 accumulators
// (v_mfma_f32_16x16x4f32: A[o][k] = dY[row k][o], B[k][i] = X[row k][i]). The 4 waves' sums are
// added through LDS in wave order and written as the block's partial; the grouped reduction sums
// the partials in block order (deterministic, as before).
//   layout 0 ([R, C]): the slot holds glds_rows images (row-major, 16-B chunks XOR-swizzled per
//     row); k-step q, lane (g, m) takes row 4 q + g and the TO (TI) CONSECUTIVE channels
//     TO m .. TO m + TO - 1 of dy (x) in one vector read: accumulator tile t holds o = TO m' + t.
//     The last tile of a problem may be ragged: its clamped rows get dy = 0.
//   layout 1 ([Bn, C, N], N % 16 == 0, batch stride 4-aligned): the slot holds per channel the
//     tile's 16 rows, 16-B chunk j of channel c at position j ^ ((c >> 2) & 3) (XOR on the
//     SOURCE address: conflict-free reads); lane (g, m) reads rows 4 g .. 4 g + 3 of channel
//     m + 16 t as one vector, i.e. k-step q takes row 4 g + q (any bijection works: A and B use
//     the same one). Tile t holds o = m' + 16 t.
// Bias: db[o] = the sum of the dy values the lanes feed the MFMAs (fixed order).
constexpr int kWgBlocks = 1024;  // blocks per grouped launch: 4 x the CU count (MI355X: 256; wg_budget)
constexpr int kWgLdsBytes = 4 * 3 * 16 * (128 + 64) * 4;  // 3 slots per wave of the largest (I + O = 192)
// ring depth: as many slots as the LDS holds, <= 8 (bytes in flight per CU = 4 (D - 1) slots:
// the thin problems are HBM-bound and need the depth, the wide ones have the MFMA work)
constexpr int wg_depth(int slot_floats) {
  return kWgLdsBytes / (4 * slot_floats * 4) < 8 ? kWgLdsBytes / (4 * slot_floats * 4) : 8;
}

// XT / DT > 0: x (dy) is a thin rows-layout operand of XT (DT) < 16 channels (TI = 1 / TO = 1):
// the input layer 3 -> 64 and the 32 -> 1 heads; lanes m >= XT (DT) feed zeros.
template <int LAYOUT, int TI, int TO, int XT = 0, int DT = 0>
__device__ __forceinline__ void wgrad_glds_body(const WgradProblem& P, int s, float* lds) {
  static_assert((XT == 0 || (TI == 1 && LAYOUT == 0)) && (DT == 0 || (TO == 1 && LAYOUT == 0)), "thin operands");
  constexpr int I = 16 * TI, O = 16 * TO;
  constexpr int XS = XT ? 64 * ((16 * XT + 63) / 64) : 16 * I;  // slot floats of the x rows
  constexpr int DS = DT ? 64 * ((16 * DT + 63) / 64) : 16 * O;  // and of the dy rows
  constexpr int SLOT = XS + DS;
  constexpr int G = (XT ? (16 * XT + 63) / 64 : I / 16) + (DT ? (16 * DT + 63) / 64 : O / 16);  // glds per tile
  constexpr int kWgD = wg_depth(SLOT);
  const int lane = pk::lane_id(), wv = pk::wave_id(), m = lane & 15, g = lane >> 4;
  const int64_t r0 = (int64_t)s * P.SL;
  const int64_t r1 = r0 + P.SL < P.R ? r0 + P.SL : P.R;
  const int64_t ntile = (r1 - r0 + 15) >> 4;
  const int64_t nt = ntile > wv ? (ntile - 1 - wv) / 4 + 1 : 0;  // tiles of this wave
  const int64_t sbx = P.sbx ? P.sbx : (int64_t)I * P.N, sbdy = P.sbdy ? P.sbdy : (int64_t)O * P.N;
  float* ring = lds + wv * kWgD * SLOT;
  constexpr int NX = XT ? (16 * XT + 63) / 64 : I / 16, ND = DT ? (16 * DT + 63) / 64 : O / 16;
  int offx[NX], offd[ND];  // lane offsets of the glds chunks (4-B pieces for a thin operand)
  if constexpr (LAYOUT == 0) {
    if constexpr (XT > 0) {
#pragma unroll
      for (int j = 0; j < NX; ++j) offx[j] = j * 64 + lane;
    } else {
      glds_rows_off<I>(I, I, lane, offx);
    }
    if constexpr (DT > 0) {
#pragma unroll
      for (int j = 0; j < ND; ++j) offd[j] = j * 64 + lane;
    } else {
      glds_rows_off<O>(O, O, lane, offd);
    }
  } else {
    glds_cf_off<I>(P.N, lane, offx);
    glds_cf_off<O>(P.N, lane, offd);
  }
  // channels-first issue cursor: item cb, first point cn of the next tile to issue (tiles of a
  // wave step by 64 rows; N % 16 == 0, so a 16-row tile never straddles two items)
  int64_t cb = 0, cn = 0, lb = 0, ln = 0, lrow = 0;
  if constexpr (LAYOUT == 1) {
    const int64_t rs = r0 + 16 * wv;
    cb = rs / P.N;
    cn = rs - cb * P.N;
  }
  auto issue = [&](int64_t k) {  // glds of the wave's k-th tile (clamped: constant op count)
    float* sl = ring + (k % kWgD) * SLOT;
    if (k < nt) {
      lrow = r0 + 16 * (wv + 4 * k);
      if constexpr (LAYOUT == 1) {
        lb = cb;
        ln = cn;
        cn += 64;
        while (cn >= P.N) {
          cn -= P.N;
          ++cb;
        }
      }
    }
    const int64_t row0 = lrow;
    if constexpr (LAYOUT == 0) {
      // thin operands: every lane of the 4-B glds loads one float, 64 per instruction, past the
      // tile's 16 C: always clamped to the tensor (glds_thin), whatever the tile
      const bool full = row0 + 16 <= P.R;  // (wave-uniform) all rows in range
      if constexpr (XT > 0) glds_thin<XT>(P.x, row0, P.R, sl, lane);
      else if (full) glds_issue<NX, 16>(P.x + row0 * I, offx, sl);
      else glds_rows<I>(P.x, I, row0, P.R, I, sl, lane);
      if constexpr (DT > 0) glds_thin<DT>(P.dy, row0, P.R, sl + XS, lane);
      else if (full) glds_issue<ND, 16>(P.dy + row0 * O, offd, sl + XS);
      else glds_rows<O>(P.dy, O, row0, P.R, O, sl + XS, lane);
    } else {
      glds_issue<NX, 16>(P.x + lb * sbx + ln, offx, sl);
      glds_issue<ND, 16>(P.dy + lb * sbdy + ln, offd, sl + XS);
    }
  };
  f32x4 acc[TO][TI];
  float bs[TO];
#pragma unroll
  for (int t = 0; t < TO; ++t) {
    bs[t] = 0.f;
#pragma unroll
    for (int u = 0; u < TI; ++u) acc[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  if (nt > 0) {
#pragma unroll
    for (int k = 0; k < kWgD - 1; ++k) issue(k);
    for (int64_t k = 0; k < nt; ++k) {
      issue(k + kWgD - 1);
      vm_wait<(kWgD - 1) * G>();  // tile k landed (glds retire in issue order)
      const float* sx = ring + (k % kWgD) * SLOT;
      const float* sd = sx + XS;
      if constexpr (LAYOUT == 0) {
        const int64_t row0 = r0 + 16 * (wv + 4 * k);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = 4 * q + g;
          float a[TO], b[TI];
          if constexpr (DT > 0) a[0] = m < DT ? sd[row * DT + m] : 0.f;
          else lds_rowvec<O, TO>(sd, row, m, a);
          if constexpr (XT > 0) b[0] = m < XT ? sx[row * XT + m] : 0.f;
          else lds_rowvec<I, TI>(sx, row, m, b);
          if (row0 + 16 > P.R) {  // (wave-uniform) clamped rows of a ragged last tile: dy = 0
            const bool ok = row0 + row < P.R;
#pragma unroll
            for (int t = 0; t < TO; ++t) a[t] = ok ? a[t] : 0.f;
          }
#pragma unroll
          for (int t = 0; t < TO; ++t) bs[t] += a[t];
#pragma unroll
          for (int t = 0; t < TO; ++t)
#pragma unroll
            for (int u = 0; u < TI; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b[u], acc[t][u], 0, 0, 0);
        }
      } else {
        f32x4 a[TO], b[TI];
#pragma unroll
        for (int t = 0; t < TO; ++t) {
          const int c = m + 16 * t;
          a[t] = *reinterpret_cast<const f32x4*>(sd + 16 * c + 4 * (g ^ ((c >> 2) & 3)));
          bs[t] += (a[t][0] + a[t][1]) + (a[t][2] + a[t][3]);
        }
#pragma unroll
        for (int u = 0; u < TI; ++u) {
          const int c = m + 16 * u;
          b[u] = *reinterpret_cast<const f32x4*>(sx + 16 * c + 4 * (g ^ ((c >> 2) & 3)));
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int t = 0; t < TO; ++t)
#pragma unroll
            for (int u = 0; u < TI; ++u)
              acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][q], b[u][q], acc[t][u], 0, 0, 0);
      }
    }
  }
  vm_wait<0>();
  // bias: the four row groups g of a channel, fixed order
#pragma unroll
  for (int t = 0; t < TO; ++t) {
    bs[t] += __shfl_xor(bs[t], 16);
    bs[t] += __shfl_xor(bs[t], 32);
  }
  __syncthreads();  // every wave is done with its ring: the LDS now holds waves 1..3's sums
  constexpr int NA = TO * TI * 4;
  if (wv > 0) {
    float* dst = lds + (wv - 1) * (NA + TO) * 64;
#pragma unroll
    for (int t = 0; t < TO; ++t)
#pragma unroll
      for (int u = 0; u < TI; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[((t * TI + u) * 4 + r) * 64 + lane] = acc[t][u][r];
#pragma unroll
    for (int t = 0; t < TO; ++t) dst[(NA + t) * 64 + lane] = bs[t];
  }
  __syncthreads();
  if (wv != 0) return;
#pragma unroll
  for (int w = 0; w < 3; ++w) {
    const float* src = lds + w * (NA + TO) * 64;
#pragma unroll
    for (int t = 0; t < TO; ++t) {
#pragma unroll
      for (int u = 0; u < TI; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][u][r] += src[((t * TI + u) * 4 + r) * 64 + lane];
      bs[t] += src[(NA + t) * 64 + lane];
    }
  }
  float* ps = P.part + (int64_t)s * P.O * P.I;
  float* pb = P.part + (int64_t)P.S * P.O * P.I + (int64_t)s * P.O;
#pragma unroll
  for (int t = 0; t < TO; ++t) {
#pragma unroll
    for (int u = 0; u < TI; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ol = 4 * g + r;
        const int o = LAYOUT == 0 ? TO * ol + t : ol + 16 * t;
        const int i = LAYOUT == 0 ? TI * m + u : m + 16 * u;
        if ((XT == 0 || i < XT) && (DT == 0 || o < DT)) ps[o * P.I + i] = acc[t][u][r];
      }
    const int ob = LAYOUT == 0 ? TO * m + t : m + 16 * t;
    if (g == 0 && (DT == 0 || ob < DT)) pb[ob] = bs[t];
  }
}

// Shapes on the pipeline: I, O in {16, 32, 64, 128}, O I <= 8192 (the acc of one wave), and the
// thin rows-layout shapes below.
// Thin rows-layout shapes (the step's 3 -> 64 input layer and 32 -> 1 heads): ids 16, 17.
__host__ __device__ constexpr int wg_shape_id(int I, int O, int layout = 0) {
  return (I == 16 || I == 32 || I == 64 || I == 128) && (O == 16 || O == 32 || O == 64 || O == 128) && I * O <= 8192
             ? (I == 16 ? 0 : I == 32 ? 1 : I == 64 ? 2 : 3) * 4 + (O == 16 ? 0 : O == 32 ? 1 : O == 64 ? 2 : 3)
         : layout == 0 && I == 3 && O == 64 ? 16
         : layout == 0 && I == 32 && O == 1 ? 17
                                            : -1;
}

template <int LAYOUT>
__device__ __forceinline__ void wgrad_glds_dispatch(const WgradProblem& P, int s, float* lds) {
  switch (wg_shape_id(P.I, P.O, LAYOUT)) {
#define PK_WG(I_, O_) case wg_shape_id(I_, O_): wgrad_glds_body<LAYOUT, I_ / 16, O_ / 16>(P, s, lds); break;
    PK_WG(16, 16) PK_WG(16, 32) PK_WG(16, 64) PK_WG(16, 128)
    PK_WG(32, 16) PK_WG(32, 32) PK_WG(32, 64) PK_WG(32, 128)
    PK_WG(64, 16) PK_WG(64, 32) PK_WG(64, 64) PK_WG(64, 128)
    PK_WG(128, 16) PK_WG(128, 32) PK_WG(128, 64)
#undef PK_WG
    case 16:
      if constexpr (LAYOUT == 0) wgrad_glds_body<0, 1, 4, 3, 0>(P, s, lds);
      break;
    case 17:
      if constexpr (LAYOUT == 0) wgrad_glds_body<0, 2, 1, 0, 1>(P, s, lds);
      break;
    default: break;
  }
}

__global__ __launch_bounds__(256, 1) void wgrad_glds_grouped_kernel(const WgradProblems tab) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int b = blockIdx.x;
  int g = 0;
  while (g + 1 < tab.G && b >= tab.p[g + 1].blk0) ++g;  // block-uniform scan
  const WgradProblem& P = tab.p[g];
  if (P.layout == 0) wgrad_glds_dispatch<0>(P, b - P.blk0, lds);
  else wgrad_glds_dispatch<1>(P, b - P.blk0, lds);
}

}  // namespace

extern "C" int pk_linear_wgrad(const float* x, const float* dy, int layout, int64_t R, int I, int O, int N,
                               float* work, float* dw, float* db, int accumulate, void* stream) {
  PK_REQUIRE((layout == 0 || layout == 1) && R >= 0 && I > 0 && O > 0 && I <= kMaxC && O <= kMaxC);
  PK_REQUIRE(layout == 0 || N > 0);
  PK_REQUIRE(((I + 15) / 16) * ((O + 15) / 16) <= 4 * kMaxTilesPerWave);
  PK_REQUIRE(dw != nullptr);
  hipStream_t s = pk::as_stream(stream);
  const int S = (int)((R + kSlice - 1) / kSlice);
  if (S == 0) {
    if (accumulate) return PK_OK;  // no rows: nothing to add
    hipError_t e = pk::zero_async(dw, sizeof(float) * O * I, s);
    if (e == hipSuccess && db) e = pk::zero_async(db, sizeof(float) * O, s);
    return e == hipSuccess ? PK_OK : (int)e;
  }
  PK_REQUIRE(x && dy && work);
  float* part = work;
  // direct-load kernel: slices of >= 128 rows (so S never exceeds the documented work
  // size), ~320 slices for the large calls
  int S2;
  {
    int64_t SL = (R + 319) / 320;
    SL = (SL + 15) / 16 * 16;
    if (SL < kSlice) SL = kSlice;
    S2 = (int)((R + SL - 1) / SL);
    float* partb = work + (int64_t)S2 * O * I;
    const int T = ((O + 31) / 32) * ((I + 31) / 32);
    const int J = T <= kV2Waves ? 1 : 2;
    auto kern = layout == 0 ? (J == 1 ? wgrad_v2_kernel<0, 1> : wgrad_v2_kernel<0, 2>)
                            : (J == 1 ? wgrad_v2_kernel<1, 1> : wgrad_v2_kernel<1, 2>);
    hipLaunchKernelGGL(kern, dim3(S2), dim3(64 * kV2Waves), 0, s, x, dy, R, I, O, N, (int)SL, part, partb);
  }
  PK_CHECK_LAUNCH();
  const int total = O * I + O;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((total + 63) / 64), dim3(64 * kRedGroups), 0, s, part,
                     work + (int64_t)S2 * O * I, S2, O * I, O, dw, db, accumulate);
  PK_CHECK_LAUNCH();
  return PK_OK;
}

// Slicing of a grouped call list. Pipeline problems (wgrad_glds_grouped_kernel: shape on
// wg_shape_id, channels-first only with N % 16 == 0, 16-B aligned operands) get blocks in
// proportion to their cost (wg_cost), about kWgBlocks in all (slices of whole 16-row tiles, >= 64
// rows); the others keep round 3's wgrad_v2 slicing. S[c] partials of call c, SL[c] rows each.
static bool wg_on_pipeline(const pk_wgrad_call& k) {
  return k.R > 0 && wg_shape_id(k.I, k.O, k.layout) >= 0 && (k.layout == 0 || k.N % 16 == 0) &&
         ((reinterpret_cast<uintptr_t>(k.x) | reinterpret_cast<uintptr_t>(k.dy)) & 15) == 0;
}

// a problem's time at the chip's rates, in HBM bytes: max(its bytes, its flops / (157.3 TF /
// 8 TB/s)) — the thin layers are byte-bound, the 128 x 64 ones flop-bound
static double wg_cost(const pk_wgrad_call& k) {
  const double bytes = 4.0 * (double)k.R * (k.I + k.O), flops = 2.0 * (double)k.R * k.I * k.O;
  return bytes > flops / 19.66 ? bytes : flops / 19.66;
}

// Blocks: one resident per CU (each holds 144 KB of LDS), so the launch runs in rounds; 4 x the
// CU count lets the dispatcher balance what the cost model misses (measured, tools/wg_bench.py
// under rocprofv3, whole step's call list: 240 / 248 / 252 / 256 blocks 243-248 us — one round,
// bound by its slowest slice — 496 135 us, 1024 136 us, 2048 155 us). Shares of the budget by
// cost, floored (>= 1 block, >= 64 rows each), leftovers to the largest remainders.
static int wg_budget() {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) !=
                                                 hipSuccess || n <= 0)
      n = kWgBlocks / 4;
    n *= 4;
    return n;
  }();
  return cus;
}

static void wg_plan(const pk_wgrad_call* calls, int n, std::vector<int64_t>& S, std::vector<int64_t>& SL,
                    std::vector<char>& glds) {
  S.assign(n, 0);
  SL.assign(n, 0);
  glds.assign(n, 0);
  double wtot = 0.0;
  int ne = 0;
  for (int c = 0; c < n; ++c)
    if (wg_on_pipeline(calls[c])) {
      wtot += wg_cost(calls[c]);
      ++ne;
    }
  std::vector<int64_t> nb(n, 0);
  std::vector<double> want(n, 0.0);
  if (ne > 0) {
    const int budget = wg_budget() > ne ? wg_budget() : ne;
    int64_t tot = 0;
    for (int c = 0; c < n; ++c) {
      if (!wg_on_pipeline(calls[c])) continue;
      const int64_t cap = (calls[c].R + 63) / 64;
      want[c] = wg_cost(calls[c]) / wtot * budget;
      int64_t v = (int64_t)want[c];
      nb[c] = v < 1 ? 1 : v > cap ? cap : v;
      tot += nb[c];
    }
    while (tot > budget) {  // (only from the >= 1 floors) take from the largest
      int best = -1;
      for (int c = 0; c < n; ++c)
        if (nb[c] > 1 && (best < 0 || nb[c] > nb[best])) best = c;
      if (best < 0) break;
      --nb[best];
      --tot;
    }
    while (tot < budget) {  // leftover CUs to the largest remainders (below their row cap)
      int best = -1;
      double rem = -1e300;
      for (int c = 0; c < n; ++c) {
        if (!wg_on_pipeline(calls[c]) || nb[c] >= (calls[c].R + 63) / 64) continue;
        const double r = want[c] - (double)nb[c];
        if (r > rem) {
          rem = r;
          best = c;
        }
      }
      if (best < 0) break;
      ++nb[best];
      ++tot;
    }
  }
  for (int c = 0; c < n; ++c) {
    const pk_wgrad_call& k = calls[c];
    if (k.R <= 0) continue;
    if (wg_on_pipeline(k)) {
      glds[c] = 1;
      SL[c] = ((k.R + nb[c] - 1) / nb[c] + 15) / 16 * 16;
    } else {
      SL[c] = grouped_slice_rows(k.R);
    }
    S[c] = (k.R + SL[c] - 1) / SL[c];
  }
}

extern "C" int64_t pk_linear_wgrad_grouped_work(const pk_wgrad_call* calls, int n) {
  if (n < 0 || (n > 0 && calls == nullptr)) return -1;
  std::vector<int64_t> S, SL;
  std::vector<char> glds;
  wg_plan(calls, n, S, SL, glds);
  int64_t tot = 0;
  for (int c = 0; c < n; ++c) tot += S[c] * ((int64_t)calls[c].O * calls[c].I + calls[c].O);
  return tot;
}

extern "C" int pk_linear_wgrad_grouped(const pk_wgrad_call* calls, int n, float* work, int64_t work_elems,
                                       void* stream) {
  PK_REQUIRE(n >= 0 && (n == 0 || calls != nullptr));
  hipStream_t st = pk::as_stream(stream);
  // validate; a call with accumulate = 1 must name the dw (and db) of an earlier call
  std::vector<int> first(n, -1), second(n, -1);
  for (int c = 0; c < n; ++c) {
    const pk_wgrad_call& k = calls[c];
    PK_REQUIRE(k.dw && k.R >= 0 && k.I > 0 && k.O > 0 && k.I <= kMaxC && k.O <= kMaxC);
    PK_REQUIRE(((k.O + 31) / 32) * ((k.I + 31) / 32) <= kV2Waves);  // one 32x32 tile per wave
    PK_REQUIRE(k.layout == 0 || (k.layout == 1 && k.N > 0));
    PK_REQUIRE((k.sx == 0 && k.sdy == 0) || (k.layout == 1 && k.sx >= 0 && k.sdy >= 0 && k.sx % 4 == 0 &&
                                               k.sdy % 4 == 0));
    PK_REQUIRE(k.R == 0 || (k.x && k.dy));
    if (k.accumulate) {
      int f = -1;
      for (int q = 0; q < c; ++q)
        if (calls[q].dw == k.dw && !calls[q].accumulate) f = q;
      PK_REQUIRE(f >= 0 && second[f] < 0 && calls[f].I == k.I && calls[f].O == k.O && calls[f].db == k.db);
      second[f] = c;
    }
  }
  const int64_t need = pk_linear_wgrad_grouped_work(calls, n);
  PK_REQUIRE(need <= work_elems && (need == 0 || work != nullptr));
  std::vector<int64_t> S, SLv, off(n, 0);
  std::vector<char> glds;
  wg_plan(calls, n, S, SLv, glds);
  int64_t o = 0;
  for (int c = 0; c < n; ++c) {
    off[c] = o;
    o += S[c] * ((int64_t)calls[c].O * calls[c].I + calls[c].O);
  }
  // pipeline partials: chunks of <= kGroupMax problems
  {
    WgradProblems tp{};
    int blocks = 0;
    auto flush = [&]() -> int {
      if (tp.G == 0) return PK_OK;
      hipLaunchKernelGGL(wgrad_glds_grouped_kernel, dim3(blocks), dim3(256), kWgLdsBytes, st, tp);
      PK_CHECK_LAUNCH();
      tp.G = 0;
      blocks = 0;
      return PK_OK;
    };
    for (int c = 0; c < n; ++c) {
      const pk_wgrad_call& k = calls[c];
      if (S[c] == 0 || !glds[c]) continue;
      WgradProblem& P = tp.p[tp.G++];
      P = WgradProblem{k.x, k.dy, work + off[c], k.R, k.I, k.O, k.N, k.layout, (int)SLv[c], (int)S[c], blocks,
                       0, k.sx, k.sdy};
      blocks += (int)S[c];
      if (tp.G == kGroupMax) {
        const int rc = flush();
        if (rc != PK_OK) return rc;
      }
    }
    const int rc = flush();
    if (rc != PK_OK) return rc;
  }
  // partials: chunks of <= kGroupMax problems
  WgradProblems tp{};
  int blocks = 0;
  auto flush_p = [&]() -> int {
    if (tp.G == 0) return PK_OK;
    hipLaunchKernelGGL(wgrad_grouped_kernel, dim3(blocks), dim3(64 * kV2Waves), 0, st, tp);
    PK_CHECK_LAUNCH();
    tp.G = 0;
    blocks = 0;
    return PK_OK;
  };
  for (int c = 0; c < n; ++c) {
    const pk_wgrad_call& k = calls[c];
    if (S[c] == 0 || glds[c]) continue;
    WgradProblem& P = tp.p[tp.G++];
    P = WgradProblem{k.x, k.dy, work + off[c], k.R, k.I, k.O, k.N, k.layout, (int)SLv[c], (int)S[c], blocks, 0,
                     k.sx, k.sdy};
    blocks += (int)S[c];
    if (tp.G == kGroupMax) {
      const int rc = flush_p();
      if (rc != PK_OK) return rc;
    }
  }
  int rc = flush_p();
  if (rc != PK_OK) return rc;
  // reductions: one output per non-accumulating call (plus its accumulating partner)
  WgradOuts to{};
  blocks = 0;
  auto flush_r = [&]() -> int {
    if (to.G == 0) return PK_OK;
    hipLaunchKernelGGL(wgrad_grouped_reduce_kernel, dim3(blocks), dim3(64 * kRedGroups), 0, st, to);
    PK_CHECK_LAUNCH();
    to.G = 0;
    blocks = 0;
    return PK_OK;
  };
  for (int c = 0; c < n; ++c) {
    const pk_wgrad_call& k = calls[c];
    if (k.accumulate) continue;
    int segs[2] = {c, second[c]};
    WgradOut W{};
    W.dw = k.dw;
    W.db = k.db;
    W.OI = k.O * k.I;
    W.O = k.O;
    W.nseg = 0;
    for (int q = 0; q < 2; ++q) {
      const int cc = segs[q];
      if (cc < 0 || S[cc] == 0) continue;  // no rows: contributes zero
      W.part[W.nseg] = work + off[cc];
      W.S[W.nseg] = (int)S[cc];
      ++W.nseg;
    }
    if (W.nseg == 0) {  // no rows in any feeding call: the gradient is zero
      hipError_t e = pk::zero_async(k.dw, sizeof(float) * k.O * k.I, st);
      if (e == hipSuccess && k.db) e = pk::zero_async(k.db, sizeof(float) * k.O, st);
      if (e != hipSuccess) return (int)e;
      continue;
    }
    W.blk0 = blocks;
    to.p[to.G++] = W;
    blocks += (W.OI + W.O + 63) / 64;
    if (to.G == kGroupMax) {
      rc = flush_r();
      if (rc != PK_OK) return rc;
    }
  }
  return flush_r();
}
