// Per-point layer products (forward and input gradient) of the per-point layers of H7 / H8 (the
// layers whose weight gradients are in linear_wgrad.hip; pk_linear_ex, pk_linear_ex2, pk_linear_fwd):
//   forward   y = x W^T (+ b) (then ReLU if asked)       W [O, I]
//   dgrad     dx = dy W            (= the forward with the weight transposed, no bias)
// in both layouts (0: [R, C] rows, nn.Linear; 1: [Bn, C, N], Conv1d(k=1)). I, O <= 128.
// Generic kernel (linear_fwd_kernel; the shape-specific kernels follow): one wave computes 32 points x all outputs on v_mfma_f32_32x32x2_f32 (up to four 32x32
// accumulators); the weight sits in LDS, the points' operands are loaded straight from
// global memory once. Contraction index k is split in halves across the lane halves
// (k = h * KH + s at step s), so a lane reads one contiguous half-row (layout 0) or the
// same column of KH consecutive channel rows (layout 1, 128-B coalesced across lanes).
// Replaces the library GEMM + separate bias / transpose kernels of these tall-skinny
// shapes (32k-65k points x <= 128 channels).
#include "mfma_tile.hpp"
#include "../../include/posekern.h"

#include <algorithm>

using namespace pk;  // the tile helpers of mfma_tile.hpp

namespace {

constexpr int kLfMaxC = 128;
constexpr int kRowsMaxBlocks = 4096;  // rows kernel grid cap (4 waves per block)

// ReLU backward folded into an input-gradient epilogue: mask = the forward output of the layer
// whose gradient this is (aten threshold_backward(grad, mask, 0): mask <= 0 -> 0)
__device__ __forceinline__ float relu_mask(float v, const float* __restrict__ mask, int64_t i) {
  return (mask != nullptr && mask[i] <= 0.f) ? 0.f : v;
}

// Output side of a per-point layer launch (pk_linear_ex): where y goes and what the epilogue
// folds in. Strides are element strides: rows layout — row stride; channels-first — batch
// stride (the channel stride is N). v = acc + bias; ReLU; mask (contiguous, the ReLU backward
// of the producing layer); + add (columns < add_cols); then stored to y (columns < split) or
// y2 (columns >= split, at column - split), or channels-first when store_cf (rows kernels).
struct LinEpi {
  float* y;
  int64_t sy;
  float* y2;
  int64_t sy2;
  int split;
  const float* add;
  int64_t sa;
  int add_cols;
  const float* mask;
  int relu;  // 0 none, 1 ReLU, 2 sigmoid (1 / (1 + exp(-v)))
  int store_cf;
  int N;
  const float* pre;  // thin kernels: input x scaled by pre (1 - pre) first (sigmoid backward)
  float* pre_out;    // ... and that scaled input written here (same indexing as x)
  const float* add2;  // channels-first kernels: a second added operand (every output), batch stride sa2
  int64_t sa2;
  const float* w2;    // stacked weight rows >= wsplit (lr_stage), and bias entries >= wsplit from bias2
  const float* bias2;
  int wsplit;
};

__device__ __forceinline__ float lin_act(int act, float v) {
  return act == 1 ? fmaxf(v, 0.f) : act == 2 ? 1.f / (1.f + expf(-v)) : v;
}

template <int LAYOUT>
__global__ __launch_bounds__(256) void linear_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, int64_t R, int N, int Cin,
                                                         int Cout, int transw, int relu, const float* __restrict__ mask,
    float* __restrict__ y) {
  // weight as Ws[out][k], out < Cout, k < KP (zero padded); row stride KP + 1 (odd);
  // dynamic LDS of Cout * (KP + 1) floats (<= 64.5 KiB)
  extern __shared__ float Ws[];
  const int KP = (Cin + 3) & ~3, KH = KP >> 1, ST = KP + 1;
  for (int e = threadIdx.x; e < Cout * KP; e += 256) {
    const int o = e / KP, k = e - o * KP;
    float v = 0.f;
    if (k < Cin) v = transw ? w[(int64_t)k * Cout + o] : w[(int64_t)o * Cin + k];
    Ws[o * ST + k] = v;
  }
  __syncthreads();
  const int lane = pk::lane_id(), wave = pk::wave_id();
  const int m = lane & 31, h = lane >> 5;
  const int TO = (Cout + 31) >> 5;
  // 32 points per wave: rows r0 .. r0 + 31 of the flattened point index
  const int64_t r0 = ((int64_t)blockIdx.x * 4 + wave) * 32;
  if (r0 >= R) return;
  const int64_t r = r0 + m;  // this lane's point (its A / B operand column)
  const bool ok = r < R;
  int64_t bb = 0, nn = 0;
  if (LAYOUT == 1) {
    bb = r / N;
    nn = r - bb * N;
  }
  float xa[kLfMaxC / 2];
#pragma unroll
  for (int s = 0; s < kLfMaxC / 2; ++s) {
    if (s < KH) {
      const int k = h * KH + s;
      float v = 0.f;
      if (ok && k < Cin) v = LAYOUT == 0 ? x[r * Cin + k] : x[(bb * Cin + k) * N + nn];
      xa[s] = v;
    }
  }
  f32x16 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
  // layout 0: D[point m][out n] = sum_k x[m][k] W[n][k]  (A = points, B = weight)
  // layout 1: D[out m][point n] = sum_k W[m][k] x[k][n]  (A = weight, B = points)
#pragma unroll
  for (int s = 0; s < kLfMaxC / 2; ++s) {
    if (s < KH) {
      const int k = h * KH + s;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (t < TO) {
          const int o = t * 32 + m;
          const float wv = o < Cout ? Ws[o * ST + k] : 0.f;
          acc[t] = LAYOUT == 0 ? __builtin_amdgcn_mfma_f32_32x32x2f32(xa[s], wv, acc[t], 0, 0, 0)
                               : __builtin_amdgcn_mfma_f32_32x32x2f32(wv, xa[s], acc[t], 0, 0, 0);
        }
      }
    }
  }
  // D element (row 8 (e / 4) + 4 h + e % 4, column m)
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t < TO) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int rr = 8 * (e >> 2) + 4 * h + (e & 3);
        if (LAYOUT == 0) {
          const int64_t pr = r0 + rr;
          const int o = t * 32 + m;
          if (pr < R && o < Cout) {
            float v = acc[t][e] + (bias != nullptr ? bias[o] : 0.f);
            if (relu) v = fmaxf(v, 0.f);
            y[pr * Cout + o] = relu_mask(v, mask, pr * Cout + o);
          }
        } else {
          const int o = t * 32 + rr;
          if (ok && o < Cout) {
            float v = acc[t][e] + (bias != nullptr ? bias[o] : 0.f);
            if (relu) v = fmaxf(v, 0.f);
            y[(bb * Cout + o) * N + nn] = relu_mask(v, mask, (bb * Cout + o) * N + nn);
          }
        }
      }
    }
  }
}

// Row layout (0) with Cin % 16 == 0: one wave computes 16 points x all outputs per tile on
// v_mfma_f32_16x16x4_f32 and walks tiles grid-stride, loading the next tile's operands
// while the current tile's MFMAs run. Contraction index at step (q, i) for lane group g:
// k = 16 q + 4 g + i, so each lane's operands are float4s of its own point row (one load
// instruction covers 16 rows x 64 contiguous bytes) and the weight row chunk is one
// ds_read_b128 from Ws[o][k] (row stride KP + 4: conflict-free over 8-lane phases).

template <int Q, int TO, bool GEN>  // Cin = 16 Q, Cout <= 16 TO; GEN: mask / add / split / cf epilogue
__global__ __launch_bounds__(256) void linear_fwd_rows_kernel(const float* __restrict__ x, int64_t sx,
                                                              const float* __restrict__ w,
                                                              const float* __restrict__ bias, int64_t R, int Cin,
                                                              int Cout, int transw, LinEpi e) {
  extern __shared__ float Ws[];  // [16 TO][Cin + 4]
  constexpr int CI = 16 * Q, ST = CI + 4;
  const int lane = pk::lane_id(), m = lane & 15, g = lane >> 4;
  const int64_t T = (R + 15) >> 4, stride = (int64_t)gridDim.x * 4;
  int64_t tile = (int64_t)blockIdx.x * 4 + pk::wave_id();
  // the first tile's operands are in flight while the weight is staged
  f32x4 cur[Q], nxt[Q];
  lr_load<Q>(x, sx, tile < T ? tile * 16 + m : R, R, g, cur);
  lr_stage<Q, TO>(w, Cout, transw, Ws, w, 1 << 30);
  __syncthreads();
  if (tile >= T) return;
  constexpr int TH = TO < 4 ? TO : 4, NH = TO / TH;
  float bv[TO];
#pragma unroll
  for (int t = 0; t < TO; ++t) {
    const int o = t * 16 + m;
    bv[t] = (bias != nullptr && o < Cout) ? bias[o] : 0.f;
  }
  for (;;) {
    const int64_t tn = tile + stride;
    if (tn < T) lr_load<Q>(x, sx, tn * 16 + m, R, g, nxt);
    // outputs in groups of TH = 4 column tiles (Cout = 128 runs two passes over the same
    // operands): acc / wv / epilogue operands stay at TH tiles, so TO = 8 keeps 4 waves per SIMD
#pragma unroll
    for (int hh = 0; hh < NH; ++hh) {
    __builtin_amdgcn_sched_barrier(0);  // one output group's registers live at a time
    // D[point 4 g + r][out t * 16 + m]; the epilogue's operand loads (mask, add) for all
    // TH x 4 outputs are issued before this group's MFMAs (their latency hides behind them),
    // not one dependent load per store
    // (workgroup-uniform branches around unconditional loads at clamped indices: no per-load
    // exec-mask branch, so no wait per load)
    float mk[TH][4], ad[TH][4];
    if (GEN && e.mask != nullptr) {
#pragma unroll
      for (int t = 0; t < TH; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t pr = tile * 16 + 4 * g + r;
          const int o = (hh * TH + t) * 16 + m;
          const float v = e.mask[(pr < R && o < Cout) ? pr * Cout + o : 0];
          mk[t][r] = v;
        }
    } else {
#pragma unroll
      for (int t = 0; t < TH; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) mk[t][r] = 1.f;
    }
    if (GEN && e.add != nullptr && hh * TH * 16 < e.add_cols) {
#pragma unroll
      for (int t = 0; t < TH; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t pr = tile * 16 + 4 * g + r;
          const int o = (hh * TH + t) * 16 + m;
          const bool ok = pr < R && o < e.add_cols;
          const float v = e.add[ok ? pr * e.sa + o : 0];
          ad[t][r] = ok ? v : 0.f;
        }
    } else {
#pragma unroll
      for (int t = 0; t < TH; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) ad[t][r] = 0.f;
    }
    f32x4 acc[TH];
#pragma unroll
    for (int t = 0; t < TH; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      {
        f32x4 wv[TH];
#pragma unroll
        for (int t = 0; t < TH; ++t)
          wv[t] = *reinterpret_cast<const f32x4*>(&Ws[((hh * TH + t) * 16 + m) * ST + 16 * q + 4 * g]);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int t = 0; t < TH; ++t) {
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[q][i], wv[t][i], acc[t], 0, 0, 0);
          }
        __builtin_amdgcn_sched_barrier(0);  // keep the weight reads per chunk (no hoisting of all Q x TH)
      }
    }
#pragma unroll
    for (int t = 0; t < TH; ++t) {
      const int o = (hh * TH + t) * 16 + m;
      const int64_t p0 = tile * 16 + 4 * g;
      if (GEN && e.store_cf && ((e.N | e.sy) & 3) == 0 && (reinterpret_cast<uintptr_t>(e.y) & 15) == 0 && p0 + 3 < R) {
        // channels-first store: the lane's 4 consecutive points of channel o (one item, as
        // N % 4 == 0) as one 16-B store
        if (o < Cout) {
          f32x4 v4;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float v = lin_act(e.relu, acc[t][r] + bv[hh * TH + t]);
            v = mk[t][r] <= 0.f ? 0.f : v;
            v4[r] = v + ad[t][r];
          }
          const int64_t b = p0 / e.N, n = p0 - b * e.N;
          *reinterpret_cast<f32x4*>(e.y + b * e.sy + (int64_t)o * e.N + n) = v4;
        }
        continue;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t pr = tile * 16 + 4 * g + r;
        if (pr < R && o < Cout) {
          float v = lin_act(e.relu, acc[t][r] + bv[hh * TH + t]);
          v = mk[t][r] <= 0.f ? 0.f : v;  // relu_mask
          v += ad[t][r];  // 0 without add / past add_cols
          if (GEN && e.store_cf) {
            const int64_t b = pr / e.N, n = pr - b * e.N;
            e.y[b * e.sy + (int64_t)o * e.N + n] = v;
          } else if (GEN && o >= e.split) {
            e.y2[pr * e.sy2 + (o - e.split)] = v;
          } else {
            e.y[pr * e.sy + o] = v;
          }
        }
      }
    }
    }
    if (tn >= T) break;
    tile = tn;
#pragma unroll
    for (int q = 0; q < Q; ++q) cur[q] = nxt[q];
  }
}

// Rows layout, LDS-DMA pipeline (the production rows path since round 4 for Cin in {32, 64, 128}):
// round 3 found the per-point layers bound by serialisation, not bytes — every wave resident from
// the start, all loads in one burst, then all MFMAs, then the stores (DESIGN.md §5 'Per-point
// layers'). Here a block is 4 waves, one per SIMD, walking 16-point tiles grid-stride through a
// ring of D LDS slots per wave filled by global_load_lds_dwordx4 (no VGPR cost, so D - 1 tiles
// are in flight while the MFMAs of the current tile run):
//   * slot = the tile's x rows (16 x Cin), then, with GEN, its mask rows and residual rows
//     (16 x 16 TO each), every 16-B chunk XOR-swizzled on the SOURCE address (the LDS image of a
//     glds is lane-linear) so the fragment reads are conflict-free;
//   * the weight sits in VGPRs (A operand: lane (g, m) of output tile t at step (q, i) holds
//     W[16 t + m][16 q + 4 g + i]), so D[out][point]: a lane ends with 4 CONSECUTIVE outputs of one
//     point — bias, mask, residual and the store move as 16-B vectors;
//   * the contraction order (k = 16 q + 4 g + i at step (q, i)) and the epilogue are those of
//     linear_fwd_rows_kernel: results are bit-identical to it;
//   * counted waits: every tile issues the same G glds (tiles past the end are loaded again at a
//     clamped index), so "tile k landed" is s_waitcnt vmcnt((D - 1) G): vector-memory ops retire
//     in issue order and at least the next D - 1 tiles' glds are younger (the stores in between
//     are left out of the count, which only makes the wait more conservative).
// MASK / ADD (GEN epilogues): the ReLU-backward mask rows (shaped like the output) and the
// residual rows (row stride sa, columns < add_cols) ride in the slot; SPLIT: outputs >= split
// (a multiple of 16) go to y2. Cout % 16 == 0, act 0 / 1, no channels-first store (host checks).
template <int Q, int TO, bool MASK, bool ADD, bool SPLIT>
__global__ __launch_bounds__(256, 1) void linear_glds_rows_kernel(const float* __restrict__ x, int64_t sx,
                                                                  const float* __restrict__ w,
                                                                  const float* __restrict__ bias, int64_t R, int Cin,
                                                                  int Cout, int transw, LinEpi e) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int CI = 16 * Q, CO = 16 * TO;
  constexpr int SLOT = 16 * CI + (MASK ? 16 * CO : 0) + (ADD ? 16 * CO : 0);  // floats
  constexpr int G = Q + (MASK ? TO : 0) + (ADD ? TO : 0);  // glds per tile
  constexpr int D = ring_depth(SLOT);
  const int lane = pk::lane_id(), wv = pk::wave_id(), m = lane & 15, g = lane >> 4;
  // weight -> VGPRs through the (not yet used) ring: Ws[o][k], row stride CI + 4
  lr_stage<Q, TO>(w, Cout, transw, lds, w, 1 << 30);
  __syncthreads();
  f32x4 wf[TO][Q];
  chain_wfrag<Q, TO>(lds, m, g, wf);
  f32x4 bv[TO];  // bias of outputs 16 t + 4 g + r
#pragma unroll
  for (int t = 0; t < TO; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = 16 * t + 4 * g + r;
      bv[t][r] = (bias != nullptr && o < Cout) ? bias[o] : 0.f;
    }
  __syncthreads();  // every wave holds its weight: the ring may now overwrite the stage
  float* ring = lds + (int64_t)wv * D * SLOT;
  const int64_t T = (R + 15) >> 4, stride = (int64_t)gridDim.x * 4;
  const int64_t t0 = (int64_t)blockIdx.x * 4 + wv;
  if (t0 >= T) return;
  const int64_t nt = (T - 1 - t0) / stride + 1;  // tiles of this wave
  // lane offsets of the glds chunks, computed once (a full tile is then issued from a scalar base)
  int offx[Q], offm[MASK ? TO : 1], offa[ADD ? TO : 1];
  glds_rows_off<CI>(sx, CI, lane, offx);
  if constexpr (MASK) glds_rows_off<CO>(Cout, Cout, lane, offm);
  if constexpr (ADD) glds_rows_off<CO>(e.sa, e.add_cols, lane, offa);
  auto issue = [&](int64_t k) {  // glds of this wave's k-th tile (clamped: constant op count)
    const int64_t tile = t0 + min(k, nt - 1) * stride;
    float* s = ring + (k % D) * SLOT;
    const int64_t r0 = tile * 16;
    if (r0 + 16 <= R) {  // (wave-uniform) every row in range
      glds_issue<Q, 16>(x + r0 * sx, offx, s);
      if constexpr (MASK) glds_issue<TO, 16>(e.mask + r0 * Cout, offm, s + 16 * CI);
      if constexpr (ADD) glds_issue<TO, 16>(e.add + r0 * e.sa, offa, s + 16 * CI + (MASK ? 16 * CO : 0));
    } else {
      glds_rows<CI>(x, sx, r0, R, CI, s, lane);
      if constexpr (MASK) glds_rows<CO>(e.mask, Cout, r0, R, Cout, s + 16 * CI, lane);
      if constexpr (ADD) glds_rows<CO>(e.add, e.sa, r0, R, e.add_cols, s + 16 * CI + (MASK ? 16 * CO : 0), lane);
    }
  };
#pragma unroll
  for (int k = 0; k < D - 1; ++k) issue(k);
  for (int64_t k = 0; k < nt; ++k) {
    issue(k + D - 1);
    // tile k landed: at least the (D - 1) G glds of tiles k+1 .. k+D-1 are younger than its own
    // (vector-memory ops retire in issue order); the stores issued in between are not counted,
    // so the wait also drains the oldest of them — conservative whatever the stores' exec masks
    vm_wait<(D - 1) * G>();
    const float* s = ring + (k % D) * SLOT;
    const int64_t tile = t0 + k * stride;
    f32x4 acc[TO];
#pragma unroll
    for (int t = 0; t < TO; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const f32x4 xv = lds_chunk<CI>(s, m, 4 * q + g);  // point m, features 16 q + 4 g .. + 3
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int t = 0; t < TO; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[t][q][i], xv[i], acc[t], 0, 0, 0);
    }
    // D[out 16 t + 4 g + r][point m]
    const int64_t pr = tile * 16 + m;
#pragma unroll
    for (int t = 0; t < TO; ++t) {
      f32x4 mk = {1.f, 1.f, 1.f, 1.f}, ad = {0.f, 0.f, 0.f, 0.f};
      if constexpr (MASK) mk = lds_chunk<CO>(s + 16 * CI, m, 4 * t + g);
      if constexpr (ADD) {
        if (16 * t + 4 * g < e.add_cols) ad = lds_chunk<CO>(s + 16 * CI + (MASK ? 16 * CO : 0), m, 4 * t + g);
      }
      f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = 16 * t + 4 * g + r;
        float u = acc[t][r] + bv[t][r];
        u = e.relu ? fmaxf(u, 0.f) : u;  // (act 0 / 1 only here: the host routes sigmoid elsewhere)
        u = mk[r] <= 0.f ? 0.f : u;      // relu_mask
        v[r] = ADD ? u + (o < e.add_cols ? ad[r] : 0.f) : u;
      }
      const int o0 = 16 * t + 4 * g;
      if (pr < R) {
        if (SPLIT && 16 * t >= e.split)  // (split % 16 == 0: wave-uniform per output tile)
          *reinterpret_cast<f32x4*>(&e.y2[pr * e.sy2 + (o0 - e.split)]) = v;
        else
          *reinterpret_cast<f32x4*>(&e.y[pr * e.sy + o0]) = v;
      }
    }
  }
  vm_wait<0>();
}

// Channels-first layout (1) [Bn, C, N] with Cin in {16, 32, 64, 128}: one wave computes 16 SUB
// consecutive points of one item x all outputs; tpc tiles per item (SUB > 1 needs N % (16 SUB)
// == 0; with SUB = 1 an item's last tile may be ragged: its columns past N compute on a clamped
// point and are not stored — the MFMA columns are independent points). A = weight
// (Ws[o][k] chunks, ds_read_b128), B = points: lane (j, g) loads its SUB consecutive points
// as one vector per channel row k = 16 q + 4 g + i, and element u of that
// vector is column j of point sub-tile u (sub-tile u holds points SUB j + u), so loads and
// the D stores (float SUB vectors of consecutive points) are both contiguous per lane.
template <int Q, int TO, int SUB>
__device__ __forceinline__ void linear_cf_body(const float* __restrict__ x, int64_t sx, const float* __restrict__ w,
                                               const float* __restrict__ bias, int64_t R, int N, int Cout, int transw,
                                               const LinEpi& e, int64_t tpc, int64_t blk, float* Ws) {
  using V = typename PtVec<SUB>::T;
  constexpr int CI = 16 * Q, ST = CI + 4, P = 16 * SUB;
  const int lane = pk::lane_id(), m = lane & 15, g = lane >> 4;
  const int64_t T = (R / N) * tpc;
  const int64_t tile = blk * 4 + pk::wave_id();
  // the tile's operands are in flight while the weight is staged
  V xv[Q][4];
  int64_t bb = 0, n0 = 0;
  bool live = true;  // this lane's point column exists (only a SUB = 1 ragged tail has dead ones)
  if (tile < T) {
    bb = tile / tpc;
    n0 = (tile - bb * tpc) * P;
    if (SUB == 1) live = n0 + m < N;
    const float* xb = x + bb * sx + n0 + (live ? SUB * m : 0);
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) xv[q][i] = *reinterpret_cast<const V*>(xb + (int64_t)(16 * q + 4 * g + i) * N);
  }
  lr_stage<Q, TO>(w, Cout, transw, Ws, e.w2 ? e.w2 : w, e.w2 ? e.wsplit : (1 << 30));
  __syncthreads();
  if (tile >= T) return;
  f32x4 acc[TO][SUB];
#pragma unroll
  for (int t = 0; t < TO; ++t)
#pragma unroll
    for (int u = 0; u < SUB; ++u) acc[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    f32x4 wv[TO];
#pragma unroll
    for (int t = 0; t < TO; ++t) wv[t] = *reinterpret_cast<const f32x4*>(&Ws[(t * 16 + m) * ST + 16 * q + 4 * g]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int u = 0; u < SUB; ++u)
#pragma unroll
        for (int t = 0; t < TO; ++t) {
          float b;
          if constexpr (SUB == 1) b = xv[q][i]; else b = xv[q][i][u];
          acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[t][i], b, acc[t][u], 0, 0, 0);
        }
    __builtin_amdgcn_sched_barrier(0);
  }
  // D[out t * 16 + 4 g + r][column m of sub-tile u] = point n0 + SUB m + u
  const int64_t pn = n0 + (live ? SUB * m : 0);
  float* yb = e.y + bb * e.sy + pn;
  const int64_t mb = bb * Cout * (int64_t)N + pn;  // contiguous index (mask)
  // epilogue operands (mask, add) of all TO x 4 output rows loaded before the first use:
  // workgroup-uniform branches around unconditional loads at clamped rows
  V mv[TO][4], av[TO][4];
  float bo4[TO][4];
#pragma unroll
  for (int t = 0; t < TO; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = t * 16 + 4 * g + r;
      bo4[t][r] = 0.f;
      if (bias != nullptr) {
        const int oc = o < Cout ? o : 0;
        const float b = (e.bias2 != nullptr && oc >= e.wsplit) ? e.bias2[oc - e.wsplit] : bias[oc];
        bo4[t][r] = o < Cout ? b : 0.f;
      }
    }
  if (e.mask != nullptr) {
#pragma unroll
    for (int t = 0; t < TO; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = t * 16 + 4 * g + r;
        mv[t][r] = *reinterpret_cast<const V*>(e.mask + mb + (int64_t)(o < Cout ? o : 0) * N);
      }
  }
  if (e.add != nullptr) {
#pragma unroll
    for (int t = 0; t < TO; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = t * 16 + 4 * g + r;
        av[t][r] = *reinterpret_cast<const V*>(e.add + bb * e.sa + (int64_t)(o < e.add_cols ? o : 0) * N + pn);
      }
  }
  V a2v[TO][4];
  if (e.add2 != nullptr) {
#pragma unroll
    for (int t = 0; t < TO; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = t * 16 + 4 * g + r;
        a2v[t][r] = *reinterpret_cast<const V*>(e.add2 + bb * e.sa2 + (int64_t)(o < Cout ? o : 0) * N + pn);
      }
  }
#pragma unroll
  for (int t = 0; t < TO; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = t * 16 + 4 * g + r;
      if (o < Cout && live) {
        const float bo = bo4[t][r];
        const bool has_add = e.add != nullptr && o < e.add_cols;
        V v;
#pragma unroll
        for (int u = 0; u < SUB; ++u) {
          float z = lin_act(e.relu, acc[t][u][r] + bo);
          if (e.mask != nullptr) {
            float mz;
            if constexpr (SUB == 1) mz = mv[t][r]; else mz = mv[t][r][u];
            z = mz <= 0.f ? 0.f : z;
          }
          if (has_add) {
            if constexpr (SUB == 1) z += av[t][r]; else z += av[t][r][u];
          }
          if (e.add2 != nullptr) {  // (z + add) + add2: the order of autograd's two accumulations
            if constexpr (SUB == 1) z += a2v[t][r]; else z += a2v[t][r][u];
          }
          if constexpr (SUB == 1) v = z; else v[u] = z;
        }
        *reinterpret_cast<V*>(yb + (int64_t)o * N) = v;
      }
    }
}

template <int Q, int TO, int SUB>
__global__ __launch_bounds__(256) void linear_fwd_cf_kernel(const float* __restrict__ x, int64_t sx,
                                                            const float* __restrict__ w,
                                                            const float* __restrict__ bias, int64_t R, int N, int Cout,
                                                            int transw, LinEpi e, int64_t tpc) {
  extern __shared__ float Ws[];
  linear_cf_body<Q, TO, SUB>(x, sx, w, bias, R, N, Cout, transw, e, tpc, blockIdx.x, Ws);
}

// Two independent channels-first layers in one launch (pk_linear_ex2): blocks [0, nb0) run
// problem 0, the rest problem 1 — the pair shares one launch's ramp and tail (the refinement's
// q / stacked k-v projections, Pq^T / [Pk; Pv]^T, the two shapes' last_lin).
struct CfProb {
  const float* x;
  int64_t sx;
  const float* w;
  const float* bias;
  int64_t R;
  int N, Cout, transw, pad;
  int64_t tpc;
  LinEpi e;
};

template <int Q0, int TO0, int Q1, int TO1, int SUB>
__global__ __launch_bounds__(256) void linear_cf_pair_kernel(const CfProb p0, const CfProb p1, int nb0) {
  extern __shared__ float Ws[];
  if ((int)blockIdx.x < nb0)
    linear_cf_body<Q0, TO0, SUB>(p0.x, p0.sx, p0.w, p0.bias, p0.R, p0.N, p0.Cout, p0.transw, p0.e, p0.tpc,
                                 blockIdx.x, Ws);
  else
    linear_cf_body<Q1, TO1, SUB>(p1.x, p1.sx, p1.w, p1.bias, p1.R, p1.N, p1.Cout, p1.transw, p1.e, p1.tpc,
                                 (int64_t)blockIdx.x - nb0, Ws);
}

// Thin layers (Cin <= 4 or Cout <= 4: DiffusionNet's first_lin 3 -> 64, the overlap head's
// 32 -> 1 and its input gradient 1 -> 32): too little contraction for MFMA tiles, so plain
// FMAs with the weight in LDS, organised for coalesced memory traffic.
//   rows layout: thread = (point, 4 consecutive outputs), one float4 store per thread
//   channels-first: thread = point n of an item, Cout coalesced row stores
constexpr int kThinMaxW = 4096;  // Cout * Cin floats in LDS

template <int LAYOUT, int CINT>  // CINT: compile-time Cin (1..4), or 0 (runtime Cin, Cout <= 4)
__global__ __launch_bounds__(256) void linear_thin_kernel(const float* __restrict__ x, int64_t sx,
                                                          const float* __restrict__ w,
                                                          const float* __restrict__ bias, int64_t R, int N, int Cin_,
                                                          int Cout, int transw, LinEpi e) {
  const int relu = e.relu;
  const float* __restrict__ mask = e.mask;
  float* __restrict__ y = e.y;
  __shared__ float Ws[kThinMaxW];  // Ws[o * Cin + k]
  __shared__ float bs[kLfMaxC];
  const int Cin = CINT > 0 ? CINT : Cin_;
  // rows layout, compile-time Cin, no prologue (first_lin 3 -> 64): the point's inputs are in
  // flight while the weight is staged (one memory latency instead of two before the stores)
  float xe[CINT > 0 ? CINT : 1];
  if (LAYOUT == 0 && CINT > 0) {
    const int G = (Cout + 3) >> 2;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = t < R * G ? t / G : 0;
#pragma unroll
    for (int k = 0; k < (CINT > 0 ? CINT : 1); ++k) xe[k] = (t < R * G && e.pre == nullptr) ? x[r * sx + k] : 0.f;
  }
  for (int e = threadIdx.x; e < Cout * Cin; e += 256) {
    const int o = e / Cin, k = e - o * Cin;
    Ws[e] = transw ? w[(int64_t)k * Cout + o] : w[e];
  }
  for (int o = threadIdx.x; o < Cout; o += 256) bs[o] = bias ? bias[o] : 0.f;
  __syncthreads();
  if (LAYOUT == 0) {
    const int G = (Cout + 3) >> 2;  // output quads per point
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= R * G) return;
    const int64_t r = t / G;
    const int o0 = (int)(t - r * G) * 4;
    float acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = o0 + u < Cout ? bs[o0 + u] : 0.f;
    int k0 = 0;
    if (CINT == 0 && e.pre == nullptr && ((sx | Cin) & 3) == 0 && (((uintptr_t)x) & 15) == 0) {
      // wide input rows (e.g. the overlap head's 32 -> 1): 16-B loads, all issued up front
      const float4* xr = reinterpret_cast<const float4*>(x + r * sx);
      for (; k0 + 16 <= Cin; k0 += 16) {
        float4 q[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = xr[(k0 >> 2) + j];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float xs[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int k = k0 + 4 * j + i;
#pragma unroll
            for (int u = 0; u < 4; ++u)
              if (o0 + u < Cout) acc[u] = fmaf(xs[i], Ws[(o0 + u) * Cin + k], acc[u]);
          }
        }
      }
    }
#pragma unroll 4
    for (int k = k0; k < Cin; ++k) {
      float xv = (CINT > 0 && e.pre == nullptr) ? xe[CINT > 0 ? k : 0] : x[r * sx + k];
      if (e.pre) {
        const float s = e.pre[r * sx + k];
        xv = xv * (s * (1.f - s));
        if (e.pre_out && o0 == 0) e.pre_out[r * sx + k] = xv;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (o0 + u < Cout) acc[u] = fmaf(xv, Ws[(o0 + u) * Cin + k], acc[u]);
    }
    float mk[4] = {1.f, 1.f, 1.f, 1.f};
    if (mask != nullptr) {  // workgroup-uniform; the loads at clamped indices, then one wait
#pragma unroll
      for (int u = 0; u < 4; ++u) mk[u] = mask[r * Cout + (o0 + u < Cout ? o0 + u : 0)];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = mk[u] <= 0.f ? 0.f : lin_act(relu, acc[u]);
    if ((Cout & 3) == 0 && (e.sy & 3) == 0) {
      *reinterpret_cast<float4*>(y + r * e.sy + o0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (o0 + u < Cout) y[r * e.sy + o0 + u] = acc[u];
    }
  } else {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= R) return;
    const int64_t b = t / N, n = t - b * N;
    const float* __restrict__ xb = x + b * sx + n;
    float* __restrict__ yb = y + b * e.sy + n;
    const int64_t mo = b * Cout * (int64_t)N + n - (yb - y);  // mask index = (yb - y) + mo + o N
    if (CINT > 0) {  // few inputs in registers, one coalesced row store per output
      float xv[CINT > 0 ? CINT : 1];
#pragma unroll
      for (int k = 0; k < CINT; ++k) {
        xv[k] = xb[(int64_t)k * N];
        if (e.pre) {
          const int64_t xi = (xb - x) + (int64_t)k * N;
          const float s = e.pre[xi];
          xv[k] = xv[k] * (s * (1.f - s));
          if (e.pre_out) e.pre_out[xi] = xv[k];
        }
      }
      for (int o = 0; o < Cout; ++o) {
        float a = bs[o];
#pragma unroll
        for (int k = 0; k < CINT; ++k) a = fmaf(xv[k], Ws[o * CINT + k], a);
        yb[(int64_t)o * N] = relu_mask(lin_act(relu, a), mask, (yb - y) + mo + (int64_t)o * N);
      }
    } else {  // Cout <= 4: one coalesced row load per input channel
      float acc[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = u < Cout ? bs[u] : 0.f;
#pragma unroll 8
      for (int k = 0; k < Cin; ++k) {
        float xv = xb[(int64_t)k * N];
        if (e.pre) {
          const int64_t xi = (xb - x) + (int64_t)k * N;
          const float s = e.pre[xi];
          xv = xv * (s * (1.f - s));
          if (e.pre_out) e.pre_out[xi] = xv;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (u < Cout) acc[u] = fmaf(xv, Ws[u * Cin + k], acc[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (u < Cout) yb[(int64_t)u * N] = relu_mask(lin_act(relu, acc[u]), mask, (yb - y) + mo + (int64_t)u * N);
    }
  }
}

}  // namespace

// argument checks, default (contiguous) strides and the epilogue record of one pk_linear_ex call
// (PK_OK or an error status; R == 0 is PK_OK with e and sx_out left alone): the one copy both
// pk_linear_ex and pk_linear_ex2 go through, so the pair and the single call accept the same calls
static int lin_setup(const pk_linear_args* a, LinEpi& e, int64_t& sx_out) {
  PK_REQUIRE(a != nullptr);
  const int layout = a->layout, Cin = a->Cin, Cout = a->Cout, N = a->N;
  const int64_t R = a->R;
  PK_REQUIRE((layout == 0 || layout == 1) && R >= 0 && Cin > 0 && Cout > 0 && Cin <= kLfMaxC && Cout <= kLfMaxC);
  PK_REQUIRE(layout == 0 || (N > 0 && R % N == 0));
  PK_REQUIRE(a->act >= 0 && a->act <= 2);
  if (R == 0) return PK_OK;
  PK_REQUIRE(a->x && a->w && a->y);
  const int split = a->y2 ? a->split : Cout;
  PK_REQUIRE(split >= 1 && split <= Cout && (a->y2 == nullptr || (layout == 0 && !a->store_cf && split < Cout)));
  PK_REQUIRE(a->store_cf == 0 || (layout == 0 && N > 0 && R % N == 0));
  PK_REQUIRE(a->add == nullptr || (a->add_cols >= 1 && a->add_cols <= Cout));
  sx_out = a->ldx ? a->ldx : (layout == 0 ? Cin : (int64_t)Cin * N);
  e = LinEpi{};
  e.y = a->y;
  e.sy = a->ldy ? a->ldy : (layout == 0 && !a->store_cf ? split : (int64_t)Cout * N);
  e.y2 = a->y2;
  e.sy2 = a->ldy2 ? a->ldy2 : Cout - split;
  e.split = split;
  e.add = a->add;
  e.sa = a->lda ? a->lda : (layout == 0 ? (int64_t)(a->add_cols > 0 ? a->add_cols : Cout) : (int64_t)Cout * N);
  e.add_cols = a->add ? a->add_cols : 0;
  e.mask = a->mask;
  e.relu = a->act;
  e.store_cf = a->store_cf;
  e.N = N;
  e.pre = a->pre;
  e.pre_out = a->pre_out;
  e.add2 = a->add2;
  e.sa2 = a->lda2 ? a->lda2 : (int64_t)Cout * N;
  e.w2 = a->w2;
  e.bias2 = a->bias2;
  e.wsplit = a->w2 ? a->wsplit : (1 << 30);
  // stacked weights and the second add operand: channels-first MFMA kernel only
  PK_REQUIRE((a->w2 == nullptr && a->add2 == nullptr && a->bias2 == nullptr) ||
             (layout == 1 && (Cin == 16 || Cin == 32 || Cin == 64 || Cin == 128) &&
              Cin > 4 && Cout > 4 && !a->store_cf && a->y2 == nullptr));
  PK_REQUIRE(a->w2 == nullptr || (a->wsplit > 0 && a->wsplit < (a->transw ? Cin : Cout)));
  PK_REQUIRE(a->bias2 == nullptr || (a->w2 != nullptr && !a->transw));
  PK_REQUIRE((e.pre == nullptr && e.relu != 2) || ((Cin <= 4 || Cout <= 4) && Cin * Cout <= kThinMaxW));
  return PK_OK;
}

// points per wave of the channels-first kernel: 16 SUB, as many as keep >= 1024 waves and <= 64
// operand VGPRs; SUB-aligned items and strides for the vector loads / stores
static int cf_sub(int64_t R, int N, int Cin, int64_t sx, const LinEpi& e) {
  // 16 points per wave below 131,072 rows (round 6: the configs[1] step's 65,536-row layers ran
  // 11 % faster than with 32 — more waves in flight per CU)
  int sub = R >= 131072 ? 4 : 1;
  sub = std::min(sub, 256 / Cin);
  while (sub > 1 && N % (16 * sub)) sub >>= 1;  // N % 16 != 0: SUB = 1 with ragged item tails
  while (sub > 1 && ((sx % sub) || (e.sy % sub) || (e.add && (e.sa % sub)) || (e.add2 && (e.sa2 % sub)))) sub >>= 1;
  return sub;
}

extern "C" int pk_linear_ex2(const pk_linear_args* a0, const pk_linear_args* a1, void* stream) {
  PK_REQUIRE(a0 != nullptr && a1 != nullptr);
  LinEpi e0, e1;
  int64_t sx0 = 0, sx1 = 0;
  int rc = lin_setup(a0, e0, sx0);
  if (rc != PK_OK) return rc;
  rc = lin_setup(a1, e1, sx1);
  if (rc != PK_OK) return rc;
  auto cf_ok = [](const pk_linear_args* a) {
    return a->layout == 1 && a->R > 0 && (a->Cin == 32 || a->Cin == 64) && (a->Cout == 32 || a->Cout == 64) &&
           a->y2 == nullptr && !a->store_cf && a->pre == nullptr && a->act <= 1;
  };
  const int sub0 = cf_ok(a0) ? cf_sub(a0->R, a0->N, a0->Cin, sx0, e0) : 0;
  const int sub1 = cf_ok(a1) ? cf_sub(a1->R, a1->N, a1->Cin, sx1, e1) : 0;
  if (sub0 == 0 || sub0 != sub1 || sub0 == 4) {  // not a pair this kernel takes: two launches
    rc = pk_linear_ex(a0, stream);
    return rc != PK_OK ? rc : pk_linear_ex(a1, stream);
  }
  auto prob = [](const pk_linear_args* a, const LinEpi& e, int64_t sx, int sub) {
    CfProb p{};
    p.x = a->x;
    p.sx = sx;
    p.w = a->w;
    p.bias = a->bias;
    p.R = a->R;
    p.N = a->N;
    p.Cout = a->Cout;
    p.transw = a->transw;
    p.tpc = (a->N + 16 * sub - 1) / (16 * sub);
    p.e = e;
    return p;
  };
  const CfProb p0 = prob(a0, e0, sx0, sub0), p1 = prob(a1, e1, sx1, sub1);
  const int64_t nb0 = ((a0->R / a0->N) * p0.tpc + 3) / 4, nb1 = ((a1->R / a1->N) * p1.tpc + 3) / 4;
  PK_REQUIRE(nb0 + nb1 <= (int64_t)INT32_MAX);
  const int TO0 = a0->Cout / 16, TO1 = a1->Cout / 16;
  const size_t lds = sizeof(float) * std::max((size_t)(16 * TO0) * (a0->Cin + 4), (size_t)(16 * TO1) * (a1->Cin + 4));
  hipStream_t st = pk::as_stream(stream);
  const dim3 grid((unsigned)(nb0 + nb1));
  // 32 / 64 channels (cf_ok) -> 2 / 4 sixteen-wide tiles, as a compile-time constant
  auto by = [](int c, auto f) { return c == 32 ? f(std::integral_constant<int, 2>{}) : f(std::integral_constant<int, 4>{}); };
  auto kern = by(a0->Cin, [&](auto q0) { return by(a0->Cout, [&](auto t0) {
    return by(a1->Cin, [&](auto q1) { return by(a1->Cout, [&](auto t1) {
      constexpr int Q0 = decltype(q0)::value, T0 = decltype(t0)::value, Q1 = decltype(q1)::value, T1 = decltype(t1)::value;
      return sub0 == 2 ? linear_cf_pair_kernel<Q0, T0, Q1, T1, 2> : linear_cf_pair_kernel<Q0, T0, Q1, T1, 1>;
    }); });
  }); });
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, p0, p1, (int)nb0);
  PK_CHECK_LAUNCH();
  return PK_OK;
}

extern "C" int pk_linear_ex(const pk_linear_args* a, void* stream) {
  LinEpi e;
  int64_t sx = 0;
  const int rc = lin_setup(a, e, sx);
  if (rc != PK_OK || a->R == 0) return rc;
  const int layout = a->layout, Cin = a->Cin, Cout = a->Cout, N = a->N, transw = a->transw;
  const int64_t R = a->R;
  const float* x = a->x;
  const float* w = a->w;
  const float* bias = a->bias;
  hipStream_t st = pk::as_stream(stream);
  const bool plain_out = e.y2 == nullptr && e.add == nullptr && !e.store_cf;
  if ((Cin <= 4 || Cout <= 4) && Cin * Cout <= kThinMaxW) {
    PK_REQUIRE(plain_out);  // the thin kernels take strides only
    const int64_t threads = layout == 0 ? R * ((Cout + 3) / 4) : R;
    const dim3 grid((unsigned)((threads + 255) / 256));
    const int ct = Cin <= 4 ? Cin : 0;  // Cin > 4 here means Cout <= 4
    auto pick = [&](auto l) {
      constexpr int L = decltype(l)::value;
      return ct == 1 ? linear_thin_kernel<L, 1> : ct == 2 ? linear_thin_kernel<L, 2> : ct == 3 ? linear_thin_kernel<L, 3>
             : ct == 4 ? linear_thin_kernel<L, 4> : linear_thin_kernel<L, 0>;
    };
    auto kern = layout == 0 ? pick(std::integral_constant<int, 0>{}) : pick(std::integral_constant<int, 1>{});
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, x, sx, w, bias, R, N, Cin, Cout, transw, e);
    PK_CHECK_LAUNCH();
    return PK_OK;
  }
  if (layout == 0 && (Cin == 16 || Cin == 32 || Cin == 64 || Cin == 128) && sx % 4 == 0) {
    // 16-point tiles, 4 per block, at most two blocks per CU's worth of waves in flight
    const int64_t tiles = (R + 15) / 16;
    const unsigned blocks = (unsigned)std::min<int64_t>((tiles + 3) / 4, (int64_t)kRowsMaxBlocks);
    const int TO = Cout <= 16 ? 1 : Cout <= 32 ? 2 : Cout <= 64 ? 4 : 8;
    auto pick = [&](auto q, auto gen) {
      constexpr int Q = decltype(q)::value;
      constexpr bool G = decltype(gen)::value;
      return TO == 1 ? linear_fwd_rows_kernel<Q, 1, G>
             : TO == 2 ? linear_fwd_rows_kernel<Q, 2, G>
             : TO == 4 ? linear_fwd_rows_kernel<Q, 4, G> : linear_fwd_rows_kernel<Q, 8, G>;
    };
    auto pickq = [&](auto gen) {
      return Cin == 16 ? pick(std::integral_constant<int, 1>{}, gen)
             : Cin == 32 ? pick(std::integral_constant<int, 2>{}, gen)
             : Cin == 64 ? pick(std::integral_constant<int, 4>{}, gen) : pick(std::integral_constant<int, 8>{}, gen);
    };
    // plain: no mask, no residual add, one contiguous output (split == Cout)
    const bool plain = e.mask == nullptr && e.add == nullptr && e.y2 == nullptr && !e.store_cf && e.split >= Cout;
    const bool glds_ok = Cin >= 32 && Cout >= 32 && Cout % 16 == 0 && TO * (Cin / 16) <= 32 &&
                         e.relu <= 1 && !e.store_cf && al16(x) && al16(e.y) && e.sy % 4 == 0 &&
                         (e.y2 == nullptr || (al16(e.y2) && e.sy2 % 4 == 0 && e.split % 16 == 0)) &&
                         (e.mask == nullptr || al16(e.mask)) && (e.add == nullptr || (al16(e.add) && e.sa % 4 == 0));
    if (glds_ok) {
      const bool MK = e.mask != nullptr, AD = e.add != nullptr, SP = e.y2 != nullptr;
      const int slot = 16 * Cin + (MK ? 16 * Cout : 0) + (AD ? 16 * Cout : 0);
      const size_t ldsg = std::max((size_t)ring_depth(slot) * 4 * slot, (size_t)(16 * TO) * (Cin + 4)) * sizeof(float);
      const unsigned bg = (unsigned)std::min<int64_t>((tiles + 3) / 4, (int64_t)kRowsPersistCUs);
      auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(bg), dim3(256), ldsg, st, x, sx, w, bias, R, Cin, Cout, transw, e);
      };
      auto pe = [&](auto q, auto to) {
        constexpr int Qv = decltype(q)::value, TOv = decltype(to)::value;
        if (SP) {
          if (MK && AD) launch(linear_glds_rows_kernel<Qv, TOv, true, true, true>);
          else if (MK) launch(linear_glds_rows_kernel<Qv, TOv, true, false, true>);
          else if (AD) launch(linear_glds_rows_kernel<Qv, TOv, false, true, true>);
          else launch(linear_glds_rows_kernel<Qv, TOv, false, false, true>);
        } else {
          if (MK && AD) launch(linear_glds_rows_kernel<Qv, TOv, true, true, false>);
          else if (MK) launch(linear_glds_rows_kernel<Qv, TOv, true, false, false>);
          else if (AD) launch(linear_glds_rows_kernel<Qv, TOv, false, true, false>);
          else launch(linear_glds_rows_kernel<Qv, TOv, false, false, false>);
        }
      };
      using I2 = std::integral_constant<int, 2>;
      using I4 = std::integral_constant<int, 4>;
      using I8 = std::integral_constant<int, 8>;
      auto pt = [&](auto q) {  // TO x Q <= 32 (the weight's VGPRs)
        if (TO == 2) pe(q, I2{});
        else if (TO == 4) pe(q, I4{});
        else if constexpr (decltype(q)::value <= 4) pe(q, I8{});
      };
      if (Cin == 32) pt(I2{}); else if (Cin == 64) pt(I4{}); else pt(I8{});
      PK_CHECK_LAUNCH();
      return PK_OK;
    }
    auto kern = plain ? pickq(std::integral_constant<bool, false>{}) : pickq(std::integral_constant<bool, true>{});
    const size_t lds = sizeof(float) * (size_t)(16 * TO) * (Cin + 4);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), lds, st, x, sx, w, bias, R, Cin, Cout, transw, e);
    PK_CHECK_LAUNCH();
    return PK_OK;
  }
  if (layout == 1 && (Cin == 16 || Cin == 32 || Cin == 64 || Cin == 128) && N > 0) {
    PK_REQUIRE(e.y2 == nullptr && !e.store_cf);
    const int sub = cf_sub(R, N, Cin, sx, e);
    const int TO = Cout <= 16 ? 1 : Cout <= 32 ? 2 : Cout <= 64 ? 4 : 8;
    auto pick = [&](auto q, auto u) {
      constexpr int Q = decltype(q)::value, U = decltype(u)::value;
      return TO == 1 ? linear_fwd_cf_kernel<Q, 1, U>
             : TO == 2 ? linear_fwd_cf_kernel<Q, 2, U>
             : TO == 4 ? linear_fwd_cf_kernel<Q, 4, U> : linear_fwd_cf_kernel<Q, 8, U>;
    };
    auto pickq = [&](auto u) {
      return Cin == 16 ? pick(std::integral_constant<int, 1>{}, u)
             : Cin == 32 ? pick(std::integral_constant<int, 2>{}, u)
             : Cin == 64 ? pick(std::integral_constant<int, 4>{}, u) : pick(std::integral_constant<int, 8>{}, u);
    };
    auto kern = sub == 4 ? pickq(std::integral_constant<int, 4>{})
                : sub == 2 ? pickq(std::integral_constant<int, 2>{}) : pickq(std::integral_constant<int, 1>{});
    const int64_t tpc = (N + 16 * sub - 1) / (16 * sub);
    const int64_t tiles = (R / N) * tpc;
    const size_t lds = sizeof(float) * (size_t)(16 * TO) * (Cin + 4);
    hipLaunchKernelGGL(kern, dim3((unsigned)((tiles + 3) / 4)), dim3(256), lds, st, x, sx, w, bias, R, N, Cout,
                       transw, e, tpc);
    PK_CHECK_LAUNCH();
    return PK_OK;
  }
  // generic fallback kernel: contiguous operands only
  PK_REQUIRE(plain_out && sx == (layout == 0 ? Cin : (int64_t)Cin * N) &&
             e.sy == (layout == 0 ? Cout : (int64_t)Cout * N));
  const unsigned blocks = (unsigned)((R + 127) / 128);
  const size_t lds = sizeof(float) * (size_t)Cout * (((Cin + 3) & ~3) + 1);
  if (layout == 0)
    hipLaunchKernelGGL(linear_fwd_kernel<0>, dim3(blocks), dim3(256), lds, st, x, w, bias, R, N, Cin, Cout, transw,
                       e.relu, e.mask, e.y);
  else
    hipLaunchKernelGGL(linear_fwd_kernel<1>, dim3(blocks), dim3(256), lds, st, x, w, bias, R, N, Cin, Cout, transw,
                       e.relu, e.mask, e.y);
  PK_CHECK_LAUNCH();
  return PK_OK;
}

extern "C" int pk_linear_fwd(const float* x, const float* w, const float* bias, int layout, int64_t R, int N,
                             int Cin, int Cout, int transw, int relu, const float* mask, float* y, void* stream) {
  pk_linear_args a{};
  a.x = x;
  a.w = w;
  a.bias = bias;
  a.layout = layout;
  a.R = R;
  a.N = N;
  a.Cin = Cin;
  a.Cout = Cout;
  a.transw = transw;
  a.act = relu ? 1 : 0;
  a.mask = mask;
  a.y = y;
  a.pre = nullptr;
  a.pre_out = nullptr;
  return pk_linear_ex(&a, stream);
}
