// ZoomOut spectral refinement of the functional map (Melzi et al. 2019, "ZoomOut: Spectral
// Upsampling for Efficient Shape Correspondence"; pyFM's zoomout_refine), in the convention of
// fmap2pointmap_solvers/naive.py:6-34: X the CAD (n1 points), Y the crop (n2 points),
//     p[j] = argmin_i || (Phi_x[:, :k] C^T)[i] - Phi_y[j, :k] ||.
// The reference repository has no ZoomOut: a build-defined addition, off by default.
//
// With k = 30 at the start:
//   1. E = Phi_x[:n1, :k] C^T;  p[j] = argmin_{i < n1} (|E_i|^2 - 2 E_i . Phi_y[j, :k]), ties lowest i
//   2. k == k_final: stop; else k <- min(k + step, k_final)
//   3. C[a, b] = sum_{j < n2} mass_y[j] Phi_y[j, a] Phi_x[p[j], b]  (a, b < k), go to 1.
//
// Launches of one call (the schedule is a host function of (k_final, step) only):
//   zo_ylayout_kernel   once: Phi_y's 64 columns in MFMA operand-tile order (rows >= n2 and columns
//                       past the operand's width as zeros); p[j] = 0 for j >= n2
//   per iteration
//   zo_embed_kernel     a wave per 16-row tile of X: -2 E on the f32 MFMA (C x^T with C's rows permuted so
//                       that the accumulators are the operand tile's chunks; C staged zero-padded in LDS,
//                       so columns >= k come out as zeros), and |E_i|^2 (+inf for rows >= n1: they
//                       never win)
//   zo_nn_kernel<S>     S = ceil(k / 4) steps of v_mfma_f32_16x16x4_f32 per 16 x 16 tile, the
//                       accumulator started at |E_i|^2, so a tile comes out as the scores themselves;
//                       a running (score, tile) per lane stream (strict <: the earliest row stays);
//                       block = crop x 64 columns x row part, 4 waves splitting the part's row tiles,
//                       meeting in LDS as (ordered score bits, row) keys. RS > 1 (small batches): the
//                       parts' keys go to scratch and zo_nn_merge_kernel takes the minimum key. The
//                       [V1, V2] matrix never exists.
//   zo_project_kernel   a block per 64-row slab of j: m_j Phi_y[j, :] and the gathered Phi_x[p_j, :]
//                       staged in LDS, a 4 x 4 patch of the 64 x 64 product per thread (fmaf over j in
//                       order), the slab's partial to scratch
//   zo_reduce_kernel    the slabs holding rows < n2 summed in slab order -> C [k, k]
// Nothing is kept in scratch across calls and nothing in it is read before this call writes it; no
// atomics, no arrival counters; a crop's result does not depend on the batch around it (the row
// split RS does, but the argmin under the full tie rule does not depend on the split).
//
// Operand-tile order (both operands, K = 64): tile = 16 rows; lane (g, c) = (lane >> 4, lane & 15)
// holds row c's values at contraction index 4 s + g of step s; steps 4 q .. 4 q + 3 form chunk q,
// one float4 per lane at float4 index (tile * 4 + q) * 64 + lane (4 KB per tile, 16-B loads).
#include <algorithm>

#include "common.hpp"
#include "mfma_tile.hpp"

namespace {

using pk::f32x4;

constexpr int kK0 = 30;      // n_fmap: the size of C0
constexpr int kKmax = 64;    // eigenvectors held per shape
constexpr int kCT = 4;       // column tiles per block (and per wave) of the nearest-neighbour pass
constexpr int kNNWaves = 4;
constexpr int kSlab = 64;    // rows of j per projection block
constexpr int kCP = kKmax + 4;  // LDS row pitch of the staged C (the embed's 64 lanes on 64 distinct banks)

using pk::al256;

// a crop's valid rows: the caller's count held to [0, the padded length]
__device__ __forceinline__ int zo_count(int n, int vmax) { return max(0, min(n, vmax)); }

// grid (ceil(T2 / 4), B), 256 threads: a wave per 16-row tile of Y
__global__ __launch_bounds__(256) void zo_ylayout_kernel(const float* __restrict__ ey, int ldy, int ky,
                                                         const int32_t* __restrict__ n2, int V2max, int T2,
                                                         f32x4* __restrict__ Yt, int64_t* __restrict__ p) {
  const int b = blockIdx.y;
  const int lane = pk::lane_id(), g = lane >> 4, c16 = lane & 15;
  const int tile = blockIdx.x * 4 + pk::wave_id();
  if (tile >= T2) return;
  const int N2 = zo_count(n2[b], V2max);
  const int r = tile * 16 + c16;
  if (g == 0 && r >= N2 && r < V2max) p[(int64_t)b * V2max + r] = 0;
  if (tile * 16 >= N2) return;  // never read by the main pass
  const bool valid = r < N2;
  const float* rowp = ey + ((int64_t)b * V2max + min(r, V2max - 1)) * ldy;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    f32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = 16 * q + 4 * i + g;
      const float x = rowp[min(k, ky - 1)];
      v[i] = (valid && k < ky) ? x : 0.f;
    }
    Yt[(((int64_t)b * T2 + tile) * 4 + q) * 64 + lane] = v;
  }
}

// grid (ceil(T1 / 4), B), 256 threads: a wave per 16-row tile of X. C [k, k] with row stride ldc.
__global__ __launch_bounds__(256) void zo_embed_kernel(const float* __restrict__ ex, int ldx,
                                                       const float* __restrict__ C, int ldc, int64_t cstride,
                                                       int k, const int32_t* __restrict__ n1, int V1max, int T1,
                                                       f32x4* __restrict__ At, float* __restrict__ nA) {
  __shared__ __attribute__((aligned(16))) float sC[kKmax * kCP];
  const int b = blockIdx.y;
  const int N1 = zo_count(n1[b], V1max);
  if (blockIdx.x * 64 >= N1) return;  // (block-uniform) tiles past the valid rows are never read
  const float* Cb = C + (int64_t)b * cstride;
  for (int e = threadIdx.x; e < kKmax * kKmax; e += 256) {
    const int a = e >> 6, bb = e & 63;
    sC[a * kCP + bb] = (a < k && bb < k) ? Cb[(int64_t)a * ldc + bb] : 0.f;
  }
  __syncthreads();
  const int lane = pk::lane_id(), g = lane >> 4, c16 = lane & 15;
  const int tile = blockIdx.x * 4 + pk::wave_id();
  if (tile >= T1 || tile * 16 >= N1) return;
  const int r = tile * 16 + c16;
  const bool valid = r < N1;
  const float* rowp = ex + ((int64_t)b * V1max + min(r, V1max - 1)) * ldx;
  // B operand: x[row c][4 t + g] of contraction step t (0 past column k and for rows >= n1)
  float xv[kKmax / 4];
#pragma unroll
  for (int t = 0; t < kKmax / 4; ++t) {
    const int bb = 4 * t + g;
    const float x = rowp[min(bb, k - 1)];
    xv[t] = (valid && bb < k) ? x : 0.f;
  }
  const int nt = (k + 3) >> 2;  // contraction steps holding a non-zero C column
  // D = C x^T per block n of 16 features, with C's rows permuted: A-operand row i = c is C row
  // 16 n + 4 (c & 3) + (c >> 2), so register q of lane group g (D row 4 g + q, column = point c) is
  // feature 16 n + 4 q + g = 4 s + g of step s = 4 n + q: the accumulator IS chunk n of the operand
  // tile. (An f32 MFMA accumulates as the fmaf chain over b in order.) Row pitch kCP = 68: the 64
  // lanes' reads fall on 64 distinct banks.
  const float* crow = sC + (4 * (c16 & 3) + (c16 >> 2)) * kCP + g;
  float part = 0.f;
  f32x4* dst = At + ((int64_t)b * T1 + tile) * 256 + lane;
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (16 * n < k) {
#pragma unroll
      for (int t = 0; t < kKmax / 4; ++t)
        if (t < nt) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(crow[16 * n * kCP + 4 * t], xv[t], acc, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) part = fmaf(acc[q], acc[q], part);
    dst[n * 64] = f32x4{-2.f * acc[0], -2.f * acc[1], -2.f * acc[2], -2.f * acc[3]};
  }
  // |E_i|^2: the row's four lane groups in the order 0, 1, 2, 3
  const float p1 = __shfl_xor(part, 16), p2 = __shfl_xor(part, 32), p3 = __shfl_xor(part, 48);
  const float mine[4] = {part, p1, p2, p3};  // lane group g, g^1, g^2, g^3
  float nrm = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) nrm += mine[q ^ g];
  if (g == 0) nA[((int64_t)b * T1 + tile) * 16 + c16] = valid ? nrm : __builtin_huge_valf();
}

// (ordered score bits, row) as one unsigned key: the smallest key is the smallest score, then the
// lowest row. -0 is folded into +0 first (they compare equal as floats).
__device__ __forceinline__ unsigned long long zo_key(float v, unsigned row) {
  return ((unsigned long long)pk::f32_ordered(v + 0.f) << 32) | row;
}

constexpr unsigned kNoRow = 0x7fffffffu;

// grid (NCG * RS, B), 256 threads. Block (cg, rs): columns [64 cg, 64 cg + 64) of crop b, row part
// rs; wave w takes the row tiles of share rs * 4 + w of RS * 4.
template <int S>
__global__ __launch_bounds__(64 * kNNWaves) void zo_nn_kernel(const f32x4* __restrict__ At,
                                                              const float* __restrict__ nA,
                                                              const f32x4* __restrict__ Yt,
                                                              const int32_t* __restrict__ n1,
                                                              const int32_t* __restrict__ n2, int V1max, int V2max,
                                                              int T1, int T2, int NCG, int RS,
                                                              int64_t* __restrict__ p,
                                                              unsigned long long* __restrict__ part) {
  constexpr int NQ = (S + 3) / 4;
  __shared__ unsigned long long wkeys[kNNWaves][kCT * 16];
  const int b = blockIdx.y;
  const int cg = blockIdx.x % NCG, rs = blockIdx.x / NCG;
  const int N1 = zo_count(n1[b], V1max), N2 = zo_count(n2[b], V2max);
  const int j0 = cg * kCT * 16;
  if (j0 >= N2) return;  // (block-uniform, before the barrier)
  const int lane = pk::lane_id(), g = lane >> 4, c16 = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(pk::wave_id());
  const int nt = (N1 + 15) >> 4, ntY = (N2 + 15) >> 4;
  const int Q = RS * kNNWaves, qw = rs * kNNWaves + w;
  const int tb = (int)((int64_t)nt * qw / Q), te = (int)((int64_t)nt * (qw + 1) / Q);
  // the wave's column operands (a column tile past the crop's last re-reads the last: not written)
  f32x4 bo[kCT][NQ];
#pragma unroll
  for (int c = 0; c < kCT; ++c) {
    const int ct = min(cg * kCT + c, ntY - 1);
#pragma unroll
    for (int q = 0; q < NQ; ++q) bo[c][q] = Yt[(((int64_t)b * T2 + ct) * 4 + q) * 64 + lane];
  }
  float bv[kCT][4];
  int bt[kCT][4];
#pragma unroll
  for (int c = 0; c < kCT; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      bv[c][r] = __builtin_huge_valf();
      bt[c][r] = -1;
    }
  const f32x4* Ab = At + (int64_t)b * T1 * 256 + lane;
  const float* nb = nA + (int64_t)b * T1 * 16 + 4 * g;
  if (tb < te) {
    f32x4 an[NQ], nn;
#pragma unroll
    for (int q = 0; q < NQ; ++q) an[q] = Ab[(int64_t)tb * 256 + q * 64];
    nn = *reinterpret_cast<const f32x4*>(nb + (int64_t)tb * 16);
    for (int t = tb; t < te; ++t) {
      f32x4 ac[NQ], acc[kCT];
#pragma unroll
      for (int q = 0; q < NQ; ++q) ac[q] = an[q];
#pragma unroll
      for (int c = 0; c < kCT; ++c) acc[c] = nn;
      const int tn = min(t + 1, te - 1);  // the next tile's operand, in flight across this tile's MFMAs
#pragma unroll
      for (int q = 0; q < NQ; ++q) an[q] = Ab[(int64_t)tn * 256 + q * 64];
      nn = *reinterpret_cast<const f32x4*>(nb + (int64_t)tn * 16);
#pragma unroll
      for (int s = 0; s < S; ++s)
#pragma unroll
        for (int c = 0; c < kCT; ++c)  // four independent accumulation chains
          acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[s >> 2][s & 3], bo[c][s >> 2][s & 3], acc[c], 0, 0, 0);
#pragma unroll
      for (int c = 0; c < kCT; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool lt = acc[c][r] < bv[c][r];
          bv[c][r] = lt ? acc[c][r] : bv[c][r];
          bt[c][r] = lt ? t : bt[c][r];
        }
    }
  }
  // per column: the lane's four row offsets, the four lane groups, then the waves through LDS
#pragma unroll
  for (int c = 0; c < kCT; ++c) {
    unsigned long long key = ~0ull;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const unsigned row = bt[c][r] < 0 ? kNoRow : (unsigned)(bt[c][r] * 16 + 4 * g + r);
      const unsigned long long kr = zo_key(bv[c][r], row);
      key = kr < key ? kr : key;
    }
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      const unsigned long long o = __shfl_xor(key, off);
      key = o < key ? o : key;
    }
    if (g == 0) wkeys[w][c * 16 + c16] = key;
  }
  __syncthreads();
  if (threadIdx.x < kCT * 16) {
    const int j = j0 + threadIdx.x;
    if (j < N2) {
      unsigned long long best = wkeys[0][threadIdx.x];
#pragma unroll
      for (int v = 1; v < kNNWaves; ++v) best = wkeys[v][threadIdx.x] < best ? wkeys[v][threadIdx.x] : best;
      if (RS == 1) {
        const unsigned row = (unsigned)(best & 0xffffffffu);
        p[(int64_t)b * V2max + j] = row >= (unsigned)N1 ? 0 : (int64_t)row;
      } else {
        part[((int64_t)b * RS + rs) * V2max + j] = best;
      }
    }
  }
}

// RS > 1: grid (ceil(V2max / 256), B): the smallest of each column's RS row-part keys
__global__ __launch_bounds__(256) void zo_nn_merge_kernel(const unsigned long long* __restrict__ part,
                                                          const int32_t* __restrict__ n1,
                                                          const int32_t* __restrict__ n2, int V1max, int V2max,
                                                          int RS, int64_t* __restrict__ p) {
  const int b = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= zo_count(n2[b], V2max)) return;
  unsigned long long best = ~0ull;
  for (int r = 0; r < RS; ++r) {
    const unsigned long long key = part[((int64_t)b * RS + r) * V2max + j];
    best = key < best ? key : best;
  }
  const unsigned row = (unsigned)(best & 0xffffffffu);
  p[(int64_t)b * V2max + j] = row >= (unsigned)zo_count(n1[b], V1max) ? 0 : (int64_t)row;
}

// grid (NSL, B), 256 threads: slab sl = rows [64 sl, 64 sl + 64) of j. Thread (ta, tb) = (tid >> 4,
// tid & 15) owns C[4 ta .. + 3][4 tb .. + 3] of the slab's partial product.
__global__ __launch_bounds__(256) void zo_project_kernel(const float* __restrict__ ex, int ldx, int kx,
                                                         const float* __restrict__ ey, int ldy, int ky,
                                                         const float* __restrict__ mass,
                                                         const int64_t* __restrict__ p,
                                                         const int32_t* __restrict__ n2, int V1max, int V2max,
                                                         int NSL, float* __restrict__ partC) {
  __shared__ __attribute__((aligned(16))) float sY[kSlab][kKmax];
  __shared__ __attribute__((aligned(16))) float sX[kSlab][kKmax];
  const int b = blockIdx.y, sl = blockIdx.x;
  const int N2 = zo_count(n2[b], V2max);
  const int jb = sl * kSlab;
  if (jb >= N2) return;  // (block-uniform) the reduction reads only the slabs holding rows < n2
  const int tid = threadIdx.x;
#pragma unroll 4
  for (int i = 0; i < kSlab * kKmax / 256; ++i) {
    const int e = tid + 256 * i, jj = e >> 6, col = e & 63;
    const int j = jb + jj;
    const bool ok = j < N2;
    const int jc = ok ? j : jb;
    const float m = mass[(int64_t)b * V2max + jc];
    const float y = ey[((int64_t)b * V2max + jc) * ldy + min(col, ky - 1)];
    int64_t pi = p[(int64_t)b * V2max + jc];
    pi = pi < 0 ? 0 : pi > V1max - 1 ? V1max - 1 : pi;
    const float x = ex[((int64_t)b * V1max + pi) * ldx + min(col, kx - 1)];
    sY[jj][col] = (ok && col < ky) ? m * y : 0.f;
    sX[jj][col] = (ok && col < kx) ? x : 0.f;
  }
  __syncthreads();
  const int ta = tid >> 4, tb = tid & 15;
  const int nj = min(kSlab, N2 - jb);
  float acc[4][4] = {};
  for (int jj = 0; jj < nj; ++jj) {
    const f32x4 ya = *reinterpret_cast<const f32x4*>(&sY[jj][4 * ta]);
    const f32x4 xb = *reinterpret_cast<const f32x4*>(&sX[jj][4 * tb]);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[a][c] = fmaf(ya[a], xb[c], acc[a][c]);
  }
  float* dst = partC + ((int64_t)b * NSL + sl) * kKmax * kKmax;
#pragma unroll
  for (int a = 0; a < 4; ++a)
    *reinterpret_cast<f32x4*>(dst + (4 * ta + a) * kKmax + 4 * tb) = f32x4{acc[a][0], acc[a][1], acc[a][2], acc[a][3]};
}

// grid (16, B), 256 threads: element (a, b) of the 64 x 64 product, its slabs in slab order
__global__ __launch_bounds__(256) void zo_reduce_kernel(const float* __restrict__ partC,
                                                        const int32_t* __restrict__ n2, int V2max, int NSL,
                                                        int k, float* __restrict__ C, int ldc, int64_t cstride) {
  const int b = blockIdx.y;
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int a = e >> 6, bb = e & 63;
  if (a >= k || bb >= k) return;
  const int nsl = (zo_count(n2[b], V2max) + kSlab - 1) / kSlab;
  float s = 0.f;
  for (int sl = 0; sl < nsl; ++sl) s += partC[((int64_t)b * NSL + sl) * kKmax * kKmax + e];
  C[(int64_t)b * cstride + (int64_t)a * ldc + bb] = s;
}

// k_final == 30: the map handed back is C0 itself
__global__ __launch_bounds__(256) void zo_copy_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                      int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

struct ZoPlan {
  int T1, T2, NCG, RS, NSL;
  int64_t a_bytes, na_bytes, y_bytes, c_bytes, pc_bytes, key_bytes;
  int64_t total() const { return a_bytes + na_bytes + y_bytes + c_bytes + pc_bytes + key_bytes; }
};

inline ZoPlan zo_plan(int B, int V1max, int V2max) {
  ZoPlan z{};
  z.T1 = (V1max + 15) / 16;
  z.T2 = (V2max + 15) / 16;
  z.NCG = (z.T2 + kCT - 1) / kCT;
  z.NSL = (V2max + kSlab - 1) / kSlab;
  const int64_t blocks = std::max<int64_t>(1, (int64_t)B * z.NCG);
  const int rs = blocks >= 512 ? 1 : (int)((512 + blocks - 1) / blocks);
  z.RS = std::min(rs, std::max(1, z.T1 / (2 * kNNWaves)));  // at least two row tiles per wave
  z.a_bytes = al256((int64_t)B * z.T1 * 4096);
  z.na_bytes = al256((int64_t)B * z.T1 * 16 * 4);
  z.y_bytes = al256((int64_t)B * z.T2 * 4096);
  z.c_bytes = al256((int64_t)B * kKmax * kKmax * 4);
  z.pc_bytes = al256((int64_t)B * z.NSL * kKmax * kKmax * 4);
  z.key_bytes = z.RS > 1 ? al256((int64_t)B * z.RS * V2max * 8) : 0;
  return z;
}

inline bool zo_args_ok(int B, int V1max, int V2max, int k_final, int step) {
  return B >= 0 && V1max >= 0 && V2max >= 0 && k_final >= kK0 && k_final <= kKmax && step >= 1 &&
         (int64_t)B * std::max(V1max, V2max) < ((int64_t)1 << 31) && B <= 65535;
}

template <int S>
void zo_nn_launch(dim3 grid, hipStream_t s, const f32x4* At, const float* nA, const f32x4* Yt, const int32_t* n1,
                  const int32_t* n2, int V1max, int V2max, const ZoPlan& z, int64_t* p, unsigned long long* part) {
  hipLaunchKernelGGL(zo_nn_kernel<S>, grid, dim3(64 * kNNWaves), 0, s, At, nA, Yt, n1, n2, V1max, V2max, z.T1, z.T2,
                     z.NCG, z.RS, p, part);
}

}  // namespace

extern "C" int64_t pk_zoomout_work_size(int B, int V1max, int V2max, int k_final, int step) {
  if (!zo_args_ok(B, V1max, V2max, k_final, step)) return -1;
  return zo_plan(B, V1max, V2max).total();
}

extern "C" int pk_zoomout(const float* evecs_x, int ldx, const float* evecs_y, int ldy, const float* mass_y,
                          const float* C0, const int32_t* n1, const int32_t* n2, int B, int V1max, int V2max,
                          int k_final, int step, void* work, int64_t work_bytes, float* C_out, int64_t* p2p,
                          void* stream) {
  PK_REQUIRE(zo_args_ok(B, V1max, V2max, k_final, step));
  PK_REQUIRE(ldx >= k_final && ldy >= k_final);
  if (B == 0) return PK_OK;
  PK_REQUIRE(C0 && C_out && n1 && n2);
  hipStream_t s = pk::as_stream(stream);
  const int64_t csz = (int64_t)k_final * k_final;
  if (V1max == 0 || V2max == 0) {  // no crop point or no CAD row: C0 stands when k_final = 30, else C = 0
    if (k_final == kK0) {
      hipLaunchKernelGGL(zo_copy_kernel, dim3((unsigned)((B * csz + 255) / 256)), dim3(256), 0, s, C0, C_out, B * csz);
      PK_CHECK_LAUNCH();
    } else {
      const hipError_t e = pk::zero_async(C_out, (size_t)(B * csz) * 4, s);
      if (e != hipSuccess) return (int)e;
    }
    if (V2max > 0) {
      PK_REQUIRE(p2p);
      const hipError_t e = pk::zero_async(p2p, (size_t)B * V2max * 8, s);
      if (e != hipSuccess) return (int)e;
    }
    return PK_OK;
  }
  PK_REQUIRE(evecs_x && evecs_y && mass_y && p2p);
  const ZoPlan z = zo_plan(B, V1max, V2max);
  PK_REQUIRE(work && work_bytes >= z.total());
  char* wp = static_cast<char*>(work);
  auto* At = reinterpret_cast<f32x4*>(wp);
  auto* nA = reinterpret_cast<float*>(wp + z.a_bytes);
  auto* Yt = reinterpret_cast<f32x4*>(wp + z.a_bytes + z.na_bytes);
  auto* Cw = reinterpret_cast<float*>(wp + z.a_bytes + z.na_bytes + z.y_bytes);
  auto* Pc = reinterpret_cast<float*>(wp + z.a_bytes + z.na_bytes + z.y_bytes + z.c_bytes);
  auto* keys = z.RS > 1 ? reinterpret_cast<unsigned long long*>(wp + z.a_bytes + z.na_bytes + z.y_bytes +
                                                                  z.c_bytes + z.pc_bytes)
                        : nullptr;
  const int kx = std::min(ldx, kKmax), ky = std::min(ldy, kKmax);
  hipLaunchKernelGGL(zo_ylayout_kernel, dim3((z.T2 + 3) / 4, B), dim3(256), 0, s, evecs_y, ldy, ky, n2, V2max, z.T2,
                     Yt, p2p);
  PK_CHECK_LAUNCH();
  if (k_final == kK0) {
    hipLaunchKernelGGL(zo_copy_kernel, dim3((unsigned)((B * csz + 255) / 256)), dim3(256), 0, s, C0, C_out, B * csz);
    PK_CHECK_LAUNCH();
  }
  const float* Ccur = C0;
  int ldc = kK0;
  int64_t cstride = (int64_t)kK0 * kK0;
  const dim3 nn_grid((unsigned)(z.NCG * z.RS), B);
  for (int k = kK0;;) {
    hipLaunchKernelGGL(zo_embed_kernel, dim3((z.T1 + 3) / 4, B), dim3(256), 0, s, evecs_x, ldx, Ccur, ldc, cstride, k,
                       n1, V1max, z.T1, At, nA);
    PK_CHECK_LAUNCH();
    switch ((k + 3) / 4) {
#define PK_ZO_NN(S_) \
  case S_: zo_nn_launch<S_>(nn_grid, s, At, nA, Yt, n1, n2, V1max, V2max, z, p2p, keys); break;
      PK_ZO_NN(8) PK_ZO_NN(9) PK_ZO_NN(10) PK_ZO_NN(11) PK_ZO_NN(12) PK_ZO_NN(13) PK_ZO_NN(14) PK_ZO_NN(15)
      PK_ZO_NN(16)
#undef PK_ZO_NN
      default: return PK_ERR_ARG;
    }
    PK_CHECK_LAUNCH();
    if (z.RS > 1) {
      hipLaunchKernelGGL(zo_nn_merge_kernel, dim3((V2max + 255) / 256, B), dim3(256), 0, s, keys, n1, n2, V1max, V2max,
                         z.RS, p2p);
      PK_CHECK_LAUNCH();
    }
    if (k == k_final) break;
    k = step >= k_final - k ? k_final : k + step;
    hipLaunchKernelGGL(zo_project_kernel, dim3(z.NSL, B), dim3(256), 0, s, evecs_x, ldx, kx, evecs_y, ldy, ky, mass_y,
                       p2p, n2, V1max, V2max, z.NSL, Pc);
    PK_CHECK_LAUNCH();
    float* Cnext = k == k_final ? C_out : Cw;
    ldc = k == k_final ? k_final : kKmax;
    cstride = k == k_final ? csz : (int64_t)kKmax * kKmax;
    hipLaunchKernelGGL(zo_reduce_kernel, dim3(16, B), dim3(256), 0, s, Pc, n2, V2max, z.NSL, k, Cnext, ldc, cstride);
    PK_CHECK_LAUNCH();
    Ccur = Cnext;
  }
  return PK_OK;
}
