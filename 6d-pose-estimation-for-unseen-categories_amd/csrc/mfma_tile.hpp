// What more than one MFMA unit uses. The vector aliases, the points-per-lane trait and the
// alignment checks serve every unit that includes this header; the rest is the tile toolkit of the
// per-point layer units (linear_fwd.hip, linear_wgrad.hip, mlp_chain.hip): weight staging and
// fragments for v_mfma_f32_16x16x4f32 with the contraction index k = 16 q + 4 g + i at step (q, i)
// on lane group g, the LDS-DMA (global_load_lds) tile images with their source-side XOR swizzle,
// and the ring depth and counted wait of a ring of such tiles (the design of the ring is written
// up at linear_glds_rows_kernel). In the style of common.hpp: __device__ __forceinline__
// templates, one copy per translation unit.
#pragma once
#include "common.hpp"

namespace pk {

using f32x2 = __attribute__((ext_vector_type(2))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;

// SUB consecutive points of one channel held by a lane of the channels-first kernels (16 SUB points
// per wave tile: linear_cf_body, attn_mlp.hip)
template <int SUB> struct PtVec;
template <> struct PtVec<1> { using T = float; };
template <> struct PtVec<2> { using T = f32x2; };
template <> struct PtVec<4> { using T = f32x4; };

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool al8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

constexpr int kRowsPersistCUs = 256;  // persistent rows grid: 2 blocks per CU of MI355X

// Ring depth of the LDS-DMA rows pipelines (linear_glds_rows_kernel, the block-MLP chains): 3 slots
// per wave when 4 waves x 3 slots of slot_floats fit the CU's LDS, else 2. The kernel sizes its
// ring and its counted wait with it, the host launcher its dynamic LDS.
__host__ __device__ constexpr int ring_depth(int slot_floats) { return 3 * 4 * slot_floats * 4 <= 159 * 1024 ? 3 : 2; }

// s_waitcnt vmcnt(N), expcnt / lgkmcnt untouched (N > 63 waits for 63, the counter's range)
template <int N>
__device__ __forceinline__ void vm_wait() {
  constexpr int n = N < 63 ? N : 63;
  __builtin_amdgcn_s_waitcnt((n & 15) | ((n >> 4) << 14) | (7 << 4) | (15 << 8));
}

// B operands of one 16-point tile of a rows-layout input (row stride sx, 16 Q channels): lane
// (m = point, g) takes the float4s 16 q + 4 g .. + 3 of its own point row, i.e. contraction index
// k = 16 q + 4 g + i at step (q, i); a row >= R reads as 0
template <int Q>
__device__ __forceinline__ void lr_load(const float* __restrict__ x, int64_t sx, int64_t row, int64_t R, int g,
                                        f32x4 (&xa)[Q]) {
#pragma unroll
  for (int q = 0; q < Q; ++q)
    xa[q] = row < R ? *reinterpret_cast<const f32x4*>(x + row * sx + 16 * q + 4 * g) : f32x4{0.f, 0.f, 0.f, 0.f};
}

// Weight staging shared by the MFMA per-point kernels: Ws[o][k] (o < 16 TO, zero rows past
// Cout; row stride 16 Q + 4), from W [Cout, 16 Q] or, with transw, from W^T's [16 Q, Cout].
// w2 / wsplit: stored weight rows >= wsplit come from w2 (row - wsplit) — two layers' weights
// stacked without a concatenation kernel (transw = 0: rows = outputs; transw = 1: rows = the
// stored [Cin, Cout] tensor's rows); w2 == nullptr: every row from w.
template <int Q, int TO>
__device__ __forceinline__ void lr_stage(const float* w, int Cout, int transw, float* Ws, const float* w2,
                                         int wsplit) {  // callers without a second weight pass w2 = w
                                                        // (arithmetic on a null w2 crashed clang-22's inliner)
  constexpr int CI = 16 * Q, ST = CI + 4;
  if (!transw) {  // W [Cout, CI] rows: float4 reads, all issued before the LDS writes
    constexpr int NV = TO * 16 * CI / 4, PER = (NV + 255) / 256;
    f32x4 v[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = threadIdx.x + 256 * i, o = e / (CI / 4);
      const float* src = o < wsplit ? w + 4 * (int64_t)e : w2 + 4 * (int64_t)(e - wsplit * (CI / 4));
      v[i] = (e < NV && o < Cout) ? *reinterpret_cast<const f32x4*>(src) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = threadIdx.x + 256 * i, o = e / (CI / 4), k4 = e - o * (CI / 4);
      if (e < NV) *reinterpret_cast<f32x4*>(&Ws[o * ST + 4 * k4]) = v[i];
    }
  } else {  // W^T from a [CI, Cout] tensor: read along Cout
    constexpr int NE = TO * 16 * CI, PER = (NE + 255) / 256;
    float v[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = threadIdx.x + 256 * i, k = e / (TO * 16), o = e - k * (TO * 16);
      const float* src = k < wsplit ? w + (int64_t)k * Cout + o : w2 + (int64_t)(k - wsplit) * Cout + o;
      v[i] = (e < NE && o < Cout) ? *src : 0.f;
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = threadIdx.x + 256 * i, k = e / (TO * 16), o = e - k * (TO * 16);
      if (e < NE) Ws[o * ST + k] = v[i];
    }
  }
}

// 16 rows x CW floats (row stride ld, columns >= cols_ok read at column 0 of the row: valid
// memory, masked at use) into an LDS region of 16 x CW floats, chunk (row, c) at position
// row * CW / 4 + (c ^ (row & (CW / 4 - 1) & 15)): CW / 16 glds per wave
template <int CW>
__device__ __forceinline__ void glds_rows(const float* __restrict__ src, int64_t ld, int64_t row0, int64_t R,
                                          int cols_ok, float* lds_dst, int lane) {
  constexpr int CPR = CW / 4, NI = CW / 16;
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int p = j * 64 + lane;
    const int row = p / CPR, cl = p % CPR;
    const int c = cl ^ (row & (CPR - 1) & 15);
    const int64_t gr = min(row0 + row, R - 1);
    const int col = 4 * c < cols_ok ? 4 * c : 0;
    __builtin_amdgcn_global_load_lds(src + gr * ld + col, (__attribute__((address_space(3))) void*)(lds_dst + j * 256),
                                     16, 0, 0);
  }
}

template <int CW>
__device__ __forceinline__ f32x4 lds_chunk(const float* region, int row, int c) {
  constexpr int CPR = CW / 4;
  return *reinterpret_cast<const f32x4*>(region + 4 * (row * CPR + (c ^ (row & (CPR - 1) & 15))));
}

// Per-lane float offsets of the 16-B chunks of a glds_rows<CW> image within one 16-row block (row
// stride ld, columns >= cols_ok at column 0), computed once: a tile whose 16 rows are all in range
// is then issued from a scalar base (glds_issue16) without per-lane 64-bit address arithmetic,
// which on gfx950 would be VALU work serialised with the f32 MFMAs.
template <int CW>
__device__ __forceinline__ void glds_rows_off(int64_t ld, int cols_ok, int lane, int (&off)[CW / 16]) {
  constexpr int CPR = CW / 4;
#pragma unroll
  for (int j = 0; j < CW / 16; ++j) {
    const int p = j * 64 + lane;
    const int row = p / CPR, cl = p % CPR;
    const int c = cl ^ (row & (CPR - 1) & 15);
    off[j] = (int)(row * ld) + (4 * c < cols_ok ? 4 * c : 0);
  }
}

// the same for a glds_cf<C> image: chunk (c, pos) holds floats 4 (pos ^ ((c >> 2) & 3)) .. + 3
// of channel c (channel stride N)
template <int C>
__device__ __forceinline__ void glds_cf_off(int N, int lane, int (&off)[C / 16]) {
#pragma unroll
  for (int j = 0; j < C / 16; ++j) {
    const int p = j * 64 + lane;
    const int c = p >> 2, pos = p & 3;
    off[j] = c * N + 4 * (pos ^ ((c >> 2) & 3));
  }
}

template <int NI, int BYTES>
__device__ __forceinline__ void glds_issue(const float* base, const int* off, float* lds_dst) {  // off[NI]
  static_assert(BYTES == 16 || BYTES == 4, "glds piece");
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    auto* d = (__attribute__((address_space(3))) void*)(lds_dst + j * BYTES * 16);
    if constexpr (BYTES == 16) __builtin_amdgcn_global_load_lds(base + off[j], d, 16, 0, 0);
    else __builtin_amdgcn_global_load_lds(base + off[j], d, 4, 0, 0);
  }
}

template <int Q, int TO>  // fragments of Ws[o][k] (lr_stage image, row stride 16 Q + 4)
__device__ __forceinline__ void chain_wfrag(const float* Ws, int m, int g, f32x4 (&wf)[TO][Q]) {
#pragma unroll
  for (int t = 0; t < TO; ++t)
#pragma unroll
    for (int q = 0; q < Q; ++q)
      wf[t][q] = *reinterpret_cast<const f32x4*>(&Ws[(t * 16 + m) * (16 * Q + 4) + 16 * q + 4 * g]);
}

template <int Q, int TO>  // acc[t] = sum over (q, i) in the per-layer kernel's order
__device__ __forceinline__ void chain_mma(const f32x4 (&wf)[TO][Q], const f32x4 (&xv)[Q], f32x4 (&acc)[TO]) {
#pragma unroll
  for (int t = 0; t < TO; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < Q; ++q)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int t = 0; t < TO; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[t][q][i], xv[q][i], acc[t], 0, 0, 0);
}

// NV consecutive floats NV m .. NV m + NV - 1 of row `row` of a glds_rows<CW> image (chunks
// XOR-swizzled per row; NV = 1, 2, 4 or 8)
template <int CW, int NV>
__device__ __forceinline__ void lds_rowvec(const float* region, int row, int m, float (&v)[NV]) {
  constexpr int CPR = CW / 4;
  const int sw = row & (CPR - 1) & 15;
  if constexpr (NV >= 4) {
#pragma unroll
    for (int h = 0; h < NV / 4; ++h) {
      const int c = (NV / 4) * m + h;
      const f32x4 u = *reinterpret_cast<const f32x4*>(region + 4 * (row * CPR + (c ^ sw)));
      v[4 * h] = u[0]; v[4 * h + 1] = u[1]; v[4 * h + 2] = u[2]; v[4 * h + 3] = u[3];
    }
  } else {
    const int c = (NV * m) >> 2, off = (NV * m) & 3;
    const float* p = region + 4 * (row * CPR + (c ^ sw)) + off;
    if constexpr (NV == 2) {
      const float2 u = *reinterpret_cast<const float2*>(p);
      v[0] = u.x; v[1] = u.y;
    } else {
      v[0] = p[0];
    }
  }
}

// 16 rows [row0, row0 + 16) of a channels-first operand (item b = row0 / N) into a [C][16] LDS image
template <int C>
__device__ __forceinline__ void glds_cf(const float* __restrict__ src, int64_t sb, int N, int64_t row0, float* lds_dst,
                                        int lane) {
  const int64_t b = row0 / N, n0 = row0 - b * N;
#pragma unroll
  for (int j = 0; j < C / 16; ++j) {
    const int p = j * 64 + lane;
    const int c = p >> 2, pos = p & 3;
    const int ch = pos ^ ((c >> 2) & 3);
    __builtin_amdgcn_global_load_lds(src + b * sb + (int64_t)c * N + n0 + 4 * ch,
                                     (__attribute__((address_space(3))) void*)(lds_dst + j * 256), 16, 0, 0);
  }
}

// Rows [row0, row0 + 16) of a thin rows-layout operand (C < 16 channels: 16 C contiguous
// floats) by 4-byte glds, lane p taking float p (indices clamped to the tensor: a ragged last
// tile reads valid memory, its rows past R are masked at use): ceil(16 C / 64) instructions.
template <int C>
__device__ __forceinline__ void glds_thin(const float* __restrict__ src, int64_t row0, int64_t R, float* lds_dst,
                                          int lane) {
#pragma unroll
  for (int j = 0; j < (16 * C + 63) / 64; ++j) {
    const int64_t idx = min(row0 * C + j * 64 + lane, R * C - 1);
    __builtin_amdgcn_global_load_lds(src + idx, (__attribute__((address_space(3))) void*)(lds_dst + j * 64), 4, 0,
                                     0);
  }
}

}  // namespace pk
