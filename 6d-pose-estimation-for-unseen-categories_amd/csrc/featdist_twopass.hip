// H10 / H11 (first half), the two-pass path of pk_feat_dist_topk (featdist.hip holds the entry
// points, the reference and the precision modes): the bf16 modes and unaligned mode-0 inputs.
//
// Pass 1 (prep): one thread per row computes the row's operand (x side: emb = x C^T, an fmaf
// chain over k in order; y side: y) and its squared norm, and writes the operand straight
// into MFMA operand-tile order (16-row tiles, lane l = 16 g + c holding row c's k values of
// its group g), so pass 2 moves whole tiles with 16-byte loads and no transposes.
// Pass 2 (main, fd_main_direct_kernel): a block = 4 waves over 4 column tiles and the block's
// row tiles; each wave takes 2 column tiles (B operands in registers) and half the rows, and
// streams its rows' fragments from L2 into registers one chunk ahead of the MFMAs (every A
// fragment feeds two accumulation chains). Epilogue per 16 x 16 tile: running argmin / sorted
// top-5 per column (ties: lowest row); the two row halves merge through LDS at the end. With
// RS > 1 the blocks' row parts write partial lists that pass 3 (fd_merge_kernel, featdist.hpp)
// merges (same tie rule), so one 4096-point crop (configs[4]) still spreads over the chip.
#include <algorithm>

#include "featdist.hpp"

namespace {

constexpr int kCW = 1;   // column tiles per wave
constexpr int kWaves = 4;
constexpr int kCH = 8;   // row tiles per LDS stage
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

// bytes of one 16-row operand tile per mode (f32: 64 lanes x 8 floats; bf16: 64 x 8 bf16;
// bf16x3: hi then lo)
__host__ __device__ constexpr int tile_bytes(int mode) { return mode == 0 ? 2048 : mode == 1 ? 1024 : 2048; }

__device__ __forceinline__ __bf16 to_bf16(float v) { return (__bf16)v; }

// grid (ceil(max(T1, T2) / 8), B, 2), block 512: wave = one 16-row tile of one side (z = 0:
// x side, 1: y side). Lane (g, c) = (lane >> 4, lane & 15).
//   x side: emb = x C^T on the f32 MFMA ([16 x 32] x [32 x 32], two 16 x 16 output tiles,
//           K = 30 zero-padded; an f32 MFMA accumulates as the fmaf chain over k in order),
//           then through LDS into the operand layout;
//   y side: y itself.
// The squared norm of a row is its lane group's 8 values summed per lane, then across the 4
// lanes of the row (fixed order). Rows >= n (and the tile padding) are written as zeros.
constexpr int kPrepWaves = 8;  // one 16-row tile per wave, 8 waves per block

template <int MODE>
__global__ __launch_bounds__(64 * kPrepWaves) void fd_prep_kernel(const float* __restrict__ ex, int ldx,
                                                      const float* __restrict__ C, const float* __restrict__ ey,
                                                      int ldy, const int32_t* __restrict__ n1,
                                                      const int32_t* __restrict__ n2, int V1max, int V2max, int T1,
                                                      int T2, char* __restrict__ A, char* __restrict__ Bq,
                                                      float* __restrict__ nA, float* __restrict__ nB) {
  __shared__ float E[kPrepWaves][16][kK + 1];  // per wave: the tile's rows (emb or y), k padded to 32
  const int b = blockIdx.y;
  const bool xside = blockIdx.z == 0;
  const int w = pk::wave_id(), lane = pk::lane_id(), g = lane >> 4, c16 = lane & 15;
  const int T = xside ? T1 : T2;
  const int tile = blockIdx.x * kPrepWaves + w;
  if (tile >= T) return;
  const int r = tile * 16 + c16;
  // every operand load is issued before the first wait: the row at a clamped index (its
  // validity against n applied by select afterwards), the C entries (both sides: C is tiny),
  // and n itself — a load addressed through n, or behind the x-side branch, would add a round
  // trip each
  const float* rowp = xside ? ex + ((int64_t)b * V1max + min(r, V1max - 1)) * ldx
                            : ey + ((int64_t)b * V2max + min(r, V2max - 1)) * ldy;
  // this lane's 8 row values at k = 4 s + g (the f32 MFMA operand layout), 0 past k = 29
  float xv[8];
  float cvs[2][8];
#pragma unroll
  for (int s = 0; s < 8; ++s) xv[s] = rowp[min(4 * s + g, kF - 1)];
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int s = 0; s < 8; ++s)
      cvs[n][s] = C[((int64_t)b * kF + min(16 * n + c16, kF - 1)) * kF + min(4 * s + g, kF - 1)];
  const int nval = xside ? n1[b] : n2[b];
  const bool valid = r < nval;
  // the empty asm pins the loads above this point (else the compiler sinks them under the
  // select / the x-side branch, behind a wait of their own)
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int s = 0; s < 8; ++s) asm volatile("" : "+v"(cvs[n][s]));
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    asm volatile("" : "+v"(xv[s]));
    xv[s] = (valid && 4 * s + g < kF) ? xv[s] : 0.f;
  }
  float (*Ew)[kK + 1] = E[w];
  if (xside) {
    // D[row 4 g' + q][col c] of output tile n: emb[row][16 n + c] = sum_k x[row][k] C[16 n + c][k]
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const int cc = 16 * n + c16;
#pragma unroll
      for (int s = 0; s < 8; ++s)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s], (cc < kF && 4 * s + g < kF) ? cvs[n][s] : 0.f, acc, 0, 0, 0);
#pragma unroll
      for (int q = 0; q < 4; ++q) Ew[4 * g + q][cc] = acc[q];
    }
  } else {
#pragma unroll
    for (int s = 0; s < 8; ++s) Ew[c16][4 * s + g] = xv[s];
  }
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  // the lane's operand values (mode 0: k = 4 s + g; bf16 modes: k = 8 g + j) and the row norm
  float v[8];
  float part = 0.f;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const int k = MODE == 0 ? 4 * s + g : 8 * g + s;
    v[s] = (valid && k < kF) ? Ew[c16][k] : 0.f;
    part = fmaf(v[s], v[s], part);
  }
  const float p1 = __shfl_xor(part, 16), p2 = __shfl_xor(part, 32), p3 = __shfl_xor(part, 48);
  const float mine[4] = {part, p1, p2, p3};  // lane group g, g^1, g^2, g^3
  float nrm = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) nrm += mine[q ^ g];  // groups 0, 1, 2, 3 in that order
  // padding rows: y side zeros; x side a row whose distance to every column is +inf (mode 0:
  // the |x|^2 slot; bf16 modes: the norm), so the main pass needs no row mask
  if (!valid) nrm = xside ? __builtin_huge_valf() : 0.f;
  char* base = (xside ? A + (int64_t)b * T1 * tile_bytes(MODE) : Bq + (int64_t)b * T2 * tile_bytes(MODE)) +
               (int64_t)tile * tile_bytes(MODE);
  if (MODE == 0) {
    // augmented operand: x side [-2 emb, |emb|^2, 1], y side [y, 1, |y|^2]
    float o[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) o[s] = xside ? -2.f * v[s] : v[s];
    if (g >= 2 && valid) o[7] = (xside == (g == 2)) ? nrm : 1.f;  // k = 30 (g = 2), 31 (g = 3)
    if (g == 2 && xside && !valid) o[7] = nrm;                      // +inf |x|^2 slot
    float4* d = reinterpret_cast<float4*>(base + (size_t)lane * 32);
    d[0] = make_float4(o[0], o[1], o[2], o[3]);
    d[1] = make_float4(o[4], o[5], o[6], o[7]);
  } else {
    // bf16 cross-term operand: x side -2 emb, y side y (k < 30, zero pad); k = 8 g + j
    bf16x8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float f = xside ? -2.f * v[j] : v[j];
      const __bf16 h = to_bf16(f);
      hi[j] = h;
      lo[j] = to_bf16(f - (float)h);
    }
    *reinterpret_cast<bf16x8*>(base + (size_t)lane * 16) = hi;
    if (MODE == 2) *reinterpret_cast<bf16x8*>(base + 1024 + (size_t)lane * 16) = lo;
    if (g == 0) (xside ? nA + (int64_t)b * T1 * 16 : nB + (int64_t)b * T2 * 16)[r] = nrm;
  }
}

// 4 distances of this lane (rows ibase .. ibase + 3 of its column) into the running top-k
template <int TOPK>
__device__ __forceinline__ void epilogue(const float (&d)[4], int ibase, TopK<TOPK>& best) {
#pragma unroll
  for (int r = 0; r < 4; ++r) best.push(fmaxf(d[r], 1e-30f), ibase + r);  // clamp_min(1e-30) (cdist mm path)
}

template <int TOPK>
__device__ __forceinline__ void lanegroup_merge(TopK<TOPK>& best) {
#pragma unroll
  for (int off = 16; off <= 32; off <<= 1) {
    float ov[TOPK];
    int oi[TOPK];
#pragma unroll
    for (int k = 0; k < TOPK; ++k) {
      ov[k] = __shfl_xor(best.v[k], off);
      oi[k] = __shfl_xor(best.i[k], off);
    }
    best.merge(ov, oi);
  }
}

// One 16 x 16 tile (rows of A tile `a`, this wave's column tile) -> 4 values per lane
// (rows 4 g + r, column c16).
template <int MODE>
struct Frag;
template <> struct Frag<0> { float a[8]; };
template <> struct Frag<1> { bf16x8 hi; float n[4]; };
template <> struct Frag<2> { bf16x8 hi, lo; float n[4]; };

template <int MODE>
__device__ __forceinline__ void read_frag(const char* __restrict__ tile, const float* __restrict__ ntile, int lane,
                                          Frag<MODE>& f) {
  if constexpr (MODE == 0) {
    const float4* p = reinterpret_cast<const float4*>(tile + lane * 32);
    const float4 u = p[0], w = p[1];
    f.a[0] = u.x; f.a[1] = u.y; f.a[2] = u.z; f.a[3] = u.w;
    f.a[4] = w.x; f.a[5] = w.y; f.a[6] = w.z; f.a[7] = w.w;
  } else {
    f.hi = *reinterpret_cast<const bf16x8*>(tile + lane * 16);
    if constexpr (MODE == 2) f.lo = *reinterpret_cast<const bf16x8*>(tile + 1024 + lane * 16);
    const float4 n = *reinterpret_cast<const float4*>(ntile + 4 * (lane >> 4));
    f.n[0] = n.x; f.n[1] = n.y; f.n[2] = n.z; f.n[3] = n.w;
  }
}

template <int MODE>
struct BOp;
template <> struct BOp<0> { float b[8]; };
template <> struct BOp<1> { bf16x8 hi; float n; };
template <> struct BOp<2> { bf16x8 hi, lo; float n; };

template <int MODE>
__device__ __forceinline__ void tile_dist(const Frag<MODE>& a, const BOp<MODE>& b, float (&d)[4]) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if constexpr (MODE == 0) {
#pragma unroll
    for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.a[s], b.b[s], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) d[r] = acc[r];
  } else {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.hi, b.hi, acc, 0, 0, 0);
    if constexpr (MODE == 2) {
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.hi, b.lo, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.lo, b.hi, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) d[r] = (acc[r] + a.n[r]) + b.n;  // |x|^2 - 2 x.y + |y|^2
  }
}

// Top-1 running state of a lane: per row offset r (rows 16 t + 4 g + r of its column) the
// smallest clamped distance so far, as its f32 bit pattern (clamped values are positive, so
// their bit patterns order as the values do), and the tile t holding it. Per distance: integer
// max (the clamp), difference, sign mask, bit-select, integer min — no compare-to-VCC, so the
// four chains interleave with each other and the MFMAs without hazard stalls. Ties stay with
// the earliest tile because tiles arrive in increasing order and only a strictly smaller key
// moves the tile.
struct Top1x4 {
  int k[4];
  int t[4];
};

// The main pass, without LDS staging. Block = 4 waves = 2 column pairs x 2 row halves: wave (wc, wr) takes column tiles
// 4 cg + 2 wc and 4 cg + 2 wc + 1 and half wr of the block's row tiles, reading the rows' MFMA
// fragments straight from L2 into registers one chunk of CHD tiles ahead of the MFMAs (two
// register buffers: the next chunk's loads are in flight during this chunk's 16 * CHD MFMAs).
// Every A fragment feeds both column tiles (two independent accumulation chains per row tile,
// half the L2 traffic per MFMA of a one-column wave); no barrier until the end, where the
// second row half hands its lists through LDS to the first, which merges them (ties: lower
// row) and writes the block's columns.
template <int TOPK, int MODE>
__global__ __launch_bounds__(64 * kWaves) void fd_main_direct_kernel(
    const char* __restrict__ A, const char* __restrict__ Bq, const float* __restrict__ nA,
    const float* __restrict__ nB, const int32_t* __restrict__ n1, const int32_t* __restrict__ n2, int T1, int T2,
    int V2max, int NCG, int RS, int64_t* __restrict__ out_idx, float* __restrict__ out_dist,
    float* __restrict__ part_v, int32_t* __restrict__ part_i) {
  constexpr int TB = tile_bytes(MODE);
  constexpr int CHD = MODE == 2 ? 2 : 4;
  __shared__ float hv[2][2][16][TOPK];  // second row half's lists: [wc][column tile][column][k]
  __shared__ int hi_[2][2][16][TOPK];
  const int per = NCG * RS;
  const int B = (int)(gridDim.x / per);
  int b, k;
  fd_crop_block(per, B, b, k);
  const int cg = k % NCG, rs = k / NCG;
  const int lane = pk::lane_id(), w = pk::wave_id();
  const int g = lane >> 4, c16 = lane & 15;
  // (readfirstlane: the wave-uniform values in scalar registers, so the chunk loop is a scalar
  // loop and not an exec-masked one whose wait counts the compiler cannot track)
  const int wc = __builtin_amdgcn_readfirstlane(w & 1), wr = __builtin_amdgcn_readfirstlane(w >> 1);
  const int ct0 = cg * kWaves + 2 * wc;  // this wave's column tiles ct0, ct0 + 1
  const int N1 = n1[b], N2 = n2[b];
  const int nt = (N1 + 15) >> 4;
  const int tb0 = (nt * rs) / RS, te0 = (nt * (rs + 1)) / RS;      // the block's row part
  const int tb = tb0 + ((te0 - tb0) * wr) / 2, te = tb0 + ((te0 - tb0) * (wr + 1)) / 2;  // this wave's half
  BOp<MODE> bo[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {  // (a column tile past T2 reads tile T2 - 1; its lists are not written)
    const char* bt = Bq + ((int64_t)b * T2 + min(ct0 + c, T2 - 1)) * TB;
    if constexpr (MODE == 0) {
      const float4* p = reinterpret_cast<const float4*>(bt + lane * 32);
      const float4 u = p[0], v = p[1];
      bo[c].b[0] = u.x; bo[c].b[1] = u.y; bo[c].b[2] = u.z; bo[c].b[3] = u.w;
      bo[c].b[4] = v.x; bo[c].b[5] = v.y; bo[c].b[6] = v.z; bo[c].b[7] = v.w;
    } else {
      bo[c].hi = *reinterpret_cast<const bf16x8*>(bt + lane * 16);
      if constexpr (MODE == 2) bo[c].lo = *reinterpret_cast<const bf16x8*>(bt + 1024 + lane * 16);
      bo[c].n = nB[((int64_t)b * T2 + min(ct0 + c, T2 - 1)) * 16 + c16];
    }
  }
  const char* At = A + (int64_t)b * T1 * TB;
  const float* nAt = MODE != 0 ? nA + (int64_t)b * T1 * 16 : nullptr;
  TopK<TOPK> best[2];
  Top1x4 b4[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    best[c].init();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      b4[c].k[r] = 0x7f800000;  // +inf: never replaced by an equal key
      b4[c].t[r] = 0x7fffffff;
    }
  }
  // tiles past te are loaded at te - 1 (unconditional loads: no branch, no early wait) and
  // their distances masked to +inf before the selection
  auto load = [&](Frag<MODE> (&f)[CHD], int c0) {
#pragma unroll
    for (int t = 0; t < CHD; ++t) {
      const int tt = min(c0 + t, te - 1);
      read_frag<MODE>(At + (int64_t)tt * TB, nAt ? nAt + (int64_t)tt * 16 : nullptr, lane, f[t]);
    }
  };
  auto compute = [&](const Frag<MODE> (&f)[CHD], int c0) {
#pragma unroll
    for (int t = 0; t < CHD; ++t) {
      float d[2][4];
      tile_dist<MODE>(f[t], bo[0], d[0]);
      tile_dist<MODE>(f[t], bo[1], d[1]);
      const bool in = c0 + t < te;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        if constexpr (TOPK == 1) {
          constexpr int kClamp = 0x0da24260;  // bits of 1e-30f: clamp_min(1e-30) (cdist mm path)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int key = in ? max(__float_as_int(d[c][r]), kClamp) : 0x7f800000;
            const int m = (key - b4[c].k[r]) >> 31;  // -1 iff key < best
            b4[c].t[r] = (m & (c0 + t)) | (~m & b4[c].t[r]);
            b4[c].k[r] = min(key, b4[c].k[r]);
          }
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) d[c][r] = in ? d[c][r] : __builtin_huge_valf();
          epilogue<TOPK>(d[c], (c0 + t) * 16 + 4 * g, best[c]);
        }
      }
    }
  };
  const int nch = __builtin_amdgcn_readfirstlane(te > tb ? (te - tb + CHD - 1) / CHD : 0);
  if (nch > 0) {
    // (sched_barrier: the scheduler would otherwise sink each load next to its first use)
    Frag<MODE> fa[CHD], fb[CHD];
    load(fa, tb);
    // (no early exit: every iteration issues both loads, so a chunk's loads are always in
    // flight across the previous chunk's MFMAs, the back edge included)
    for (int ci = 0; ci < nch; ci += 2) {
      const int c0 = tb + ci * CHD;
      load(fb, c0 + CHD);
      __builtin_amdgcn_sched_barrier(0);
      compute(fa, c0);
      load(fa, c0 + 2 * CHD);
      __builtin_amdgcn_sched_barrier(0);
      if (ci + 1 < nch) compute(fb, c0 + CHD);
    }
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    if constexpr (TOPK == 1) {  // the 4 row offsets: smallest value, ties lowest row
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = b4[c].t[r] == 0x7fffffff ? 0x7fffffff : b4[c].t[r] * 16 + 4 * g + r;
        const float v = __int_as_float(b4[c].k[r]);
        const bool take = v < best[c].v[0] || (v == best[c].v[0] && row < best[c].i[0]);
        best[c].v[0] = take ? v : best[c].v[0];
        best[c].i[0] = take ? row : best[c].i[0];
      }
    }
    lanegroup_merge<TOPK>(best[c]);
  }
  // the second row half's lists to the first (ties: lower row — the merge's index rule)
  if (wr == 1 && g == 0) {
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int q = 0; q < TOPK; ++q) {
        hv[wc][c][c16][q] = best[c].v[q];
        hi_[wc][c][c16][q] = best[c].i[q];
      }
  }
  __syncthreads();
  if (wr == 1 || g != 0) return;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    float ov[TOPK];
    int oi[TOPK];
#pragma unroll
    for (int q = 0; q < TOPK; ++q) {
      ov[q] = hv[wc][c][c16][q];
      oi[q] = hi_[wc][c][c16][q];
    }
    best[c].merge(ov, oi);
    const int ct = ct0 + c;
    const int j = ct * 16 + c16;
    if (ct >= T2 || j >= N2) continue;
    if (RS == 1) {
      const int64_t o = ((int64_t)b * V2max + j) * TOPK;
#pragma unroll
      for (int q = 0; q < TOPK; ++q) {
        out_idx[o + q] = best[c].i[q] == 0x7fffffff ? -1 : best[c].i[q];
        if (out_dist) out_dist[o + q] = sqrtf(best[c].v[q]);
      }
    } else {
      const int64_t o = (((int64_t)b * RS + rs) * V2max + j) * TOPK;
#pragma unroll
      for (int q = 0; q < TOPK; ++q) {
        part_v[o + q] = best[c].v[q];
        part_i[o + q] = best[c].i[q];
      }
    }
  }
}

struct FdPlan {
  int T1, T2, NCG, RS;
  int64_t a_bytes, b_bytes, na_bytes, nb_bytes, pv_bytes, pi_bytes;
};

inline FdPlan fd_plan(int B, int V1max, int V2max, int topk, int mode) {
  using pk::al256;
  FdPlan p{};
  p.T1 = (V1max + 15) / 16;
  p.T2 = (V2max + 15) / 16;
  p.NCG = (p.T2 + kWaves * kCW - 1) / (kWaves * kCW);
  const int64_t blocks = (int64_t)B * p.NCG;
  int rs = blocks >= 512 ? 1 : (int)((512 + blocks - 1) / blocks);
  const int max_rs = std::max(1, p.T1 / (2 * kCH));  // at least two chunks per row part
  p.RS = std::min(rs, max_rs);
  const int TB = tile_bytes(mode);
  p.a_bytes = al256((int64_t)B * p.T1 * TB);
  p.b_bytes = al256((int64_t)B * p.T2 * TB);
  p.na_bytes = mode ? al256((int64_t)B * p.T1 * 16 * 4) : 0;
  p.nb_bytes = mode ? al256((int64_t)B * p.T2 * 16 * 4) : 0;
  p.pv_bytes = p.RS > 1 ? al256((int64_t)B * p.RS * V2max * topk * 4) : 0;
  p.pi_bytes = p.pv_bytes;
  return p;
}

}  // namespace

int64_t pk::fd_twopass_work_size(int B, int V1max, int V2max, int topk, int mode) {
  const FdPlan p = fd_plan(B, V1max, V2max, topk, mode);
  return p.a_bytes + p.b_bytes + p.na_bytes + p.nb_bytes + p.pv_bytes + p.pi_bytes;
}

int pk::fd_twopass_launch(const float* evecs_x, int ldx, const float* C, const float* evecs_y, int ldy,
                          const int32_t* n1, const int32_t* n2, int B, int V1max, int V2max, int topk, int mode,
                          void* work, int64_t* out_idx, float* out_dist, hipStream_t s) {
  const FdPlan p = fd_plan(B, V1max, V2max, topk, mode);
  char* wp = static_cast<char*>(work);
  char* A = wp;
  char* Bq = A + p.a_bytes;
  float* nA = mode ? reinterpret_cast<float*>(Bq + p.b_bytes) : nullptr;
  float* nB = mode ? reinterpret_cast<float*>(Bq + p.b_bytes + p.na_bytes) : nullptr;
  float* pv = p.RS > 1 ? reinterpret_cast<float*>(Bq + p.b_bytes + p.na_bytes + p.nb_bytes) : nullptr;
  int32_t* pi = p.RS > 1 ? reinterpret_cast<int32_t*>(reinterpret_cast<char*>(pv) + p.pv_bytes) : nullptr;
  const dim3 pg((std::max(p.T1, p.T2) + kPrepWaves - 1) / kPrepWaves, B, 2);
#define PK_FD_PREP(M)                                                                                              \
  hipLaunchKernelGGL((fd_prep_kernel<M>), pg, dim3(64 * kPrepWaves), 0, s, evecs_x, ldx, C, evecs_y, ldy, n1, n2, V1max, V2max, \
                     p.T1, p.T2, A, Bq, nA, nB)
  if (mode == 0) PK_FD_PREP(0); else if (mode == 1) PK_FD_PREP(1); else PK_FD_PREP(2);
#undef PK_FD_PREP
  PK_CHECK_LAUNCH();
  const dim3 grid((unsigned)((int64_t)B * p.NCG * p.RS)), block(64 * kWaves);
#define PK_FD_MAIN(K, M)                                                                                          \
  hipLaunchKernelGGL((fd_main_direct_kernel<K, M>), grid, block, 0, s, A, Bq, nA, nB, n1, n2, p.T1, p.T2, V2max,  \
                     p.NCG, p.RS, out_idx, out_dist, pv, pi)
  if (topk == 1) {
    if (mode == 0) PK_FD_MAIN(1, 0); else if (mode == 1) PK_FD_MAIN(1, 1); else PK_FD_MAIN(1, 2);
  } else {
    if (mode == 0) PK_FD_MAIN(5, 0); else if (mode == 1) PK_FD_MAIN(5, 1); else PK_FD_MAIN(5, 2);
  }
#undef PK_FD_MAIN
  PK_CHECK_LAUNCH();
  if (p.RS > 1) {
    const dim3 mg((V2max + 255) / 256, B);
    if (topk == 1)
      hipLaunchKernelGGL(fd_merge_kernel<1>, mg, dim3(256), 0, s, pv, pi, n2, V2max, p.RS, out_idx, out_dist);
    else
      hipLaunchKernelGGL(fd_merge_kernel<5>, mg, dim3(256), 0, s, pv, pi, n2, V2max, p.RS, out_idx, out_dist);
    PK_CHECK_LAUNCH();
  }
  return PK_OK;
}
