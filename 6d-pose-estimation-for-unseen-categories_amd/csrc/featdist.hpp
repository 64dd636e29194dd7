// What the two feature-distance units share: featdist.hip (the entry points and the one-pass fp32
// path) and featdist_twopass.hip (the two-pass path: the bf16 modes and unaligned mode-0 inputs).
#pragma once
#include "common.hpp"
#include "mfma_tile.hpp"

namespace pk {

// The two-pass path, defined in featdist_twopass.hip (hidden: not part of the C ABI). The scratch
// bytes of a call, and its launches; `work` holds at least that many bytes and the arguments are
// pk_feat_dist_topk's, already checked.
__attribute__((visibility("hidden"))) int64_t fd_twopass_work_size(int B, int V1max, int V2max, int topk, int mode);
__attribute__((visibility("hidden"))) int fd_twopass_launch(const float* evecs_x, int ldx, const float* C,
                                                            const float* evecs_y, int ldy, const int32_t* n1,
                                                            const int32_t* n2, int B, int V1max, int V2max, int topk,
                                                            int mode, void* work, int64_t* out_idx, float* out_dist,
                                                            hipStream_t s);

}  // namespace pk

namespace {

constexpr int kF = 30;   // n_fmap
constexpr int kK = 32;   // contraction length (K padded)
using pk::f32x4;

// Block numbering of the 1-D grids that give every crop `per` blocks: hardware block L lands on
// XCD L % 8, so when B % 8 == 0 all blocks of crop b are put on XCD b % 8 (one L2 holds the crop's
// operands). Sets the crop b and the block's number k among the crop's.
__device__ __forceinline__ void fd_crop_block(int per, int B, int& b, int& k) {
  const int L = blockIdx.x;
  if ((B & 7) == 0) {
    const int x8 = L & 7, q = L >> 3;
    b = x8 + 8 * (q / per);
    k = q - (q / per) * per;
  } else {
    b = L / per;
    k = L - b * per;
  }
}

template <int TOPK>
struct TopK {
  float v[TOPK];
  int i[TOPK];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int k = 0; k < TOPK; ++k) {
      v[k] = __builtin_huge_valf();
      i[k] = 0x7fffffff;
    }
  }
  // rows arrive in increasing index order: strict < keeps the lowest index on ties
  __device__ __forceinline__ void push(float x, int idx) {
    if (TOPK == 1) {
      const bool lt = x < v[0];
      v[0] = lt ? x : v[0];
      i[0] = lt ? idx : i[0];
      return;
    }
    if (!(x < v[TOPK - 1])) return;
    float cv = x;
    int ci = idx;
#pragma unroll
    for (int k = 0; k < TOPK; ++k) {
      const bool sw = cv < v[k];
      const float tv = sw ? v[k] : cv;
      const int ti = sw ? i[k] : ci;
      v[k] = sw ? cv : v[k];
      i[k] = sw ? ci : i[k];
      cv = tv;
      ci = ti;
    }
  }
  // merge an incoming sorted list (ties: lower index first)
  __device__ __forceinline__ void merge(const float (&ov)[TOPK], const int (&oi)[TOPK]) {
#pragma unroll
    for (int k = 0; k < TOPK; ++k) {
      float cv = ov[k];
      int ci = oi[k];
#pragma unroll
      for (int m = 0; m < TOPK; ++m) {
        const bool sw = cv < v[m] || (cv == v[m] && ci < i[m]);
        const float tv = sw ? v[m] : cv;
        const int ti = sw ? i[m] : ci;
        v[m] = sw ? cv : v[m];
        i[m] = sw ? ci : i[m];
        cv = tv;
        ci = ti;
      }
    }
  }
};

// RS > 1, the last pass of the two-pass path and of the one-pass top-5 (each unit instantiates what
// it launches): grid (ceil(V2max / 256), B): merge the RS partial lists of each column in row-split
// order (ties: lower row).
template <int TOPK>
__global__ __launch_bounds__(256) void fd_merge_kernel(const float* __restrict__ part_v,
                                                       const int32_t* __restrict__ part_i,
                                                       const int32_t* __restrict__ n2, int V2max, int RS,
                                                       int64_t* __restrict__ out_idx, float* __restrict__ out_dist) {
  const int b = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n2[b]) return;
  TopK<TOPK> best;
  best.init();
  for (int rs = 0; rs < RS; ++rs) {
    const int64_t o = (((int64_t)b * RS + rs) * V2max + j) * TOPK;
    float ov[TOPK];
    int oi[TOPK];
#pragma unroll
    for (int q = 0; q < TOPK; ++q) {
      ov[q] = part_v[o + q];
      oi[q] = part_i[o + q];
    }
    best.merge(ov, oi);
  }
  const int64_t o = ((int64_t)b * V2max + j) * TOPK;
#pragma unroll
  for (int q = 0; q < TOPK; ++q) {
    out_idx[o + q] = best.i[q] == 0x7fffffff ? -1 : best.i[q];
    if (out_dist) out_dist[o + q] = sqrtf(best.v[q]);
  }
}

}  // namespace
