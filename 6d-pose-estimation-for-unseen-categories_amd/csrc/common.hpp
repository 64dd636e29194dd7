// Shared helpers for the posekern HIP kernels (gfx950 / CDNA4, wave64).
//
// Every translation unit is compiled with -ffp-contract=off: kernels that must be
// bit-exact against the CPU oracle (FPS, ball query, crop formation) rely on each
// product and sum being rounded separately, exactly like numpy / torch-CPU do.
// Kernels that want fused multiply-adds spell them out with fma()/fmaf().
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdlib>
#include <cstring>

#define PK_OK 0
#define PK_ERR_ARG 1000      // invalid argument (shape / size / null pointer)
#define PK_ERR_CAPACITY 1001 // a variable-size output exceeded the caller's capacity

#define PK_CHECK_LAUNCH()                                   \
  do {                                                      \
    hipError_t e__ = hipGetLastError();                     \
    if (e__ != hipSuccess) return (int)e__;                 \
  } while (0)

#define PK_REQUIRE(cond)            \
  do {                              \
    if (!(cond)) return PK_ERR_ARG; \
  } while (0)

namespace pk {

// Wave priority of the crop-formation kernels that run beside the training step on the second
// stream (FPS, SOR): s_setprio(1..3) raises their waves' issue priority over the training
// kernels' waves sharing a SIMD; 0: unchanged. The product library uses PK_SIDE_PRIO_DEFAULT;
// the development library reads PK_SIDE_PRIO (tools/prio_ab.py).
#ifndef PK_SIDE_PRIO_DEFAULT
#define PK_SIDE_PRIO_DEFAULT 0
#endif
// development diagnostics (libposekern_dev.so only): PK_DIAG_SKIP=<name>[,<name>] skips the named
// crop-formation launches (fps, sorknn, bpwrite, bqmask) so a bench run measures how much each one's
// occupancy costs the overlapped step; the product library never skips anything
inline bool diag_skip(const char* name) {
#ifdef PK_DEVBUILD
  static const char* e = std::getenv("PK_DIAG_SKIP");
  if (e == nullptr) return false;
  const char* p = std::strstr(e, name);
  return p != nullptr;
#else
  (void)name;
  return false;
#endif
}

// development diagnostic (dev library only): PK_DIAG_TWICE names launches issued twice (the
// marginal cost of a crop-formation kernel beside the overlapped training step; results unchanged:
// the repeated kernels are idempotent)
inline bool diag_twice(const char* name) {
#ifdef PK_DEVBUILD
  static const char* e = std::getenv("PK_DIAG_TWICE");
  return e != nullptr && std::strstr(e, name) != nullptr;
#else
  (void)name;
  return false;
#endif
}

inline int side_prio() {
#ifdef PK_DEVBUILD
  static const int v = [] {
    const char* e = std::getenv("PK_SIDE_PRIO");
    const int x = e ? std::atoi(e) : PK_SIDE_PRIO_DEFAULT;
    return x < 0 ? 0 : x > 3 ? 3 : x;
  }();
  return v;
#else
  return PK_SIDE_PRIO_DEFAULT;
#endif
}
__device__ __forceinline__ void set_wave_prio(int prio) {
  if (prio == 1) __builtin_amdgcn_s_setprio(1);
  else if (prio == 2) __builtin_amdgcn_s_setprio(2);
  else if (prio == 3) __builtin_amdgcn_s_setprio(3);
}

constexpr int kWave = 64;

__device__ __forceinline__ int lane_id() { return threadIdx.x & (kWave - 1); }

// XCD-aware block renumbering for a 3-D grid: hardware block L = x + X (y + Y z) runs on XCD
// L % 8 (round-robin dispatch, MI355X_MICROARCH.md); each XCD gets a contiguous range of
// logical blocks (bijective for any grid size), so the x-blocks of one (y, z) — e.g. the
// query blocks of one (crop, head), which share their K / V — sit in one XCD's L2.
// Returns the logical (x, y, z).
__device__ __forceinline__ int3 xcd_block3() {
  const int X = gridDim.x, Y = gridDim.y;
  const int G = X * Y * gridDim.z;
  const int L = blockIdx.x + X * (blockIdx.y + Y * blockIdx.z);
  const int q8 = G >> 3, r8 = G & 7, x8 = L & 7;
  const int lg = x8 * q8 + (x8 < r8 ? x8 : r8) + (L >> 3);
  return make_int3(lg % X, (lg / X) % Y, lg / (X * Y));
}
__device__ __forceinline__ int wave_id() { return threadIdx.x >> 6; }

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    uint64_t o = __shfl_xor(v, off);
    v = o > v ? o : v;
  }
  return v;
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    uint64_t o = __shfl_xor(v, off);
    v = o < v ? o : v;
  }
  return v;
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// Inclusive prefix sum across a wave (Hillis-Steele on shuffles).
__device__ __forceinline__ int wave_inclusive_scan_i32(int v) {
  const int lane = lane_id();
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    int o = __shfl_up(v, off);
    if (lane >= off) v += o;
  }
  return v;
}

__device__ __forceinline__ int64_t wave_sum_i64(int64_t v) {  // exact: any order
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ int64_t wave_inclusive_scan_i64(int64_t v) {
  const int lane = lane_id();
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    int64_t o = __shfl_up(v, off);
    if (lane >= off) v += o;
  }
  return v;
}

// Bits of a non-negative float are monotone as an unsigned integer.
__device__ __forceinline__ uint32_t f32_bits(float f) { return __float_as_uint(f); }

// Order-preserving map of any float to uint32 (for min/max keys on signed values).
__device__ __forceinline__ uint32_t f32_ordered(float f) {
  uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Inverse of f32_ordered.
__device__ __forceinline__ float f32_unordered(uint32_t u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Bytes rounded up to the 256-byte granule at which the entry points carve their scratch.
__host__ __device__ inline int64_t al256(int64_t x) { return (x + 255) & ~(int64_t)255; }

}  // namespace pk

namespace pk {

// ---- DPP row (16-lane) all-reductions, u32. After the call every lane of a 16-lane
// row holds the row's reduction. dpp_ctrl: quad_perm[1,0,3,2]=0xB1, quad_perm[2,3,0,1]
// =0x4E, row_half_mirror=0x141, row_mirror=0x140.
#define PK_DPP(v, ctrl) ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), ctrl, 0xF, 0xF, false))

__device__ __forceinline__ uint32_t row_max_u32(uint32_t v) {
  uint32_t o;
  o = PK_DPP(v, 0xB1); v = o > v ? o : v;
  o = PK_DPP(v, 0x4E); v = o > v ? o : v;
  o = PK_DPP(v, 0x141); v = o > v ? o : v;
  o = PK_DPP(v, 0x140); v = o > v ? o : v;
  return v;
}

__device__ __forceinline__ uint32_t row_min_u32(uint32_t v) {
  uint32_t o;
  o = PK_DPP(v, 0xB1); v = o < v ? o : v;
  o = PK_DPP(v, 0x4E); v = o < v ? o : v;
  o = PK_DPP(v, 0x141); v = o < v ? o : v;
  o = PK_DPP(v, 0x140); v = o < v ? o : v;
  return v;
}

__device__ __forceinline__ uint32_t readlane(uint32_t v, int l) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}

// Wave-uniform max / min of a u32 (result is a scalar).
__device__ __forceinline__ uint32_t wave_max_u32_s(uint32_t v) {
  v = row_max_u32(v);
  uint32_t a = readlane(v, 0), b = readlane(v, 16), c = readlane(v, 32), d = readlane(v, 48);
  a = a > b ? a : b;
  c = c > d ? c : d;
  return a > c ? a : c;
}

// Wave-uniform signed max of an i32 (result is a scalar).
__device__ __forceinline__ int wave_max_i32_s(int v) {
  int o;
  o = (int)PK_DPP(v, 0xB1); v = o > v ? o : v;
  o = (int)PK_DPP(v, 0x4E); v = o > v ? o : v;
  o = (int)PK_DPP(v, 0x141); v = o > v ? o : v;
  o = (int)PK_DPP(v, 0x140); v = o > v ? o : v;
  int a = (int)readlane((uint32_t)v, 0), b = (int)readlane((uint32_t)v, 16), c = (int)readlane((uint32_t)v, 32),
      d = (int)readlane((uint32_t)v, 48);
  a = a > b ? a : b;
  c = c > d ? c : d;
  return a > c ? a : c;
}

__device__ __forceinline__ uint32_t wave_min_u32_s(uint32_t v) {
  v = row_min_u32(v);
  uint32_t a = readlane(v, 0), b = readlane(v, 16), c = readlane(v, 32), d = readlane(v, 48);
  a = a < b ? a : b;
  c = c < d ? c : d;
  return a < c ? a : c;
}

}  // namespace pk

namespace pk {
__device__ __forceinline__ int row_sum_i32(int v) {
  v += (int)PK_DPP(v, 0xB1);
  v += (int)PK_DPP(v, 0x4E);
  v += (int)PK_DPP(v, 0x141);
  v += (int)PK_DPP(v, 0x140);
  return v;
}
// Wave-uniform sum of an int (scalar result), DPP + readlane (no LDS traffic).
__device__ __forceinline__ int wave_sum_i32_s(int v) {
  v = row_sum_i32(v);
  return (int)(readlane((uint32_t)v, 0) + readlane((uint32_t)v, 16) + readlane((uint32_t)v, 32) +
               readlane((uint32_t)v, 48));
}
}  // namespace pk

namespace pk {
// Zero-fill on the stream with a kernel instead of hipMemsetAsync: memset nodes captured
// into a HIP graph were observed not to order correctly against the kernels around them
// on replay (ROCm 7.2, tools/replay_diag3.py), so no libposekern entry point issues one.
namespace {  // one copy per translation unit
__global__ void zero_fill_kernel(uint8_t* __restrict__ p, size_t n) {
  const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
  if (i + 16 <= n && (((uintptr_t)p) & 15) == 0) {
    *reinterpret_cast<uint4*>(p + i) = make_uint4(0u, 0u, 0u, 0u);
  } else {
    for (size_t k = i; k < n && k < i + 16; ++k) p[k] = 0;
  }
}

inline hipError_t zero_async(void* p, size_t bytes, hipStream_t s) {
  if (bytes == 0) return hipSuccess;
  const size_t threads = (bytes + 15) / 16;
  const unsigned blocks = (unsigned)((threads + 255) / 256);
  hipLaunchKernelGGL(zero_fill_kernel, dim3(blocks), dim3(256), 0, s, static_cast<uint8_t*>(p), bytes);
  return hipGetLastError();
}
}  // namespace
}  // namespace pk
