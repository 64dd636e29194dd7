// (f2) TEASER++ scale estimation (estimate_scaling = true) on the device: TLSScaleSolver's adaptive
// voting over the translation-invariant measurements (TIMs) of all pairs, and the consistency
// graph at the estimated scale. Restated from the published TEASER++ source (parity unpinned, as
// the rest of f2; csrc/teaser.hip has the solver's other steps).
//
//   pair p = (i, j), i < j, row-major:  va = |a_j - a_i|, vb = |b_j - b_i| (the graph kernel's
//   sqrt((dx dx + dy dy) + dz dz)), X_p = vb / va, alpha_p = beta / va, beta = 2 noise sqrt(cbar2).
//   Vote (ScalarTLSEstimator::estimate with per-element ranges): endpoints (X_p - alpha_p, +p),
//   (X_p + alpha_p, -p) in pair order, stably ordered by key; sweep with eps = +-1: card += eps,
//   dw += eps w_p (w_p = 1 / alpha_p^2), dxw += eps w_p X_p, rsum -= eps alpha_p (from sum alpha),
//   sx += eps X_p, sx2 += eps X_p^2; xh = dxw / dw; cost = (card xh xh + sx2 - 2 sx xh) + rsum;
//   the scale is xh at the first minimum of cost among positions with card > 0.
//   Scaled graph: edge (i, j) iff the pair is usable and |X_p - scale| <= alpha_p.
//   Build-defined deviation: a pair with va == 0 or a non-finite X_p takes no part in the vote and
//   is never an edge (upstream would produce inf / NaN). No usable pair: scale 1, status 0.
//
// MI355X layout. Crop b owns the fixed slot range [b S, b S + n_b (n_b - 1)), S = nmax (nmax - 1),
// of every record buffer, so nothing depends on the other crops of the batch or on nmax:
//   emit     grid (row, crop): pair p writes records 2p, 2p + 1: key = the f64 endpoint mapped to an
//            order-preserving u64 (an unusable pair: the all-ones key, which sorts last and is
//            skipped by the sweep), payload = i << 17 | j << 1 | upper (32 bits; nmax <= 32768).
//            The sweep recomputes X_p, alpha_p from the payload with the device function that made
//            the key (the coordinates, n x 48 B, stay in L2): no K-sized side arrays.
//   sort     stable LSD radix sort, 8 passes of 8 bits, segmented by crop: every pass ranks inside
//            the crop's own slot range, which is what a ninth pass on the crop id would achieve,
//            without moving the records once more. A block owns a tile of 4096 consecutive records:
//            histogram (per tile and per wave of the tile) -> exclusive scan over (digit, tile) ->
//            scatter. The rank of a record inside its tile comes from wave ballots in record order
//            on top of the histogram's counts of the waves before it (no atomic decides a position,
//            so the order is the input order: stable and deterministic); the tile is staged in LDS
//            in ranked order and written out in runs of equal digits. A pass whose digit is the same for all of a
//            crop's records is skipped for that crop (a per-crop parity word on the device says
//            which of the two buffers holds its records). Every scatter index is clamped to the
//            crop's slot range.
//   sweep    segmented inclusive scans of the running sums in fp64 over a fixed partition (tiles
//            of 2048 records: tile sums -> per-crop carry pass -> apply), the cost at each
//            position, block argmin with the lowest position winning ties, then a per-crop
//            reduction over the tiles. No float atomics; every word of the workspace that is read
//            has been written by the same call, so results are bitwise reproducible and do not
//            depend on the workspace's prior contents, on B or on nmax.
#include <cmath>
#include <limits>

#include "posekern.h"
#include "common.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSortThreads = 512;  // the sort's blocks: 8 waves hide the ranking chain's latency
constexpr int kSortWaves = kSortThreads / 64;
constexpr int kIter = 8;
constexpr int kWaveTile = 64 * kIter;          // consecutive records ranked by one wave
constexpr int kTile = kSortWaves * kWaveTile;  // records ranked by one block of the sort
constexpr int kScanItems = 8;
constexpr int kScanTile = kThreads * kScanItems;  // records swept by one block
constexpr int kNQ = 7;  // card, dw, dxw, eps alpha, sx, sx2, alpha of the lower endpoints
constexpr uint64_t kSentinel = ~0ull;
constexpr int kMaxN = 32768;

__device__ __forceinline__ int crop_n(const int64_t* __restrict__ off, int b, int nmax) {
  const int64_t n = off[b + 1] - off[b];
  return n < 0 ? 0 : n > nmax ? nmax : (int)n;
}

// The TIM ratio of pair (i, j): X = |b_j - b_i| / |a_j - a_i|, alpha = beta / |a_j - a_i|.
// false: the pair is unusable (va == 0 or X not finite).
__device__ __forceinline__ bool tim_measure(const double* __restrict__ A, const double* __restrict__ D, int i, int j,
                                            double beta, double* X, double* alpha) {
  const double sx = A[3 * j] - A[3 * i], sy = A[3 * j + 1] - A[3 * i + 1], sz = A[3 * j + 2] - A[3 * i + 2];
  const double tx = D[3 * j] - D[3 * i], ty = D[3 * j + 1] - D[3 * i + 1], tz = D[3 * j + 2] - D[3 * i + 2];
  const double va = sqrt((sx * sx + sy * sy) + sz * sz);
  const double vb = sqrt((tx * tx + ty * ty) + tz * tz);
  const double x = vb / va;
  *X = x;
  *alpha = beta / va;
  return va != 0.0 && isfinite(x);
}

// Order-preserving map of a double (no NaN) to u64; -0.0 and +0.0 map to one key.
__device__ __forceinline__ uint64_t f64_ordered(double v) {
  const uint64_t u = (uint64_t)__double_as_longlong(v + 0.0);
  return (u >> 63) ? ~u : (u | (1ull << 63));
}

// grid (nmax, B): row i of crop b emits the records of the pairs (i, j), j > i.
__global__ __launch_bounds__(kThreads) void scale_emit_kernel(const double* __restrict__ src,
                                                              const double* __restrict__ dst,
                                                              const int64_t* __restrict__ off, int nmax, int64_t S,
                                                              double beta, uint64_t* __restrict__ keys,
                                                              uint32_t* __restrict__ pay) {
  const int b = blockIdx.y, i = blockIdx.x;
  const int n = crop_n(off, b, nmax);
  if (i >= n - 1) return;
  const double* A = src + 3 * off[b];
  const double* D = dst + 3 * off[b];
  const int64_t count = (int64_t)n * (n - 1);
  const int64_t p0 = (int64_t)i * n - ((int64_t)i * (i + 1)) / 2;  // pairs of the rows above
  for (int j = i + 1 + threadIdx.x; j < n; j += kThreads) {
    double X, al;
    const bool ok = tim_measure(A, D, i, j, beta, &X, &al);
    const int64_t r = 2 * (p0 + (j - i - 1));
    if (r + 1 >= count) continue;  // cannot happen: r + 1 <= n (n - 1) - 1
    const uint32_t pl = ((uint32_t)i << 17) | ((uint32_t)j << 1);
    keys[b * S + r] = ok ? f64_ordered(X - al) : kSentinel;
    keys[b * S + r + 1] = ok ? f64_ordered(X + al) : kSentinel;
    pay[b * S + r] = pl;
    pay[b * S + r + 1] = pl | 1u;
  }
}

// Lanes of the wave holding the same digit as this lane, among the valid lanes.
__device__ __forceinline__ uint64_t match_digit(bool valid, uint32_t digit) {
  uint64_t m = __ballot(valid);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const bool bit = (digit >> k) & 1u;
    const uint64_t bal = __ballot(valid && bit);
    m &= bit ? bal : ~bal;
  }
  return m;
}

// grid (ntile_max, B): the digit counts of tile t of crop b: wave w counts the tile's records
// [512 w, 512 w + 512) -> wtable[b][t][w][digit] (the scatter's wave bases), their sum over the
// waves -> table[b][digit][t].
__global__ __launch_bounds__(kSortThreads) void scale_hist_kernel(const uint64_t* __restrict__ keys0,
                                                                  const uint64_t* __restrict__ keys1,
                                                                  const int64_t* __restrict__ off, int B, int nmax,
                                                                  int64_t S, int ntile_max, int pass,
                                                                  const int32_t* __restrict__ parity,
                                                                  uint32_t* __restrict__ table,
                                                                  uint32_t* __restrict__ wtable) {
  __shared__ uint32_t wc[kSortWaves][256];
  const int b = blockIdx.y, w = pk::wave_id(), lane = pk::lane_id();
  const int n = crop_n(off, b, nmax);
  const int64_t count = (int64_t)n * (n - 1);
  const int64_t t = blockIdx.x;
  if (t * kTile >= count) return;  // block-uniform
  const int par = pass == 0 ? 0 : parity[(pass - 1) * B + b];
  const uint64_t* keys = (par ? keys1 : keys0) + b * S;
  for (int k = threadIdx.x; k < kSortWaves * 256; k += kSortThreads) (&wc[0][0])[k] = 0u;
  __syncthreads();
  const int shift = 8 * pass;
#pragma unroll 4
  for (int it = 0; it < kIter; ++it) {
    const int64_t r = t * kTile + w * kWaveTile + it * 64 + lane;
    const bool valid = r < count;
    const uint32_t digit = valid ? (uint32_t)(keys[r] >> shift) & 255u : 0u;
    const uint64_t m = match_digit(valid, digit);
    if (valid && lane == __builtin_ctzll(m)) wc[w][digit] += (uint32_t)__builtin_popcountll(m);
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  uint32_t* wt = wtable + ((int64_t)b * ntile_max + t) * (kSortWaves * 256);
  for (int k = threadIdx.x; k < kSortWaves * 256; k += kSortThreads) wt[k] = (&wc[0][0])[k];
  if (threadIdx.x < 256) {
    uint32_t tot = 0u;
#pragma unroll
    for (int k = 0; k < kSortWaves; ++k) tot += wc[k][threadIdx.x];
    table[((int64_t)b * 256 + threadIdx.x) * ntile_max + t] = tot;
  }
}

// grid (256, B): exclusive scan of table[b][d][0 .. ntiles_b) in place, its total to dtot[b][d].
__global__ __launch_bounds__(kThreads) void scale_scan_tiles_kernel(const int64_t* __restrict__ off, int nmax,
                                                                    int ntile_max, uint32_t* __restrict__ table,
                                                                    uint32_t* __restrict__ dtot) {
  __shared__ uint32_t wsum[kWaves];
  const int b = blockIdx.y, d = blockIdx.x, w = pk::wave_id(), lane = pk::lane_id();
  const int n = crop_n(off, b, nmax);
  const int64_t count = (int64_t)n * (n - 1);
  int64_t nt = (count + kTile - 1) / kTile;
  if (nt > ntile_max) nt = ntile_max;
  uint32_t* e = table + ((int64_t)b * 256 + d) * ntile_max;
  const int64_t c = (nt + kThreads - 1) / kThreads;
  const int64_t lo = threadIdx.x * c, hi = lo + c < nt ? lo + c : nt;
  uint32_t s = 0u;
  for (int64_t k = lo; k < hi; ++k) s += e[k];
  uint32_t inc = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_up(inc, o);
    if (lane >= o) inc += v;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  uint32_t run = inc - s;
  for (int k = 0; k < w; ++k) run += wsum[k];
  for (int64_t k = lo; k < hi; ++k) {
    const uint32_t v = e[k];
    e[k] = run;
    run += v;
  }
  if (threadIdx.x == kThreads - 1) dtot[b * 256 + d] = run;
}

// grid (B): exclusive scan of the 256 digit totals of crop b; the pass is skipped for the crop
// when one digit holds all of its records (parity[pass][b] keeps the previous value).
__global__ __launch_bounds__(256) void scale_scan_digits_kernel(const int64_t* __restrict__ off, int B, int nmax,
                                                                int pass, const uint32_t* __restrict__ dtot,
                                                                uint32_t* __restrict__ dbase,
                                                                int32_t* __restrict__ parity) {
  __shared__ uint32_t wsum[kWaves];
  __shared__ int same;
  const int b = blockIdx.x, d = threadIdx.x, w = pk::wave_id(), lane = pk::lane_id();
  const int n = crop_n(off, b, nmax);
  const int64_t count = (int64_t)n * (n - 1);
  if (d == 0) same = count == 0 ? 1 : 0;
  __syncthreads();
  const uint32_t s = dtot[b * 256 + d];
  if (count > 0 && (int64_t)s == count) same = 1;  // at most one thread
  uint32_t inc = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_up(inc, o);
    if (lane >= o) inc += v;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  uint32_t run = inc - s;
  for (int k = 0; k < w; ++k) run += wsum[k];
  dbase[b * 256 + d] = run;
  if (d == 0) parity[pass * B + b] = (pass == 0 ? 0 : parity[(pass - 1) * B + b]) ^ (same ? 0 : 1);
}

// grid as scale_hist_kernel: the block ranks the records of its tile by digit in LDS (wave w ranks
// its 512 consecutive records by ballots on top of the counts of the waves before it — wtable, so the
// local order is the input order), then writes the staged tile out in local order: the records of
// one digit go to consecutive slots, in runs.
__global__ __launch_bounds__(kSortThreads) void scale_scatter_kernel(uint64_t* __restrict__ keys0,
                                                                     uint64_t* __restrict__ keys1,
                                                                     uint32_t* __restrict__ pay0,
                                                                     uint32_t* __restrict__ pay1,
                                                                     const int64_t* __restrict__ off, int B, int nmax,
                                                                     int64_t S, int ntile_max, int pass,
                                                                     const int32_t* __restrict__ parity,
                                                                     const uint32_t* __restrict__ table,
                                                                     const uint32_t* __restrict__ wtable,
                                                                     const uint32_t* __restrict__ dbase) {
  __shared__ uint64_t sk[kTile];
  __shared__ uint32_t sp[kTile];
  __shared__ uint32_t wc[kSortWaves][256];
  __shared__ uint32_t lbase[256], gbase[256], wsum[4];
  const int b = blockIdx.y, w = pk::wave_id(), lane = pk::lane_id(), d = threadIdx.x;
  const int n = crop_n(off, b, nmax);
  const int64_t count = (int64_t)n * (n - 1);
  const int64_t t = blockIdx.x;
  if (t * kTile >= count) return;  // block-uniform
  const int par = pass == 0 ? 0 : parity[(pass - 1) * B + b];
  if (parity[pass * B + b] == par) return;  // pass skipped for this crop (block-uniform)
  const uint64_t* ki = (par ? keys1 : keys0) + b * S;
  const uint32_t* pi = (par ? pay1 : pay0) + b * S;
  uint64_t* ko = (par ? keys0 : keys1) + b * S;
  uint32_t* po = (par ? pay0 : pay1) + b * S;
  const int shift = 8 * pass;
  const int64_t r0 = t * kTile + w * kWaveTile + lane;
  // thread d < 256: the local base of digit d (exclusive scan of the tile's counts), then of each wave
  uint32_t c[kSortWaves], tot = 0u, inc = 0u;
  if (d < 256) {
#pragma unroll
    for (int k = 0; k < kSortWaves; ++k) {  // the histogram kernel's per-wave counts of this tile
      c[k] = wtable[((int64_t)b * ntile_max + t) * (kSortWaves * 256) + k * 256 + d];
      tot += c[k];
    }
    inc = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t v = __shfl_up(inc, o);
      if (lane >= o) inc += v;
    }
    if (lane == 63) wsum[w] = inc;
  }
  __syncthreads();
  if (d < 256) {
    uint32_t lb = inc - tot;
    for (int k = 0; k < w; ++k) lb += wsum[k];
    lbase[d] = lb;
    gbase[d] = dbase[b * 256 + d] + table[((int64_t)b * 256 + d) * ntile_max + t];
#pragma unroll
    for (int k = 0; k < kSortWaves; ++k) {
      wc[k][d] = lb;
      lb += c[k];
    }
  }
  __syncthreads();
#pragma unroll 4
  for (int it = 0; it < kIter; ++it) {
    const int64_t r = r0 + it * 64;
    const bool valid = r < count;
    const uint64_t key = valid ? ki[r] : 0ull;
    const uint32_t pl = valid ? pi[r] : 0u;
    const uint32_t digit = (uint32_t)(key >> shift) & 255u;
    const uint64_t m = match_digit(valid, digit);
    uint32_t pos = 0u;
    if (valid) pos = wc[w][digit] + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
    __builtin_amdgcn_wave_barrier();
    if (valid && lane == __builtin_ctzll(m)) wc[w][digit] += (uint32_t)__builtin_popcountll(m);
    __builtin_amdgcn_wave_barrier();
    if (valid) {
      pos = pos < (uint32_t)kTile ? pos : (uint32_t)kTile - 1u;  // a ranking bug must not leave the stage
      sk[pos] = key;
      sp[pos] = pl;
    }
  }
  __syncthreads();
  const int64_t left = count - t * kTile;
  const int nvalid = left < kTile ? (int)left : kTile;
  for (int l = threadIdx.x; l < nvalid; l += kSortThreads) {
    const uint64_t k = sk[l];
    const uint32_t dg = (uint32_t)(k >> shift) & 255u;
    int64_t g = (int64_t)gbase[dg] + ((uint32_t)l - lbase[dg]);
    g = g < count ? g : count - 1;  // ... nor the crop's slots
    ko[g] = k;
    po[g] = sp[l];
  }
}

// The sweep contributions of one sorted record (zero for the records of unusable pairs).
__device__ __forceinline__ void contribution(uint64_t key, uint32_t pl, const double* __restrict__ A,
                                             const double* __restrict__ D, int n, double beta, double v[kNQ]) {
#pragma unroll
  for (int q = 0; q < kNQ; ++q) v[q] = 0.0;
  if (key == kSentinel) return;
  int i = (int)(pl >> 17), j = (int)((pl >> 1) & 0xFFFFu);
  i = i < n ? i : n - 1;
  j = j < n ? j : n - 1;
  double X, al;
  tim_measure(A, D, i, j, beta, &X, &al);
  const double eps = (pl & 1u) ? -1.0 : 1.0;
  const double wgt = 1.0 / (al * al);
  v[0] = eps;
  v[1] = eps * wgt;
  v[2] = (eps * wgt) * X;
  v[3] = eps * al;
  v[4] = eps * X;
  v[5] = (eps * X) * X;
  v[6] = (pl & 1u) ? 0.0 : al;
}

// grid (nscan_max, B): the sums of tile t of crop b -> partial[b][t][0..7).
__global__ __launch_bounds__(kThreads) void scale_partial_kernel(const uint64_t* __restrict__ keys0,
                                                                 const uint64_t* __restrict__ keys1,
                                                                 const uint32_t* __restrict__ pay0,
                                                                 const uint32_t* __restrict__ pay1,
                                                                 const double* __restrict__ src,
                                                                 const double* __restrict__ dst,
                                                                 const int64_t* __restrict__ off, int B, int nmax,
                                                                 int64_t S, int nscan_max, double beta,
                                                                 const int32_t* __restrict__ parity,
                                                                 double* __restrict__ partial) {
  __shared__ double wsum[kWaves][kNQ];
  const int b = blockIdx.y, t = blockIdx.x;
  const int n = crop_n(off, b, nmax);
  const int64_t count = (int64_t)n * (n - 1);
  if ((int64_t)t * kScanTile >= count) return;  // block-uniform
  const int par = parity[7 * B + b];
  const uint64_t* keys = (par ? keys1 : keys0) + b * S;
  const uint32_t* pay = (par ? pay1 : pay0) + b * S;
  const double* A = src + 3 * off[b];
  const double* D = dst + 3 * off[b];
  double s[kNQ];
#pragma unroll
  for (int q = 0; q < kNQ; ++q) s[q] = 0.0;
  const int64_t r0 = (int64_t)t * kScanTile + (int64_t)threadIdx.x * kScanItems;
  for (int k = 0; k < kScanItems; ++k) {
    const int64_t r = r0 + k;
    if (r >= count) break;
    double v[kNQ];
    contribution(keys[r], pay[r], A, D, n, beta, v);
#pragma unroll
    for (int q = 0; q < kNQ; ++q) s[q] += v[q];
  }
#pragma unroll
  for (int q = 0; q < kNQ; ++q) {
    const double x = pk::wave_sum_f64(s[q]);
    if (pk::lane_id() == 0) wsum[pk::wave_id()][q] = x;
  }
  __syncthreads();
  if (threadIdx.x < kNQ) {
    double x = 0.0;
    for (int w = 0; w < kWaves; ++w) x += wsum[w][threadIdx.x];
    partial[((int64_t)b * nscan_max + t) * 8 + threadIdx.x] = x;
  }
}

// Exclusive prefix of v over the block's threads in thread order (fixed association).
__device__ __forceinline__ double block_exclusive_f64(double v, double* sh) {
  const int w = pk::wave_id(), lane = pk::lane_id();
  double inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double u = __shfl_up(inc, o);
    if (lane >= o) inc += u;
  }
  double ex = __shfl_up(inc, 1);
  if (lane == 0) ex = 0.0;
  __syncthreads();
  if (lane == 63) sh[w] = inc;
  __syncthreads();
  double base = 0.0;
  for (int k = 0; k < w; ++k) base += sh[k];
  return base + ex;
}

// grid (B): carry[b][t] = the sums of the tiles before t; salpha[b] = the sum of alpha.
__global__ __launch_bounds__(kThreads) void scale_carry_kernel(const int64_t* __restrict__ off, int nmax,
                                                               int nscan_max, const double* __restrict__ partial,
                                                               double* __restrict__ carry,
                                                               double* __restrict__ salpha) {
  __shared__ double sh[kWaves];
  const int b = blockIdx.x;
  const int n = crop_n(off, b, nmax);
  const int64_t count = (int64_t)n * (n - 1);
  int64_t nt = (count + kScanTile - 1) / kScanTile;
  if (nt > nscan_max) nt = nscan_max;
  const double* P = partial + (int64_t)b * nscan_max * 8;
  double* C = carry + (int64_t)b * nscan_max * 8;
  const int64_t c = (nt + kThreads - 1) / kThreads;
  const int64_t lo = threadIdx.x * c, hi = lo + c < nt ? lo + c : nt;
  for (int q = 0; q < kNQ; ++q) {
    double s = 0.0;
    for (int64_t k = lo; k < hi; ++k) s += P[k * 8 + q];
    double run = block_exclusive_f64(s, sh);
    for (int64_t k = lo; k < hi; ++k) {
      C[k * 8 + q] = run;
      run += P[k * 8 + q];
    }
    if (q == kNQ - 1 && threadIdx.x == kThreads - 1) salpha[b] = run;
  }
}

struct Best {
  double cost, xh, pos, card;
};

__device__ __forceinline__ Best better(const Best& a, const Best& o) {
  return (o.cost < a.cost || (o.cost == a.cost && o.pos < a.pos)) ? o : a;
}

__device__ __forceinline__ Best wave_best(Best v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    Best u;
    u.cost = __shfl_xor(v.cost, o);
    u.xh = __shfl_xor(v.xh, o);
    u.pos = __shfl_xor(v.pos, o);
    u.card = __shfl_xor(v.card, o);
    v = better(v, u);
  }
  return v;
}

// grid (nscan_max, B): inclusive scan inside tile t on top of its carry, the cost at every
// position, the tile's best (cost, lowest position) -> tbest[b][t].
__global__ __launch_bounds__(kThreads) void scale_apply_kernel(const uint64_t* __restrict__ keys0,
                                                               const uint64_t* __restrict__ keys1,
                                                               const uint32_t* __restrict__ pay0,
                                                               const uint32_t* __restrict__ pay1,
                                                               const double* __restrict__ src,
                                                               const double* __restrict__ dst,
                                                               const int64_t* __restrict__ off, int B, int nmax,
                                                               int64_t S, int nscan_max, double beta,
                                                               const int32_t* __restrict__ parity,
                                                               const double* __restrict__ carry,
                                                               const double* __restrict__ salpha,
                                                               double* __restrict__ tbest) {
  __shared__ double sh[kWaves];
  __shared__ Best wb[kWaves];
  const int b = blockIdx.y, t = blockIdx.x;
  const int n = crop_n(off, b, nmax);
  const int64_t count = (int64_t)n * (n - 1);
  if ((int64_t)t * kScanTile >= count) return;  // block-uniform
  const int par = parity[7 * B + b];
  const uint64_t* keys = (par ? keys1 : keys0) + b * S;
  const uint32_t* pay = (par ? pay1 : pay0) + b * S;
  const double* A = src + 3 * off[b];
  const double* D = dst + 3 * off[b];
  const int64_t r0 = (int64_t)t * kScanTile + (int64_t)threadIdx.x * kScanItems;
  double v[kScanItems][kNQ], s[kNQ];
#pragma unroll
  for (int q = 0; q < kNQ; ++q) s[q] = 0.0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    const int64_t r = r0 + k;
    if (r < count) {
      contribution(keys[r], pay[r], A, D, n, beta, v[k]);
    } else {
#pragma unroll
      for (int q = 0; q < kNQ; ++q) v[k][q] = 0.0;
    }
#pragma unroll
    for (int q = 0; q < kNQ; ++q) s[q] += v[k][q];
  }
  const double* C = carry + ((int64_t)b * nscan_max + t) * 8;
  double run[kNQ];
#pragma unroll
  for (int q = 0; q < kNQ - 1; ++q) run[q] = C[q] + block_exclusive_f64(s[q], sh);
  const double sa = salpha[b];
  Best best{std::numeric_limits<double>::infinity(), 1.0, 9.0e18, 0.0};
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
#pragma unroll
    for (int q = 0; q < kNQ - 1; ++q) run[q] += v[k][q];
    if (v[k][0] != 0.0 && run[0] > 0.0) {
      const double xh = run[2] / run[1];
      const double cost = (run[0] * xh * xh + run[5] - 2 * run[4] * xh) + (sa - run[3]);
      if (cost < best.cost) best = Best{cost, xh, (double)(r0 + k), run[0]};
    }
  }
  best = wave_best(best);
  if (pk::lane_id() == 0) wb[pk::wave_id()] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWaves; ++w) best = better(best, wb[w]);
    double* o = tbest + ((int64_t)b * nscan_max + t) * 4;
    o[0] = best.cost;
    o[1] = best.xh;
    o[2] = best.pos;
    o[3] = best.card;
  }
}

// grid (B): the crop's best tile -> scale[b], scale_info[b] = (status, consensus size).
__global__ __launch_bounds__(kThreads) void scale_final_kernel(const int64_t* __restrict__ off, int nmax,
                                                               int nscan_max, const double* __restrict__ tbest,
                                                               double* __restrict__ scale,
                                                               int32_t* __restrict__ scale_info) {
  __shared__ Best wb[kWaves];
  const int b = blockIdx.x;
  const int n = crop_n(off, b, nmax);
  const int64_t count = (int64_t)n * (n - 1);
  int64_t nt = (count + kScanTile - 1) / kScanTile;
  if (nt > nscan_max) nt = nscan_max;
  Best best{std::numeric_limits<double>::infinity(), 1.0, 9.0e18, 0.0};
  for (int64_t k = threadIdx.x; k < nt; k += kThreads) {
    const double* o = tbest + ((int64_t)b * nscan_max + k) * 4;
    best = better(best, Best{o[0], o[1], o[2], o[3]});
  }
  best = wave_best(best);
  if (pk::lane_id() == 0) wb[pk::wave_id()] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWaves; ++w) best = better(best, wb[w]);
    const bool voted = best.cost < std::numeric_limits<double>::infinity();
    scale[b] = voted ? best.xh : 1.0;
    scale_info[2 * b] = voted ? 1 : 0;
    scale_info[2 * b + 1] = voted ? (int32_t)best.card : 0;
  }
}

// teaser_graph_kernel's layout (grid (nmax, B), wave ballots -> adjacency words) with the scaled
// pair test |X_p - scale[b]| <= alpha_p.
__global__ __launch_bounds__(kThreads) void teaser_graph_scaled_kernel(const double* __restrict__ src,
                                                                       const double* __restrict__ dst,
                                                                       const int64_t* __restrict__ off, int nmax,
                                                                       int W, double beta,
                                                                       const double* __restrict__ scale,
                                                                       uint64_t* __restrict__ adj,
                                                                       int32_t* __restrict__ deg) {
  __shared__ int wsum[kWaves];
  const int b = blockIdx.y, i = blockIdx.x;
  const int n = crop_n(off, b, nmax);
  uint64_t* row = adj + ((int64_t)b * nmax + i) * W;
  if (i >= n) {  // padding rows: empty (block-uniform)
    for (int w = threadIdx.x; w < W; w += kThreads) row[w] = 0ull;
    if (threadIdx.x == 0) deg[(int64_t)b * nmax + i] = 0;
    return;
  }
  const double* A = src + 3 * off[b];
  const double* D = dst + 3 * off[b];
  const double s = scale[b];
  int cnt = 0;
  for (int j0 = 0; j0 < W * 64; j0 += kThreads) {
    const int j = j0 + threadIdx.x;
    bool e = false;
    if (j < n && j != i) {
      double X, al;
      const bool ok = tim_measure(A, D, i < j ? i : j, i < j ? j : i, beta, &X, &al);
      e = ok && fabs(X - s) <= al;
    }
    const uint64_t word = __ballot(e);
    if (pk::lane_id() == 0 && (j0 >> 6) + pk::wave_id() < W) row[(j0 >> 6) + pk::wave_id()] = word;
    cnt += e ? 1 : 0;
  }
  cnt = pk::wave_sum_i32(cnt);
  if (pk::lane_id() == 0) wsum[pk::wave_id()] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < kWaves; ++w) t += wsum[w];
    deg[(int64_t)b * nmax + i] = t;
  }
}

struct Layout {
  int64_t S, E, keys0, keys1, pay0, pay1, table, wtable, dtot, dbase, parity, partial, carry, salpha, tbest, total;
  int ntile_max, nscan_max;
};

using pk::al256;

Layout layout(int B, int nmax) {
  Layout L;
  L.S = (int64_t)nmax * (nmax > 0 ? nmax - 1 : 0);
  L.E = (int64_t)B * L.S;
  L.ntile_max = (int)((L.S + kTile - 1) / kTile);
  L.nscan_max = (int)((L.S + kScanTile - 1) / kScanTile);
  int64_t o = 0;
  auto take = [&](int64_t bytes) {
    const int64_t at = o;
    o += al256(bytes);
    return at;
  };
  L.keys0 = take(8 * L.E);
  L.keys1 = take(8 * L.E);
  L.pay0 = take(4 * L.E);
  L.pay1 = take(4 * L.E);
  L.table = take(4 * (int64_t)B * 256 * L.ntile_max);
  L.wtable = take(4 * (int64_t)B * L.ntile_max * kSortWaves * 256);
  L.dtot = take(4 * (int64_t)B * 256);
  L.dbase = take(4 * (int64_t)B * 256);
  L.parity = take(4 * (int64_t)B * 8);
  L.partial = take(8 * (int64_t)B * L.nscan_max * 8);
  L.carry = take(8 * (int64_t)B * L.nscan_max * 8);
  L.salpha = take(8 * (int64_t)B);
  L.tbest = take(8 * (int64_t)B * L.nscan_max * 4);
  L.total = o;
  return L;
}

}  // namespace

extern "C" int64_t pk_teaser_scale_work_size(int B, int nmax) {
  if (B < 0 || nmax < 0 || nmax > kMaxN) return -1;
  return layout(B, nmax).total;
}

extern "C" int pk_teaser_scale(const double* src, const double* dst, const int64_t* off, int B, int nmax, double beta,
                               void* work, int64_t work_bytes, double* scale, int32_t* scale_info, void* stream) {
  PK_REQUIRE(B >= 0 && B <= 65535 && nmax >= 0 && nmax <= kMaxN && beta >= 0.0 && std::isfinite(beta));
  if (B == 0) return PK_OK;
  PK_REQUIRE(off && scale && scale_info);
  const Layout L = layout(B, nmax);
  PK_REQUIRE(work_bytes >= L.total && (L.total == 0 || work));
  PK_REQUIRE(L.S == 0 || (src && dst));
  hipStream_t s = pk::as_stream(stream);
  char* base = static_cast<char*>(work);
  uint64_t* keys0 = reinterpret_cast<uint64_t*>(base + L.keys0);
  uint64_t* keys1 = reinterpret_cast<uint64_t*>(base + L.keys1);
  uint32_t* pay0 = reinterpret_cast<uint32_t*>(base + L.pay0);
  uint32_t* pay1 = reinterpret_cast<uint32_t*>(base + L.pay1);
  uint32_t* table = reinterpret_cast<uint32_t*>(base + L.table);
  uint32_t* wtable = reinterpret_cast<uint32_t*>(base + L.wtable);
  uint32_t* dtot = reinterpret_cast<uint32_t*>(base + L.dtot);
  uint32_t* dbase = reinterpret_cast<uint32_t*>(base + L.dbase);
  int32_t* parity = reinterpret_cast<int32_t*>(base + L.parity);
  double* partial = reinterpret_cast<double*>(base + L.partial);
  double* carry = reinterpret_cast<double*>(base + L.carry);
  double* salpha = reinterpret_cast<double*>(base + L.salpha);
  double* tbest = reinterpret_cast<double*>(base + L.tbest);
  if (L.S > 0) {
    hipLaunchKernelGGL(scale_emit_kernel, dim3(nmax, B), dim3(kThreads), 0, s, src, dst, off, nmax, L.S, beta, keys0,
                       pay0);
    PK_CHECK_LAUNCH();
    const dim3 tg(L.ntile_max, B);
    for (int pass = 0; pass < 8; ++pass) {
      hipLaunchKernelGGL(scale_hist_kernel, tg, dim3(kSortThreads), 0, s, keys0, keys1, off, B, nmax, L.S, L.ntile_max,
                         pass, parity, table, wtable);
      PK_CHECK_LAUNCH();
      hipLaunchKernelGGL(scale_scan_tiles_kernel, dim3(256, B), dim3(kThreads), 0, s, off, nmax, L.ntile_max, table,
                         dtot);
      PK_CHECK_LAUNCH();
      hipLaunchKernelGGL(scale_scan_digits_kernel, dim3(B), dim3(256), 0, s, off, B, nmax, pass, dtot, dbase, parity);
      PK_CHECK_LAUNCH();
      hipLaunchKernelGGL(scale_scatter_kernel, tg, dim3(kSortThreads), 0, s, keys0, keys1, pay0, pay1, off, B, nmax, L.S,
                         L.ntile_max, pass, parity, table, wtable, dbase);
      PK_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(scale_partial_kernel, dim3(L.nscan_max, B), dim3(kThreads), 0, s, keys0, keys1, pay0, pay1, src,
                       dst, off, B, nmax, L.S, L.nscan_max, beta, parity, partial);
    PK_CHECK_LAUNCH();
    hipLaunchKernelGGL(scale_carry_kernel, dim3(B), dim3(kThreads), 0, s, off, nmax, L.nscan_max, partial, carry,
                       salpha);
    PK_CHECK_LAUNCH();
    hipLaunchKernelGGL(scale_apply_kernel, dim3(L.nscan_max, B), dim3(kThreads), 0, s, keys0, keys1, pay0, pay1, src,
                       dst, off, B, nmax, L.S, L.nscan_max, beta, parity, carry, salpha, tbest);
    PK_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(scale_final_kernel, dim3(B), dim3(kThreads), 0, s, off, nmax, L.nscan_max, tbest, scale,
                     scale_info);
  PK_CHECK_LAUNCH();
  return PK_OK;
}

extern "C" int pk_teaser_graph_scaled(const double* src, const double* dst, const int64_t* off, int B, int nmax,
                                      double beta, const double* scale, uint64_t* adj, int32_t* deg, void* stream) {
  PK_REQUIRE(B >= 0 && B <= 65535 && nmax >= 0 && beta >= 0.0 && std::isfinite(beta));
  if (B == 0 || nmax == 0) return PK_OK;
  PK_REQUIRE(src && dst && off && scale && adj && deg);
  const int W = (nmax + 63) / 64;
  hipLaunchKernelGGL(teaser_graph_scaled_kernel, dim3(nmax, B), dim3(kThreads), 0, pk::as_stream(stream), src, dst,
                     off, nmax, W, beta, scale, adj, deg);
  PK_CHECK_LAUNCH();
  return PK_OK;
}
