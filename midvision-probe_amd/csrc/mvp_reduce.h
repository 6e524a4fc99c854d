// The fixed-order reductions of the loss, metric and scoring kernels: same inputs, same bits.
//
// The rule.  A floating-point sum is never left to arrival order (no float atomics).  A thread adds its own elements in index order; a
// wave adds its 64 lanes with the xor butterfly, offsets 32, 16, 8, 4, 2, 1 (every lane ends with the same bits); a 256-thread
// workgroup adds its four wave sums as (w0 + w1) + (w2 + w3); partials of several workgroups go to the caller's workspace, one row per
// workgroup, and whoever folds them takes rows t, t + T, t + 2T, ... in that order (T = 256 threads, or the 64 lanes of a wave) and
// then the sums above.  Integer counts are exact in any order and may use atomics.
//
// The helpers are device code for one-dimensional workgroups of exactly 256 threads (wave_sum and wave_fold_rows: any whole wave).
// block_sum and fold_rows issue two workgroup barriers, one before lane 0 of each wave writes `red` and one after, so every thread of
// the workgroup must reach them, and `red` may be reused — by the next call too — as soon as they return.  block_sum_once issues only
// the second one and leaves the sums in thread 0 alone: for a kernel that reduces once, at its end, into an array nothing else touches.
#pragma once
#include "mvp_common.h"

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// every thread ends with the sums of the workgroup's 256 values of v[0..N): N values, one LDS round.  (The butterfly is written out:
// through wave_sum the compiler schedules the N butterflies in another order, and the kernels of taskonomy.hip and objectness.hip,
// which had this body, would no longer compile to the instructions they had: profiles/reduce_header_kernel_resources.txt.)
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], double (*red)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) red[threadIdx.x >> 6][k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
}

// The same sums in the same order, in THREAD 0 ONLY, with one barrier: `red` must not have been read or written before in this launch.
// (The PSNR partial kernel, many short workgroups, measured about 1 % slower with block_sum's two barriers, and the compiler scheduled
// the pixel walk of augment_stats_kernel differently around them, 63 VGPRs for 55 and 1 to 2.5 % slower: profiles/reduce_header_bench.txt.)
template <int N>
__device__ __forceinline__ void block_sum_once(double (&v)[N], double (*red)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = wave_sum(v[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) red[threadIdx.x >> 6][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  }
}

// Fold of partial rows: v[k] = the sum over `rows` rows of `stride` doubles of column k, k < N <= stride.  Every workgroup that calls it
// on the same rows gets the same bits, so a kernel can fold the partials of the launch before it itself, without a launch in between.
template <int N>
__device__ __forceinline__ void fold_rows(const double* part, int rows, int stride, double (&v)[N], double (*red)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = 0.0;
  for (int r = threadIdx.x; r < rows; r += 256) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] += part[(size_t)r * stride + k];
  }
  block_sum<N>(v, red);
}

// The same by one wave, no LDS and no barrier: lane j takes rows j, j + 64, ...; every lane ends with the sums of the N columns.
template <int N>
__device__ __forceinline__ void wave_fold_rows(const double* part, int rows, double (&v)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = 0.0;
  for (int j = threadIdx.x & 63; j < rows; j += 64) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] += part[(size_t)j * N + k];
  }
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = wave_sum(v[k]);
}

// The verdict of 2AFC triplet b from its two scores (mvp_twoafc_score, mvp_pixel_score): called by one lane.
__device__ __forceinline__ void twoafc_verdict(float s_l, float s_r, int b, float* sim, int32_t* pred, const float* label, int64_t* counts) {
  const int pr = s_l > s_r ? 0 : 1;  // on the fp32 values that are written; NaN compares false -> 1, two +inf -> 1
  sim[2 * (size_t)b] = s_l;
  sim[2 * (size_t)b + 1] = s_r;
  pred[b] = pr;
  if (label && counts) {
    const float t = label[b];
    const int slot = t == 1.0f ? (pr ? 0 : 2) : (t == 0.0f ? (pr ? 1 : 3) : -1);  // TP FP FN TN, positive = 1
    if (slot >= 0) atomicAdd((unsigned long long*)(counts + slot), 1ull);  // integers: exact in any order
  }
}

// host: q is a multiple of a (a power of two); NULL is aligned to anything
inline bool aligned_to(const void* q, uintptr_t a) { return ((uintptr_t)q & (a - 1)) == 0; }
