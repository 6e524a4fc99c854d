// Range scan of the fp16 `hi` half of a pair operand (the guard under MVP_PREC_F16X2, whose producers saturate at +-65504 instead of
// overflowing: a saturated operand gives a finite, wrong result with nothing to show for it):
//   mvp_f16_range_scan   hi [rows, ld] 16-bit words (MVP_PAIR_SEPARATE) or one hi | lo array interleaved per 32 columns (MVP_PAIR_A_ILV32),
//                        columns [col0, col0 + cols) of every row -> a 16-byte record (max |bits|, n saturated, n non-finite, n scanned)
// Read-only and HBM-bound (2 B per element, nothing written but the record): a lane owns 8 consecutive columns of one row — one 16-byte
// load — and walks the (row, chunk) space with the grid's stride, four loads in flight per step.  Integer work only: |bits| = bits &
// 0x7FFF orders fp16 magnitudes (NaNs above inf above 65504), so one running maximum says whether a chunk needs counting at all; the two
// counters are touched only in a chunk whose maximum reaches 0x7BFF.  Gap columns (ld > window) and the lo blocks of the interleaved
// layout are never loaded.
// Reduction: per-lane accumulators -> wave64 shuffles -> one LDS row per wave -> ONE atomicMax and THREE atomicAdd on unsigned per
// workgroup into the caller's record (global vector atomics; the record is accumulated into, so several launches may share one; an
// add of zero — the two counters of a clean operand — is left out, which changes nothing).  This library otherwise has no atomics
// because float sums depend on arrival order; integer max and add commute and associate exactly, so the record holds the same four
// words whatever order the workgroups arrive in: two runs give the same bits.
// Few, large workgroups — at most one of 1 024 threads per CU of a 256-CU device, two atomics each on a clean operand — because
// the kernel's first shape, up to 1 024 workgroups of 256 threads (the same 16 waves per CU) with four atomics each, took 49 us per
// launch at every size measured, and this one 9 us at the small ones (profiles/f16_scan_bench.txt).  Supposed cause, not isolated by
// a measurement of its own (the two shapes differ in workgroup size AND atomic count): the atomics all land on one 16-byte line and
// are served one after the other, which would be about 12 ns each.
#include "mvp_reduce.h"

namespace {

constexpr unsigned SCAN_THREADS = 1024;
constexpr unsigned SCAN_MAX_BLOCKS = 256;  // one workgroup per CU of a 256-CU device; the rest by the grid stride
constexpr unsigned F16_SAT = 0x7BFFu;       // |v| = 65504, where the producers saturate
constexpr unsigned F16_INF = 0x7C00u;

struct scan_acc {
  unsigned max_bits, n_sat, n_nonfinite, n_scanned;
};

__device__ __forceinline__ void count_word(unsigned w, scan_acc& a) {
  const unsigned e0 = w & 0x7FFFu, e1 = (w >> 16) & 0x7FFFu;
  a.n_sat += (e0 == F16_SAT) + (e1 == F16_SAT);
  a.n_nonfinite += (e0 >= F16_INF) + (e1 >= F16_INF);
}

// 8 halves in four words.  The maximum of the upper halves is the upper half of the maximum of the masked words (the comparison of two
// words is decided by their upper halves unless those are equal); the lower halves are compared on their own.
__device__ __forceinline__ void scan_chunk(const u32x4_t v, scan_acc& a) {
  const unsigned w0 = v.x & 0x7FFF7FFFu, w1 = v.y & 0x7FFF7FFFu, w2 = v.z & 0x7FFF7FFFu, w3 = v.w & 0x7FFF7FFFu;
  const unsigned up = max(max(w0, w1), max(w2, w3)) >> 16;
  const unsigned dn = max(max(w0 & 0xFFFFu, w1 & 0xFFFFu), max(w2 & 0xFFFFu, w3 & 0xFFFFu));
  const unsigned m = max(up, dn);
  if (m >= F16_SAT) {  // rare: only then do the counters need the elements one by one
    count_word(w0, a);
    count_word(w1, a);
    count_word(w2, a);
    count_word(w3, a);
  }
  a.max_bits = max(a.max_bits, m);
  a.n_scanned += 8u;
}

__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
  return v;
}

// Chunk g of the window = 8 columns from col0 + 8 (g % nv) of row g / nv; (row, c) are carried along instead of divided out per step.
template <bool ILV>
__global__ __launch_bounds__(SCAN_THREADS) void f16_range_scan_kernel(const mvp_f16_scan_args p) {
  const unsigned nv = (unsigned)p.cols >> 3;
  const unsigned total = (unsigned)p.rows * nv;  // < 2^31: checked by the launcher
  const unsigned stride = gridDim.x * SCAN_THREADS;
  const unsigned d_row = stride / nv, d_c = stride - d_row * nv;  // one grid stride in (rows, chunks)
  unsigned g = blockIdx.x * SCAN_THREADS + threadIdx.x;
  unsigned row = g / nv, c = g - row * nv;
  scan_acc a = {0u, 0u, 0u, 0u};
  while (g < total) {
    u32x4_t v[4];
    bool live[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // four independent 16-byte loads before any of them is looked at
      live[u] = g < total;
      if (live[u]) {
        const int col = p.col0 + (int)c * 8;
        v[u] = *(const u32x4_t*)(p.hi + (size_t)row * (size_t)p.ld + (ILV ? ilv32_col(col) : col));
      }
      const unsigned left = total - min(g, total);
      g = left > stride ? g + stride : total;  // (no wrap of g near 2^32)
      row += d_row;
      c += d_c;
      if (c >= nv) {
        c -= nv;
        ++row;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (live[u]) scan_chunk(v[u], a);
  }
  a.max_bits = wave_max_u32(a.max_bits);
  a.n_sat = wave_sum(a.n_sat);
  a.n_nonfinite = wave_sum(a.n_nonfinite);
  a.n_scanned = wave_sum(a.n_scanned);
  __shared__ unsigned part[SCAN_THREADS / 64][4];
  const unsigned wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) {
    part[wave][0] = a.max_bits;
    part[wave][1] = a.n_sat;
    part[wave][2] = a.n_nonfinite;
    part[wave][3] = a.n_scanned;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned m = 0u, s = 0u, n = 0u, k = 0u;
#pragma unroll
    for (unsigned w = 0; w < SCAN_THREADS / 64; ++w) {
      m = max(m, part[w][0]);
      s += part[w][1];
      n += part[w][2];
      k += part[w][3];
    }
    atomicMax(p.record + 0, m);
    if (s) atomicAdd(p.record + 1, s);
    if (n) atomicAdd(p.record + 2, n);
    atomicAdd(p.record + 3, k);  // (wraps mod 2^32)
  }
}

}  // namespace

extern "C" int mvp_f16_range_scan(const mvp_f16_scan_args* a, void* stream) {
  if (!a || !a->hi || !a->record) return MVP_EINVAL;
  if (a->layout != MVP_PAIR_SEPARATE && a->layout != MVP_PAIR_A_ILV32) return MVP_EINVAL;
  if (a->rows < 1 || a->cols < 8 || a->col0 < 0 || a->ld < 8) return MVP_EINVAL;
  if ((a->col0 | a->cols | a->ld) & 7) return MVP_EINVAL;  // every chunk is one aligned 16-byte load
  if (((uintptr_t)a->hi & 15) || ((uintptr_t)a->record & 3)) return MVP_EINVAL;
  // the last word read of a row must lie inside it (interleaved: hi of columns 32 b .. 32 b + 31 sits at words 64 b .. 64 b + 31)
  const int64_t last = (int64_t)a->col0 + a->cols - 8;
  const int64_t end = (a->layout == MVP_PAIR_A_ILV32 ? ((last >> 5) << 6) + (last & 31) : last) + 8;
  if (end > (int64_t)a->ld) return MVP_EINVAL;
  const int64_t total = (int64_t)a->rows * (a->cols >> 3);
  if (total >= 0x80000000ll) return MVP_EINVAL;
  const int64_t blocks = (total + SCAN_THREADS - 1) / SCAN_THREADS;
  const dim3 grid((unsigned)(blocks < SCAN_MAX_BLOCKS ? blocks : SCAN_MAX_BLOCKS));
  if (a->layout == MVP_PAIR_A_ILV32)
    hipLaunchKernelGGL(f16_range_scan_kernel<true>, grid, dim3(SCAN_THREADS), 0, (hipStream_t)stream, *a);
  else
    hipLaunchKernelGGL(f16_range_scan_kernel<false>, grid, dim3(SCAN_THREADS), 0, (hipStream_t)stream, *a);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}
