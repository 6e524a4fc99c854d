// The gate of DINOv2's SwiGLU MLP (SwiGLUFFNFused: w3(silu(x1) * x2) with x1 | x2 = w12(x); ViT-g/14), between the two GEMMs:
//   mvp_swiglu_fwd   h12 [M, ld_in] fp32 (gate | value, the w12 GEMM's fp32 output) -> silu(gate) * value as the A operand pair of the w3
//                    GEMM (zero padded to ld_out columns) and / or fp32 [M, H]
// Pointwise and HBM-bound (8 B read, 4 B written per element): a lane owns 8 consecutive columns of one row — two 16-byte loads of the
// gate, two of the value, one 16-byte store per output array — grid-stride over (row, chunk).  No LDS, no atomics, fp32 arithmetic in a
// fixed order: the same inputs give the same bits.
#include "mvp_common.h"

namespace {

// silu(x) = x / (1 + exp2(-x log2 e)): one v_exp_f32 and one v_rcp_f32, the form of quick_gelu (gemm_epilogue.h).  Contraction off and every
// multiply-add spelled out for that function's reason: the same bits from every build.
// The exponent argument is carried as t + r: t = fp32(x * -L_hi), r = the rounding error of that product (one fma, exact) plus x * -L_lo,
// where L_hi + L_lo = log2 e to 48 bits.  Rounding t alone costs |x| 2^-24 ln 2 relative on exp2 — 1.2e-6 at x = -20, twenty roundings — and
// all of it lands on silu where x < 0.  exp2(t + r) = exp2(t) (1 + r ln 2) moves the sigmoid s = 1 / (1 + exp2(t)) by -s (1 - s) r ln 2: one
// more fma on s, which stays 0 where exp2 overflowed (x below about -88.7: s = 0, the result is -0 * value; from about -87.3 down s is
// subnormal and v_rcp_f32 may already have flushed it: the contract is "below about -87 may return +-0") and exact where it underflowed.
// An infinite x has no finite t + r: r is dropped there, so +inf gives +inf and NaN stays NaN, as in the plain form.
__device__ __forceinline__ float silu(float x) {
#pragma clang fp contract(off)
  const float t = x * -1.44269502162933349609375f;
  float r = __builtin_fmaf(x, -1.44269502162933349609375f, -t);
  r = __builtin_fmaf(x, -1.92596299112661746e-8f, r);
  r = __builtin_fabsf(x) < __builtin_inff() ? r : 0.f;
  const float e = __builtin_amdgcn_exp2f(t);
  const float s = __builtin_amdgcn_rcpf(1.0f + e);
  const float c = s * (1.0f - s);
  const float s2 = __builtin_fmaf(c, r * -0.693147182464599609375f, s);
  return x * s2;
}

__device__ __forceinline__ float gate_mul(float g, float v) {
#pragma clang fp contract(off)
  return silu(g) * v;
}

// A lane per 8 consecutive columns of the ld_out-wide output row; chunks at or beyond H are the zero padding of the pair.
__global__ __launch_bounds__(256) void swiglu_kernel(const mvp_swiglu_args p) {
  f16_saturate_mode();
  const unsigned nv = (unsigned)p.ld_out >> 3;
  const unsigned total = (unsigned)p.M * nv;  // < 2^31: checked by the launcher
  for (unsigned g = blockIdx.x * 256u + threadIdx.x; g < total; g += gridDim.x * 256u) {
    const unsigned row = g / nv;
    const int c0 = (int)(g - row * nv) * 8;
    const bool live = c0 < p.H;
    float y[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (live) {
      const float* in = p.h12 + (size_t)row * p.ld_in + c0;
      const float4 g0 = *(const float4*)in, g1 = *(const float4*)(in + 4);
      const float4 v0 = *(const float4*)(in + p.H), v1 = *(const float4*)(in + p.H + 4);
      y[0] = gate_mul(g0.x, v0.x);
      y[1] = gate_mul(g0.y, v0.y);
      y[2] = gate_mul(g0.z, v0.z);
      y[3] = gate_mul(g0.w, v0.w);
      y[4] = gate_mul(g1.x, v1.x);
      y[5] = gate_mul(g1.y, v1.y);
      y[6] = gate_mul(g1.z, v1.z);
      y[7] = gate_mul(g1.w, v1.w);
    }
    if (p.out_hi) {
      uint32_t h[4] = {0u, 0u, 0u, 0u}, l[4] = {0u, 0u, 0u, 0u};
      if (live) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (p.out_f16) split2_f16_comp(y[2 * e], y[2 * e + 1], h[e], l[e]);
          else split2_bf16(y[2 * e], y[2 * e + 1], h[e], l[e]);
        }
      }
      if (p.out_layout == MVP_PAIR_A_ILV32) {  // one array, hi | lo interleaved per 32 columns (an 8-column chunk never straddles a block)
        const size_t oi = (size_t)row * 2 * p.ld_out + ilv32_col(c0);
        *(u32x4_t*)(p.out_hi + oi) = u32x4_t{h[0], h[1], h[2], h[3]};
        *(u32x4_t*)(p.out_hi + oi + 32) = u32x4_t{l[0], l[1], l[2], l[3]};
      } else {
        const size_t o = (size_t)row * p.ld_out + c0;
        *(u32x4_t*)(p.out_hi + o) = u32x4_t{h[0], h[1], h[2], h[3]};
        if (p.out_lo) *(u32x4_t*)(p.out_lo + o) = u32x4_t{l[0], l[1], l[2], l[3]};
      }
    }
    if (p.out_f32 && live) {
      float* o = p.out_f32 + (size_t)row * p.H + c0;
      *(float4*)o = make_float4(y[0], y[1], y[2], y[3]);
      *(float4*)(o + 4) = make_float4(y[4], y[5], y[6], y[7]);
    }
  }
}

}  // namespace

extern "C" int mvp_swiglu_fwd(const mvp_swiglu_args* a, void* stream) {
  if (!a || !a->h12 || (!a->out_hi && !a->out_f32) || (a->out_lo && !a->out_hi)) return MVP_EINVAL;
  if (a->M < 1 || a->H < 8 || (a->H & 7)) return MVP_EINVAL;
  if (a->ld_in < 0 || (int64_t)a->ld_in < 2 * (int64_t)a->H || (a->ld_in & 3)) return MVP_EINVAL;  // 16-byte loads of both halves
  if (a->out_layout != MVP_PAIR_SEPARATE && a->out_layout != MVP_PAIR_A_ILV32) return MVP_EINVAL;
  if (a->out_f16 != 0 && a->out_f16 != 1) return MVP_EINVAL;
  if (a->ld_out < a->H || (a->ld_out & (a->out_layout == MVP_PAIR_A_ILV32 ? 31 : 7))) return MVP_EINVAL;
  // the second half of the pair may be left out only where one bf16 product reads it (MVP_PREC_BF16): the fp16 pair is one operand
  if (a->out_hi && a->out_layout == MVP_PAIR_SEPARATE && a->out_f16 && !a->out_lo) return MVP_EINVAL;
  if (((uintptr_t)a->h12 | (uintptr_t)a->out_hi | (uintptr_t)a->out_lo | (uintptr_t)a->out_f32) & 15) return MVP_EINVAL;
  const int64_t total = (int64_t)a->M * (a->ld_out >> 3);
  if (total >= 0x80000000ll) return MVP_EINVAL;
  const int64_t blocks = (total + 255) / 256;
  // memory-bound: at most 8 workgroups per CU of a 256-CU device, the rest by the grid stride
  hipLaunchKernelGGL(swiglu_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, (hipStream_t)stream, *a);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}
