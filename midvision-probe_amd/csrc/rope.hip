// 2-D rotary position embedding of the fused qkv projection (CroCo v2's RoPE100; include/mvp_hip.h, mvp_rope2d_qkv):
//   fp32 [M, 3*H*64] (the qkv GEMM's out_f32 form)  ->  the 16-bit pair buffer the attention kernel reads, Q and K rotated by the
//   token's (y, x) grid position, V passed through, every third in the pair form the qkv GEMM's epilogue would have written.
// HBM-bound (4 B read + 4 B written per value), no LDS, no atomics, no state: a thread owns 4 consecutive d of one 32-wide half of a
// head and their partners at d + 16 — two 16-byte loads, two 8-byte stores per output array; the cos / sin rows (128 B each) hit in cache.
// Positions come from the row index alone (t = m % N): no index array in device memory, so no table read can leave the table once the
// host has checked tab_rows >= max(gh, gw).
#include "mvp_common.h"

namespace {

// out[d] = t[d] c - t[d+16] s  (d < 16),  out[d+16] = t[d+16] c' + t[d] s'.  Separate multiplies and one add / subtract each, contraction
// off: what torch's (tokens * cos) + (rotate_half(tokens) * sin) computes in fp32, so a host can reproduce the bits.
__device__ __forceinline__ float rope_first(float t, float tp, float c, float s) {
#pragma clang fp contract(off)
  const float tc = t * c, ts = tp * s;
  return tc - ts;
}
__device__ __forceinline__ float rope_second(float t, float tp, float c, float s) {
#pragma clang fp contract(off)
  const float tc = t * c, ts = tp * s;
  return tc + ts;
}

// f16_col0: the qkv GEMM's out_f16_col0 for the same (precision, v_format) — one definition of "which form does column c take"
// (out_pair_form) and of each form (split2_form), shared with the GEMM epilogues (mvp_common.h).
__global__ __launch_bounds__(256) void rope2d_qkv_kernel(const mvp_rope2d_qkv_args p, const int f16_col0, const unsigned total) {
  f16_saturate_mode();  // (the fp16 forms saturate instead of overflowing, as in the GEMM epilogues)
  const unsigned i = blockIdx.x * 256u + threadIdx.x;  // (total < 2^31, host check: 32-bit index arithmetic, 64-bit addresses)
  if (i >= total) return;
  const unsigned per_row = 24u * p.H;  // 3 * H * 2 halves of 32 columns, 4 threads each
  const int m = (int)(i / per_row), r = (int)(i - (unsigned)m * per_row);
  const int chunk = r >> 2, d0 = (r & 3) << 2;  // chunk: 32-wide half (even = y half of a head, odd = x half); d0 in {0, 4, 8, 12}
  const int col = chunk * 32 + d0;
  const float* src = p.qkv + (size_t)m * p.ld_in + col;
  const float4 a4 = *(const float4*)src, b4 = *(const float4*)(src + 16);
  float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};  // t[d0 ..], t[d0 + 16 ..]
  const int t = m % p.N;
  if (chunk < 4 * p.H && t >= p.n_prefix) {  // Q and K thirds of a grid token (V and the prefix rows pass through)
    const int pp = t - p.n_prefix, y = pp / p.gw;
    const int pos = (chunk & 1) ? pp - y * p.gw : y;  // < gh or < gw <= tab_rows (host check)
    const float* ct = p.cos_tab + (size_t)pos * 32 + d0;
    const float* st = p.sin_tab + (size_t)pos * 32 + d0;
    const float4 c0 = *(const float4*)ct, c1 = *(const float4*)(ct + 16), s0 = *(const float4*)st, s1 = *(const float4*)(st + 16);
    const float ca[4] = {c0.x, c0.y, c0.z, c0.w}, cb[4] = {c1.x, c1.y, c1.z, c1.w};
    const float sa[4] = {s0.x, s0.y, s0.z, s0.w}, sb[4] = {s1.x, s1.y, s1.z, s1.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float lo = rope_first(a[e], b[e], ca[e], sa[e]), hi = rope_second(b[e], a[e], cb[e], sb[e]);
      a[e] = lo;
      b[e] = hi;
    }
  }
  const int form = out_pair_form(f16_col0, col);  // (every form boundary is a multiple of 64: the same form at col and col + 16)
  uint32_t h01, l01, h23, l23;
  const size_t o = (size_t)m * p.ld_out + col;
  split2_form(form, a[0], a[1], h01, l01);
  split2_form(form, a[2], a[3], h23, l23);
  *(u32x2_t*)(p.out_hi + o) = u32x2_t{h01, h23};
  if (p.out_lo) *(u32x2_t*)(p.out_lo + o) = u32x2_t{l01, l23};
  split2_form(form, b[0], b[1], h01, l01);
  split2_form(form, b[2], b[3], h23, l23);
  *(u32x2_t*)(p.out_hi + o + 16) = u32x2_t{h01, h23};
  if (p.out_lo) *(u32x2_t*)(p.out_lo + o + 16) = u32x2_t{l01, l23};
}

}  // namespace

extern "C" int mvp_rope2d_qkv(const mvp_rope2d_qkv_args* a, void* stream) {
  if (!a || !a->qkv || !a->out_hi || !a->cos_tab || !a->sin_tab) return MVP_EINVAL;
  if (a->precision != MVP_PREC_BF16 && a->precision != MVP_PREC_BF16X3) return MVP_EINVAL;
  if (a->precision == MVP_PREC_BF16X3 && !a->out_lo) return MVP_EINVAL;
  if (a->v_format < MVP_ATT_V_BF16_PAIR || a->v_format > MVP_ATT_V_F16_QK_F16) return MVP_EINVAL;
  if (a->v_format != MVP_ATT_V_BF16_PAIR && a->precision != MVP_PREC_BF16X3) return MVP_EINVAL;
  if (a->M <= 0 || a->N <= 0 || a->H <= 0 || a->n_prefix < 0 || a->gh <= 0 || a->gw <= 0) return MVP_EINVAL;
  if (a->M % a->N != 0 || (int64_t)a->N != (int64_t)a->n_prefix + (int64_t)a->gh * a->gw) return MVP_EINVAL;
  if (a->tab_rows < (a->gh > a->gw ? a->gh : a->gw)) return MVP_EINVAL;
  const int64_t C3 = 3 * (int64_t)a->H * 64;
  if (a->ld_in < C3 || a->ld_out < C3) return MVP_EINVAL;
  // 16-byte aligned rows: fp32 input (ld_in % 4), 16-bit outputs (ld_out % 8), the tables' 128-byte rows
  if (((size_t)a->qkv & 15) || (a->ld_in & 3) || ((size_t)a->out_hi & 15) || ((size_t)a->out_lo & 15) || (a->ld_out & 7)) return MVP_EINVAL;
  if (((size_t)a->cos_tab & 15) || ((size_t)a->sin_tab & 15)) return MVP_EINVAL;
  mvp_rope2d_qkv_args k = *a;
  if (k.precision == MVP_PREC_BF16) k.out_lo = nullptr;  // one bf16 product: only hi is written
  const int v0 = 2 * a->H * 64;  // first column of the V third
  const int f16_col0 = a->v_format == MVP_ATT_V_F16 ? v0 : a->v_format == MVP_ATT_V_F16_QK_F16 ? -v0 : 0;
  const int64_t total = (int64_t)a->M * 24 * a->H;
  if (total > 0x7fffffffll) return MVP_EINVAL;  // one thread per 8 values, indexed in 32 bits (M < 7.4 M rows at H = 12)
  hipLaunchKernelGGL(rope2d_qkv_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, k, f16_col0, (unsigned)total);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}
