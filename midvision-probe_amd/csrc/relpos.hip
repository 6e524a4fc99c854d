// SAM's decomposed relative-position terms (include/mvp_hip.h, mvp_relpos_terms):
//   fp32 [M, 3*H*64] (the qkv GEMM's out_f32 form)  ->  (1) rel[(b, h)][q][0 .. Kh + Kw): the dot products of the UNSCALED q with the
//   row yq of Rh and the row xq of Rw, fp32 fma over d = 0 .. 63;  (2) the 16-bit pair buffer the attention kernel reads, every third in
//   the pair form the qkv GEMM's epilogue would have written (the conversion of mvp_rope2d_qkv, through the same helpers of mvp_common.h).
// One workgroup per row m.  Phase 1: every thread converts 4-column pieces of the row; the Q third also goes to LDS (H * 64 floats).
// Phase 2: output o = h * (Kh + Kw) + j per thread: 16 float4 loads of one 256-byte table row against q[h] from LDS (a broadcast
// within a head).  The tables (Rh[yq]: Kh * 256 B, Rw[xq]: Kw * 256 B) are shared by all heads and by the rows of a grid line: L2 traffic.
// Positions come from the row index alone (q = m % N, yq = q / Qw, xq = q % Qw with Qh * Qw == N checked on the host): no table read
// can leave the tables.
#include "mvp_common.h"

namespace {

__global__ __launch_bounds__(256) void relpos_terms_kernel(const mvp_relpos_terms_args p, const int f16_col0) {
  f16_saturate_mode();
  extern __shared__ __attribute__((aligned(16))) float qs[];  // [H * 64]
  const int m = blockIdx.x, C = p.H * 64;
  const float* src = p.qkv + (size_t)m * p.ld_in;
  for (int col = threadIdx.x * 4; col < 3 * C; col += 1024) {
    const float4 v = *(const float4*)(src + col);
    if (col < C) *(float4*)(qs + col) = v;
    const int form = out_pair_form(f16_col0, col);
    uint32_t h01, l01, h23, l23;
    split2_form(form, v.x, v.y, h01, l01);
    split2_form(form, v.z, v.w, h23, l23);
    const size_t o = (size_t)m * p.ld_out + col;
    *(u32x2_t*)(p.out_hi + o) = u32x2_t{h01, h23};
    if (p.out_lo) *(u32x2_t*)(p.out_lo + o) = u32x2_t{l01, l23};
  }
  __syncthreads();
  const int b = m / p.N, q = m - b * p.N;
  const int yq = q / p.Qw, xq = q - yq * p.Qw;  // yq < Qh: Qh * Qw == N (host check)
  const int K = p.Kh + p.Kw;
  const float* rh = p.rh + (size_t)yq * p.Kh * 64;
  const float* rw = p.rw + (size_t)xq * p.Kw * 64;
  for (int o = threadIdx.x; o < p.H * K; o += 256) {
    const int h = o / K, j = o - h * K;
    const float* t = j < p.Kh ? rh + (size_t)j * 64 : rw + (size_t)(j - p.Kh) * 64;
    const float* qh = qs + h * 64;
    float acc = 0.f;
#pragma unroll
    for (int d = 0; d < 64; d += 4) {
      const float4 tv = *(const float4*)(t + d), qv = *(const float4*)(qh + d);
      acc = __builtin_fmaf(qv.x, tv.x, acc);
      acc = __builtin_fmaf(qv.y, tv.y, acc);
      acc = __builtin_fmaf(qv.z, tv.z, acc);
      acc = __builtin_fmaf(qv.w, tv.w, acc);
    }
    p.rel[(size_t)(b * p.H + h) * (size_t)p.rel_bh_stride + (size_t)q * p.ld_rel + j] = acc;
  }
}

}  // namespace

extern "C" int mvp_relpos_terms(const mvp_relpos_terms_args* a, void* stream) {
  if (!a || !a->qkv || !a->out_hi || !a->rel || !a->rh || !a->rw) return MVP_EINVAL;
  if (a->precision != MVP_PREC_BF16 && a->precision != MVP_PREC_BF16X3) return MVP_EINVAL;
  if (a->precision == MVP_PREC_BF16X3 && !a->out_lo) return MVP_EINVAL;
  if (a->v_format < MVP_ATT_V_BF16_PAIR || a->v_format > MVP_ATT_V_F16_QK_F16) return MVP_EINVAL;
  if (a->v_format != MVP_ATT_V_BF16_PAIR && a->precision != MVP_PREC_BF16X3) return MVP_EINVAL;
  if (a->M <= 0 || a->N <= 0 || a->H <= 0 || a->Qh <= 0 || a->Qw <= 0 || a->Kh <= 0 || a->Kw <= 0) return MVP_EINVAL;
  if (a->M % a->N != 0 || (int64_t)a->Qh * a->Qw != (int64_t)a->N) return MVP_EINVAL;
  const int64_t C3 = 3 * (int64_t)a->H * 64;
  if (a->ld_in < C3 || a->ld_out < C3) return MVP_EINVAL;
  if ((int64_t)a->ld_rel < (int64_t)a->Kh + a->Kw || (a->ld_rel & 3) || a->rel_bh_stride < (int64_t)a->N * a->ld_rel) return MVP_EINVAL;
  if (a->H > 256) return MVP_EINVAL;  // the Q row in LDS: H * 256 bytes <= 64 KiB
  // 16-byte aligned rows: fp32 input (ld_in % 4), 16-bit outputs (ld_out % 8), the tables' 256-byte rows; rel is written one float at a time
  if (((size_t)a->qkv & 15) || (a->ld_in & 3) || ((size_t)a->out_hi & 15) || ((size_t)a->out_lo & 15) || (a->ld_out & 7)) return MVP_EINVAL;
  if (((size_t)a->rh & 15) || ((size_t)a->rw & 15) || ((size_t)a->rel & 15)) return MVP_EINVAL;
  mvp_relpos_terms_args k = *a;
  if (k.precision == MVP_PREC_BF16) k.out_lo = nullptr;  // one bf16 product: only hi is written
  const int v0 = 2 * a->H * 64;  // first column of the V third
  const int f16_col0 = a->v_format == MVP_ATT_V_F16 ? v0 : a->v_format == MVP_ATT_V_F16_QK_F16 ? -v0 : 0;
  hipLaunchKernelGGL(relpos_terms_kernel, dim3((unsigned)a->M), dim3(256), (size_t)a->H * 64 * sizeof(float), (hipStream_t)stream, k, f16_col0);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}
