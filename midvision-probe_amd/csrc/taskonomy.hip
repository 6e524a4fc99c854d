// The task-specific ends of Taskonomy probing (reference: evals/datasets/transforms.py task_transform / make_valid_mask,
// evals/utils/losses.py:77-94 MaskedL1Loss, evals/utils/metrics.py:580-739 the curvature and reshading metrics):
//   mvp_task_prepare        raw uint8 / uint16 target + raw uint8 mask -> fp32 [B, Ct, H, W] target and the 0 / 1 valid mask
//   mvp_masked_l1_fwd_bwd   sum valid |pred - target| / sum valid, and its gradient
//   mvp_task_metrics        per image and channel: sum of AbsRel, valid pixels, pixels under three ratio thresholds
// All three stream their operands once (the loss twice: the count is known only after the first pass) and are bound by memory.
// Every reduction is per-workgroup fp64 partials in the caller's workspace, folded in a fixed order (no float atomics;
// csrc/mvp_reduce.h): the same inputs give the same bits.  Counts are carried in fp64, exact below 2^53.
// The metric arithmetic reproduces a chain of separately rounded fp32 tensor operations: no contraction anywhere in this file.
#pragma clang fp contract(off)
#include "mvp_reduce.h"

namespace {

constexpr int TK_NB = MVP_TASK_WORKSPACE_BYTES / (5 * 8);  // 1024: partial rows at most (5 fp64 each for the metrics, 2 for the loss)

// ----------------------------------------------------------------------------- target + valid mask
// k / 255 or k / 65535 (correctly rounded), then the task's clamp_to (0, maxx): min(max(x, 0), maxx) / maxx
__device__ __forceinline__ float tk_value(unsigned k, float den, float maxx) {
  float x = __fdiv_rn((float)k, den);
  if (maxx > 0.f) x = __fdiv_rn(fminf(fmaxf(x, 0.f), maxx), maxx);
  return x;
}

// Any shape: one pixel per thread, 16 byte loads of the mask block its index map names.
__global__ __launch_bounds__(256) void prepare_any_kernel(const mvp_task_prepare_args p) {
  const int hp = p.H >> 2, wp = p.W >> 2;
  const int64_t HW = (int64_t)p.H * p.W, P = (int64_t)p.B * HW;
  const float den = p.bits == 8 ? 255.f : 65535.f;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < P; r += (int64_t)gridDim.x * 256) {
    const int64_t b = r / HW, i = r - b * HW;
    const int y = (int)(i / p.W), x = (int)(i - (int64_t)y * p.W);
    const int bi = (int)(((int64_t)y * hp) / p.H), bj = (int)(((int64_t)x * wp) / p.W);  // < hp, < wp: rows 4 bi + 3 < H, columns 4 bj + 3 < W
    const uint8_t* m = p.mask_raw + b * HW + (int64_t)(4 * bi) * p.W + 4 * bj;
    bool ok = true;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) ok = ok && m[(int64_t)rr * p.W + cc] == 255;
    p.valid[r] = ok ? 1 : 0;
    for (int c = 0; c < p.Ct; ++c) {
      const unsigned k = p.bits == 8 ? ((const uint8_t*)p.target_raw)[r * p.Cs + c] : ((const uint16_t*)p.target_raw)[r];
      p.target[(b * p.Ct + c) * HW + i] = tk_value(k, den, p.clamp_max);
    }
  }
}

// H % 4 == 0, W % 4 == 0, aligned bases: the index map is (y / 4, x / 4), so four pixels of one row share a mask block.  Per thread: four
// 4-byte mask loads, CS words (8-bit, 4 pixels x CS channels) or 8 bytes (16-bit) of raw target, one 4-byte mask store, one 16-byte
// store per kept channel.  CS = 0: the 16-bit form.
template <int CS>
__global__ __launch_bounds__(256) void prepare_v4_kernel(const mvp_task_prepare_args p) {
  const int W4 = p.W >> 2;
  const int64_t HW = (int64_t)p.H * p.W, Q = (int64_t)p.B * (HW >> 2);
  const float den = CS ? 255.f : 65535.f;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < Q; q += (int64_t)gridDim.x * 256) {
    const int64_t b = q / (HW >> 2), iq = q - b * (HW >> 2);
    const int y = (int)(iq / W4), xq = (int)(iq - (int64_t)y * W4);
    const uint8_t* m = p.mask_raw + b * HW + (int64_t)(y & ~3) * p.W + 4 * xq;
    uint32_t all = 0xffffffffu;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) all &= *(const uint32_t*)(m + (int64_t)rr * p.W);
    const int64_t r = q << 2;  // first of the four pixels
    *(uint32_t*)(p.valid + r) = all == 0xffffffffu ? 0x01010101u : 0u;
    unsigned k[4][4];  // [pixel][channel]
    if (CS) {
      constexpr int NW = CS ? CS : 1;
      uint32_t w[NW];
#pragma unroll
      for (int j = 0; j < NW; ++j) w[j] = ((const uint32_t*)p.target_raw)[q * NW + j];
#pragma unroll
      for (int px = 0; px < 4; ++px)
#pragma unroll
        for (int c = 0; c < NW; ++c) {
          const int e = px * NW + c;
          k[px][c] = (w[e >> 2] >> (8 * (e & 3))) & 255u;
        }
    } else {
      const uint2 w = ((const uint2*)p.target_raw)[q];
      k[0][0] = w.x & 0xffffu; k[1][0] = w.x >> 16; k[2][0] = w.y & 0xffffu; k[3][0] = w.y >> 16;
    }
    const int64_t i = r - b * HW;
#pragma unroll
    for (int c = 0; c < (CS ? CS : 1); ++c) {
      if (c < p.Ct) {
        float4 o;
        o.x = tk_value(k[0][c], den, p.clamp_max);
        o.y = tk_value(k[1][c], den, p.clamp_max);
        o.z = tk_value(k[2][c], den, p.clamp_max);
        o.w = tk_value(k[3][c], den, p.clamp_max);
        *(float4*)(p.target + (b * p.Ct + c) * HW + i) = o;
      }
    }
  }
}

// ----------------------------------------------------------------------------- rows of [B, C, HW] against a [B, Cm, HW] mask
// grid (gx, gy): workgroup (bx, by) takes elements [bx * per, bx * per + per) of rows by, by + gy, ...; per % 4 == 0.
struct RowPart { int gx, gy; int64_t per; };

inline RowPart row_partition(int64_t R, int64_t HW) {
  RowPart q;
  q.gy = (int)(R < TK_NB ? R : TK_NB);
  int64_t gx = (HW + 4095) / 4096;  // 4 x 16 bytes of each fp32 operand per thread
  const int64_t cap = TK_NB / q.gy;
  gx = gx < 1 ? 1 : (gx > cap ? cap : gx);
  q.per = (((HW + gx - 1) / gx) + 3) & ~(int64_t)3;
  q.gx = (int)((HW + q.per - 1) / q.per);
  return q;
}

// ----------------------------------------------------------------------------- masked L1
__device__ __forceinline__ void l1_acc(float a, float t, uint32_t m, double (&acc)[2]) {
  if (m) {  // a select: what lies under an invalid pixel never enters the sum
    acc[0] += fabs((double)a - (double)t);  // exact difference of two fp32 values
    acc[1] += 1.0;
  }
}

template <bool V4>
__global__ __launch_bounds__(256) void l1_reduce_kernel(const mvp_masked_l1_args p, const int64_t per) {
  __shared__ double red[4][2];
  const int64_t R = (int64_t)p.B * p.C;
  const int64_t i0 = (int64_t)blockIdx.x * per, i1 = min(p.HW, i0 + per);
  double acc[2] = {0.0, 0.0};
  for (int64_t row = blockIdx.y; row < R; row += gridDim.y) {
    const float* pr = p.pred + row * p.HW;
    const float* tg = p.target + row * p.HW;
    const uint8_t* vm = p.valid + (p.Cm == p.C ? row : row / p.C) * p.HW;
    if (V4) {
      for (int64_t v = (i0 >> 2) + threadIdx.x; v < (i1 >> 2); v += 256) {
        const float4 a = ((const float4*)pr)[v], t = ((const float4*)tg)[v];
        const uint32_t m = ((const uint32_t*)vm)[v];
        l1_acc(a.x, t.x, m & 0xffu, acc);
        l1_acc(a.y, t.y, m & 0xff00u, acc);
        l1_acc(a.z, t.z, m & 0xff0000u, acc);
        l1_acc(a.w, t.w, m & 0xff000000u, acc);
      }
    } else {
      for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) l1_acc(pr[i], tg[i], vm[i], acc);
    }
  }
  block_sum<2>(acc, red);
  if (threadIdx.x == 0) {
    double* ws = (double*)p.workspace + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
    ws[0] = acc[0];
    ws[1] = acc[1];
  }
}

__device__ __forceinline__ float l1_grad(float a, float t, uint32_t m, float inv) {
  const float s = a > t ? inv : (a < t ? -inv : 0.f);  // sign(0) = 0
  return m ? s : 0.f;
}

// nb partial rows of l1_reduce_kernel; launched on the same grid (one workgroup when there is no gradient to write)
template <bool V4>
__global__ __launch_bounds__(256) void l1_apply_kernel(const mvp_masked_l1_args p, const int64_t per, const int nb) {
  __shared__ double red[4][2];
  // every workgroup folds the partial rows itself, in the same fixed order: the same count everywhere
  double acc[2];
  fold_rows<2>((const double*)p.workspace, nb, 2, acc, red);
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) p.loss[0] = (float)(acc[0] / acc[1]);  // no valid pixel: 0 / 0
  if (!p.grad_pred) return;
  const float inv = (float)(1.0 / acc[1]);
  const int64_t R = (int64_t)p.B * p.C;
  const int64_t i0 = (int64_t)blockIdx.x * per, i1 = min(p.HW, i0 + per);
  for (int64_t row = blockIdx.y; row < R; row += gridDim.y) {
    const float* pr = p.pred + row * p.HW;
    const float* tg = p.target + row * p.HW;
    float* gr = p.grad_pred + row * p.HW;
    const uint8_t* vm = p.valid + (p.Cm == p.C ? row : row / p.C) * p.HW;
    if (V4) {
      for (int64_t v = (i0 >> 2) + threadIdx.x; v < (i1 >> 2); v += 256) {
        const float4 a = ((const float4*)pr)[v], t = ((const float4*)tg)[v];
        const uint32_t m = ((const uint32_t*)vm)[v];
        float4 g;
        g.x = l1_grad(a.x, t.x, m & 0xffu, inv);
        g.y = l1_grad(a.y, t.y, m & 0xff00u, inv);
        g.z = l1_grad(a.z, t.z, m & 0xff0000u, inv);
        g.w = l1_grad(a.w, t.w, m & 0xff000000u, inv);
        ((float4*)gr)[v] = g;
      }
    } else {
      for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) gr[i] = l1_grad(pr[i], tg[i], vm[i], inv);
    }
  }
}

// ----------------------------------------------------------------------------- AbsRel and threshold counts
// torch.max(a, b): NaN when either operand is (fmaxf would drop it)
__device__ __forceinline__ float nan_max(float a, float b) {
  return (a != a || b != b) ? __builtin_nanf("") : (a > b ? a : b);
}

// FORM 0: curvature (metrics.py:580-678); FORM 1: reshading (:681-739).  One rounding per fp32 tensor operation of the reference.
template <int FORM>
__device__ __forceinline__ void tm_acc(float pred, float gt, uint32_t vb, float t1, float t2, float t3, double (&acc)[5]) {
  const float m = vb ? 1.f : 0.f;
  float absrel, ratio;
  if (FORM == 0) {
    const float q = pred < -1.f ? -1.f : (pred > 1.f ? 1.f : pred);  // torch.clamp: NaN stays NaN
    absrel = __fdiv_rn(fabsf(__fsub_rn(q, gt)), fabsf(__fadd_rn(gt, 1e-6f)));
    ratio = nan_max(__fdiv_rn(q, gt), __fdiv_rn(gt, q));
  } else {
    const float q = __fmul_rn(pred, m), t = __fmul_rn(gt, m);  // a product: a non-finite value under the mask stays non-finite
    absrel = __fdiv_rn(fabsf(__fsub_rn(q, t)), __fadd_rn(t, 1e-6f));
    ratio = nan_max(__fdiv_rn(q, __fadd_rn(t, 1e-6f)), __fdiv_rn(t, __fadd_rn(q, 1e-6f)));
  }
  acc[0] += (double)__fmul_rn(absrel, m);  // multiplied by the mask as the reference does, not selected
  acc[1] += (double)m;
  if (vb) {
    acc[2] += ratio < t1 ? 1.0 : 0.0;
    acc[3] += ratio < t2 ? 1.0 : 0.0;
    acc[4] += ratio < t3 ? 1.0 : 0.0;
  }
}

template <int FORM, bool V4>
__global__ __launch_bounds__(256) void metrics_kernel(const mvp_task_metrics_args p, const int64_t per) {
  __shared__ double red[4][5];
  const int64_t row = blockIdx.y;  // one (image, channel) per grid row
  const int64_t i0 = (int64_t)blockIdx.x * per, i1 = min(p.HW, i0 + per);
  const float* pr = p.pred + row * p.HW;
  const float* tg = p.target + row * p.HW;
  const uint8_t* vm = p.valid + (p.Cm == p.C ? row : row / p.C) * p.HW;
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (V4) {
    for (int64_t v = (i0 >> 2) + threadIdx.x; v < (i1 >> 2); v += 256) {
      const float4 a = ((const float4*)pr)[v], t = ((const float4*)tg)[v];
      const uint32_t m = ((const uint32_t*)vm)[v];
      tm_acc<FORM>(a.x, t.x, m & 0xffu, p.t1, p.t2, p.t3, acc);
      tm_acc<FORM>(a.y, t.y, m & 0xff00u, p.t1, p.t2, p.t3, acc);
      tm_acc<FORM>(a.z, t.z, m & 0xff0000u, p.t1, p.t2, p.t3, acc);
      tm_acc<FORM>(a.w, t.w, m & 0xff000000u, p.t1, p.t2, p.t3, acc);
    }
  } else {
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) tm_acc<FORM>(pr[i], tg[i], vm[i], p.t1, p.t2, p.t3, acc);
  }
  block_sum<5>(acc, red);
  if (threadIdx.x < 5) ((double*)p.workspace)[(row * gridDim.x + blockIdx.x) * 5 + threadIdx.x] = acc[threadIdx.x];
}

// out[row][k] = the gx partials of the row, first to last
__global__ __launch_bounds__(256) void metrics_fold_kernel(const mvp_task_metrics_args p, const int gx) {
  const int64_t n = (int64_t)p.B * p.C * 5, t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int64_t row = t / 5;
  const int k = (int)(t - row * 5);
  const double* ws = (const double*)p.workspace + row * gx * 5 + k;
  double s = 0.0;
  for (int i = 0; i < gx; ++i) s += ws[i * 5];
  p.out[t] = s;
}

template <int FORM>
void metrics_launch(const mvp_task_metrics_args& a, const RowPart& q, bool v4, hipStream_t s) {
  const dim3 grid((unsigned)q.gx, (unsigned)q.gy);
  if (v4) hipLaunchKernelGGL((metrics_kernel<FORM, true>), grid, dim3(256), 0, s, a, q.per);
  else hipLaunchKernelGGL((metrics_kernel<FORM, false>), grid, dim3(256), 0, s, a, q.per);
}

}  // namespace

extern "C" int mvp_task_prepare(const mvp_task_prepare_args* a, void* stream) {
  if (!a || !a->target_raw || !a->mask_raw || !a->target || !a->valid) return MVP_EINVAL;
  if (a->B <= 0 || a->H < 4 || a->W < 4 || a->Ct < 1 || a->Cs < a->Ct) return MVP_EINVAL;
  if (a->bits != 8 && a->bits != 16) return MVP_EINVAL;
  if (a->bits == 16 && (a->Cs != 1 || !aligned_to(a->target_raw, 2))) return MVP_EINVAL;
  if (!(a->clamp_max >= 0.f)) return MVP_EINVAL;
  const int64_t HW = (int64_t)a->H * a->W;
  if (HW > ((int64_t)1 << 40) / a->B / a->Cs) return MVP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const bool v4 = (a->H & 3) == 0 && (a->W & 3) == 0 && aligned_to(a->mask_raw, 4) && aligned_to(a->valid, 4) && aligned_to(a->target, 16) &&
                  aligned_to(a->target_raw, a->bits == 16 ? 8 : 4) && a->Cs <= 4;
  const int64_t items = v4 ? (int64_t)a->B * (HW >> 2) : (int64_t)a->B * HW;
  int64_t nb = (items + 255) / 256;
  nb = nb > 16384 ? 16384 : nb;
  const dim3 grid((unsigned)nb), blk(256);
  if (!v4) hipLaunchKernelGGL(prepare_any_kernel, grid, blk, 0, s, *a);
  else if (a->bits == 16) hipLaunchKernelGGL(prepare_v4_kernel<0>, grid, blk, 0, s, *a);
  else if (a->Cs == 1) hipLaunchKernelGGL(prepare_v4_kernel<1>, grid, blk, 0, s, *a);
  else if (a->Cs == 2) hipLaunchKernelGGL(prepare_v4_kernel<2>, grid, blk, 0, s, *a);
  else if (a->Cs == 3) hipLaunchKernelGGL(prepare_v4_kernel<3>, grid, blk, 0, s, *a);
  else hipLaunchKernelGGL(prepare_v4_kernel<4>, grid, blk, 0, s, *a);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}

extern "C" int mvp_masked_l1_fwd_bwd(const mvp_masked_l1_args* a, void* stream) {
  if (!a || !a->pred || !a->target || !a->valid || !a->loss || !a->workspace) return MVP_EINVAL;
  if (a->B <= 0 || a->C <= 0 || a->HW <= 0 || (a->Cm != 1 && a->Cm != a->C)) return MVP_EINVAL;
  if (a->HW > ((int64_t)1 << 40) / a->B / a->C) return MVP_EINVAL;
  if (a->workspace_bytes < MVP_TASK_WORKSPACE_BYTES || !aligned_to(a->workspace, 8)) return MVP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const RowPart q = row_partition((int64_t)a->B * a->C, a->HW);
  const bool v4 = (a->HW & 3) == 0 && aligned_to(a->pred, 16) && aligned_to(a->target, 16) && aligned_to(a->grad_pred, 16) && aligned_to(a->valid, 4);
  const dim3 grid((unsigned)q.gx, (unsigned)q.gy), one(1, 1);
  const int nb = q.gx * q.gy;
  if (v4) {
    hipLaunchKernelGGL(l1_reduce_kernel<true>, grid, dim3(256), 0, s, *a, q.per);
    hipLaunchKernelGGL(l1_apply_kernel<true>, a->grad_pred ? grid : one, dim3(256), 0, s, *a, q.per, nb);
  } else {
    hipLaunchKernelGGL(l1_reduce_kernel<false>, grid, dim3(256), 0, s, *a, q.per);
    hipLaunchKernelGGL(l1_apply_kernel<false>, a->grad_pred ? grid : one, dim3(256), 0, s, *a, q.per, nb);
  }
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}

extern "C" int mvp_task_metrics(const mvp_task_metrics_args* a, void* stream) {
  if (!a || !a->pred || !a->target || !a->valid || !a->out || !a->workspace) return MVP_EINVAL;
  if (a->B <= 0 || a->C <= 0 || a->HW <= 0 || (a->Cm != 1 && a->Cm != a->C)) return MVP_EINVAL;
  if ((int64_t)a->B * a->C > TK_NB || a->HW > ((int64_t)1 << 40) / a->B / a->C) return MVP_EINVAL;
  if (a->form != MVP_TASK_METRICS_CURVATURE && a->form != MVP_TASK_METRICS_RESHADING) return MVP_EINVAL;
  if (a->workspace_bytes < MVP_TASK_WORKSPACE_BYTES || !aligned_to(a->workspace, 8) || !aligned_to(a->out, 8)) return MVP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const RowPart q = row_partition((int64_t)a->B * a->C, a->HW);  // gy = B C rows exactly (<= TK_NB)
  const bool v4 = (a->HW & 3) == 0 && aligned_to(a->pred, 16) && aligned_to(a->target, 16) && aligned_to(a->valid, 4);
  if (a->form == MVP_TASK_METRICS_CURVATURE) metrics_launch<0>(*a, q, v4, s);
  else metrics_launch<1>(*a, q, v4, s);
  const int64_t n = (int64_t)a->B * a->C * 5;
  hipLaunchKernelGGL(metrics_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, *a, q.gx);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}
