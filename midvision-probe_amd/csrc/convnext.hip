// ConvNeXt / ConvNeXt V2 block kernels on channels-last fp32 maps (reference: evals/models/convnext.py:87-91 runs timm's blocks;
// the arithmetic is timm's ConvNeXtBlock / transformers' ConvNextLayer and ConvNextV2GRN):
//   mvp_dwconv7_ln_fwd   depthwise 7x7 (stride 1, zero padding 3) + LayerNorm over the channels -> the A operand of fc1
//   mvp_grn_stats        V2's global response normalisation, statistics: G[b, c] = ||h[b, :, c]||_2, N = G / (mean_c G + 1e-6)
//   mvp_grn_apply        gamma (h N) + beta + h -> the A operand of fc2
// fp32 arithmetic in a fixed order everywhere (no atomics): the same inputs give the same bits.  The fp64 mean of GRN: csrc/mvp_reduce.h.
#include "mvp_reduce.h"

namespace {

// ----------------------------------------------------------------------------- depthwise 7x7 + LayerNorm
// A thread owns 8 consecutive channels of DW_TW consecutive pixels of one image row (a "strip"); the C / 8 threads of a strip sit
// side by side, 256 / (C / 8) strips per workgroup, so one workgroup holds every channel of its pixels and the LayerNorm
// reductions stay inside it.  The 49 x C weight table does not fit LDS at C = 1024: a thread reads the 7 taps of one ky row of its 8
// channels into registers (56 values), applies them to the row's DW_TW + 6 input pixels, and moves to the next row.
// (Measured against it, B = 16 at ConvNeXt-B's stage shapes: staging each ky row through LDS once per workgroup, 54 / 36 / 33 / 44 us
// against 62 / 35 / 27 / 20; two ky rows per iteration: no change; 2-pixel strips: 83 / 53 / 40 / 23 us.)
// Taps are summed ky-major, then kx, bias last, whatever the position of the pixel: a tap outside the image contributes
// fma(w, 0, acc) = acc.  Out-of-image taps are never loaded, at the vertical edges of an image inside a batch either.
constexpr int DW_TW = 4;
constexpr int DW_CH = 8;

// The sum over the strip's threads of v[i], for every pixel i of the strip, through LDS: part[(strip * TW + i) * tps + q], then
// tp = 2^k threads per pixel add their share in a fixed order and a butterfly over those tp lanes finishes it.
__device__ __forceinline__ void strip_reduce(float (&v)[DW_TW], float* part, float* stat, int strip, int q, int tps, int npix, int tp,
                                             bool active) {
  __syncthreads();  // the previous round's readers of part / stat are done
  if (active) {
#pragma unroll
    for (int i = 0; i < DW_TW; ++i) part[(strip * DW_TW + i) * tps + q] = v[i];
  }
  __syncthreads();
  const int t = threadIdx.x;
  const int p = t / tp, j = t - p * tp;
  float s = 0.f;
  if (p < npix)
    for (int k = j; k < tps; k += tp) s += part[p * tps + k];
  for (int o = tp >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (p < npix && j == 0) stat[p] = s;
  __syncthreads();
  if (active) {
#pragma unroll
    for (int i = 0; i < DW_TW; ++i) v[i] = stat[strip * DW_TW + i];
  }
}

__global__ __launch_bounds__(256) void dwconv7_ln_kernel(const mvp_dwconv7_ln_args p, const int tps, const int spb, const int tp,
                                                         const int strips_per_row, const long long nstrips) {
  f16_saturate_mode();
  __shared__ float part[256 * DW_TW];
  __shared__ float stat[256];
  const int t = threadIdx.x;
  const int strip = t / tps, q = t - strip * tps;
  const long long sid = (long long)blockIdx.x * spb + strip;
  const bool active = strip < spb && sid < nstrips;
  const int npix = spb * DW_TW;
  const int c0 = q * DW_CH;

  int x0 = 0, y = 0;
  long long b = 0;
  float acc[DW_TW][DW_CH];
#pragma unroll
  for (int i = 0; i < DW_TW; ++i)
#pragma unroll
    for (int e = 0; e < DW_CH; ++e) acc[i][e] = 0.f;

  if (active) {
    const long long rowid = sid / strips_per_row;  // b * H + y
    x0 = (int)(sid - rowid * strips_per_row) * DW_TW;
    b = rowid / p.H;
    y = (int)(rowid - b * p.H);
#pragma unroll 1
    for (int ky = 0; ky < 7; ++ky) {
      const int yi = y + ky - 3;
      const bool row_in = yi >= 0 && yi < p.H;
      float w[DW_CH][7];
#pragma unroll
      for (int e = 0; e < DW_CH; ++e)
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) w[e][kx] = p.weight[(size_t)(c0 + e) * 49 + ky * 7 + kx];
      const float* xrow = p.x + ((size_t)(b * p.H + (row_in ? yi : 0)) * p.W) * p.ldx + c0;
      float in[DW_TW + 6][DW_CH];
#pragma unroll
      for (int j = 0; j < DW_TW + 6; ++j) {
        const int xi = x0 + j - 3;
        float4 u0 = make_float4(0.f, 0.f, 0.f, 0.f), u1 = u0;
        if (row_in && xi >= 0 && xi < p.W) {
          const float4* src = (const float4*)(xrow + (size_t)xi * p.ldx);
          u0 = src[0];
          u1 = src[1];
        }
        in[j][0] = u0.x; in[j][1] = u0.y; in[j][2] = u0.z; in[j][3] = u0.w;
        in[j][4] = u1.x; in[j][5] = u1.y; in[j][6] = u1.z; in[j][7] = u1.w;
      }
#pragma unroll
      for (int kx = 0; kx < 7; ++kx)
#pragma unroll
        for (int i = 0; i < DW_TW; ++i)
#pragma unroll
          for (int e = 0; e < DW_CH; ++e) acc[i][e] = __builtin_fmaf(w[e][kx], in[i + kx][e], acc[i][e]);
    }
    const float4 bv0 = *(const float4*)(p.bias + c0), bv1 = *(const float4*)(p.bias + c0 + 4);
    const float bb[DW_CH] = {bv0.x, bv0.y, bv0.z, bv0.w, bv1.x, bv1.y, bv1.z, bv1.w};
#pragma unroll
    for (int i = 0; i < DW_TW; ++i)
#pragma unroll
      for (int e = 0; e < DW_CH; ++e) acc[i][e] += bb[e];
  }

  // LayerNorm over the channels, two-pass (mean, then the centred sum of squares), as csrc/layernorm.hip
  float s[DW_TW];
#pragma unroll
  for (int i = 0; i < DW_TW; ++i)
    s[i] = ((acc[i][0] + acc[i][1]) + (acc[i][2] + acc[i][3])) + ((acc[i][4] + acc[i][5]) + (acc[i][6] + acc[i][7]));
  strip_reduce(s, part, stat, strip, q, tps, npix, tp, active);
  float mean[DW_TW], qs[DW_TW];
#pragma unroll
  for (int i = 0; i < DW_TW; ++i) {
    mean[i] = s[i] / (float)p.C;
    float d[DW_CH];
#pragma unroll
    for (int e = 0; e < DW_CH; ++e) d[e] = acc[i][e] - mean[i];
    qs[i] = ((d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3])) + ((d[4] * d[4] + d[5] * d[5]) + (d[6] * d[6] + d[7] * d[7]));
  }
  strip_reduce(qs, part, stat, strip, q, tps, npix, tp, active);
  if (!active) return;

  const float4 g0 = *(const float4*)(p.gamma + c0), g1 = *(const float4*)(p.gamma + c0 + 4);
  const float4 e0 = *(const float4*)(p.beta + c0), e1 = *(const float4*)(p.beta + c0 + 4);
  const float gg[DW_CH] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
  const float be[DW_CH] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
#pragma unroll
  for (int i = 0; i < DW_TW; ++i) {
    if (x0 + i >= p.W) break;
    const float rstd = rsqrtf(qs[i] / (float)p.C + p.eps);
    float yv[DW_CH];
#pragma unroll
    for (int e = 0; e < DW_CH; ++e) yv[e] = (acc[i][e] - mean[i]) * rstd * gg[e] + be[e];
    const size_t row = (size_t)(b * p.H + y) * p.W + x0 + i;
    const size_t o = row * p.C + c0;
    if (p.out_hi) {
      uint32_t h[4], l[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (p.out_f16) split2_f16_comp(yv[2 * e], yv[2 * e + 1], h[e], l[e]);
        else split2_bf16(yv[2 * e], yv[2 * e + 1], h[e], l[e]);
      }
      if (p.out_layout == MVP_PAIR_A_ILV32) {  // one array, hi | lo interleaved per 32 columns (an 8-element chunk never straddles a block)
        const size_t oi = row * 2 * p.C + ilv32_col(c0);
        *(u32x4_t*)(p.out_hi + oi) = u32x4_t{h[0], h[1], h[2], h[3]};
        *(u32x4_t*)(p.out_hi + oi + 32) = u32x4_t{l[0], l[1], l[2], l[3]};
      } else {
        *(u32x4_t*)(p.out_hi + o) = u32x4_t{h[0], h[1], h[2], h[3]};
        if (p.out_lo) *(u32x4_t*)(p.out_lo + o) = u32x4_t{l[0], l[1], l[2], l[3]};
      }
    }
    if (p.out_f32) {
      *(float4*)(p.out_f32 + o) = make_float4(yv[0], yv[1], yv[2], yv[3]);
      *(float4*)(p.out_f32 + o + 4) = make_float4(yv[4], yv[5], yv[6], yv[7]);
    }
  }
}

// ----------------------------------------------------------------------------- GRN
constexpr int GRN_ROWS = 64;   // rows of one partial sum at least
constexpr int GRN_SLABS = 64;  // partial sums per (image, channel) at most

__host__ __device__ inline int grn_slabs(int HW) {
  const int s = (HW + GRN_ROWS - 1) / GRN_ROWS;
  return s < 1 ? 1 : (s > GRN_SLABS ? GRN_SLABS : s);
}

// partial[(b * S + s) * C4 + c] = sum over the slab's rows of h^2, fp64, rows in order.  One wave per 256 channels (float4 per lane).
__global__ __launch_bounds__(64) void grn_partial_kernel(const mvp_grn_args p, const int S, double* __restrict__ partial) {
  const int c = (blockIdx.x * 64 + threadIdx.x) * 4;
  if (c >= p.C4) return;
  const int s = blockIdx.y, b = blockIdx.z;
  const int per = (p.HW + S - 1) / S;
  const int r0 = s * per, r1 = min(p.HW, r0 + per);
  const float* h = p.h + ((size_t)b * p.HW) * p.C4 + c;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int r = r0; r < r1; ++r) {
    const float4 v = *(const float4*)(h + (size_t)r * p.C4);
    a0 += (double)v.x * (double)v.x;
    a1 += (double)v.y * (double)v.y;
    a2 += (double)v.z * (double)v.z;
    a3 += (double)v.w * (double)v.w;
  }
  double* o = partial + ((size_t)b * S + s) * p.C4 + c;
  o[0] = a0; o[1] = a1; o[2] = a2; o[3] = a3;
}

// One workgroup per image: G = sqrt(sum of the partials, slabs in order), mean over the channels (fp64, fixed order), N.
__global__ __launch_bounds__(256) void grn_finish_kernel(const mvp_grn_args p, const int S, const double* __restrict__ partial) {
  __shared__ double red[4][1];
  const int b = blockIdx.x, t = threadIdx.x;
  double local[1] = {0.0};
  for (int c = t; c < p.C4; c += 256) {
    double a = 0.0;
    for (int s = 0; s < S; ++s) a += partial[((size_t)b * S + s) * p.C4 + c];
    const float g = (float)sqrt(a);
    p.G[(size_t)b * p.C4 + c] = g;
    local[0] += (double)g;
  }
  block_sum<1>(local, red);
  const double mean = local[0] / (double)p.C4;
  const float den = (float)mean + 1e-6f;
  for (int c = t; c < p.C4; c += 256) p.N[(size_t)b * p.C4 + c] = p.G[(size_t)b * p.C4 + c] / den;  // (this thread wrote G[b, c] itself)
}

// out = gamma (h N) + beta + h as the pair of the next GEMM's A operand; a thread per 8 consecutive channels, grid-stride.
__global__ __launch_bounds__(256) void grn_apply_kernel(const mvp_grn_args p) {
  const int nv = p.C4 >> 3;
  const long long total = (long long)p.B * p.HW * nv;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long long)gridDim.x * 256) {
    const long long row = g / nv;
    const int c0 = (int)(g - row * nv) * 8;
    const int b = (int)(row / p.HW);
    const size_t o = (size_t)row * p.C4 + c0;
    const float4 h0 = *(const float4*)(p.h + o), h1 = *(const float4*)(p.h + o + 4);
    const float4 n0 = *(const float4*)(p.N + (size_t)b * p.C4 + c0), n1 = *(const float4*)(p.N + (size_t)b * p.C4 + c0 + 4);
    const float4 g0 = *(const float4*)(p.gamma + c0), g1 = *(const float4*)(p.gamma + c0 + 4);
    const float4 e0 = *(const float4*)(p.beta + c0), e1 = *(const float4*)(p.beta + c0 + 4);
    float yv[8];
    yv[0] = g0.x * (h0.x * n0.x) + e0.x + h0.x;
    yv[1] = g0.y * (h0.y * n0.y) + e0.y + h0.y;
    yv[2] = g0.z * (h0.z * n0.z) + e0.z + h0.z;
    yv[3] = g0.w * (h0.w * n0.w) + e0.w + h0.w;
    yv[4] = g1.x * (h1.x * n1.x) + e1.x + h1.x;
    yv[5] = g1.y * (h1.y * n1.y) + e1.y + h1.y;
    yv[6] = g1.z * (h1.z * n1.z) + e1.z + h1.z;
    yv[7] = g1.w * (h1.w * n1.w) + e1.w + h1.w;
    if (p.out_hi) {
      uint32_t hh[4], ll[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) split2_bf16(yv[2 * e], yv[2 * e + 1], hh[e], ll[e]);
      if (p.out_layout == MVP_PAIR_A_ILV32) {
        const size_t oi = (size_t)row * 2 * p.C4 + ilv32_col(c0);
        *(u32x4_t*)(p.out_hi + oi) = u32x4_t{hh[0], hh[1], hh[2], hh[3]};
        *(u32x4_t*)(p.out_hi + oi + 32) = u32x4_t{ll[0], ll[1], ll[2], ll[3]};
      } else {
        *(u32x4_t*)(p.out_hi + o) = u32x4_t{hh[0], hh[1], hh[2], hh[3]};
        if (p.out_lo) *(u32x4_t*)(p.out_lo + o) = u32x4_t{ll[0], ll[1], ll[2], ll[3]};
      }
    }
    if (p.out_f32) {
      *(float4*)(p.out_f32 + o) = make_float4(yv[0], yv[1], yv[2], yv[3]);
      *(float4*)(p.out_f32 + o + 4) = make_float4(yv[4], yv[5], yv[6], yv[7]);
    }
  }
}

bool grn_shape_ok(const mvp_grn_args* a) {
  return a && a->B > 0 && a->HW > 0 && a->C4 >= 8 && (a->C4 & 7) == 0 && a->B <= 65535 && (int64_t)a->B * a->HW <= 0x7fffffffll;
}

}  // namespace

extern "C" int mvp_dwconv7_ln_fwd(const mvp_dwconv7_ln_args* a, void* stream) {
  if (!a || !a->x || !a->weight || !a->bias || !a->gamma || !a->beta || (!a->out_hi && !a->out_f32)) return MVP_EINVAL;
  if (a->B <= 0 || a->H <= 0 || a->W <= 0 || a->C < 32 || a->C > 2048 || (a->C & 31)) return MVP_EINVAL;
  if (a->ldx < a->C || (a->ldx & 3)) return MVP_EINVAL;  // 16-byte loads of 8-channel chunks
  if (a->out_layout != MVP_PAIR_SEPARATE && a->out_layout != MVP_PAIR_A_ILV32) return MVP_EINVAL;
  const int tps = a->C / DW_CH;                    // threads per strip: 4 ... 256
  const int spb = 256 / tps;                       // strips per workgroup
  int tp = 1;                                      // reduction threads per pixel: the largest power of two <= 256 / pixels
  while (tp * 2 * spb * DW_TW <= 256 && tp < 64) tp *= 2;
  const int spr = (a->W + DW_TW - 1) / DW_TW;
  const long long nstrips = (long long)a->B * a->H * spr;
  const long long blocks = (nstrips + spb - 1) / spb;
  if (blocks > 0x7fffffffll) return MVP_EINVAL;
  hipLaunchKernelGGL(dwconv7_ln_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, *a, tps, spb, tp, spr, nstrips);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}

extern "C" int64_t mvp_grn_workspace_bytes(int B, int HW, int C4) {
  if (B <= 0 || HW <= 0 || C4 <= 0) return 0;
  return (int64_t)B * grn_slabs(HW) * C4 * (int64_t)sizeof(double);
}

extern "C" int mvp_grn_stats(const mvp_grn_args* a, void* stream) {
  if (!grn_shape_ok(a) || !a->h || !a->G || !a->N || !a->workspace) return MVP_EINVAL;
  if (!aligned_to(a->workspace, 8) || a->workspace_bytes < mvp_grn_workspace_bytes(a->B, a->HW, a->C4)) return MVP_EINVAL;
  const int S = grn_slabs(a->HW);
  double* partial = (double*)a->workspace;
  hipLaunchKernelGGL(grn_partial_kernel, dim3((a->C4 / 4 + 63) / 64, S, a->B), dim3(64), 0, (hipStream_t)stream, *a, S, partial);
  MVP_LAUNCH_CHECK();
  hipLaunchKernelGGL(grn_finish_kernel, dim3(a->B), dim3(256), 0, (hipStream_t)stream, *a, S, (const double*)partial);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}

extern "C" int mvp_grn_apply(const mvp_grn_args* a, void* stream) {
  if (!grn_shape_ok(a) || !a->h || !a->N || !a->gamma || !a->beta || (!a->out_hi && !a->out_f32)) return MVP_EINVAL;
  if (a->out_layout != MVP_PAIR_SEPARATE && (a->out_layout != MVP_PAIR_A_ILV32 || (a->C4 & 31))) return MVP_EINVAL;
  const long long total = (long long)a->B * a->HW * (a->C4 >> 3);
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(grn_apply_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, *a);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}
