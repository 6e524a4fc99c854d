// Training losses with analytic gradients, deterministic reductions (per-block fp64 partials
// combined in a fixed order; no float atomics: csrc/mvp_reduce.h has the rule and the sums):
//   DepthLoss   = 10*sig_loss + 0.5*gradient_loss   (evals/utils/losses.py:54-74,97-154)
//   angular_loss (optionally uncertainty-aware)      (evals/utils/losses.py:157-182)
// Reference quirks are reproduced on purpose: target > max_depth is zeroed in place (Q2); the
// "gradient" term pairs batch entries j and j+2 of the stride-{1,2,4,6} sub-batches (Q1).
#include "mvp_reduce.h"

namespace {

constexpr int DL_NCH = 32;   // chunks per image in the statistics pass
constexpr int DL_NCH2 = 512; // chunks in the pair pass
constexpr int DL_SCAL = 16;  // fp64 scalars

struct DLWs {
  float* ld;       // [B*HW]
  double* partA;   // [B][DL_NCH][3]
  double* partB;   // [DL_NCH2][4]
  double* scal;    // [DL_SCAL]
};

__device__ __host__ inline DLWs dl_ws(void* ws, int B, int64_t HW) {
  DLWs w;
  char* base = (char*)ws;
  int64_t off = ((int64_t)B * HW * 4 + 15) & ~(int64_t)15;
  w.ld = (float*)base;
  w.partA = (double*)(base + off);
  w.partB = w.partA + (int64_t)B * DL_NCH * 3;
  w.scal = w.partB + DL_NCH2 * 4;
  return w;
}

__global__ __launch_bounds__(256) void dl_stats_kernel(const mvp_depth_loss_args p) {
  __shared__ double red[4][3];
  const DLWs w = dl_ws(p.workspace, p.B, p.HW);
  const int b = blockIdx.y, ch = blockIdx.x;
  const int64_t per = (p.HW + DL_NCH - 1) / DL_NCH;
  const int64_t i0 = ch * per, i1 = min(p.HW, i0 + per);
  double v[3] = {0.0, 0.0, 0.0};  // sum g, sum g^2, valid pixels
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    const int64_t o = (int64_t)b * p.HW + i;
    float t = p.target[o];
    if (t > p.max_depth) {
      t = 0.f;
      p.target[o] = 0.f;
    }
    float g = 0.f;
    if (t > 0.f) {
      g = logf(p.pred[o] + p.eps) - logf(t + p.eps);
      v[2] += 1.0;
    }
    w.ld[o] = g;
    v[0] += (double)g;
    v[1] += (double)g * (double)g;
  }
  block_sum<3>(v, red);
  if (threadIdx.x == 0) {
    double* o = w.partA + ((int64_t)b * DL_NCH + ch) * 3;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
  }
}

__device__ __forceinline__ int dl_stride(int k) { return k == 0 ? 1 : (k == 1 ? 2 : (k == 2 ? 4 : 6)); }

__global__ __launch_bounds__(256) void dl_pairs_kernel(const mvp_depth_loss_args p) {
  __shared__ double red[4][4];
  const DLWs w = dl_ws(p.workspace, p.B, p.HW);
  const int64_t per = (p.HW + DL_NCH2 - 1) / DL_NCH2;
  const int64_t i0 = blockIdx.x * per, i1 = min(p.HW, i0 + per);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  constexpr int BMAX = 16;  // fast path: the pixel's B log-differences and validity flags are loaded ONCE (2B loads in
                            // flight together) instead of 4 dependent loads per pair (92 per pixel at B = 16)
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    if (p.B <= BMAX) {
      float g[BMAX];
      bool ok[BMAX];
#pragma unroll
      for (int b = 0; b < BMAX; ++b) {
        const int64_t o = (int64_t)min(b, p.B - 1) * p.HW + i;
        g[b] = w.ld[o];
        ok[b] = (b < p.B) && (p.target[o] > 0.f);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int s = dl_stride(k);  // compile-time after unrolling
        float a = 0.f;
#pragma unroll
        for (int b1 = 0; b1 + 2 * s < BMAX; b1 += s)
          if (ok[b1] && ok[b1 + 2 * s]) a += fabsf(g[b1] - g[b1 + 2 * s]);  // ok[] is false beyond B: same pairs, same order
        acc[k] += (double)a;
      }
      continue;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int s = dl_stride(k);
      float a = 0.f;
      for (int b1 = 0; b1 + 2 * s < p.B; b1 += s) {
        const int64_t o1 = (int64_t)b1 * p.HW + i, o2 = (int64_t)(b1 + 2 * s) * p.HW + i;
        if (p.target[o1] > 0.f && p.target[o2] > 0.f) a += fabsf(w.ld[o1] - w.ld[o2]);
      }
      acc[k] += (double)a;
    }
  }
  block_sum<4>(acc, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) w.partB[blockIdx.x * 4 + k] = acc[k];
  }
}

__global__ __launch_bounds__(256) void dl_finalize_kernel(const mvp_depth_loss_args p) {
  __shared__ double red2[4][2], red4[4][4];
  __shared__ double cntb[1024];
  const DLWs w = dl_ws(p.workspace, p.B, p.HW);
  double s12[2], pr[4];
  fold_rows<2>(w.partA, p.B * DL_NCH, 3, s12, red2);  // columns 0 and 1 of [B * DL_NCH][3]
  fold_rows<4>(w.partB, DL_NCH2, 4, pr, red4);
  const double s1 = s12[0], s2 = s12[1];
  for (int b = threadIdx.x; b < p.B; b += 256) {
    double c = 0.0;
    for (int ch = 0; ch < DL_NCH; ++ch) c += w.partA[((int64_t)b * DL_NCH + ch) * 3 + 2];
    cntb[b] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double n = 0.0;
    for (int b = 0; b < p.B; ++b) n += cntb[b];
    const double mean = s1 / n;
    const double ls = sqrt(s2 / n - (double)p.sigma * mean * mean);
    double lg = 0.0;
    for (int k = 0; k < 4; ++k) {
      const int s = dl_stride(k);
      double ns = 0.0;
      for (int b = 0; b < p.B; b += s) ns += cntb[b];
      lg += pr[k] / ns;  // 0/0 -> NaN exactly like the reference when a sub-batch has no valid pixel
      w.scal[4 + k] = (double)p.w_grad / ns;
    }
    p.loss[0] = (float)((double)p.w_sig * ls + (double)p.w_grad * lg);
    p.loss[1] = (float)ls;
    p.loss[2] = (float)lg;
    w.scal[0] = (double)p.w_sig / (ls * n);                               // coefficient of g
    w.scal[1] = (double)p.w_sig * (double)p.sigma * s1 / (ls * n * n);    // constant term
  }
}

__global__ __launch_bounds__(256) void dl_grad_kernel(const mvp_depth_loss_args p) {
  const DLWs w = dl_ws(p.workspace, p.B, p.HW);
  const float c1 = (float)w.scal[0], c2 = (float)w.scal[1];
  float invn[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) invn[k] = (float)w.scal[4 + k];
  const int64_t total = (int64_t)p.B * p.HW;
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
    float out = 0.f;
    if (p.target[o] > 0.f) {
      const int b = (int)(o / p.HW);
      const float g = w.ld[o];
      float acc = c1 * g - c2;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int s = dl_stride(k);
        if (b % s) continue;
        float sg = 0.f;
        if (b - 2 * s >= 0) {
          const int64_t o2 = o - (int64_t)2 * s * p.HW;
          if (p.target[o2] > 0.f) { const float d = g - w.ld[o2]; sg += (d > 0.f) ? 1.f : (d < 0.f ? -1.f : 0.f); }
        }
        if (b + 2 * s < p.B) {
          const int64_t o2 = o + (int64_t)2 * s * p.HW;
          if (p.target[o2] > 0.f) { const float d = g - w.ld[o2]; sg += (d > 0.f) ? 1.f : (d < 0.f ? -1.f : 0.f); }
        }
        acc += invn[k] * sg;
      }
      out = acc / (p.pred[o] + p.eps);
    }
    p.grad_pred[o] = out;
  }
}

// ----------------------------------------------------------------------------- DepthLoss in two launches (B <= 16)
// The four-kernel form above passes the log-differences through HBM (a [B*HW] scratch array written once and read by two kernels)
// and strings three dependent launches before the gradient: ~36 B per element and four launch latencies for an algorithmic 12 B.
// For B <= 16 (the reference's batch size and every configuration of BASELINE.json) a thread keeps the B log-differences of ONE pixel
// in registers, so (1) one pass over pred / target yields every sum the loss needs — s1, s2, the per-image valid counts and the four
// pair sums — and (2) the gradient pass re-derives the log-differences from the same two arrays (2B logf per pixel, cheap next to
// the loads) after every block has reduced the partials itself (fixed order: same scalars in every block, no finalize launch).
// 20 B per element, two launches.  Arithmetic per term as above (fp32 log-differences, fp64 sums, Q1 pairs, Q2 zeroing).
constexpr int DLF_NB = 512;  // blocks (pixel chunks) at most

struct DLFWs {
  double* part;  // [DLF_NB][6]: s1, s2, pair sums of strides 1, 2, 4, 6
  int* cnt;      // [DLF_NB][16]: valid pixels per image
};

__device__ __host__ inline DLFWs dlf_ws(void* ws, int B, int64_t HW) {
  const DLWs w = dl_ws(ws, B, HW);
  DLFWs f;
  f.part = w.scal + DL_SCAL;
  f.cnt = (int*)(f.part + DLF_NB * 6);
  return f;
}

template <bool WRITE_TARGET>
__device__ __forceinline__ void dlf_pixel(const mvp_depth_loss_args& p, int64_t i, float (&g)[16], bool (&ok)[16], float (&pr)[16]) {
#pragma unroll
  for (int b = 0; b < 16; ++b) {
    const int64_t o = (int64_t)min(b, p.B - 1) * p.HW + i;
    float t = p.target[o];
    pr[b] = p.pred[o];
    if (WRITE_TARGET && b < p.B && t > p.max_depth) p.target[o] = 0.f;  // Q2: zeroed in place
    if (t > p.max_depth) t = 0.f;
    ok[b] = (b < p.B) && (t > 0.f);
    g[b] = ok[b] ? logf(pr[b] + p.eps) - logf(t + p.eps) : 0.f;
  }
}

__global__ __launch_bounds__(256) void dlf_stats_kernel(const mvp_depth_loss_args p) {
  __shared__ double red[4][6];
  __shared__ int scnt[16];
  const DLFWs w = dlf_ws(p.workspace, p.B, p.HW);
  const int64_t per = (p.HW + gridDim.x - 1) / gridDim.x;
  const int64_t i0 = blockIdx.x * per, i1 = min(p.HW, i0 + per);
  if (threadIdx.x < 16) scnt[threadIdx.x] = 0;
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // s1, s2, pair sums of strides 1, 2, 4, 6
  int cnt[16];
#pragma unroll
  for (int b = 0; b < 16; ++b) cnt[b] = 0;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    float g[16], pr[16];
    bool ok[16];
    dlf_pixel<true>(p, i, g, ok, pr);
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      v[0] += (double)g[b];
      v[1] += (double)g[b] * (double)g[b];
      cnt[b] += ok[b] ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int s = dl_stride(k);
      float a = 0.f;
#pragma unroll
      for (int b1 = 0; b1 + 2 * s < 16; b1 += s)
        if (ok[b1] && ok[b1 + 2 * s]) a += fabsf(g[b1] - g[b1 + 2 * s]);
      v[2 + k] += (double)a;
    }
  }
  __syncthreads();
#pragma unroll
  for (int b = 0; b < 16; ++b) {
    const int c = (int)wave_sum((unsigned)cnt[b]);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&scnt[b], c);  // integers: exact in any order
  }
  block_sum<6>(v, red);  // its second barrier also orders the atomics above before the read of scnt below
  if (threadIdx.x == 0) {
    double* o = w.part + (int64_t)blockIdx.x * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = v[k];
  }
  if (threadIdx.x < 16) w.cnt[blockIdx.x * 16 + threadIdx.x] = scnt[threadIdx.x];
}

__global__ __launch_bounds__(256) void dlf_grad_kernel(const mvp_depth_loss_args p, const int nb) {
  __shared__ double red[4][6];
  __shared__ int scnt[16];
  __shared__ float coef[8];
  const DLFWs w = dlf_ws(p.workspace, p.B, p.HW);
  // every block reduces the nb partial rows itself, in the same fixed order: identical scalars everywhere, no finalize launch
  if (threadIdx.x < 16) scnt[threadIdx.x] = 0;
  __syncthreads();
  int c16 = 0;
  for (int e = threadIdx.x; e < nb * 16; e += 256) {  // e % 16 is the same image for every e of a thread (256 % 16 == 0)
    c16 += w.cnt[e];
  }
  if (c16) atomicAdd(&scnt[threadIdx.x & 15], c16);
  double v[6];
  fold_rows<6>(w.part, nb, 6, v, red);  // its second barrier also orders the atomics above before the read of scnt below
  if (threadIdx.x == 0) {
    double n = 0.0;
    for (int b = 0; b < p.B; ++b) n += (double)scnt[b];
    const double mean = v[0] / n;
    const double ls = sqrt(v[1] / n - (double)p.sigma * mean * mean);
    double lg = 0.0;
    for (int k = 0; k < 4; ++k) {
      const int s = dl_stride(k);
      double ns = 0.0;
      for (int b = 0; b < p.B; b += s) ns += (double)scnt[b];
      lg += v[2 + k] / ns;  // 0/0 -> NaN exactly like the reference when a sub-batch has no valid pixel
      coef[2 + k] = (float)((double)p.w_grad / ns);
    }
    coef[0] = (float)((double)p.w_sig / (ls * n));                             // coefficient of g
    coef[1] = (float)((double)p.w_sig * (double)p.sigma * v[0] / (ls * n * n));  // constant term
    if (blockIdx.x == 0) {
      p.loss[0] = (float)((double)p.w_sig * ls + (double)p.w_grad * lg);
      p.loss[1] = (float)ls;
      p.loss[2] = (float)lg;
    }
  }
  __syncthreads();
  if (!p.grad_pred) return;
  const float c1 = coef[0], c2 = coef[1];
  const float invn[4] = {coef[2], coef[3], coef[4], coef[5]};
  const int64_t per = (p.HW + gridDim.x - 1) / gridDim.x;
  const int64_t i0 = blockIdx.x * per, i1 = min(p.HW, i0 + per);
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    float g[16], pr[16];
    bool ok[16];
    dlf_pixel<false>(p, i, g, ok, pr);
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      float out = 0.f;
      if (ok[b]) {
        float acc = c1 * g[b] - c2;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int s = dl_stride(k);
          if (b % s) continue;
          float sg = 0.f;
          if (b - 2 * s >= 0 && ok[(b - 2 * s) & 15]) { const float d = g[b] - g[(b - 2 * s) & 15]; sg += (d > 0.f) ? 1.f : (d < 0.f ? -1.f : 0.f); }
          if (b + 2 * s < 16 && ok[(b + 2 * s) & 15]) { const float d = g[b] - g[(b + 2 * s) & 15]; sg += (d > 0.f) ? 1.f : (d < 0.f ? -1.f : 0.f); }
          acc += invn[k] * sg;
        }
        out = acc / (pr[b] + p.eps);
      }
      if (b < p.B) p.grad_pred[(int64_t)b * p.HW + i] = out;
    }
  }
}

// ----------------------------------------------------------------------------- angular loss
constexpr int AL_NB = 128;

struct AngPix { float loss; float g[4]; };

__device__ __forceinline__ AngPix ang_pixel(const mvp_angular_loss_args& p, int64_t b, int64_t i, bool want_grad) {
  AngPix r;
  const float* pr = p.pred + (b * p.Cp) * p.HW + i;
  const float* gt = p.gt + (b * 3) * p.HW + i;
  const float p0 = pr[0], p1 = pr[p.HW], p2 = pr[2 * p.HW];
  const float g0 = gt[0], g1 = gt[p.HW], g2 = gt[2 * p.HW];
  const float np = fmaxf(sqrtf(p0 * p0 + p1 * p1 + p2 * p2), 1e-8f);
  const float ng = fmaxf(sqrtf(g0 * g0 + g1 * g1 + g2 * g2), 1e-8f);
  const float ph0 = p0 / np, ph1 = p1 / np, ph2 = p2 / np;
  const float gh0 = g0 / ng, gh1 = g1 / ng, gh2 = g2 / ng;
  const float cosv = ph0 * gh0 + ph1 * gh1 + ph2 * gh2;
  const float lo = -1.f + p.eps, hi = 1.f - p.eps;
  const bool clamped = (cosv < lo) || (cosv > hi);
  const float cc = fminf(fmaxf(cosv, lo), hi);
  const float ang = acosf(cc);
  float dang = clamped ? 0.f : -1.0f / sqrtf(1.f - cc * cc);  // d ang / d cos
  float kappa = 1.f;
  r.g[3] = 0.f;
  if (p.Cp == 4) {
    const float p3 = pr[3 * p.HW];
    kappa = (p3 > 0.f ? p3 : expm1f(p3)) + 1.01f;
    const float e = expf(-kappa * 3.14159265358979323846f);
    r.loss = log1pf(e) - logf(kappa * kappa + 1.f) + kappa * ang;
    if (want_grad) {
      const float dk = -3.14159265358979323846f * e / (1.f + e) - 2.f * kappa / (kappa * kappa + 1.f) + ang;
      r.g[3] = dk * (p3 > 0.f ? 1.f : expf(p3));
    }
  } else {
    r.loss = ang;
  }
  if (want_grad) {
    const float c = kappa * dang / np;
    r.g[0] = c * (gh0 - cosv * ph0);
    r.g[1] = c * (gh1 - cosv * ph1);
    r.g[2] = c * (gh2 - cosv * ph2);
  }
  return r;
}

__global__ __launch_bounds__(256) void ang_stats_kernel(const mvp_angular_loss_args p, double* part) {
  __shared__ double red[4][2];
  const int64_t total = (int64_t)p.B * p.HW;
  double v[2] = {0.0, 0.0};  // sum of the losses, masked pixels
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)AL_NB * 256) {
    if (p.mask[o]) {
      v[0] += (double)ang_pixel(p, o / p.HW, o % p.HW, false).loss;
      v[1] += 1.0;
    }
  }
  block_sum<2>(v, red);
  if (threadIdx.x == 0) { part[blockIdx.x * 2] = v[0]; part[blockIdx.x * 2 + 1] = v[1]; }
}

__global__ void ang_finalize_kernel(const mvp_angular_loss_args p, double* part) {
  if (threadIdx.x != 0) return;
  double s = 0.0, c = 0.0;
  for (int i = 0; i < AL_NB; ++i) { s += part[i * 2]; c += part[i * 2 + 1]; }
  p.loss[0] = (float)(s / c);
  part[AL_NB * 2] = 1.0 / c;
}

__global__ __launch_bounds__(256) void ang_grad_kernel(const mvp_angular_loss_args p, const double* part) {
  const float invn = (float)part[AL_NB * 2];
  const int64_t total = (int64_t)p.B * p.HW;
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
    const int64_t b = o / p.HW, i = o % p.HW;
    float* g = p.grad_pred + (b * p.Cp) * p.HW + i;
    if (p.mask[o]) {
      const AngPix r = ang_pixel(p, b, i, true);
      for (int c = 0; c < p.Cp; ++c) g[c * p.HW] = r.g[c] * invn;
    } else {
      for (int c = 0; c < p.Cp; ++c) g[c * p.HW] = 0.f;
    }
  }
}

inline int grid_for(int64_t work) {
  int64_t g = (work + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

}  // namespace

extern "C" int64_t mvp_depth_loss_workspace_bytes(int B, int64_t HW) {
  const int64_t ld = ((int64_t)B * HW * 4 + 15) & ~(int64_t)15;
  return ld + ((int64_t)B * DL_NCH * 3 + DL_NCH2 * 4 + DL_SCAL) * 8 + (int64_t)DLF_NB * (6 * 8 + 16 * 4);
}

extern "C" int mvp_depth_loss_fwd_bwd(const mvp_depth_loss_args* a, void* stream) {
  if (!a || !a->pred || !a->target || !a->loss || !a->workspace) return MVP_EINVAL;
  if (a->B <= 0 || a->B > 1024 || a->HW <= 0) return MVP_EINVAL;
  if (a->workspace_bytes < mvp_depth_loss_workspace_bytes(a->B, a->HW)) return MVP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  static const bool fused_ok = [] { const char* e = getenv("MVP_DEPTH_LOSS_FUSED"); return !e || atoi(e) != 0; }();
  if (a->B <= 16 && fused_ok) {  // two launches, log-differences in registers
    const int nb = (int)max((int64_t)1, min((int64_t)DLF_NB, (a->HW + 255) / 256));
    hipLaunchKernelGGL(dlf_stats_kernel, dim3(nb), dim3(256), 0, s, *a);
    hipLaunchKernelGGL(dlf_grad_kernel, dim3(a->grad_pred ? nb : 1), dim3(256), 0, s, *a, nb);
    MVP_LAUNCH_CHECK();
    return MVP_OK;
  }
  hipLaunchKernelGGL(dl_stats_kernel, dim3(DL_NCH, a->B), dim3(256), 0, s, *a);
  hipLaunchKernelGGL(dl_pairs_kernel, dim3(DL_NCH2), dim3(256), 0, s, *a);
  hipLaunchKernelGGL(dl_finalize_kernel, dim3(1), dim3(256), 0, s, *a);
  if (a->grad_pred) hipLaunchKernelGGL(dl_grad_kernel, dim3(grid_for((int64_t)a->B * a->HW)), dim3(256), 0, s, *a);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}

extern "C" int mvp_angular_loss_fwd_bwd(const mvp_angular_loss_args* a, void* stream) {
  if (!a || !a->pred || !a->gt || !a->mask || !a->loss || !a->workspace) return MVP_EINVAL;
  if (a->B <= 0 || a->HW <= 0 || (a->Cp != 3 && a->Cp != 4)) return MVP_EINVAL;
  if (a->workspace_bytes < (int64_t)(AL_NB * 2 + 2) * 8) return MVP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)a->workspace;
  hipLaunchKernelGGL(ang_stats_kernel, dim3(AL_NB), dim3(256), 0, s, *a, part);
  hipLaunchKernelGGL(ang_finalize_kernel, dim3(1), dim3(64), 0, s, *a, part);
  if (a->grad_pred) hipLaunchKernelGGL(ang_grad_kernel, dim3(grid_for((int64_t)a->B * a->HW)), dim3(256), 0, s, *a, part);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}
