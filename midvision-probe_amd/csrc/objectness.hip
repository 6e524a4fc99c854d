// The tail of the objectness probe (reference: evals/models/probes.py:7-43 BinaryHead / TaskonomyHead,
// train_generic_objectness.py:391-395 BCELoss, :56-183 + :446-454 the mask metrics):
//   mvp_bn_act_fwd / _bwd   train- or eval-mode BatchNorm2d + sigmoid (or plain tanh / identity) on a map of 1..8 channels
//   mvp_bce_loss_fwd_bwd    nn.BCELoss (mean) and its gradient
//   mvp_binary_counts       TP / FP / FN / TN of a thresholded prediction
// All three stream their operands once or twice and are bound by memory.  Every floating-point reduction is per-workgroup partials in
// the caller's workspace, folded in a fixed order (no float atomics; csrc/mvp_reduce.h): the same inputs give the same bits.  The
// counts are integers, so their 64-bit atomics are exact in any order.
#include "mvp_reduce.h"

namespace {

constexpr int OB_NB = MVP_BN_ACT_WORKSPACE_BYTES / (8 * 3 * 8);  // 512: partial rows of the BatchNorm reductions at most
constexpr int BCE_NB = MVP_BCE_WORKSPACE_BYTES / 8;              // 1024: partial sums of the loss at most
constexpr int ACT_NONE = 0, ACT_SIGMOID = 1, ACT_TANH = 2;

// ----------------------------------------------------------------------------- (count, mean, M2) and its merge (Chan et al.)
// The batch variance is never formed as E[x^2] - E[x]^2: a thread sums (x - k) and (x - k)^2 around ITS first element k (k is one of
// its samples, so the sum of squares is at most count x the thread's own M2: no cancellation to speak of), turns that into
// (count, mean, M2) and from there on only merges — every term of a merge is a sum of non-negative parts.  fp64 throughout (a few
// operations per element next to a 16-byte load).
struct Wf { double n, mean, m2; };

__device__ __forceinline__ Wf wf_merge(const Wf a, const Wf b) {
  const double n = a.n + b.n;
  if (n == 0.0) return a;
  const double d = b.mean - a.mean, fb = b.n / n;
  Wf r;
  r.n = n;
  r.mean = a.mean + d * fb;
  r.m2 = a.m2 + b.m2 + d * d * a.n * fb;
  return r;
}

// every thread returns the merge of the workgroup's 256 values, in the order of block_sum (csrc/mvp_reduce.h): butterfly inside a wave
// (lane 0 is what counts), waves 0..3 in order
template <int CM>
__device__ __forceinline__ void block_merge(Wf (&w)[CM], Wf (*red)[CM]) {
#pragma unroll
  for (int c = 0; c < CM; ++c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      Wf t;
      t.n = __shfl_xor(w[c].n, o, 64);
      t.mean = __shfl_xor(w[c].mean, o, 64);
      t.m2 = __shfl_xor(w[c].m2, o, 64);
      w[c] = wf_merge(w[c], t);
    }
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < CM; ++c) red[threadIdx.x >> 6][c] = w[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < CM; ++c) w[c] = wf_merge(wf_merge(red[0][c], red[1][c]), wf_merge(red[2][c], red[3][c]));
}

// Row r of the channels-last map: channels 0..C-1 (padding columns are not used).  V4: ld == 4 and a 16-byte aligned base, one
// 16-byte load per row.
template <int CM, bool V4>
__device__ __forceinline__ void load_row(const float* x, int64_t r, int ld, int C, float (&v)[CM]) {
  if (V4) {
    const float4 t = *(const float4*)(x + r * 4);
    v[0] = t.x;
    if (CM > 1) v[1 % CM] = t.y;
    if (CM > 2) { v[2 % CM] = t.z; v[3 % CM] = t.w; }
  } else {
#pragma unroll
    for (int c = 0; c < CM; ++c) v[c] = c < C ? x[r * ld + c] : 0.f;
  }
}

template <int CM, bool V4>
__device__ __forceinline__ void store_row(float* g, int64_t r, int ld, int C, const float (&v)[CM]) {
  if (V4) {
    float4 t;
    t.x = v[0];
    t.y = (CM > 1 && 1 < C) ? v[1 % CM] : 0.f;
    t.z = (CM > 2 && 2 < C) ? v[2 % CM] : 0.f;
    t.w = (CM > 2 && 3 < C) ? v[3 % CM] : 0.f;
    *(float4*)(g + r * 4) = t;
  } else {
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) g[r * ld + c] = v[c];
    for (int c = C; c < ld; ++c) g[r * ld + c] = 0.f;  // padding columns: zero
  }
}

// (image, pixel) of row r
__device__ __forceinline__ void split_row(int64_t r, int64_t HW, bool small, int64_t& b, int64_t& i) {
  if (small) {
    const uint32_t q = (uint32_t)r / (uint32_t)HW;
    b = q;
    i = (uint32_t)r - q * (uint32_t)HW;
  } else {
    b = r / HW;
    i = r - b * HW;
  }
}

__device__ __forceinline__ float sigmoidf_(float z) { return 1.0f / (1.0f + expf(-z)); }

// per-channel constants of the normalisation: xhat = ((x - mean) - mean_lo) * rstd (the batch mean is kept to fp32 twice: at
// |mean| >> sigma one fp32 alone would be wrong by half an ulp of the MEAN, which is not small against sigma), z = xhat * gamma + beta
struct BnC { float mean, mean_lo, rstd, gamma, beta; };

template <int CM>
__device__ __forceinline__ void load_bnc(const mvp_bn_act_args& p, BnC (&k)[CM]) {
#pragma unroll
  for (int c = 0; c < CM; ++c) {
    const int cc = c < p.C ? c : 0;
    k[c].mean = p.stats[cc];
    k[c].rstd = p.stats[p.C + cc];
    k[c].mean_lo = p.stats[2 * p.C + cc];
    k[c].gamma = p.gamma[cc];
    k[c].beta = p.beta[cc];
  }
}

// ----------------------------------------------------------------------------- BatchNorm + activation, forward
template <int CM, bool V4>
__global__ __launch_bounds__(256) void bn_stats_kernel(const mvp_bn_act_args p, const int64_t per) {
  __shared__ Wf red[4][CM];
  const int64_t P = (int64_t)p.B * p.HW;
  const int64_t r0 = (int64_t)blockIdx.x * per, r1 = min(P, r0 + per);
  double k[CM], s1[CM], s2[CM], cnt = 0.0;
#pragma unroll
  for (int c = 0; c < CM; ++c) k[c] = s1[c] = s2[c] = 0.0;
  for (int64_t r = r0 + threadIdx.x; r < r1; r += 256) {
    float v[CM];
    load_row<CM, V4>(p.x, r, p.ld, p.C, v);
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      if (cnt == 0.0) k[c] = (double)v[c];
      const double d = (double)v[c] - k[c];
      s1[c] += d;
      s2[c] += d * d;
    }
    cnt += 1.0;
  }
  Wf w[CM];
#pragma unroll
  for (int c = 0; c < CM; ++c) {
    w[c].n = cnt;
    w[c].mean = cnt > 0.0 ? k[c] + s1[c] / cnt : 0.0;
    w[c].m2 = cnt > 0.0 ? fmax(s2[c] - s1[c] * s1[c] / cnt, 0.0) : 0.0;
  }
  block_merge<CM>(w, red);
  if (threadIdx.x == 0) {
    double* ws = (double*)p.workspace;
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      if (c < p.C) {
        double* o = ws + ((int64_t)blockIdx.x * p.C + c) * 3;
        o[0] = w[c].n; o[1] = w[c].mean; o[2] = w[c].m2;
      }
    }
  }
}

// nbs: partial rows bn_stats_kernel wrote (training sigmoid form), 0 otherwise
template <int CM, bool V4>
__global__ __launch_bounds__(256) void bn_apply_kernel(const mvp_bn_act_args p, const int64_t per, const int nbs) {
  __shared__ Wf red[4][CM];
  const int64_t P = (int64_t)p.B * p.HW;
  BnC k[CM];
#pragma unroll
  for (int c = 0; c < CM; ++c) k[c] = BnC{0.f, 0.f, 1.f, 1.f, 0.f};
  if (p.act == ACT_SIGMOID) {
    double mean[CM], var[CM];
    if (p.training) {
      // every workgroup folds the partial rows itself, in the same fixed order: the same statistics everywhere, no launch in between
      Wf w[CM];
#pragma unroll
      for (int c = 0; c < CM; ++c) w[c] = Wf{0.0, 0.0, 0.0};
      const double* ws = (const double*)p.workspace;
      for (int i = threadIdx.x; i < nbs; i += 256) {
#pragma unroll
        for (int c = 0; c < CM; ++c) {
          if (c < p.C) {
            const double* o = ws + ((int64_t)i * p.C + c) * 3;
            w[c] = wf_merge(w[c], Wf{o[0], o[1], o[2]});
          }
        }
      }
      block_merge<CM>(w, red);
#pragma unroll
      for (int c = 0; c < CM; ++c) { mean[c] = w[c].mean; var[c] = w[c].m2 / (double)P; }
    } else {
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        const int cc = c < p.C ? c : 0;
        mean[c] = (double)p.running_mean[cc];
        var[c] = (double)p.running_var[cc];
      }
    }
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      const int cc = c < p.C ? c : 0;
      k[c].mean = (float)mean[c];
      k[c].mean_lo = (float)(mean[c] - (double)k[c].mean);
      k[c].rstd = (float)(1.0 / sqrt(var[c] + (double)p.eps));
      k[c].gamma = p.gamma[cc];
      k[c].beta = p.beta[cc];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        if (c < p.C) {
          p.stats[c] = k[c].mean;
          p.stats[p.C + c] = k[c].rstd;
          p.stats[2 * p.C + c] = k[c].mean_lo;
          if (p.training && p.running_mean && p.running_var) {
            const double m = (double)p.momentum, unb = var[c] * ((double)p.n / (double)(p.n - 1));
            p.running_mean[c] = (float)((1.0 - m) * (double)p.running_mean[c] + m * mean[c]);
            p.running_var[c] = (float)((1.0 - m) * (double)p.running_var[c] + m * unb);
          }
        }
      }
      if (p.training && p.num_batches_tracked) p.num_batches_tracked[0] += 1;
    }
  }
  const bool small = P <= (int64_t)0x7fffffff;
  const int64_t r0 = (int64_t)blockIdx.x * per, r1 = min(P, r0 + per);
  for (int64_t r = r0 + threadIdx.x; r < r1; r += 256) {
    float v[CM];
    load_row<CM, V4>(p.x, r, p.ld, p.C, v);
    int64_t b, i;
    split_row(r, p.HW, small, b, i);
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      if (c < p.C) {
        float y = v[c];
        if (p.act == ACT_SIGMOID) y = sigmoidf_(((v[c] - k[c].mean) - k[c].mean_lo) * k[c].rstd * k[c].gamma + k[c].beta);
        else if (p.act == ACT_TANH) y = tanhf(v[c]);
        p.y[(b * p.C + c) * p.HW + i] = y;
      }
    }
  }
}

// ----------------------------------------------------------------------------- BatchNorm + activation, backward
// g_z = grad_y * sigmoid'(z), recomputed from x and the saved statistics (y is not kept).  Pass 1: dbeta = sum g_z, dgamma = sum g_z * xhat.
template <int CM, bool V4>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const mvp_bn_act_args p, const int64_t per) {
  __shared__ double red[4][2 * CM];
  const int64_t P = (int64_t)p.B * p.HW;
  const bool small = P <= (int64_t)0x7fffffff;
  BnC k[CM];
  load_bnc<CM>(p, k);
  double acc[2 * CM];
#pragma unroll
  for (int c = 0; c < 2 * CM; ++c) acc[c] = 0.0;
  const int64_t r0 = (int64_t)blockIdx.x * per, r1 = min(P, r0 + per);
  for (int64_t r = r0 + threadIdx.x; r < r1; r += 256) {
    float v[CM];
    load_row<CM, V4>(p.x, r, p.ld, p.C, v);
    int64_t b, i;
    split_row(r, p.HW, small, b, i);
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      if (c < p.C) {
        const float xh = ((v[c] - k[c].mean) - k[c].mean_lo) * k[c].rstd;
        const float s = sigmoidf_(xh * k[c].gamma + k[c].beta);
        const float gz = p.grad_y[(b * p.C + c) * p.HW + i] * (s * (1.0f - s));
        acc[2 * c] += (double)gz;
        acc[2 * c + 1] += (double)gz * (double)xh;
      }
    }
  }
  block_sum<2 * CM>(acc, red);
  if (threadIdx.x == 0) {
    double* ws = (double*)p.workspace;
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      if (c < p.C) {
        ws[((int64_t)blockIdx.x * p.C + c) * 2] = acc[2 * c];
        ws[((int64_t)blockIdx.x * p.C + c) * 2 + 1] = acc[2 * c + 1];
      }
    }
  }
}

// Pass 2 (sigmoid form; nbs partial rows) or the only pass (tanh / identity; nbs = 0): grad_x in the [P, ld] layout of the trunk's backward.
template <int CM, bool V4>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const mvp_bn_act_args p, const int64_t per, const int nbs) {
  __shared__ double red[4][2 * CM];
  const int64_t P = (int64_t)p.B * p.HW;
  const bool small = P <= (int64_t)0x7fffffff;
  BnC k[CM];
  float mb[CM], mg[CM];  // dbeta / P and dgamma / P of the training form, 0 in eval mode
#pragma unroll
  for (int c = 0; c < CM; ++c) { k[c] = BnC{0.f, 0.f, 1.f, 1.f, 0.f}; mb[c] = mg[c] = 0.f; }
  if (p.act == ACT_SIGMOID) {
    load_bnc<CM>(p, k);
    double acc[2 * CM];
#pragma unroll
    for (int c = 0; c < 2 * CM; ++c) acc[c] = 0.0;
    const double* ws = (const double*)p.workspace;
    for (int i = threadIdx.x; i < nbs; i += 256) {  // (not fold_rows<2 * CM>: a row holds 2 C <= 2 CM doubles)
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        if (c < p.C) {
          acc[2 * c] += ws[((int64_t)i * p.C + c) * 2];
          acc[2 * c + 1] += ws[((int64_t)i * p.C + c) * 2 + 1];
        }
      }
    }
    block_sum<2 * CM>(acc, red);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        if (c < p.C) {
          const float db = (float)acc[2 * c], dg = (float)acc[2 * c + 1];
          if (p.grad_beta) p.grad_beta[c] = p.accumulate ? p.grad_beta[c] + db : db;
          if (p.grad_gamma) p.grad_gamma[c] = p.accumulate ? p.grad_gamma[c] + dg : dg;
        }
      }
    }
    if (p.training) {
#pragma unroll
      for (int c = 0; c < CM; ++c) { mb[c] = (float)(acc[2 * c] / (double)P); mg[c] = (float)(acc[2 * c + 1] / (double)P); }
    }
  }
  if (!p.grad_x) return;
  const int64_t r0 = (int64_t)blockIdx.x * per, r1 = min(P, r0 + per);
  for (int64_t r = r0 + threadIdx.x; r < r1; r += 256) {
    float v[CM], g[CM];
    load_row<CM, V4>(p.x, r, p.ld, p.C, v);
    int64_t b, i;
    split_row(r, p.HW, small, b, i);
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      g[c] = 0.f;
      if (c < p.C) {
        const float gy = p.grad_y[(b * p.C + c) * p.HW + i];
        if (p.act == ACT_SIGMOID) {
          const float xh = ((v[c] - k[c].mean) - k[c].mean_lo) * k[c].rstd;
          const float s = sigmoidf_(xh * k[c].gamma + k[c].beta);
          const float gz = gy * (s * (1.0f - s));
          g[c] = k[c].gamma * k[c].rstd * ((gz - mb[c]) - xh * mg[c]);
        } else if (p.act == ACT_TANH) {
          const float t = tanhf(v[c]);
          g[c] = gy * (1.0f - t * t);
        } else {
          g[c] = gy;
        }
      }
    }
    store_row<CM, V4>(p.grad_x, r, p.ld, p.C, g);
  }
}

// ----------------------------------------------------------------------------- BCELoss
// l = -(t * max(log p, -100) + (1 - t) * max(log1p(-p), -100)),  d l / d p = (p - t) / max((1 - p) p, 1e-12); both over N.
__device__ __forceinline__ float bce_elem(float pr, float t, float n, float& g) {
  const float lp = fmaxf(logf(pr), -100.f), lq = fmaxf(log1pf(-pr), -100.f);
  g = (pr - t) / fmaxf((1.0f - pr) * pr, 1e-12f) / n;
  return -(t * lp + (1.0f - t) * lq);
}

template <bool V4>
__global__ __launch_bounds__(256) void bce_kernel(const mvp_bce_loss_args p) {
  __shared__ double red[4][1];
  const float n = (float)p.N;
  double acc[1] = {0.0};
  const int64_t stride = (int64_t)gridDim.x * 256, t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (V4) {
    const int64_t nv = p.N >> 2;
    for (int64_t v = t0; v < nv; v += stride) {
      const float4 a = ((const float4*)p.pred)[v], t = ((const float4*)p.target)[v];
      float4 g;
      float l = bce_elem(a.x, t.x, n, g.x);
      l += bce_elem(a.y, t.y, n, g.y);
      l += bce_elem(a.z, t.z, n, g.z);
      l += bce_elem(a.w, t.w, n, g.w);
      acc[0] += (double)l;
      if (p.grad_pred) ((float4*)p.grad_pred)[v] = g;
    }
    for (int64_t i = (nv << 2) + t0; i < p.N; i += stride) {  // the last N % 4 elements
      float g;
      acc[0] += (double)bce_elem(p.pred[i], p.target[i], n, g);
      if (p.grad_pred) p.grad_pred[i] = g;
    }
  } else {
    for (int64_t i = t0; i < p.N; i += stride) {
      float g;
      acc[0] += (double)bce_elem(p.pred[i], p.target[i], n, g);
      if (p.grad_pred) p.grad_pred[i] = g;
    }
  }
  block_sum<1>(acc, red);
  if (threadIdx.x == 0) ((double*)p.workspace)[blockIdx.x] = acc[0];
}

__global__ __launch_bounds__(256) void bce_finalize_kernel(const mvp_bce_loss_args p, const int nb) {
  __shared__ double red[4][1];
  double acc[1];
  fold_rows<1>((const double*)p.workspace, nb, 1, acc, red);
  if (threadIdx.x == 0) p.loss[0] = (float)(acc[0] / (double)p.N);
}

// ----------------------------------------------------------------------------- confusion counts
template <bool V4>
__global__ __launch_bounds__(256) void counts_kernel(const mvp_binary_counts_args p) {
  __shared__ unsigned int red[4][4];
  const int64_t g = blockIdx.y;
  const float* pr = p.pred + g * p.n;
  const float* gt = p.gt + g * p.n;
  unsigned int c[4] = {0u, 0u, 0u, 0u};  // TP FP FN TN (a thread sees far fewer than 2^32 elements: the host bounds n / grid)
  auto count = [&](float a, float t) {
    const bool pos = a > p.threshold;
    c[0] += (pos && t == 1.0f) ? 1u : 0u;
    c[1] += (pos && t == 0.0f) ? 1u : 0u;
    c[2] += (!pos && t == 1.0f) ? 1u : 0u;
    c[3] += (!pos && t == 0.0f) ? 1u : 0u;
  };
  const int64_t stride = (int64_t)gridDim.x * 256, t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (V4) {
    const int64_t nv = p.n >> 2;
    for (int64_t v = t0; v < nv; v += stride) {
      const float4 a = ((const float4*)pr)[v], t = ((const float4*)gt)[v];
      count(a.x, t.x); count(a.y, t.y); count(a.z, t.z); count(a.w, t.w);
    }
    for (int64_t i = (nv << 2) + t0; i < p.n; i += stride) count(pr[i], gt[i]);
  } else {
    for (int64_t i = t0; i < p.n; i += stride) count(pr[i], gt[i]);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) c[k] = wave_sum(c[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) red[threadIdx.x >> 6][k] = c[k];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const unsigned long long s = (unsigned long long)red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    if (s) atomicAdd((unsigned long long*)(p.counts + g * 4 + threadIdx.x), s);  // integers: exact in any order
  }
}

// rows per workgroup and workgroups: at least 1024 rows each, OB_NB workgroups at most
inline void bn_partition(int64_t P, int64_t& per, int& nb) {
  int64_t n = (P + 1023) / 1024;
  n = n < 1 ? 1 : (n > OB_NB ? OB_NB : n);
  per = (P + n - 1) / n;
  nb = (int)((P + per - 1) / per);
}

// fwd != 0: bn_stats (when stats) + bn_apply;  fwd == 0: bn_bwd_reduce (when stats) + bn_bwd_apply
template <int CM, bool V4>
void bn_launch(const mvp_bn_act_args& a, bool fwd, bool reduce, hipStream_t s) {
  int64_t per;
  int nb;
  bn_partition((int64_t)a.B * a.HW, per, nb);
  if (fwd) {
    if (reduce) hipLaunchKernelGGL((bn_stats_kernel<CM, V4>), dim3(nb), dim3(256), 0, s, a, per);
    hipLaunchKernelGGL((bn_apply_kernel<CM, V4>), dim3(nb), dim3(256), 0, s, a, per, reduce ? nb : 0);
  } else {
    if (reduce) hipLaunchKernelGGL((bn_bwd_reduce_kernel<CM, V4>), dim3(nb), dim3(256), 0, s, a, per);
    hipLaunchKernelGGL((bn_bwd_apply_kernel<CM, V4>), dim3(a.grad_x ? nb : 1), dim3(256), 0, s, a, per, reduce ? nb : 0);
  }
}

void bn_dispatch(const mvp_bn_act_args& a, bool fwd, bool reduce, bool v4, hipStream_t s) {
  if (a.C == 1) v4 ? bn_launch<1, true>(a, fwd, reduce, s) : bn_launch<1, false>(a, fwd, reduce, s);
  else if (a.C == 2) v4 ? bn_launch<2, true>(a, fwd, reduce, s) : bn_launch<2, false>(a, fwd, reduce, s);
  else if (a.C <= 4) v4 ? bn_launch<4, true>(a, fwd, reduce, s) : bn_launch<4, false>(a, fwd, reduce, s);
  else bn_launch<8, false>(a, fwd, reduce, s);
}

bool bn_shape_ok(const mvp_bn_act_args* a) {
  if (!a || !a->x) return false;
  if (a->B <= 0 || a->HW <= 0 || a->C < 1 || a->C > MVP_BN_ACT_MAX_C || a->ld < a->C) return false;
  if (a->HW > ((int64_t)1 << 40) / a->B) return false;
  if (a->act < ACT_NONE || a->act > ACT_TANH) return false;
  if (a->act == ACT_SIGMOID) {
    if (!a->gamma || !a->beta || !a->stats) return false;
    if (!a->workspace || a->workspace_bytes < MVP_BN_ACT_WORKSPACE_BYTES) return false;
  }
  return true;
}

}  // namespace

extern "C" int mvp_bn_act_fwd(const mvp_bn_act_args* a, void* stream) {
  if (!bn_shape_ok(a) || !a->y) return MVP_EINVAL;
  const bool sig = a->act == ACT_SIGMOID;
  if (sig && a->training && ((int64_t)a->B * a->HW < 2 || a->n < 2)) return MVP_EINVAL;  // one value per channel has no variance
  if (sig && !a->training && (!a->running_mean || !a->running_var)) return MVP_EINVAL;
  if (sig && ((a->running_mean == nullptr) != (a->running_var == nullptr))) return MVP_EINVAL;
  bn_dispatch(*a, true, sig && a->training, a->ld == 4 && aligned_to(a->x, 16), (hipStream_t)stream);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}

extern "C" int mvp_bn_act_bwd(const mvp_bn_act_args* a, void* stream) {
  if (!bn_shape_ok(a) || !a->grad_y) return MVP_EINVAL;
  const bool sig = a->act == ACT_SIGMOID;
  if (!a->grad_x && !(sig && (a->grad_gamma || a->grad_beta))) return MVP_EINVAL;  // nothing to compute
  bn_dispatch(*a, false, sig, a->ld == 4 && aligned_to(a->x, 16) && aligned_to(a->grad_x, 16), (hipStream_t)stream);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}

extern "C" int mvp_bce_loss_fwd_bwd(const mvp_bce_loss_args* a, void* stream) {
  if (!a || !a->pred || !a->target || !a->loss || !a->workspace || a->N <= 0) return MVP_EINVAL;
  if (a->workspace_bytes < MVP_BCE_WORKSPACE_BYTES || !aligned_to(a->workspace, 8)) return MVP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const bool v4 = aligned_to(a->pred, 16) && aligned_to(a->target, 16) && aligned_to(a->grad_pred, 16);
  int64_t nb = (a->N + 4095) / 4096;  // 4 x 16 bytes of each operand per thread
  nb = nb < 1 ? 1 : (nb > BCE_NB ? BCE_NB : nb);
  if (v4) hipLaunchKernelGGL(bce_kernel<true>, dim3((unsigned)nb), dim3(256), 0, s, *a);
  else hipLaunchKernelGGL(bce_kernel<false>, dim3((unsigned)nb), dim3(256), 0, s, *a);
  hipLaunchKernelGGL(bce_finalize_kernel, dim3(1), dim3(256), 0, s, *a, (int)nb);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}

extern "C" int mvp_binary_counts(const mvp_binary_counts_args* a, void* stream) {
  if (!a || !a->pred || !a->gt || !a->counts || a->G <= 0 || a->G > 65535 || a->n <= 0) return MVP_EINVAL;
  if (a->n > ((int64_t)1 << 40) / a->G || !aligned_to(a->counts, 8)) return MVP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(a->counts, 0, (size_t)a->G * 4 * sizeof(int64_t), s) != hipSuccess) return MVP_ELAUNCH;
  int64_t nb = (a->n + 4095) / 4096;
  const int64_t cap = a->G >= 1024 ? 1 : 1024 / a->G;  // about 1024 workgroups over all groups
  nb = nb < 1 ? 1 : (nb > cap ? cap : nb);
  // every row of a group must start 16-byte aligned for the vector form
  const bool v4 = aligned_to(a->pred, 16) && aligned_to(a->gt, 16) && (a->G == 1 || (a->n & 3) == 0);
  if (v4) hipLaunchKernelGGL(counts_kernel<true>, dim3((unsigned)nb, (unsigned)a->G), dim3(256), 0, s, *a);
  else hipLaunchKernelGGL(counts_kernel<false>, dim3((unsigned)nb, (unsigned)a->G), dim3(256), 0, s, *a);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}
