// Dense-CRF refinement of the MaskCut masks (include/mvp_hip.h, "Dense CRF"): the two Gaussian message-passing sums of a fully connected
// CRF evaluated exactly over all pixel pairs (mvp_crf_filter), the pointwise mean-field algebra (mvp_crf_update) and the mask
// post-processing of the reference's process_image: hole filling, the IoU rule, the union (mvp_mask_finish).  No kernel talks to the host,
// none uses a floating-point atomic; two calls give the same bits.
#include "mvp_common.h"

namespace {

#define CRF_T 16                 // tile edge: targets and sources are walked in 16 x 16 pixel tiles
#define CRF_TP (CRF_T * CRF_T)   // 256 = threads of a filter workgroup = pixels of a tile
#define CRF_MAX_F 8
#define CRF_SKIP_LOG2 (-40.f)    // a tile pair whose largest weight is <= 2^-40 is skipped
#define CRF_MAX_EDGE 4096
#define CRF_MAX_PIXELS (1 << 22)

struct filter_params {
  const uint8_t* rgb; const float* in; const uint8_t* active; float* out;
  int64_t in_stride, out_stride;
  int H, W, tiles_x, tiles_y;
  float cs, cc, cs_over_cc;  // -log2(e) / 2 * inverse variance (space, colour); their ratio when cc != 0
};

// Lanes own the 256 target pixels of one tile; the source tiles pass through LDS one after the other and are read as broadcasts.
// The differences are formed directly (exact small integers in fp32).  Per source row the 16 terms of a field are summed in fp32 and the
// row sums are folded into an fp64 accumulator, in row and tile order: every fp32 chunk has 16 positive terms.
template <int F, bool COLOR>
__global__ __launch_bounds__(CRF_TP) void crf_filter_kernel(const filter_params p) {
  __shared__ float4 s_px[CRF_TP];                       // r, g, b, field 0 of a source pixel
  __shared__ float s_f[F > 1 ? F - 1 : 1][CRF_TP];      // fields 1 .. F-1
  const int b = blockIdx.y;
  if (p.active && !p.active[b]) return;
  const int tid = threadIdx.x, lx = tid & (CRF_T - 1), ly = tid >> 4;
  const int tty = blockIdx.x / p.tiles_x, ttx = blockIdx.x - tty * p.tiles_x;
  const int tx = ttx * CRF_T + lx, ty = tty * CRF_T + ly;
  const bool valid = tx < p.W && ty < p.H;
  const int64_t N = (int64_t)p.H * p.W;
  const uint8_t* rgb = p.rgb + (size_t)b * N * 3;
  const float* in = p.in ? p.in + (size_t)b * p.in_stride : nullptr;
  float tr = 0.f, tg = 0.f, tb = 0.f;
  if (COLOR && valid) {
    const uint8_t* c = rgb + ((size_t)ty * p.W + tx) * 3;
    tr = (float)c[0]; tg = (float)c[1]; tb = (float)c[2];
  }
  double tot[F];
#pragma unroll
  for (int f = 0; f < F; ++f) tot[f] = 0.0;

  for (int sty = 0; sty < p.tiles_y; ++sty) {
    const int gy = max(0, abs(sty - tty) * CRF_T - (CRF_T - 1));
    for (int stx = 0; stx < p.tiles_x; ++stx) {
      const int gx = max(0, abs(stx - ttx) * CRF_T - (CRF_T - 1));
      // the closest pair of the two tiles bounds every weight of the pair (the colour term only lowers it); uniform over the workgroup
      if (p.cs * (float)(gx * gx + gy * gy) <= CRF_SKIP_LOG2) continue;
      __syncthreads();  // the tile before has been read
      {
        const int sx = stx * CRF_T + lx, sy = sty * CRF_T + ly;
        const bool ok = sx < p.W && sy < p.H;
        const size_t j = ok ? (size_t)sy * p.W + sx : 0;
        float4 px = {0.f, 0.f, 0.f, 0.f};
        if (COLOR && ok) { px.x = (float)rgb[j * 3]; px.y = (float)rgb[j * 3 + 1]; px.z = (float)rgb[j * 3 + 2]; }
        // a source outside the image carries the value 0 in every field: its (finite) weight adds nothing
        px.w = ok ? (in ? in[j] : 1.f) : 0.f;
        s_px[tid] = px;
#pragma unroll
        for (int f = 1; f < F; ++f) s_f[f - 1][tid] = ok ? (in ? in[(size_t)f * N + j] : 1.f) : 0.f;
      }
      __syncthreads();
      float e[CRF_T];  // the x part of the exponent: the same for every row of the source tile
#pragma unroll
      for (int k = 0; k < CRF_T; ++k) {
        const float dx = (float)(stx * CRF_T + k - tx);
        e[k] = p.cs * dx * dx;
      }
      for (int r = 0; r < CRF_T; ++r) {
        const float dy = (float)(sty * CRF_T + r - ty);
        const float ry = COLOR ? p.cs_over_cc * dy * dy : p.cs * dy * dy;
        float acc[F];
#pragma unroll
        for (int f = 0; f < F; ++f) acc[f] = 0.f;
#pragma unroll
        for (int k = 0; k < CRF_T; ++k) {
          const float4 s = s_px[r * CRF_T + k];
          float arg;
          if (COLOR) {
            const float dr = s.x - tr, dg = s.y - tg, db = s.z - tb;
            float t = __builtin_fmaf(db, db, ry);
            t = __builtin_fmaf(dg, dg, t);
            t = __builtin_fmaf(dr, dr, t);
            arg = __builtin_fmaf(t, p.cc, e[k]);
          } else {
            arg = e[k] + ry;
          }
          const float w = __builtin_amdgcn_exp2f(arg);  // one v_exp_f32 per pair; log2(e) is inside cs and cc
          acc[0] = __builtin_fmaf(w, s.w, acc[0]);
#pragma unroll
          for (int f = 1; f < F; ++f) acc[f] = __builtin_fmaf(w, s_f[f - 1][r * CRF_T + k], acc[f]);
        }
#pragma unroll
        for (int f = 0; f < F; ++f) tot[f] += (double)acc[f];
      }
    }
  }
  if (valid) {
    float* out = p.out + (size_t)b * p.out_stride + (size_t)ty * p.W + tx;
#pragma unroll
    for (int f = 0; f < F; ++f) out[(size_t)f * N] = (float)tot[f];
  }
}

template <int F>
void crf_filter_launch(const filter_params& p, int B, bool color, hipStream_t s) {
  const dim3 grid((unsigned)(p.tiles_x * p.tiles_y), (unsigned)B), block(CRF_TP);
  if (color) hipLaunchKernelGGL((crf_filter_kernel<F, true>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((crf_filter_kernel<F, false>), grid, block, 0, s, p);
}

// ------------------------------------------------------------------------------------------------ mean-field update
struct update_params {
  const float* mask; const uint8_t* active;
  float* norm_g; float* norm_b; const float* ones_g; const float* ones_b; const float* filt_g; const float* filt_b;
  float* q; float* x_g; float* x_b; uint8_t* map;
  int64_t stride, N;
  int mode;
  float w_g, w_b;
};

// Pointwise, in fp64 on the fp32 fields.  With two labels one field per object is enough: Q_0 = 1 - Q_1, so the filtered Q_0 is the
// filtered ones field minus the filtered Q_1, and the softmax over the two labels is the logistic function of a_1 - a_0.
__global__ __launch_bounds__(256) void crf_update_kernel(const update_params p) {
  const int b = blockIdx.z, f = blockIdx.y;
  if (p.active && !p.active[b]) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.N) return;
  const size_t bn = (size_t)b * p.N + i;
  if (p.mode == MVP_CRF_NORMALISE) {
    p.norm_g[bn] = (float)(1.0 / sqrt((double)p.norm_g[bn] + 1e-20));
    p.norm_b[bn] = (float)(1.0 / sqrt((double)p.norm_b[bn] + 1e-20));
    return;
  }
  const size_t k = (size_t)b * p.stride + (size_t)f * p.N + i;
  const double m = (double)p.mask[k];
  double d = 2.0 * m - 1.0;  // a_1 - a_0 of Q^0 = softmax(1 - m, m)
  const float ng = p.norm_g[bn], nb = p.norm_b[bn];
  if (p.mode == MVP_CRF_STEP) {
    const double p1 = 1.0 / (1.0 + exp(-d)), p0 = 1.0 / (1.0 + exp(d));
    const double u = log(fmax(p1, 1e-5)) - log(fmax(p0, 1e-5));  // U_0 - U_1 (unary_from_softmax clips at 1e-5)
    const double g = (double)ng * (2.0 * (double)p.filt_g[k] - (double)p.ones_g[bn]);
    const double c = (double)nb * (2.0 * (double)p.filt_b[k] - (double)p.ones_b[bn]);
    d = u + (double)p.w_g * g + (double)p.w_b * c;
  }
  const float q = (float)(1.0 / (1.0 + exp(-d)));
  p.q[k] = q;
  p.x_g[k] = ng * q;
  p.x_b[k] = nb * q;
  if (p.map) p.map[k] = d > 0.0 ? 1 : 0;  // Q_1 > Q_0; a tie goes to label 0
}

// ------------------------------------------------------------------------------------------------ mask post-processing
#define MF_THREADS 1024
#define MF_WAVES (MF_THREADS / 64)
#define MF_MAX_WORDS 32768  // 2^20 bits = 128 KiB of LDS
#define MF_WPT (MF_MAX_WORDS / MF_THREADS)
#define MF_MAX_PASSES 64

struct finish_params {
  const uint8_t* map; const uint8_t* ref; const uint8_t* active;
  uint8_t* refined; uint8_t* kept; uint8_t* union_mask;
  int64_t stride;
  int F, H, W, Wd, nwords;
};

// ndimage.binary_fill_holes of the mask whose complement (inside the image) is `open`: the background 4-connected to the border is
// flooded, everything else is the result.  `reach` holds the flood, one bit per pixel, rows padded to whole words; thread t owns
// the `per` = ceil(nwords / 1024) consecutive words from t * per on (LDS addresses that differ by immediates) and keeps their `open`
// words in registers.  A round takes the bits of the four neighbours and then runs along the row inside the word; words are only ever
// grown, and only by their owner, so rounds need no read / write separation.  On return reach is final and the workgroup is
// synchronised.
__device__ __forceinline__ void mf_flood(uint32_t* reach, const uint32_t (&open)[MF_WPT], const int H, const int W, const int Wd,
                                         const int nwords) {
  const int t = threadIdx.x, per = (nwords + MF_THREADS - 1) / MF_THREADS;
  // bit k: word k of this thread exists / has that neighbour inside the image (rolled: 32 divisions side by side would not fit the registers)
  uint32_t own = 0, up = 0, down = 0, left = 0, right = 0;
#pragma unroll 1
  for (int k = 0; k < per; ++k) {
    const int idx = t * per + k;
    if (idx >= nwords) break;
    const int y = idx / Wd, wx = idx - y * Wd;
    own |= 1u << k;
    up |= (y > 0 ? 1u : 0u) << k;
    down |= (y + 1 < H ? 1u : 0u) << k;
    left |= (wx > 0 ? 1u : 0u) << k;
    right |= (wx + 1 < Wd ? 1u : 0u) << k;
  }
  const uint32_t last_bit = 1u << ((W - 1) & 31);
#pragma unroll
  for (int k = 0; k < MF_WPT; ++k) {
    if ((own >> k) & 1u) {  // the seeds: the open pixels of the first and last row and column
      uint32_t seed = (((up & down) >> k) & 1u) ? 0u : 0xffffffffu;
      if (!((left >> k) & 1u)) seed |= 1u;
      if (!((right >> k) & 1u)) seed |= last_bit;
      reach[t * per + k] = seed & open[k];
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  __syncthreads();
  for (;;) {
    int changed = 0;
#pragma unroll
    for (int k = 0; k < MF_WPT; ++k) {
      const int idx = t * per + k;
      if ((own >> k) & 1u) {
        const uint32_t r = reach[idx];
        uint32_t o = open[k];
        asm volatile("" : "+v"(o));  // opaque per round: the run masks below depend on o alone, and hoisted out of the rounds they
                                     // are 8 registers per word, more than the 128 a lane of 1024 threads has
        uint32_t n = r;
        if ((up >> k) & 1u) n |= reach[idx - Wd];
        if ((down >> k) & 1u) n |= reach[idx + Wd];
        if ((left >> k) & 1u) n |= reach[idx - 1] >> 31;
        if ((right >> k) & 1u) n |= reach[idx + 1] << 31;
        n &= o;
        uint32_t g = n, pr = o;  // run towards the high bits through open pixels
        g |= pr & (g << 1); pr &= pr << 1;
        g |= pr & (g << 2); pr &= pr << 2;
        g |= pr & (g << 4); pr &= pr << 4;
        g |= pr & (g << 8); pr &= pr << 8;
        g |= pr & (g << 16);
        pr = o;                  // ... and towards the low bits
        g |= pr & (g >> 1); pr &= pr >> 1;
        g |= pr & (g >> 2); pr &= pr >> 2;
        g |= pr & (g >> 4); pr &= pr >> 4;
        g |= pr & (g >> 8); pr &= pr >> 8;
        g |= pr & (g >> 16);
        if (g != r) { reach[idx] = g; changed = 1; }
      }
      __builtin_amdgcn_sched_barrier(0);  // keep one word's loads from being hoisted over the others' (32 words would not fit the registers)
    }
    if (!__syncthreads_or(changed)) break;
  }
}

// the `open` words of this thread from up to nsrc byte masks ORed together (nsrc = 1: one mask).  The words are put together in a rolled
// loop through `stage` (the LDS array of the flood, free at this point) so that only the 32 words themselves stay in registers.
__device__ __forceinline__ void mf_open_words(uint32_t (&open)[MF_WPT], uint32_t* stage, const uint8_t* src, const int64_t src_step,
                                              const uint8_t* use, const int nsrc, const int W, const int Wd, const int nwords) {
#pragma unroll 1
  for (int idx = threadIdx.x; idx < nwords; idx += MF_THREADS) {
    const int y = idx / Wd, wx = idx - y * Wd;
    const int x0 = wx * 32, nb = min(32, W - x0);
    uint32_t fg = 0;
#pragma unroll 1
    for (int s = 0; s < nsrc; ++s) {
      if (use && !use[s]) continue;
      const uint8_t* row = src + (size_t)s * src_step + (size_t)y * W + x0;
      for (int j = 0; j < nb; ++j) fg |= (row[j] ? 1u : 0u) << j;
    }
    const uint32_t in_image = nb == 32 ? 0xffffffffu : ((1u << nb) - 1u);
    stage[idx] = ~fg & in_image;
  }
  __syncthreads();
  const int per = (nwords + MF_THREADS - 1) / MF_THREADS;
#pragma unroll
  for (int k = 0; k < MF_WPT; ++k) {
    const int idx = threadIdx.x * per + k;
    open[k] = (k < per && idx < nwords) ? stage[idx] : 0u;
  }
  __syncthreads();
}

// one workgroup per (pass, image): fill the holes of the MAP, compare with the CRF's input on integer counts, write the refined mask
__global__ __launch_bounds__(MF_THREADS) void mask_refine_kernel(const finish_params p) {
  __shared__ uint32_t reach[MF_MAX_WORDS];
  __shared__ int red[MF_WAVES * 2];
  const int f = blockIdx.x, b = blockIdx.y;
  if (p.active && !p.active[b * p.F + f]) return;
  const int N = p.H * p.W;
  const size_t base = (size_t)b * p.stride + (size_t)f * N;
  uint32_t open[MF_WPT];
  mf_open_words(open, reach, p.map + base, 0, nullptr, 1, p.W, p.Wd, p.nwords);
  mf_flood(reach, open, p.H, p.W, p.Wd, p.nwords);
  int inter = 0, uni = 0;
  for (int i = threadIdx.x; i < N; i += MF_THREADS) {
    const int y = i / p.W, x = i - y * p.W;
    const bool a = !((reach[y * p.Wd + (x >> 5)] >> (x & 31)) & 1u);
    const bool r = p.ref[base + i] != 0;
    inter += (a && r) ? 1 : 0;
    uni += (a || r) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { inter += __shfl_xor(inter, o, 64); uni += __shfl_xor(uni, o, 64); }
  if ((threadIdx.x & 63) == 0) { red[(threadIdx.x >> 6) * 2] = inter; red[(threadIdx.x >> 6) * 2 + 1] = uni; }
  __syncthreads();
  inter = 0; uni = 0;
  for (int w = 0; w < MF_WAVES; ++w) { inter += red[w * 2]; uni += red[w * 2 + 1]; }
  const bool keep = !(2 * inter < uni);  // IoU < 0.5 drops the mask; an empty union (0 / 0 in the reference: NaN < 0.5 is false) keeps it
  for (int i = threadIdx.x; i < N; i += MF_THREADS) {
    const int y = i / p.W, x = i - y * p.W;
    const bool a = !((reach[y * p.Wd + (x >> 5)] >> (x & 31)) & 1u);
    p.refined[base + i] = (keep && a) ? 1 : 0;
  }
  if (p.kept && threadIdx.x == 0) p.kept[b * p.F + f] = keep ? 1 : 0;
}

// one workgroup per image: the union of the active passes' refined masks, with its own holes filled
__global__ __launch_bounds__(MF_THREADS) void mask_union_kernel(const finish_params p) {
  __shared__ uint32_t reach[MF_MAX_WORDS];
  const int b = blockIdx.x;
  const int N = p.H * p.W;
  uint32_t open[MF_WPT];
  mf_open_words(open, reach, p.refined + (size_t)b * p.stride, N, p.active ? p.active + b * p.F : nullptr, p.F, p.W, p.Wd, p.nwords);
  mf_flood(reach, open, p.H, p.W, p.Wd, p.nwords);
  for (int i = threadIdx.x; i < N; i += MF_THREADS) {
    const int y = i / p.W, x = i - y * p.W;
    p.union_mask[(size_t)b * N + i] = ((reach[y * p.Wd + (x >> 5)] >> (x & 31)) & 1u) ? 0 : 1;
  }
}

inline bool crf_shape_ok(int B, int F, int H, int W) {
  return B > 0 && B <= 65535 && F > 0 && F <= CRF_MAX_F && H > 0 && W > 0 && H <= CRF_MAX_EDGE && W <= CRF_MAX_EDGE &&
         (int64_t)H * W <= CRF_MAX_PIXELS;
}

}  // namespace

extern "C" int mvp_crf_filter(const mvp_crf_filter_args* a, void* stream) {
  if (!a || !a->rgb || !a->out) return MVP_EINVAL;
  if (!crf_shape_ok(a->B, a->F, a->H, a->W)) return MVP_EINVAL;
  const int64_t N = (int64_t)a->H * a->W;
  if ((a->in && a->in_stride < a->F * N) || a->out_stride < a->F * N) return MVP_EINVAL;
  if (!(a->inv_var_xy > 0.f) || !(a->inv_var_rgb >= 0.f) || !(a->inv_var_xy < INFINITY) || !(a->inv_var_rgb < INFINITY)) return MVP_EINVAL;
  if (((uintptr_t)a->in & 3) || ((uintptr_t)a->out & 3)) return MVP_EINVAL;
  filter_params p;
  p.rgb = a->rgb; p.in = a->in; p.active = a->active; p.out = a->out; p.in_stride = a->in_stride; p.out_stride = a->out_stride;
  p.H = a->H; p.W = a->W; p.tiles_x = (a->W + CRF_T - 1) / CRF_T; p.tiles_y = (a->H + CRF_T - 1) / CRF_T;
  const double log2e = 1.4426950408889634;
  p.cs = (float)(-0.5 * log2e * (double)a->inv_var_xy);
  p.cc = (float)(-0.5 * log2e * (double)a->inv_var_rgb);
  const bool color = a->inv_var_rgb > 0.f;
  p.cs_over_cc = color ? (float)((double)a->inv_var_xy / (double)a->inv_var_rgb) : 0.f;
  hipStream_t s = (hipStream_t)stream;
  switch (a->F) {
    case 1: crf_filter_launch<1>(p, a->B, color, s); break;
    case 2: crf_filter_launch<2>(p, a->B, color, s); break;
    case 3: crf_filter_launch<3>(p, a->B, color, s); break;
    case 4: crf_filter_launch<4>(p, a->B, color, s); break;
    case 5: crf_filter_launch<5>(p, a->B, color, s); break;
    case 6: crf_filter_launch<6>(p, a->B, color, s); break;
    case 7: crf_filter_launch<7>(p, a->B, color, s); break;
    default: crf_filter_launch<8>(p, a->B, color, s); break;
  }
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}

extern "C" int mvp_crf_update(const mvp_crf_update_args* a, void* stream) {
  if (!a || !a->norm_g || !a->norm_b) return MVP_EINVAL;
  if (a->B <= 0 || a->B > 65535 || a->N <= 0 || a->N > CRF_MAX_PIXELS) return MVP_EINVAL;
  if (((uintptr_t)a->norm_g & 3) || ((uintptr_t)a->norm_b & 3)) return MVP_EINVAL;
  int F = 1;
  if (a->mode == MVP_CRF_INIT || a->mode == MVP_CRF_STEP) {
    F = a->F;
    if (F <= 0 || F > CRF_MAX_F || a->stride < F * a->N) return MVP_EINVAL;
    if (!a->mask || !a->q || !a->x_g || !a->x_b) return MVP_EINVAL;
    if (a->mode == MVP_CRF_STEP && (!a->ones_g || !a->ones_b || !a->filt_g || !a->filt_b)) return MVP_EINVAL;
    if (((uintptr_t)a->mask & 3) || ((uintptr_t)a->q & 3) || ((uintptr_t)a->x_g & 3) || ((uintptr_t)a->x_b & 3) || ((uintptr_t)a->ones_g & 3) ||
        ((uintptr_t)a->ones_b & 3) || ((uintptr_t)a->filt_g & 3) || ((uintptr_t)a->filt_b & 3))
      return MVP_EINVAL;
  } else if (a->mode != MVP_CRF_NORMALISE) {
    return MVP_EINVAL;
  }
  update_params p;
  p.mask = a->mask; p.active = a->active; p.norm_g = a->norm_g; p.norm_b = a->norm_b; p.ones_g = a->ones_g; p.ones_b = a->ones_b;
  p.filt_g = a->filt_g; p.filt_b = a->filt_b; p.q = a->q; p.x_g = a->x_g; p.x_b = a->x_b; p.map = a->map;
  p.stride = a->stride; p.N = a->N; p.mode = a->mode; p.w_g = a->w_g; p.w_b = a->w_b;
  const dim3 grid((unsigned)((a->N + 255) / 256), (unsigned)F, (unsigned)a->B);
  hipLaunchKernelGGL(crf_update_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}

extern "C" int mvp_mask_finish(const mvp_mask_finish_args* a, void* stream) {
  if (!a || !a->map || !a->ref || !a->refined) return MVP_EINVAL;
  if (a->B <= 0 || a->B > 65535 || a->F <= 0 || a->F > MF_MAX_PASSES || a->H <= 0 || a->W <= 0) return MVP_EINVAL;
  if (a->H > 65535 || a->W > CRF_MAX_PIXELS) return MVP_EINVAL;
  const int Wd = (a->W + 31) / 32;
  if ((int64_t)a->H * Wd > MF_MAX_WORDS) return MVP_EINVAL;
  if (a->stride < (int64_t)a->F * a->H * a->W) return MVP_EINVAL;
  finish_params p;
  p.map = a->map; p.ref = a->ref; p.active = a->active; p.refined = a->refined; p.kept = a->kept; p.union_mask = a->union_mask;
  p.stride = a->stride; p.F = a->F; p.H = a->H; p.W = a->W; p.Wd = Wd; p.nwords = a->H * Wd;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(mask_refine_kernel, dim3((unsigned)a->F, (unsigned)a->B), dim3(MF_THREADS), 0, s, p);
  if (a->union_mask) hipLaunchKernelGGL(mask_union_kernel, dim3((unsigned)a->B), dim3(MF_THREADS), 0, s, p);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}
