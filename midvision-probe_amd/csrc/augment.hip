// mvp_augment_stats / mvp_augment_apply: the training augmentation of an NYU / NAVI batch on the device (reference: get_nyu_transforms,
// evals/datasets/utils.py:160-218, and the shared albumentations transform of nyu.py:227-239), two launches per batch.
//     image  -> RandomApply([ColorJitter(0.2, 0.2, 0.2, 0.2)], 0.8) -> flip -> rotate -> resized crop -> Normalize(mean, std)
//     depth, normals                                               -> flip -> rotate -> resized crop         (the same draws)
// The draws come from a device table of MVP_AUGMENT_WORDS words per image (include/mvp_hip.h has the layout and the exact maps).
// Every geometric stage is nearest-neighbour, so the three stages compose to one integer source index per output pixel, and the jitter,
// being pointwise, is evaluated only on the pixels that are gathered.  The one non-local quantity is the contrast operation's mean grey
// value over the whole source image at the moment contrast is reached in that image's order:
// Launch 1, grid = (MVP_AUGMENT_PARTIALS, B): workgroup k of image b walks the pixel groups g (4 pixels) with (g / 256) % 32 == k, runs
// the operations that precede contrast, and sums the grey values in fp64: per lane in pixel order, a butterfly inside the wave, the four
// waves in a fixed order through LDS (csrc/mvp_reduce.h).  One partial per workgroup (0 for an image whose jitter is off): no atomics.
// Launch 2, grid = (rows of 256 lanes, B): a lane owns four consecutive output x of one row.  It adds the image's partials in index
// order (every lane the same 32 additions: every workgroup gets the same bits), builds the composed map, gathers the source pixel of the
// image, the depth and the normals, runs the jitter chain in registers, normalises and writes each plane with one 16-byte store (scalar
// stores where Wo % 4 != 0 leaves the rows unaligned, which also covers the ragged last lane of a row).
// Rows of the source are read by neighbouring lanes in x order (reversed under a flip, slanted under a rotation): the loads of the uint8
// form are byte loads of 3-byte pixels, those of the fp32 form dword loads per plane.
#include <math.h>

#include "mvp_reduce.h"

namespace {

#define AU_THREADS 256
#define AU_P MVP_AUGMENT_PARTIALS
#define AU_K MVP_AUGMENT_WORDS
#define AU_MAX_SIDE 32768  // dy * ch and dx * cw then fit 32 bits

struct au_params {
  const void* image; const float* depth; const float* snorm; const int32_t* table;
  double* partials;
  float* out_image; float* out_depth; float* out_snorm;
  int B, H, W, Ho, Wo;
  int vec;  // stats: source groups are aligned for wide loads; apply: output rows are aligned for 16-byte stores
  float mean[3], std[3];
};

__device__ __forceinline__ float au_clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }
__device__ __forceinline__ float au_grey(float r, float g, float b) { return 0.2989f * r + 0.587f * g + 0.114f * b; }
// torchvision _blend(x, y, f) for float tensors
__device__ __forceinline__ float au_blend(float x, float y, float f) { return au_clamp01(f * x + (1.f - f) * y); }

// torchvision adjust_hue: _rgb2hsv, h <- (h + f) mod 1, _hsv2rgb, with its branch structure (a grey pixel has s = 0 and h = 0, a black
// one v = 0 as well).  The three differences maxc - x share ONE reciprocal of the chroma instead of three divisions.
__device__ __forceinline__ void au_hue(float& r, float& g, float& b, float f) {
  const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
  const bool eq = maxc == minc;
  const float cr = maxc - minc;
  const float s = cr / (eq ? 1.f : maxc);
  const float inv = 1.f / (eq ? 1.f : cr);
  const float rc = (maxc - r) * inv, gc = (maxc - g) * inv, bc = (maxc - b) * inv;
  float h = maxc == r ? bc - gc : (maxc == g ? 2.f + rc - bc : 4.f + gc - rc);
  h = fmodf(h / 6.f + 1.f, 1.f);
  h += f;
  h -= floorf(h);  // Python's % 1.0 (a tiny negative sum rounds to 1.0, which the sector index below folds to 0 like torch does)
  const float v = maxc, h6 = h * 6.f, fl = floorf(h6), fr = h6 - fl;
  int i = (int)fl % 6;
  i = i < 0 ? i + 6 : i;
  const float p = au_clamp01(v * (1.f - s)), q = au_clamp01(v * (1.f - s * fr)), t = au_clamp01(v * (1.f - s * (1.f - fr)));
  r = i == 0 ? v : (i == 1 ? q : (i == 2 ? p : (i == 3 ? p : (i == 4 ? t : v))));
  g = i == 0 ? t : (i == 1 ? v : (i == 2 ? v : (i == 3 ? q : (i == 4 ? p : p))));
  b = i == 0 ? p : (i == 1 ? p : (i == 2 ? t : (i == 3 ? v : (i == 4 ? v : q))));
}

struct au_jit {
  int order;
  float fb, fc, fs, fh;
};

// The four operations in the image's order; UNTIL_CONTRAST stops in front of contrast (what the statistics pass needs).
template <bool UNTIL_CONTRAST>
__device__ __forceinline__ void au_chain(float& r, float& g, float& b, const au_jit& j, float m) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int op = (j.order >> (2 * i)) & 3;  // uniform over the workgroup
    if (op == 0) {
      r = au_clamp01(j.fb * r); g = au_clamp01(j.fb * g); b = au_clamp01(j.fb * b);
    } else if (op == 1) {
      if (UNTIL_CONTRAST) return;
      r = au_blend(r, m, j.fc); g = au_blend(g, m, j.fc); b = au_blend(b, m, j.fc);
    } else if (op == 2) {
      const float y = au_grey(r, g, b);
      r = au_blend(r, y, j.fs); g = au_blend(g, y, j.fs); b = au_blend(b, y, j.fs);
    } else {
      au_hue(r, g, b, j.fh);
    }
  }
}

__device__ __forceinline__ au_jit au_read_jit(const int32_t* t) {
  au_jit j;
  j.order = t[1];
  j.fb = u2f((uint32_t)t[2]); j.fc = u2f((uint32_t)t[3]); j.fs = u2f((uint32_t)t[4]); j.fh = u2f((uint32_t)t[5]);
  return j;
}

// pixel `src` of image b as floats in [0, 1]
template <bool U8>
__device__ __forceinline__ void au_load_px(const void* image, size_t b, int HW, int src, float& r, float& g, float& bl) {
  if (U8) {
    const uint8_t* q = (const uint8_t*)image + (b * (size_t)HW + (size_t)src) * 3;
    r = (float)q[0] / 255.f; g = (float)q[1] / 255.f; bl = (float)q[2] / 255.f;
  } else {
    const float* q = (const float*)image + b * 3 * (size_t)HW + (size_t)src;
    r = q[0]; g = q[HW]; bl = q[2 * (size_t)HW];
  }
}

// the 4 pixels i0 .. i0 + 3 of image b (the last n of them repeat pixel i0 + n - 1 where the image ends inside the group)
template <bool U8>
__device__ __forceinline__ void au_load_group(const au_params& p, int b, int HW, int i0, int n, float (&r)[4], float (&g)[4], float (&bl)[4]) {
  if (p.vec) {  // HW % 4 == 0: every group is whole and starts on a dword (uint8) / on 16 bytes (fp32)
    if (U8) {
      const uint32_t* q = (const uint32_t*)((const uint8_t*)p.image + ((size_t)b * HW + i0) * 3);
      const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
      r[0] = (float)(w0 & 255) / 255.f; g[0] = (float)((w0 >> 8) & 255) / 255.f; bl[0] = (float)((w0 >> 16) & 255) / 255.f;
      r[1] = (float)(w0 >> 24) / 255.f; g[1] = (float)(w1 & 255) / 255.f; bl[1] = (float)((w1 >> 8) & 255) / 255.f;
      r[2] = (float)((w1 >> 16) & 255) / 255.f; g[2] = (float)(w1 >> 24) / 255.f; bl[2] = (float)(w2 & 255) / 255.f;
      r[3] = (float)((w2 >> 8) & 255) / 255.f; g[3] = (float)((w2 >> 16) & 255) / 255.f; bl[3] = (float)(w2 >> 24) / 255.f;
    } else {
      const float* q = (const float*)p.image + (size_t)b * 3 * HW + i0;
      const float4 vr = *(const float4*)q, vg = *(const float4*)(q + HW), vb = *(const float4*)(q + 2 * (size_t)HW);
      r[0] = vr.x; r[1] = vr.y; r[2] = vr.z; r[3] = vr.w;
      g[0] = vg.x; g[1] = vg.y; g[2] = vg.z; g[3] = vg.w;
      bl[0] = vb.x; bl[1] = vb.y; bl[2] = vb.z; bl[3] = vb.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) au_load_px<U8>(p.image, (size_t)b, HW, i0 + min(j, n - 1), r[j], g[j], bl[j]);  // in the image whatever j
  }
}

template <bool U8>
__global__ __launch_bounds__(AU_THREADS) void augment_stats_kernel(const au_params p) {
  __shared__ double red[AU_THREADS / 64][1];
  const int b = blockIdx.y, k = blockIdx.x;
  const int32_t* t = p.table + (size_t)b * AU_K;
  const int HW = p.H * p.W, ngroups = (HW + 3) >> 2;
  double acc[1] = {0.0};
  if (t[0] & 1) {  // uniform
    const au_jit jit = au_read_jit(t);
    // one group per trip: the walk is bound by the jitter arithmetic, not by load latency (four groups in flight per lane measured
    // 1.5x to 2.2x SLOWER: 115 VGPRs, and the trips past the image's end still pay for their chains)
    for (int g = k * AU_THREADS + (int)threadIdx.x; g < ngroups; g += AU_P * AU_THREADS) {
      const int i0 = g << 2, n = min(4, HW - i0);
      float r[4], gg[4], bb[4];
      au_load_group<U8>(p, b, HW, i0, n, r, gg, bb);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        au_chain<true>(r[j], gg[j], bb[j], jit, 0.f);
        acc[0] += j < n ? (double)au_grey(r[j], gg[j], bb[j]) : 0.0;
      }
    }
  }
  block_sum_once<1>(acc, red);
  if (threadIdx.x == 0) p.partials[(size_t)b * AU_P + k] = acc[0];
}

// index i reflected into [0, n) without repeating the edge (reflect-101), any i
__device__ __forceinline__ int au_reflect(int i, int n) {
  const int period = 2 * (n - 1);
  int m = i % period;
  m = m < 0 ? m + period : m;
  return m > n - 1 ? period - m : m;
}

template <bool U8>
__global__ __launch_bounds__(AU_THREADS) void augment_apply_kernel(const au_params p) {
  const int b = blockIdx.y;
  const int Q = (p.Wo + 3) >> 2;
  const int64_t tt = (int64_t)blockIdx.x * AU_THREADS + threadIdx.x;
  if (tt >= (int64_t)Q * p.Ho) return;
  const int dy = (int)(tt / Q), dx0 = ((int)(tt - (int64_t)dy * Q)) << 2;
  const int H = p.H, W = p.W, HW = H * W;
  const int32_t* t = p.table + (size_t)b * AU_K;
  const int flags = t[0];
  const bool jitter = (flags & 1) && p.partials, flip = flags & 2, rot = flags & 4;
  const au_jit jit = au_read_jit(t);
  const float cs = u2f((uint32_t)t[6]), sn = u2f((uint32_t)t[7]);
  // the box clamped into the image: no table content takes a read outside the inputs
  const int cw = min(max(t[10], 1), W), ch = min(max(t[11], 1), H);
  const int x0 = min(max(t[8], 0), W - cw), y0 = min(max(t[9], 0), H - ch);
  float m = 0.f;
  if (jitter) {  // uniform
    const double* part = p.partials + (size_t)b * AU_P;
    double s = 0.0;
#pragma unroll 8
    for (int i = 0; i < AU_P; ++i) s += part[i];
    m = (float)(s / (double)HW);
  }
  const float cx = 0.5f * (float)(W - 1), cy = 0.5f * (float)(H - 1);
  const int sy = y0 + (dy * ch) / p.Ho;
  float o[3][4], od[4], on[3][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int dx = min(dx0 + j, p.Wo - 1);  // a lane past the row's end repeats the last pixel and drops it at the store
    int xx = x0 + (dx * cw) / p.Wo, yy = sy;
    if (rot) {  // uniform
      const float u = (float)xx - cx, v = (float)yy - cy;
      const float xs = __builtin_fmaf(cs, u, __builtin_fmaf(-sn, v, cx)), ys = __builtin_fmaf(cs, v, __builtin_fmaf(sn, u, cy));
      xx = au_reflect((int)floorf(xs + 0.5f), W);
      yy = au_reflect((int)floorf(ys + 0.5f), H);
    }
    if (flip) xx = W - 1 - xx;
    const int src = yy * W + xx;
    float r, g, bl;
    au_load_px<U8>(p.image, (size_t)b, HW, src, r, g, bl);
    od[j] = p.depth[(size_t)b * HW + src];
    if (p.snorm) {
      const float* q = p.snorm + (size_t)b * 3 * HW + src;
      on[0][j] = q[0]; on[1][j] = q[HW]; on[2][j] = q[2 * (size_t)HW];
    }
    if (jitter) au_chain<false>(r, g, bl, jit, m);
    o[0][j] = (r - p.mean[0]) / p.std[0];
    o[1][j] = (g - p.mean[1]) / p.std[1];
    o[2][j] = (bl - p.mean[2]) / p.std[2];
  }
  const size_t plane = (size_t)p.Ho * p.Wo, row = (size_t)dy * p.Wo + dx0;
  const int n = min(4, p.Wo - dx0);
  float* oi = p.out_image + (size_t)b * 3 * plane + row;
  float* odp = p.out_depth + (size_t)b * plane + row;
  float* onp = p.snorm ? p.out_snorm + (size_t)b * 3 * plane + row : nullptr;
  if (p.vec) {  // Wo % 4 == 0: n == 4 and every row starts on 16 bytes
#pragma unroll
    for (int c = 0; c < 3; ++c) *(float4*)(oi + c * plane) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
    *(float4*)odp = make_float4(od[0], od[1], od[2], od[3]);
    if (onp) {
#pragma unroll
      for (int c = 0; c < 3; ++c) *(float4*)(onp + c * plane) = make_float4(on[c][0], on[c][1], on[c][2], on[c][3]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < n) {
#pragma unroll
        for (int c = 0; c < 3; ++c) oi[c * plane + j] = o[c][j];
        odp[j] = od[j];
        if (onp) {
#pragma unroll
          for (int c = 0; c < 3; ++c) onp[c * plane + j] = on[c][j];
        }
      }
    }
  }
}

inline bool au_source_ok(const void* image, const int32_t* table, int B, int H, int W, int image_u8) {
  if (!image || !table || B <= 0 || B > 65535 || H < 4 || W < 4 || H > AU_MAX_SIDE || W > AU_MAX_SIDE) return false;
  if ((int64_t)H * W > ((int64_t)1 << 29)) return false;
  if (image_u8 != 0 && image_u8 != 1) return false;
  return aligned_to(table, 4) && (image_u8 || aligned_to(image, 4));
}

}  // namespace

extern "C" int64_t mvp_augment_partials_bytes(int B) { return B > 0 ? (int64_t)B * AU_P * (int64_t)sizeof(double) : 0; }

extern "C" int mvp_augment_stats(const mvp_augment_stats_args* a, void* stream) {
  if (!a || !au_source_ok(a->image, a->params, a->B, a->H, a->W, a->image_u8)) return MVP_EINVAL;
  if (!a->partials || !aligned_to(a->partials, 8) || a->partials_bytes < mvp_augment_partials_bytes(a->B)) return MVP_EINVAL;
  au_params p = {};
  p.image = a->image; p.table = a->params; p.partials = a->partials;
  p.B = a->B; p.H = a->H; p.W = a->W;
  p.vec = ((a->H * a->W) & 3) == 0 && aligned_to(a->image, a->image_u8 ? 4 : 16);
  const dim3 grid(AU_P, (unsigned)a->B);
  hipStream_t s = (hipStream_t)stream;
  if (a->image_u8) hipLaunchKernelGGL(augment_stats_kernel<true>, grid, dim3(AU_THREADS), 0, s, p);
  else hipLaunchKernelGGL(augment_stats_kernel<false>, grid, dim3(AU_THREADS), 0, s, p);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}

extern "C" int mvp_augment_apply(const mvp_augment_apply_args* a, void* stream) {
  if (!a || !au_source_ok(a->image, a->params, a->B, a->H, a->W, a->image_u8)) return MVP_EINVAL;
  if (!a->depth || !a->out_image || !a->out_depth || (a->snorm == nullptr) != (a->out_snorm == nullptr)) return MVP_EINVAL;
  if (a->Ho <= 0 || a->Wo <= 0 || a->Ho > AU_MAX_SIDE || a->Wo > AU_MAX_SIDE) return MVP_EINVAL;
  if (a->partials && (!aligned_to(a->partials, 8) || a->partials_bytes < mvp_augment_partials_bytes(a->B))) return MVP_EINVAL;
  if (!aligned_to(a->depth, 4) || !aligned_to(a->snorm, 4) || !aligned_to(a->out_image, 4) || !aligned_to(a->out_depth, 4) ||
      !aligned_to(a->out_snorm, 4))
    return MVP_EINVAL;
  if (!(a->std_r != 0.f) || !(a->std_g != 0.f) || !(a->std_b != 0.f)) return MVP_EINVAL;
  au_params p = {};
  p.image = a->image; p.depth = a->depth; p.snorm = a->snorm; p.table = a->params; p.partials = (double*)a->partials;
  p.out_image = a->out_image; p.out_depth = a->out_depth; p.out_snorm = a->out_snorm;
  p.B = a->B; p.H = a->H; p.W = a->W; p.Ho = a->Ho; p.Wo = a->Wo;
  p.mean[0] = a->mean_r; p.mean[1] = a->mean_g; p.mean[2] = a->mean_b;
  p.std[0] = a->std_r; p.std[1] = a->std_g; p.std[2] = a->std_b;
  p.vec = (a->Wo & 3) == 0 && aligned_to(a->out_image, 16) && aligned_to(a->out_depth, 16) && aligned_to(a->out_snorm, 16);
  const int64_t lanes = (int64_t)((a->Wo + 3) >> 2) * a->Ho;
  const dim3 grid((unsigned)((lanes + AU_THREADS - 1) / AU_THREADS), (unsigned)a->B);
  hipStream_t s = (hipStream_t)stream;
  if (a->image_u8) hipLaunchKernelGGL(augment_apply_kernel<true>, grid, dim3(AU_THREADS), 0, s, p);
  else hipLaunchKernelGGL(augment_apply_kernel<false>, grid, dim3(AU_THREADS), 0, s, p);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}
