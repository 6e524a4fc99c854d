// mvp_pixel_score: the pixel-level baselines of the 2AFC evaluation, PSNR and SSIM, scored like mvp_twoafc_score (csrc/twoafc.hip):
// sim[b] = {score(ref, left), score(ref, right)}, pred[b] = sim_left > sim_right ? 0 : 1, running TP / FP / FN / TN.
//     SSIM (reference: evals/utils/losses.py:222-251, size_average=False): 11 x 11 Gaussian window (sigma 1.5, fp32 weights), zero
//          padding, per channel; the mean of the map over C * H * W.
//     PSNR: 10 log10(1 / mse), mse = mean over C * H * W of (a - b)^2; the peak is 1.      (include/mvp_hip.h has the full definition)
//
// SSIM, pass 1, one workgroup per (triplet, channel, 16 x 32 tile of output pixels).  The three images are read ONCE:
//   load   the tile with a 5-pixel halo of the three images into LDS as fp32 (26 x 42 each, 13 KB in all); positions outside the image
//          hold 0, which is the reference's zero padding.  Dword loads with a bounds test: any W, any base address.
//   filter separably, in fp64.  Vertical: a lane takes four consecutive rows of one column of the haloed tile and forms the 11-tap
//          sums of the EIGHT planes r, l, q, r^2, l^2, q^2, r l, r q (the reference image's mean and second moment serve both pairs:
//          eight, not ten); the product of two fp32 values is exact in fp64, and a raw value is read, converted and multiplied once
//          for the four sums it belongs to.  The sums are stored as fp64 (8 x 16 x 42 x 8 = 42 KB).  Horizontal: a lane takes two
//          adjacent output pixels and reads the 12 values they span as six aligned 16-byte pairs per plane (ds_read_b128).  The weights
//          are the fp32 values of the reference's 1-D window; the 2-D window the reference convolves with is their outer product
//          ROUNDED to fp32 (whose sum is not the square of the 1-D sum), so the two differ by 2^-24 relative per tap: measured on the
//          scores, <= 3e-8 on noise and <= 1.7e-7 on smooth images, where E - mu^2 is small and torch's own fp32 error is 1e-5.
//   map    in fp64 with contraction off: E[x^2] - mu^2 cancels against C2 = 9e-4, which is where fp32 loses 1e-5 on smooth 8-bit
//          images.  Both pairs go through ONE inlined sequence (ssim_point): bitwise-equal left and right give bitwise-equal scores,
//          and a candidate bitwise equal to the reference image gives numerator == denominator in every pixel (2 m m == m m + m m),
//          i.e. a map of exactly 1.
//   sum    the two maps over the tile's pixels inside the image, fp64, fixed order; two partials per workgroup to the workspace.
// 56 KB of LDS per workgroup: two workgroups (8 waves) per CU; 92 VGPRs.  A 32 x 32 tile would cut the halo reads from 2.1x to 1.7x but
// needs 107 KB with fp64 planes, one workgroup per CU; 16 x 32 keeps a row of outputs at 32 columns (16 lanes x 16 bytes, contiguous).
// The kernel is bound by its fp64 arithmetic (about 2 700 wave instructions per tile, most of them v_fma_f64 at 4 cycles), not by
// memory: 5 to 7 times a copy of the same bytes (tools/pixelsim_bench.py).
// PSNR, pass 1, one workgroup per (triplet, chunk of >= 4096 elements): differences and squares in fp64; a lane takes four consecutive
// elements at a time, with one 16-byte load when ld % 4 == 0 and the bases are 16-byte aligned, with four dword loads otherwise (the
// same elements in the same order: the bits do not depend on the alignment); two partials per workgroup.
// Pass 2 (both metrics), one wave per triplet: folds the partial rows in a fixed order (lane j takes rows j, j + 64, ...; then the
// butterfly), forms both scores with one inlined sequence, rounds each ONCE to fp32 and counts.  No floating-point atomics
// (csrc/mvp_reduce.h has the order of every sum); the counts are integers, whose 64-bit atomics are exact in any order.  Two calls give
// the same bits.  Nothing between C * H * W and ld is read.
#include <math.h>

#include "mvp_reduce.h"

namespace {

#define PX_THREADS 256
#define PX_HALO 5
#define PX_TAPS 11
#define PX_TH 16  // output rows of a tile
#define PX_TW 32  // output columns of a tile
#define PX_RH (PX_TH + 2 * PX_HALO)  // 26 rows of the haloed tile
#define PX_RW (PX_TW + 2 * PX_HALO)  // 42 columns of the haloed tile
#define PX_PLANES 8
#define PX_VR 4  // rows a lane of the vertical pass takes (divides PX_TH)
static_assert(PX_TH % PX_VR == 0 && PX_TW % 2 == 0 && PX_RW % 2 == 0 && PX_TH * (PX_TW / 2) == PX_THREADS, "tile geometry");
#define PX_CHUNK_ELEMS 4096  // PSNR: elements of one image a chunk holds at least
#define PX_MAX_CHUNKS 1024   // PSNR: chunks per triplet at most

struct px_params {
  const float* ref; const float* left; const float* right; const float* label;
  float* sim; int32_t* pred; int64_t* counts; double* ws;
  int64_t ld, n;        // n = C * H * W
  int64_t chunk;        // PSNR: elements per chunk (a multiple of 4)
  int B, C, H, W, metric;
  int tx, ty;           // SSIM: tiles along W and H
  int nblk;             // workgroups (= partial rows) per triplet
};

// gaussian(11, 1.5) of the reference as it evaluates in fp32: exp(-(k - 5)^2 / 4.5) rounded to fp32, divided by their fp32 sum
// (tests/test_pixelsim_cpu.py holds these literals to evals.utils.losses.gaussian and to the recorded create_window, to the bit)
__device__ __constant__ const float PX_G[PX_TAPS] = {
    0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f,
    0x1.b43c3ep-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};

// partial rows per triplet; false where the call is rejected
inline bool px_partition(int B, int C, int H, int W, int metric, px_params* p) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || (metric != 0 && metric != 1)) return false;
  if ((int64_t)C * H > (int64_t)0x7fffffff) return false;  // (then C * H * W < 2^62: no overflow below)
  const int64_t n = (int64_t)C * H * W;
  if (n > (int64_t)0x7fffffff) return false;
  int64_t nblk, chunk = PX_CHUNK_ELEMS;
  int tx = 0, ty = 0;
  if (metric == 1) {
    tx = (W - 1) / PX_TW + 1;
    ty = (H - 1) / PX_TH + 1;
    nblk = (int64_t)C * tx * ty;  // <= n
  } else {
    while ((n + chunk - 1) / chunk > PX_MAX_CHUNKS) chunk *= 2;
    nblk = (n + chunk - 1) / chunk;
  }
  if ((int64_t)B * nblk > (int64_t)0x7fffffff) return false;
  if (p) { p->n = n; p->chunk = chunk; p->tx = tx; p->ty = ty; p->nblk = (int)nblk; }
  return true;
}

// the workgroup's two sums (left, right) to its partial row
__device__ __forceinline__ void px_store_partial(double sum_l, double sum_q, double (*red)[2], double* out) {
  double v[2] = {sum_l, sum_q};
  block_sum_once<2>(v, red);
  if (threadIdx.x == 0) {
    out[0] = v[0];
    out[1] = v[1];
  }
}

// One pixel of the SSIM map of a pair from its five filtered planes.  Every operation is rounded on its own (no fma): with
// mu1 == mu2 and e11 == e22 == e12 bitwise, 2 * m12 == m11 + m22 and 2 * s12 == s1 + s2 bitwise, hence num == den.
__device__ __forceinline__ double ssim_point(double mu1, double mu2, double e11, double e22, double e12) {
#pragma clang fp contract(off)
  const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
  const double m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2;
  const double s1 = e11 - m11, s2 = e22 - m22, s12 = e12 - m12;
  const double num = (2.0 * m12 + C1) * (2.0 * s12 + C2);
  const double den = ((m11 + m22) + C1) * ((s1 + s2) + C2);
  return num / den;
}

__global__ __launch_bounds__(PX_THREADS) void pixel_ssim_partial_kernel(const px_params p) {
  __shared__ float raw[3][PX_RH][PX_RW];
  __shared__ __attribute__((aligned(16))) double vert[PX_PLANES][PX_TH][PX_RW];  // (rows of 336 bytes: 16-byte pairs at even columns)
  __shared__ double red[PX_THREADS / 64][2];
  const int tiles = p.tx * p.ty;
  const int b = blockIdx.x / p.nblk, rem = blockIdx.x - b * p.nblk;
  const int c = rem / tiles, t = rem - c * tiles;
  const int y0 = (t / p.tx) * PX_TH, x0 = (t % p.tx) * PX_TW;
  const size_t plane = (size_t)b * (size_t)p.ld + (size_t)c * (size_t)p.H * (size_t)p.W;
  const float* r = p.ref + plane;
  const float* l = p.left + plane;
  const float* q = p.right + plane;
  for (int i = threadIdx.x; i < PX_RH * PX_RW; i += PX_THREADS) {
    const int yy = i / PX_RW, xx = i - yy * PX_RW;
    const int gy = y0 + yy - PX_HALO, gx = x0 + xx - PX_HALO;
    float vr = 0.f, vl = 0.f, vq = 0.f;
    if (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) {  // inside the image: inside [0, C * H * W)
      const size_t o = (size_t)gy * (size_t)p.W + (size_t)gx;
      vr = r[o];
      vl = l[o];
      vq = q[o];
    }
    raw[0][yy][xx] = vr;
    raw[1][yy][xx] = vl;
    raw[2][yy][xx] = vq;
  }
  __syncthreads();
  // vertical: a lane takes PX_VR consecutive rows of one column, so that a raw value is read, converted and multiplied once for the
  // up to PX_VR sums it belongs to (14 raw rows for 4 outputs, not 44); every sum takes its taps in the order k = 0 .. 10
  for (int i = threadIdx.x; i < (PX_TH / PX_VR) * PX_RW; i += PX_THREADS) {
    const int yg = i / PX_RW, xx = i - yg * PX_RW, y = yg * PX_VR;
    double a[PX_VR][PX_PLANES];
#pragma unroll
    for (int o = 0; o < PX_VR; ++o) {
#pragma unroll
      for (int j = 0; j < PX_PLANES; ++j) a[o][j] = 0.0;
    }
#pragma unroll
    for (int j = 0; j < PX_TAPS + PX_VR - 1; ++j) {
      const double vr = (double)raw[0][y + j][xx], vl = (double)raw[1][y + j][xx], vq = (double)raw[2][y + j][xx];
      const double v[PX_PLANES] = {vr, vl, vq, vr * vr, vl * vl, vq * vq, vr * vl, vr * vq};  // (exact products)
#pragma unroll
      for (int o = 0; o < PX_VR; ++o) {
        const int k = j - o;  // the tap of raw row y + j in the sum of output row y + o
        if (k >= 0 && k < PX_TAPS) {
          const double g = (double)PX_G[k];
#pragma unroll
          for (int pl = 0; pl < PX_PLANES; ++pl) a[o][pl] = fma(g, v[pl], a[o][pl]);
        }
      }
    }
#pragma unroll
    for (int o = 0; o < PX_VR; ++o) {
#pragma unroll
      for (int j = 0; j < PX_PLANES; ++j) vert[j][y + o][xx] = a[o][j];
    }
  }
  __syncthreads();
  // horizontal: a lane takes two adjacent outputs (x even) and reads the 12 values they span as six aligned 16-byte pairs per plane
  const int y = threadIdx.x / (PX_TW / 2), x = (threadIdx.x % (PX_TW / 2)) * 2;
  double m0[PX_PLANES], m1[PX_PLANES];
#pragma unroll
  for (int j = 0; j < PX_PLANES; ++j) m0[j] = m1[j] = 0.0;
#pragma unroll
  for (int jj = 0; jj < (PX_TAPS + 1) / 2; ++jj) {
#pragma unroll
    for (int j = 0; j < PX_PLANES; ++j) {
      const double2 v = *(const double2*)&vert[j][y][x + 2 * jj];  // columns x + 2 jj, x + 2 jj + 1
      // output x: taps 2 jj and 2 jj + 1 (the latter up to 10); output x + 1: taps 2 jj - 1 (from 0) and 2 jj
      m0[j] = fma((double)PX_G[2 * jj], v.x, m0[j]);
      if (2 * jj + 1 < PX_TAPS) m0[j] = fma((double)PX_G[2 * jj + 1], v.y, m0[j]);
      if (2 * jj - 1 >= 0) m1[j] = fma((double)PX_G[2 * jj - 1], v.x, m1[j]);
      m1[j] = fma((double)PX_G[2 * jj], v.y, m1[j]);
    }
  }
  const bool in_y = y0 + y < p.H, in0 = in_y && x0 + x < p.W, in1 = in_y && x0 + x + 1 < p.W;
  const double l0 = ssim_point(m0[0], m0[1], m0[3], m0[4], m0[6]), q0 = ssim_point(m0[0], m0[2], m0[3], m0[5], m0[7]);
  const double l1 = ssim_point(m1[0], m1[1], m1[3], m1[4], m1[6]), q1 = ssim_point(m1[0], m1[2], m1[3], m1[5], m1[7]);
  const double sum_l = (in0 ? l0 : 0.0) + (in1 ? l1 : 0.0), sum_q = (in0 ? q0 : 0.0) + (in1 ? q1 : 0.0);
  px_store_partial(sum_l, sum_q, red, p.ws + (size_t)blockIdx.x * 2);
}

__device__ __forceinline__ void px_sq(double& acc, float a, float b) {
  const double d = (double)a - (double)b;  // exact
  acc = fma(d, d, acc);
}

// four consecutive elements: one 16-byte load, or four dword loads of the same elements (any alignment)
template <bool V4>
__device__ __forceinline__ void px_load4(const float* src, float (&v)[4]) {
  if (V4) {
    const float4 t = *(const float4*)src;
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = src[j];
  }
}

// Both forms give every lane the same elements in the same order: the sums do not depend on the alignment of the call.
template <bool V4>
__global__ __launch_bounds__(PX_THREADS) void pixel_psnr_partial_kernel(const px_params p) {
  __shared__ double red[PX_THREADS / 64][2];
  const int b = blockIdx.x / p.nblk, k = blockIdx.x - b * p.nblk;
  const int64_t e0 = (int64_t)k * p.chunk, e1 = min(e0 + p.chunk, p.n);  // e0 is a multiple of 4
  const size_t img = (size_t)b * (size_t)p.ld;
  const float* r = p.ref + img;
  const float* l = p.left + img;
  const float* q = p.right + img;
  double sum_l = 0.0, sum_q = 0.0;
  const int64_t n4 = (e1 - e0) >> 2;  // whole groups of four inside [e0, e1)
  for (int64_t i = threadIdx.x; i < n4; i += PX_THREADS) {
    float a[4], u[4], v[4];
    px_load4<V4>(r + e0 + 4 * i, a);
    px_load4<V4>(l + e0 + 4 * i, u);
    px_load4<V4>(q + e0 + 4 * i, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      px_sq(sum_l, a[j], u[j]);
      px_sq(sum_q, a[j], v[j]);
    }
  }
  for (int64_t i = e0 + 4 * n4 + threadIdx.x; i < e1; i += PX_THREADS) {  // the last chunk's 0..3 elements
    const float a = r[i];
    px_sq(sum_l, a, l[i]);
    px_sq(sum_q, a, q[i]);
  }
  px_store_partial(sum_l, sum_q, red, p.ws + (size_t)blockIdx.x * 2);
}

// the score of one pair from the sum over C * H * W: the mean of the SSIM map, or 10 log10(1 / mse) (mse = 0: +inf)
__device__ __forceinline__ float px_score(double sum, double n, int metric) {
  const double mean = sum / n;
  return (float)(metric ? mean : 10.0 * log10(1.0 / mean));
}

__global__ __launch_bounds__(PX_THREADS) void pixel_finish_kernel(const px_params p) {
  const int b = blockIdx.x * (PX_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= p.B) return;  // whole waves
  double v[2];
  wave_fold_rows<2>(p.ws + (size_t)b * p.nblk * 2, p.nblk, v);
  if (lane != 0) return;
  const double n = (double)p.n;
  twoafc_verdict(px_score(v[0], n, p.metric), px_score(v[1], n, p.metric), b, p.sim, p.pred, p.label, p.counts);
}

}  // namespace

extern "C" int64_t mvp_pixel_score_workspace_bytes(int B, int C, int H, int W, int metric) {
  px_params p;
  if (!px_partition(B, C, H, W, metric, &p)) return 0;
  return (int64_t)B * p.nblk * 2 * (int64_t)sizeof(double);
}

extern "C" int mvp_pixel_score(const mvp_pixel_score_args* a, void* stream) {
  if (!a || !a->ref || !a->left || !a->right || !a->sim || !a->pred) return MVP_EINVAL;
  if (a->counts && !a->label) return MVP_EINVAL;
  px_params p;
  if (!px_partition(a->B, a->C, a->H, a->W, a->metric, &p) || a->ld < p.n) return MVP_EINVAL;
  if (!a->workspace || !aligned_to(a->workspace, 8) ||
      a->workspace_bytes < mvp_pixel_score_workspace_bytes(a->B, a->C, a->H, a->W, a->metric))
    return MVP_EINVAL;
  if (!aligned_to(a->counts, 8)) return MVP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  p.ref = a->ref; p.left = a->left; p.right = a->right; p.label = a->label;
  p.sim = a->sim; p.pred = a->pred; p.counts = a->counts; p.ws = (double*)a->workspace;
  p.ld = a->ld; p.B = a->B; p.C = a->C; p.H = a->H; p.W = a->W; p.metric = a->metric;
  if (a->counts && !a->accumulate && hipMemsetAsync(a->counts, 0, 4 * sizeof(int64_t), s) != hipSuccess) return MVP_ELAUNCH;
  const dim3 grid((unsigned)((int64_t)a->B * p.nblk));
  if (a->metric == 1) {
    hipLaunchKernelGGL(pixel_ssim_partial_kernel, grid, dim3(PX_THREADS), 0, s, p);
  } else {
    const bool v4 = (a->ld & 3) == 0 && aligned_to(a->ref, 16) && aligned_to(a->left, 16) && aligned_to(a->right, 16);
    if (v4) hipLaunchKernelGGL(pixel_psnr_partial_kernel<true>, grid, dim3(PX_THREADS), 0, s, p);
    else hipLaunchKernelGGL(pixel_psnr_partial_kernel<false>, grid, dim3(PX_THREADS), 0, s, p);
  }
  hipLaunchKernelGGL(pixel_finish_kernel, dim3((unsigned)((a->B - 1) / 4 + 1)), dim3(PX_THREADS), 0, s, p);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}
