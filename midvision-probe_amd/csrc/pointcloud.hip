// mvp_pointcloud_sample: dense features sampled at the projections of a point cloud (evals/utils/correspondence.py:164-176,
// sample_pointcloud_features = project with K, normalise to [-1, 1], grid_sample(bilinear, zeros, align_corners=False)), written
// channel-major [C, ld_out] — the layout mvp_knn_ratio reads, so the ScanNet correspondence path transposes nothing.
//
// Lanes run along the points: the stores of one channel row are coalesced, the 4 corner offsets / weights are computed once per
// point and reused for every channel of the block's chunk.  The grid is (point blocks) x (channel chunks of PCS_CCHUNK), so a small N
// still spreads over several workgroups.  The loads are gathers from a map that fits L2 (C = 768, 30 x 40: 3.7 MB); neighbouring
// points read neighbouring texels.  No atomics, no sync, no allocation; every output element is one thread's fixed expression.
#include <math.h>

#include "mvp_common.h"

namespace {

#define PCS_THREADS 256
#define PCS_CCHUNK 16

struct pcs_params {
  const float* feat; const float* pc; const float* K;
  float* out; uint8_t* valid;
  int C, fh, fw, N, H, W, ld_out;
};

__global__ __launch_bounds__(PCS_THREADS) void pointcloud_sample_kernel(const pcs_params p) {
  const int n = blockIdx.x * PCS_THREADS + threadIdx.x;
  if (n >= p.N) return;
  const float px = p.pc[3 * (size_t)n], py = p.pc[3 * (size_t)n + 1], pz = p.pc[3 * (size_t)n + 2];
  if (blockIdx.y == 0 && p.valid) p.valid[n] = pz > 0.f ? 1 : 0;
  // uvd = K p: every sum takes all three coordinates, so a NaN in any of them reaches both u and v
  const float* K = p.K;
  const float ux = fmaf(K[2], pz, fmaf(K[1], py, K[0] * px));
  const float uy = fmaf(K[5], pz, fmaf(K[4], py, K[3] * px));
  const float uz = fmaf(K[8], pz, fmaf(K[7], py, K[6] * px));
  const float d = fmaxf(uz, 1e-9f);  // clamp(min=1e-9): z <= 0 sends u, v to ~1e9 * x, far outside the map
  const float x = (ux / d) * (float)p.fw / (float)p.W - 0.5f;
  const float y = (uy / d) * (float)p.fh / (float)p.H - 0.5f;
  // decided on the floats: false for NaN / inf, and floor() of what passes lies in [-1, fw - 1] x [-1, fh - 1]
  const bool inside = x > -1.f && x < (float)p.fw && y > -1.f && y < (float)p.fh;
  const size_t plane = (size_t)p.fh * p.fw;
  size_t o00 = 0, o01 = 0, o10 = 0, o11 = 0;
  float w00 = 0.f, w01 = 0.f, w10 = 0.f, w11 = 0.f;
  bool k00 = false, k01 = false, k10 = false, k11 = false;
  if (inside) {
    const float xf = floorf(x), yf = floorf(y);
    const int x0 = (int)xf, y0 = (int)yf, x1 = x0 + 1, y1 = y0 + 1;
    const float tx = x - xf, ty = y - yf;
    w00 = (1.f - tx) * (1.f - ty); w01 = tx * (1.f - ty); w10 = (1.f - tx) * ty; w11 = tx * ty;
    const bool xa = x0 >= 0, xb = x1 <= p.fw - 1, ya = y0 >= 0, yb = y1 <= p.fh - 1;
    k00 = xa && ya; k01 = xb && ya; k10 = xa && yb; k11 = xb && yb;
    // a corner outside the map contributes 0 (zeros padding): its load goes to a clamped, in-range texel and is discarded
    const int xc0 = xa ? x0 : 0, xc1 = xb ? x1 : p.fw - 1, yc0 = ya ? y0 : 0, yc1 = yb ? y1 : p.fh - 1;
    o00 = (size_t)yc0 * p.fw + xc0; o01 = (size_t)yc0 * p.fw + xc1;
    o10 = (size_t)yc1 * p.fw + xc0; o11 = (size_t)yc1 * p.fw + xc1;
  }
  for (int c0 = blockIdx.y * PCS_CCHUNK; c0 < p.C; c0 += gridDim.y * PCS_CCHUNK) {
    const int c1 = min(c0 + PCS_CCHUNK, p.C);
    for (int c = c0; c < c1; ++c) {
      float v = 0.f;
      if (inside) {
        const float* f = p.feat + (size_t)c * plane;
        const float f00 = k00 ? f[o00] : 0.f, f01 = k01 ? f[o01] : 0.f, f10 = k10 ? f[o10] : 0.f, f11 = k11 ? f[o11] : 0.f;
        v = fmaf(w11, f11, fmaf(w10, f10, fmaf(w01, f01, w00 * f00)));
      }
      p.out[(size_t)c * p.ld_out + n] = v;
    }
  }
}

}  // namespace

extern "C" int mvp_pointcloud_sample(const mvp_pointcloud_sample_args* a, void* stream) {
  if (!a || !a->feat || !a->pc || !a->K || !a->out) return MVP_EINVAL;
  if (a->C <= 0 || a->fh <= 0 || a->fw <= 0 || a->N <= 0 || a->H <= 0 || a->W <= 0 || a->ld_out <= 0) return MVP_EINVAL;
  if (a->ld_out < a->N || a->N > (1 << 24)) return MVP_EINVAL;
  const pcs_params p = {a->feat, a->pc, a->K, a->out, a->valid, a->C, a->fh, a->fw, a->N, a->H, a->W, a->ld_out};
  const int chunks = (a->C + PCS_CCHUNK - 1) / PCS_CCHUNK;
  const dim3 grid((a->N + PCS_THREADS - 1) / PCS_THREADS, chunks < 65535 ? chunks : 65535);
  hipLaunchKernelGGL(pointcloud_sample_kernel, grid, dim3(PCS_THREADS), 0, (hipStream_t)stream, p);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}
