// MaskCut (normalised cuts on the patch affinity of a frozen backbone's last-layer keys; reference: evals/models/maskcut_processor.py)
// as four launches per pass, batched over images, none of which talks to the host (include/mvp_hip.h has the definitions):
//   mvp_ncut_affinity   A = F^T F of the L2-normalised, painted-out key columns on the fp32-input MFMA (v_mfma_f32_32x32x2_f32: an
//                       exact k-ordered fp32 fma chain, so A is bitwise symmetric and accurate to ~1e-7: its entries are compared
//                       with a threshold), plus the fp64 sum and sum of squares of its entries, folded in a fixed order.
//   mvp_ncut_threshold  tau = fixed point of Lloyd's 1-D 2-means from the centres mean -+ std (fp64 sums, one workgroup per image),
//                       then the bit matrix B = [A > tau] and the degrees d = cnt + eps (N - cnt) from the integer row counts.
//   mvp_ncut_fiedler    one workgroup per image with the image's whole bit matrix resident in LDS (128 KiB of the CU's 160): block
//                       subspace iteration (4 vectors) on (I + S) / 2, S = D^-1/2 W D^-1/2, with the known top pair deflated and a
//                       Rayleigh-Ritz step in fp64 every round.  W is never formed: W x = (1 - eps) (B x) + eps sum(x).
//   mvp_ncut_partition  mean, bipartition, corner rule, seed, 4-connected component of the seed, the rejection rule of pass >= 2,
//                       painting update and the hole-filled union, all in LDS, one workgroup per image.
// Every kernel takes a per-image `active` byte (NULL = all active): the workgroups of an inactive image return at once and leave its
// outputs untouched.  No floating-point atomics anywhere (csrc/mvp_reduce.h has the rule); two calls give the same bits.
#include <math.h>

#include "mvp_reduce.h"

namespace {

#define NC_MAX_N 1024
#define NC_MAX_C 4096
#define NC_THREADS 1024
#define NC_WAVES (NC_THREADS / 64)
#define NC_EPS 1e-5
#define NC_K 4  // vectors of the block iteration

typedef __attribute__((ext_vector_type(16))) float f32x16_t;

// Sum of K doubles per thread over the workgroup, the same bits in every thread: butterfly inside each wave, then the wave partials
// in wave order.  red: NC_WAVES * K doubles of LDS; synchronises before and after, so red may be reused at once.
template <int K>
__device__ __forceinline__ void block_sum_f64(double (&v)[K], double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[wave * K + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double s = 0.0;
    for (int w = 0; w < nw; ++w) s += red[w * K + k];
    v[k] = s;
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------ affinity
// inverse column norms: inv[b, n] = painted ? 0 : 1 / max(|F[:, n]|, 1e-12) (F.normalize).  64 columns x 4 channel groups per workgroup.
__global__ __launch_bounds__(256) void ncut_norm_kernel(const float* __restrict__ feats, const uint8_t* __restrict__ painted,
                                                        const uint8_t* __restrict__ active, float* __restrict__ inv, int C, int N,
                                                        int64_t ldf, int64_t img_stride) {
  __shared__ double part[4][64];
  const int b = blockIdx.y;
  if (active && !active[b]) return;
  const int col = threadIdx.x & 63, g = threadIdx.x >> 6, n = blockIdx.x * 64 + col;
  const float* f = feats + (size_t)b * img_stride;
  double s = 0.0;
  if (n < N) {
    for (int c = g; c < C; c += 4) {
      const double x = (double)f[(size_t)c * ldf + n];
      s = fma(x, x, s);
    }
  }
  part[g][col] = s;
  __syncthreads();
  if (g == 0 && n < N) {
    const double t = (part[0][col] + part[1][col]) + (part[2][col] + part[3][col]);
    const bool p = painted && painted[(size_t)b * N + n];
    inv[(size_t)b * N + n] = p ? 0.f : (float)(1.0 / fmax(sqrt(t), 1e-12));
  }
}

// One 64 x 64 tile of A per workgroup, one 32 x 32 quadrant per wave.  Operand lane map of v_mfma_f32_32x32x2_f32: lane l holds
// A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]; C/D: col = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).
// Both operands are columns of F scaled by their inverse norm, read straight from global memory (runs of 32 consecutive floats);
// columns >= N and channels >= C are read from a clamped, legal position and multiplied by zero.
__global__ __launch_bounds__(256) void ncut_gram_kernel(const float* __restrict__ feats, const float* __restrict__ inv,
                                                        const uint8_t* __restrict__ active, float* __restrict__ A,
                                                        double* __restrict__ part, int C, int N, int64_t ldf, int64_t img_stride, int T) {
  __shared__ double red[4][2];
  const int b = blockIdx.y;
  if (active && !active[b]) return;
  const int ti = blockIdx.x / T, tj = blockIdx.x - ti * T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i0 = ti * 64 + (wave >> 1) * 32, j0 = tj * 64 + (wave & 1) * 32;
  const int r = lane & 31, kh = lane >> 5;
  const int ia = i0 + r, jb = j0 + r;
  const int iac = min(ia, N - 1), jbc = min(jb, N - 1);
  const float* f = feats + (size_t)b * img_stride;
  const float sa = ia < N ? inv[(size_t)b * N + iac] : 0.f, sb = jb < N ? inv[(size_t)b * N + jbc] : 0.f;
  f32x16_t acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  for (int c = 0; c < C; c += 2) {
    const int ck = c + kh;
    const int cc = min(ck, C - 1);
    const float m = ck < C ? 1.f : 0.f;
    const float a = f[(size_t)cc * ldf + iac] * (sa * m), bb = f[(size_t)cc * ldf + jbc] * sb;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb, acc, 0, 0, 0);
  }
  float* Ab = A + (size_t)b * N * N;
  double s1 = 0.0, s2 = 0.0;
  const int col = j0 + r;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int row = i0 + (e & 3) + 8 * (e >> 2) + 4 * kh;
    if (row < N && col < N) {
      const float v = acc[e];
      Ab[(size_t)row * N + col] = v;
      s1 += (double)v;
      s2 = fma((double)v, (double)v, s2);
    }
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if (lane == 0) { red[wave][0] = s1; red[wave][1] = s2; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int k = threadIdx.x;
    part[((size_t)b * T * T + blockIdx.x) * 2 + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  }
}

// sums[b] = {sum, sum of squares} of A[b]: the tile partials in tile order, one wave per image
__global__ __launch_bounds__(64) void ncut_sums_kernel(const double* __restrict__ part, const uint8_t* __restrict__ active,
                                                       double* __restrict__ sums, int ntiles) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (active && !active[b]) return;
  double s1 = 0.0, s2 = 0.0;
  for (int t = lane; t < ntiles; t += 64) {
    s1 += part[((size_t)b * ntiles + t) * 2];
    s2 += part[((size_t)b * ntiles + t) * 2 + 1];
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if (lane == 0) { sums[2 * b] = s1; sums[2 * b + 1] = s2; }
}

// ------------------------------------------------------------------------------------------------ threshold
// Lloyd's iteration on the N^2 entries of A[b] with two centres.  Round: t = (c0 + c1) / 2, upper cluster = {a > t}, new centres =
// the cluster means (fp64).  The clusters are nested in t, so an unchanged upper count is an unchanged assignment: the fixed point.
// An empty cluster ends the iteration with the centres of the round before.  Then bits and degrees from tau = (c0 + c1) / 2.
__global__ __launch_bounds__(NC_THREADS) void ncut_threshold_kernel(const float* __restrict__ A, const double* __restrict__ sums,
                                                                    const uint8_t* __restrict__ active, double* __restrict__ tau_out,
                                                                    uint32_t* __restrict__ bits, double* __restrict__ deg,
                                                                    int32_t* __restrict__ rounds_out, int N, int NW, int max_rounds) {
  __shared__ double red[NC_WAVES * 3];
  const int b = blockIdx.x;
  if (active && !active[b]) return;
  const float* Ab = A + (size_t)b * N * N;
  const int64_t M = (int64_t)N * N;
  const double mean = sums[2 * b] / (double)M;
  const double var = fmax(sums[2 * b + 1] / (double)M - mean * mean, 0.0);
  const double sd = sqrt(var);
  double c0 = mean - sd, c1 = mean + sd;
  int64_t prev_cnt = -1;
  int rounds = 0;
  for (int r = 0; r < max_rounds; ++r) {
    const double t = 0.5 * (c0 + c1);
    double v[3] = {0.0, 0.0, 0.0};  // upper count, upper sum, lower sum
    for (int64_t i = threadIdx.x; i < M; i += NC_THREADS) {
      const double a = (double)Ab[i];
      const bool up = a > t;
      v[0] += up ? 1.0 : 0.0;
      v[1] += up ? a : 0.0;
      v[2] += up ? 0.0 : a;
    }
    block_sum_f64<3>(v, red);
    const int64_t cnt = (int64_t)v[0];
    rounds = r + 1;
    if (cnt == 0 || cnt == M) break;
    c1 = v[1] / (double)cnt;
    c0 = v[2] / (double)(M - cnt);
    if (cnt == prev_cnt) break;
    prev_cnt = cnt;
  }
  const double tau = 0.5 * (c0 + c1);
  if (threadIdx.x == 0) {
    tau_out[b] = tau;
    if (rounds_out) rounds_out[b] = rounds;
  }
  // bits and degrees: one wave per row, 64 columns per step; bits beyond column N - 1 of the last word are zero
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t* bb = bits + (size_t)b * N * NW;
  for (int row = wave; row < N; row += NC_WAVES) {
    int cnt = 0;
    for (int j0 = 0; j0 < NW * 32; j0 += 64) {
      const int j = j0 + lane;
      const bool up = j < N && (double)Ab[(size_t)row * N + j] > tau;
      const unsigned long long m = __ballot(up);
      cnt += __popcll(m);
      if (lane == 0) bb[(size_t)row * NW + (j0 >> 5)] = (uint32_t)m;
      if (lane == 1 && (j0 >> 5) + 1 < NW) bb[(size_t)row * NW + (j0 >> 5) + 1] = (uint32_t)(m >> 32);
    }
    // (a product and a sum, each rounded: no fma, so that the value is the one numpy's cnt + eps * (N - cnt) gives)
    if (lane == 0) deg[(size_t)b * N + row] = __dadd_rn((double)cnt, __dmul_rn(NC_EPS, (double)(N - cnt)));
  }
}

// ------------------------------------------------------------------------------------------------ Fiedler vector
// eigen-decomposition of a symmetric K x K matrix by cyclic Jacobi sweeps (fp64; every thread runs it on the same numbers and gets the
// same bits).  On return the columns of V are the eigenvectors and w the eigenvalues, sorted descending.
__device__ __forceinline__ void jacobi_eig(double (&Hm)[NC_K][NC_K], double (&V)[NC_K][NC_K], double (&w)[NC_K]) {
#pragma unroll
  for (int a = 0; a < NC_K; ++a)
#pragma unroll
    for (int c = 0; c < NC_K; ++c) V[a][c] = a == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 8; ++sweep) {
#pragma unroll
    for (int p = 0; p < NC_K - 1; ++p) {
#pragma unroll
      for (int q = p + 1; q < NC_K; ++q) {
        const double apq = Hm[p][q];
        if (fabs(apq) > 1e-300) {
          const double th = (Hm[q][q] - Hm[p][p]) / (2.0 * apq);
          const double tt = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
          const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
#pragma unroll
          for (int k = 0; k < NC_K; ++k) {  // columns p, q
            const double hkp = Hm[k][p], hkq = Hm[k][q];
            Hm[k][p] = cs * hkp - sn * hkq;
            Hm[k][q] = sn * hkp + cs * hkq;
          }
#pragma unroll
          for (int k = 0; k < NC_K; ++k) {  // rows p, q
            const double hpk = Hm[p][k], hqk = Hm[q][k];
            Hm[p][k] = cs * hpk - sn * hqk;
            Hm[q][k] = sn * hpk + cs * hqk;
          }
#pragma unroll
          for (int k = 0; k < NC_K; ++k) {
            const double vkp = V[k][p], vkq = V[k][q];
            V[k][p] = cs * vkp - sn * vkq;
            V[k][q] = sn * vkp + cs * vkq;
          }
        }
      }
    }
  }
#pragma unroll
  for (int a = 0; a < NC_K; ++a) w[a] = Hm[a][a];
#pragma unroll
  for (int a = 0; a < NC_K - 1; ++a) {  // selection sort, descending
#pragma unroll
    for (int c = a + 1; c < NC_K; ++c) {
      if (w[c] > w[a]) {
        const double t = w[a]; w[a] = w[c]; w[c] = t;
#pragma unroll
        for (int k = 0; k < NC_K; ++k) { const double u = V[k][a]; V[k][a] = V[k][c]; V[k][c] = u; }
      }
    }
  }
}

struct fiedler_params {
  const uint32_t* bits; const double* deg; const uint8_t* active;
  float* v; double* lambda; double* residual; int32_t* iters; uint8_t* converged;
  int N, NW, max_iters;
  float r_tol, mix_tol;
};

__device__ __forceinline__ float nc_hash_unit(uint32_t x) {  // a fixed pseudo-random value in [-1, 1)
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return (float)(int32_t)x * (1.0f / 2147483648.0f);
}

// S y in fp64 for the row of this thread: x = D^-1/2 y goes to LDS (xd, NC_MAX_N doubles), W x = (1 - eps) (B x) + eps sum(x).
// Synchronises before the reads and after them, so xd may be rewritten at once.
__device__ __forceinline__ double nc_apply_S64(const uint32_t* bitsT, double* xd, double* red, double s, double yv, int i, int NW, bool row) {
  const double x = s * yv;
  xd[i] = x;
  double sx[1] = {x};
  block_sum_f64<1>(sx, red);  // (orders the xd writes before the reads below)
  double acc = 0.0;
  for (int w = 0; w < NW; ++w) {
    const uint32_t word = bitsT[w * NC_MAX_N + i];
    for (int bit = 0; bit < 32; ++bit) acc += (word >> bit) & 1u ? xd[w * 32 + bit] : 0.0;
  }
  __syncthreads();
  return row ? s * ((1.0 - NC_EPS) * acc + NC_EPS * sx[0]) : 0.0;
}

// Thread i owns row i of the image (N <= 1024 = the workgroup).  LDS: the bit matrix word-major (word w of row i at w * 1024 + i: the
// lanes of a wave read consecutive dwords), the current block of scaled vectors x = D^-1/2 y as one float4 per column (every lane reads
// the same address: a broadcast), and the reduction scratch.  The vectors themselves live in registers, one row per thread.
__global__ __launch_bounds__(NC_THREADS) void ncut_fiedler_kernel(const fiedler_params p) {
  __shared__ uint32_t bitsT[32 * NC_MAX_N];        // 128 KiB
  __shared__ float4 xs[NC_MAX_N];                  // 16 KiB (the final pass reuses it as NC_MAX_N doubles)
  __shared__ double red[NC_WAVES * 30];
  const int b = blockIdx.x;
  if (p.active && !p.active[b]) return;
  const int N = p.N, NW = p.NW, i = threadIdx.x;
  const bool row = i < N;
  {
    const uint32_t* g = p.bits + ((size_t)b * N + (row ? i : 0)) * NW;
    for (int w = 0; w < NW; ++w) bitsT[w * NC_MAX_N + i] = row ? g[w] : 0u;
  }
  const double d = row ? p.deg[(size_t)b * N + i] : 1.0;
  const double sq = sqrt(d);
  const double s = row ? 1.0 / sq : 0.0;  // D^-1/2
  double u;                                // the known top eigenvector D^1/2 1 / |.|
  {
    double t[1] = {row ? d : 0.0};
    block_sum_f64<1>(t, red);  // (also orders the bitsT writes before the first read)
    u = row ? sq / sqrt(t[0]) : 0.0;
  }
  float y[NC_K], z[NC_K];
#pragma unroll
  for (int k = 0; k < NC_K; ++k) { y[k] = 0.f; z[k] = row ? nc_hash_unit((uint32_t)(i * NC_K + k) + 0x9e3779b9u) : 0.f; }
  double theta0 = 0.0, theta1 = 0.0, res = INFINITY;
  double sumx[NC_K] = {0.0, 0.0, 0.0, 0.0};
  int it = 0;
  bool done = false;
  const float r_loop = 0.5f * p.r_tol;  // the loop's fp32 estimate stops at half the tolerance; the fp64 residual below decides
  for (;;) {
    // z = candidate block (it == 0: the start vectors; later (I + S) / 2 times the orthonormal block y).  Deflate the top pair.
    {
      double c[NC_K];
#pragma unroll
      for (int k = 0; k < NC_K; ++k) c[k] = u * (double)z[k];
      block_sum_f64<NC_K>(c, red);
#pragma unroll
      for (int k = 0; k < NC_K; ++k) z[k] = (float)((double)z[k] - u * c[k]);
    }
    // H = y^T z (symmetrised), G = z^T z, t = sum of D^-1/2 z
    double r30[30];
    {
      int o = 0;
#pragma unroll
      for (int a = 0; a < NC_K; ++a)
#pragma unroll
        for (int c = 0; c < NC_K; ++c) r30[o++] = (double)y[a] * (double)z[c];
#pragma unroll
      for (int a = 0; a < NC_K; ++a)
#pragma unroll
        for (int c = a; c < NC_K; ++c) r30[o++] = (double)z[a] * (double)z[c];
#pragma unroll
      for (int a = 0; a < NC_K; ++a) r30[o++] = s * (double)z[a];
    }
    block_sum_f64<30>(r30, red);
    double V[NC_K][NC_K], G[NC_K][NC_K], th[NC_K], tz[NC_K];
    {
      int o = 16;
#pragma unroll
      for (int a = 0; a < NC_K; ++a)
#pragma unroll
        for (int c = a; c < NC_K; ++c) { G[a][c] = r30[o]; G[c][a] = r30[o]; ++o; }
#pragma unroll
      for (int a = 0; a < NC_K; ++a) tz[a] = r30[o++];
    }
    if (it > 0) {
      double Hm[NC_K][NC_K];
#pragma unroll
      for (int a = 0; a < NC_K; ++a)
#pragma unroll
        for (int c = 0; c < NC_K; ++c) Hm[a][c] = 0.5 * (r30[a * NC_K + c] + r30[c * NC_K + a]);
      jacobi_eig(Hm, V, th);
      // rotate y, z, G and t into the Ritz basis
      double yr[NC_K], zr[NC_K];
#pragma unroll
      for (int c = 0; c < NC_K; ++c) {
        double ya = 0.0, za = 0.0;
#pragma unroll
        for (int a = 0; a < NC_K; ++a) { ya = fma((double)y[a], V[a][c], ya); za = fma((double)z[a], V[a][c], za); }
        yr[c] = ya; zr[c] = za;
      }
      double GV[NC_K][NC_K], G2[NC_K][NC_K], t2[NC_K];
#pragma unroll
      for (int a = 0; a < NC_K; ++a)
#pragma unroll
        for (int c = 0; c < NC_K; ++c) {
          double acc = 0.0;
#pragma unroll
          for (int k = 0; k < NC_K; ++k) acc = fma(G[a][k], V[k][c], acc);
          GV[a][c] = acc;
        }
#pragma unroll
      for (int a = 0; a < NC_K; ++a)
#pragma unroll
        for (int c = 0; c < NC_K; ++c) {
          double acc = 0.0;
#pragma unroll
          for (int k = 0; k < NC_K; ++k) acc = fma(V[k][a], GV[k][c], acc);
          G2[a][c] = acc;
        }
#pragma unroll
      for (int c = 0; c < NC_K; ++c) {
        double acc = 0.0;
#pragma unroll
        for (int a = 0; a < NC_K; ++a) acc = fma(tz[a], V[a][c], acc);
        t2[c] = acc;
      }
#pragma unroll
      for (int a = 0; a < NC_K; ++a) {
        y[a] = (float)yr[a]; z[a] = (float)zr[a]; tz[a] = t2[a];
#pragma unroll
        for (int c = 0; c < NC_K; ++c) G[a][c] = G2[a][c];
      }
      // residual of the leading Ritz pair of (I + S) / 2; in terms of S it is twice that, and so is the gap
      double rr[1];
      {
        const double e = zr[0] - th[0] * yr[0];
        rr[0] = e * e;
      }
      block_sum_f64<1>(rr, red);
      res = 2.0 * sqrt(rr[0]);
      theta0 = 2.0 * th[0] - 1.0;
      theta1 = 2.0 * th[1] - 1.0;
      if ((res <= (double)r_loop && res <= 0.5 * (double)p.mix_tol * (theta0 - theta1)) || it >= p.max_iters) done = true;
    }
    if (done) break;
    // orthonormalise: z = Q R by Cholesky of G (the Ritz images are close to orthogonal), y = z R^-1; sum(D^-1/2 y) follows linearly
    {
      double R[NC_K][NC_K];
#pragma unroll
      for (int a = 0; a < NC_K; ++a)
#pragma unroll
        for (int c = 0; c < NC_K; ++c) R[a][c] = 0.0;
#pragma unroll
      for (int c = 0; c < NC_K; ++c) {
#pragma unroll
        for (int a = 0; a <= c; ++a) {
          double acc = G[a][c];
#pragma unroll
          for (int k = 0; k < a; ++k) acc -= R[k][a] * R[k][c];
          if (a == c) R[a][a] = sqrt(fmax(acc, 1e-300));
          else R[a][c] = acc / R[a][a];
        }
      }
      double yn[NC_K], sn[NC_K];
#pragma unroll
      for (int c = 0; c < NC_K; ++c) {  // forward substitution on rows: yn R = z
        double acc = (double)z[c], acs = tz[c];
#pragma unroll
        for (int k = 0; k < c; ++k) { acc -= yn[k] * R[k][c]; acs -= sn[k] * R[k][c]; }
        yn[c] = acc / R[c][c];
        sn[c] = acs / R[c][c];
      }
#pragma unroll
      for (int c = 0; c < NC_K; ++c) { y[c] = (float)yn[c]; sumx[c] = sn[c]; }
    }
    // z = (y + S y) / 2, S y = D^-1/2 ((1 - eps) B x + eps sum(x)), x = D^-1/2 y
    xs[i] = make_float4((float)(s * (double)y[0]), (float)(s * (double)y[1]), (float)(s * (double)y[2]), (float)(s * (double)y[3]));
    __syncthreads();
    {
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      for (int w = 0; w < NW; ++w) {
        const uint32_t word = bitsT[w * NC_MAX_N + i];
#pragma unroll 8
        for (int bit = 0; bit < 32; ++bit) {
          const float4 x = xs[w * 32 + bit];
          const float m = (word >> bit) & 1u ? 1.f : 0.f;
          a0 = fmaf(m, x.x, a0); a1 = fmaf(m, x.y, a1); a2 = fmaf(m, x.z, a2); a3 = fmaf(m, x.w, a3);
        }
      }
      const float acc[NC_K] = {a0, a1, a2, a3};
#pragma unroll
      for (int k = 0; k < NC_K; ++k) {
        const double wy = (1.0 - NC_EPS) * (double)acc[k] + NC_EPS * sumx[k];
        z[k] = (float)(0.5 * ((double)y[k] + s * wy));
      }
    }
    __syncthreads();  // xs is rewritten next round
    ++it;
  }
  // Polish: one step of S in fp64 on the leading Ritz vector.  The fp32 iteration leaves an error of ~r / gap in y; v = D^-1/2 y
  // amplifies it by d^-1/2 on the cells of tiny degree (painted cells: d = eps N), whose side of the mean is decided by a margin of
  // ~lambda |mean|.  Their modes have eigenvalues near 0, so one application of S removes that error by a factor ~1 / (N theta).
  double* xd = (double*)xs;
  double yd = row ? (double)y[0] : 0.0;
  {
    const double Sy = nc_apply_S64(bitsT, xd, red, s, yd, i, NW, row);
    double c[2] = {u * Sy, 0.0};
    block_sum_f64<2>(c, red);
    yd = Sy - u * c[0];
  }
  // The output vector v = D^-1/2 y, sign: the entry of largest |v| is positive (lowest index on ties); |D^1/2 v| = 1.
  {
    double t[1] = {yd * yd};
    block_sum_f64<1>(t, red);
    yd = t[0] > 0.0 ? yd / sqrt(t[0]) : 0.0;
  }
  float vout = (float)(s * yd);
  {
    __shared__ float bestv[NC_WAVES];
    __shared__ int besti[NC_WAVES];
    __shared__ float lead;
    float av = row ? fabsf(vout) : -1.f;
    int ai = i;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(av, o, 64);
      const int oi = __shfl_xor(ai, o, 64);
      if (ov > av || (ov == av && oi < ai)) { av = ov; ai = oi; }
    }
    if ((i & 63) == 0) { bestv[i >> 6] = av; besti[i >> 6] = ai; }
    __syncthreads();
    for (int w = 0; w < NC_WAVES; ++w) {
      const float ov = bestv[w];
      const int oi = besti[w];
      if (w == 0 || ov > av || (ov == av && oi < ai)) { av = ov; ai = oi; }
    }
    if (i == ai) lead = vout;
    __syncthreads();
    if (lead < 0.f) vout = -vout;
  }
  if (row) p.v[(size_t)b * N + i] = vout;
  // lambda and the residual of the vector that was WRITTEN (fp32 v), everything in fp64: y = D^1/2 v / |.|, theta = y^T S y
  yd = row ? sq * (double)vout : 0.0;
  {
    double t[1] = {yd * yd};
    block_sum_f64<1>(t, red);
    yd = t[0] > 0.0 ? yd / sqrt(t[0]) : 0.0;
  }
  const double Sy = nc_apply_S64(bitsT, xd, red, s, yd, i, NW, row);
  double th1[1] = {yd * Sy};
  block_sum_f64<1>(th1, red);
  const double e = Sy - th1[0] * yd;
  double r2[1] = {e * e};
  block_sum_f64<1>(r2, red);
  const double rfin = sqrt(r2[0]);
  if (i == 0) {
    p.lambda[b] = 1.0 - th1[0];
    p.residual[b] = rfin;
    p.iters[b] = it;
    p.converged[b] = (rfin <= (double)p.r_tol && rfin <= (double)p.mix_tol * (theta0 - theta1) && res <= (double)r_loop) ? 1 : 0;
  }
}

// ------------------------------------------------------------------------------------------------ partition
struct partition_params {
  const float* v; const uint8_t* prev_mask; const uint8_t* active;
  uint8_t* pass_mask; uint8_t* painted; uint8_t* union_mask; int32_t* seed;
  int h, w, use_prev;
};

// grows `reach` (LDS, one byte per cell) inside `open` by 4-neighbour steps until nothing changes
__device__ __forceinline__ void nc_flood(uint8_t* reach, bool open, int i, int N, int h, int w) {
  const int yy = i / w, xx = i - yy * w;
  const bool in = i < N;
  for (int round = 0; round <= N; ++round) {
    int grew = 0;
    if (in && open && !reach[i]) {
      const bool nb = (yy > 0 && reach[i - w]) || (yy + 1 < h && reach[i + w]) || (xx > 0 && reach[i - 1]) || (xx + 1 < w && reach[i + 1]);
      if (nb) grew = 1;
    }
    __syncthreads();  // every read of this round before any write
    if (grew) reach[i] = 1;
    if (!__syncthreads_or(grew)) break;
  }
}

__global__ __launch_bounds__(NC_THREADS) void ncut_partition_kernel(const partition_params p) {
  __shared__ double red[NC_WAVES * 2];
  __shared__ uint8_t reach[NC_MAX_N];
  __shared__ float bv[NC_WAVES];
  __shared__ int bi[NC_WAVES];
  __shared__ int corners[4];
  const int b = blockIdx.x;
  if (p.active && !p.active[b]) return;
  const int h = p.h, w = p.w, N = h * w, i = threadIdx.x;
  const bool in = i < N;
  const float vi = in ? p.v[(size_t)b * N + i] : 0.f;
  double t[1] = {in ? (double)vi : 0.0};
  block_sum_f64<1>(t, red);
  const double mean = t[0] / (double)N;
  bool bip = in && (double)vi > mean;
  if (in) {
    if (i == 0) corners[0] = bip;
    if (i == w - 1) corners[1] = bip;
    if (i == (h - 1) * w) corners[2] = bip;
    if (i == N - 1) corners[3] = bip;
  }
  // three arg-extrema with the lowest index on ties: max |v| (the reference's first seed), max v, min v
  int arg[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float key = k == 0 ? fabsf(vi) : (k == 1 ? vi : -vi);
    if (!in) key = -INFINITY;
    int ai = i;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(key, o, 64);
      const int oi = __shfl_xor(ai, o, 64);
      if (ov > key || (ov == key && oi < ai)) { key = ov; ai = oi; }
    }
    if ((i & 63) == 0) { bv[i >> 6] = key; bi[i >> 6] = ai; }
    __syncthreads();
    for (int wv = 0; wv < NC_WAVES; ++wv) {
      const float ov = bv[wv];
      const int oi = bi[wv];
      if (wv == 0 || ov > key || (ov == key && oi < ai)) { key = ov; ai = oi; }
    }
    arg[k] = ai;
    __syncthreads();
  }
  const int nc = corners[0] + corners[1] + corners[2] + corners[3];
  // is the first seed on the foreground side?  every thread needs that cell's bit
  reach[i] = bip ? 1 : 0;
  __syncthreads();
  const bool seed_fg = reach[arg[0]] != 0;
  __syncthreads();
  const bool reverse = nc >= 3 || !seed_fg;
  if (reverse) bip = in && !bip;
  const int seed = reverse ? arg[2] : arg[1];
  // the 4-connected component of the seed (ndimage.label's default structure).  The seed is always a foreground cell: without the
  // reversal it is argmax v with v[argmax |v|] > mean, with it argmin v <= mean on the complemented side.
  reach[i] = (i == seed) ? 1 : 0;
  __syncthreads();
  nc_flood(reach, bip, i, N, h, w);
  bool mask = in && reach[i] != 0;
  const bool prev = in && p.use_prev && p.prev_mask && p.prev_mask[(size_t)b * N + i] != 0;
  if (p.use_prev) {
    double c[2] = {(mask && prev) ? 1.0 : 0.0, (mask || prev) ? 1.0 : 0.0};
    double a[1] = {mask ? 1.0 : 0.0};
    block_sum_f64<2>(c, red);
    block_sum_f64<1>(a, red);
    const bool iou_rej = 2.0 * c[0] > c[1];                       // IoU > 0.5 on integer counts (0 / 0 is not a rejection)
    const bool area_rej = a[0] / (double)h / (double)w <= 0.01;  // as the reference divides
    if (iou_rej || area_rej) mask = false;
  }
  __syncthreads();
  bool painted = in && (p.painted[(size_t)b * N + i] != 0 || mask);
  if (in) {
    p.pass_mask[(size_t)b * N + i] = mask ? 1 : 0;
    p.painted[(size_t)b * N + i] = painted ? 1 : 0;
  }
  // union = binary_fill_holes(painted): the background reachable from the border stays background
  const int yy = i / w, xx = i - yy * w;
  const bool border = in && (yy == 0 || yy == h - 1 || xx == 0 || xx == w - 1);
  reach[i] = (border && !painted) ? 1 : 0;
  __syncthreads();
  nc_flood(reach, in && !painted, i, N, h, w);
  if (in) p.union_mask[(size_t)b * N + i] = reach[i] ? 0 : 1;
  if (i == 0) p.seed[b] = seed;
}

inline bool nc_sizes_ok(int Bimg, int N) { return Bimg > 0 && Bimg <= 65535 && N > 0 && N <= NC_MAX_N; }
inline int nc_tiles(int N) { return (N + 63) / 64; }

}  // namespace

extern "C" int64_t mvp_ncut_workspace_bytes(int Bimg, int N) {
  if (!nc_sizes_ok(Bimg, N)) return 0;
  const int T = nc_tiles(N);
  // inverse norms (rounded up to 8 bytes per image row) + the tile partials
  const int64_t inv = ((int64_t)Bimg * N * 4 + 7) / 8 * 8;
  return inv + (int64_t)Bimg * T * T * 2 * 8;
}

extern "C" int mvp_ncut_affinity(const mvp_ncut_affinity_args* a, void* stream) {
  if (!a || !a->feats || !a->A || !a->sums || !a->workspace) return MVP_EINVAL;
  if (!nc_sizes_ok(a->Bimg, a->N) || a->C <= 0 || a->C > NC_MAX_C || a->ldf < a->N) return MVP_EINVAL;
  if (((uintptr_t)a->feats & 3) || ((uintptr_t)a->A & 3) || ((uintptr_t)a->sums & 7) || ((uintptr_t)a->workspace & 7)) return MVP_EINVAL;
  if (a->workspace_bytes < mvp_ncut_workspace_bytes(a->Bimg, a->N)) return MVP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int T = nc_tiles(a->N);
  float* inv = (float*)a->workspace;
  double* part = (double*)((char*)a->workspace + ((int64_t)a->Bimg * a->N * 4 + 7) / 8 * 8);
  const int64_t img_stride = (int64_t)a->C * a->ldf;
  hipLaunchKernelGGL(ncut_norm_kernel, dim3((unsigned)T, (unsigned)a->Bimg), dim3(256), 0, s, a->feats, a->painted, a->active, inv, a->C, a->N,
                     a->ldf, img_stride);
  hipLaunchKernelGGL(ncut_gram_kernel, dim3((unsigned)(T * T), (unsigned)a->Bimg), dim3(256), 0, s, a->feats, (const float*)inv, a->active, a->A,
                     part, a->C, a->N, a->ldf, img_stride, T);
  hipLaunchKernelGGL(ncut_sums_kernel, dim3((unsigned)a->Bimg), dim3(64), 0, s, (const double*)part, a->active, a->sums, T * T);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}

extern "C" int mvp_ncut_threshold(const mvp_ncut_threshold_args* a, void* stream) {
  if (!a || !a->A || !a->sums || !a->tau || !a->bits || !a->deg) return MVP_EINVAL;
  if (!nc_sizes_ok(a->Bimg, a->N) || a->max_rounds <= 0) return MVP_EINVAL;
  if (((uintptr_t)a->A & 3) || ((uintptr_t)a->sums & 7) || ((uintptr_t)a->tau & 7) || ((uintptr_t)a->bits & 3) || ((uintptr_t)a->deg & 7) ||
      ((uintptr_t)a->rounds & 3))
    return MVP_EINVAL;
  hipLaunchKernelGGL(ncut_threshold_kernel, dim3((unsigned)a->Bimg), dim3(NC_THREADS), 0, (hipStream_t)stream, a->A, a->sums, a->active, a->tau,
                     a->bits, a->deg, a->rounds, a->N, (a->N + 31) / 32, a->max_rounds);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}

extern "C" int mvp_ncut_fiedler(const mvp_ncut_fiedler_args* a, void* stream) {
  if (!a || !a->bits || !a->deg || !a->v || !a->lambda || !a->residual || !a->iters || !a->converged) return MVP_EINVAL;
  if (!nc_sizes_ok(a->Bimg, a->N) || a->max_iters <= 0 || !(a->r_tol > 0.f) || !(a->mix_tol > 0.f)) return MVP_EINVAL;
  if (((uintptr_t)a->bits & 3) || ((uintptr_t)a->deg & 7) || ((uintptr_t)a->v & 3) || ((uintptr_t)a->lambda & 7) || ((uintptr_t)a->residual & 7) ||
      ((uintptr_t)a->iters & 3))
    return MVP_EINVAL;
  fiedler_params p;
  p.bits = a->bits; p.deg = a->deg; p.active = a->active; p.v = a->v; p.lambda = a->lambda; p.residual = a->residual;
  p.iters = a->iters; p.converged = a->converged; p.N = a->N; p.NW = (a->N + 31) / 32; p.max_iters = a->max_iters;
  p.r_tol = a->r_tol; p.mix_tol = a->mix_tol;
  hipLaunchKernelGGL(ncut_fiedler_kernel, dim3((unsigned)a->Bimg), dim3(NC_THREADS), 0, (hipStream_t)stream, p);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}

extern "C" int mvp_ncut_partition(const mvp_ncut_partition_args* a, void* stream) {
  if (!a || !a->v || !a->pass_mask || !a->painted || !a->union_mask || !a->seed) return MVP_EINVAL;
  if (a->h <= 0 || a->w <= 0 || (int64_t)a->h * a->w > NC_MAX_N || !nc_sizes_ok(a->Bimg, a->h * a->w)) return MVP_EINVAL;
  if (a->use_prev && !a->prev_mask) return MVP_EINVAL;
  if (((uintptr_t)a->v & 3) || ((uintptr_t)a->seed & 3)) return MVP_EINVAL;
  partition_params p;
  p.v = a->v; p.prev_mask = a->prev_mask; p.active = a->active; p.pass_mask = a->pass_mask; p.painted = a->painted;
  p.union_mask = a->union_mask; p.seed = a->seed; p.h = a->h; p.w = a->w; p.use_prev = a->use_prev;
  hipLaunchKernelGGL(ncut_partition_kernel, dim3((unsigned)a->Bimg), dim3(NC_THREADS), 0, (hipStream_t)stream, p);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}
