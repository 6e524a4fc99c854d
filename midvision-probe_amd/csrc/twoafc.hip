// mvp_twoafc_score: the scoring of a batch of 2AFC triplets (reference: evaluate_model_percepture.py:104-120 — three
// adaptive_avg_pool2d for CNN maps, two F.cosine_similarity, one torch.where) in two launches, plus the running confusion counts.
//     f_x[c] = mean over HW of x[b, c, :],   sim(x) = <f_ref, f_x> / (max(|f_ref|, 1e-8) * max(|f_x|, 1e-8)),
//     pred[b] = sim(left) > sim(right) ? 0 : 1          (include/mvp_hip.h has the full definition)
//
// Pass 1, grid = (triplet, channel chunk): a group of G lanes walks one channel row of the three images together and sums it in fp64;
// a wave holds 64 / G rows at once.  G is a power of two chosen from HW: about 16 elements per lane, but runs of at least 64
// contiguous bytes per group and load (G = 16 at HW = 9 ... 256, 32 up to 512, the whole wave beyond, one lane at HW = 1, where the
// lanes run along C).  Rows are read with 16-byte loads when every row starts 16-byte aligned (HW % 4 == 0, ld % 4 == 0, aligned bases; a
// lane then takes 4 elements at once and G is a quarter), with dword loads otherwise (HW = 225: rows start at any dword).  Full passes
// of 4 (2) loads per lane and image carry no bounds test; the last, partial pass loads from a clamped in-row position and selects 0,
// and adding +0.0 changes no value.  A butterfly inside the group (ds_bpermute with the partner addresses computed once; all groups of
// the wave at once) gives the three pooled SUMS S_r, S_l, S_q of the row, whose five products the group's first lane adds to its
// partials <r,l>, <r,r'>, |r|^2, |l|^2, |r'|^2.  The division by HW is left to pass 2 (the cosine is a ratio: only the two clamps see
// the scale).  The workgroup's five sums go to the workspace, one row per (triplet, chunk).
// Pass 2, one wave per triplet: folds the chunk rows in a fixed order (lane j takes rows j, j + 64, ...; then the butterfly), forms both
// similarities with ONE inlined sequence (bitwise-equal left / right give bitwise-equal results), rounds each once to fp32 and counts.
// No floating-point atomics (csrc/mvp_reduce.h has the order of every sum); the counts are integers, whose 64-bit atomics are exact
// in any order.  Two calls give the same bits.
// Nothing between C * HW and ld is read.
#include <math.h>

#include "mvp_reduce.h"

namespace {

#define TA_THREADS 256
#define TA_CHUNK_ELEMS 4096  // elements of ONE image a chunk holds at least (x 3 images x 4 bytes = 48 KB per workgroup)
#define TA_MAX_CHUNKS 256    // chunk rows per triplet at most (pass 2 reads them all)

struct ta_params {
  const float* ref; const float* left; const float* right; const float* label;
  float* sim; int32_t* pred; int64_t* counts; double* ws;
  int64_t ld;
  int B, C, HW;
  int cc, nchunks;  // channels per chunk, chunks per triplet
  int gshift;       // log2 of the lanes per channel row
};

// Channels per chunk and chunks per triplet.  rows_per_pass = channel rows a workgroup holds at once: the chunk is a multiple of it
// (or all of C), so that no pass runs part empty.  With rows_per_pass = 1 (the workspace query, which does not know the alignment and
// hence not G) the chunks are the most any launch uses: rounding the chunk up only lowers their number.
inline void ta_partition(int C, int HW, int rows_per_pass, int& cc, int& nchunks) {
  const int64_t per_min = ((int64_t)TA_CHUNK_ELEMS + HW - 1) / HW;
  int64_t n = ((int64_t)C + per_min - 1) / per_min;
  n = n < 1 ? 1 : (n > TA_MAX_CHUNKS ? TA_MAX_CHUNKS : n);
  int64_t c = ((int64_t)C + n - 1) / n;
  c = (c + rows_per_pass - 1) / rows_per_pass * rows_per_pass;
  cc = (int)(c > C ? C : c);
  nchunks = (int)(((int64_t)C + cc - 1) / cc);
}

inline bool ta_sizes_ok(int B, int C, int HW) {
  if (B <= 0 || C <= 0 || HW <= 0) return false;
  if ((int64_t)C * HW > (int64_t)0x7fffffff) return false;
  int cc, nchunks;
  ta_partition(C, HW, 1, cc, nchunks);
  return (int64_t)B * nchunks <= (int64_t)0x7fffffff;
}

// log2 of the lanes per row
inline int ta_gshift(int HW, bool v4) {
  int s = 0, full = 0;
  while (s < 6 && (16 << s) < HW) ++s;        // about 16 elements per lane
  while (full < 6 && (1 << full) < HW) ++full;  // lanes that a row can feed at all
  const int smin = full < 4 ? full : 4;       // 16 lanes x 4 bytes: runs of 64 bytes where a row is that long
  if (s < smin) s = smin;
  if (v4) s = s > 2 ? s - 2 : 0;              // a lane takes 4 elements at once
  return s;
}

// the value of the lane at byte address `addr` (4 x lane): two ds_bpermute_b32, nothing else
__device__ __forceinline__ double ta_shfl(double v, int addr) {
  const int lo = __builtin_amdgcn_ds_bpermute(addr, __double2loint(v)), hi = __builtin_amdgcn_ds_bpermute(addr, __double2hiint(v));
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double ta_sum4(const float4 v) { return ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w); }

template <bool V4>
__global__ __launch_bounds__(TA_THREADS) void twoafc_partial_kernel(const ta_params p) {
  __shared__ double red[4][5];
  const int b = blockIdx.x / p.nchunks, k = blockIdx.x - b * p.nchunks;
  const int64_t c0 = (int64_t)k * p.cc, c1 = min(c0 + p.cc, (int64_t)p.C);
  const int G = 1 << p.gshift, gl = threadIdx.x & (G - 1), gid = threadIdx.x >> p.gshift, ng = TA_THREADS >> p.gshift;
  const size_t img = (size_t)b * (size_t)p.ld;
  const float* r = p.ref + img;
  const float* l = p.left + img;
  const float* q = p.right + img;
  int xaddr[6];  // byte address of lane ^ 2^s for the butterfly inside a group, computed once (__shfl_xor recomputes it per call)
#pragma unroll
  for (int s = 0; s < 6; ++s) xaddr[s] = (int)(((threadIdx.x & 63) ^ (1u << s)) << 2);
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t c = c0 + gid; c < c1; c += ng) {  // every lane of a group runs the same trips; groups exchange nothing
    const size_t row = (size_t)c * p.HW;
    double sr = 0.0, sl = 0.0, sq = 0.0;
    if (V4) {
      const float4* r4 = (const float4*)(r + row);
      const float4* l4 = (const float4*)(l + row);
      const float4* q4 = (const float4*)(q + row);
      const int64_t n4 = p.HW >> 2, step = 2 * (int64_t)G;
      int64_t u = 0;
      for (; u + step <= n4; u += step) {  // 6 loads in flight
        const float4 a0 = r4[u + gl], u0 = l4[u + gl], v0 = q4[u + gl];
        const float4 a1 = r4[u + G + gl], u1 = l4[u + G + gl], v1 = q4[u + G + gl];
        sr += ta_sum4(a0); sl += ta_sum4(u0); sq += ta_sum4(v0);
        sr += ta_sum4(a1); sl += ta_sum4(u1); sq += ta_sum4(v1);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int64_t i = u + j * G + gl;
        if (u + j * G < n4) {  // uniform: some lane of the group still has a position
          const bool ok = i < n4;
          const int64_t ic = ok ? i : n4 - 1;  // in the row whatever the lane: the load is always legal, its value dropped
          const float4 a = r4[ic], uu = l4[ic], v = q4[ic];
          sr += ok ? ta_sum4(a) : 0.0;
          sl += ok ? ta_sum4(uu) : 0.0;
          sq += ok ? ta_sum4(v) : 0.0;
        }
      }
    } else {
      const float* rr = r + row;
      const float* ll = l + row;
      const float* qq = q + row;
      const int64_t n = p.HW, step = 4 * (int64_t)G;
      int64_t u = 0;
      for (; u + step <= n; u += step) {  // 12 loads in flight
        float a[4], uu[4], v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          a[j] = rr[u + j * G + gl];
          uu[j] = ll[u + j * G + gl];
          v[j] = qq[u + j * G + gl];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          sr += (double)a[j];
          sl += (double)uu[j];
          sq += (double)v[j];
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t i = u + j * G + gl;
        if (u + j * G < n) {  // uniform
          const bool ok = i < n;
          const int64_t ic = ok ? i : n - 1;
          const float a = rr[ic], uu = ll[ic], v = qq[ic];
          sr += ok ? (double)a : 0.0;
          sl += ok ? (double)uu : 0.0;
          sq += ok ? (double)v : 0.0;
        }
      }
    }
#pragma unroll
    for (int s = 5; s >= 0; --s) {
      if (s < p.gshift) {  // uniform over the workgroup
        sr += ta_shfl(sr, xaddr[s]);
        sl += ta_shfl(sl, xaddr[s]);
        sq += ta_shfl(sq, xaddr[s]);
      }
    }
    if (gl == 0) {
      acc[0] = fma(sr, sl, acc[0]);
      acc[1] = fma(sr, sq, acc[1]);
      acc[2] = fma(sr, sr, acc[2]);
      acc[3] = fma(sl, sl, acc[3]);
      acc[4] = fma(sq, sq, acc[4]);
    }
  }
  block_sum<5>(acc, red);  // (block_sum_once here: 64 VGPRs for 103 in the dword form and 2.6 % slower, profiles/reduce_header_bench.txt)
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < 5; ++j) p.ws[(size_t)blockIdx.x * 5 + j] = acc[j];
  }
}

// <f_ref, f_x> / (max(|f_ref|, 1e-8) * max(|f_x|, 1e-8)) from the sums over channels of the pooled SUMS; nr = the clamped |f_ref|.
// A NaN or inf norm comes with a NaN or inf dot product, so the result is NaN exactly where the definition's is.
__device__ __forceinline__ float ta_cosine(double dot, double nx2, double nr, double hw) {
  const double nx = fmax(sqrt(nx2) / hw, 1e-8);
  return (float)((dot / (hw * hw)) / (nr * nx));
}

__global__ __launch_bounds__(TA_THREADS) void twoafc_finish_kernel(const ta_params p) {
  const int b = blockIdx.x * (TA_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= p.B) return;  // whole waves
  double v[5];
  wave_fold_rows<5>(p.ws + (size_t)b * p.nchunks * 5, p.nchunks, v);
  if (lane != 0) return;
  const double hw = (double)p.HW;
  const double nr = fmax(sqrt(v[2]) / hw, 1e-8);
  const float s_l = ta_cosine(v[0], v[3], nr, hw), s_r = ta_cosine(v[1], v[4], nr, hw);
  twoafc_verdict(s_l, s_r, b, p.sim, p.pred, p.label, p.counts);
}

}  // namespace

extern "C" int64_t mvp_twoafc_workspace_bytes(int B, int C, int HW) {
  if (!ta_sizes_ok(B, C, HW)) return 0;
  int cc, nchunks;
  ta_partition(C, HW, 1, cc, nchunks);
  return (int64_t)B * nchunks * 5 * (int64_t)sizeof(double);
}

extern "C" int mvp_twoafc_score(const mvp_twoafc_args* a, void* stream) {
  if (!a || !a->ref || !a->left || !a->right || !a->sim || !a->pred) return MVP_EINVAL;
  if (a->counts && !a->label) return MVP_EINVAL;
  if (!ta_sizes_ok(a->B, a->C, a->HW) || a->ld < (int64_t)a->C * a->HW) return MVP_EINVAL;
  if (!a->workspace || !aligned_to(a->workspace, 8) || a->workspace_bytes < mvp_twoafc_workspace_bytes(a->B, a->C, a->HW)) return MVP_EINVAL;
  if (!aligned_to(a->counts, 8)) return MVP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ta_params p;
  p.ref = a->ref; p.left = a->left; p.right = a->right; p.label = a->label;
  p.sim = a->sim; p.pred = a->pred; p.counts = a->counts; p.ws = (double*)a->workspace;
  p.ld = a->ld; p.B = a->B; p.C = a->C; p.HW = a->HW;
  const bool v4 = (a->HW & 3) == 0 && (a->ld & 3) == 0 && aligned_to(a->ref, 16) && aligned_to(a->left, 16) && aligned_to(a->right, 16);
  p.gshift = ta_gshift(a->HW, v4);
  ta_partition(a->C, a->HW, TA_THREADS >> p.gshift, p.cc, p.nchunks);  // never more chunks than the workspace query counted
  if (a->counts && !a->accumulate && hipMemsetAsync(a->counts, 0, 4 * sizeof(int64_t), s) != hipSuccess) return MVP_ELAUNCH;
  const dim3 grid((unsigned)((int64_t)a->B * p.nchunks));
  if (v4) hipLaunchKernelGGL(twoafc_partial_kernel<true>, grid, dim3(TA_THREADS), 0, s, p);
  else hipLaunchKernelGGL(twoafc_partial_kernel<false>, grid, dim3(TA_THREADS), 0, s, p);
  hipLaunchKernelGGL(twoafc_finish_kernel, dim3((unsigned)((a->B - 1) / 4 + 1)), dim3(TA_THREADS), 0, s, p);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}
