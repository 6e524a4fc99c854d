// Top-2 cosine nearest neighbours with the ratio test (mvp_knn_ratio): the hot loop of the NAVI / ScanNet 3-D correspondence
// evaluation (evals/utils/correspondence.py:26-121; the reference searches with faiss and recomputes the distances exactly).
//
//   pack      per view: inverse L2 norm per column of the channel-major [C, N] map, then the normalised rows row-major [N, Cpad] in
//             fp32 (for the exact step) and as the compensated fp16 pair of MVP_PREC_F16X2 (queries: activation form, targets: weight
//             form; mvp_common.h), C zero-padded to a multiple of 32.
//   cand      one workgroup = 128 queries x one slice of the target range.  Target tiles of 128 stream through LDS; the scores of a
//             tile are 32x32x16 f16 MFMA accumulators with the TARGETS on the rows and the QUERIES on the columns, so that a lane
//             holds 16 target scores of ONE query per MFMA tile and keeps that query's best 4 (score, index) in registers with no
//             lane traffic.  The lists of the 2 lane halves x 2 waves that share a query are merged through LDS once, at the end,
//             and the slice's best 4 go to the workspace.  The N0 x N1 score matrix is never written.
//   refine    one wave per query: merge the slices' lists to the best 4 by MFMA score, recompute those 4 distances in fp32 from the
//             fp32 rows, order them, write nn_idx / dist / weight.
// Every merge orders by (score descending, index ascending): ties go to the lowest target index and the result does not depend on
// how the targets were sliced.  Bounds are handled by masking: rows beyond N0 / N1 are loaded as zeros and their scores never enter a list.
#include <math.h>

#include "mvp_common.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16_t;

constexpr int KNN_TQ = 128;   // queries per workgroup
constexpr int KNN_TT = 128;   // targets per LDS tile
constexpr int KNN_BK = 32;    // channels per LDS tile (two k = 16 MFMA steps)
constexpr int KNN_LDR = 80;   // bytes per LDS row: 64 of data + 16 of padding (keeps 16-byte alignment, spreads the banks)
constexpr int KNN_ARR = KNN_TQ * KNN_LDR;  // bytes of one 128-row operand image
constexpr int KNN_KEEP = 4;   // candidates kept per query
constexpr int KNN_BLOCKS = 512;  // workgroups the target slicing aims at (2 per CU of a 256-CU part; a constant, so that the workspace size is a pure function of the shape)

struct knn_plan {
  int Cpad, qtiles, ttiles, tps, splits;  // tps: target tiles per slice
};

inline knn_plan knn_make_plan(int C, int N0, int N1) {
  knn_plan p;
  p.Cpad = (C + KNN_BK - 1) / KNN_BK * KNN_BK;
  p.qtiles = (N0 + KNN_TQ - 1) / KNN_TQ;
  p.ttiles = (N1 + KNN_TT - 1) / KNN_TT;
  int want = (KNN_BLOCKS + p.qtiles - 1) / p.qtiles;
  if (want > p.ttiles) want = p.ttiles;
  if (want < 1) want = 1;
  p.tps = (p.ttiles + want - 1) / want;
  p.splits = (p.ttiles + p.tps - 1) / p.tps;
  return p;
}

__device__ __forceinline__ bool knn_better(float s, int i, float v, int j) {
  return s > v || (s == v && (unsigned)i < (unsigned)j);  // an empty slot is (-inf, -1): -1 is the largest unsigned index
}

// insert (s, idx) into a list sorted by (score descending, index ascending)
__device__ __forceinline__ void knn_insert(float (&v)[KNN_KEEP], int (&i)[KNN_KEEP], float s, int idx) {
  if (!knn_better(s, idx, v[KNN_KEEP - 1], i[KNN_KEEP - 1])) return;
  v[KNN_KEEP - 1] = s;
  i[KNN_KEEP - 1] = idx;
#pragma unroll
  for (int k = KNN_KEEP - 1; k > 0; --k) {
    const bool up = knn_better(v[k], i[k], v[k - 1], i[k - 1]);
    const float tv = v[k - 1];
    const int ti = i[k - 1];
    v[k - 1] = up ? v[k] : tv;
    i[k - 1] = up ? i[k] : ti;
    v[k] = up ? tv : v[k];
    i[k] = up ? ti : i[k];
  }
}

// valid rows of both views: n_valid[0] queries, n_valid[1] targets (block b counts view b)
__global__ __launch_bounds__(256) void knn_count_kernel(const uint8_t* sv, const uint8_t* tv, int N0, int N1, int32_t* n_valid) {
  __shared__ int part[256];
  const uint8_t* m = blockIdx.x ? tv : sv;
  const int N = blockIdx.x ? N1 : N0;
  int c = 0;
  if (m)
    for (int i = threadIdx.x; i < N; i += 256) c += m[i] != 0;
  part[threadIdx.x] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) n_valid[blockIdx.x] = m ? part[0] : N;
}

// One workgroup packs 64 columns of a [C, N] map.  WEIGHT selects the pair form (targets) against the activation form (queries).
template <bool WEIGHT>
__global__ __launch_bounds__(256) void knn_pack_kernel(const float* f, int C, int Cpad, int N, float* rows, uint16_t* hi, uint16_t* lo) {
  __shared__ float s_part[4][64];
  __shared__ float s_den[64];
  __shared__ float s_tile[64][KNN_BK + 1];
  const int tid = threadIdx.x, tn = tid & 63, ts = tid >> 6;
  const int n0 = blockIdx.x * 64, n = n0 + tn;
  const bool ok = n < N;
  float s = 0.f;
  for (int c = ts; c < C; c += 4) {
    const float v = ok ? f[(size_t)c * N + n] : 0.f;
    s = fmaf(v, v, s);
  }
  s_part[ts][tn] = s;
  __syncthreads();
  if (tid < 64) s_den[tid] = fmaxf(sqrtf((s_part[0][tid] + s_part[1][tid]) + (s_part[2][tid] + s_part[3][tid])), 1e-12f);  // F.normalize eps
  __syncthreads();
  const float den = s_den[tn];
  const int rn = tid >> 2, ch = (tid & 3) * 8;
  for (int c0 = 0; c0 < Cpad; c0 += KNN_BK) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int cc = c0 + ts + 4 * j;
      s_tile[tn][ts + 4 * j] = (ok && cc < C) ? f[(size_t)cc * N + n] / den : 0.f;
    }
    __syncthreads();
    if (n0 + rn < N) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = s_tile[rn][ch + j];
      const size_t o = (size_t)(n0 + rn) * Cpad + c0 + ch;
      *(f32x4_t*)(rows + o) = f32x4_t{v[0], v[1], v[2], v[3]};
      *(f32x4_t*)(rows + o + 4) = f32x4_t{v[4], v[5], v[6], v[7]};
      uint32_t h[4], l[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (WEIGHT) split2_f16_wcomp(v[2 * j], v[2 * j + 1], h[j], l[j]);
        else split2_f16_comp(v[2 * j], v[2 * j + 1], h[j], l[j]);
      }
      *(u32x4_t*)(hi + o) = u32x4_t{h[0], h[1], h[2], h[3]};
      *(u32x4_t*)(lo + o) = u32x4_t{l[0], l[1], l[2], l[3]};
    }
    __syncthreads();
  }
}

struct knn_cand_args {
  const uint16_t* q_hi; const uint16_t* q_lo; const uint16_t* t_hi; const uint16_t* t_lo;
  const uint8_t* t_valid;
  u32x2_t* cand;  // [splits][N0][KNN_KEEP] (score bits, index)
  int Cpad, N0, N1, ttiles, tps;
};

// 16 bytes of row `row` of a [N, Cpad] 16-bit array, zeros beyond N
__device__ __forceinline__ u32x4_t knn_load16(const uint16_t* base, int row, int N, int Cpad, int col) {
  if (row >= N) return u32x4_t{0u, 0u, 0u, 0u};
  return *(const u32x4_t*)(base + (size_t)row * Cpad + col);
}

__global__ __launch_bounds__(256) void knn_cand_kernel(const knn_cand_args p) {
  __shared__ u32x4_t smem4[4 * KNN_ARR / 16];  // q_hi | q_lo | t_hi | t_lo images of [128][KNN_LDR bytes]; reused for the final merge
  __shared__ uint8_t s_tv[KNN_TT];
  char* smem = (char*)smem4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wq = wave & 1, wt = wave >> 1;  // the wave's 64 queries / 64 targets of the tile
  const int lr = lane & 31, lh = lane >> 5;
  const int q0 = blockIdx.x * KNN_TQ;
  const int t_begin = blockIdx.y * p.tps;
  const int t_end = min(t_begin + p.tps, p.ttiles);
  const int KT = p.Cpad / KNN_BK;
  const int total = (t_end - t_begin) * KT;
  const int ld_row = tid >> 2, ld_col = (tid & 3) * 8;  // loader: rows ld_row and ld_row + 64, 8 halves at ld_col

  float bv[2][KNN_KEEP];
  int bi[2][KNN_KEEP];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int k = 0; k < KNN_KEEP; ++k) { bv[a][k] = -INFINITY; bi[a][k] = -1; }

  u32x4_t pre[4][2];
  {
    const int t0 = t_begin * KNN_TT;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      pre[0][h] = knn_load16(p.q_hi, q0 + ld_row + 64 * h, p.N0, p.Cpad, ld_col);
      pre[1][h] = knn_load16(p.q_lo, q0 + ld_row + 64 * h, p.N0, p.Cpad, ld_col);
      pre[2][h] = knn_load16(p.t_hi, t0 + ld_row + 64 * h, p.N1, p.Cpad, ld_col);
      pre[3][h] = knn_load16(p.t_lo, t0 + ld_row + 64 * h, p.N1, p.Cpad, ld_col);
    }
  }
  f32x16_t acc[2][2];
  int tile = t_begin, kt = 0;
  for (int it = 0; it < total; ++it) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int h = 0; h < 2; ++h) *(u32x4_t*)(smem + a * KNN_ARR + (ld_row + 64 * h) * KNN_LDR + ld_col * 2) = pre[a][h];
    if (kt == 0 && tid < KNN_TT) {
      const int t = tile * KNN_TT + tid;
      s_tv[tid] = (t < p.N1 && (!p.t_valid || p.t_valid[t])) ? 1 : 0;
    }
    __syncthreads();
    if (it + 1 < total) {
      const int nkt = (kt + 1 == KT) ? 0 : kt + 1;
      const int t0 = ((kt + 1 == KT) ? tile + 1 : tile) * KNN_TT;
      const int col = nkt * KNN_BK + ld_col;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        pre[0][h] = knn_load16(p.q_hi, q0 + ld_row + 64 * h, p.N0, p.Cpad, col);
        pre[1][h] = knn_load16(p.q_lo, q0 + ld_row + 64 * h, p.N0, p.Cpad, col);
        pre[2][h] = knn_load16(p.t_hi, t0 + ld_row + 64 * h, p.N1, p.Cpad, col);
        pre[3][h] = knn_load16(p.t_lo, t0 + ld_row + 64 * h, p.N1, p.Cpad, col);
      }
    }
    if (kt == 0) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nq = 0; nq < 2; ++nq)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[mt][nq][r] = 0.f;
    }
#pragma unroll
    for (int s = 0; s < KNN_BK / 16; ++s) {
      const int koff = s * 32 + lh * 16;  // bytes: k = 16 s + 8 (lane >> 5) .. + 7
      f16x8_t qh[2], ql[2], th[2], tl[2];
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        const int qrow = (wq * 64 + x * 32 + lr) * KNN_LDR + koff, trow = (wt * 64 + x * 32 + lr) * KNN_LDR + koff;
        qh[x] = *(const f16x8_t*)(smem + 0 * KNN_ARR + qrow);
        ql[x] = *(const f16x8_t*)(smem + 1 * KNN_ARR + qrow);
        th[x] = *(const f16x8_t*)(smem + 2 * KNN_ARR + trow);
        tl[x] = *(const f16x8_t*)(smem + 3 * KNN_ARR + trow);
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nq = 0; nq < 2; ++nq) {
          acc[mt][nq] = __builtin_amdgcn_mfma_f32_32x32x16_f16(tl[mt], ql[nq], acc[mt][nq], 0, 0, 0);
          acc[mt][nq] = __builtin_amdgcn_mfma_f32_32x32x16_f16(th[mt], qh[nq], acc[mt][nq], 0, 0, 0);
        }
    }
    if (kt == KT - 1) {
      // accumulator r of lane (lr, lh) = target row (r & 3) + 8 (r >> 2) + 4 lh of the MFMA tile, query column lr; visited in ascending
      // target index, so the (score, index) order keeps the lowest index among equal scores
#pragma unroll
      for (int nq = 0; nq < 2; ++nq)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int tl_ = wt * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (s_tv[tl_]) knn_insert(bv[nq], bi[nq], acc[mt][nq][r], tile * KNN_TT + tl_);  // an invalid or out-of-range column never enters a list
          }
    }
    __syncthreads();
    if (++kt == KT) { kt = 0; ++tile; }
  }

  // merge the 4 lists of each query (2 target halves of the tile x 2 lane halves) and write the slice's best KNN_KEEP
  u32x2_t* s_c = (u32x2_t*)smem;  // [128 queries][4 sources][KNN_KEEP]: 16 KiB of the 40 KiB above (the loop ended on a barrier)
#pragma unroll
  for (int nq = 0; nq < 2; ++nq)
#pragma unroll
    for (int k = 0; k < KNN_KEEP; ++k)
      s_c[((wq * 64 + nq * 32 + lr) * 4 + wt * 2 + lh) * KNN_KEEP + k] = u32x2_t{f2u(bv[nq][k]), (uint32_t)bi[nq][k]};
  __syncthreads();
  if (tid < KNN_TQ && q0 + tid < p.N0) {
    float v[KNN_KEEP];
    int i[KNN_KEEP];
#pragma unroll
    for (int k = 0; k < KNN_KEEP; ++k) { v[k] = -INFINITY; i[k] = -1; }
    for (int e = 0; e < 4 * KNN_KEEP; ++e) {
      const u32x2_t c = s_c[tid * 4 * KNN_KEEP + e];
      const uint32_t cs = c[0], ci = c[1];
      if ((int)ci >= 0) knn_insert(v, i, u2f(cs), (int)ci);
    }
    u32x4_t* out = (u32x4_t*)(p.cand + ((size_t)blockIdx.y * p.N0 + q0 + tid) * KNN_KEEP);
    out[0] = u32x4_t{f2u(v[0]), (uint32_t)i[0], f2u(v[1]), (uint32_t)i[1]};
    out[1] = u32x4_t{f2u(v[2]), (uint32_t)i[2], f2u(v[3]), (uint32_t)i[3]};
  }
}

struct knn_refine_args {
  const float* q_rows; const float* t_rows;
  const uint8_t* q_valid;
  const u32x2_t* cand;
  int32_t* nn_idx; float* dist; float* weight;
  int Cpad, N0, splits;
};

__global__ __launch_bounds__(256) void knn_refine_kernel(const knn_refine_args p) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= p.N0) return;  // whole waves leave: no barrier below
  float v[KNN_KEEP];
  int i[KNN_KEEP];
#pragma unroll
  for (int k = 0; k < KNN_KEEP; ++k) { v[k] = -INFINITY; i[k] = -1; }
  for (int s = 0; s < p.splits; ++s) {
    const u32x2_t* c = p.cand + ((size_t)s * p.N0 + q) * KNN_KEEP;
#pragma unroll
    for (int k = 0; k < KNN_KEEP; ++k) {
      const u32x2_t e = c[k];
      const uint32_t es = e[0], ei = e[1];
      if ((int)ei >= 0) knn_insert(v, i, u2f(es), (int)ei);
    }
  }
  const bool q_ok = !p.q_valid || p.q_valid[q];
  if (!q_ok || i[1] < 0) {  // an invalid query, or fewer than two valid targets
    if (lane == 0) {
      p.nn_idx[q] = -1;
      p.dist[2 * q] = INFINITY;
      p.dist[2 * q + 1] = INFINITY;
      p.weight[q] = -INFINITY;
    }
    return;
  }
  // exact step: 1 - <q^, t^> in fp32 from the fp32 rows, lanes across the channels, butterfly sum
  float dot[KNN_KEEP] = {0.f, 0.f, 0.f, 0.f};
  const float* qr = p.q_rows + (size_t)q * p.Cpad;
  const float* tr[KNN_KEEP];
#pragma unroll
  for (int k = 0; k < KNN_KEEP; ++k) tr[k] = p.t_rows + (size_t)(i[k] >= 0 ? i[k] : 0) * p.Cpad;  // never dereferenced for an empty slot
  for (int c = lane; c < p.Cpad; c += 64) {
    const float qv = qr[c];
#pragma unroll
    for (int k = 0; k < KNN_KEEP; ++k)
      if (i[k] >= 0) dot[k] = fmaf(qv, tr[k][c], dot[k]);
  }
  float d[KNN_KEEP];
  int di[KNN_KEEP];
#pragma unroll
  for (int k = 0; k < KNN_KEEP; ++k) {
    d[k] = i[k] >= 0 ? 1.0f - wave_sum(dot[k]) : INFINITY;
    di[k] = i[k];
  }
  // the two smallest by (distance ascending, index ascending)
  float d0 = INFINITY, d1 = INFINITY;
  int i0 = -1, i1 = -1;
#pragma unroll
  for (int k = 0; k < KNN_KEEP; ++k) {
    if (di[k] < 0) continue;
    if (d[k] < d0 || (d[k] == d0 && (unsigned)di[k] < (unsigned)i0)) {
      d1 = d0; i1 = i0;
      d0 = d[k]; i0 = di[k];
    } else if (d[k] < d1 || (d[k] == d1 && (unsigned)di[k] < (unsigned)i1)) {
      d1 = d[k]; i1 = di[k];
    }
  }
  if (lane == 0) {
    p.nn_idx[q] = i0;
    p.dist[2 * q] = d0;
    p.dist[2 * q + 1] = d1;
    p.weight[q] = 1.0f - fmaxf(d0, 1e-9f) / fmaxf(d1, 1e-9f);  // calculate_ratio_test: both clamps
  }
}

inline bool knn_shape_ok(int C, int N0, int N1) { return C > 0 && C <= 16384 && N0 > 0 && N1 >= 2 && N0 <= (1 << 24) && N1 <= (1 << 24); }

}  // namespace

extern "C" int64_t mvp_knn_workspace_bytes(int C, int N0, int N1) {
  if (!knn_shape_ok(C, N0, N1)) return 0;
  const knn_plan pl = knn_make_plan(C, N0, N1);
  // fp32 rows (4 B) + the fp16 pair (2 + 2 B) of both views, then the slices' candidate lists (8 B each)
  return ((int64_t)N0 + N1) * pl.Cpad * 8 + (int64_t)pl.splits * N0 * KNN_KEEP * 8;
}

extern "C" int mvp_knn_ratio(const mvp_knn_ratio_args* a, void* stream) {
  if (!a || !a->src_feat || !a->tgt_feat || !a->nn_idx || !a->dist || !a->weight || !a->n_valid || !a->workspace) return MVP_EINVAL;
  if (!knn_shape_ok(a->C, a->N0, a->N1)) return MVP_EINVAL;
  if (a->workspace_bytes < mvp_knn_workspace_bytes(a->C, a->N0, a->N1) || ((uintptr_t)a->workspace & 15)) return MVP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const knn_plan pl = knn_make_plan(a->C, a->N0, a->N1);
  const int64_t nq = (int64_t)a->N0 * pl.Cpad, nt = (int64_t)a->N1 * pl.Cpad;
  char* w = (char*)a->workspace;
  float* q_rows = (float*)w;                  w += nq * 4;
  float* t_rows = (float*)w;                  w += nt * 4;
  uint16_t* q_hi = (uint16_t*)w;              w += nq * 2;
  uint16_t* q_lo = (uint16_t*)w;              w += nq * 2;
  uint16_t* t_hi = (uint16_t*)w;              w += nt * 2;
  uint16_t* t_lo = (uint16_t*)w;              w += nt * 2;
  u32x2_t* cand = (u32x2_t*)w;
  hipLaunchKernelGGL(knn_count_kernel, dim3(2), dim3(256), 0, s, a->src_valid, a->tgt_valid, a->N0, a->N1, a->n_valid);
  hipLaunchKernelGGL(knn_pack_kernel<false>, dim3((a->N0 + 63) / 64), dim3(256), 0, s, a->src_feat, a->C, pl.Cpad, a->N0, q_rows, q_hi, q_lo);
  hipLaunchKernelGGL(knn_pack_kernel<true>, dim3((a->N1 + 63) / 64), dim3(256), 0, s, a->tgt_feat, a->C, pl.Cpad, a->N1, t_rows, t_hi, t_lo);
  const knn_cand_args ca = {q_hi, q_lo, t_hi, t_lo, a->tgt_valid, cand, pl.Cpad, a->N0, a->N1, pl.ttiles, pl.tps};
  hipLaunchKernelGGL(knn_cand_kernel, dim3(pl.qtiles, pl.splits), dim3(256), 0, s, ca);
  const knn_refine_args ra = {q_rows, t_rows, a->src_valid, cand, a->nn_idx, a->dist, a->weight, pl.Cpad, a->N0, pl.splits};
  hipLaunchKernelGGL(knn_refine_kernel, dim3((a->N0 + 3) / 4), dim3(256), 0, s, ra);
  MVP_LAUNCH_CHECK();
  return MVP_OK;
}
