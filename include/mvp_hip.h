/*
 * mvp_hip.h — C ABI of libmvp_hip.so: the MI355X (gfx950) kernels behind the
 * midvision-probe feature-extraction + probe-training hot path.
 *
 * Conventions (SURVEY.md §8b "Lower" boundary):
 *   - every entry point is  extern "C" int mvp_<op>(const mvp_<op>_args*, void* hip_stream)
 *     returning 0 on success or a negative MVP_E* code; nothing throws, nothing exits;
 *   - plain pointers and sizes only (no torch types); all pointers are DEVICE pointers
 *     unless a field says "host";
 *   - the caller allocates every buffer, including workspaces (sizes documented per op);
 *   - kernels are enqueued asynchronously on the stream passed in; no hidden syncs, no
 *     allocation, no global mutable state  => safe under hipGraph capture, re-entrant
 *     across streams and devices;
 *   - "bf16 pair" = two uint16 bf16 arrays (hi, lo) with value = hi + lo.  With
 *     precision MVP_PREC_BF16 only hi is read/written (lo pointers may be NULL); with
 *     MVP_PREC_BF16X3 contractions run as hi*hi + hi*lo + lo*hi on the bf16 MFMA pipe
 *     with fp32 accumulation (~2^-16 relative operand error, needed for the reference's
 *     1e-3 feature-parity bar).
 *
 * Each op cites the reference interface (file:line under the upstream repo) it replaces.
 */
#ifndef MVP_HIP_H
#define MVP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVP_OK 0
#define MVP_EINVAL (-1)   /* bad argument (shape / alignment / NULL) */
#define MVP_ELAUNCH (-2)  /* hipLaunch failed */
#define MVP_ENODEV (-3)   /* no gfx950 device */

#define MVP_PREC_BF16 1   /* one bf16 MFMA pass                              */
#define MVP_PREC_BF16X3 3 /* three passes (split bf16), ~fp32 operand accuracy */
#define MVP_PREC_F16X2 2  /* (ABI 6; the ViT wrappers' default) TWO fp16 passes per contraction of mvp_gemm_bias_act_res / mvp_gemm_pp (plain linear GEMMs only), with the
                             weight's fp16 rounding error carried by the second pass ("compensated" pairs).  With s = 2^-6:
                               activation  a_hi = fp16(a),            a_lo = fp16(8 (a - a_hi) + a_hi / 8)       (LayerNorm / attention out_f16 = 1,
                                                                                                                  a GEMM epilogue's out_f16_col0 = -1)
                               weight      w_hi = fp16((1 - s) w),    w_lo = fp16((w + d / s) / 8),  d = (1 - s) w - w_hi    (built once, frozen)
                             and the product runs as  a_lo . w_lo + a_hi . w_hi  (two f16 MFMAs, fp32 accumulate).  Exactly:
                               a_hi w_hi + a_lo w_lo = a_hi ((1 - s) w - d) + ((a - a_hi) + s a_hi) (w + d / s) = a w + (a - a_hi) d / s,
                             i.e. the s a_hi w that the first pass leaves out and its rounding error d both ride in the second; what is left is
                             (a - a_hi) d / s <= 2^-12 * 2^-6 |a w| plus the fp16 roundings of a_lo and w_lo (2^-18 each) — the accuracy class of
                             BF16X3 (tests/test_gpu_kernels.py measures it against fp64, with the ViT goldens' feature error) at 2/3 of its
                             matrix-pipe work, on a chip whose clock is held down by exactly that work (the large-M kernel: -19 % time).
                             Range: |a| <= 65504 (hi and lo saturate there; beyond it the result is wrong, not NaN); values whose lo half falls
                             below fp16's normal range (|a| < 5e-4, |w| < 5e-4) keep absolute, not relative, precision.
                             The ViT wrappers run this mode unless told otherwise (mvp/backbone.py default_precision(); MVP_PREC_BF16X3 is what a bare
                             engine, the ResNet / ConvNeXt trunks and the probes run).  Because saturation is silent, the wrappers carry a range
                             guard (range_guard= / MVP_F16_GUARD: off | auto | warn | raise | fallback): one audited forward in which
                             mvp_f16_range_scan reads every fp16-form operand right before its consumer; a saturated or non-finite half
                             warns, raises, or rebuilds the engine in MVP_PREC_BF16X3.  `auto` (the default) arms it for weights read from a
                             checkpoint file only.                                                                                            */

#define MVP_ACT_NONE 0
#define MVP_ACT_GELU 1 /* exact erf GELU (torch nn.GELU default)            */
#define MVP_ACT_RELU 2
/* (added within ABI 8; constants only.)  The two sigmoid-form GELUs, x / (1 + exp2(-k(x))), for plain linear GEMMs — mvp_gemm_bias_act_res,
 * mvp_gemm_pp, mvp_gemm_scaled, mvp_gemm_route: every kernel family and both epilogue outputs (pair, the MVP_PREC_F16X2 activation pair of
 * out_f16_col0 = -1 included, and fp32), the same bits from each.  Convolutions (conv), split-K (splitk > 1) and the mask / pair-residual /
 * residual2 / act_after_res forms return MVP_EINVAL for them, as does any act value outside MVP_ACT_NONE ... MVP_ACT_GELU_TANH.  Max |error|
 * against fp64 over [-12, 12]: see DESIGN.md. */
#define MVP_ACT_QUICK_GELU 3 /* x sigmoid(1.702 x): OpenAI CLIP                                          */
#define MVP_ACT_GELU_TANH 4  /* x/2 (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))): torch nn.GELU("tanh"), SigLIP */

typedef uint16_t mvp_bf16;

/* Library / device introspection. Returns MVP_OK and fills the fields. */
typedef struct {
  int abi_version;      /* = MVP_ABI_VERSION                                 */
  int device_count;     /* visible HIP devices (0 on a CPU-only box)         */
  int gfx950;           /* 1 if device 0 is gfx950                           */
  int cu_count;         /* multiProcessorCount of device 0                   */
  char arch[64];        /* gcnArchName of device 0                           */
} mvp_info_t;
#define MVP_ABI_VERSION 8 /* 8: two exports removed, one added.  Removed: the round-2 k-balanced GEMM (its launch and workspace query; slower than
                                the tile kernels on every shape measured), so splitk < 0 is now MVP_EINVAL.  Added: mvp_gemm_route
                                (and its struct mvp_gemm_route_t, tagged like the later additions within 7), which reports the kernel
                                mvp_gemm_bias_act_res would run.  Every other struct, mvp_gemm_args included, as in 7.
                                Added within 8: mvp_rope2d_qkv (a new export with its own tagged argument struct; no existing struct changed).
                                Added within 8: mvp_attention_bias_fwd (attention with a dense per-head additive logit bias; a new export with its own
                                tagged argument struct that wraps mvp_attention_args unchanged).
                                Added within 8: mvp_gather_rows (row gather of 16-bit pair buffers by an index table), mvp_relpos_terms (SAM's
                                decomposed relative-position terms of the unscaled q) and mvp_attention_relpos_fwd (attention with that decomposed
                                bias); three new exports, each with its own tagged argument struct, no existing struct changed.
                                Added within 8: mvp_knn_ratio and mvp_knn_workspace_bytes (top-2 cosine nearest neighbours with the ratio test,
                                NAVI / ScanNet 3-D correspondence); a new export with its own tagged argument struct, no existing struct changed.
                                Added within 8: mvp_bn_act_fwd, mvp_bn_act_bwd, mvp_bce_loss_fwd_bwd and mvp_binary_counts (the tail of the objectness
                                probe: BatchNorm2d + sigmoid on a few-channel map, BCELoss, confusion counts); new exports with their own tagged
                                argument structs, no existing struct changed.
                                Added within 8: mvp_pointcloud_sample (zero-padded bilinear sampling of a feature map at the projections of a point
                                cloud, ScanNet pair correspondence); a new export with its own tagged argument struct, no existing struct changed.
                                Added within 8: mvp_twoafc_score and mvp_twoafc_workspace_bytes (pooled cosine scoring of 2AFC triplets with the
                                running confusion counts, the perceptual-similarity evaluation); new exports with their own tagged argument struct,
                                no existing struct changed.
                                Added within 8: mvp_ncut_affinity, mvp_ncut_threshold, mvp_ncut_fiedler, mvp_ncut_partition and
                                mvp_ncut_workspace_bytes (MaskCut: thresholded patch affinity, LDS-resident normalised-cut solver, partition);
                                new exports with their own tagged argument structs, no existing struct changed.
                                Added within 8: mvp_dwconv7_ln_fwd, mvp_grn_stats, mvp_grn_apply and mvp_grn_workspace_bytes (ConvNeXt / ConvNeXt V2
                                blocks: depthwise 7x7 + LayerNorm, global response normalisation); new exports with their own tagged argument
                                structs, no existing struct changed.
                                Added within 8: mvp_crf_filter, mvp_crf_update and mvp_mask_finish (dense-CRF refinement of the MaskCut masks: exact
                                all-pairs Gaussian filtering, mean-field update, hole filling / IoU rule / union); new exports with their own tagged
                                argument structs, no existing struct changed.
                                Added within 8: mvp_augment_stats, mvp_augment_apply and mvp_augment_partials_bytes (device-side training
                                augmentation: fused ColorJitter + shared flip / rotate / resized crop + normalisation); new exports with their own
                                tagged argument structs, no existing struct changed.
                                Added within 8: mvp_swiglu_fwd (the gate of DINOv2's SwiGLU MLP, silu(x1) * x2 between the w12 and w3 GEMMs of
                                ViT-g/14, written as the zero-padded A operand pair of w3); a new export with its own tagged argument struct,
                                no existing struct changed.
                                Added within 8: mvp_task_prepare, mvp_masked_l1_fwd_bwd and mvp_task_metrics (Taskonomy probing: raw target and
                                valid mask on the device, masked L1 loss, AbsRel / threshold sums); new exports with their own tagged argument
                                structs, no existing struct changed.
                                Added within 8: mvp_pixel_score and mvp_pixel_score_workspace_bytes (the pixel-level baselines of the 2AFC
                                evaluation: PSNR and SSIM of triplets with the running confusion counts); new exports with their own tagged
                                argument struct, no existing struct changed.
                                Added within 8: mvp_f16_range_scan (one read-only pass over the fp16 hi half of a pair operand into a 16-byte
                                record of maximum / saturated / non-finite / scanned counts: the range guard under MVP_PREC_F16X2); a new export
                                with its own tagged argument struct, no existing struct changed.
                             7: mvp_bn_running_update_n (a new export); mvp_gemm_args.out_f16_col0 < -1 and MVP_ATT_V_F16_QK_F16 (new values of existing fields); every struct as in 6.
                                Later additions within 7 (new exports with their own argument structs; no existing struct changed):
                                mvp_gemm_scaled (LayerScale epilogue), mvp_patch_gather_ld (padded patch rows), mvp_prefix_rows (CLS + register rows);
                                their argument structs are tagged structs (struct X {...}; typedef'd ahead), the ABI 7 set of `} mvp_*;` structs is unchanged
                             6: mvp_gemm_args.out_f16_col0, mvp_attention_args.v_format (both structs grew by one int at the end; zero = the ABI 5 behaviour)
                             5: mvp_upconv3_fwd_gather, mvp_upconv3_grad_boxsum; mvp_gemm_pp accepts conv; depth-loss workspace grew (query mvp_depth_loss_workspace_bytes) */
int mvp_get_info(mvp_info_t* out);
const char* mvp_strerror(int code);
int mvp_sizeof(const char* struct_name); /* sizeof(<struct_name>) as compiled into the library, -1 if unknown: for bindings to self-check */

/* ------------------------------------------------------------------------------------
 * Elementwise split:  fp32 [n] -> bf16 pair.  Used once per frozen-weight tensor.
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const float* src;
  mvp_bf16* hi;
  mvp_bf16* lo; /* may be NULL */
  int64_t n;
} mvp_split_bf16_args;
int mvp_split_bf16(const mvp_split_bf16_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * Patch gather (im2col) for the 16x16/16 patch-embed conv.
 * Replaces the data movement inside nn.Conv2d(3,768,16,16) of
 * evals/models/ibot_transformers.py:216-222 (PatchEmbed.proj) and center_padding
 * (evals/models/utils.py:55-72): zero padding (pad_top/pad_left) is applied on the fly.
 * out row (b*gh*gw + py*gw + px), col (c*P*P + ky*P + kx)  — matches weight.view(768,-1).
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const float* images; /* [B,C,H,W] fp32 NCHW                                  */
  mvp_bf16* out_hi;    /* [B*gh*gw, C*P*P]                                      */
  mvp_bf16* out_lo;    /* or NULL                                              */
  int B, C, H, W;      /* un-padded image dims                                 */
  int P;               /* patch size (16); must be a multiple of 4             */
  int gh, gw;          /* patch grid after padding                             */
  int pad_top, pad_left;
} mvp_patch_gather_args;
int mvp_patch_gather(const mvp_patch_gather_args*, void* stream);
/* The same gather into rows of ldk >= C*P*P elements, columns [C*P*P, ldk) written as zeros, and any P >= 1 (DINOv2: P = 14,
 * C*P*P = 588 padded to ldk = 608 so that the patch-embed GEMM gets K % 32 == 0; its weights are padded with zero columns once). */
typedef struct mvp_patch_gather_ld_args mvp_patch_gather_ld_args;
struct mvp_patch_gather_ld_args {
  mvp_patch_gather_args g;
  int ldk;             /* row stride of out_hi / out_lo, elements; % 4 == 0     */
};
int mvp_patch_gather_ld(const mvp_patch_gather_ld_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * GEMM with fused epilogue:   Y = act(A · Wᵀ + bias) + residual
 *   A  [M, K]  bf16 pair, row stride lda;   W  [N, K]  bf16 pair (torch Linear layout),
 *   row stride ldw;  K % 64 == 0 (K % 32 == 0 in bf16x3 mode, without split-K);  fp32 accumulation on the bf16 MFMA pipe.
 * Replaces nn.Linear / 1x1 conv call sites: ibot_transformers.py:124,143 (qkv, proj),
 * :95-106 (fc1+GELU+fc2), :216-222 (patch-embed as GEMM), probes.py:352-355,420-432.
 * Output rows can be remapped (patch-embed writes token rows behind the CLS slot):
 *   out_row(m) = (m / row_group) * row_group_stride + row_group_off + (m % row_group)
 * when row_group > 0; residual row = m % res_row_mod when res_row_mod > 0 (pos-embed),
 * else the (remapped) output row.
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const mvp_bf16* a_hi; const mvp_bf16* a_lo;
  const mvp_bf16* w_hi; const mvp_bf16* w_lo;
  const float* bias;      /* [N] or NULL                                        */
  const float* residual;  /* fp32, row stride ldr, or NULL                      */
  float* out_f32;         /* row stride ldo, or NULL                            */
  mvp_bf16* out_hi;       /* row stride ldob, or NULL                           */
  mvp_bf16* out_lo;       /* or NULL                                            */
  int M, N, K;
  int lda, ldw, ldr, ldo, ldob;
  int act;                /* MVP_ACT_*                                          */
  int precision;          /* MVP_PREC_*                                         */
  int row_group, row_group_stride, row_group_off, res_row_mod;
  /* --- implicit-GEMM convolution (conv != 0): A = channels-last activation [B, cH>>cup, cW>>cup, cC]
   * read as the im2col of its (nearest-upsampled by 2^cup) [B, cH, cW, cC] view; K = ckh*ckw*cC with
   * k = (ky*ckw + kx)*cC + c (weights laid out [N, ckh, ckw, cC]); M = B*cHo*cWo; cC % 32 == 0.
   * Replaces nn.Conv2d 3x3 / strided convs of probes.py:283-306,318-375 and the ResNet trunk
   * (dino_res50.py:38-51); padding taps are read as out-of-range buffer offsets (zeros); the activation must
   * stay below 2 GiB; zero_page (>= 256 zero bytes) is still validated for ABI stability but no longer read.  */
  int conv, cH, cW, cC, cHo, cWo, ckh, ckw, cstride, cpad, cup;
  const mvp_bf16* zero_page;
  /* --- ReLU bookkeeping (byte masks, row stride ldm):
   * out_mask  (forward): 1 where the activated value (before any residual add) is > 0;
   * relu_mask (backward): gate by a saved mask; mask_mode 2 gates the result before the residual
   * add, mask_mode 1 gates only the bf16-pair output (out_f32 stays un-gated: skip-path gradient). */
  const uint8_t* relu_mask; uint8_t* out_mask; int ldm; int mask_mode;
  const float* residual2; /* optional second fp32 addend, same row stride ldr (fusion-block "+ skip") */
  int act_after_res;      /* 1: apply MVP_ACT_RELU after the residual adds (ResNet bottleneck)          */
  /* --- split-K (splitk > 1, plain linear GEMMs only: ignored with conv / mask / residual2 / act_after_res):
   * the K range is cut into `splitk` parts that run as separate workgroups; the last part to finish sums
   * the fp32 partial tiles in a fixed order (bit-reproducible) and runs the fused epilogue.  For GEMMs
   * with too few output tiles to fill 256 CUs (N = 768 projections, the probe head at M ~ 3k rows).
   * splitk_ws: >= mvp_gemm_splitk_workspace_bytes(M, N, splitk) bytes whose leading tile counters are ZERO
   * at first use (they reset themselves); not shared by GEMMs running concurrently on other streams.
   * splitk 0 or 1: no split; splitk < 0: MVP_EINVAL.                                                                  */
  int splitk; void* splitk_ws; int64_t splitk_ws_bytes;
  /* --- optional residual given as a bf16 pair (row stride ldr, elements), added like `residual`:
   * lets a frozen trunk keep block outputs only as pairs (ResNet identities, dino_res50.py:83-101). */
  const mvp_bf16* residual_hi; const mvp_bf16* residual_lo;
  /* --- tile policy of the plain (non-conv, non-split-K) bf16x3 GEMMs:
   * MVP_TILES_ALONE (0): the launch has the chip to itself (one serial kernel chain): tiles small enough that every CU holds
   *   several workgroups (64x64 for the N = 768 projections at M ~ 3k: 600 tiles on 256 CUs);
   * MVP_TILES_SHARED (1): other kernel chains run beside it on other streams (mvp/pipeline.py keeps >= 3 frozen forwards in
   *   flight): 128x128 tiles everywhere.  They need 31 % less SIMD time per output (an LDS-DMA piece costs its SIMD ~5 MFMAs, and a
   *   128x128 tile issues 6 MFMAs per piece against 3), and the CUs their coarse grid leaves idle are filled by the other chains. */
  int tile_policy;
  /* --- layout of the bf16-pair operands A and W (MVP_PREC_BF16X3 only):
   * MVP_PAIR_SEPARATE (0): a_hi / a_lo and w_hi / w_lo are separate K-contiguous arrays (what every producer of this library writes);
   * MVP_PAIR_A_ILV32 (1) / MVP_PAIR_W_ILV32 (2), or-ed: that operand is ONE array, hi | lo interleaved per 32-deep k block — row =
   *   [k / 32][hi 32 | lo 32] bf16, so a 32-deep k-step of a row is one whole 128-byte line; a_hi (w_hi) points at the array, lda
   *   (ldw) is its row stride in elements (2 * K when dense), a_lo (w_lo) is ignored.  Only the large-M kernel (mvp_gemm_pp) reads
   *   this layout; MVP_PAIR_ILV32 (3) = both operands.                                                                           */
  int pair_layout;
  /* --- layout of the bf16-pair OUTPUT (out_hi / out_lo): MVP_PAIR_SEPARATE, or MVP_PAIR_A_ILV32 (1): out_hi is ONE array
   * [rows][N / 32][hi 32 | lo 32] with row stride ldob (2 * N when dense), out_lo is ignored, N % 32 == 0 — the A operand of a following
   * large-M GEMM (fc1 -> fc2).  Any kernel of mvp_gemm_bias_act_res writes it.                                                        */
  int out_pair_layout;
  /* --- 16-bit forms other than the bf16 pair inside the pair output (ABI 6; MVP_PREC_BF16X3 / F16X2, out_hi and a lo half required).
   * out_f16_col0 = -1: EVERY column is written as the activation pair of MVP_PREC_F16X2 above (fc1 -> fc2).
   * out_f16_col0 > 0 (a multiple of 64): columns >= out_f16_col0 are written as hi = fp16(v) (round to nearest even), lo = bf16(v - hi) instead of
   * hi = bf16(v), lo = bf16(v - hi) — the V third of the fused qkv projection (out_f16_col0 = 2 * H * 64), which the attention
   * kernel multiplies with probabilities held as ONE fp16 value (mvp_attention_args.v_format).  Same 2 + 2 bytes, same arrays and
   * layouts; |v - hi - lo| <= 2^-20 |v|.  Every kernel of mvp_gemm_bias_act_res / mvp_gemm_pp writes it.
   * out_f16_col0 = -V0 < -1 (ABI 7; V0 a multiple of 128 = the first column of the V third, 2 * H * 64): the fused qkv projection for
   * MVP_ATT_V_F16_QK_F16 — columns [0, V0 / 2) (Q) as the compensated activation pair, [V0 / 2, V0) (K) as the compensated WEIGHT-side pair
   * (hi = fp16((1 - 2^-6) v), lo = fp16((v + 64 d) / 8), d = (1 - 2^-6) v - hi, fp32 arithmetic; hi + lo / 8 = v to ~2^-17), [V0, N) (V) as above. */
  int out_f16_col0;
} mvp_gemm_args;
#define MVP_TILES_ALONE 0
#define MVP_TILES_SHARED 1
#define MVP_TILES_NO_PP 2 /* flag, or-ed in: never dispatch to the large-M kernel mvp_gemm_pp (A/B measurements, tests of the tile kernels) */
#define MVP_TILES_NO_UNI 4 /* flag, or-ed in: keep the row-guarded epilogue where the universal branch-free one (gemm_epilogue_uni) would serve (A/B, bit-identity tests) */
#define MVP_PAIR_SEPARATE 0
#define MVP_PAIR_A_ILV32 1
#define MVP_PAIR_W_ILV32 2
#define MVP_PAIR_ILV32 3
int mvp_gemm_bias_act_res(const mvp_gemm_args*, void* stream);
/* The large-M bf16x3 kernel (csrc/gemm_pp.hip): 256x256 output tiles, one 8-wave workgroup per CU, LDS-DMA prefetch kept in flight
 * across raw barriers with counted vmcnt, the two wave groups of a SIMD alternating between MFMA clusters and loads.  Same contract,
 * same epilogue and — same accumulation order — the same bits as the tile kernels; plain linear GEMMs only (no conv, no split-K),
 * K % 32 == 0, K >= 64.  mvp_gemm_bias_act_res dispatches to it by itself when M is large enough (see the rule in gemm.hip);
 * this entry point forces it (benchmarks, tests).  Replaces the same nn.Linear call sites (ibot_transformers.py:95-106,124-145). */
int mvp_gemm_pp(const mvp_gemm_args*, void* stream);
int64_t mvp_gemm_splitk_workspace_bytes(int M, int N, int splits);
/* (ABI 8) Which kernel mvp_gemm_bias_act_res runs for these arguments — the library's one rule, csrc/gemm.hip — and the template
 * arguments of that instantiation.  Host only: touches no device, reads no operand (pointers are only tested for NULL).  Returns what
 * mvp_gemm_bias_act_res would return, MVP_OK or MVP_EINVAL, except that the split-K workspace is not checked.  mvp_gemm_scaled routes
 * its `gemm` part the same way.                                                                                                  */
#define MVP_GEMM_ROUTE_PP 1     /* the large-M kernel (mvp_gemm_pp): bm, bn, bk = 256, 256, 32, and split; nstage, nw, wnw are 0  */
#define MVP_GEMM_ROUTE_TILE 2   /* a tile kernel                                                                                 */
#define MVP_GEMM_ROUTE_SPLITK 3 /* a tile kernel with split-K (splitk > 1)                                                       */
#define MVP_GEMM_ROUTE_CONV 4   /* a tile kernel of the implicit-GEMM convolution (conv != 0)                                    */
typedef struct mvp_gemm_route_t mvp_gemm_route_t;
struct mvp_gemm_route_t {
  int family;           /* MVP_GEMM_ROUTE_*                                                                   */
  int bm, bn, bk;       /* output tile, k-depth of one LDS stage                                              */
  int split;            /* products per contraction: 1 (MVP_PREC_BF16), 3 (MVP_PREC_BF16X3), 2 (MVP_PREC_F16X2) */
  int nstage, nw, wnw;  /* LDS stages, waves per workgroup, waves along N                                     */
};
int mvp_gemm_route(const mvp_gemm_args*, mvp_gemm_route_t* out);
/* LayerScale fused into the epilogue (DINOv2 blocks: x + ls1.gamma * proj(.), x + ls2.gamma * fc2(.)):
 *   Y[m, n] = col_scale[n] * act(A · Wᵀ + bias)[m, n] + residual
 * i.e. the scale is applied after bias and activation, before the residual add.  `gemm` keeps mvp_gemm_bias_act_res's contract and
 * tile / large-M dispatch (both pair layouts, every precision); not supported (MVP_EINVAL): convolutions, split-K, masks,
 * pair residuals, residual2, act_after_res.  The scale is NOT folded into the weights: a tiny gamma (1e-5) would push the fp16 halves
 * of the MVP_PREC_F16X2 weight pairs into subnormals.  col_scale: [N] fp32, 16-byte aligned.                                       */
typedef struct mvp_gemm_scaled_args mvp_gemm_scaled_args;
struct mvp_gemm_scaled_args {
  mvp_gemm_args gemm;
  const float* col_scale;
};
int mvp_gemm_scaled(const mvp_gemm_scaled_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * LayerNorm forward: fp32 rows [M, C] -> bf16 pair [M, C] (the next GEMM's A operand).
 * Replaces nn.LayerNorm(eps=1e-6) at ibot_transformers.py:164,174,194,199 (eps 1e-12 for
 * the HF ViT-MAE path, evals/models/mae.py:33).  One wave64 per row, two-pass in registers.
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const float* x; const float* gamma; const float* beta;
  mvp_bf16* out_hi; mvp_bf16* out_lo; /* lo may be NULL; out_hi may be NULL when out_f32 is set (no pair output); both NULL: MVP_EINVAL */
  float* out_f32;                     /* optional fp32 copy, or NULL.  out_f32 == x is allowed (in place: a row is read whole before it is written) */
  int M, C;                           /* C % 8 == 0, C <= 2048 */
  float eps;
  int out_layout;                     /* MVP_PAIR_SEPARATE, or MVP_PAIR_A_ILV32 (1): out_hi is ONE [M][C / 32][hi 32 | lo 32] array (row stride
                                         2 * C), out_lo ignored, C % 32 == 0 — the A operand of the large-M GEMM (mvp_gemm_args.pair_layout) */
  int out_f16;                        /* (ABI 6) 1: the pair is written as the activation operand of MVP_PREC_F16X2 (hi = fp16(y), lo = fp16(8 (y - hi) + hi / 8)) */
} mvp_layernorm_args;
int mvp_layernorm_fwd(const mvp_layernorm_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * Multi-head self-attention forward, flash-style (no N x N materialisation):
 *   O = softmax(Q Kᵀ * scale) V   per (batch, head), head_dim = 64.
 * qkv is the fused projection output [B*N, 3*H*64] (bf16 pair) laid out as the reference
 * reshapes it: col = which*H*64 + head*64 + d  (ibot_transformers.py:129-142).
 * out [B*N, H*64] bf16 pair = (attn @ v).transpose(1,2).reshape(B,N,C)  (:142).
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const mvp_bf16* qkv_hi; const mvp_bf16* qkv_lo;
  mvp_bf16* out_hi; mvp_bf16* out_lo;
  int B, N, H;      /* tokens per image N (incl. CLS), heads H; head_dim fixed 64 */
  int ld_qkv, ld_out;
  float scale;      /* head_dim^-0.5 */
  int precision;
  int out_layout;   /* MVP_PAIR_SEPARATE, or MVP_PAIR_A_ILV32 (1): out_hi is ONE [B*N][H*2][hi 32 | lo 32] array with row stride ld_out
                       (>= 2 * H * 64), out_lo ignored — the A operand of the large-M proj GEMM (mvp_gemm_args.pair_layout)               */
  int v_format;     /* MVP_PREC_BF16X3 only.  MVP_ATT_V_BF16_PAIR (0): V is a bf16 pair like Q and K; the probabilities are split into a bf16
                       pair too and P.V runs three products (hi.hi + hi.lo + lo.hi).  MVP_ATT_V_F16 (1, ABI 6): the V third of qkv holds
                       hi = fp16(v), lo = bf16(v - hi) (mvp_gemm_args.out_f16_col0); the probabilities are held as ONE fp16 value
                       (+ its bf16 rounding for the lo product): P.V = v_hi.p on the f16 MFMA + v_lo.p on the bf16 MFMA — two products
                       instead of three and no hi / lo split of P on the vector pipe (the kernel is VALU-bound); the online softmax
                       rescales its running maximum only when it rises by more than 2^6.  Q.K^T keeps its three products either way.
                       Relative error of the output: ~2^-12 per probability (random, averaged over the keys) instead of 2^-17.        */
  int out_f16;      /* (ABI 6) 1: the output pair is written as the activation operand of a MVP_PREC_F16X2 proj GEMM (hi = fp16(o), lo = fp16(8 (o - hi) + hi / 8)) */
} mvp_attention_args;
#define MVP_ATT_V_BF16_PAIR 0
#define MVP_ATT_V_F16 1
#define MVP_ATT_V_F16_QK_F16 2 /* ABI 7.  V and the probabilities as MVP_ATT_V_F16; Q is the compensated ACTIVATION pair and K the compensated WEIGHT-side
                                  pair of MVP_PREC_F16X2 (mvp_gemm_args.out_f16_col0 = -(first column of the V third)): Q.K^T as two f16 products instead of
                                  three bf16 ones, same ~2^-18 relative error per term; Q and K must stay within fp16's range (saturating) */
int mvp_attention_fwd(const mvp_attention_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * (added within ABI 8; a new export with its own tagged argument struct, no existing struct changed.)
 * Attention with a dense per-head additive bias on the logits (BEiT's relative-position bias; the base of SAM's):
 *   O = softmax(Q K^T * att.scale + bias[h]) V
 * Everything else as mvp_attention_fwd (same kernels, same operand forms, same N <= 256 resident / streaming split).
 * bias is fp32 [H][N][ld_bias], bias[h][q][k], the same for every image of the batch, in natural-log units, finite, of any sign and
 * magnitude.  Columns k >= N of a row (up to 64 * ceil(N / 64)) may be read; they may hold anything, NaN included, and never reach
 * the output.  No row q >= N and no head >= H is read.
 * MVP_EINVAL: everything mvp_attention_fwd rejects; bias NULL or not 16-byte aligned; ld_bias % 4 != 0 or
 * ld_bias < 64 * ceil(N / 64); bias_head_stride < N * ld_bias or bias_head_stride % 4 != 0 (every row starts 16-byte aligned).
 * ---------------------------------------------------------------------------------- */
typedef struct mvp_attention_bias_args mvp_attention_bias_args;
struct mvp_attention_bias_args {
  mvp_attention_args att;      /* everything as mvp_attention_fwd */
  const float* bias;           /* fp32 [H][N][ld_bias]: bias[h][q][k], the same for every image of the batch */
  int64_t bias_head_stride;    /* elements; >= N * ld_bias, % 4 == 0 */
  int ld_bias;                 /* elements; % 4 == 0 and >= 64 * ceil(N / 64) */
};
int mvp_attention_bias_fwd(const mvp_attention_bias_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * (added within ABI 8; a new export with its own tagged argument struct, no existing struct changed.)
 * 2-D rotary position embedding of the fused qkv projection: CroCo v2's RoPE100, the reference's RoPE2D.forward
 * (evals/models/croco_models/pos_embed.py:110-157) applied to q and k in Attention.forward (croco_models/blocks.py:94-103).
 * Sits between the qkv GEMM and mvp_attention_fwd: reads the projection as fp32 [M, ld_in] (the GEMM's out_f32 form), rotates the Q and K
 * thirds, passes V through, and writes the pair buffer mvp_attention_fwd reads — every third in exactly the 16-bit form the qkv GEMM's
 * epilogue writes for the same (precision, v_format) (mvp_gemm_args.out_f16_col0 = 0 / 2*H*64 / -2*H*64 for v_format 0 / 1 / 2;
 * one definition of each form, shared with the epilogues: <= 2^-17 relative each).
 * Per head, dims 0..31 take the token's y coordinate and dims 32..63 its x coordinate; within a 32-wide half, with
 * c = cos_tab[pos][d], s = sin_tab[pos][d]:
 *     d <  16:  out[d] = t[d] * c - t[d + 16] * s
 *     d >= 16:  out[d] = t[d] * c + t[d - 16] * s
 * in fp32 as SEPARATE multiplies and one add / subtract (never contracted into an fma): torch's (t * cos) + (rotate_half(t) * sin),
 * bit for bit.  Positions come from the row index alone: token t = m % N; t < n_prefix is not rotated; else p = t - n_prefix,
 * y = p / gw, x = p % gw.  Stateless, no workspace, no sync.
 * MVP_EINVAL: NULL pointers (out_lo may be NULL under MVP_PREC_BF16 only, and is then not written), M % N != 0,
 * N != n_prefix + gh * gw, tab_rows < max(gh, gw), ld_in or ld_out < 3 * H * 64, rows not 16-byte aligned (pointers % 16, ld_in % 4,
 * ld_out % 8), a precision other than MVP_PREC_BF16 / MVP_PREC_BF16X3, a v_format other than 0 under a precision other than MVP_PREC_BF16X3,
 * M * 24 * H >= 2^31 (one thread per 8 values, indexed in 32 bits).
 * ---------------------------------------------------------------------------------- */
typedef struct mvp_rope2d_qkv_args mvp_rope2d_qkv_args;
struct mvp_rope2d_qkv_args {
  const float* qkv;            /* [M, ld_in] fp32, col = which*H*64 + head*64 + d                   */
  mvp_bf16* out_hi; mvp_bf16* out_lo;  /* [M, ld_out] pair, MVP_PAIR_SEPARATE                       */
  const float* cos_tab; const float* sin_tab;  /* [tab_rows, 32] fp32, row = grid coordinate        */
  int M, N, H;                 /* rows, tokens per image, heads; M % N == 0                         */
  int n_prefix, gh, gw;        /* N == n_prefix + gh*gw                                             */
  int tab_rows;                /* >= max(gh, gw), checked on the host                               */
  int ld_in, ld_out;
  int precision, v_format;     /* as mvp_attention_args: which 16-bit form each third gets          */
};
int mvp_rope2d_qkv(const mvp_rope2d_qkv_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * (added within ABI 8; a new export with its own tagged argument struct, no existing struct changed.)
 * Row gather of a 16-bit pair buffer by an int32 index table (SAM's window partition and un-partition):
 *     out[r][0 .. cols) = idx[r] >= 0 ? in[idx[r]][0 .. cols) : 0          r in [0, rows)
 * a pure copy, bit for bit, of ``cols`` 16-bit elements per row of in_hi -> out_hi and (when both are given) in_lo -> out_lo.  An
 * interleaved pair (MVP_PAIR_A_ILV32: ONE array of 2 C elements per row) is gathered as in_hi / out_hi with cols = 2 C and in_lo =
 * out_lo = NULL.  An index >= rows_in gives a zero row too (no row beyond the input is ever read).  in and out must not overlap.
 * MVP_EINVAL: NULL in_hi / out_hi / idx, in_lo without out_lo or the reverse, rows <= 0, rows_in <= 0, cols <= 0 or cols % 8 != 0,
 * ld_in or ld_out < cols or % 8 != 0, a pointer not 16-byte aligned (idx: 4-byte), rows * (cols / 8) >= 2^31.
 * ---------------------------------------------------------------------------------- */
typedef struct mvp_gather_rows_args mvp_gather_rows_args;
struct mvp_gather_rows_args {
  const mvp_bf16* in_hi; const mvp_bf16* in_lo;   /* [rows_in, ld_in]; in_lo may be NULL (then out_lo must be NULL) */
  mvp_bf16* out_hi; mvp_bf16* out_lo;             /* [rows, ld_out]                                                  */
  const int* idx;                                 /* [rows] int32: source row, < 0 = zero row                        */
  int rows, rows_in, cols;                        /* cols: 16-bit elements copied per row, % 8 == 0                  */
  int ld_in, ld_out;                              /* elements, % 8 == 0, >= cols                                     */
};
int mvp_gather_rows(const mvp_gather_rows_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * (added within ABI 8; a new export with its own tagged argument struct, no existing struct changed.)
 * SAM's decomposed relative-position terms (segment_anything's add_decomposed_rel_pos) of the UNSCALED q, in natural-log units.
 * Sits between the qkv GEMM and mvp_attention_relpos_fwd, like mvp_rope2d_qkv: reads the projection as fp32 [M, ld_in] (the GEMM's
 * out_f32 form), and writes
 *   (1) rel[(b * H + h) * rel_bh_stride + q * ld_rel + j], b = m / N, q = m % N, (yq, xq) = (q / Qw, q % Qw):
 *         j in [0, Kh):        sum_d q[b, h, q, d] * rh[yq][j][d]
 *         j in [Kh, Kh + Kw):  sum_d q[b, h, q, d] * rw[xq][j - Kh][d]
 *       accumulated in fp32 with fma, d = 0 .. 63 in order; columns j >= Kh + Kw of a row are not written;
 *   (2) the pair buffer the attention kernels read: every third of the projection in exactly the 16-bit form the qkv GEMM's epilogue
 *       writes for the same (precision, v_format), as mvp_rope2d_qkv does (Q, K and V all pass through unchanged).
 * rh is fp32 [Qh][Kh][64], rw fp32 [Qw][Kw][64]; both are shared by all heads and images.
 * MVP_EINVAL: NULL pointers (out_lo may be NULL under MVP_PREC_BF16 only), M % N != 0, Qh * Qw != N, Kh or Kw <= 0,
 * ld_rel < Kh + Kw or ld_rel % 4 != 0, rel_bh_stride < N * ld_rel, ld_in or ld_out < 3 * H * 64, rows not 16-byte aligned (pointers % 16,
 * ld_in % 4, ld_out % 8), H > 256 (the Q row of a token is held in LDS: H * 256 bytes), precision / v_format as mvp_rope2d_qkv.
 * ---------------------------------------------------------------------------------- */
typedef struct mvp_relpos_terms_args mvp_relpos_terms_args;
struct mvp_relpos_terms_args {
  const float* qkv;            /* [M, ld_in] fp32, col = which*H*64 + head*64 + d                   */
  mvp_bf16* out_hi; mvp_bf16* out_lo;  /* [M, ld_out] pair, MVP_PAIR_SEPARATE                       */
  float* rel;                  /* [B*H][N][ld_rel] fp32                                             */
  const float* rh; const float* rw;    /* [Qh][Kh][64], [Qw][Kw][64] fp32                           */
  int64_t rel_bh_stride;       /* elements; >= N * ld_rel                                           */
  int M, N, H;                 /* rows, tokens per image (window), heads; M % N == 0                */
  int Qh, Qw, Kh, Kw;          /* query grid (Qh * Qw == N) and key grid                            */
  int ld_in, ld_out, ld_rel;
  int precision, v_format;     /* as mvp_attention_args: which 16-bit form each third gets          */
};
int mvp_relpos_terms(const mvp_relpos_terms_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * (added within ABI 8; a new export with its own tagged argument struct, no existing struct changed.)
 * Attention with a decomposed relative-position bias on the logits (SAM's image encoder):
 *   O = softmax(Q K^T * att.scale + rel[bh][q][k / Kw] + rel[bh][q][Kh + k % Kw]) V,       bh = b * H + h, N == Kh * Kw
 * with rel as mvp_relpos_terms writes it (fp32, natural-log units, finite).  The bias differs per image, head and query, so no [N, N]
 * array of it exists anywhere: a query row's Kh + Kw values are read as they are needed.  Everything else as mvp_attention_fwd (same
 * kernels, same operand forms, same N <= 256 resident / streaming split).  Only columns [0, Kh + Kw) of rows q < N of pairs
 * bh < B * H are read.
 * MVP_EINVAL: everything mvp_attention_fwd rejects; rel NULL or not 4-byte aligned; Kh or Kw <= 0 or Kh * Kw != N;
 * ld_rel < Kh + Kw; rel_bh_stride < N * ld_rel; N * ld_rel >= 2^30 (a row's byte offset inside a pair is a 32-bit lane offset).
 * ---------------------------------------------------------------------------------- */
typedef struct mvp_attention_relpos_args mvp_attention_relpos_args;
struct mvp_attention_relpos_args {
  mvp_attention_args att;      /* everything as mvp_attention_fwd */
  const float* rel;            /* fp32 [B*H][N][ld_rel] */
  int64_t rel_bh_stride;       /* elements; >= N * ld_rel */
  int ld_rel;                  /* elements; >= Kh + Kw */
  int Kh, Kw;                  /* key grid; Kh * Kw == N */
};
int mvp_attention_relpos_fwd(const mvp_attention_relpos_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * CLS row writer: x[b, 0, :] = cls[:] + pos[0, :]   (ibot_transformers.py:347-352).
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const float* cls; const float* pos0; float* x; int B, N, C;
} mvp_cls_rows_args;
int mvp_cls_rows(const mvp_cls_rows_args*, void* stream);
/* Prefix rows of every image in one launch: x[b, 0, :] = cls + pos0, x[b, 1 + r, :] = reg[r, :] for r < R (DINOv2 register tokens:
 * no position embedding).  R = 0 is mvp_cls_rows.  The patch rows follow at 1 + R (patch-embed GEMM: row_group_off = 1 + R). */
typedef struct mvp_prefix_rows_args mvp_prefix_rows_args;
struct mvp_prefix_rows_args {
  const float* cls; const float* pos0; const float* reg; float* x; int B, N, C, R;
};
int mvp_prefix_rows(const mvp_prefix_rows_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * Tap BatchNorm over tokens (train-mode batch statistics, CLS included) fused with the
 * token -> NCHW dense-map transpose.  Replaces nn.BatchNorm1d on x.permute(0,2,1)
 * (evals/models/dino.py:185-191) + tokens_to_output("dense") (evals/models/utils.py:111-114).
 *   stats pass : per-channel mean / biased var over all B*N rows -> stats[2*C] (mean, var),
 *                running stats updated with momentum & unbiased var when running_* != NULL (unless defer_running);
 *   apply pass : y = (x - mean) * rsqrt(var + eps) * gamma + beta, spatial tokens only
 *                (the last hw tokens of each image), written as
 *                  nchw   [B, C, h, w] fp32          (the reference's return value)
 *                  tok_hi/lo [B*hw (ld_tok)] bf16 pair at column offset col_off
 *                           (token-major operand of the probe-head GEMM; optional)
 *                  tokT_hi/lo [C rows at row offset col_off][ldT] bf16 pair
 *                           (transposed copy, operand of the head's dW GEMM; optional)
 * mode: 0 = train (batch stats), 1 = eval (use running stats), 2 = no norm (identity).
 * workspace: ws_bytes = mvp_bn_tokens_workspace_bytes(M, C) (fp32 partials).
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const float* x;       /* [B, N, C] fp32 token stream                           */
  const float* gamma; const float* beta; /* [C] or NULL (identity)               */
  float* running_mean; float* running_var; /* [C] or NULL                        */
  float* stats;         /* [2*C] out: batch mean, biased var                      */
  float* nchw;          /* [B, C, hw] or NULL                                     */
  mvp_bf16* tok_hi; mvp_bf16* tok_lo; int ld_tok; int col_off;
  mvp_bf16* tokT_hi; mvp_bf16* tokT_lo; int ldT;
  void* workspace; int64_t workspace_bytes;
  int B, N, C, hw;      /* hw = spatial tokens per image (N - hw leading tokens dropped) */
  float eps, momentum;
  int mode;
  float* cls_out;       /* [B, C] fp32 or NULL: the normalised FIRST token of each image (the CLS token that
                           tokens_to_output(output="cls" / "dense-cls") returns, utils.py:105-124); needs N > hw */
  int64_t* num_batches_tracked; /* or NULL: BatchNorm's step counter, incremented in train mode (mode 0) by the statistics kernel */
  int defer_running;    /* 1 (mode 0 only): leave running_mean / running_var / num_batches_tracked untouched and write the unbiased
                           variance to stats[2*C .. 3*C) (stats then holds 3*C floats); mvp_bn_running_update applies the update later.
                           For forwards that run concurrently on several streams (mvp/pipeline.py): the running statistics are the only
                           state a frozen forward mutates, and their momentum updates must happen in batch order.                     */
  /* --- several batches in one launch (groups = G > 1; mvp/pipeline.py stacks G equal batches into one frozen forward): x holds
   * G * B images; statistics, normalisation and outputs are those of each batch of B images ALONE (train-mode BatchNorm is per batch,
   * dino.py:185-191) — the same bits as G separate calls.  Group g reads x + g * B*N*C and writes stats + g * stats_gstride,
   * nchw + g * nchw_gstride, tok_* + g * tok_gstride, cls_out + g * cls_gstride (strides in elements).  Train mode needs
   * defer_running = 1 (the running statistics are then updated per batch by mvp_bn_running_update, in batch order); tokT_* is not
   * supported; workspace_bytes >= G * mvp_bn_tokens_workspace_bytes(B * N, C).  groups <= 1: one batch, the strides are ignored.     */
  int groups;
  int64_t stats_gstride, nchw_gstride, tok_gstride, cls_gstride;
} mvp_bn_tokens_args;
int64_t mvp_bn_tokens_workspace_bytes(int M, int C);
int mvp_bn_tokens_to_nchw_fwd(const mvp_bn_tokens_args*, void* stream);

/* The deferred half of nn.BatchNorm's train-mode bookkeeping (torch/nn/modules/batchnorm.py; dino.py:185-191 keeps the tap BNs in
 * train mode): running = (1 - momentum) * running + momentum * batch statistic (unbiased variance), num_batches_tracked += 1.
 * Same arithmetic, bit for bit, as the in-kernel update of mvp_bn_tokens_to_nchw_fwd with defer_running = 0. */
typedef struct {
  const float* stats;   /* [3*C]: mean, biased var, unbiased var — as written with defer_running = 1 */
  float* running_mean; float* running_var;  /* [C] */
  int64_t* num_batches_tracked;             /* or NULL */
  int C; float momentum;
} mvp_bn_running_update_args;
int mvp_bn_running_update(const mvp_bn_running_update_args*, void* stream);
/* The same update for n (1..MVP_BN_RUNNING_MAX) BatchNorm modules in ONE launch — the four tap BNs of a multilayer extract
 * (dino.py:185-191) are handed to the trainer together, and beside a frozen forward every launch of the probe step's stream costs
 * its queueing delay, not its 2 us of work.  Element-wise identical to n calls of mvp_bn_running_update. */
#define MVP_BN_RUNNING_MAX 8
int mvp_bn_running_update_n(const mvp_bn_running_update_args* items, int n, void* stream);

/* ------------------------------------------------------------------------------------
 * NCHW fp32 feature maps -> token-major bf16 pair (+ transposed copy).  Fallback packer
 * used when the probe is handed plain NCHW tensors (e.g. features loaded from disk).
 * Replaces torch.cat(feats, dim=1) of probes.py:427-429 as an operand-layout change.
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const float* nchw;    /* [B, C, hw]                                             */
  mvp_bf16* tok_hi; mvp_bf16* tok_lo; int ld_tok; int col_off;
  mvp_bf16* tokT_hi; mvp_bf16* tokT_lo; int ldT;
  int B, C, hw;
} mvp_pack_nchw_args;
int mvp_pack_nchw_tokens(const mvp_pack_nchw_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * Bilinear / bicubic / nearest resampling of NCHW-like planes, forward and adjoint.
 * Replaces F.interpolate(..., mode=..., align_corners=False|True) at
 * train_depth.py:114 (bilinear), train_snorm.py:110 (bicubic), probes.py:255-258,388,396-398.
 * Coordinates follow ATen's area_pixel_compute_source_index; bicubic uses A = -0.75 with
 * clamped taps.  planes = B*C.  bwd computes grad_in[planes, Hi, Wi] (gather form, no atomics).
 * channels_last = 1 treats the tensor as [B, H, W, C] (token-major logits), planes = B.
 * ---------------------------------------------------------------------------------- */
#define MVP_RESIZE_NEAREST 0
#define MVP_RESIZE_BILINEAR 1
#define MVP_RESIZE_BICUBIC 2
typedef struct {
  const float* src; float* dst;
  int planes, Hi, Wi, Ho, Wo;
  int mode; int align_corners; /* align_corners belongs to bilinear / bicubic.  Callers pass 0 with MVP_RESIZE_NEAREST: torch has no such
                                * form (F.interpolate raises ValueError, and so does mvp.functional.interpolate); a kernel given 1 would
                                * take (in - 1) / (out - 1) as the nearest scale, which matches nothing in torch. */
  int channels_last; int C; /* C used only when channels_last */
  float scale_h, scale_w;   /* >0: the scale_factor given by the caller (recompute_scale_factor=False semantics); 0: derive from sizes */
} mvp_resize_args;
int mvp_resize_fwd(const mvp_resize_args*, void* stream);
int mvp_resize_bwd(const mvp_resize_args*, void* stream); /* src = grad_out [.,Ho,Wo], dst = grad_in [.,Hi,Wi] */
/* Antialiased bilinear, forward only, planar, align_corners = 0, sizes given (torchvision transforms.Resize on a tensor =
 * interpolate(bilinear, antialias=True), dino_res50.py:80,85 for inputs larger than fixed_size on an axis). */
int mvp_resize_aa_fwd(const mvp_resize_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * Depth predictors on token-major logits [P, K] (P = B*H*W pixels, K channels contiguous).
 *   bins   : p = relu(l) + 0.1; p /= sum(p); depth = sum_k p_k * linspace(min,max,K)[k]
 *            (probes.py:176-200);  saves inv_sum[P] for the backward.
 *   sigmoid: depth = min + sigmoid(l) * (max - min)          (probes.py:209-212), K == 1.
 * bwd: grad_logits[P,K] from grad_depth[P].
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const float* logits; float* depth; float* inv_sum;
  const float* grad_depth; float* grad_logits;
  int64_t P; int K;
  float min_depth, max_depth;
  int kind; /* 0 = bins, 1 = sigmoid */
} mvp_depth_predict_args;
int mvp_depth_predict_fwd(const mvp_depth_predict_args*, void* stream);
int mvp_depth_predict_bwd(const mvp_depth_predict_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * DepthLoss = 10 * sig_loss + 0.5 * gradient_loss  (evals/utils/losses.py:97-154),
 * including the reference's quirks: target > max_depth is zeroed IN PLACE (Q2) and the
 * "gradient" term differences samples b and b+2 over batch strides {1,2,4,6} (Q1).
 * pred/target [B, HW] fp32.  Outputs: loss[0] (total), loss[1] sig, loss[2] grad term;
 * grad_pred [B, HW] = d loss / d pred (already scaled by the 10 / 0.5 weights).
 * workspace >= mvp_depth_loss_workspace_bytes(B, HW) bytes, zero-initialised by the op.
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const float* pred; float* target; float* loss; float* grad_pred;
  void* workspace; int64_t workspace_bytes;
  int B; int64_t HW;
  float w_sig, w_grad, max_depth, eps, sigma;
} mvp_depth_loss_args;
int64_t mvp_depth_loss_workspace_bytes(int B, int64_t HW);
int mvp_depth_loss_fwd_bwd(const mvp_depth_loss_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * angular_loss (evals/utils/losses.py:157-182), optional uncertainty-aware (4-channel).
 * pred [B, Cp, HW], gt [B, 3, HW], mask [B, HW] (uint8, non-zero = valid).
 * loss[0] = masked mean; grad_pred = d loss / d pred.
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const float* pred; const float* gt; const uint8_t* mask;
  float* loss; float* grad_pred;
  void* workspace; int64_t workspace_bytes; /* >= 4096 bytes */
  int B; int Cp; int64_t HW;
  float eps;
} mvp_angular_loss_args;
int mvp_angular_loss_fwd_bwd(const mvp_angular_loss_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * Column sums of a fp32 matrix [M, N] -> out[N] (bias gradients), deterministic two-level sum.
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const float* x; float* out; int M, N, ld;
  int accumulate;                       /* 1: out += column sums (gradient accumulation) */
  void* workspace; int64_t workspace_bytes; /* >= mvp_colsum_workspace_bytes(M, N)       */
} mvp_colsum_args;
int64_t mvp_colsum_workspace_bytes(int M, int N);
int mvp_colsum(const mvp_colsum_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * Fused AdamW over a flat fp32 parameter buffer (torch.optim.AdamW defaults,
 * train_depth.py:624-627): decoupled weight decay, bias correction, eps outside sqrt.
 * Schedule state: hyper == NULL -> lr, bias_c1 = 1 - beta1^t, bias_c2 = 1 - beta2^t are taken BY VALUE from the
 * struct (no host->device staging that a host running ahead of the stream could overwrite);
 * hyper != NULL -> device scalars hyper[0..2] = {lr, bias_c1, bias_c2} (replay of a captured hipGraph).
 * grad_scale multiplies the gradient first (1/world_size after an all-reduce SUM).
 * ---------------------------------------------------------------------------------- */
typedef struct {
  float* param; const float* grad; float* exp_avg; float* exp_avg_sq;
  const float* hyper; int64_t n;
  float beta1, beta2, eps, weight_decay, grad_scale;
  float lr, bias_c1, bias_c2;
} mvp_adamw_args;
int mvp_adamw_step(const mvp_adamw_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * SPair correspondence core (evaluate_spair_correspondence.py:59-83 + argmax_2d,
 * evals/utils/correspondence.py:179-190): L2-normalise features over C, bilinearly sample
 * the source map at K keypoints (grid_sample align_corners=True), cosine heat-map against
 * the target map, 2-D argmax.  out_xy [K,2] int64 = (col,row), out_val [K] fp32.
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const float* src_feat; const float* tgt_feat; /* [C, h, w] fp32 each            */
  const float* kp_xy;                            /* [K,2] normalised coords in [-1,1] (x,y) */
  int64_t* out_xy; float* out_val;
  float* workspace; int64_t workspace_bytes;    /* >= mvp_corr_workspace_bytes(C, h, w, K), 8-byte aligned */
  int C, h, w, K;
  float* heat_out;                               /* optional [K, h, w]: the cosine heat-maps (compute_errors(return_heatmaps=True)) */
} mvp_corr_argmax_args;
int64_t mvp_corr_workspace_bytes(int C, int h, int w, int K);
int mvp_corr_argmax(const mvp_corr_argmax_args*, void* stream);
/* argmax_2d (evals/utils/correspondence.py:179-190) on materialised maps x [K, h, w] fp32: out_xy [K,2] int64 = (col,row) of
 * the flat argmax (max_value != 0) or argmin (max_value == 0); ties -> lowest flat index, as torch. */
typedef struct {
  const float* x; int64_t* out_xy; int K, h, w, max_value;
} mvp_argmax_2d_args;
int mvp_argmax_2d(const mvp_argmax_2d_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * (added within ABI 8; a new export with its own tagged argument struct, no existing struct changed.)
 * Top-2 cosine nearest neighbours with the ratio test: the hot loop of the NAVI / ScanNet 3-D correspondence evaluation
 * (evals/utils/correspondence.py:26-121, where faiss does the search).  Definition, per query i with src_valid[i] != 0:
 *     q^ = q / max(|q|, 1e-12),  t^_j likewise (F.normalize),  d(i, j) = 1 - <q^_i, t^_j>   over the targets with tgt_valid[j] != 0
 *     nn_idx[i] = argmin_j d(i, j)  (GRID index j, lowest j among ties),  dist[i] = the two smallest d, ascending
 *     weight[i] = 1 - max(dist[i][0], 1e-9) / max(dist[i][1], 1e-9)          (calculate_ratio_test, both clamps)
 * An invalid query, and every query when fewer than two targets are valid, gets nn_idx = -1, weight = -inf, dist = +inf.
 * n_valid = {number of valid queries, number of valid targets}.
 * How: both views are normalised and packed once (fp32 rows for the exact step, compensated fp16 pairs of MVP_PREC_F16X2 for the
 * matrix pipe, C zero-padded to a multiple of 32); an MFMA kernel keeps, per query, the best 4 targets of each slice of the target
 * range in registers (the N0 x N1 score matrix is never written); a last kernel merges the slices, recomputes the 4 survivors'
 * distances in fp32 from the fp32 rows and orders them.  Every merge orders by (score, index), so the result does not depend on
 * the slicing and two calls give the same bits.  No atomics, no sync, no allocation.
 * MVP_EINVAL: a NULL pointer other than src_valid / tgt_valid, C <= 0 or C > 16384, N0 <= 0, N1 < 2, N0 or N1 > 2^24,
 * workspace_bytes < mvp_knn_workspace_bytes(C, N0, N1), a workspace that is not 16-byte aligned.
 * ---------------------------------------------------------------------------------- */
typedef struct mvp_knn_ratio_args mvp_knn_ratio_args;
struct mvp_knn_ratio_args {
  const float* src_feat; const float* tgt_feat;       /* fp32, channel-major [C, N0] / [C, N1] (a [C, h, w] map, flattened)   */
  const uint8_t* src_valid; const uint8_t* tgt_valid; /* optional [N0] / [N1], non-zero = valid; NULL = all valid             */
  int32_t* nn_idx;                                    /* [N0]   index into the target grid, -1 for an invalid query           */
  float* dist;                                        /* [N0,2] the two smallest cosine distances, ascending                  */
  float* weight;                                      /* [N0]   ratio-test weight, -inf for an invalid query                  */
  int32_t* n_valid;                                   /* [2]    device counts of valid queries / targets                      */
  void* workspace; int64_t workspace_bytes;           /* >= mvp_knn_workspace_bytes(C, N0, N1), 16-byte aligned               */
  int C, N0, N1;
};
/* Workspace: (N0 + N1) * Cpad * 8 + S * N0 * 32 bytes, Cpad = C rounded up to 32 (fp32 rows and the fp16 pair of both views, then 4
 * candidates of 8 bytes per query and target slice); S = ceil(T / ceil(T / min(T, ceil(512 / ceil(N0 / 128))))) slices of the
 * T = ceil(N1 / 128) target tiles.  0 for sizes that mvp_knn_ratio rejects. */
int64_t mvp_knn_workspace_bytes(int C, int N0, int N1);
int mvp_knn_ratio(const mvp_knn_ratio_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * (added within ABI 8; a new export with its own tagged argument struct, no existing struct changed.)
 * Dense features sampled at the projections of a point cloud: the depth path in front of mvp_knn_ratio in the ScanNet pair
 * correspondence evaluation (evals/utils/correspondence.py:164-176, sample_pointcloud_features = projection by K, then
 * grid_sample(mode="bilinear", padding_mode="zeros", align_corners=False)).  Definition, per point p = pc[n]:
 *     uvd = K p,   u = uvd.x / max(uvd.z, 1e-9),   v = uvd.y / max(uvd.z, 1e-9)
 *     x = u * fw / W - 0.5,   y = v * fh / H - 0.5          (= ((2 u / W - 1) + 1) * fw / 2 - 0.5)
 *     out[c, n] = sum over the 4 corners (floor / floor + 1 of x and y) of w_corner * feat[c, yc, xc]
 * A corner outside [0, fw - 1] x [0, fh - 1] contributes 0 (its texel is not used, whatever it holds).  A point whose x or y is not
 * finite or lies outside (-1, fw) x (-1, fh) gives exactly 0.0f in every channel; that is decided on the floats, before any
 * conversion to int (z = 0 and z < 0 reach u ~ 1e9 x through the clamp; a NaN coordinate reaches both u and v).  The point 0 itself, which
 * a depth hole back-projects to, has u = v = 0 and so samples the corner texel at a quarter weight, as grid_sample does: mask by valid.
 * out is channel-major with column n = point n, the layout mvp_knn_ratio reads; columns N..ld_out-1 are never written.
 * valid[n] (optional) = pc[n].z > 0, the reference's test for a real point.
 * One launch: lanes along the points, corner offsets and weights once per point, the grid cut over chunks of 16 channels.
 * No atomics, no sync, no allocation, no workspace; two calls give the same bits.
 * MVP_EINVAL: a NULL pointer other than valid, a size <= 0, ld_out < N, N > 2^24.
 * ---------------------------------------------------------------------------------- */
typedef struct mvp_pointcloud_sample_args mvp_pointcloud_sample_args;
struct mvp_pointcloud_sample_args {
  const float* feat;  /* [C, fh, fw] fp32                                                    */
  const float* pc;    /* [N, 3] fp32 camera-frame points                                     */
  const float* K;     /* [3, 3] fp32 intrinsics ON THE DEVICE (row-major)                    */
  float* out;         /* [C, ld_out] fp32                                                    */
  uint8_t* valid;     /* optional [N]: 1 where pc[n].z > 0; NULL = not wanted                */
  int C, fh, fw, N;
  int H, W;           /* the image (depth grid) size K projects into                         */
  int ld_out;         /* >= N                                                                */
};
int mvp_pointcloud_sample(const mvp_pointcloud_sample_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * (added within ABI 8; new exports with their own tagged argument structs, no existing struct changed.)
 * The tail of the objectness probe (evals/models/probes.py:7-43 BinaryHead / TaskonomyHead, train_generic_objectness.py).
 *
 * mvp_bn_act_fwd / mvp_bn_act_bwd: nn.BatchNorm2d(C) followed by an activation, on the head's channels-last logits.
 *   x [P, ld] fp32, P = B * HW rows, channel c in column c, 1 <= C <= MVP_BN_ACT_MAX_C, ld >= C; columns C..ld-1 never enter a result.
 *   y [B, C, HW] fp32 (the NCHW tensor the caller resizes).
 *   act MVP_BN_ACT_SIGMOID: z = (x - mean) * rstd * gamma + beta, y = sigmoid(z), rstd = 1 / sqrt(var + eps).
 *       training != 0: mean and BIASED variance of the P rows; running_mean / running_var (both or neither; NULL = not tracked)
 *       move by `momentum`, running_var towards var * n / (n - 1) with the count n of the arguments (a caller that normalises
 *       before a nearest x2 upsample passes n = 4 P: the statistics of the upsampled map), num_batches_tracked[0] += 1 (NULL: skipped).
 *       training == 0: the running statistics, nothing updated.
 *       The variance is merged from (count, mean, M2) partials (Chan et al.), never E[x^2] - E[x]^2.
 *       stats [3 C] is written by the forward and read by the backward: mean, rstd, then the part of the mean that fp32 dropped.
 *   act MVP_BN_ACT_TANH: y = tanh(x);  MVP_BN_ACT_NONE: y = x.  Neither normalises; gamma / beta / stats / workspace are unused.
 *   bwd: grad_y [B, C, HW] -> grad_x [P, ld] (columns C..ld-1 written as zero; NULL: parameter gradients only), with g_z =
 *       grad_y * act'(z) recomputed from x: training  grad_x = gamma rstd (g_z - dbeta / P - xhat dgamma / P),  eval  gamma rstd g_z;
 *       grad_beta [C] = sum g_z, grad_gamma [C] = sum g_z xhat (either may be NULL; accumulate != 0: added to what is there).
 *   Reductions: per-workgroup fp64 partials in the workspace, folded in a fixed order; two calls give the same bits.
 *   MVP_EINVAL: NULL x / y (fwd) / grad_y (bwd), B, HW <= 0, C outside 1..8, ld < C, an unknown act; for the sigmoid form NULL gamma /
 *   beta / stats / workspace or workspace_bytes < MVP_BN_ACT_WORKSPACE_BYTES, training with P < 2 or n < 2 (torch refuses one value
 *   per channel), eval without running statistics; bwd with nothing to write.
 * ---------------------------------------------------------------------------------- */
#define MVP_BN_ACT_MAX_C 8
#define MVP_BN_ACT_NONE 0
#define MVP_BN_ACT_SIGMOID 1
#define MVP_BN_ACT_TANH 2
#define MVP_BN_ACT_WORKSPACE_BYTES 98304 /* 512 partial rows x 8 channels x 3 fp64 */
typedef struct mvp_bn_act_args mvp_bn_act_args;
struct mvp_bn_act_args {
  const float* x; float* y;
  const float* gamma; const float* beta;
  float* running_mean; float* running_var; int64_t* num_batches_tracked;
  float* stats;
  const float* grad_y; float* grad_x; float* grad_gamma; float* grad_beta;
  void* workspace; int64_t workspace_bytes;
  int B; int64_t HW; int C; int ld;
  int64_t n;
  float eps, momentum;
  int act, training, accumulate;
};
int mvp_bn_act_fwd(const mvp_bn_act_args*, void* stream);
int mvp_bn_act_bwd(const mvp_bn_act_args*, void* stream);

/* nn.BCELoss() (mean reduction) and its gradient in one launch chain (train_generic_objectness.py:395,575).
 * pred, target [N] fp32 in [0, 1].  loss[0] = mean of -(t max(log p, -100) + (1 - t) max(log1p(-p), -100)) (torch's clamp);
 * grad_pred [N] (NULL: loss only) = (p - t) / max((1 - p) p, 1e-12) / N.  At p in {0, 1}: 100 and -+1e12 / N against the other
 * target, 0 and 0 against its own.  fp64 partial sums in the workspace, folded in a fixed order.
 * MVP_EINVAL: NULL pred / target / loss / workspace, N <= 0, workspace_bytes < MVP_BCE_WORKSPACE_BYTES or not 8-byte aligned. */
#define MVP_BCE_WORKSPACE_BYTES 8192
typedef struct mvp_bce_loss_args mvp_bce_loss_args;
struct mvp_bce_loss_args {
  const float* pred; const float* target; float* loss; float* grad_pred;
  void* workspace; int64_t workspace_bytes;
  int64_t N;
};
int mvp_bce_loss_fwd_bwd(const mvp_bce_loss_args*, void* stream);

/* Confusion counts of a thresholded prediction (train_generic_objectness.py:56-183 count these with numpy on the host).
 * pred, gt [G, n] fp32, gt holding exactly 0 or 1; counts [G, 4] int64 = TP, FP, FN, TN with "positive" = pred > threshold
 * (strictly; NaN is negative).  G = 1, n = B H W is the reference's whole-batch form; G = B gives per-image counts.  The op zeroes
 * counts itself.  MVP_EINVAL: a NULL pointer, G <= 0 or G > 65535, n <= 0, counts not 8-byte aligned. */
typedef struct mvp_binary_counts_args mvp_binary_counts_args;
struct mvp_binary_counts_args {
  const float* pred; const float* gt; int64_t* counts;
  int G; int64_t n;
  float threshold;
};
int mvp_binary_counts(const mvp_binary_counts_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * (added within ABI 8; new exports with their own tagged argument struct, no existing struct changed.)
 * Scoring of a batch of 2AFC triplets, the perceptual-similarity evaluation (evaluate_model_percepture.py:104-120: global average
 * pool of CNN maps, two F.cosine_similarity, torch.where) with the running confusion counts.  For triplet b, x in {ref, left, right}
 * points at B images of [C, HW] fp32, image b starting at element b * ld (the three parts of one stacked [3B, C, h, w] forward output
 * are passed as three pointers; they may alias).  HW = 1: [B, C] class tokens.  Definition:
 *     f_x[c]  = mean over HW of x[b, c, :]                                    (HW = 1: the value itself)
 *     sim(x)  = <f_ref, f_x> / (max(|f_ref|, 1e-8) * max(|f_x|, 1e-8))        (F.cosine_similarity: each norm is clamped)
 *     sim[b]  = {sim(left), sim(right)},   pred[b] = sim(left) > sim(right) ? 0 : 1     (compared as written, in fp32; NaN gives 1)
 *     counts  = TP, FP, FN, TN of pred against label with positive = 1; a label that is neither 0 nor 1 is counted nowhere
 * The pooled sums, both dot products, the three squared norms, the square roots and the division are fp64; each similarity is rounded
 * once to fp32: |sim - exact| < 2^-24 for every finite input (no sum of squares of fp32 values overflows fp64, so features near 1e20,
 * whose fp32 norms are inf, are scored like any others).  Both similarities of a triplet come from the same instruction sequence: bitwise-equal left and right give bitwise-equal similarities, hence pred = 1.
 * counts is written only when label is given: overwritten when accumulate == 0, added to otherwise (a loop over batches keeps its
 * running counts on the device without a launch of its own).
 * How: a grid over (triplet, chunk of channels) streams the three images once, lanes along HW inside a channel row (16-byte loads when
 * HW % 4 == 0, ld % 4 == 0 and the bases are 16-byte aligned, dword loads otherwise), and writes five fp64 partials per chunk; one wave
 * per triplet folds them in a fixed order.  No floating-point atomics (the counts are integers), no sync, no allocation; two calls
 * give the same bits.  Elements C * HW .. ld - 1 of an image are never read.
 * MVP_EINVAL: NULL ref / left / right / sim / pred; counts without label; B, C or HW <= 0; ld < C * HW; C * HW > 2^31 - 1;
 * B * chunks > 2^31 - 1 (chunks <= 256); workspace NULL, not 8-byte aligned or shorter than mvp_twoafc_workspace_bytes(B, C, HW);
 * counts not 8-byte aligned.
 * ---------------------------------------------------------------------------------- */
typedef struct mvp_twoafc_args mvp_twoafc_args;
struct mvp_twoafc_args {
  const float* ref; const float* left; const float* right; /* image b of each at element b * ld, [C, HW] fp32                */
  const float* label;                                      /* optional [B] fp32, exactly 0 or 1                              */
  float* sim;                                              /* [B, 2]  sim(left), sim(right)                                  */
  int32_t* pred;                                           /* [B]     0 = left is the closer one, 1 = right                  */
  int64_t* counts;                                         /* optional [4] TP, FP, FN, TN; needs label                       */
  void* workspace; int64_t workspace_bytes;                /* >= mvp_twoafc_workspace_bytes(B, C, HW), 8-byte aligned        */
  int64_t ld;                                              /* elements between consecutive images, >= C * HW                 */
  int B, C, HW;
  int accumulate;                                          /* != 0: add to counts instead of overwriting them                */
};
/* Workspace: B * chunks * 40 bytes, chunks = ceil(C / ceil(C / min(256, ceil(C / ceil(4096 / HW))))): the most a launch uses (it
 * rounds the channels of a chunk up to what a workgroup holds at once, which depends on the alignment).  0 for sizes that
 * mvp_twoafc_score rejects. */
int64_t mvp_twoafc_workspace_bytes(int B, int C, int HW);
int mvp_twoafc_score(const mvp_twoafc_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * (added within ABI 8; new exports with their own tagged argument struct, no existing struct changed.)
 * The pixel-level baselines of the 2AFC evaluation: PSNR and SSIM of a batch of triplets, scored and counted like mvp_twoafc_score.
 * x in {ref, left, right} points at B images of [C, H, W] fp32, image b starting at element b * ld (the three parts of one stacked
 * [3B, C, H, W] batch are passed as three pointers; they may alias).  Values are used as they are: nothing is clamped to [0, 1].
 *   metric 1, SSIM (evals/utils/losses.py:203-251 of the reference, size_average=False):
 *     g[k]   = exp(-(k - 5)^2 / (2 * 1.5^2)), k = 0..10, rounded to fp32 and divided by their fp32 sum; window = g g^T
 *     mu_x   = window * x,  E_xy = window * (x y)      per channel, zero padding of 5 pixels
 *     map    = ((2 mu_1 mu_2 + C1) (2 (E_12 - mu_1 mu_2) + C2)) / ((mu_1^2 + mu_2^2 + C1) ((E_11 - mu_1^2) + (E_22 - mu_2^2) + C2))
 *              with C1 = 1e-4, C2 = 9e-4;   score = mean of map over C * H * W.   Any H, W >= 1.
 *   metric 0, PSNR:  mse = mean over C * H * W of (a - b)^2,  score = 10 log10(1 / mse): the peak is 1; mse = 0 gives +inf.
 *     sim[b] = {score(ref, left), score(ref, right)},   pred[b] = sim[b][0] > sim[b][1] ? 0 : 1   (compared as written, in fp32; NaN
 *     gives 1, two +inf give 1);   counts = TP, FP, FN, TN of pred against label with positive = 1, as in mvp_twoafc_score: written only
 *     when label is given, overwritten when accumulate == 0, added to otherwise.
 * Precision.  PSNR: differences, squares and sums in fp64, one rounding to fp32: |sim - exact| <= 2^-24 max(1, |exact|).  SSIM: the window
 * is applied separably with the fp32 weights g in fp64 arithmetic (the reference's 2-D window is g g^T rounded to fp32: 2^-24 relative
 * per tap; on the score <= 3e-8 for noise and <= 2e-7 for smooth images, where torch's own fp32 error is 1e-5), the map, whose E - mu^2 cancels against C2, and every sum in fp64, one rounding to fp32.  Both scores of
 * a triplet come from the same instruction sequence: bitwise-equal left and right give bitwise-equal scores, hence pred = 1; a
 * candidate bitwise equal to the reference image gives SSIM 1.0f exactly and PSNR +inf.  A NaN in left does not reach sim[b][1].
 * How: the three images are read once.  SSIM: a grid over (triplet, channel, 16 x 32 tile); the tile with a 5-pixel zero-filled halo
 * in LDS, eight filtered planes (r, l, q, r^2, l^2, q^2, r l, r q: the reference image's serve both pairs), two fp64 partials per
 * workgroup.  PSNR: a grid over (triplet, chunk of >= 4096 elements), 16-byte loads when ld % 4 == 0 and the bases are 16-byte aligned.
 * One wave per triplet folds the partials in a fixed order.  No floating-point atomics (the counts are integers), no sync, no
 * allocation; two calls give the same bits.  Elements C * H * W .. ld - 1 of an image are never read.
 * MVP_EINVAL: NULL ref / left / right / sim / pred; counts without label; B, C, H or W <= 0; C * H * W > 2^31 - 1; ld < C * H * W;
 * metric not 0 or 1; B * (partials per triplet) > 2^31 - 1; workspace NULL, not 8-byte aligned or shorter than
 * mvp_pixel_score_workspace_bytes(B, C, H, W, metric); counts not 8-byte aligned.
 * ---------------------------------------------------------------------------------- */
typedef struct mvp_pixel_score_args mvp_pixel_score_args;
struct mvp_pixel_score_args {
  const float* ref; const float* left; const float* right; /* image b of each at element b * ld, [C, H, W] fp32              */
  const float* label;                                      /* optional [B] fp32, exactly 0 or 1                              */
  float* sim;                                              /* [B, 2]  score(ref, left), score(ref, right)                    */
  int32_t* pred;                                           /* [B]     0 = left is the closer one, 1 = right                  */
  int64_t* counts;                                         /* optional [4] TP, FP, FN, TN; needs label                       */
  void* workspace; int64_t workspace_bytes;                /* >= mvp_pixel_score_workspace_bytes(...), 8-byte aligned        */
  int64_t ld;                                              /* elements between consecutive images, >= C * H * W              */
  int B, C, H, W;
  int metric;                                              /* 0 = PSNR, 1 = SSIM                                             */
  int accumulate;                                          /* != 0: add to counts instead of overwriting them                */
};
/* Workspace: 16 bytes per workgroup of the first pass.  SSIM: B * C * ceil(H / 16) * ceil(W / 32) of them; PSNR: B * chunks, chunks =
 * ceil(C H W / e) with e the smallest of 4096, 8192, ... that gives at most 1024.  0 for sizes (or a metric) that mvp_pixel_score
 * rejects. */
int64_t mvp_pixel_score_workspace_bytes(int B, int C, int H, int W, int metric);
int mvp_pixel_score(const mvp_pixel_score_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * (added within ABI 8; new exports with their own tagged argument structs, no existing struct changed.)
 * MaskCut: normalised cuts on the patch affinity of a backbone's last-layer keys (evals/models/maskcut_processor.py of the
 * reference: get_affinity_matrix, second_smallest_eigenvector, get_salient_areas, check_num_fg_corners, detect_box and the loop of
 * maskcut_forward), one pass = four launches batched over Bimg images, none of which talks to the host.  N = h * w cells of the patch
 * grid, N <= 1024, C <= 4096, Bimg <= 65535.  Every launch takes `active` (optional [Bimg] bytes; NULL = all): the workgroups of an
 * image whose byte is 0 return at once and none of that image's outputs is written.  No floating-point atomics; two calls give the
 * same bits.  eps = 1e-5 is the reference's off-weight.
 *
 * mvp_ncut_affinity: feats [Bimg, C, ldf] fp32 channel-major (image b at element b * C * ldf; columns N..ldf-1 never read), painted
 * optional [Bimg, N] bytes.  f_n = column n divided by max(|column n|, 1e-12) (F.normalize; norm in fp64), or 0 where painted[n] != 0;
 * A[b, i, j] = <f_i, f_j> as a k-ordered fp32 fma chain on the fp32-input MFMA (|A - exact| ~ 1e-7; A is bitwise symmetric);
 * sums[b] = {sum, sum of squares} of the N^2 entries in fp64, folded in a fixed order.  workspace >= mvp_ncut_workspace_bytes(Bimg, N).
 *   MVP_EINVAL: NULL feats / A / sums / workspace; Bimg, N or C out of range; ldf < N; feats or A not 4-byte, sums or workspace not
 *   8-byte aligned; workspace too short.
 * mvp_ncut_threshold: tau[b] = the fixed point of Lloyd's iteration for two centres on the N^2 entries of A[b], started from
 * mean -+ std (from sums): a round assigns a to the upper cluster iff a > (c0 + c1) / 2 and replaces the centres by the cluster means
 * (fp64 sums); it stops when the upper count repeats (the clusters are nested, so that is the assignment repeating), when a cluster is
 * empty (the centres of the round before stand), or after max_rounds; tau = (c0 + c1) / 2.  bits [Bimg, N, ceil(N / 32)] uint32: bit
 * (j & 31) of word j >> 5 of row i = [A[i, j] > tau], the bits beyond column N - 1 zero; deg [Bimg, N] fp64 =
 * cnt + eps (N - cnt) from the integer row counts; rounds (optional [Bimg] int32) = rounds run.  One workgroup per image.
 *   MVP_EINVAL: NULL A / sums / tau / bits / deg; Bimg or N out of range; max_rounds <= 0; a misaligned pointer (4 bytes for A, bits
 *   and rounds, 8 for sums, tau and deg).
 * mvp_ncut_fiedler: with W = B + eps (1 - B) for the bit matrix B and D = diag(deg), the second-largest eigenpair (theta, y) of
 * S = D^-1/2 W D^-1/2, i.e. the second-smallest generalised pair (D - W) v = lambda D v with lambda = 1 - theta, v = D^-1/2 y.  One
 * workgroup per image, the image's bit matrix resident in LDS; block subspace iteration (4 vectors, fp32) on (I + S) / 2 with the top
 * pair (D^1/2 1, 1) deflated and a Rayleigh-Ritz step in fp64 every round; W is applied as (1 - eps) (B x) + eps sum(x).
 *   v [Bimg, N] fp32, scaled so that |D^1/2 v| = 1 up to rounding, sign: the entry of largest |v| is positive (lowest index on ties);
 *   lambda, residual [Bimg] fp64: 1 - theta and |S y - theta y| of y = D^1/2 v / |D^1/2 v| for the v that was written, in fp64;
 *   iters [Bimg] int32 = rounds run; converged [Bimg] bytes = 1 iff residual <= r_tol and residual <= mix_tol * (theta - theta_3)
 *   (theta_3 = the next Ritz value: residual / gap bounds the admixture of the neighbouring eigenvector) within max_iters rounds.
 *   MVP_EINVAL: a NULL pointer other than active; Bimg or N out of range; max_iters <= 0; r_tol or mix_tol not > 0; a misaligned
 *   pointer (4 bytes for bits, v and iters, 8 for deg, lambda and residual).
 * mvp_ncut_partition: from v [Bimg, h * w] (any sign): bipartition = v > mean(v) (fp64 mean); seed0 = argmax |v|; nc = foreground
 * corners (0, w - 1, (h - 1) w, N - 1, each counted as often as it is listed); reverse = nc >= 3 or seed0 not foreground; reversed:
 * the bipartition is complemented and seed = argmin v, else seed = argmax v (lowest index on ties everywhere); mask = the 4-connected
 * component of the seed.  use_prev != 0 (passes >= 2): the mask is emptied when 2 |mask & prev| > |mask | prev| (IoU > 0.5) or
 * |mask| / h / w <= 0.01.  Then pass_mask = mask (may alias prev_mask), painted |= mask (in place), union_mask = painted with its
 * holes filled (the complement of the background 4-connected to the border), seed[b] = seed.  All [Bimg, h * w] bytes, 0 / 1.
 *   MVP_EINVAL: NULL v / pass_mask / painted / union_mask / seed; use_prev without prev_mask; h, w <= 0 or h * w > 1024; Bimg out of
 *   range; v or seed not 4-byte aligned.
 * ---------------------------------------------------------------------------------- */
typedef struct mvp_ncut_affinity_args mvp_ncut_affinity_args;
struct mvp_ncut_affinity_args {
  const float* feats; const uint8_t* painted; const uint8_t* active;
  float* A; double* sums;
  void* workspace; int64_t workspace_bytes;
  int64_t ldf;
  int Bimg, C, N;
};
typedef struct mvp_ncut_threshold_args mvp_ncut_threshold_args;
struct mvp_ncut_threshold_args {
  const float* A; const double* sums; const uint8_t* active;
  double* tau; uint32_t* bits; double* deg; int32_t* rounds;
  int Bimg, N, max_rounds;
};
typedef struct mvp_ncut_fiedler_args mvp_ncut_fiedler_args;
struct mvp_ncut_fiedler_args {
  const uint32_t* bits; const double* deg; const uint8_t* active;
  float* v; double* lambda; double* residual; int32_t* iters; uint8_t* converged;
  int Bimg, N, max_iters;
  float r_tol, mix_tol;
};
typedef struct mvp_ncut_partition_args mvp_ncut_partition_args;
struct mvp_ncut_partition_args {
  const float* v; const uint8_t* prev_mask; const uint8_t* active;
  uint8_t* pass_mask; uint8_t* painted; uint8_t* union_mask; int32_t* seed;
  int Bimg, h, w, use_prev;
};
/* Workspace of mvp_ncut_affinity: the inverse column norms and one {sum, sum of squares} pair per 64 x 64 tile of A.  0 for sizes
 * that it rejects. */
int64_t mvp_ncut_workspace_bytes(int Bimg, int N);
int mvp_ncut_affinity(const mvp_ncut_affinity_args*, void* stream);
int mvp_ncut_threshold(const mvp_ncut_threshold_args*, void* stream);
int mvp_ncut_fiedler(const mvp_ncut_fiedler_args*, void* stream);
int mvp_ncut_partition(const mvp_ncut_partition_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * (added within ABI 8; new exports with their own tagged argument structs, no existing struct changed.)
 * Dense CRF: the refinement the reference applies to every MaskCut bipartition (evals/models/crf.py::densecrf and
 * maskcut_processor.py:376-404), with the CRF's two message-passing sums evaluated exactly over all pixel pairs.  The model:
 *
 * Given an image `I` (uint8 RGB, H × W) and a binary mask `m` (H × W; `crf.py` bilinearly resizes the two logit planes `(1−m, m)` to
 * H × W when sizes differ, an identity in the processor):
 *
 * - **Unary.** `p_l(i) = softmax_l(1−m_i, m_i)`, that is `e/(1+e)` for the pixel's own label and `1/(1+e)` for the other.
 *   `U_l(i) = −log p_l(i)`. `unary_from_softmax` clips at 1e-5, which is never reached here.
 * - **Kernels.** Both include `j = i`.
 *   - `k_g(i,j) = exp(−(Δx²+Δy²)/(2·3²))`, weight 7.
 *   - `k_b(i,j) = exp(−(Δx²+Δy²)/(2·50²) − (Δr²+Δg²+Δb²)/(2·5²))`, weight 10.
 *   - These are `POS_W`, `POS_XY_STD`, `Bi_W`, `Bi_XY_STD`, `Bi_RGB_STD` of `crf.py`.
 * - **Symmetric normalisation.** `n(i) = (Σ_j k(i,j) + 1e-20)^(−1/2)`. The filtered field is `n(i)·Σ_j k(i,j)·n(j)·Q_l(j)`.
 * - **Mean field.** `Q⁰ = p`. For t = 1…10 (`MAX_ITER`): `a_l = −U_l + 7·(filtered_g Q_l) + 10·(filtered_b Q_l)` with Potts
 *   compatibility, then `Q = softmax_l(a)`.
 * - **MAP.** `MAP(i) = 1` iff `Q_1(i) > Q_0(i)`. Ties go to 0.
 *
 * With two labels one field per object is kept: Q_0 = 1 - Q_1, so per image K·1 (-> n) and K·n are filtered once and K·(n Q_1) once
 * per iteration, all objects of an image as the F fields of one pass.  `active` (optional [B] bytes; NULL = all) as for MaskCut: the
 * workgroups of an image whose byte is 0 return at once and none of its outputs is written.  No floating-point atomics; two calls
 * give the same bits.
 *
 * mvp_crf_filter: out[b, f, i] = sum over ALL pixels j of image b of w(i, j) in[b, f, j],
 *     w(i, j) = exp(-(dx^2 + dy^2) inv_var_xy / 2 - (dr^2 + dg^2 + db^2) inv_var_rgb / 2)      (inv_var = 1 / sigma^2)
 * rgb [B, H, W, 3] bytes; in / out: field f of image b at element b * stride + f * H * W, F <= 8 fields (fields >= F are neither read
 * nor written); in == NULL stands for the all-ones field.  inv_var_rgb == 0 gives the spatial kernel (rgb is then not read).  The
 * differences are formed directly (exact integers in fp32, no |a|^2 + |b|^2 - 2ab expansion), the weight is one hardware exp2 with
 * log2(e) folded into the constants.  Lanes own the pixels of a 16 x 16 target tile, the 16 x 16 source tiles pass through LDS and are
 * read as broadcasts; each source row's 16 terms are summed in fp32 and the row sums are folded into an fp64 accumulator in row and
 * tile order, rounded once to fp32 at the end.  A tile pair whose closest pixels already give a weight <= 2^-40 is skipped: every sum
 * of a non-negative field changes by less than H W 2^-40 times the field's maximum (sigma = 3 makes the kernel local: 23 pixels).
 *   MVP_EINVAL: NULL rgb / out; B not in 1..65535; F not in 1..8; H or W not in 1..4096 or H W > 2^22; a stride < F H W; inv_var_xy not
 *   > 0 or inv_var_rgb < 0 (or not finite); in / out not 4-byte aligned.
 * mvp_crf_update: pointwise, fp64 arithmetic on fp32 fields; N = H W; the [B, F, N] buffers (mask, filt_*, q, x_*, map) hold field f
 * of image b at element b * stride + f * N, the [B, N] buffers (norm_*, ones_*) are dense.
 *   MVP_CRF_NORMALISE: norm_k <- (norm_k + 1e-20)^(-1/2) in place (norm_k holding K_k·1 on entry), k = g, b.
 *   MVP_CRF_INIT:      q = Q_1^0 = 1 / (1 + exp(1 - 2 mask)) (mask in [0, 1]: the resized logit plane, 0 / 1 in the processor).
 *   MVP_CRF_STEP:      q = 1 / (1 + exp(-(a_1 - a_0))),  a_1 - a_0 = U_0 - U_1 + w_g n_g (2 filt_g - ones_g) + w_b n_b (2 filt_b - ones_b)
 *                      with filt_k = K_k·(n_k Q_1) and ones_k = K_k·n_k (U from mask, clipped at 1e-5 like unary_from_softmax).
 *   INIT and STEP also write x_k = n_k q (the next filter inputs) and, when map != NULL, map = [a_1 - a_0 > 0] as bytes.
 *   MVP_EINVAL: a NULL pointer the mode needs; B not in 1..65535; F not in 1..8; N not in 1..2^22; stride < F N; an unknown mode; a
 *   float pointer not 4-byte aligned.
 * mvp_mask_finish: the post-processing of process_image.  map, ref, refined: [B, F, H W] bytes (field f of image b at
 * b * stride + f * H W, F <= 64 passes); active here is optional [B, F] bytes, one per (image, pass).  One workgroup per active (image, pass), the
 * mask bit-packed in LDS (H * 32 * ceil(W / 32) <= 2^20 bits): A = binary_fill_holes(map) (the complement of the background that is
 * 4-connected to the border); refined = A, or all zeros iff 2 |A & ref| < |A | ref| (IoU < 0.5 on integer counts; an empty union keeps
 * it, like the NaN comparison of the reference); kept (optional [B, F] bytes) = 0 where it was dropped.  Then, when union_mask
 * (optional [B, H W] bytes) is given, one workgroup per image: union_mask = binary_fill_holes(OR of the active passes' refined).
 *   MVP_EINVAL: NULL map / ref / refined; B not in 1..65535; F not in 1..64; H, W <= 0 or H * ceil(W / 32) > 32768; stride < F H W.
 * ---------------------------------------------------------------------------------- */
#define MVP_CRF_NORMALISE 0
#define MVP_CRF_INIT 1
#define MVP_CRF_STEP 2
typedef struct mvp_crf_filter_args mvp_crf_filter_args;
struct mvp_crf_filter_args {
  const uint8_t* rgb; const float* in; const uint8_t* active;
  float* out;
  int64_t in_stride, out_stride;
  int B, F, H, W;
  float inv_var_xy, inv_var_rgb;
};
typedef struct mvp_crf_update_args mvp_crf_update_args;
struct mvp_crf_update_args {
  const float* mask; const uint8_t* active;
  float* norm_g; float* norm_b;
  const float* ones_g; const float* ones_b; const float* filt_g; const float* filt_b;
  float* q; float* x_g; float* x_b; uint8_t* map;
  int64_t stride, N;
  int B, F, mode;
  float w_g, w_b;
};
typedef struct mvp_mask_finish_args mvp_mask_finish_args;
struct mvp_mask_finish_args {
  const uint8_t* map; const uint8_t* ref; const uint8_t* active;
  uint8_t* refined; uint8_t* kept; uint8_t* union_mask;
  int64_t stride;
  int B, F, H, W;
};
int mvp_crf_filter(const mvp_crf_filter_args*, void* stream);
int mvp_crf_update(const mvp_crf_update_args*, void* stream);
int mvp_mask_finish(const mvp_mask_finish_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * Convolution weight re-layout (per step; the probe's conv weights are trained):
 *   mode 0: [Cout,Cin,kh,kw] fp32 -> forward GEMM operand [Cout, kh*kw*Cin] bf16 pair (k = tap*Cin + c)
 *   mode 1: -> data-gradient operand [Cin, kh*kw*Cout] (k = tap'*Cout + n, taps flipped)
 * Replaces the implicit weight access of nn.Conv2d fwd / bwd-data (probes.py:283-288,371-375).
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const float* w; mvp_bf16* out_hi; mvp_bf16* out_lo;
  int Cout, Cin, kh, kw, mode;
} mvp_conv_weight_pack_args;
int mvp_conv_weight_pack(const mvp_conv_weight_pack_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * Nearest-neighbour upsample by an integer factor f on channels-last fp32 [B,H,W,C]
 * (F.interpolate(x, scale_factor=f), probes.py:388,396,398); backward = f x f block sums
 * (src is then the fine [B,H*f,W*f,C] gradient).  Outputs: fp32 and/or bf16 pair.
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const float* src; float* dst_f32; mvp_bf16* dst_hi; mvp_bf16* dst_lo;
  int B, H, W, C, f; int backward; /* H,W = COARSE dims in both directions */
} mvp_upsample_cl_args;
int mvp_upsample_nearest_cl(const mvp_upsample_cl_args*, void* stream);

/* Backward of "nearest x f upsample, then 3x3 / pad 1 convolution" folded onto the COARSE grid (the DPT probe's out_conv,
 * probes.py:384-398: F.interpolate(scale_factor=4) then Conv2d(3x3)): box sums of the fine-grid output gradient g [B, H*f, W*f, C]
 * per coarse pixel and tap, G[(b,i,j), ky*3+kx, c] = sum of g[p, c] over fine pixels p with p + (ky-1, kx-1) in block (i, j), written
 * as a bf16 pair [B*H*W, 9*C] (out_lo may be null).  Then dW = Gᵀ·x (mvp_gemm_tn_conv, 1x1) and dx = G·Wᵀ (mvp_gemm_bias_act_res)
 * over the coarse pixels replace the autograd backward of that Conv2d + interpolate pair.  f in {2, 4}; C % 4 == 0. */
typedef struct {
  const float* g; mvp_bf16* out_hi; mvp_bf16* out_lo;
  int B, H, W, C, f; /* H, W = COARSE dims */
} mvp_upconv_boxsum_args;
int mvp_upconv3_grad_boxsum(const mvp_upconv_boxsum_args*, void* stream);

/* Forward of the same pair from COARSE tap products: t [B*H*W, 9*C] fp32 = x · W_tapᵀ for the 9 taps (ONE GEMM over the coarse pixels,
 * column tap*C + c); y[p] = act(bias + sum over the taps of t[cell(p + d_tap), tap]) per fine pixel p (taps outside the image = zero
 * padding), written as the convolution's epilogue would: fp32 and / or bf16 pair [B*H*f*W*f, C], gate mask (post-ReLU value > 0).
 * act in {MVP_ACT_NONE, MVP_ACT_RELU}; f in {2, 4}; C % 4 == 0. */
typedef struct {
  const float* t; const float* bias; float* out_f32; mvp_bf16* out_hi; mvp_bf16* out_lo; uint8_t* out_mask;
  int B, H, W, C, f, act; /* H, W = COARSE dims */
} mvp_upconv_gather_args;
int mvp_upconv3_fwd_gather(const mvp_upconv_gather_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * Convolution weight gradient (TN GEMM over pixels, split-K):
 *   dW[n, c, ky, kx] (+)= sum_m G[m, n] * X[pix(m, ky, kx), c]
 * G = output gradient [M = B*Ho*Wo, ldg] channels-last bf16 pair (ldg >= roundup(Cout,128),
 * pad columns zero), X = layer input [B, H>>up, W>>up, ldx] channels-last bf16 pair seen through
 * a nearest upsample by 2^up; Cin % 128 == 0.  1x1 convs / linear layers use kh=kw=1, pad=0.
 * partial: fp32 workspace of mvp_gemm_tn_workspace_bytes(...) bytes.  Replaces the autograd
 * weight-gradient of nn.Conv2d (probes.py:283-288,352-355,371-375).
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const mvp_bf16* g_hi; const mvp_bf16* g_lo; const mvp_bf16* x_hi; const mvp_bf16* x_lo;
  float* partial; float* dw; const mvp_bf16* zero_page; /* >= 512 zero bytes (ABI stability: no longer read, padding = out-of-range offsets) */
  int64_t M; int Cout, Cin, ldg, ldx;
  int H, W, Ho, Wo, kh, kw, stride, pad, up;
  int splits, accumulate, precision;
} mvp_gemm_tn_args;
/* ------------------------------------------------------------------------------------
 * Validation metrics, fused masked reductions per image:
 *   depth : evaluate_depth global metrics (evals/utils/metrics.py:106-178): out[b] =
 *           {d1,d2,d3,rmse,mean_pred,std_pred,variance_pred,mean_gt,std_gt,variance_gt,variance_ratio,n_valid};
 *           scale_invariant != 0 first solves match_scale_and_shift (metrics.py:742-780) per image and
 *           writes (scale, shift) to scale_shift[b].  pred/gt [B, HW].
 *   snorm : evaluate_surface_norm global metrics (metrics.py:397-440): out[b] = {d1,d2,d3,rmse_deg,n_valid};
 *           pred [B,Cp>=3,HW] (first 3 channels), gt [B,3,HW], valid = |gt|_1 > 0.
 * workspace >= mvp_metrics_workspace_bytes(B).
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const float* pred; const float* gt; float* out; float* scale_shift;
  void* workspace; int64_t workspace_bytes; int B; int64_t HW; int scale_invariant;
} mvp_depth_metrics_args;
typedef struct {
  const float* pred; const float* gt; float* out;
  void* workspace; int64_t workspace_bytes; int B; int Cp; int64_t HW; float t1, t2, t3;
} mvp_snorm_metrics_args;
int64_t mvp_metrics_workspace_bytes(int B);
int mvp_depth_metrics(const mvp_depth_metrics_args*, void* stream);
int mvp_snorm_metrics(const mvp_snorm_metrics_args*, void* stream);
/* y = x * scale[b] + shift[b] per image (match_scale_and_shift, metrics.py:775-777), optionally clamped to [lo, hi]
 * (scale-invariant training, train_depth.py:116-118).  backward != 0: out = d/dx = grad_out * scale[b] where the clamp
 * is inactive, else 0 (scale/shift are detached in the reference).  x / out / grad_out [B, HW]; scale_shift [B, 2]. */
typedef struct {
  const float* x; const float* scale_shift; const float* grad_out; float* out;
  int B; int64_t HW; float lo, hi; int clamp; int backward;
} mvp_scale_shift_args;
int mvp_scale_shift(const mvp_scale_shift_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * Per-level / per-segment breakdown of the validation metrics (evaluate_depth
 * evals/utils/metrics.py:179-358, evaluate_surface_norm metrics.py:441-577) as one segmented masked
 * reduction per batch.  Every pixel is binned by its "centroid level" (nested centre boxes whose
 * offset (H / L) * (L - level) / 2 is applied to both axes, metrics.py:249-262) and by its
 * integer segment id:
 *   level_sums [B, L, 5] fp64 = {n_valid, #(x<t1), #(x<t2), #(x<t3), sum err^2}
 *   seg_sums   [B, S, 6] fp64 = {n_all, n_valid, #(x<t1), #(x<t2), #(x<t3), sum err^2}   (ids outside [0,S) are skipped)
 * Cp == 0: depth — pred/gt [B,H,W], valid = gt > 0, x = max(gt/pred, pred/gt) with thresholds 1.25^k,
 *          err = gt - pred; scale_shift != NULL applies the per-image (scale, shift) of mvp_depth_metrics first.
 * Cp >= 3: surface normals — pred [B,Cp,H,W], gt [B,3,H,W], valid = |gt|_1 > 0, x = err = angular error in degrees,
 *          thresholds t1..t3.
 * seg == NULL: levels only (the reference's is_navi=True path).  The 1e-6 / clamp(1) normalisations, the
 * stuff/things grouping and the segment list are finished by the host from these bins.
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const float* pred; const float* gt; const int32_t* seg; const float* scale_shift;
  double* level_sums; double* seg_sums;
  void* workspace; int64_t workspace_bytes;   /* >= mvp_metrics_breakdown_workspace_bytes(B, L, S), 8-byte aligned */
  int B, H, W, Cp, num_levels, num_ids;
  float t1, t2, t3;
} mvp_metrics_breakdown_args;
int64_t mvp_metrics_breakdown_workspace_bytes(int B, int num_levels, int num_ids);
int mvp_metrics_breakdown(const mvp_metrics_breakdown_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * Fused tail of the linear depth-bin probe: bilinear x f (align_corners=False) of the
 * token-resolution logits L0 [B,h,w,K] fused with DepthBinPrediction (probes.py:431 + :176-200).
 * The upsampled logits are never materialised; gate holds 1 bit per (pixel, bin) = [logit > 0].
 *   fwd: l0 -> depth [B*hf*wf], inv_sum [B*hf*wf], gate [B*hf*wf, K/8]
 *   bwd: grad_depth, depth, inv_sum, gate -> grad_l0 [B,h,w,K]          (K % 8 == 0)
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const float* l0; float* depth; float* inv_sum; uint8_t* gate;
  const float* grad_depth; float* grad_l0;
  int B, h, w, K, f;
  float min_depth, max_depth;
} mvp_linear_bins_args;
int mvp_linear_bins_fwd(const mvp_linear_bins_args*, void* stream);
int mvp_linear_bins_bwd(const mvp_linear_bins_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * im2col of an NCHW fp32 image for convs whose Cin is not a multiple of 32 (the ResNet 7x7/2 RGB
 * stem, dino_res50.py:38-44): out[(b,yo,xo), (ky*kw+kx)*C + c], zero padded to ldk columns (ldk % 8 == 0).
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const float* src; mvp_bf16* out_hi; mvp_bf16* out_lo;
  int B, C, H, W, Ho, Wo, kh, kw, stride, pad, ldk;
} mvp_im2col_args;
int mvp_im2col_nchw(const mvp_im2col_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * Max-pool k x k / stride on channels-last fp32 [B,H,W,C] (-inf padding, torchvision
 * resnet50.maxpool 3x3/2 pad 1).  Outputs fp32 and/or bf16 pair.
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const float* src; float* dst_f32; mvp_bf16* dst_hi; mvp_bf16* dst_lo;
  int B, H, W, C, Ho, Wo, k, stride, pad;
} mvp_maxpool_cl_args;
int mvp_maxpool_cl(const mvp_maxpool_cl_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * ResNet-50 stem fused: conv 7x7 / 2 / pad 3 (3 -> 64, BatchNorm folded into w / bias) + ReLU + max-pool 3x3 / 2 / pad 1,
 * NCHW fp32 image -> channels-last [B, Hp, Wp, 64] (torchvision resnet50.conv1/bn1/relu/maxpool, dino_res50.py:38-44,83-90).
 * w_hi/lo [64, 160] bf16: k = (ky*7 + kx)*3 + c, zero padded from 147.  Ho = (H-1)/2+1, Hp = (Ho-1)/2+1 (same for W).
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const float* images; const mvp_bf16* w_hi; const mvp_bf16* w_lo; const float* bias;
  float* out_f32; mvp_bf16* out_hi; mvp_bf16* out_lo;
  int B, H, W, precision;
} mvp_stem_args;
int mvp_stem7x7_pool(const mvp_stem_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * Gradient gate + split: dst = src * (mask != 0) as fp32 (may alias src) and as a bf16 pair
 * with row stride ldo >= N (pad columns zeroed) — the ReLU backward of probes.py:283-288 fused
 * with the operand conversion for the next MFMA GEMM.  mask may be NULL (plain split).
 * relu_mask_out != NULL: forward ReLU instead — dst = max(src, 0), relu_mask_out[r*ldm + c] = (src > 0)
 * (the ReLU that follows a bilinear upsample in MultiscaleHead, probes.py:449-457, fused with the split).
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const float* src; const uint8_t* mask; float* dst_f32; mvp_bf16* dst_hi; mvp_bf16* dst_lo;
  int64_t M; int N, lds, ldm, ldo;
  uint8_t* relu_mask_out;
} mvp_mask_split_args;
int mvp_mask_split(const mvp_mask_split_args*, void* stream);

int64_t mvp_gemm_tn_workspace_bytes(int Cout, int Cin, int kh, int kw, int splits);
int mvp_gemm_tn_conv(const mvp_gemm_tn_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * ConvNeXt block, first half: depthwise 7x7 convolution (stride 1, zero padding 3) + LayerNorm over the channels on a
 * channels-last fp32 map, written as the A operand of the block's fc1 GEMM.  Replaces what evals/models/convnext.py:87-91 runs
 * inside `self.visual.stages` for every block: timm ConvNeXtBlock.conv_dw + .norm (transformers ConvNextLayer.dwconv + .layernorm).
 *   y[b, y, x, c] = bias[c] + sum_{ky, kx} weight[c, ky, kx] * x[b, y + ky - 3, x + kx - 3, c]      (taps outside the image: zero,
 *   at the seam between two images of a batch too), taps summed ky-major, then kx, the bias last, in fp32;
 *   out[b, y, x, :] = LayerNorm_C(y[b, y, x, :]) * gamma + beta, two-pass (mean, then the centred variance) like mvp_layernorm_fwd.
 * The same inputs give the same bits.  C % 32 == 0, 32 <= C <= 2048, any B, H, W >= 1 (maps smaller than the window included);
 * anything else is MVP_EINVAL before any launch.
 * ---------------------------------------------------------------------------------- */
typedef struct mvp_dwconv7_ln_args mvp_dwconv7_ln_args;
struct mvp_dwconv7_ln_args {
  const float* x;                     /* [B, H, W, ldx] fp32 channels-last, channels 0 .. C-1 of every pixel are read; 16-byte aligned */
  const float* weight;                /* [C, 7, 7] fp32 (nn.Conv2d(C, C, 7, padding=3, groups=C).weight)                             */
  const float* bias;                  /* [C]                                                                                         */
  const float* gamma; const float* beta; /* [C] LayerNorm weight / bias                                                              */
  mvp_bf16* out_hi; mvp_bf16* out_lo; /* [B*H*W, C] pair as mvp_layernorm_args writes it (lo may be NULL; both NULL needs out_f32)   */
  float* out_f32;                     /* optional fp32 copy [B*H*W, C], or NULL (must not alias x: neighbours read x)                */
  int B, H, W, C;
  int ldx;                            /* pixel stride of x, elements: >= C, % 4 == 0                                                 */
  float eps;
  int out_layout;                     /* MVP_PAIR_SEPARATE or MVP_PAIR_A_ILV32, as mvp_layernorm_args.out_layout                     */
  int out_f16;                        /* 1: the pair is the activation operand of MVP_PREC_F16X2, as mvp_layernorm_args.out_f16      */
};
int mvp_dwconv7_ln_fwd(const mvp_dwconv7_ln_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * ConvNeXt V2's global response normalisation on the fc1 output h [B, HW, C4] fp32 (timm GlobalResponseNormMlp.grn /
 * transformers ConvNextV2GRN, run per block by evals/models/convnext.py:87-91 for the fcmae checkpoint, :42-47):
 *   mvp_grn_stats:  G[b, c] = sqrt(sum_hw h[b, hw, c]^2)  (fp64 partial sums folded in a fixed order),  N[b, c] = G[b, c] / (mean_c G[b, :] + 1e-6)
 *   mvp_grn_apply:  out = gamma[c] * (h * N[b, c]) + beta[c] + h, written as the A operand pair of fc2 (and / or fp32)
 * Both are plain launches on `stream`: no host synchronisation between them.  C4 % 8 == 0 (% 32 for MVP_PAIR_A_ILV32).
 * workspace (mvp_grn_stats): >= mvp_grn_workspace_bytes(B, HW, C4) bytes, 8-byte aligned; it needs no initialisation.
 * ---------------------------------------------------------------------------------- */
typedef struct mvp_grn_args mvp_grn_args;
struct mvp_grn_args {
  const float* h;                     /* [B, HW, C4] fp32                                                                            */
  const float* gamma; const float* beta; /* [C4] (mvp_grn_apply)                                                                     */
  float* G;                           /* [B, C4] out of mvp_grn_stats                                                                */
  float* N;                           /* [B, C4] out of mvp_grn_stats, in of mvp_grn_apply                                           */
  mvp_bf16* out_hi; mvp_bf16* out_lo; /* [B*HW, C4] bf16 pair (mvp_grn_apply; lo may be NULL)                                        */
  float* out_f32;                     /* optional fp32 copy (may be h itself), or NULL                                               */
  void* workspace; int64_t workspace_bytes;
  int B, HW, C4;
  int out_layout;                     /* MVP_PAIR_SEPARATE or MVP_PAIR_A_ILV32                                                       */
};
int64_t mvp_grn_workspace_bytes(int B, int HW, int C4);
int mvp_grn_stats(const mvp_grn_args*, void* stream);
int mvp_grn_apply(const mvp_grn_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * Device-side training augmentation of an NYU / NAVI batch (added within ABI 8; new exports with their own tagged argument structs,
 * no existing struct changed).  Replaces what the reference runs per sample on the host in get_nyu_transforms (evals/datasets/utils.py:160-218)
 * and nyu.py:227-239: RandomApply([ColorJitter(0.2, 0.2, 0.2, 0.2)], p=0.8) on the image, then ONE geometric transform shared by image, depth and
 * normals (HorizontalFlip, Rotate(limit=10), RandomResizedCrop, all nearest-neighbour), then Normalize(mean, std).  The random draws are
 * made on the host (mvp/augment.py: sample_params); the kernels read them from a device table of MVP_AUGMENT_WORDS 32-bit words per image:
 *   word 0       flags: bit 0 = colour jitter on, bit 1 = horizontal flip, bit 2 = rotate
 *   word 1       order of the jitter operations: bits [2i, 2i+1] = operation at position i (0 brightness, 1 contrast, 2 saturation, 3 hue)
 *   words 2..5   fp32 factors: brightness, contrast, saturation (each multiplies), hue shift in turns
 *   words 6, 7   fp32 cos(theta), sin(theta) of the rotation
 *   words 8..11  int32 crop box x0, y0, cw, ch in the (flipped, rotated) H x W image; the full image is (0, 0, W, H)
 *   words 12..15 reserved, zero
 * Output pixel (dy, dx) of the Ho x Wo result takes source pixel (yy, xx) of EVERY input plane, composed from the three integer maps
 *   crop:    sx = x0 + (dx * cw) / Wo,  sy = y0 + (dy * ch) / Ho                      (integer division: nearest resize without half-pixel)
 *   rotate:  u = sx - (W-1)/2, v = sy - (H-1)/2;  rx = floor((W-1)/2 + cos*u - sin*v + 0.5), ry = floor((H-1)/2 + sin*u + cos*v + 0.5) in fp32
 *            (fused multiply-adds, the sin term first), indices outside the image reflected without repeating the edge (reflect-101)
 *   flip:    xx = W-1-rx
 * which is exactly flip, then rotate, then crop-and-resize applied one after the other.  The box is clamped into the image first, so no
 * table content makes a read leave the inputs.  The jitter uses torchvision's float-tensor formulas on values in [0, 1] (uint8 / 255), in
 * fp32; it is evaluated at the gathered pixels only, except that the contrast operation's mean m is the mean grey value
 * 0.2989 r + 0.587 g + 0.114 b over the WHOLE source image as it stands when contrast is reached: mvp_augment_stats writes, per image,
 * MVP_AUGMENT_PARTIALS fp64 partial sums of it (one per workgroup, fixed order inside; zero for images whose jitter is off), and
 * mvp_augment_apply adds them in index order and divides by H * W.  No atomics: the same inputs give the same bits.
 * H, W >= 4; H * W <= 2^29; Ho, Wo >= 1.  partials: 8-byte aligned, >= mvp_augment_partials_bytes(B) bytes, no initialisation needed.
 * mvp_augment_apply with partials == NULL treats every image's jitter as off (the validation path: normalisation only).
 * ---------------------------------------------------------------------------------- */
#define MVP_AUGMENT_WORDS 16
#define MVP_AUGMENT_PARTIALS 32
typedef struct mvp_augment_stats_args mvp_augment_stats_args;
struct mvp_augment_stats_args {
  const void* image;                  /* uint8 [B, H, W, 3] (image_u8 = 1) or fp32 [B, 3, H, W] in [0, 1] (image_u8 = 0)                */
  const int32_t* params;              /* [B, MVP_AUGMENT_WORDS] on the device                                                        */
  double* partials;                   /* [B, MVP_AUGMENT_PARTIALS] out                                                               */
  int64_t partials_bytes;
  int B, H, W;
  int image_u8;
};
typedef struct mvp_augment_apply_args mvp_augment_apply_args;
struct mvp_augment_apply_args {
  const void* image;                  /* as mvp_augment_stats_args.image                                                             */
  const float* depth;                 /* [B, 1, H, W] fp32                                                                           */
  const float* snorm;                 /* [B, 3, H, W] fp32, or NULL                                                                  */
  const int32_t* params;              /* [B, MVP_AUGMENT_WORDS] on the device                                                        */
  const double* partials;             /* out of mvp_augment_stats for the same image and params, or NULL (no jitter)                 */
  float* out_image;                   /* [B, 3, Ho, Wo] fp32, (v - mean) / std                                                       */
  float* out_depth;                   /* [B, 1, Ho, Wo]                                                                              */
  float* out_snorm;                   /* [B, 3, Ho, Wo], NULL iff snorm is                                                           */
  int64_t partials_bytes;
  int B, H, W, Ho, Wo;
  int image_u8;
  float mean_r, mean_g, mean_b;       /* Normalize(mean, std) of get_nyu_transforms; (0, 0, 0) / (1, 1, 1) for image_mean "None"     */
  float std_r, std_g, std_b;
};
int64_t mvp_augment_partials_bytes(int B);
int mvp_augment_stats(const mvp_augment_stats_args*, void* stream);
int mvp_augment_apply(const mvp_augment_apply_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * The gate of DINOv2's SwiGLU MLP (added within ABI 8; a new export with its own tagged argument struct, no existing struct changed).
 * Replaces the middle of SwiGLUFFNFused.forward, which the reference runs inside torch.hub's dinov2_vitg14 (evals/models/dino.py:25-32,
 * "vitg14"): x12 = w12(x); x1, x2 = x12.chunk(2, dim=-1); out = w3(F.silu(x1) * x2), hidden width H = (int(4C * 2 / 3) + 7) / 8 * 8
 * (4096 at C = 1536).  The two Linear layers are GEMMs of this library; this is the pointwise step between them:
 *   out[m, c] = silu(h12[m, c]) * h12[m, H + c],   silu(x) = x / (1 + exp2(-x log2 e))     (c < H)
 *   out[m, c] = 0                                                                           (H <= c < ld_out, pair outputs only)
 * in fp32 with one v_exp_f32 and one v_rcp_f32 per element, multiply-adds spelled out (no contraction): the same inputs give the same
 * bits.  The exponent argument keeps the rounding error of x * log2 e as a first-order correction of the sigmoid (csrc/swiglu.hip).
 * A gate below about -87 may return +-0 (the sigmoid is subnormal there and the reciprocal may flush it; from about -88.7 down exp2
 * overflows and the reciprocal is 0); NaN propagates; an fp16 half saturates at +-65504 like
 * every compensated pair of this library.  The pair halves are bit for bit what mvp_layernorm_fwd writes for the same fp32 value.
 * The zero columns let the w3 GEMM run at K = ld_out (the tile kernels take K % 64, % 32 in bf16x3; H is a multiple of 8 only) against
 * weights padded with zero columns.  M >= 1, H >= 8, H % 8 == 0, M * ld_out / 8 < 2^31, every pointer 16-byte aligned; anything else
 * is MVP_EINVAL before any launch.  No output may alias h12.
 * ---------------------------------------------------------------------------------- */
typedef struct mvp_swiglu_args mvp_swiglu_args;
struct mvp_swiglu_args {
  const float* h12;                   /* [M, ld_in] fp32: gate in columns 0 .. H-1, value in H .. 2H-1 (mvp_gemm_args.out_f32 of w12)  */
  mvp_bf16* out_hi; mvp_bf16* out_lo; /* [M, ld_out] pair as mvp_layernorm_args writes it; both NULL needs out_f32; lo may be NULL only
                                         for MVP_PAIR_SEPARATE with out_f16 = 0 (the operand of a one-product bf16 GEMM)               */
  float* out_f32;                     /* optional fp32 copy [M, H] (row stride H), or NULL                                           */
  int M, H;
  int ld_in;                          /* row stride of h12, elements: >= 2H, % 4 == 0                                                */
  int ld_out;                         /* columns of a pair row: >= H, % 8 == 0 (% 32 for MVP_PAIR_A_ILV32, whose row stride is 2 ld_out) */
  int out_layout;                     /* MVP_PAIR_SEPARATE or MVP_PAIR_A_ILV32, as mvp_layernorm_args.out_layout                     */
  int out_f16;                        /* 1: the pair is the activation operand of MVP_PREC_F16X2, as mvp_layernorm_args.out_f16      */
};
int mvp_swiglu_fwd(const mvp_swiglu_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * (added within ABI 8; new exports with their own tagged argument structs, no existing struct changed.)
 * The task-specific ends of Taskonomy probing (evals/datasets/transforms.py task_transform / make_valid_mask, evals/utils/losses.py:77-94
 * MaskedL1Loss, evals/utils/metrics.py:580-739).  All reductions: per-workgroup fp64 partials in the workspace, folded in a fixed
 * order, no float atomics; two calls give the same bits.  One workspace size serves the loss and the metrics.
 *
 * mvp_task_prepare: the raw target and the raw mask, as a decoder leaves them, -> the training tensors.
 *   target_raw  bits = 8: uint8 [B, H, W, Cs], the first Ct channels kept;  bits = 16: uint16 [B, H, W] (Cs = Ct = 1).
 *   mask_raw    uint8 [B, H, W]
 *   target      fp32 [B, Ct, H, W] = k / 255 or k / 65535, a correctly rounded fp32 division; clamp_max > 0 (the task's clamp_to
 *               (0, maxx)): then min(max(x, 0), clamp_max) / clamp_max, correctly rounded again.
 *   valid       uint8 [B, 1, H, W], 0 or 1: make_valid_mask.  With hp = H / 4, wp = W / 4 (integer), pixel (y, x) is valid iff all 16
 *               raw mask values of rows 4i .. 4i+3, columns 4j .. 4j+3 equal 255, (i, j) = ((y hp) / H, (x wp) / W).  Rows and columns
 *               from 4 hp / 4 wp on belong to no block: what they hold invalidates nothing, and they read a block through the map.
 *   H % 4 == 0, W % 4 == 0, Cs <= 4 and aligned bases (16 bytes target, 8 the 16-bit raw target, 4 the rest): 16-byte stores, 4-byte
 *   mask words; anything else one pixel per thread.
 *   MVP_EINVAL: a NULL pointer, B <= 0, H < 4 or W < 4 (the reference's pooling has no output), Ct < 1, Cs < Ct, bits not 8 or 16,
 *   bits = 16 with Cs != 1, clamp_max < 0 or NaN.
 *
 * mvp_masked_l1_fwd_bwd: pred, target fp32 [B, C, HW]; valid uint8 [B, Cm, HW], Cm = 1 (one mask for every channel) or C.
 *   loss[0] = sum valid |pred - target| / (sum valid * C / Cm): differences taken in fp64 (exact), summed in fp64, one rounding to
 *   fp32.  grad_pred [B, C, HW] (NULL: loss only) = sign(pred - target) * fp32(1 / count) where valid, exactly 0 elsewhere (a select;
 *   sign(0) = 0).  No valid pixel: the loss is NaN (0 / 0, as the reference) and the gradient all zeros.  Two launches: the count
 *   is complete before the gradient is written.
 *   MVP_EINVAL: a NULL pointer other than grad_pred, B, C or HW <= 0, Cm not 1 or C, workspace_bytes < MVP_TASK_WORKSPACE_BYTES or
 *   the workspace not 8-byte aligned.
 *
 * mvp_task_metrics: pred, target fp32 [B, C, HW], valid as above -> out fp64 [B, C, 5] =
 *   (sum absrel * v, sum v, n(ratio < t1), n(ratio < t2), n(ratio < t3)), v the mask as 0.0 / 1.0; a pixel is counted iff valid and
 *   ratio < t.  Every fp32 tensor operation of the reference is one separately rounded fp32 operation here (no FMA); the terms are
 *   widened to fp64 before they are summed.
 *   MVP_TASK_METRICS_CURVATURE (evaluate_curvature_absrel): p = clamp(pred, -1, 1) (NaN stays), absrel = |p - g| / |g + 1e-6f|,
 *       ratio = max(p / g, g / p), NaN if either quotient is; negative ratios count (a quirk of the reference).
 *   MVP_TASK_METRICS_RESHADING (evaluate_reshading_absrel_and_delta): p = pred * v, t = target * v, absrel = |p - t| / (t + 1e-6f),
 *       ratio = max(p / (t + 1e-6f), t / (p + 1e-6f)).
 *   absrel is MULTIPLIED by v: a non-finite value at an invalid pixel makes the image's sum NaN, as in the reference.
 *   MVP_EINVAL: a NULL pointer, B, C or HW <= 0, B * C > 1024, Cm not 1 or C, an unknown form, workspace_bytes <
 *   MVP_TASK_WORKSPACE_BYTES, workspace or out not 8-byte aligned.
 * ---------------------------------------------------------------------------------- */
#define MVP_TASK_WORKSPACE_BYTES 40960 /* 1024 partial rows x 5 fp64 */
#define MVP_TASK_METRICS_CURVATURE 0
#define MVP_TASK_METRICS_RESHADING 1
typedef struct mvp_task_prepare_args mvp_task_prepare_args;
struct mvp_task_prepare_args {
  const void* target_raw; const uint8_t* mask_raw; float* target; uint8_t* valid;
  int B, H, W, Cs, Ct, bits;
  float clamp_max;
};
int mvp_task_prepare(const mvp_task_prepare_args*, void* stream);

typedef struct mvp_masked_l1_args mvp_masked_l1_args;
struct mvp_masked_l1_args {
  const float* pred; const float* target; const uint8_t* valid; float* loss; float* grad_pred;
  void* workspace; int64_t workspace_bytes;
  int B, C, Cm; int64_t HW;
};
int mvp_masked_l1_fwd_bwd(const mvp_masked_l1_args*, void* stream);

typedef struct mvp_task_metrics_args mvp_task_metrics_args;
struct mvp_task_metrics_args {
  const float* pred; const float* target; const uint8_t* valid; double* out;
  void* workspace; int64_t workspace_bytes;
  int B, C, Cm; int64_t HW;
  int form;
  float t1, t2, t3;
};
int mvp_task_metrics(const mvp_task_metrics_args*, void* stream);

/* ------------------------------------------------------------------------------------
 * Range scan of an fp16-form pair operand (added within ABI 8; a new export with its own tagged argument struct, no existing struct
 * changed).  No reference counterpart: the reference computes in fp32.  Under MVP_PREC_F16X2 the kernels that write activation pairs and
 * Q / K (LayerNorm, attention, the GEMM epilogues, mvp_swiglu_fwd, mvp_rope2d_qkv, mvp_relpos_terms) saturate the hi half at +-65504
 * instead of overflowing, so an operand that left fp16's range gives a finite, wrong result.  This pass reads the hi halves of
 * columns [col0, col0 + cols) of `rows` rows, 16 bytes per lane, at read rate, and writes nothing but the record:
 *   record[0]  max over the scanned elements of bits & 0x7FFF  (atomic max: the fp16 magnitude order; NaN > inf > 65504)
 *   record[1] += number with bits & 0x7FFF == 0x7BFF           (|v| = 65504: saturated, or exactly representable — not told apart)
 *   record[2] += number with bits & 0x7FFF >= 0x7C00           (inf or NaN)
 *   record[3] += number scanned, mod 2^32                      (rows * cols per call)
 * The caller zeroes the record; calls accumulate into it (several operands, or several launches, may share one).  Only hi is read: lo
 * may be bf16 (the V third of qkv) and cannot saturate unless hi did.  Words outside the window — the gap up to ld, the lo blocks of
 * the interleaved layout — are never loaded.  One atomic max and up to three atomic adds on unsigned per workgroup (an add of zero is
 * left out), at most 256 workgroups: integer max and add commute, so the record is bit-reproducible.
 * MVP_EINVAL before any launch: a NULL pointer, rows < 1, cols < 8, col0 < 0, col0 / cols / ld not multiples of 8, hi not 16-byte or
 * record not 4-byte aligned, a window that ends beyond ld, an unknown layout, rows * cols / 8 >= 2^31.
 * ---------------------------------------------------------------------------------- */
typedef struct mvp_f16_scan_args mvp_f16_scan_args;
struct mvp_f16_scan_args {
  const mvp_bf16* hi;  /* MVP_PAIR_SEPARATE: the hi array [rows, ld]; MVP_PAIR_A_ILV32: the one array, hi | lo interleaved per 32 columns */
  uint32_t* record;    /* 4 words on the device, accumulated into                                                                        */
  int rows;
  int col0, cols;      /* the window of pair columns, each % 8 == 0                                                                      */
  int ld;              /* row stride of the STORED array in 16-bit words, % 8 == 0 (MVP_PAIR_A_ILV32: twice the pair's column count)      */
  int layout;          /* MVP_PAIR_SEPARATE or MVP_PAIR_A_ILV32                                                                          */
};
int mvp_f16_range_scan(const mvp_f16_scan_args*, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MVP_HIP_H */
