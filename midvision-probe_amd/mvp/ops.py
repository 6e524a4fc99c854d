"""Tensor-level wrappers over the C ABI (one function per entry point).

A "pair" is a tuple ``(hi, lo)`` of torch.bfloat16 tensors with value hi + lo; ``lo`` is
None in MVP_PREC_BF16 mode.  All tensors must live on the current HIP device; outputs are
allocated by the caller (or by these helpers with torch.empty — plumbing only).
"""
from __future__ import annotations

import ctypes
import functools
from typing import Optional, Tuple

import torch

from . import lib, pipeline
from .lib import PREC_BF16, PREC_BF16X3

Pair = Tuple[torch.Tensor, Optional[torch.Tensor]]


class IlvPair:
    """A bf16 pair stored as ONE array, hi | lo interleaved per 32 columns (MVP_PAIR_A_ILV32, include/mvp_hip.h): ``t`` is
    [rows, 2 * cols] bf16.  LayerNorm, attention and the GEMM epilogue write it, the large-M GEMM kernel reads it as its A operand
    (a 32-deep k-step of a row is then one whole 128-byte line)."""

    def __init__(self, rows: int, cols: int, device):
        if cols % 32:
            raise lib.MvpError("an interleaved pair needs cols % 32 == 0")
        self.rows, self.cols = rows, cols
        self.t = torch.empty(rows, 2 * cols, dtype=torch.bfloat16, device=device)

    def separate(self) -> Pair:
        """The same values as two [rows, cols] arrays (tests)."""
        v = self.t.view(self.rows, self.cols // 32, 2, 32)
        return v[:, :, 0].reshape(self.rows, self.cols).contiguous(), v[:, :, 1].reshape(self.rows, self.cols).contiguous()

# Optional per-launch timing hook used by bench.py's roofline leg: when a list is installed,
# every GEMM / attention launch is bracketed by HIP events recorded on the launch stream.
_TRACE = None


def set_trace(lst) -> None:
    global _TRACE
    _TRACE = lst


def _traced(kind: str, tile: str, precision: int, work: float, fn) -> None:
    """Run ``fn`` bracketed by HIP events on the launch stream when bench.py has installed a trace list
    (``work`` = algorithmic flops for MFMA-bound kernels, algorithmic HBM bytes for memory-bound ones)."""
    if _TRACE is None:
        fn()
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    _TRACE.append((kind, tile, precision, work, e0, e1))


@functools.lru_cache(maxsize=None)
def _route_label(M: int, N: int, K: int, precision: int, splitk: int, tile_policy: int, a_ilv: bool = False, ext: bool = False) -> str:
    """The kernel mvp_gemm_bias_act_res runs for a linear GEMM of this form (mvp_gemm_route: the library's rule, csrc/gemm.hip), "" where
    it would refuse the arguments.  ``a_ilv``: interleaved A operand; ``ext``: an EXT epilogue (an output mask stands for all of them).
    Operands are stand-ins: the query only tests pointers for NULL.  (Memoized: the library reads its overrides once per process.)"""
    a = lib.GemmArgs(a_hi=16, a_lo=16, w_hi=16, w_lo=16, out_f32=16, out_hi=16, out_lo=16, M=M, N=N, K=K, lda=2 * K if a_ilv else K, ldw=K,
                     ldr=N, ldo=N, ldob=N, precision=precision, splitk=splitk, tile_policy=tile_policy,
                     pair_layout=lib.PAIR_A_ILV32 if a_ilv else lib.PAIR_SEPARATE, out_mask=16 if ext else None, ldm=N)
    r = lib.GemmRoute()
    if lib.load().mvp_gemm_route(ctypes.byref(a), ctypes.byref(r)) != 0:
        return ""
    if r.family == lib.ROUTE_PP:
        return f"pp {r.bm}, {r.bn}, {r.bk}, {r.split}"
    return f"{r.bm}, {r.bn}, {r.bk}, {r.split}, {r.nstage}" + (", splitk" if r.family == lib.ROUTE_SPLITK else "")


def gemm_tile(M: int, N: int, K: int = 0, precision: int = PREC_BF16X3, splitk: int = 1, tile_policy: int = 0) -> str:
    """The kernel of a plain linear GEMM: "pp 256, 256, 32, SPLIT" (the large-M kernel) or the tile kernel's template arguments
    "BM, BN, BK, SPLIT, NSTAGE" (+ ", splitk")."""
    label = _route_label(M, N, K, precision, splitk, tile_policy)
    if not label:
        raise lib.MvpError(f"mvp_gemm_route: no kernel takes M={M} N={N} K={K} precision={precision} splitk={splitk}")
    return label


def _chk(t: torch.Tensor, dtype, name: str):
    if t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
        raise lib.MvpError(f"{name}: expected contiguous {dtype} device tensor, got {t.dtype} {t.device} contiguous={t.is_contiguous()}")


def _v_format(who: str, v_f16: bool, qk_f16: bool) -> int:
    """mvp_attention_args.v_format of the (v_f16, qk_f16) a wrapper was given."""
    if qk_f16 and not v_f16:
        raise lib.MvpError(f"{who}: qk_f16 needs v_f16 (mvp_attention_args.v_format = MVP_ATT_V_F16_QK_F16)")
    return (lib.ATT_V_F16_QK_F16 if qk_f16 else lib.ATT_V_F16) if v_f16 else lib.ATT_V_BF16_PAIR


def empty_pair(shape, precision: int, device) -> Pair:
    hi = torch.empty(shape, dtype=torch.bfloat16, device=device)
    lo = torch.empty(shape, dtype=torch.bfloat16, device=device) if precision == PREC_BF16X3 else None
    return hi, lo


def zeros_pair(shape, precision: int, device) -> Pair:
    hi = torch.zeros(shape, dtype=torch.bfloat16, device=device)
    lo = torch.zeros(shape, dtype=torch.bfloat16, device=device) if precision == PREC_BF16X3 else None
    return hi, lo


def split_bf16(src: torch.Tensor, precision: int = PREC_BF16X3) -> Pair:
    src = src.contiguous()
    _chk(src, torch.float32, "split_bf16.src")
    hi, lo = empty_pair(src.shape, precision, src.device)
    a = lib.SplitArgs(lib.ptr(src), lib.ptr(hi), lib.ptr(lo), src.numel())
    lib.call("mvp_split_bf16", a)
    return hi, lo


F16X2_S = 2.0 ** -6  # the share of the hi product that PREC_F16X2 moves into the lo product (include/mvp_hip.h, MVP_PREC_F16X2)


def f16x2_weight(w: torch.Tensor) -> Pair:
    """The weight operand of a PREC_F16X2 GEMM (include/mvp_hip.h): hi = fp16((1 - s) w), lo = fp16((w + d / s) / 8) with
    d = (1 - s) w - hi — fp16 bits in bf16-typed arrays, like every pair half of this library.  fp64 arithmetic: one rounding each."""
    w = w.detach().double().contiguous()
    t = (1.0 - F16X2_S) * w
    hi = t.clamp(-65504.0, 65504.0).to(torch.float16)
    lo = ((w + (t - hi.double()) / F16X2_S) / 8.0).clamp(-65504.0, 65504.0).to(torch.float16)
    return hi.view(torch.bfloat16).contiguous(), lo.view(torch.bfloat16).contiguous()


def split_f16_comp(src: torch.Tensor) -> Pair:
    """fp32 -> the activation pair of a PREC_F16X2 GEMM: hi = fp16(x), lo = fp16(8 (x - hi) + hi / 8), both saturating at +-65504
    (bits in bf16-typed arrays).  (torch ops: tests and one-off conversions; the kernels write this form themselves.)"""
    x = src.float()
    hi = x.clamp(-65504.0, 65504.0).half()
    h = hi.float()
    lo = ((x - h) * 8.0 + h * 0.125).clamp(-65504.0, 65504.0).half()
    return hi.view(torch.bfloat16).contiguous(), lo.view(torch.bfloat16).contiguous()


def split_f16_bf16(src: torch.Tensor) -> Pair:
    """fp32 -> hi = fp16(x) (bits in a bf16-typed array, saturating), lo = bf16(x - hi): the form of the V third under
    ``gemm(..., f16_col0=2 * H * 64)``.  (torch ops: tests.)"""
    x = src.float()
    hi = x.clamp(-65504.0, 65504.0).half()
    return hi.view(torch.bfloat16).contiguous(), (x - hi.float()).bfloat16().contiguous()


def interleave_pair(pair: Pair) -> Optional[torch.Tensor]:
    """(hi, lo) [R, K] -> ONE [R, 2K] bf16 array, hi | lo interleaved per 32-deep k block (MVP_PAIR_*_ILV32, include/mvp_hip.h): the
    operand layout in which a 32-deep k-step of a row is one whole 128-byte line.  Used for the frozen weights (built once at load; the
    large-M GEMM kernel reads them 2-3.5 % faster than the separate arrays).  None when K % 32 != 0 or the pair has no lo part."""
    hi, lo = pair
    if lo is None or hi.dim() != 2 or hi.shape[1] % 32:
        return None
    R, K = hi.shape
    return torch.stack((hi.view(R, K // 32, 32), lo.view(R, K // 32, 32)), dim=2).reshape(R, 2 * K).contiguous()


def patch_gather(images: torch.Tensor, out: Pair, P: int, gh: int, gw: int, pad_top: int, pad_left: int) -> None:
    _chk(images, torch.float32, "patch_gather.images")
    B, Cc, H, W = images.shape
    a = lib.PatchGatherArgs(lib.ptr(images), lib.ptr(out[0]), lib.ptr(out[1]), B, Cc, H, W, P, gh, gw, pad_top, pad_left)
    lib.call("mvp_patch_gather", a)


def patch_gather_ld(images: torch.Tensor, out: Pair, P: int, gh: int, gw: int, pad_top: int, pad_left: int, ldk: int) -> None:
    """``patch_gather`` into rows of ``ldk`` >= C*P*P elements with zeroed tail columns, any P (mvp_patch_gather_ld: DINOv2's P = 14)."""
    _chk(images, torch.float32, "patch_gather_ld.images")
    B, Cc, H, W = images.shape
    g = lib.PatchGatherArgs(lib.ptr(images), lib.ptr(out[0]), lib.ptr(out[1]), B, Cc, H, W, P, gh, gw, pad_top, pad_left)
    lib.call("mvp_patch_gather_ld", lib.PatchGatherLdArgs(g, int(ldk)))


_SPLITK_WS = {}  # (device, stream) -> zero-initialised workspace (tile counters reset themselves)


def splitk_auto(M: int, N: int, K: int) -> int:
    """Split-K factor used when the caller does not give one.  Measured on MI355X (tools/splitk_bench.py and in-step,
    bf16x3): the N = 768 projections do NOT profit (proj 27.1 us unsplit vs 33.6 at S=2; fc2 71.8 vs 77.3): they are
    bound by the L2->LDS operand path, not by tile imbalance.  The one shape that does is the probe head at small M
    (skinny N <= 256, long K, <= 128 tiles): its A operand was just written by the tap kernels and comes from HBM /
    Infinity Cache, and 4x more workgroups pull it 4x wider: 52.5 -> 40.4 us inside the step at B=16.
    (The intra-launch partial-tile hand-over was suspected when pipelined trajectories stopped reproducing the serial ones; the cause
    was elsewhere — csrc/Makefile, packed fp32 — and 1500 trajectories with this rule beside other kernel chains are bit-exact,
    tools/micro/race_hunt2.py VAR=splitk.  The hand-over carries an agent-scope release since.)"""
    if N <= 256 and K >= 2048 and ((M + 127) // 128) * ((N + 63) // 64) <= 128:
        return 4
    return 1


def _ws_key(device):
    # launches on one stream are ordered, so they may share a workspace; launches on different streams (mvp/pipeline.py) may not.
    # A pipelined forward is keyed by its SLOT, not by the stream it happens to be enqueued on: every slot's hipGraph is captured on
    # one stream and replayed on whichever stream its turn falls on, so a workspace keyed by stream would be baked into several graphs
    # that replay side by side
    if pipeline.pipelined():
        return (device, "slot", pipeline.current_slot())
    return (device, lib.stream_ptr())


def _splitk_workspace(M: int, N: int, S: int, device) -> torch.Tensor:
    need = int(lib.load().mvp_gemm_splitk_workspace_bytes(M, N, S))
    key = _ws_key(device)
    ws = _SPLITK_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _SPLITK_WS[key] = torch.zeros(max(need, 32 << 20), dtype=torch.uint8, device=device)
    return ws


def gemm(a: Pair, w: Pair, M: int, N: int, K: int, *, bias=None, residual=None, out_f32=None, out: Optional[Pair] = None,
         act: int = lib.ACT_NONE, precision: int = PREC_BF16X3, lda=None, ldw=None, ldr=None, ldo=None, ldob=None,
         row_group=0, row_group_stride=0, row_group_off=0, res_row_mod=0, act_after_res=False, out_mask=None, ldm=0,
         splitk: Optional[int] = None, residual_pair: Optional[Pair] = None,
         w_ilv: Optional[torch.Tensor] = None, f16_col0: int = 0, col_scale: Optional[torch.Tensor] = None) -> None:
    """Y = act(A Wᵀ + bias) + residual (see mvp_gemm_bias_act_res).
    col_scale: fp32 [N] LayerScale vector: Y = col_scale * act(A Wᵀ + bias) + residual in the epilogue (mvp_gemm_scaled; never split-K,
    which does not take a scale).  splitk: None = automatic, 1 = off.
    f16_col0 > 0: columns from there on of the pair output are written as hi = fp16, lo = bf16 (mvp_gemm_args.out_f16_col0: the V
    third of the fused qkv projection for ``attention(..., v_f16=True)``); f16_col0 = -1: EVERY column as the activation operand of a
    PREC_F16X2 GEMM (``split_f16_comp``'s form: fc1 -> fc2); no split-K either way.
    residual_pair: the residual as a bf16 pair (hi, lo) instead of / in addition to the fp32 ``residual``.
    w_ilv: the same weights as ``interleave_pair(w)``; handed over when the library routes the GEMM to the large-M kernel."""
    a_ilv, o_ilv = isinstance(a, IlvPair), isinstance(out, IlvPair)
    if a_ilv:
        a, lda = (a.t, None), (lda if lda is not None else 2 * K)
    if o_ilv:
        out, ldob = (out.t, None), (ldob if ldob is not None else 2 * N)
    o_hi, o_lo = out if out is not None else (None, None)
    args = lib.GemmArgs(
        lib.ptr(a[0]), lib.ptr(a[1]), lib.ptr(w[0]), lib.ptr(w[1]), lib.ptr(bias), lib.ptr(residual),
        lib.ptr(out_f32), lib.ptr(o_hi), lib.ptr(o_lo), M, N, K,
        lda if lda is not None else K, ldw if ldw is not None else K,
        ldr if ldr is not None else N, ldo if ldo is not None else N, ldob if ldob is not None else N,
        act, precision, row_group, row_group_stride, row_group_off, res_row_mod)
    args.act_after_res = int(act_after_res)
    args.tile_policy = pipeline.tile_policy()
    args.pair_layout = lib.PAIR_A_ILV32 if a_ilv else lib.PAIR_SEPARATE  # (an interleaved A operand always goes to the large-M kernel)
    args.out_pair_layout = lib.PAIR_A_ILV32 if o_ilv else lib.PAIR_SEPARATE
    if f16_col0:
        args.out_f16_col0 = int(f16_col0)
        splitk = 1
    if precision == lib.PREC_F16X2:  # two products per contraction: plain linear GEMMs, no split-K (mvp_hip.h)
        splitk = 1
    if col_scale is not None:
        _chk(col_scale, torch.float32, "gemm.col_scale")
        splitk = 1
    if out_mask is not None:
        args.out_mask, args.ldm = lib.ptr(out_mask), ldm or N
    if residual_pair is not None:
        args.residual_hi, args.residual_lo = lib.ptr(residual_pair[0]), lib.ptr(residual_pair[1])
    S = 1
    plain = out_mask is None and not act_after_res and residual_pair is None
    if (a_ilv or o_ilv) and (not plain or splitk not in (None, 1)):
        raise lib.MvpError("interleaved pair operands: plain GEMMs only (no masks or split-K)")
    if plain and not a_ilv:
        S = splitk_auto(M, N, K) if splitk is None else int(splitk)
    if S > 1:
        ws = _splitk_workspace(M, N, S, a[0].device)
        args.splitk, args.splitk_ws, args.splitk_ws_bytes = S, lib.ptr(ws), ws.numel()
    tile = _route_label(M, N, K, precision, S, args.tile_policy, a_ilv, not plain) if (w_ilv is not None or _TRACE is not None) else ""
    if w_ilv is not None and tile.startswith("pp ") and ldw is None:
        args.w_hi, args.w_lo, args.ldw = lib.ptr(w_ilv), None, 2 * K
        args.pair_layout |= lib.PAIR_W_ILV32
    if col_scale is not None:
        name, args = "mvp_gemm_scaled", lib.GemmScaledArgs(args, lib.ptr(col_scale))
    else:
        name = "mvp_gemm_bias_act_res"
    _traced("gemm", tile, precision, 2.0 * M * N * K, lambda: lib.call(name, args))


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, out: Optional[Pair], M: int, Cdim: int, eps: float,
              out_f32: Optional[torch.Tensor] = None, out_f16: bool = False) -> None:
    """``out_f16``: the pair is written as the activation operand of a PREC_F16X2 GEMM (``split_f16_comp``'s form).
    ``out`` = None with ``out_f32`` set: fp32 output only; ``out_f32`` may be ``x`` itself (in place: CLIP's ln_pre)."""
    ilv = isinstance(out, IlvPair)
    if ilv:
        out = (out.t, None)
    elif out is None:
        out = (None, None)
    a = lib.LayerNormArgs(lib.ptr(x), lib.ptr(gamma), lib.ptr(beta), lib.ptr(out[0]), lib.ptr(out[1]), lib.ptr(out_f32), M, Cdim, eps,
                          lib.PAIR_A_ILV32 if ilv else lib.PAIR_SEPARATE, 1 if out_f16 else 0)
    # algorithmic HBM bytes: the fp32 row read once + the bf16 pair (or single bf16) written once
    nb = M * Cdim * (4 + (2 * (2 if (ilv or out[1] is not None) else 1) if (ilv or out[0] is not None) else 0) + (4 if out_f32 is not None else 0))
    _traced("hbm", "layernorm_kernel", 0, float(nb), lambda: lib.call("mvp_layernorm_fwd", a))


def attention(qkv: Pair, out: Pair, B: int, N: int, H: int, scale: float, precision: int, ld_qkv=None, ld_out=None, v_f16: bool = False,
              out_f16: bool = False, qk_f16: bool = False, bias: Optional[torch.Tensor] = None, ld_bias=None, bias_head_stride=None,
              rel: Optional[torch.Tensor] = None, rel_grid: Optional[Tuple[int, int]] = None) -> None:
    """``v_f16``: the V third of ``qkv`` holds hi = fp16, lo = bf16 (``gemm(..., f16_col0=2 * H * 64)``); the probabilities are then held
    as one fp16 value (mvp_attention_args.v_format = MVP_ATT_V_F16; bf16x3 only).  ``out_f16``: the output pair leaves as the activation
    operand of a PREC_F16X2 GEMM (``split_f16_comp``'s form).  ``qk_f16`` (with ``v_f16``): Q and K are the compensated fp16 pairs of
    ``gemm(..., f16_col0=-2 * H * 64)`` (activation / weight-side form) and Q.K^T runs two f16 products (MVP_ATT_V_F16_QK_F16).
    ``bias``: fp32 [H, N, ld_bias] added to the logits of every image, softmax(Q K^T * scale + bias[h]) (mvp_attention_bias_fwd; natural-log
    units; ``ld_bias`` >= 64 * ceil(N / 64), default ``bias.stride(1)``; ``bias_head_stride`` default ``bias.stride(0)``; columns >= N may hold
    anything).  None: mvp_attention_fwd, exactly as before.
    ``rel`` with ``rel_grid`` = (Kh, Kw), Kh * Kw == N: fp32 [B * H, N, ld_rel] as ``relpos_terms`` writes it; softmax(Q K^T * scale +
    rel[bh][q][k // Kw] + rel[bh][q][Kh + k % Kw]) (mvp_attention_relpos_fwd: SAM's decomposed relative-position bias, never densified)."""
    v_format = _v_format("attention", v_f16, qk_f16)
    ilv = isinstance(out, IlvPair)
    if ilv:
        out, ld_out = (out.t, None), (ld_out if ld_out is not None else 2 * H * 64)
    a = lib.AttentionArgs(lib.ptr(qkv[0]), lib.ptr(qkv[1]), lib.ptr(out[0]), lib.ptr(out[1]), B, N, H,
                          ld_qkv if ld_qkv is not None else 3 * H * 64, ld_out if ld_out is not None else H * 64, scale, precision,
                          lib.PAIR_A_ILV32 if ilv else lib.PAIR_SEPARATE, v_format, 1 if out_f16 else 0)
    if rel is not None:
        if bias is not None:
            raise lib.MvpError("attention: a dense bias and decomposed relative-position terms exclude each other")
        if rel.dtype != torch.float32 or rel.dim() != 3 or rel.stride(2) != 1 or rel_grid is None:
            raise lib.MvpError("attention: rel must be fp32 [B * H, N, ld_rel] with unit column stride, with rel_grid=(Kh, Kw)")
        ar = lib.AttentionRelposArgs(a, lib.ptr(rel), rel.stride(0), rel.stride(1), int(rel_grid[0]), int(rel_grid[1]))
        _traced("attention", "4x32q relpos", precision, 4.0 * B * H * N * N * 64, lambda: lib.call("mvp_attention_relpos_fwd", ar))
        return
    if bias is not None:
        if bias.dtype != torch.float32 or bias.dim() != 3 or bias.stride(2) != 1:
            raise lib.MvpError("attention: bias must be fp32 [H, N, ld_bias] with unit column stride")
        ab = lib.AttentionBiasArgs(a, lib.ptr(bias), bias_head_stride if bias_head_stride is not None else bias.stride(0),
                                   ld_bias if ld_bias is not None else bias.stride(1))
        _traced("attention", "4x32q bias", precision, 4.0 * B * H * N * N * 64, lambda: lib.call("mvp_attention_bias_fwd", ab))
        return
    _traced("attention", "4x32q", precision, 4.0 * B * H * N * N * 64, lambda: lib.call("mvp_attention_fwd", a))


def rope2d_qkv(qkv_f32: torch.Tensor, out: Pair, cos_tab: torch.Tensor, sin_tab: torch.Tensor, M: int, N: int, H: int, n_prefix: int,
               gh: int, gw: int, precision: int, v_f16: bool = False, qk_f16: bool = False, ld_in=None, ld_out=None) -> None:
    """2-D RoPE of the fused qkv projection (mvp_rope2d_qkv): ``qkv_f32`` [M, 3 * H * 64] fp32 (``gemm(..., out_f32=...)``) -> the pair
    ``out`` that ``attention`` reads, Q and K rotated by each token's (y, x) grid position, V passed through, every third in the form
    ``gemm(..., f16_col0=...)`` writes for the same ``v_f16`` / ``qk_f16`` (see ``attention``).  ``cos_tab`` / ``sin_tab``: fp32
    [rows >= max(gh, gw), 32], row = grid coordinate."""
    v_format = _v_format("rope2d_qkv", v_f16, qk_f16)
    _chk(cos_tab, torch.float32, "rope2d_qkv.cos_tab")
    _chk(sin_tab, torch.float32, "rope2d_qkv.sin_tab")
    if qkv_f32.dtype != torch.float32 or cos_tab.dim() != 2 or cos_tab.shape[1] != 32 or sin_tab.shape != cos_tab.shape:
        raise lib.MvpError("rope2d_qkv: fp32 projection and fp32 [rows, 32] cos / sin tables of one shape expected")
    a = lib.Rope2dQkvArgs(lib.ptr(qkv_f32), lib.ptr(out[0]), lib.ptr(out[1]), lib.ptr(cos_tab), lib.ptr(sin_tab), M, N, H, n_prefix, gh, gw,
                          int(cos_tab.shape[0]), ld_in if ld_in is not None else 3 * H * 64, ld_out if ld_out is not None else 3 * H * 64,
                          precision, v_format)
    # algorithmic HBM bytes: the fp32 projection read once, the 16-bit pair (or single bf16) written once
    nb = M * 3 * H * 64 * (4 + (4 if out[1] is not None else 2))
    _traced("hbm", "rope2d_qkv_kernel", 0, float(nb), lambda: lib.call("mvp_rope2d_qkv", a))


def relpos_terms(qkv_f32: torch.Tensor, out: Pair, rel: torch.Tensor, rh: torch.Tensor, rw: torch.Tensor, M: int, N: int, H: int, precision: int,
                 v_f16: bool = False, qk_f16: bool = False, ld_in=None, ld_out=None) -> None:
    """SAM's decomposed relative-position terms (mvp_relpos_terms): ``qkv_f32`` [M, 3 * H * 64] fp32 (``gemm(..., out_f32=...)``) ->
    ``rel`` fp32 [M // N * H, N, ld_rel], rel[bh][q][ky] = q . rh[yq][ky], rel[bh][q][Kh + kx] = q . rw[xq][kx] on the UNSCALED q, and the
    pair ``out`` that ``attention`` reads, every third in the form ``gemm(..., f16_col0=...)`` writes for the same ``v_f16`` / ``qk_f16``.
    ``rh`` fp32 [Qh, Kh, 64], ``rw`` fp32 [Qw, Kw, 64], Qh * Qw == N."""
    v_format = _v_format("relpos_terms", v_f16, qk_f16)
    _chk(rh, torch.float32, "relpos_terms.rh")
    _chk(rw, torch.float32, "relpos_terms.rw")
    if qkv_f32.dtype != torch.float32 or rh.dim() != 3 or rw.dim() != 3 or rh.shape[2] != 64 or rw.shape[2] != 64:
        raise lib.MvpError("relpos_terms: fp32 projection and fp32 [Q, K, 64] tables expected")
    if rel.dtype != torch.float32 or rel.dim() != 3 or rel.stride(2) != 1:
        raise lib.MvpError("relpos_terms: rel must be fp32 [B * H, N, ld_rel] with unit column stride")
    a = lib.RelposTermsArgs(lib.ptr(qkv_f32), lib.ptr(out[0]), lib.ptr(out[1]), lib.ptr(rel), lib.ptr(rh), lib.ptr(rw), rel.stride(0), M, N, H,
                            int(rh.shape[0]), int(rw.shape[0]), int(rh.shape[1]), int(rw.shape[1]),
                            ld_in if ld_in is not None else 3 * H * 64, ld_out if ld_out is not None else 3 * H * 64, rel.stride(1),
                            precision, v_format)
    nb = M * 3 * H * 64 * (4 + (4 if out[1] is not None else 2)) + M * H * (rh.shape[1] + rw.shape[1]) * 4
    _traced("hbm", "relpos_terms_kernel", 0, float(nb), lambda: lib.call("mvp_relpos_terms", a))


def gather_rows(src, dst, idx: torch.Tensor, rows_in: int, cols: int, ld_in=None, ld_out=None) -> None:
    """dst[r] = src[idx[r]] if idx[r] >= 0 else 0 for r < len(idx) (mvp_gather_rows): a bit copy of ``cols`` 16-bit elements per row of a
    pair (hi, lo) — lo may be None on both sides — or of an ``IlvPair`` (then ``cols`` counts the pair's columns; both sides interleaved)."""
    if isinstance(src, IlvPair) != isinstance(dst, IlvPair):
        raise lib.MvpError("gather_rows: source and destination must have the same pair form")
    if isinstance(src, IlvPair):
        src, dst, cols = (src.t, None), (dst.t, None), 2 * cols
    if idx.dtype != torch.int32 or not idx.is_contiguous():
        raise lib.MvpError("gather_rows: idx must be a contiguous int32 tensor")
    a = lib.GatherRowsArgs(lib.ptr(src[0]), lib.ptr(src[1]), lib.ptr(dst[0]), lib.ptr(dst[1]), lib.ptr(idx), int(idx.numel()), int(rows_in), int(cols),
                           ld_in if ld_in is not None else cols, ld_out if ld_out is not None else cols)
    nb = idx.numel() * cols * 2 * (2 if src[1] is not None else 1) * 2
    _traced("hbm", "gather_rows_kernel", 0, float(nb), lambda: lib.call("mvp_gather_rows", a))


def cls_rows(cls: torch.Tensor, pos0: torch.Tensor, x: torch.Tensor, B: int, N: int, Cdim: int) -> None:
    lib.call("mvp_cls_rows", lib.ClsRowsArgs(lib.ptr(cls), lib.ptr(pos0), lib.ptr(x), B, N, Cdim))


def prefix_rows(cls: torch.Tensor, pos0: torch.Tensor, reg: Optional[torch.Tensor], x: torch.Tensor, B: int, N: int, Cdim: int) -> None:
    """x[b, 0] = cls + pos0 and x[b, 1 + r] = reg[r] (register tokens, no position embedding) in one launch (mvp_prefix_rows)."""
    R = 0 if reg is None else int(reg.shape[0])
    lib.call("mvp_prefix_rows", lib.PrefixRowsArgs(lib.ptr(cls), lib.ptr(pos0), lib.ptr(reg), lib.ptr(x), B, N, Cdim, R))


def bn_tokens_workspace_bytes(M: int, Cdim: int) -> int:
    return int(lib.load().mvp_bn_tokens_workspace_bytes(M, Cdim))


def bn_tokens_to_nchw(x, B, N, Cdim, hw, *, workspace, stats=None, gamma=None, beta=None, running_mean=None, running_var=None,
                      nchw=None, tok: Optional[Pair] = None, ld_tok=0, col_off=0, tokT: Optional[Pair] = None, ldT=0,
                      eps=1e-5, momentum=0.1, mode=0, cls_out=None, num_batches_tracked=None, defer_running=False,
                      groups=1, stats_gstride=0, nchw_gstride=0, tok_gstride=0, cls_gstride=0) -> None:
    """``defer_running`` (mode 0): the running statistics and the step counter are left alone, ``stats`` ([3*C]) also receives the
    unbiased variance, and ``bn_running_update`` applies the momentum update later (forwards in flight on several streams).
    ``groups`` = G > 1: ``x`` holds G stacked batches of B images; every batch is normalised with its own statistics in the same three
    launches, outputs at the given element strides between batches (mvp_bn_tokens_args.groups)."""
    t_hi, t_lo = tok if tok is not None else (None, None)
    tt_hi, tt_lo = tokT if tokT is not None else (None, None)
    a = lib.BnTokensArgs(lib.ptr(x), lib.ptr(gamma), lib.ptr(beta), lib.ptr(running_mean), lib.ptr(running_var), lib.ptr(stats),
                         lib.ptr(nchw), lib.ptr(t_hi), lib.ptr(t_lo), ld_tok, col_off, lib.ptr(tt_hi), lib.ptr(tt_lo), ldT,
                         lib.ptr(workspace), workspace.numel() * workspace.element_size(), B, N, Cdim, hw, eps, momentum, mode, lib.ptr(cls_out),
                         lib.ptr(num_batches_tracked) if mode == 0 else None, int(bool(defer_running) and mode == 0),
                         int(groups), int(stats_gstride), int(nchw_gstride), int(tok_gstride), int(cls_gstride))
    # algorithmic HBM bytes: x read twice in train mode (statistics, apply), NCHW fp32 + token-major pair written
    M = B * N * max(1, int(groups))
    B = B * max(1, int(groups))
    nb = M * Cdim * 4 * (2 if mode == 0 else 1) + B * hw * Cdim * ((4 if nchw is not None else 0) + (4 if tok is not None and tok[1] is not None else (2 if tok is not None else 0)))
    _traced("hbm", "bn_tokens (partial+finalize+apply)", 0, float(nb), lambda: lib.call("mvp_bn_tokens_to_nchw_fwd", a))


def bn_running_update(stats, running_mean, running_var, num_batches_tracked, Cdim, momentum=0.1) -> None:
    """The deferred running-statistics update of a ``bn_tokens_to_nchw(..., defer_running=True)`` call (same bits as the fused form)."""
    lib.call("mvp_bn_running_update", lib.BnRunningUpdateArgs(lib.ptr(stats), lib.ptr(running_mean), lib.ptr(running_var),
                                                               lib.ptr(num_batches_tracked), Cdim, momentum))


def bn_running_update_many(items, momentum=0.1) -> None:
    """``bn_running_update`` for several BatchNorm modules — items of (stats, running_mean, running_var, num_batches_tracked, Cdim) — in
    one launch per lib.BN_RUNNING_MAX of them (mvp_bn_running_update_n; element-wise the same bits)."""
    if len({it[1].data_ptr() for it in items}) != len(items):  # one module tapped twice: its updates are ordered, one launch each
        for st, rm, rv, nbt, Cdim in items:
            bn_running_update(st, rm, rv, nbt, Cdim, momentum)
        return
    for i0 in range(0, len(items), lib.BN_RUNNING_MAX):
        part = items[i0:i0 + lib.BN_RUNNING_MAX]
        arr = (lib.BnRunningUpdateArgs * len(part))(*[
            lib.BnRunningUpdateArgs(lib.ptr(st), lib.ptr(rm), lib.ptr(rv), lib.ptr(nbt), Cdim, momentum) for st, rm, rv, nbt, Cdim in part])
        lib.check(lib.load().mvp_bn_running_update_n(arr, len(part), lib.stream_ptr()), "mvp_bn_running_update_n")


def pack_nchw_tokens(nchw: torch.Tensor, B: int, Cdim: int, hw: int, *, tok: Optional[Pair] = None, ld_tok=0, col_off=0,
                     tokT: Optional[Pair] = None, ldT=0) -> None:
    t_hi, t_lo = tok if tok is not None else (None, None)
    tt_hi, tt_lo = tokT if tokT is not None else (None, None)
    a = lib.PackNchwArgs(lib.ptr(nchw), lib.ptr(t_hi), lib.ptr(t_lo), ld_tok, col_off, lib.ptr(tt_hi), lib.ptr(tt_lo), ldT, B, Cdim, hw)
    lib.call("mvp_pack_nchw_tokens", a)


def resize(src: torch.Tensor, dst: torch.Tensor, planes: int, Hi: int, Wi: int, Ho: int, Wo: int, mode: int, *, align_corners=False,
           channels_last=False, Cdim=0, scale_h=0.0, scale_w=0.0, backward=False) -> None:
    """forward: src [.,Hi,Wi] -> dst [.,Ho,Wo];  backward: src = grad_out [.,Ho,Wo] -> dst = grad_in [.,Hi,Wi]."""
    a = lib.ResizeArgs(lib.ptr(src), lib.ptr(dst), planes, Hi, Wi, Ho, Wo, mode, int(align_corners), int(channels_last), Cdim, scale_h, scale_w)
    lib.call("mvp_resize_bwd" if backward else "mvp_resize_fwd", a)


def depth_predict_fwd(logits, depth, inv_sum, P, K, min_depth, max_depth, kind) -> None:
    a = lib.DepthPredictArgs(lib.ptr(logits), lib.ptr(depth), lib.ptr(inv_sum), None, None, P, K, min_depth, max_depth, kind)
    lib.call("mvp_depth_predict_fwd", a)


def depth_predict_bwd(logits, depth, inv_sum, grad_depth, grad_logits, P, K, min_depth, max_depth, kind) -> None:
    a = lib.DepthPredictArgs(lib.ptr(logits), lib.ptr(depth), lib.ptr(inv_sum), lib.ptr(grad_depth), lib.ptr(grad_logits), P, K, min_depth, max_depth, kind)
    lib.call("mvp_depth_predict_bwd", a)


def depth_loss_workspace_bytes(B: int, HW: int) -> int:
    return int(lib.load().mvp_depth_loss_workspace_bytes(B, HW))


def depth_loss(pred, target, loss, grad_pred, workspace, B, HW, w_sig=10.0, w_grad=0.5, max_depth=10.0, eps=1e-3, sigma=0.85) -> None:
    a = lib.DepthLossArgs(lib.ptr(pred), lib.ptr(target), lib.ptr(loss), lib.ptr(grad_pred), lib.ptr(workspace),
                          workspace.numel() * workspace.element_size(), B, HW, w_sig, w_grad, max_depth, eps, sigma)
    # algorithmic HBM bytes: pred + target read, gradient written (one pass each)
    _traced("hbm", "depth_loss (dlf_stats+dlf_grad)" if B <= 16 else "depth_loss (dl_stats+dl_pairs+dl_finalize+dl_grad)", 0, float(B * HW * 12), lambda: lib.call("mvp_depth_loss_fwd_bwd", a))


def angular_loss(pred, gt, mask_u8, loss, grad_pred, workspace, B, Cp, HW, eps=1e-4) -> None:
    a = lib.AngularLossArgs(lib.ptr(pred), lib.ptr(gt), lib.ptr(mask_u8), lib.ptr(loss), lib.ptr(grad_pred), lib.ptr(workspace),
                            workspace.numel() * workspace.element_size(), B, Cp, HW, eps)
    lib.call("mvp_angular_loss_fwd_bwd", a)


def colsum(x, out, M, N, ld=None, accumulate=False, workspace=None) -> None:
    if workspace is None:
        workspace = torch.empty(int(lib.load().mvp_colsum_workspace_bytes(M, N)) // 4 + 4, dtype=torch.float32, device=x.device)
    lib.call("mvp_colsum", lib.ColsumArgs(lib.ptr(x), lib.ptr(out), M, N, ld if ld is not None else N, int(accumulate),
                                          lib.ptr(workspace), workspace.numel() * workspace.element_size()))


def adamw_step(param, grad, exp_avg, exp_avg_sq, hyper, n, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, grad_scale=1.0,
               lr=0.0, bias_c1=0.0, bias_c2=0.0) -> None:
    """hyper: device tensor {lr, 1-beta1^t, 1-beta2^t} or None (then lr / bias_c1 / bias_c2 go by value)."""
    a = lib.AdamWArgs(lib.ptr(param), lib.ptr(grad), lib.ptr(exp_avg), lib.ptr(exp_avg_sq), lib.ptr(hyper), n, beta1, beta2, eps, weight_decay, grad_scale,
                      lr, bias_c1, bias_c2)
    lib.call("mvp_adamw_step", a)


def corr_argmax(src_feat, tgt_feat, kp_xy, out_xy, out_val, workspace, Cdim, h, w, K, heat_out=None) -> None:
    a = lib.CorrArgmaxArgs(lib.ptr(src_feat), lib.ptr(tgt_feat), lib.ptr(kp_xy), lib.ptr(out_xy), lib.ptr(out_val), lib.ptr(workspace),
                           workspace.numel() * workspace.element_size(), Cdim, h, w, K, lib.ptr(heat_out))
    lib.call("mvp_corr_argmax", a)


def knn_ratio(src_feat, tgt_feat, src_valid, tgt_valid, nn_idx, dist, weight, n_valid, workspace, Cdim, N0, N1) -> None:
    """Top-2 cosine nearest neighbours of every valid query among the valid targets + the ratio-test weight (include/mvp_hip.h)."""
    a = lib.KnnRatioArgs(lib.ptr(src_feat), lib.ptr(tgt_feat), lib.ptr(src_valid), lib.ptr(tgt_valid), lib.ptr(nn_idx), lib.ptr(dist),
                         lib.ptr(weight), lib.ptr(n_valid), lib.ptr(workspace), workspace.numel() * workspace.element_size(), Cdim, N0, N1)
    lib.call("mvp_knn_ratio", a)


def pointcloud_sample(feat, pc, K, out, valid, Cdim, fh, fw, N, H, W, ld_out) -> None:
    """Zero-padded bilinear samples of feat [C, fh, fw] at the projections of pc [N, 3] -> out [C, ld_out] (include/mvp_hip.h)."""
    a = lib.PointcloudSampleArgs(lib.ptr(feat), lib.ptr(pc), lib.ptr(K), lib.ptr(out), lib.ptr(valid), Cdim, fh, fw, N, H, W, ld_out)
    lib.call("mvp_pointcloud_sample", a)


def twoafc_workspace_bytes(B: int, Cdim: int, HW: int) -> int:
    return int(lib.load().mvp_twoafc_workspace_bytes(B, Cdim, HW))


def twoafc_score(ref, left, right, sim, pred, workspace, B, Cdim, HW, ld, label=None, counts=None, accumulate=False) -> None:
    """sim [B, 2] / pred [B] int32 of B triplets of [C, HW] fp32 images ld elements apart, and (with label [B]) the TP / FP / FN / TN in
    counts [4] int64, overwritten or added to (include/mvp_hip.h: mvp_twoafc_score).  ref / left / right may be slices of one tensor."""
    a = lib.TwoafcArgs(lib.ptr(ref), lib.ptr(left), lib.ptr(right), lib.ptr(label), lib.ptr(sim), lib.ptr(pred), lib.ptr(counts),
                       lib.ptr(workspace), workspace.numel() * workspace.element_size(), ld, B, Cdim, HW, int(accumulate))
    _traced("hbm", "twoafc_score", 0, float(3 * B * Cdim * HW * 4), lambda: lib.call("mvp_twoafc_score", a))


PIXEL_METRICS = {"psnr": 0, "ssim": 1}  # mvp_pixel_score_args.metric


def pixel_score_workspace_bytes(B: int, Cdim: int, H: int, W: int, metric: str) -> int:
    return int(lib.load().mvp_pixel_score_workspace_bytes(B, Cdim, H, W, PIXEL_METRICS[metric]))


def pixel_score(ref, left, right, sim, pred, workspace, B, Cdim, H, W, ld, metric, label=None, counts=None, accumulate=False) -> None:
    """sim [B, 2] / pred [B] int32 of B triplets of [C, H, W] fp32 images ld elements apart under ``metric`` ("psnr": 10 log10(1 / mse),
    peak 1; "ssim": the reference's 11 x 11 Gaussian SSIM), and (with label [B]) the TP / FP / FN / TN in counts [4] int64, overwritten or
    added to (include/mvp_hip.h: mvp_pixel_score).  ref / left / right may be slices of one tensor."""
    a = lib.PixelScoreArgs(lib.ptr(ref), lib.ptr(left), lib.ptr(right), lib.ptr(label), lib.ptr(sim), lib.ptr(pred), lib.ptr(counts),
                           lib.ptr(workspace), workspace.numel() * workspace.element_size(), ld, B, Cdim, H, W, PIXEL_METRICS[metric],
                           int(accumulate))
    _traced("hbm", "pixel_score", 0, float(3 * B * Cdim * H * W * 4), lambda: lib.call("mvp_pixel_score", a))


def bn_act_workspace(device) -> torch.Tensor:
    """A workspace for bn_act_fwd / bn_act_bwd (MVP_BN_ACT_WORKSPACE_BYTES of fp64 partials)."""
    return torch.empty(lib.BN_ACT_WORKSPACE_BYTES // 8, dtype=torch.float64, device=device)


def _bn_act_args(x, B, HW, Cdim, ld, act, training, *, y=None, gamma=None, beta=None, running_mean=None, running_var=None,
                 num_batches_tracked=None, stats=None, grad_y=None, grad_x=None, grad_gamma=None, grad_beta=None, workspace=None, n=0,
                 eps=1e-5, momentum=0.1, accumulate=False):
    return lib.BnActArgs(lib.ptr(x), lib.ptr(y), lib.ptr(gamma), lib.ptr(beta), lib.ptr(running_mean), lib.ptr(running_var),
                         lib.ptr(num_batches_tracked), lib.ptr(stats), lib.ptr(grad_y), lib.ptr(grad_x), lib.ptr(grad_gamma), lib.ptr(grad_beta),
                         lib.ptr(workspace), workspace.numel() * workspace.element_size() if workspace is not None else 0,
                         B, HW, Cdim, ld, int(n), eps, momentum, act, int(training), int(accumulate))


def bn_act_fwd(x, y, B, HW, Cdim, ld, act, training, **kw) -> None:
    """BatchNorm2d + activation of channels-last logits x [B*HW, ld] -> y [B, C, HW] (include/mvp_hip.h: mvp_bn_act_fwd)."""
    a = _bn_act_args(x, B, HW, Cdim, ld, act, training, y=y, **kw)
    # algorithmic HBM bytes: the C used columns read (twice when the batch statistics are taken first), y written
    work = float(B * HW * Cdim * 4 * (3 if (act == lib.BN_ACT_SIGMOID and training) else 2))
    _traced("hbm", "bn_act_fwd", 0, work, lambda: lib.call("mvp_bn_act_fwd", a))


def bn_act_bwd(x, grad_y, grad_x, B, HW, Cdim, ld, act, training, **kw) -> None:
    """grad_y [B, C, HW] -> grad_x [B*HW, ld] (+ grad_gamma / grad_beta of the sigmoid form): mvp_bn_act_bwd."""
    a = _bn_act_args(x, B, HW, Cdim, ld, act, training, grad_y=grad_y, grad_x=grad_x, **kw)
    work = float(B * HW * 4 * ((4 if act == lib.BN_ACT_SIGMOID else 2) * Cdim + ld))
    _traced("hbm", "bn_act_bwd", 0, work, lambda: lib.call("mvp_bn_act_bwd", a))


def bce_loss(pred, target, loss, grad_pred, workspace, N) -> None:
    """nn.BCELoss (mean) of pred / target [N] and its gradient (grad_pred may be None): mvp_bce_loss_fwd_bwd."""
    a = lib.BceLossArgs(lib.ptr(pred), lib.ptr(target), lib.ptr(loss), lib.ptr(grad_pred), lib.ptr(workspace),
                        workspace.numel() * workspace.element_size(), N)
    _traced("hbm", "bce_loss", 0, float(N * (12 if grad_pred is not None else 8)), lambda: lib.call("mvp_bce_loss_fwd_bwd", a))


def binary_counts(pred, gt, counts, G, n, threshold=0.5) -> None:
    """counts [G, 4] int64 = TP, FP, FN, TN of (pred > threshold) against gt in {0, 1}, pred / gt [G, n]: mvp_binary_counts."""
    a = lib.BinaryCountsArgs(lib.ptr(pred), lib.ptr(gt), lib.ptr(counts), G, n, threshold)
    _traced("hbm", "binary_counts", 0, float(G * n * 8), lambda: lib.call("mvp_binary_counts", a))


def ncut_workspace_bytes(Bimg: int, N: int) -> int:
    return int(lib.load().mvp_ncut_workspace_bytes(Bimg, N))


def ncut_affinity(feats, A, sums, workspace, Bimg, Cdim, N, ldf=None, painted=None, active=None) -> None:
    """A [Bimg, N, N] fp32 = the Gram matrix of the L2-normalised, painted-out columns of feats [Bimg, C, ldf] and sums [Bimg, 2] fp64
    (sum, sum of squares of A's entries): mvp_ncut_affinity."""
    a = lib.NcutAffinityArgs(lib.ptr(feats), lib.ptr(painted), lib.ptr(active), lib.ptr(A), lib.ptr(sums), lib.ptr(workspace),
                             workspace.numel() * workspace.element_size(), N if ldf is None else ldf, Bimg, Cdim, N)
    _traced("mfma", "ncut_affinity", 0, 2.0 * Bimg * N * N * Cdim, lambda: lib.call("mvp_ncut_affinity", a))


def ncut_threshold(A, sums, tau, bits, deg, Bimg, N, max_rounds=64, rounds=None, active=None) -> None:
    """tau [Bimg] fp64 (Lloyd's fixed point), bits [Bimg, N, ceil(N / 32)] int32 words of A > tau, deg [Bimg, N] fp64: mvp_ncut_threshold."""
    a = lib.NcutThresholdArgs(lib.ptr(A), lib.ptr(sums), lib.ptr(active), lib.ptr(tau), lib.ptr(bits), lib.ptr(deg), lib.ptr(rounds),
                              Bimg, N, max_rounds)
    _traced("hbm", "ncut_threshold", 0, float(Bimg * N * N * 4), lambda: lib.call("mvp_ncut_threshold", a))


def ncut_fiedler(bits, deg, v, lam, residual, iters, converged, Bimg, N, max_iters, r_tol, mix_tol, active=None) -> None:
    """The second-smallest generalised eigenvector of (D - W) v = lambda D v per image, solved out of LDS: mvp_ncut_fiedler."""
    a = lib.NcutFiedlerArgs(lib.ptr(bits), lib.ptr(deg), lib.ptr(active), lib.ptr(v), lib.ptr(lam), lib.ptr(residual), lib.ptr(iters),
                            lib.ptr(converged), Bimg, N, max_iters, r_tol, mix_tol)
    _traced("lds", "ncut_fiedler", 0, float(Bimg * N * N), lambda: lib.call("mvp_ncut_fiedler", a))


def ncut_partition(v, pass_mask, painted, union_mask, seed, Bimg, h, w, prev_mask=None, use_prev=False, active=None) -> None:
    """Bipartition, corner rule, seed component, rejection rule, painting and hole-filled union of one pass: mvp_ncut_partition."""
    a = lib.NcutPartitionArgs(lib.ptr(v), lib.ptr(prev_mask), lib.ptr(active), lib.ptr(pass_mask), lib.ptr(painted), lib.ptr(union_mask),
                              lib.ptr(seed), Bimg, h, w, int(use_prev))
    _traced("lds", "ncut_partition", 0, float(Bimg * h * w), lambda: lib.call("mvp_ncut_partition", a))


CRF_MODES = {"normalise": 0, "init": 1, "step": 2}  # MVP_CRF_NORMALISE / _INIT / _STEP


def crf_filter_pairs(B: int, H: int, W: int, inv_var_xy: float) -> float:
    """Pair evaluations of one mvp_crf_filter launch: the library's rule (csrc/densecrf.hip) that a 16 x 16 tile pair is skipped when its
    closest pixels already give a weight <= 2^-40; every pair of a tile pair that is not skipped is evaluated, padding included."""
    import math

    ty, tx = (H + 15) // 16, (W + 15) // 16
    cs = 0.5 * math.log2(math.e) * inv_var_xy
    gap = lambda d: max(0, d * 16 - 15)  # noqa: E731
    pairs = 0
    for dy in range(ty):
        for dx in range(tx):
            if cs * (gap(dx) ** 2 + gap(dy) ** 2) >= 40.0:
                continue
            pairs += (ty - dy) * (1 if dy == 0 else 2) * (tx - dx) * (1 if dx == 0 else 2)
    return float(B) * pairs * 256.0 * 256.0


def crf_filter(rgb, out, B, F, H, W, inv_var_xy, inv_var_rgb, *, inp=None, in_stride=None, out_stride=None, active=None) -> None:
    """out[b, f, i] = sum over all pixels j of image b of exp(-|dxy|^2 inv_var_xy / 2 - |drgb|^2 inv_var_rgb / 2) inp[b, f, j], rgb
    [B, H, W, 3] uint8, inp / out [B, >= F, H W] fp32 (inp None: the all-ones field): mvp_crf_filter.  Traced work = pair evaluations."""
    a = lib.CrfFilterArgs(lib.ptr(rgb), lib.ptr(inp), lib.ptr(active), lib.ptr(out), F * H * W if in_stride is None else in_stride,
                          F * H * W if out_stride is None else out_stride, B, F, H, W, inv_var_xy, inv_var_rgb)
    _traced("valu", "crf_filter bilateral" if inv_var_rgb > 0 else "crf_filter spatial", 0, crf_filter_pairs(B, H, W, inv_var_xy),
            lambda: lib.call("mvp_crf_filter", a))


def crf_update(mode: str, norm_g, norm_b, B, F, N, *, mask=None, ones_g=None, ones_b=None, filt_g=None, filt_b=None, q=None, x_g=None,
               x_b=None, map_out=None, stride=None, w_g=0.0, w_b=0.0, active=None) -> None:
    """The pointwise part of the dense CRF ("normalise": K·1 -> n in place; "init": Q^0 from the mask; "step": one mean-field update from
    the filtered fields), with the next filter inputs n Q and optionally the MAP bytes: mvp_crf_update."""
    a = lib.CrfUpdateArgs(lib.ptr(mask), lib.ptr(active), lib.ptr(norm_g), lib.ptr(norm_b), lib.ptr(ones_g), lib.ptr(ones_b), lib.ptr(filt_g),
                          lib.ptr(filt_b), lib.ptr(q), lib.ptr(x_g), lib.ptr(x_b), lib.ptr(map_out), F * N if stride is None else stride, N, B, F,
                          CRF_MODES[mode], w_g, w_b)
    _traced("hbm", "crf_update " + mode, 0, float(B * N * (8 if mode == "normalise" else F * 29)), lambda: lib.call("mvp_crf_update", a))


def mask_finish(map_in, ref, refined, B, F, H, W, *, kept=None, union_mask=None, stride=None, active=None) -> None:
    """refined [B, F, H W] bytes = binary_fill_holes(map), zeroed where its IoU with ref is below 0.5; union_mask [B, H W] = the hole-filled
    OR of the active passes: mvp_mask_finish (``active``: [B, F] bytes)."""
    a = lib.MaskFinishArgs(lib.ptr(map_in), lib.ptr(ref), lib.ptr(active), lib.ptr(refined), lib.ptr(kept), lib.ptr(union_mask),
                           F * H * W if stride is None else stride, B, F, H, W)
    _traced("lds", "mask_finish", 0, float(B * F * H * W), lambda: lib.call("mvp_mask_finish", a))


def dwconv7_ln(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, out, B: int, H: int, W: int,
               Cdim: int, eps: float, *, ldx: Optional[int] = None, out_f32: Optional[torch.Tensor] = None, out_f16: bool = False) -> None:
    """Depthwise 7x7 (padding 3) + LayerNorm over the channels of the channels-last fp32 map ``x`` [B, H, W, ldx] -> ``out`` (a Pair, an
    IlvPair or None) [B*H*W, C] and / or ``out_f32``: mvp_dwconv7_ln_fwd.  ``weight`` [C, 7, 7] (or the conv's [C, 1, 7, 7])."""
    ilv = isinstance(out, IlvPair)
    if ilv:
        out = (out.t, None)
    elif out is None:
        out = (None, None)
    a = lib.Dwconv7LnArgs(lib.ptr(x), lib.ptr(weight), lib.ptr(bias), lib.ptr(gamma), lib.ptr(beta), lib.ptr(out[0]), lib.ptr(out[1]),
                          lib.ptr(out_f32), B, H, W, Cdim, Cdim if ldx is None else ldx, eps, lib.PAIR_A_ILV32 if ilv else lib.PAIR_SEPARATE,
                          1 if out_f16 else 0)
    # algorithmic HBM bytes: the map read once, the pair written once
    _traced("hbm", "dwconv7_ln_kernel", 0, float(B * H * W * Cdim * 8), lambda: lib.call("mvp_dwconv7_ln_fwd", a))


def grn_workspace_bytes(B: int, HW: int, C4: int) -> int:
    return int(lib.load().mvp_grn_workspace_bytes(B, HW, C4))


def _grn_args(h, B, HW, C4, *, G=None, N=None, gamma=None, beta=None, out=None, out_f32=None, workspace=None):
    ilv = isinstance(out, IlvPair)
    if ilv:
        out = (out.t, None)
    elif out is None:
        out = (None, None)
    return lib.GrnArgs(lib.ptr(h), lib.ptr(gamma), lib.ptr(beta), lib.ptr(G), lib.ptr(N), lib.ptr(out[0]), lib.ptr(out[1]), lib.ptr(out_f32),
                       lib.ptr(workspace), workspace.numel() * workspace.element_size() if workspace is not None else 0, B, HW, C4,
                       lib.PAIR_A_ILV32 if ilv else lib.PAIR_SEPARATE)


def grn_stats(h: torch.Tensor, G: torch.Tensor, N: torch.Tensor, workspace: torch.Tensor, B: int, HW: int, C4: int) -> None:
    """G [B, C4] = the L2 norm of h [B, HW, C4] over HW, N = G / (mean_c G + 1e-6): mvp_grn_stats (ConvNeXt V2's GRN)."""
    a = _grn_args(h, B, HW, C4, G=G, N=N, workspace=workspace)
    _traced("hbm", "grn_stats", 0, float(B * HW * C4 * 4), lambda: lib.call("mvp_grn_stats", a))


def grn_apply(h: torch.Tensor, N: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, out, B: int, HW: int, C4: int,
              out_f32: Optional[torch.Tensor] = None) -> None:
    """gamma (h N) + beta + h -> ``out`` (a Pair, an IlvPair or None) and / or ``out_f32``: mvp_grn_apply."""
    a = _grn_args(h, B, HW, C4, N=N, gamma=gamma, beta=beta, out=out, out_f32=out_f32)
    _traced("hbm", "grn_apply", 0, float(B * HW * C4 * 8), lambda: lib.call("mvp_grn_apply", a))


def swiglu(h12: torch.Tensor, out, M: int, H: int, *, ld_in: Optional[int] = None, ld_out: Optional[int] = None,
           out_f32: Optional[torch.Tensor] = None, precision: int = PREC_BF16X3) -> None:
    """silu(h12[:, :H]) * h12[:, H:2H] of the fp32 ``h12`` [M, ld_in] (``gemm(..., out_f32=...)`` of DINOv2's w12) -> ``out`` (a Pair, an
    IlvPair or None) with ``ld_out`` >= H columns, the ones from H on zero, and / or ``out_f32`` [M, H]: mvp_swiglu_fwd.  ``precision``
    PREC_F16X2: the pair is the activation operand of a two-product GEMM (``split_f16_comp``'s form), else a bf16 pair."""
    ilv = isinstance(out, IlvPair)
    if ilv:
        ld_out = out.cols if ld_out is None else ld_out
        out = (out.t, None)
    elif out is None:
        out = (None, None)
    ld_in = 2 * H if ld_in is None else ld_in
    ld_out = H if ld_out is None else ld_out
    a = lib.SwigluArgs(lib.ptr(h12), lib.ptr(out[0]), lib.ptr(out[1]), lib.ptr(out_f32), M, H, ld_in, ld_out,
                       lib.PAIR_A_ILV32 if ilv else lib.PAIR_SEPARATE, 1 if precision == lib.PREC_F16X2 else 0)
    # algorithmic HBM bytes: gate and value read once, the pair (or single bf16) and the fp32 copy written once
    nb = M * H * (8 + (2 * (2 if (ilv or out[1] is not None) else 1) if out[0] is not None else 0) + (4 if out_f32 is not None else 0))
    _traced("hbm", "swiglu_kernel", 0, float(nb), lambda: lib.call("mvp_swiglu_fwd", a))


def f16_range_scan(pair, rows: int, cols: int, record: torch.Tensor, col0: int = 0) -> None:
    """Scan the fp16 ``hi`` half of columns [col0, col0 + cols) of the first ``rows`` rows of ``pair`` (a Pair — its hi array may be
    wider than the window and must have unit column stride — or an IlvPair) into ``record``, 4 uint32 words on the device that are
    accumulated into (max of bits & 0x7FFF, n at +-65504, n non-finite, n scanned): mvp_f16_range_scan.  Nothing else is written."""
    ilv = isinstance(pair, IlvPair)
    hi = pair.t if ilv else pair[0]
    if hi.dim() != 2 or hi.element_size() != 2 or not hi.is_cuda or hi.stride(1) != 1:
        raise lib.MvpError("f16_range_scan: a 2-D device array of 16-bit words with unit column stride expected")
    width = hi.shape[1] // 2 if ilv else hi.shape[1]
    if not (0 < rows <= hi.shape[0] and 0 <= col0 and 0 < cols and col0 + cols <= width):
        raise lib.MvpError(f"f16_range_scan: rows {rows}, columns [{col0}, {col0 + cols}) outside the operand of {hi.shape[0]} x {width}")
    if record.dtype not in (torch.uint32, torch.int32) or record.numel() != 4 or not record.is_cuda or not record.is_contiguous():
        raise lib.MvpError("f16_range_scan: the record is 4 contiguous uint32 words on the device")
    a = lib.F16ScanArgs(lib.ptr(hi), lib.ptr(record), rows, col0, cols, hi.stride(0), lib.PAIR_A_ILV32 if ilv else lib.PAIR_SEPARATE)
    _traced("hbm", "f16_range_scan_kernel", 0, float(rows * cols * 2), lambda: lib.call("mvp_f16_range_scan", a))


def augment_partials(B: int, device) -> torch.Tensor:
    """The [B, MVP_AUGMENT_PARTIALS] fp64 buffer augment_stats writes and augment_apply reads (no initialisation needed)."""
    return torch.empty(int(lib.load().mvp_augment_partials_bytes(B)) // 8, dtype=torch.float64, device=device).view(B, -1)


def _augment_image(image: torch.Tensor):
    """(B, H, W, image_u8) of a uint8 [B, H, W, 3] or fp32 [B, 3, H, W] image batch."""
    if image.dtype == torch.uint8 and image.dim() == 4 and image.shape[3] == 3:
        B, H, W, u8 = image.shape[0], image.shape[1], image.shape[2], 1
    elif image.dtype == torch.float32 and image.dim() == 4 and image.shape[1] == 3:
        B, H, W, u8 = image.shape[0], image.shape[2], image.shape[3], 0
    else:
        raise lib.MvpError(f"augment: image must be uint8 [B, H, W, 3] or float32 [B, 3, H, W], got {image.dtype} {tuple(image.shape)}")
    if not image.is_contiguous():
        raise lib.MvpError("augment: image must be contiguous")
    return B, H, W, u8


def augment_stats(image: torch.Tensor, params: torch.Tensor, partials: torch.Tensor) -> None:
    """Per-image partial sums of the grey value the contrast operation averages (include/mvp_hip.h: mvp_augment_stats)."""
    B, H, W, u8 = _augment_image(image)
    _chk(params, torch.int32, "params")
    _chk(partials, torch.float64, "partials")
    if params.numel() < B * 16:
        raise lib.MvpError("augment: the parameter table is too small for the batch")
    a = lib.AugmentStatsArgs(lib.ptr(image), lib.ptr(params), lib.ptr(partials), partials.numel() * 8, B, H, W, u8)
    _traced("hbm", "augment_stats", 0, float(B * H * W * (3 if u8 else 12)), lambda: lib.call("mvp_augment_stats", a))


def augment_apply(image, depth, snorm, params, partials, out_image, out_depth, out_snorm, mean, std) -> None:
    """Jitter + shared flip / rotate / resized crop + normalisation into out_image [B, 3, Ho, Wo], out_depth [B, 1, Ho, Wo] and
    out_snorm [B, 3, Ho, Wo] (snorm / out_snorm may both be None; partials None = no jitter): mvp_augment_apply."""
    B, H, W, u8 = _augment_image(image)
    _chk(params, torch.int32, "params")
    for t, name, ch in ((depth, "depth", 1), (snorm, "snorm", 3)):
        if t is not None:
            _chk(t, torch.float32, name)
            if tuple(t.shape) != (B, ch, H, W):
                raise lib.MvpError(f"augment: {name} must be [B, {ch}, H, W] = {(B, ch, H, W)}, got {tuple(t.shape)}")
    Ho, Wo = out_image.shape[-2:]
    for t, name, ch in ((out_image, "out_image", 3), (out_depth, "out_depth", 1), (out_snorm, "out_snorm", 3)):
        if t is not None:
            _chk(t, torch.float32, name)
            if tuple(t.shape) != (B, ch, Ho, Wo):
                raise lib.MvpError(f"augment: {name} must be {(B, ch, Ho, Wo)}, got {tuple(t.shape)}")
    if params.numel() < B * 16 or (partials is not None and partials.numel() * 8 < int(lib.load().mvp_augment_partials_bytes(B))):
        raise lib.MvpError("augment: the parameter table or the partials buffer is too small for the batch")
    a = lib.AugmentApplyArgs(lib.ptr(image), lib.ptr(depth), lib.ptr(snorm), lib.ptr(params), lib.ptr(partials), lib.ptr(out_image),
                             lib.ptr(out_depth), lib.ptr(out_snorm), partials.numel() * 8 if partials is not None else 0,
                             B, H, W, Ho, Wo, u8, mean[0], mean[1], mean[2], std[0], std[1], std[2])
    planes = 4 + (3 if snorm is not None else 0)
    work = float(B * H * W * (3 if u8 else 12) + B * H * W * 4 * (planes - 3) + B * Ho * Wo * 4 * planes)
    _traced("hbm", "augment_apply", 0, work, lambda: lib.call("mvp_augment_apply", a))


# --------------------------------------------------------------------------- Taskonomy probing (csrc/taskonomy.hip)
_TASK_WS_BYTES = 40960  # MVP_TASK_WORKSPACE_BYTES
TASK_METRICS_FORMS = {"curvature": 0, "reshading": 1}  # MVP_TASK_METRICS_*


def task_workspace(device) -> torch.Tensor:
    """A workspace for masked_l1 / task_metrics (MVP_TASK_WORKSPACE_BYTES of fp64 partials; no initialisation needed)."""
    return torch.empty(_TASK_WS_BYTES // 8, dtype=torch.float64, device=device)


def task_prepare(target_raw, mask_raw, target, valid, bits: int, clamp_max: float = 0.0) -> None:
    """Raw uint8 [B, H, W, Cs] (bits 8) or 16-bit [B, H, W] (bits 16; an int16 tensor holding the uint16 patterns) target and raw uint8
    [B, H, W] mask -> target fp32 [B, Ct, H, W], valid uint8 [B, 1, H, W] (include/mvp_hip.h: mvp_task_prepare)."""
    _chk(mask_raw, torch.uint8, "mask_raw")
    _chk(target_raw, torch.uint8 if bits == 8 else torch.int16, "target_raw")
    _chk(target, torch.float32, "target")
    _chk(valid, torch.uint8, "valid")
    B, H, W = mask_raw.shape
    Cs = target_raw.shape[3] if bits == 8 else 1
    Ct = target.shape[1]
    if tuple(target_raw.shape[:3]) != (B, H, W) or tuple(target.shape) != (B, Ct, H, W) or valid.numel() != B * H * W:
        raise lib.MvpError(f"task_prepare: shapes disagree: raw {tuple(target_raw.shape)}, mask {tuple(mask_raw.shape)}, "
                           f"target {tuple(target.shape)}, valid {tuple(valid.shape)}")
    a = lib.TaskPrepareArgs(lib.ptr(target_raw), lib.ptr(mask_raw), lib.ptr(target), lib.ptr(valid), B, H, W, Cs, Ct, bits, clamp_max)
    # algorithmic HBM bytes: the raw target and mask read once, the fp32 target and the byte mask written once
    work = float(B * H * W * (Cs * (bits // 8) + 1 + 4 * Ct + 1))
    _traced("hbm", "task_prepare", 0, work, lambda: lib.call("mvp_task_prepare", a))


def masked_l1(pred, target, valid, loss, grad_pred, workspace, B: int, Cdim: int, Cm: int, HW: int) -> None:
    """MaskedL1Loss of pred / target [B, C, HW] under valid uint8 [B, Cm, HW] and its gradient (grad_pred may be None):
    mvp_masked_l1_fwd_bwd."""
    a = lib.MaskedL1Args(lib.ptr(pred), lib.ptr(target), lib.ptr(valid), lib.ptr(loss), lib.ptr(grad_pred), lib.ptr(workspace),
                         workspace.numel() * workspace.element_size(), B, Cdim, Cm, HW)
    # pred, target and the mask are read twice when the gradient is written (the count comes first), once otherwise
    n = B * Cdim * HW
    work = float(2 * (8 * n + n) + 4 * n) if grad_pred is not None else float(9 * n)
    _traced("hbm", "masked_l1", 0, work, lambda: lib.call("mvp_masked_l1_fwd_bwd", a))


def task_metrics(pred, target, valid, out, workspace, B: int, Cdim: int, Cm: int, HW: int, form: str, thresholds) -> None:
    """out fp64 [B, C, 5] = (sum absrel v, sum v, n < t1, n < t2, n < t3) per image and channel: mvp_task_metrics."""
    a = lib.TaskMetricsArgs(lib.ptr(pred), lib.ptr(target), lib.ptr(valid), lib.ptr(out), lib.ptr(workspace),
                            workspace.numel() * workspace.element_size(), B, Cdim, Cm, HW, TASK_METRICS_FORMS[form],
                            thresholds[0], thresholds[1], thresholds[2])
    _traced("hbm", "task_metrics", 0, float(B * Cdim * HW * 9), lambda: lib.call("mvp_task_metrics", a))
