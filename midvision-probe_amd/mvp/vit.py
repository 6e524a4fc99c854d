"""ViT-B/16-class frozen backbone forward on the HIP kernels (DINO / iBOT / MoCo-v3 / MAE
share this engine; the wrappers under evals/models differ in weights, pos-embed policy,
LayerNorm eps and which block outputs are tapped).

DINOv2 (ViT-B/14, B/14 with registers, L/14) runs on the same engine: R register tokens follow the CLS row (n_prefix = 1 + R prefix
rows per image, written by mvp_prefix_rows), LayerScale vectors (blocks.i.ls1.gamma / ls2.gamma) are applied in the proj / fc2 epilogues
(mvp_gemm_scaled), and the 14x14 patches are gathered into zero-padded rows (mvp_patch_gather_ld) against zero-padded weights.
ViT-g/14's SwiGLU MLP (blocks.i.mlp.w12 / mlp.w3) runs as the w12 GEMM into fp32, mvp_swiglu_fwd, and the w3 GEMM in fc2's place.

BEiT v2 runs on it too: no position table, a learned relative-position bias per block expanded once into a dense [H, N, ld] array and
added to the attention logits (mvp_attention_bias_fwd; ``rel_pos_grid``), and the reference wrapper's replay pass (``replay_after_norm``).

Data layout in HBM (per batch of B images, N = n_prefix + gh*gw tokens, n_prefix = 1 + R, M = B*N rows):
  x        fp32  [M, C]      residual stream (kept fp32: LN statistics and residual adds)
  xn       bf16 pair [M, C]  LayerNorm output = A operand of the next GEMM
  qkv      bf16 pair [M, 3C] fused projection, read in place by the attention kernel
  ao       bf16 pair [M, C]  attention output (already in (B, N, H*64) order)
  hmid     bf16 pair [M, hidden] fc1+GELU output (hidden = 4C; a SwiGLU model: silu(gate) * value, hidden = H padded to a multiple of 64)
  h12      fp32  [M, 2H]     SwiGLU models only (DINOv2 ViT-g/14): the w12 projection, gate | value, read once by mvp_swiglu_fwd
  weights  bf16 pairs, torch Linear layout [N_out, K] (K contiguous) — split once at load.
Everything is allocated once per (B, gh, gw) and reused: the frozen forward allocates only
the returned NCHW maps.
"""
from __future__ import annotations

import math
import os
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import lib, ops, pipeline
from .buffers import EngineBuffers
from .lib import PREC_BF16, PREC_BF16X3


def parse_precision(p) -> int:
    """'bf16x3' (three bf16 products per contraction, ~1e-5 on the features), 'f16x2' (the four GEMMs of every block
    with two fp16 products over compensated fp16 pairs, include/mvp_hip.h MVP_PREC_F16X2; everything else as in bf16x3; the same
    ~1e-5 on the features, |activation| <= 65504), 'bf16' (one product: fails the 1e-3 feature contract).  The ViT wrappers run
    'f16x2' unless told otherwise (backbone.default_precision()); a bare ViTEngine(...) without ``precision`` is a 'bf16x3' engine.
    'f16x2' saturates silently beyond fp16's range: the wrappers' range guard (``range_guard=`` / MVP_F16_GUARD, backbone.ViTBackbone)
    audits one forward with ``RangeAudit`` and warns, raises or falls back to 'bf16x3'."""
    if p in (PREC_BF16, PREC_BF16X3, lib.PREC_F16X2):
        return p
    s = str(p).lower()
    if s in ("bf16", "fast"):
        return PREC_BF16
    if s in ("bf16x3", "x3", "exact", "fp32"):
        return PREC_BF16X3
    if s in ("f16x2", "fp16x2", "x2"):
        return lib.PREC_F16X2
    raise ValueError(f"unknown precision {p!r} (use 'bf16x3', 'f16x2' or 'bf16')")


class TapOutputs(list):
    """The list of NCHW maps a backbone returns, plus (privately) the token-major bf16
    packing of the same features that the probe-head GEMMs consume."""
    packed = None


class TapGroups(list):
    """What a GROUPED forward returns (``forward_taps(..., groups=G)``): one ``TapOutputs`` per batch of the group, in batch order."""


class PackedFeatures:
    """Token-major operand of the linear-probe GEMMs: F [Mpad, Cpad] bf16 pair (forward: F·Wᵀ by the NT GEMM;
    weight gradient: gᵀ·F by the TN split-K kernel, which reads the same row-major image through transposed LDS reads)."""

    @staticmethod
    def padded(B, h, w, Ctot):
        """(Mpad, Cpad) of a packing: NT GEMM K % 64, TN kernel Cin % 128; pad rows / columns stay zero."""
        return (B * h * w + 63) // 64 * 64, (Ctot + 127) // 128 * 128

    def __init__(self, B, h, w, Ctot, precision, device, tok=None):
        self.B, self.h, self.w, self.Ctot, self.precision = B, h, w, Ctot, precision
        self.M = B * h * w
        self.Mpad, self.Cpad = self.padded(B, h, w, Ctot)
        # ``tok``: a zero-initialised [Mpad, Cpad] pair owned by the caller (the batches of a grouped forward share one allocation)
        self.tok = tok if tok is not None else ops.zeros_pair((self.Mpad, self.Cpad), precision, device)
        self.sources: List[Tuple[int, int]] = []  # (data_ptr, _version) of the NCHW maps packed here
        self.source_refs: List[torch.Tensor] = []  # the maps themselves: while they live, their addresses cannot be recycled
        self.generation = 0  # bumped every time the buffers are rewritten (they are reused across steps)
        self.registry_key: Optional[int] = None  # where register_pack last entered this packing
        self.scratch: Dict[str, object] = {}  # per-shape scratch of the head backward (zero-padded once)

    def rewritten(self, maps: Optional[Sequence[torch.Tensor]] = None) -> None:
        """The buffers now hold the features of ``maps`` (None: of the same maps again — a graph replay, which runs none of the forward's
        host code): count the rewrite and (re-)enter the registry (an entry aged out by other pipelines' packings comes back)."""
        self.generation += 1
        register_pack(self.source_refs if maps is None else maps, self)


_PACK_REGISTRY: Dict[int, PackedFeatures] = {}
# one entry per (pipeline slot, forward shape, batch of the forward): a span pipeline keeps 2 slots x two shapes (floor / ceil of T / B
# whole batches) x up to 14 batches = 54 entries at B = 8, and a model has a train and an eval pipeline; a graph replay re-registers
# its packings (pipeline._forward), so an entry that ages out anyway comes back at its forward's next replay
ACTIVATIONS = {"gelu": lib.ACT_GELU, "quick_gelu": lib.ACT_QUICK_GELU, "gelu_tanh": lib.ACT_GELU_TANH}  # ViTEngine(act=...): after fc1
ATT_QK_DEFAULT = "auto"  # MVP_ATT_QK: "f16" = Q.K^T in two f16 products (ViTEngine.att_qk_f16), "pair" = three bf16 products, "auto" = f16 for f16x2 engines
_PACK_REGISTRY_MAX = 256


def _ver(t: torch.Tensor) -> int:
    try:
        return t._version
    except RuntimeError:  # inference tensors do not track a version counter
        return -1


def register_pack(maps: Sequence[torch.Tensor], pack: PackedFeatures) -> None:
    """The cache key is (data_ptr, _version) of each map.  The registry also KEEPS the maps (strong references, dropped at the next
    backbone forward): were they freed, the caching allocator could hand the same addresses to unrelated same-shape tensors with
    version 0 (re-uploaded cached features, clones), which would then silently alias this packing."""
    pack.sources = [(m.data_ptr(), _ver(m)) for m in maps]
    pack.source_refs = list(maps)
    # one entry per packing buffer: the probe consumes features right after the backbone, or — with several forwards in flight
    # (mvp/pipeline.py) — one entry per pipeline slot.  Entries of other engines / shapes age out beyond the newest few.
    if _PACK_REGISTRY.get(pack.registry_key) is pack:
        del _PACK_REGISTRY[pack.registry_key]
    pack.registry_key = maps[0].data_ptr()
    _PACK_REGISTRY[pack.registry_key] = pack
    while len(_PACK_REGISTRY) > _PACK_REGISTRY_MAX:
        del _PACK_REGISTRY[next(iter(_PACK_REGISTRY))]


def lookup_pack(maps: Sequence[torch.Tensor]) -> Optional[PackedFeatures]:
    """Return the packing produced alongside ``maps`` if these are still the very same
    (unmodified) buffers; ``.detach()`` in the training loop keeps data_ptr and version."""
    if not maps:
        return None
    pack = _PACK_REGISTRY.get(maps[0].data_ptr())
    if pack is None or len(pack.sources) != len(maps):
        return None
    for m, (p, v), src in zip(maps, pack.sources, pack.source_refs):
        if m.data_ptr() != p or _ver(m) != v or m.shape != src.shape or m.dtype != src.dtype or m.stride() != src.stride():
            return None
    return pack


def plan_taps(Bt: int, groups) -> Tuple[int, int, int, int]:
    """(G, B, carry, tail) of a forward over ``Bt`` images (ViTEngine.forward_taps): its taps complete G batches of B images, the first
    of them together with the ``carry`` images the previous span ended in, and leave the ``tail`` images of a cut batch to the next
    span: carry + Bt == G * B + tail.  ``groups``: G equal batches (no carry, no tail) or a ``pipeline.Span``."""
    if not isinstance(groups, pipeline.Span):
        if groups < 1 or Bt % groups:
            raise lib.MvpError(f"grouped forward: {Bt} images do not split into {groups} equal batches")
        return groups, Bt // groups, 0, 0
    B, carry = int(groups.batch), int(groups.carry)
    if B < 1 or not 0 <= carry < B:
        raise lib.MvpError(f"span forward: carry {carry} outside [0, {B})")
    G, tail = divmod(carry + Bt, B)
    if G < 1:
        raise lib.MvpError(f"span forward: {carry} + {Bt} images complete no batch of {B}")
    return G, B, carry, tail


def rel_pos_index(gh: int, gw: int) -> torch.Tensor:
    """BEiT's relative-position index for a gh x gw grid behind one class token: int64 [N, N], N = 1 + gh * gw, row = query, column = key,
    into a table of (2gh - 1)(2gw - 1) + 3 rows.  Patch tokens are row-major (p = y * gw + x); query (yq, xq) against key (yk, xk) reads
    row (yq - yk + gh - 1) * (2gw - 1) + (xq - xk + gw - 1); the last three rows are cls -> token, token -> cls and cls -> cls
    (the reference's rule: evals/models/impl_utils/beit_model.py:117-140)."""
    n = (2 * gh - 1) * (2 * gw - 1) + 3
    y, x = torch.arange(gh).repeat_interleave(gw), torch.arange(gw).repeat(gh)
    idx = torch.empty(1 + gh * gw, 1 + gh * gw, dtype=torch.int64)
    idx[1:, 1:] = (y[:, None] - y[None, :] + gh - 1) * (2 * gw - 1) + (x[:, None] - x[None, :] + gw - 1)
    idx[0, :] = n - 3
    idx[:, 0] = n - 2
    idx[0, 0] = n - 1
    return idx


def dense_rel_pos_bias(table: torch.Tensor, gh: int, gw: int, ld: Optional[int] = None) -> torch.Tensor:
    """A relative-position table [(2gh - 1)(2gw - 1) + 3, H] -> the dense fp32 [H, N, ld] array mvp_attention_bias_fwd reads
    (bias[h][q][k] = table[rel_pos_index[q][k]][h]; natural-log units, the kernel folds log2 e itself), on the CPU.  ``ld``: the padded row
    length, default 64 * ceil(N / 64); padding columns are zero (the kernel may read them and never uses them)."""
    N = 1 + gh * gw
    if table.dim() != 2 or table.shape[0] != (2 * gh - 1) * (2 * gw - 1) + 3:
        raise lib.MvpError(f"relative-position table of {tuple(table.shape)} does not belong to a {gh} x {gw} grid "
                           f"({(2 * gh - 1) * (2 * gw - 1) + 3} rows expected): re-interpolating tables to another grid is not supported")
    ld = ld if ld is not None else 64 * ((N + 63) // 64)
    t = table.detach().to("cpu", torch.float32)
    out = torch.zeros(t.shape[1], N, ld, dtype=torch.float32)
    out[:, :, :N] = t[rel_pos_index(gh, gw).reshape(-1)].reshape(N, N, -1).permute(2, 0, 1)
    return out


def check_head_dim(C: int, heads: int) -> None:
    if C != heads * 64:
        raise lib.MvpError(f"attention kernel requires head_dim 64 (C={C}, heads={heads})")


def sam_rel_pos(q_size: int, k_size: int, rel_pos: torch.Tensor) -> torch.Tensor:
    """segment_anything's ``get_rel_pos`` (image_encoder.py; transformers' SamVisionAttention.get_rel_pos is the same code) followed by the
    gather: a table [L, 64] -> fp32 [q_size, k_size, 64], R[q][k] = the table row of the relative position of query coordinate q and key
    coordinate k.  On the CPU in fp32 with the reference's own torch expressions: linear ``F.interpolate`` to 2 * max(q, k) - 1 rows when
    the length differs, then the coordinate index with its q / k scale factors."""
    rel_pos = rel_pos.detach().to("cpu", torch.float32)
    max_rel_dist = int(2 * max(q_size, k_size) - 1)
    if rel_pos.shape[0] != max_rel_dist:
        r = F.interpolate(rel_pos.reshape(1, rel_pos.shape[0], -1).permute(0, 2, 1), size=max_rel_dist, mode="linear")
        r = r.reshape(-1, max_rel_dist).permute(1, 0)
    else:
        r = rel_pos
    q_coords = torch.arange(q_size)[:, None] * max(k_size / q_size, 1.0)
    k_coords = torch.arange(k_size)[None, :] * max(q_size / k_size, 1.0)
    relative_coords = (q_coords - k_coords) + (k_size - 1) * max(q_size / k_size, 1.0)
    return r[relative_coords.long()].contiguous()


def sam_window_index(B: int, gh: int, gw: int, w: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The row tables of SAM's window partition for B images of a gh x gw grid and w x w windows (segment_anything's window_partition /
    window_unpartition as row gathers, mvp_gather_rows), int32 on the CPU: ``part`` [B * nW * w * w] — row ((b * nWh + wy) * nWw + wx) * w * w
    + iy * w + ix of the window-major order takes token row b * gh * gw + y * gw + x with (y, x) = (wy * w + iy, wx * w + ix), or -1 (a
    zero row) where the zero-padded grid (gh, gw rounded up to multiples of w) lies outside the image; ``unpart`` [B * gh * gw] — its inverse
    on the real rows."""
    nwh, nww = -(-gh // w), -(-gw // w)
    y = (torch.arange(nwh)[:, None, None, None] * w + torch.arange(w)[None, None, :, None]).expand(nwh, nww, w, w)
    x = (torch.arange(nww)[None, :, None, None] * w + torch.arange(w)[None, None, None, :]).expand(nwh, nww, w, w)
    one = torch.where((y < gh) & (x < gw), y * gw + x, torch.full_like(y, -1)).reshape(-1)  # one image, window-major
    part = torch.where(one[None, :] >= 0, one[None, :] + torch.arange(B)[:, None] * (gh * gw), torch.full((1, 1), -1, dtype=torch.int64)).reshape(-1)
    unpart = torch.empty(B * gh * gw, dtype=torch.int64)
    live = part >= 0
    unpart[part[live]] = torch.arange(part.numel())[live]
    return part.to(torch.int32).contiguous(), unpart.to(torch.int32).contiguous()


class RangeAudit:
    """The record of one or more audited forwards of ``engine`` (``forward_taps(..., audit=...)``, ``last_block_qkv(..., audit=...)``):
    one zeroed [S, 4] uint32 device tensor, a row per site — an fp16-form operand of a block, scanned in the buffer its consumer reads,
    right before that consumer (mvp_f16_range_scan) — and the sites' names, which are the strings ``ViTEngine._check_f16_range`` uses.
    The scans run on the forward's stream without a sync and touch nothing but the record; ``read()`` is the one device-to-host copy.
    An engine without fp16-form operands ('bf16x3' without ``att_qk_f16``) has no sites: auditing it is a no-op."""

    def __init__(self, engine: "ViTEngine"):
        self.sites: List[str] = engine.audit_sites()
        self.blocks: List[int] = [int(s.split(":")[0].split()[1]) for s in self.sites]
        self._row = {s: j for j, s in enumerate(self.sites)}
        # (allocated as int32 and viewed: zero fill and copies of the unsigned types are not available in every torch build)
        self.record = torch.zeros(max(len(self.sites), 1), 4, dtype=torch.int32, device=engine.device).view(torch.uint32)[:len(self.sites)]

    def scan(self, site: str, pair, rows: int, cols: int, col0: int = 0) -> None:
        ops.f16_range_scan(pair, rows, cols, self.record[self._row[site]], col0)

    def read(self) -> List[dict]:
        """One dict(site, block, max_abs, n_sat, n_nonfinite, n_scanned) per site, in forward order (one copy, which waits for the
        stream's work as any device-to-host copy does).  ``max_abs`` is the fp16 value of the largest magnitude seen (inf / nan included)."""
        if not self.sites:
            return []
        words = (self.record.view(torch.int32).cpu().to(torch.int64) & 0xFFFFFFFF).tolist()
        out = []
        for site, blk, (mx, n_sat, n_nonf, n) in zip(self.sites, self.blocks, words):
            max_abs = float(torch.tensor([mx], dtype=torch.int32).to(torch.int16).view(torch.float16)[0])
            out.append(dict(site=site, block=blk, max_abs=max_abs, n_sat=int(n_sat), n_nonfinite=int(n_nonf), n_scanned=int(n)))
        return out


def tripped_sites(report: Sequence[dict]) -> List[dict]:
    """The rows of a ``RangeAudit.read()`` report with a saturated or non-finite element (an exactly representable 65504 counts, as in
    ``ViTEngine._check_f16_range``)."""
    return [r for r in report if r["n_sat"] + r["n_nonfinite"] > 0]


class ViTEngine:
    def __init__(self, state_dict: Dict[str, torch.Tensor], *, heads: int, patch: int = 16, ln_eps: float = 1e-6,
                 precision="bf16x3", device="cuda", pos_embed_mode: str = "dino", qkv_fused: bool = True, act: str = "gelu",
                 rope_freq: Optional[float] = None, rel_pos_grid: Optional[Tuple[int, int]] = None):
        """``state_dict`` in the DINO / timm layout; DINOv2's extras are picked up from it: ``register_tokens`` [1, R, C] (then
        n_prefix = 1 + R) and ``blocks.i.ls1.gamma`` / ``blocks.i.ls2.gamma`` (LayerScale, fused into the proj / fc2 epilogues).
        So are CLIP's and SigLIP's: ``norm_pre.weight`` / ``norm_pre.bias`` (a LayerNorm over the residual stream before block 0, in place),
        a missing ``patch_embed.proj.bias`` (bias-free patch convolution), a missing ``cls_token`` (no prefix row at all: n_prefix = 0,
        ``pos_embed`` [1, n, C] without a CLS entry).
        precision: ``parse_precision``; 'bf16x3' when not given — the wrappers always give theirs (backbone.default_precision(): 'f16x2').
        pos_embed_mode: 'dino' (bicubic with the +0.1 scale nudge), 'fixed', 'dinov2_reg' (bicubic to the grid size, antialiased:
        DINOv2's register models), or 'resize_aa' (the same resample, applied whenever the table's grid-entry COUNT differs from
        gh * gw — the reference's resize_pos_embed, evals/models/utils.py:12-52 — with or without a CLS entry).
        act: the activation after fc1: 'gelu' (erf), 'quick_gelu' (x sigmoid(1.702 x): OpenAI CLIP) or 'gelu_tanh' (SigLIP).
        A state dict with ``blocks.i.mlp.w12.weight`` [2H, C] / ``mlp.w3.weight`` [C, H] (DINOv2's SwiGLUFFNFused: ViT-g/14) makes a SwiGLU
        engine whatever ``act`` says (``act_name`` = 'swiglu'): w12 into fp32 [M, 2H], mvp_swiglu_fwd into the A operand of w3 with H padded
        to ``hidden`` = 64 * ceil(H / 64) zero columns (the GEMMs' K rule; ``w3`` is padded with zero columns once, here), w3 where fc2 runs.
        rope_freq: CroCo v2's RoPE<freq> (100.0 for the published models): Q and K of every block are rotated by the token's (y, x) grid
        position (mvp_rope2d_qkv, between the qkv GEMM — which then writes fp32 — and attention).  The state dict may then come without
        ``pos_embed`` (C is read from the patch-embedding weight and ``tokens`` adds no position residual).
        rel_pos_grid: BEiT's relative-position bias.  (gh, gw) of the ONE grid the model runs at — explicit, because a table's length does
        not determine a non-square grid; every block's ``blocks.i.attn.rel_pos_bias_table`` [(2gh - 1)(2gw - 1) + 3, H] is expanded here, on
        the CPU in fp32, into the dense [H, N, ld] array that attention adds to its logits (``dense_rel_pos_bias``; blocks with identical
        tables share one array).  Such a model may have a class token and no ``pos_embed`` (the class row is ``cls_token`` alone, the patch
        rows get no position residual), and a forward at another grid raises.  ``fc_norm.weight`` / ``fc_norm.bias`` (BEiT's final norm)
        are kept for ``forward_taps(..., replay_after_norm=True)``.
        SAM's image encoder is picked up from ``blocks.i.attn.rel_pos_h`` / ``rel_pos_w`` [2S - 1, 64] (with pos_embed_mode='sam' and a
        [1, S0, S0, C] ``pos_embed``): a block whose S equals S0 attends globally, any other inside S x S windows of the zero-padded grid
        (``_sam_attention``).  No class token, no prefix rows."""
        self.device = torch.device(device)
        self.precision = parse_precision(precision)
        # 'f16x2': a bf16x3 engine (buffers, patch embedding, attention, taps) whose four block GEMMs run two products (lib.PREC_F16X2)
        self.f16x2 = self.precision == lib.PREC_F16X2
        if self.f16x2:
            self.precision = PREC_BF16X3
        self.heads, self.patch, self.ln_eps = heads, patch, ln_eps
        self.att_v_f16 = self.precision == lib.PREC_BF16X3 and os.environ.get("MVP_ATT_V", "f16") != "pair"
        # Q.K^T as TWO f16 products over compensated fp16 pairs (Q: activation form, K: weight-side form, both written by the qkv GEMM's
        # epilogue; csrc/attention.hip, VF16 == 2) instead of three bf16 ones; MVP_ATT_QK=pair brings the bf16 pairs back
        # Default: on for an f16x2 engine (whose activations are bound to fp16's range anyway), off for bf16x3 (which keeps fp32's exponent
        # range for Q and K).  +0.4 % at 224^2, +1.3 % at 480x640 (profiles/r04_qk_ab.txt); the reference's goldens read the same 1.5e-5 ... 2.4e-5.
        qk = os.environ.get("MVP_ATT_QK", ATT_QK_DEFAULT)
        self.att_qk_f16 = self.att_v_f16 and (qk == "f16" or (qk == "auto" and self.f16x2))
        self.check_f16_range = os.environ.get("MVP_CHECK_F16_RANGE", "0") == "1"  # diagnostic: see _check_f16_range
        self.pos_embed_mode = pos_embed_mode
        if act not in ACTIVATIONS:
            raise ValueError(f"unknown activation {act!r} (use one of {sorted(ACTIVATIONS)})")
        self.act_name, self.act = act, ACTIVATIONS[act]
        sd = {k: v.detach().to(self.device, torch.float32).contiguous() for k, v in state_dict.items()}
        self.has_cls = "cls_token" in sd
        self.rope_freq = None if rope_freq is None else float(rope_freq)
        self.rel_pos_grid = None if rel_pos_grid is None else (int(rel_pos_grid[0]), int(rel_pos_grid[1]))
        if "pos_embed" not in sd and (self.rope_freq is None or self.has_cls) and self.rel_pos_grid is None:
            raise lib.MvpError("state dict without pos_embed: only a RoPE model without a class token (rope_freq=...) or a model with "
                               "relative-position bias tables (rel_pos_grid=...) has none")
        self.C = sd["cls_token"].shape[-1] if self.has_cls else sd["pos_embed"].shape[-1] if "pos_embed" in sd else sd["patch_embed.proj.weight"].shape[0]
        check_head_dim(self.C, heads)
        self.depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
        self.cls = sd["cls_token"].reshape(-1).contiguous() if self.has_cls else None
        self.pos_embed = sd.get("pos_embed")  # [1, 1+n, C] fp32 ([1, n, C] without a CLS token); None: a RoPE model without a table
        reg = sd.get("register_tokens")
        self.reg = reg.reshape(-1, self.C).contiguous() if reg is not None and reg.numel() else None  # [R, C]
        if not self.has_cls and self.reg is not None:
            raise lib.MvpError("register tokens without a cls_token: no model on this path has them")
        self.n_prefix = (1 + (0 if self.reg is None else self.reg.shape[0])) if self.has_cls else 0
        self.pre_norm = (sd["norm_pre.weight"], sd["norm_pre.bias"]) if "norm_pre.weight" in sd else None  # CLIP's ln_pre
        pw = sd["patch_embed.proj.weight"]
        self.in_chans = pw.shape[1]
        # patch-embed GEMM depth: C*P*P, padded with zero columns to what the tile kernels take (K % 32 in bf16x3, else K % 64) when the
        # patch is not a multiple of 4 or the depth is not aligned (P = 14: 588 -> 608); the gather then writes zero tails (mvp_patch_gather_ld)
        kp = pw[0].numel()
        q = 32 if self.precision == PREC_BF16X3 else 64
        self.k_patch = kp if (kp % q == 0 and patch % 4 == 0) else -(-kp // q) * q
        pw2 = pw.reshape(self.C, -1)
        if self.k_patch != kp:
            pw2 = F.pad(pw2, (0, self.k_patch - kp)).contiguous()
        self.w_patch = ops.split_bf16(pw2, self.precision)
        self.b_patch = sd.get("patch_embed.proj.bias")  # (CLIP's patch convolution has none)
        self.sam = "blocks.0.attn.rel_pos_h" in sd
        if self.sam and (self.pos_embed is None or self.pos_embed.dim() != 4 or self.pos_embed.shape[1] != self.pos_embed.shape[2]
                         or self.has_cls or pos_embed_mode != "sam" or self.rope_freq is not None or self.rel_pos_grid is not None):
            raise lib.MvpError("decomposed relative-position tables (blocks.i.attn.rel_pos_h): a SAM encoder has a square [1, S, S, C] pos_embed, "
                               "no class token and pos_embed_mode='sam'")
        self._pos_cpu = state_dict["pos_embed"].detach().to("cpu", torch.float32) if self.sam else None  # the checkpoint's table: every size resamples THIS
        self._sam_tables: List[Tuple[torch.Tensor, torch.Tensor]] = []  # distinct (rel_pos_h, rel_pos_w) on the CPU
        self._sam_rel: Dict[Tuple[int, int, int], Tuple[torch.Tensor, torch.Tensor]] = {}  # (table id, Kh, Kw) -> (Rh, Rw) on the device
        self._sam_win: Dict[Tuple[int, int, int, int], Tuple[torch.Tensor, torch.Tensor, int]] = {}  # (B, gh, gw, w) -> (part, unpart, windows)
        self.swiglu = "blocks.0.mlp.w12.weight" in sd  # DINOv2's SwiGLUFFNFused (ViT-g/14)
        if self.swiglu:
            self.act_name, self.act = "swiglu", lib.ACT_NONE
            self.swiglu_h = sd["blocks.0.mlp.w12.weight"].shape[0] // 2
            self.hidden = -(-self.swiglu_h // 64) * 64
        self.blocks = []
        self._bias_tables: List[Tuple[torch.Tensor, torch.Tensor]] = []  # (table on the CPU, its dense [H, N, ld] bias on the device)
        for i in range(self.depth):
            p = f"blocks.{i}."
            # the two MLP projections: fc1 / fc2, or a SwiGLU block's w12 / w3 in their places (w3 [C, H] zero padded to [C, hidden])
            fc1, fc2 = ("mlp.w12", "mlp.w3") if self.swiglu else ("mlp.fc1", "mlp.fc2")
            w = {"qkv_w": sd[p + "attn.qkv.weight"], "proj_w": sd[p + "attn.proj.weight"], "fc1_w": sd[p + fc1 + ".weight"], "fc2_w": sd[p + fc2 + ".weight"]}
            if self.swiglu:
                if tuple(w["fc1_w"].shape) != (2 * self.swiglu_h, self.C) or tuple(w["fc2_w"].shape) != (self.C, self.swiglu_h):
                    raise lib.MvpError(f"block {i}: mlp.w12 / mlp.w3 of {tuple(w['fc1_w'].shape)} / {tuple(w['fc2_w'].shape)}: "
                                       f"[2H, C] / [C, H] with H = {self.swiglu_h}, C = {self.C} expected")
                if self.hidden != self.swiglu_h:
                    w["fc2_w"] = F.pad(w["fc2_w"], (0, self.hidden - self.swiglu_h)).contiguous()
            blk = dict(
                n1w=sd[p + "norm1.weight"], n1b=sd[p + "norm1.bias"],
                qkv_w=ops.split_bf16(w["qkv_w"], self.precision),
                qkv_b=sd.get(p + "attn.qkv.bias"),
                proj_w=ops.split_bf16(w["proj_w"], self.precision), proj_b=sd[p + "attn.proj.bias"],
                n2w=sd[p + "norm2.weight"], n2b=sd[p + "norm2.bias"],
                fc1_w=ops.split_bf16(w["fc1_w"], self.precision), fc1_b=sd[p + fc1 + ".bias"],
                fc2_w=ops.split_bf16(w["fc2_w"], self.precision), fc2_b=sd[p + fc2 + ".bias"],
                ls1=sd.get(p + "ls1.gamma"), ls2=sd.get(p + "ls2.gamma"),  # LayerScale (DINOv2) or None
            )
            if self.f16x2:  # the weight operands of the two-product GEMMs (ops.f16x2_weight: compensated fp16 pairs)
                for n in ("qkv_w", "proj_w", "fc1_w", "fc2_w"):
                    blk[n] = ops.f16x2_weight(w[n])
            if self.precision == PREC_BF16X3:  # hi|lo-interleaved copies of the frozen weights for the large-M GEMM kernel (mvp.ops.interleave_pair)
                for n in ("qkv_w", "proj_w", "fc1_w", "fc2_w"):
                    blk[n + "_ilv"] = ops.interleave_pair(blk[n])
            if self.rel_pos_grid is not None:
                blk["att_bias"] = self._dense_bias(state_dict[p + "attn.rel_pos_bias_table"])
            if self.sam:
                th, tw = (state_dict[p + "attn.rel_pos_" + a].detach().to("cpu", torch.float32) for a in "hw")
                if th.dim() != 2 or th.shape != tw.shape or th.shape[1] != 64 or th.shape[0] % 2 == 0:
                    raise lib.MvpError(f"block {i}: rel_pos_h / rel_pos_w of {tuple(th.shape)} / {tuple(tw.shape)}: two [2S - 1, 64] tables expected")
                side = (th.shape[0] + 1) // 2
                blk["window"] = 0 if side == self.pos_embed.shape[1] else side  # 0: global attention
                blk["sam_tid"] = next((j for j, (a, b) in enumerate(self._sam_tables) if torch.equal(a, th) and torch.equal(b, tw)), len(self._sam_tables))
                if blk["sam_tid"] == len(self._sam_tables):
                    self._sam_tables.append((th, tw))
            self.blocks.append(blk)
        self.fc_norm = (sd["fc_norm.weight"], sd["fc_norm.bias"]) if "fc_norm.weight" in sd else None  # BEiT's final norm (replay_after_norm)
        self._zero_c = torch.zeros(self.C, dtype=torch.float32, device=self.device) if self.pos_embed is None and self.has_cls else None
        if not self.swiglu:
            self.hidden = self.blocks[0]["fc1_b"].numel()
        self.fc1_out = 2 * self.swiglu_h if self.swiglu else self.hidden  # columns the first MLP GEMM writes
        self._buffers = EngineBuffers()  # everything a forward reuses, per pipeline slot (mvp/buffers.py)
        self._pos: Dict[Tuple[int, int], torch.Tensor] = {}
        self._rope: Dict[Tuple[int, int], Tuple[torch.Tensor, torch.Tensor]] = {}  # (gh, gw) -> cos / sin tables [max(gh, gw), 32] (rope_for)
        pipeline.publish()  # the split weights are read by forwards on any stream

    # ------------------------------------------------------------------ helpers
    def _dense_bias(self, table: torch.Tensor) -> torch.Tensor:
        """The dense logit bias of one block's table on the device; a table equal to one seen before shares its array."""
        if not self.has_cls:
            raise lib.MvpError("relative-position bias tables: the index rule has a class token (cls_token missing)")
        if table.dim() != 2 or table.shape[1] != self.heads:
            raise lib.MvpError(f"relative-position table of {tuple(table.shape)}: [rows, heads = {self.heads}] expected")
        t = table.detach().to("cpu", torch.float32)
        for seen, dense in self._bias_tables:
            if torch.equal(seen, t):
                return dense
        dense = dense_rel_pos_bias(t, *self.rel_pos_grid).to(self.device)
        self._bias_tables.append((t, dense))
        return dense

    def _workspace(self, B: int, gh: int, gw: int, headroom: int = 0) -> dict:
        def alloc():
            N = self.n_prefix + gh * gw
            M = B * N
            C, dev, pr = self.C, self.device, self.precision
            # When every GEMM of a block goes to the large-M kernel (M fills whole rounds of 256x256 tiles: grouped forwards), its A
            # operands — LayerNorm output, attention output, fc1 output — are kept as hi|lo-interleaved arrays (ops.IlvPair): a 32-deep
            # k-step of a row is then one whole 128-byte line for the LDS-DMA (2-3 % per GEMM on top of the interleaved weights).
            gp = lib.PREC_F16X2 if self.f16x2 else pr  # precision of the four block GEMMs
            # SAM: the qkv GEMM of a windowed block runs over the padded row count Mp of its windows, so that shape must go there as well
            Mp, nrel, windowed = M, 0, False
            if self.sam:  # the padded row count of the windowed blocks and the longest rel buffer of any block
                for w in {b["window"] for b in self.blocks}:
                    Bp, Np, K = (B * -(-gh // w) * -(-gw // w), w * w, 2 * w) if w else (B, N, gh + gw)
                    Mp, nrel, windowed = max(Mp, Bp * Np), max(nrel, Bp * self.heads * Np * (-(-K // 4) * 4)), windowed or w > 0
            shapes = [(M, 3 * C, C), (M, C, C), (M, self.fc1_out, C), (M, C, self.hidden)] + ([(Mp, 3 * C, C)] if windowed else [])
            ilv = (pr == PREC_BF16X3 and os.environ.get("MVP_ILV", "1") != "0" and C % 32 == 0 and self.hidden % 32 == 0 and
                   all(ops.gemm_tile(m, n, k, gp, 1, pipeline.tile_policy()).startswith("pp ") for m, n, k in shapes))
            a_pair = lambda rows, cols: ops.IlvPair(rows, cols, dev) if ilv else ops.empty_pair((rows, cols), pr, dev)
            xfull = torch.empty(M + headroom * N, C, dtype=torch.float32, device=dev)
            # RoPE engines only: the fp32 projection that mvp_rope2d_qkv reads, and the grid its positions come from
            rope = dict(qkv_f32=torch.empty(M, 3 * C, dtype=torch.float32, device=dev), grid=(gh, gw)) if self.rope_freq is not None else {}
            sam = {}
            if self.sam:
                sam = dict(grid=(gh, gw), qkv_f32=torch.empty(Mp, 3 * C, dtype=torch.float32, device=dev), rel=torch.empty(nrel, dtype=torch.float32, device=dev),
                           qkv=ops.empty_pair((Mp, 3 * C), pr, dev))
                if windowed:  # LayerNorm 1's output and the attention output in window order (A operands like xn and ao)
                    sam.update(xw=a_pair(Mp, C), aow=a_pair(Mp, C))
            # SwiGLU engines only: the fp32 w12 projection (gate | value) that mvp_swiglu_fwd reads
            glu = dict(h12=torch.empty(M, self.fc1_out, dtype=torch.float32, device=dev)) if self.swiglu else {}
            return dict(
                **rope,
                **glu,
                xfull=xfull, headroom=headroom, x=xfull[headroom * N:],
                xn=a_pair(M, C),
                qkv=sam["qkv"] if self.sam else ops.empty_pair((M, 3 * C), pr, dev),
                ao=a_pair(M, C),
                hmid=a_pair(M, self.hidden),
                patches=ops.empty_pair((B * gh * gw, self.k_patch), pr, dev),
                **{k: v for k, v in sam.items() if k != "qkv"},
            )

        return self._buffers.workspace((B, gh, gw), headroom, alloc)

    def slot_state(self, slot) -> list:
        """Every buffer set this engine currently keeps for pipeline slot ``slot`` (activation workspaces, feature packings, output
        maps), the carry stores and the position tables.  A captured hipGraph of that slot's forward holds their raw addresses: the
        pipeline keeps this list alive with the graph, because the engine itself drops the buffers of other resolutions when a new one
        arrives."""
        return (self._buffers.snapshot(slot) + list(self._pos.values()) + [t for cs in self._rope.values() for t in cs] +
                [dense for _, dense in self._bias_tables] + [t for rs in self._sam_rel.values() for t in rs] +
                [t for pu in self._sam_win.values() for t in pu[:2]])

    def sam_rel_tables(self, i: int, kh: int, kw: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(Rh [kh, kh, 64], Rw [kw, kw, 64]) of block i for a kh x kw query = key grid, on the device (``sam_rel_pos`` of the block's
        tables); cached per grid and per distinct table pair beside the position tables."""
        key = (self.blocks[i]["sam_tid"], kh, kw)
        rs = self._sam_rel.get(key)
        if rs is None:
            th, tw = self._sam_tables[key[0]]
            rs = self._sam_rel[key] = (sam_rel_pos(kh, kh, th).to(self.device), sam_rel_pos(kw, kw, tw).to(self.device))
            pipeline.publish()
        return rs

    def sam_windows(self, B: int, gh: int, gw: int, w: int) -> Tuple[torch.Tensor, torch.Tensor, int]:
        """(partition table, un-partition table, number of windows) of B images at gh x gw with w x w windows, on the device
        (``sam_window_index``); built once per (B, gh, gw, w)."""
        key = (B, gh, gw, w)
        pu = self._sam_win.get(key)
        if pu is None:
            part, unpart = sam_window_index(B, gh, gw, w)
            pu = self._sam_win[key] = (part.to(self.device), unpart.to(self.device), B * -(-gh // w) * -(-gw // w))
            pipeline.publish()
        return pu

    def rope_for(self, gh: int, gw: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The cos / sin tables of RoPE<rope_freq> for a gh x gw grid, fp32 [max(gh, gw), 32], row = grid coordinate: the reference's
        RoPE2D.get_cos_sin (croco_models/pos_embed.py:119-129) with D = 32 (half a head) and seq_len = the largest coordinate + 1,
        evaluated in fp32 ON THE CPU with the same torch expressions and then copied — bit-equal to the reference's CPU tables.  Cached
        per grid beside the position tables."""
        key = (gh, gw)
        cs = self._rope.get(key)
        if cs is None:
            D = 32
            inv_freq = 1.0 / (self.rope_freq ** (torch.arange(0, D, 2).float() / D))
            t = torch.arange(max(gh, gw), dtype=inv_freq.dtype)
            freqs = torch.einsum("i,j->ij", t, inv_freq)
            freqs = torch.cat((freqs, freqs), dim=-1)
            cs = self._rope[key] = (freqs.cos().contiguous().to(self.device), freqs.sin().contiguous().to(self.device))
            pipeline.publish()
        return cs

    def pos_for(self, gh: int, gw: int, dim2: int, dim3: int) -> torch.Tensor:
        """Pos-embed for a gh x gw grid.  'dino': bicubic resize with the +0.1 scale nudge of
        ibot_transformers.py:311-336 (done once per resolution, cached; torch's bicubic on the
        device is used for this one-time [1,C,14,14] resample)."""
        key = (gh, gw)
        pe = self._pos.get(key)
        if pe is not None:
            return pe
        if self.pos_embed_mode == "sam":  # plain bicubic resample of the CHECKPOINT's [1, S, S, C] table (sam.py:70-83), on the CPU in fp32
            t = self._pos_cpu
            if (gh, gw) != tuple(t.shape[1:3]):
                t = F.interpolate(t.permute(0, 3, 1, 2), size=(gh, gw), mode="bicubic").permute(0, 2, 3, 1)
            pe = self._pos[key] = t.reshape(gh * gw, self.C).contiguous().to(self.device)
            pipeline.publish()
            return pe
        c0 = 1 if self.has_cls else 0  # the table's CLS entry
        n = self.pos_embed.shape[1] - c0

        def resampled(expect=None, **how):
            """The table with its grid entries resampled and the CLS entry re-attached.  ``how`` goes to F.interpolate untouched: torch's
            bicubic is not bit-stable across ``size`` / ``scale_factor`` (nor antialias / align_corners), so each rule names its own."""
            side = int(math.sqrt(n))
            grid = self.pos_embed[:, c0:].reshape(1, side, side, self.C).permute(0, 3, 1, 2)
            grid = F.interpolate(grid, mode="bicubic", **how)
            assert expect is None or expect == tuple(grid.shape[-2:])
            return torch.cat((self.pos_embed[0, :c0], grid.permute(0, 2, 3, 1).reshape(-1, self.C)), dim=0).contiguous()

        if self.pos_embed_mode == "resize_aa":  # the count test, not the shape test
            pe = self.pos_embed[0].contiguous() if gh * gw == n else resampled(size=(gh, gw), antialias=True, align_corners=False)
        elif not self.has_cls and self.pos_embed_mode != "fixed":
            raise lib.MvpError(f"pos_embed_mode {self.pos_embed_mode!r} needs a CLS entry in the table: use 'resize_aa' or 'fixed'")
        elif self.pos_embed_mode == "fixed" or (gh * gw == n and dim2 == dim3):
            pe = self.pos_embed[0].contiguous()
        elif self.pos_embed_mode == "dinov2_reg":  # DINOv2 register models: interpolate_offset 0, antialias (size = the grid)
            pe = resampled(size=(dim2 // self.patch, dim3 // self.patch), antialias=True)
        else:
            w0, h0 = dim2 // self.patch + 0.1, dim3 // self.patch + 0.1
            pe = resampled(scale_factor=(w0 / math.sqrt(n), h0 / math.sqrt(n)), expect=(int(w0), int(h0)))
        self._pos[key] = pe
        pipeline.publish()
        return pe

    def set_pos_embed(self, pos_embed: torch.Tensor) -> None:
        self.pos_embed = pos_embed.detach().to(self.device, torch.float32).contiguous()
        self._pos.clear()

    # ------------------------------------------------------------------ forward
    def tokens(self, images: torch.Tensor, headroom: int = 0) -> Tuple[dict, int, int, int]:
        """Patch-embed + CLS + pos-embed into ws['x'] (K1); returns (ws, B, gh, gw).  ``headroom``: images' worth of rows kept free in
        front of ws['x'] (ws['xfull'] = head-room + x; span forwards, see forward_taps)."""
        images = images.to(self.device, torch.float32).contiguous()
        B, Cin, H, W = images.shape
        P = self.patch
        rh, rw = H % P, W % P
        if rh == 0 and rw == 0:
            ph = pw = 0
        else:  # center_padding quirk: a non-ragged dim still gets a full patch (utils.py:55-72)
            ph, pw = P - rh, P - rw
        gh, gw = (H + ph) // P, (W + pw) // P
        if self.rel_pos_grid is not None and (gh, gw) != self.rel_pos_grid:
            raise lib.MvpError(f"images of {H} x {W} make a {gh} x {gw} token grid; this model's relative-position bias was built for "
                               f"{self.rel_pos_grid[0]} x {self.rel_pos_grid[1]} (rel_pos_grid)")
        ws = self._workspace(B, gh, gw, headroom)
        npre, C = self.n_prefix, self.C
        N = npre + gh * gw
        Kp = self.k_patch
        if Kp == Cin * P * P:
            ops.patch_gather(images, ws["patches"], P, gh, gw, ph // 2, pw // 2)
        else:
            ops.patch_gather_ld(images, ws["patches"], P, gh, gw, ph // 2, pw // 2, Kp)
        pos = self.pos_for(gh, gw, H + ph, W + pw) if self.pos_embed is not None else None  # (None: RoPE / relative-position bias, nothing to add here)
        # x[b, npre+p, :] = patches · Wᵀ + bias + pos[1+p]   (row remap skips the CLS / register slots)
        ops.gemm(ws["patches"], self.w_patch, B * gh * gw, C, Kp, bias=self.b_patch, residual=pos[1:] if (self.has_cls and pos is not None) else pos, out_f32=ws["x"],
                 precision=self.precision, row_group=gh * gw, row_group_stride=N, row_group_off=npre, res_row_mod=gh * gw if pos is not None else 0)
        if self.rope_freq is not None:
            self.rope_for(gh, gw)  # (built and published here, before any block runs)
        if self.sam:  # index tables and relative-position tables of every block, likewise
            for i, blk in enumerate(self.blocks):
                w = blk["window"]
                if w:
                    self.sam_windows(B, gh, gw, w)
                self.sam_rel_tables(i, w or gh, w or gw)
        if not self.has_cls:
            pass  # no prefix rows at all (SigLIP)
        elif self.reg is None:
            ops.cls_rows(self.cls, pos if pos is not None else self._zero_c, ws["x"], B, N, C)  # (no table: the class row is cls alone)
        else:
            ops.prefix_rows(self.cls, pos, self.reg, ws["x"], B, N, C)
        if self.pre_norm is not None:  # CLIP's ln_pre: every row of the residual stream, in place
            ops.layernorm(ws["x"], self.pre_norm[0], self.pre_norm[1], None, B * N, C, self.ln_eps, out_f32=ws["x"])
        return ws, B, gh, gw

    def _check_f16_range(self, what: str, pair, rows: int) -> None:
        """MVP_CHECK_F16_RANGE=1 (diagnostic, synchronises): an fp16 half at +-65504 means an activation left the range of the two-product
        mode (its pairs saturate instead of overflowing, so the result would be wrong without a NaN to show for it)."""
        for t in ([pair.t[:rows]] if isinstance(pair, ops.IlvPair) else [pair[0][:rows], pair[1][:rows]]):
            if not bool((t.view(torch.float16).abs() < 65504.0).all()):  # (NaN fails the comparison too)
                raise lib.MvpError(f"f16x2: {what} holds values beyond fp16's range (|v| >= 65504): run this model with precision='bf16x3' (MVP_PRECISION=bf16x3)")

    def _act_site(self) -> str:
        return {"gelu": "GELU(fc1) output", "swiglu": "SwiGLU gate output silu(x1) * x2"}.get(self.act_name, f"{self.act_name}(fc1) output")

    def audit_sites(self) -> List[str]:
        """The names of the fp16-form operands a forward of this engine reads, in forward order (``RangeAudit``): per block the four
        activation operands of an f16x2 engine's GEMMs and, with ``att_qk_f16``, the Q / K the attention kernel reads."""
        out = []
        for i in range(self.depth):
            kinds = (["LayerNorm 1 output"] if self.f16x2 else []) + (["Q / K"] if self.att_qk_f16 else [])
            kinds += ["attention output", "LayerNorm 2 output", self._act_site()] if self.f16x2 else []
            out += [f"block {i}: {k}" for k in kinds]
        return out

    def _ln1_qkv(self, i: int, ws: dict, M: int, out_f32: Optional[torch.Tensor] = None, audit: Optional[RangeAudit] = None) -> None:
        """LayerNorm 1 and the fused qkv projection of block i, into ws['qkv'] in the forms the attention kernel reads — or, with
        ``out_f32`` (last_block_qkv: no attention follows), as plain fp32 [M, 3C] without any f16 output form."""
        blk, C, f2 = self.blocks[i], self.C, self.f16x2
        ops.layernorm(ws["x"], blk["n1w"], blk["n1b"], ws["xn"], M, C, self.ln_eps, out_f16=f2)
        if audit is not None and f2:
            audit.scan(f"block {i}: LayerNorm 1 output", ws["xn"], M, C)
        # bf16x3: the V third of qkv leaves the GEMM as hi = fp16, lo = bf16, and the attention kernel holds its probabilities as one
        # fp16 value (csrc/attention.hip, VF16; MVP_ATT_V=pair brings back the bf16-pair probabilities of rounds 1-3)
        # (f16x2: Q and K leave as compensated fp16 pairs too — activation / weight-side form, Q.K^T in two f16 products — unless MVP_ATT_QK=pair;
        #  the attention output, LayerNorm's and fc1's output leave as compensated fp16 activation pairs)
        pairs = out_f32 is None
        ops.gemm(ws["xn"], blk["qkv_w"], M, 3 * C, C, bias=blk["qkv_b"], out=ws["qkv"] if pairs else None, out_f32=out_f32,
                 precision=lib.PREC_F16X2 if f2 else self.precision, w_ilv=blk.get("qkv_w_ilv"),
                 f16_col0=(-2 * C if self.att_qk_f16 else 2 * C) if (pairs and self.att_v_f16) else 0)

    def _sam_attention(self, i: int, ws: dict, B: int, N: int, audit: Optional[RangeAudit] = None) -> None:
        """LayerNorm 1 up to the attention output ws['ao'] of a SAM block.  Windowed block: LN1, gather into windows (pad rows zero AFTER the
        norm, so they pass the qkv GEMM and are real keys with k = b_k, v = b_v, as in segment_anything), qkv GEMM over the B * nW * w^2
        padded rows as fp32, relative-position terms + conversion (mvp_relpos_terms), attention per window with the decomposed bias, gather
        back (pad rows dropped).  Global block: no gathers, one "window" per image of the whole gh x gw grid."""
        blk, C, M, pr, f2 = self.blocks[i], self.C, B * N, self.precision, self.f16x2
        gh, gw = ws["grid"]
        w = blk["window"]
        ops.layernorm(ws["x"], blk["n1w"], blk["n1b"], ws["xn"], M, C, self.ln_eps, out_f16=f2)
        if w:
            part, unpart, Bp = self.sam_windows(B, gh, gw, w)
            Np, kh, kw = w * w, w, w
            ops.gather_rows(ws["xn"], ws["xw"], part, M, C)
            a_in, ao = ws["xw"], ws["aow"]
        else:
            Bp, Np, kh, kw, a_in, ao = B, N, gh, gw, ws["xn"], ws["ao"]
        Mp = Bp * Np
        if audit is not None and f2:  # (a windowed block: the gathered rows the GEMM reads, zero pad rows included)
            audit.scan(f"block {i}: LayerNorm 1 output", a_in, Mp, C)
        ops.gemm(a_in, blk["qkv_w"], Mp, 3 * C, C, bias=blk["qkv_b"], out_f32=ws["qkv_f32"], precision=lib.PREC_F16X2 if f2 else pr, w_ilv=blk.get("qkv_w_ilv"))
        rh, rw = self.sam_rel_tables(i, kh, kw)
        ld = -(-(kh + kw) // 4) * 4
        rel = ws["rel"][:Bp * self.heads * Np * ld].view(Bp * self.heads, Np, ld)
        ops.relpos_terms(ws["qkv_f32"], ws["qkv"], rel, rh, rw, Mp, Np, self.heads, pr, v_f16=self.att_v_f16, qk_f16=self.att_qk_f16)
        if audit is not None and self.att_qk_f16:
            audit.scan(f"block {i}: Q / K", ws["qkv"], Mp, 2 * C)
        ops.attention(ws["qkv"], ao, Bp, Np, self.heads, 64 ** -0.5, pr, v_f16=self.att_v_f16, qk_f16=self.att_qk_f16, out_f16=f2, rel=rel, rel_grid=(kh, kw))
        if w:
            ops.gather_rows(ws["aow"], ws["ao"], unpart, Mp, C)

    def run_block(self, i: int, ws: dict, B: int, N: int, audit: Optional[RangeAudit] = None) -> None:
        """Block i over the M = B * N rows of ws['x'].  ``audit``: scan every fp16-form operand in the buffer its consumer reads, right
        before that consumer (one extra read-only launch per site on this stream; nothing the block computes changes)."""
        blk, C, M, pr = self.blocks[i], self.C, B * N, self.precision
        f2 = self.f16x2
        chk = f2 and self.check_f16_range
        aud = audit if f2 else None  # the four activation operands exist in fp16 form only in an f16x2 engine
        gp = lib.PREC_F16X2 if f2 else pr  # precision of the four block GEMMs
        x = ws["x"]
        vf16, qk16 = self.att_v_f16, self.att_qk_f16
        if self.sam:
            self._sam_attention(i, ws, B, N, audit)
        elif self.rope_freq is None:
            self._ln1_qkv(i, ws, M, audit=audit)
        else:  # the projection as fp32, then rotation + conversion into the forms the attention kernel reads (mvp_rope2d_qkv)
            gh, gw = ws["grid"]
            cos, sin = self.rope_for(gh, gw)
            self._ln1_qkv(i, ws, M, out_f32=ws["qkv_f32"], audit=audit)
            ops.rope2d_qkv(ws["qkv_f32"], ws["qkv"], cos, sin, M, N, self.heads, self.n_prefix, gh, gw, pr, v_f16=vf16, qk_f16=qk16)
        if chk:  # (after the projection: ws["xn"] still holds LayerNorm 1's output)
            self._check_f16_range(f"block {i}: LayerNorm 1 output", ws["xn"], M)
        if chk and qk16:
            self._check_f16_range(f"block {i}: Q / K", (ws["qkv"][0][:, :2 * C], ws["qkv"][1][:, :2 * C]), M)
        if not self.sam:
            if audit is not None and qk16:
                audit.scan(f"block {i}: Q / K", ws["qkv"], M, 2 * C)
            ops.attention(ws["qkv"], ws["ao"], B, N, self.heads, 64 ** -0.5, pr, v_f16=vf16, qk_f16=qk16, out_f16=f2, bias=blk.get("att_bias"))
        if chk:
            self._check_f16_range(f"block {i}: attention output", ws["ao"], M)
        if aud is not None:
            aud.scan(f"block {i}: attention output", ws["ao"], M, C)
        ops.gemm(ws["ao"], blk["proj_w"], M, C, C, bias=blk["proj_b"], residual=x, out_f32=x, precision=gp, w_ilv=blk.get("proj_w_ilv"),
                 col_scale=blk["ls1"])
        ops.layernorm(x, blk["n2w"], blk["n2b"], ws["xn"], M, C, self.ln_eps, out_f16=f2)
        if chk:
            self._check_f16_range(f"block {i}: LayerNorm 2 output", ws["xn"], M)
        if aud is not None:
            aud.scan(f"block {i}: LayerNorm 2 output", ws["xn"], M, C)
        if self.swiglu:  # w12 as fp32 [M, 2H], then silu(gate) * value into the A operand of w3 (columns H .. hidden-1 zero)
            ops.gemm(ws["xn"], blk["fc1_w"], M, self.fc1_out, C, bias=blk["fc1_b"], out_f32=ws["h12"], precision=gp, w_ilv=blk.get("fc1_w_ilv"))
            ops.swiglu(ws["h12"], ws["hmid"], M, self.swiglu_h, ld_out=self.hidden, precision=gp)
        else:
            ops.gemm(ws["xn"], blk["fc1_w"], M, self.hidden, C, bias=blk["fc1_b"], out=ws["hmid"], act=self.act, precision=gp, w_ilv=blk.get("fc1_w_ilv"),
                     f16_col0=-1 if f2 else 0)
        if chk:
            what = {"gelu": "GELU(fc1) output", "swiglu": "SwiGLU gate output silu(x1) * x2"}.get(self.act_name, f"{self.act_name}(fc1) output")
            self._check_f16_range(f"block {i}: {what}", ws["hmid"], M)
        if aud is not None:
            aud.scan(f"block {i}: {self._act_site()}", ws["hmid"], M, self.hidden)
        ops.gemm(ws["hmid"], blk["fc2_w"], M, C, self.hidden, bias=blk["fc2_b"], residual=x, out_f32=x, precision=gp, w_ilv=blk.get("fc2_w_ilv"),
                 col_scale=blk["ls2"])

    def forward_taps(self, images: torch.Tensor, layers: Sequence[int], *, bn: Optional[Sequence[dict]] = None,
                     bn_mode: int = 0, pack: bool = True, tap_input_of_block: bool = False, want_cls: bool = False, groups: int = 1,
                     replay_after_norm: bool = False, audit: Optional[RangeAudit] = None):
        """Run blocks up to the last tapped one; at each tap apply the (train-mode) tap BN and
        emit the NCHW map (+ token-major packing).  ``bn[j]`` = dict(weight,bias,running_mean,
        running_var) tensors or None; bn_mode: 0 train stats, 1 eval, 2 no norm.
        ``tap_input_of_block``: tap the INPUT of block i instead of its output (HF
        hidden_states indexing used by the MAE wrapper, quirk Q4).
        ``groups`` = G > 1: ``images`` holds G batches of equal size stacked along dim 0 (mvp/pipeline.py).  Patch embedding,
        LayerNorm, the GEMMs and attention are per-row / per-image, so the G batches simply share their launches (M = G * B * N
        rows: the large-M GEMM kernel); the tap BN — train-mode statistics over ONE batch (dino.py:185-191) — runs per batch on that
        batch's rows.  Every batch gets exactly the bits it would get alone; returns ``TapGroups`` (one ``TapOutputs`` per batch).
        ``groups`` = ``pipeline.Span(batch, carry)``: the forward's images are a SPAN of the image stream that need not start or end on
        a batch boundary (batches of ``batch`` images; the first ``batch - carry`` images complete the batch whose first ``carry``
        images ended the previous span, when carry > 0).  The blocks do not care; per tap, the carried images' rows (kept in
        the stream's carry store, written by the previous span's forward on the same stream) are copied in FRONT of this span's rows — the
        ``x`` workspace has that head-room — so that all complete batches are contiguous and one grouped tap-BN launch serves them, and
        the rows of a trailing incomplete batch are copied to the carry store for the next span.  Returns ``TapGroups`` of the
        (carry + images) // batch batches this forward completes.
        ``replay_after_norm`` (BEiT v2's wrapper, beit_v2.py:261-265): before the tapped loop, run ALL ``depth`` blocks over the token
        stream and apply ``fc_norm`` to every row of it in place; the tapped loop then runs the blocks AGAIN on that result.  Blocks and
        LayerNorm are per row, so grouped and span forwards and graph capture need nothing new.
        ``audit`` (a ``RangeAudit`` of this engine): every block run by this forward — the replay pass included, into the same sites —
        also scans its fp16-form operands into the audit's record, on this stream and without a sync; the taps are bit for bit those of
        an unaudited forward.  ``audit.read()`` afterwards."""
        if want_cls and not self.has_cls:
            raise lib.MvpError("want_cls: this model has no CLS token (n_prefix = 0); use output 'dense' or 'gap'")
        span = groups if isinstance(groups, pipeline.Span) else None
        layers = list(layers)
        G, B, carry, tail = plan_taps(images.shape[0], groups)
        # Train-mode tap BN updates its running statistics in place: the only state a frozen forward mutates.  Forwards in flight on
        # different streams finish in any order, so a pipelined forward leaves that update to the consumer (pipeline.defer), which
        # applies it on the trainer's stream in batch order — same arithmetic, same bits (mvp_bn_running_update).
        defer = bn is not None and bn_mode == 0 and pipeline.pipelined()
        if (G > 1 or span is not None) and bn is not None and bn_mode == 0 and not defer:
            raise lib.MvpError("a grouped forward with train-mode tap BN must run under the pipeline (its running-statistics updates are per batch)")
        ws, Bt, gh, gw = self.tokens(images, headroom=span.batch if span else 0)
        N = self.n_prefix + gh * gw
        if replay_after_norm:
            if self.fc_norm is None:
                raise lib.MvpError("replay_after_norm: the state dict has no fc_norm.weight / fc_norm.bias")
            for i in range(self.depth):
                self.run_block(i, ws, Bt, N, audit)
            ops.layernorm(ws["x"], self.fc_norm[0], self.fc_norm[1], None, Bt * N, self.C, self.ln_eps, out_f32=ws["x"])
        x_bn, store, bn_ws, packs, out = self._tap_buffers(ws, span, G, B, carry, gh, gw, layers, pack, want_cls)
        t = SimpleNamespace(ws=ws, x_bn=x_bn, store=store, bn_ws=bn_ws, packs=packs, out=out, Bt=Bt, N=N, hw=gh * gw, G=G, B=B, carry=carry, tail=tail,
                            bn=bn, bn_mode=bn_mode, want_cls=want_cls, defer=defer, outs=[TapOutputs() for _ in range(G)],
                            running=[[] for _ in range(G)])  # per batch of the group: its taps' deferred running-statistics updates
        for o in t.outs:
            o.cls = []
        for i in range(self.depth):
            if tap_input_of_block and i in layers:
                self._tap(t, layers.index(i))
                if len(t.outs[0]) == len(layers):
                    break
            self.run_block(i, ws, Bt, N, audit)
            if (not tap_input_of_block) and i in layers:
                self._tap(t, layers.index(i))
                if len(t.outs[0]) == len(layers):
                    break
        for g, o in enumerate(t.outs):
            if t.running[g]:  # all taps of a batch in ONE launch on the consumer's stream (mvp_bn_running_update_n; the modules are distinct)
                pipeline.defer(lambda items=t.running[g]: ops.bn_running_update_many(items), group=g)
            o.stats = t.out["stats"][g]
            if t.packs is not None:
                o.packed = t.packs[g]
                t.packs[g].rewritten(o)
        return t.outs[0] if (G == 1 and span is None) else TapGroups(t.outs)

    def _tap_buffers(self, ws: dict, span, G: int, B: int, carry: int, gh: int, gw: int, layers: List[int], pack: bool, want_cls: bool):
        """What the taps of a forward over G batches of B images read and write, from the engine's store (the steady state allocates
        nothing): ``x_bn`` the rows of the complete batches, ``store`` the span's carry store, ``bn_ws`` the tap-BN scratch, ``packs``
        the G packings (None without ``pack``), ``out`` the output maps."""
        N, C, dev, taps = self.n_prefix + gh * gw, self.C, self.device, len(layers)
        x_bn, store = ws["x"], None
        if span is not None:
            x_bn = ws["xfull"][(ws["headroom"] - carry) * N:]  # the complete batches: carried rows (copied per tap) + this span's rows
            # [taps, B * N, C] tap-level rows of a batch cut by a span's end; one store per image stream (pipeline): see pipeline.Span
            store = self._buffers.carry(span.stream, (B, gh, gw, taps), lambda: torch.empty(taps, B * N, C, dtype=torch.float32, device=dev))
        bn_ws = ws.get(("bn_ws", G))  # tap-BN partials + scale / shift of G batches of B * N rows
        if bn_ws is None:
            bn_ws = ws[("bn_ws", G)] = torch.empty(G * ops.bn_tokens_workspace_bytes(B * N, C) // 4 + 16, dtype=torch.float32, device=dev)

        def new_packs():
            Mpad, Cpad = PackedFeatures.padded(B, gh, gw, C * taps)
            big = ops.zeros_pair((G, Mpad, Cpad), self.precision, dev)  # one allocation: the tap kernel writes all batches in one launch
            return [PackedFeatures(B, gh, gw, C * taps, self.precision, dev, tok=(big[0][g], big[1][g] if big[1] is not None else None))
                    for g in range(G)]

        def new_out():
            return dict(stats=torch.empty(G, taps, 3 * C, dtype=torch.float32, device=dev),
                        nchw=[torch.empty(G, B, C, gh, gw, dtype=torch.float32, device=dev) for _ in layers],
                        cls=[torch.empty(G, B, C, dtype=torch.float32, device=dev) if want_cls else None for _ in layers])

        # reuse the (zero padded) packing buffers across steps: only the valid region is rewritten
        packs = self._buffers.packings((B, gh, gw, taps), G, new_packs) if pack else None
        # Plain calls return freshly allocated maps (the caller may keep them).  A pipelined forward (mvp/pipeline.py) writes into
        # buffers owned by its slot instead — valid until the slot's next forward, which is the pipeline's contract — so the
        # steady state allocates nothing and no block ever changes hands between the side stream's and the trainer's allocator pools.
        out = self._buffers.outputs((B, gh, gw, tuple(layers), bool(want_cls)), G, new_out) if pipeline.pipelined() else new_out()
        return x_bn, store, bn_ws, packs, out

    def _tap(self, t, j: int) -> None:
        """Tap j of the forward ``t`` (forward_taps), on the residual stream as it stands: complete the cut batches through the carry
        store, then ONE tap-BN launch for all batches; collects every batch's outputs and deferred running-statistics updates."""
        N, C, G, want_cls, pk = t.N, self.C, t.G, t.want_cls, t.packs[0] if t.packs is not None else None
        b = t.bn[j] if t.bn is not None else None
        nchw, cls, stats = t.out["nchw"][j], t.out["cls"][j], t.out["stats"]
        if t.carry:
            t.x_bn[:t.carry * N].copy_(t.store[j, :t.carry * N])
        if t.tail:
            t.store[j, :t.tail * N].copy_(t.ws["x"][(t.Bt - t.tail) * N:t.Bt * N])
        # ONE call for all batches of the group: statistics, normalisation and outputs per batch (mvp_bn_tokens_args.groups)
        ops.bn_tokens_to_nchw(
            t.x_bn, t.B, N, C, t.hw, workspace=t.bn_ws, stats=stats[0, j],
            gamma=b["weight"] if b else None, beta=b["bias"] if b else None,
            running_mean=b["running_mean"] if b else None, running_var=b["running_var"] if b else None,
            nchw=nchw[0], tok=pk.tok if pk else None, ld_tok=pk.Cpad if pk else 0, col_off=j * C,
            mode=t.bn_mode, cls_out=cls[0] if want_cls else None, num_batches_tracked=b.get("num_batches_tracked") if b else None, defer_running=t.defer,
            groups=G, stats_gstride=stats.stride(0), nchw_gstride=nchw.stride(0),
            tok_gstride=(pk.Mpad * pk.Cpad) if pk else 0, cls_gstride=cls.stride(0) if want_cls else 0)
        for g in range(G):
            if want_cls:
                t.outs[g].cls.append(cls[g])
            if t.defer and b is not None and b.get("running_mean") is not None:
                t.running[g].append((stats[g, j], b["running_mean"], b["running_var"], b.get("num_batches_tracked"), C))
            t.outs[g].append(nchw[g])

    def last_block_qkv(self, images: torch.Tensor, audit: Optional[RangeAudit] = None) -> torch.Tensor:
        """The fused qkv projection of the LAST block (fp32 [B, N, 3C]: q | k | v, heads side by side) — what the reference captures
        with a forward hook on ``blocks[-1].attn.qkv`` (dino.py:82-113).  Blocks 0 .. depth-2 run as usual; the last block stops after
        LayerNorm 1 and the projection (its attention output is never used on that path).  ``audit``: as in ``forward_taps``; of the
        last block only LayerNorm 1's output is an operand here."""
        ws, B, gh, gw = self.tokens(images)
        N = self.n_prefix + gh * gw
        for i in range(self.depth - 1):
            self.run_block(i, ws, B, N, audit)
        out = torch.empty(B * N, 3 * self.C, dtype=torch.float32, device=self.device)
        self._ln1_qkv(self.depth - 1, ws, B * N, out_f32=out, audit=audit)
        return out.view(B, N, 3 * self.C)

    def forward_tokens(self, images: torch.Tensor, n_blocks: Optional[int] = None) -> torch.Tensor:
        """Raw fp32 token stream after ``n_blocks`` blocks ([B, N, C]); for tests / CLS outputs."""
        ws, B, gh, gw = self.tokens(images)
        N = self.n_prefix + gh * gw
        for i in range(self.depth if n_blocks is None else n_blocks):
            self.run_block(i, ws, B, N)
        return ws["x"].view(B, N, self.C).clone()
