"""fp64 reference, rounding model and per-row error budget of the attention kernels (csrc/attention.hip).  Torch only, no HIP: runs in
fp64 on whatever device its inputs live on.

A test hands the kernel a qkv operand pair in one of four forms (FORMS).  ``halves`` reads the stored 16-bit halves back as fp64,
``decode`` / ``decode_halves`` give the Q, K, V those halves stand for — the reference ``exact`` is taken on them, so the packing error
of the operands is not charged to the kernel — and ``model`` repeats the computation with the roundings and dropped products that
include/mvp_hip.h and the header of attention.hip document.  ``row_err`` measures every query row on its own, and ``bound`` turns the
model's own error into the budget of a case:

    4 * max row_err(model, exact) + 2^-22 * max(1, max |score * scale * log2 e|)

4x: fp32 accumulation order and v_exp_f32's ulp, which the model does not emulate; the additive term: the fp32 rounding of the exponent
argument plus one ulp of exp2.  Test infrastructure only."""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, Optional, Tuple

import torch

FORMS = ("bf16x3", "bf16x3_vf16", "bf16x3_vf16_qk16", "bf16")
CAPS = {"bf16x3": 6e-5, "bf16x3_vf16": 3e-4, "bf16x3_vf16_qk16": 3e-4, "bf16": 4e-3}  # the whole-tensor rel-L2 bounds of test_attention
STAGE_BYTES = {"bf16x3": 32768, "bf16x3_vf16": 32768, "bf16x3_vf16_qk16": 32768, "bf16": 16384}  # one K + V tile slot of the LDS ring
LOG2E = 1.4426950408889634

Pair = Tuple[torch.Tensor, Optional[torch.Tensor]]


def _bf16(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _f16(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.float32).to(torch.float16).to(torch.float64)


def _bits_f16(t: torch.Tensor) -> torch.Tensor:
    """fp16 bits stored in a bf16-typed array -> fp64."""
    return t.contiguous().view(torch.float16).to(torch.float64)


def split_bf16(x: torch.Tensor) -> Pair:
    """Torch restatement of the bf16 pair (csrc/mvp_common.h, split2_bf16): hi = bf16(x), lo = bf16(x - hi)."""
    x = x.float()
    hi = x.bfloat16()
    return hi, (x - hi.float()).bfloat16()


def pack(qkv: torch.Tensor, C: int, form: str, split=split_bf16) -> Pair:
    """fp32 qkv [rows, 3C] -> the operand pair of ``form``, built as the GPU tests build it (``split`` = ops.split_bf16 there): the bf16
    pair, then the V third as fp16 + bf16 (vf16) and the Q / K thirds as compensated fp16 pairs (qk16); hi alone for bf16."""
    from test_gpu_kernels import _qk_thirds_as_f16_comp, _v_third_as_f16_bf16

    assert form in FORMS, form
    qp = split(qkv)
    if form == "bf16":
        return qp[0], None
    if "_vf16" in form:
        qp = _v_third_as_f16_bf16(qp, C)
    if form.endswith("_qk16"):
        qp = _qk_thirds_as_f16_comp(qp, C)
    return qp


def heads(x: torch.Tensor, B: int, N: int, H: int) -> torch.Tensor:
    """[B * N, H * 64] -> [B, H, N, 64]."""
    return x.reshape(B, N, H, 64).permute(0, 2, 1, 3)


def rows(x: torch.Tensor) -> torch.Tensor:
    """[B, H, N, 64] -> [B * N, H * 64]."""
    B, H, N, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * N, H * 64)


def halves(qp: Pair, C: int, form: str) -> Dict[str, torch.Tensor]:
    """The six stored halves of a qkv pair ([rows, >= 3C] each) as fp64 [rows, C]: fp16 bits are read as fp16, a missing lo is zero."""
    assert form in FORMS, form
    hi, lo = qp
    vf16, qk16 = "_vf16" in form, form.endswith("_qk16")
    out = {}
    for i, name in enumerate("qkv"):
        f16_hi = vf16 if name == "v" else qk16
        f16_lo = qk16 and name != "v"
        h = hi[:, i * C:(i + 1) * C]
        out[name + "_hi"] = _bits_f16(h) if f16_hi else h.to(torch.float64)
        if form == "bf16" or lo is None:
            out[name + "_lo"] = torch.zeros_like(out[name + "_hi"])
        else:
            l = lo[:, i * C:(i + 1) * C]
            out[name + "_lo"] = _bits_f16(l) if f16_lo else l.to(torch.float64)
    return out


def decode_halves(h: Dict[str, torch.Tensor], form: str):
    """Q, K, V that the halves stand for.  qk16: Q is the compensated activation pair (hi + (lo - hi / 8) / 8), K the compensated
    weight-side pair (hi + lo / 8); everything else is hi + lo (bf16: lo = 0)."""
    if form.endswith("_qk16"):
        q = h["q_hi"] + (h["q_lo"] - h["q_hi"] / 8.0) / 8.0
        k = h["k_hi"] + h["k_lo"] / 8.0
    else:
        q, k = h["q_hi"] + h["q_lo"], h["k_hi"] + h["k_lo"]
    return q, k, h["v_hi"] + h["v_lo"]


def decode(qp: Pair, C: int, form: str):
    """fp64 Q, K, V ([rows, C] each) that the kernel was actually handed."""
    return decode_halves(halves(qp, C, form), form)


def decode_out_f16(hi: torch.Tensor, lo: torch.Tensor) -> torch.Tensor:
    """The out_f16 = 1 output pair (compensated activation form, fp16 bits in bf16-typed arrays) -> fp64."""
    h, l = _bits_f16(hi), _bits_f16(lo)
    return h + (l - h / 8.0) / 8.0


def exact(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float) -> torch.Tensor:
    """softmax(q k^T * scale) v in fp64, over the last two dimensions."""
    return ((q @ k.transpose(-2, -1)) * scale).softmax(-1) @ v


def model(h: Dict[str, torch.Tensor], scale: float, form: str, ideal: bool = False) -> torch.Tensor:
    """The kernel's arithmetic in fp64 (halves as [..., N, 64]): the products it keeps and the roundings it performs, nothing else.
      Q.K^T   hi.hi + hi.lo + lo.hi (bf16 pairs);  q_lo.k_lo + q_hi.k_hi on the fp16 halves (qk16);  hi.hi (bf16)
      P       relative to the true row maximum;  bf16 pair (bf16x3) | fp16 for v_hi and bf16 for v_lo (vf16) | bf16 (bf16).  (The
              kernel rounds relative to its running maximum.  To a relative rounding that is an exponent offset, with one exception:
              here a row's largest probability is exactly 1 and rounds without error, while under the deferred maximum of the vf16
              forms it is 2^d, d < 6, whenever the best key lies behind tile 0 — measured, the kernel's worst vf16 row is up to 3.9 x
              this model's at N > 64 and equal to it at N <= 64: profiles/attention_row_error.txt.  The factor 4 of ``bound`` holds it.)
      P.V     p_hi.v_hi + p_hi.v_lo + p_lo.v_hi | p16.v_hi + bf16(p).v_lo | p.v_hi
      l       the sum of the UNROUNDED probabilities
      O / l   stored as a bf16 pair: hi = bf16(o), lo = bf16(o - hi)
    ``ideal``: no rounding, no dropped product — equals ``exact`` on the decoded operands."""
    assert form in FORMS, form
    T = lambda x: x.transpose(-2, -1)
    if ideal:
        q, k, v = decode_halves(h, form)
        s = q @ T(k)
    elif form == "bf16":
        s = h["q_hi"] @ T(h["k_hi"])
    elif form.endswith("_qk16"):
        s = h["q_lo"] @ T(h["k_lo"]) + h["q_hi"] @ T(h["k_hi"])
    else:
        s = h["q_hi"] @ T(h["k_hi"]) + h["q_hi"] @ T(h["k_lo"]) + h["q_lo"] @ T(h["k_hi"])
    x = s * scale
    p = torch.exp(x - x.max(-1, keepdim=True).values)
    l = p.sum(-1, keepdim=True)
    if ideal:
        return (p @ v) / l
    if form == "bf16x3":
        p_hi = _bf16(p)
        p_lo = _bf16(p - p_hi)
        o = p_hi @ h["v_hi"] + p_hi @ h["v_lo"] + p_lo @ h["v_hi"]
    elif "_vf16" in form:
        o = _f16(p) @ h["v_hi"] + _bf16(p) @ h["v_lo"]
    else:
        o = _bf16(p) @ h["v_hi"]
    o = o / l
    o_hi = _bf16(o)
    return o_hi + _bf16(o - o_hi)


def row_err(got: torch.Tensor, ref: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """Per (batch, head, query): ||got - ref||_2 / max_k ||v[b, h, k]||_2 -> [B, H, N].  The output is a convex combination of V rows,
    so this scale cannot vanish by cancellation."""
    vmax = v.norm(dim=-1).max(dim=-1, keepdim=True).values
    return (got - ref).norm(dim=-1) / vmax


def bound(model_err: torch.Tensor, smax_exp2: float) -> float:
    """The per-row budget of a case from the model's row errors and the largest |score * scale * log2 e|."""
    return 4.0 * float(model_err.max()) + 2.0 ** -22 * max(1.0, float(smax_exp2))


def worst(err: torch.Tensor):
    """(value, (b, h, q)) of the largest entry of a [B, H, N] error tensor (NaN counts as the largest)."""
    e = torch.nan_to_num(err, nan=float("inf"))
    i = int(e.reshape(-1).argmax())
    _, H, N = err.shape
    return float(e.reshape(-1)[i]), (i // (H * N), (i // N) % H, i % N)


def reference(qp: Pair, B: int, N: int, H: int, scale: float, form: str) -> SimpleNamespace:
    """Everything a test needs about one case, computed once: per-head halves, decoded q / k / v, ``ref`` = exact, ``mdl`` = model,
    ``model_err`` = row_err(mdl, ref), ``smax`` = max |score * scale * log2 e| per row [B, H, N], ``bound``."""
    C = H * 64
    h = {k: heads(t, B, N, H) for k, t in halves(qp, C, form).items()}
    q, k, v = decode_halves(h, form)
    ref = exact(q, k, v, scale)
    mdl = model(h, scale, form)
    smax = (q @ k.transpose(-2, -1)).abs().max(-1).values * (abs(scale) * LOG2E)
    merr = row_err(mdl, ref, v)
    return SimpleNamespace(h=h, q=q, k=k, v=v, ref=ref, mdl=mdl, model_err=merr, smax=smax, bound=bound(merr, float(smax.max())),
                           B=B, N=N, H=H, scale=scale, form=form)


def per_cu(nkt: int, form: str) -> int:
    """Workgroups of the resident kernel per CU: how many rings of nkt + 1 slots fit into 160 KiB of LDS (launch_attention)."""
    return max(1, (160 * 1024) // ((nkt + 1) * STAGE_BYTES[form]))


def ring_pairs(nkt: int, form: str, cu_count: int) -> int:
    """The (batch, head) count at which every workgroup of the persistent kernel walks its ring past every slot offset
    s0 = (nkt * i) % (nkt + 1) and wraps once (nkt + 2 pairs each), with 3 workgroups taking one pair more."""
    return (nkt + 2) * cu_count * per_cu(nkt, form) + 3


def nkt_of(N: int) -> int:
    return (N + 63) // 64


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a - b).norm() / b.norm().clamp_min(1e-300))
