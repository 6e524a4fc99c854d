"""fp64 reference, rounding model and per-row budget of attention with a logit bias (mvp_attention_bias_fwd): tests/attention_ref.py with
``x = s * scale + bias`` inserted.  The budget of a case is

    4 * max row_err(model, exact) + 2^-21 * max(1, max |logit * log2 e|),    logit = score * scale + bias

2^-21 instead of attention_ref's 2^-22: two more fp32 roundings of magnitude <= the argument (the biased logit s * scale + bias, and its
product with log2 e before the maximum is subtracted) on top of what 2^-22 holds there.  Test infrastructure only."""
from __future__ import annotations

from types import SimpleNamespace

import torch

import attention_ref as ar


def exact(q, k, v, scale, bias):
    """softmax(q k^T * scale + bias) v in fp64; ``bias`` [H, N, N] broadcasts over the batch."""
    return ((q @ k.transpose(-2, -1)) * scale + bias).softmax(-1) @ v


def model(h, scale, form, bias):
    """attention_ref.model (the products the kernel keeps, the roundings it performs) with the bias added to the scaled score."""
    assert form in ar.FORMS, form
    T = lambda x: x.transpose(-2, -1)
    if form == "bf16":
        s = h["q_hi"] @ T(h["k_hi"])
    elif form.endswith("_qk16"):
        s = h["q_lo"] @ T(h["k_lo"]) + h["q_hi"] @ T(h["k_hi"])
    else:
        s = h["q_hi"] @ T(h["k_hi"]) + h["q_hi"] @ T(h["k_lo"]) + h["q_lo"] @ T(h["k_hi"])
    x = s * scale + bias
    p = torch.exp(x - x.max(-1, keepdim=True).values)
    l = p.sum(-1, keepdim=True)
    if form == "bf16x3":
        p_hi = ar._bf16(p)
        p_lo = ar._bf16(p - p_hi)
        o = p_hi @ h["v_hi"] + p_hi @ h["v_lo"] + p_lo @ h["v_hi"]
    elif "_vf16" in form:
        o = ar._f16(p) @ h["v_hi"] + ar._bf16(p) @ h["v_lo"]
    else:
        o = ar._bf16(p) @ h["v_hi"]
    o = o / l
    o_hi = ar._bf16(o)
    return o_hi + ar._bf16(o - o_hi)


def bound(model_err, lmax_exp2: float) -> float:
    return 4.0 * float(model_err.max()) + 2.0 ** -21 * max(1.0, float(lmax_exp2))


def reference(qp, B, N, H, scale, form, bias) -> SimpleNamespace:
    """attention_ref.reference for a biased case (``bias`` fp64 [H, N, N]): ``smax`` is max |logit * log2 e| per row, bias included."""
    C = H * 64
    h = {k: ar.heads(t, B, N, H) for k, t in ar.halves(qp, C, form).items()}
    q, k, v = ar.decode_halves(h, form)
    bias = bias.to(torch.float64)
    ref = exact(q, k, v, scale, bias)
    mdl = model(h, scale, form, bias)
    smax = ((q @ k.transpose(-2, -1)) * scale + bias).abs().max(-1).values * ar.LOG2E
    merr = ar.row_err(mdl, ref, v)
    return SimpleNamespace(h=h, q=q, k=k, v=v, ref=ref, mdl=mdl, model_err=merr, smax=smax, bound=bound(merr, float(smax.max())),
                           B=B, N=N, H=H, scale=scale, form=form, bias=bias)


def padded(N: int) -> int:
    """The smallest ld_bias: 64 * ceil(N / 64)."""
    return 64 * ((N + 63) // 64)


def bias_buffer(dense: torch.Tensor, ld: int = 0, head_stride: int = 0, lead: int = 0):
    """fp32 [H, N, N] -> (the [H, N, ld] strided view the kernel is handed, its backing buffer): everything outside [h, q < N, k < N] — padding
    columns, the gap between heads, ``lead`` elements in front and 64 behind — holds NaN."""
    H, N, _ = dense.shape
    ld = ld or padded(N)
    head_stride = head_stride or N * ld
    buf = torch.full((lead + H * head_stride + 64,), float("nan"), dtype=torch.float32, device=dense.device)
    view = buf[lead:].as_strided((H, N, ld), (head_stride, ld, 1))
    view[:, :, :N] = dense.to(torch.float32)
    return view, buf
