"""Plain-torch fp64 restatement of the SAM image encoder's forward as the reference wrapper runs it (evals/models/sam.py:85-113 around
segment_anything's ImageEncoderViT), written from the formulas: patch embedding, the [1, S, S, C] position table (bicubic resample when
the grid differs), per block LayerNorm -> (zero-padded 'w x w' windows | the whole grid) -> qkv -> softmax(q k^T / 8 + q . Rh[yq, yk] +
q . Rw[xq, xk]) v on the UNSCALED q for the two extra terms -> proj -> residual, then the erf-GELU MLP.  Pad rows are zero after norm1 and are
real keys (k = b_k, v = b_v).  Test infrastructure only: tests/test_sam_cpu.py pins it to the goldens built from transformers'
SamVisionEncoder; GPU tests use it where they need values the goldens do not hold (another size, intermediate tensors)."""
from __future__ import annotations

import torch
import torch.nn.functional as F


def rel_pos(q_size: int, k_size: int, table: torch.Tensor) -> torch.Tensor:
    """get_rel_pos + gather: [L, 64] -> [q_size, k_size, 64] in the table's dtype (linear interpolation to 2 max(q, k) - 1 rows)."""
    n = 2 * max(q_size, k_size) - 1
    if table.shape[0] != n:
        table = F.interpolate(table.t()[None], size=n, mode="linear")[0].t()
    q = torch.arange(q_size)[:, None] * max(k_size / q_size, 1.0)
    k = torch.arange(k_size)[None, :] * max(q_size / k_size, 1.0)
    return table[((q - k) + (k_size - 1) * max(q_size / k_size, 1.0)).long()]


def block_windows(sd) -> list:
    s0 = sd["pos_embed"].shape[1]
    out, i = [], 0
    while f"blocks.{i}.attn.rel_pos_h" in sd:
        side = (sd[f"blocks.{i}.attn.rel_pos_h"].shape[0] + 1) // 2
        out.append(0 if side == s0 else side)
        i += 1
    return out


def attention(x, p, sd, heads, keep=None):
    """x [B', h, w, C] (a window or the whole grid) -> [B', h, w, C]."""
    Bp, h, w, C = x.shape
    qkv = F.linear(x.reshape(Bp, h * w, C), sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"]).reshape(Bp, h * w, 3, heads, 64).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]  # [B', H, N, 64]
    Rh, Rw = rel_pos(h, h, sd[p + "attn.rel_pos_h"]), rel_pos(w, w, sd[p + "attn.rel_pos_w"])
    rq = q.reshape(Bp, heads, h, w, 64)
    rel_h = torch.einsum("bnhwc,hkc->bnhwk", rq, Rh)
    rel_w = torch.einsum("bnhwc,wkc->bnhwk", rq, Rw)
    if keep is not None:
        keep.update(rel_h=rel_h, rel_w=rel_w, Rh=Rh, Rw=Rw)
    logit = (q * 64 ** -0.5) @ k.transpose(-2, -1)
    logit = (logit.reshape(Bp, heads, h, w, h, w) + rel_h[..., :, None] + rel_w[..., None, :]).reshape(Bp, heads, h * w, h * w)
    o = (logit.softmax(-1) @ v).transpose(1, 2).reshape(Bp, h, w, C)
    return F.linear(o, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])


def block(x, i, sd, heads, window, keep=None):
    p = f"blocks.{i}."
    B, gh, gw, C = x.shape
    y = F.layer_norm(x, (C,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-6)
    if window:
        ph, pw = (window - gh % window) % window, (window - gw % window) % window
        y = F.pad(y, (0, 0, 0, pw, 0, ph))
        Hp, Wp = gh + ph, gw + pw
        y = y.reshape(B, Hp // window, window, Wp // window, window, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, window, window, C)
        y = attention(y, p, sd, heads, keep)
        y = y.reshape(B, Hp // window, Wp // window, window, window, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)[:, :gh, :gw]
    else:
        y = attention(y, p, sd, heads, keep)
    x = x + y
    y = F.layer_norm(x, (C,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], 1e-6)
    y = F.linear(F.gelu(F.linear(y, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
    return x + y


def pos_table(sd, gh, gw):
    """The checkpoint's table at gh x gw: itself, or its bicubic resample (align_corners=False, no antialias) in its own dtype."""
    t = sd["pos_embed"]
    if (gh, gw) != tuple(t.shape[1:3]):
        t = F.interpolate(t.permute(0, 3, 1, 2), size=(gh, gw), mode="bicubic").permute(0, 2, 3, 1)
    return t


def forward(sd, images, layers, keep_blocks=()):
    """Engine-layout state dict (any dtype; converted to fp64) + images [B, 3, H, W] -> (list of NCHW fp64 maps after the blocks in
    ``layers``, {block: dict(rel_h, rel_w, Rh, Rw)} for ``keep_blocks``)."""
    sd = {k: v.double() for k, v in sd.items()}
    x = F.conv2d(images.double(), sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=16).permute(0, 2, 3, 1)
    B, gh, gw, C = x.shape
    x = x + pos_table(sd, gh, gw)
    wins, outs, kept = block_windows(sd), [], {}
    for i, w in enumerate(wins):
        keep = {} if i in keep_blocks else None
        x = block(x, i, sd, C // 64, w, keep)
        if keep is not None:
            kept[i] = keep
        if i in layers:
            outs.append(x.permute(0, 3, 1, 2).contiguous())
            if len(outs) == len(layers):
                break
    return outs, kept
