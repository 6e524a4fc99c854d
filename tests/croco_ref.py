"""Torch restatement of the CroCo / CroCo v2 feature paths (the reference's wrappers, evals/models/croco.py:133-178 and crocov2.py,
around croco_models.CroCoNet's encoder): bilinear resize (align_corners=False) to the model's image size, no centre padding -> patch
convolution -> the fixed sin-cos table ('cosine') or nothing ('RoPE<freq>') -> pre-norm blocks with biased qkv, erf GELU, LayerNorm
eps 1e-6; under RoPE, q and k of every block are rotated by the token's (y, x) grid position (croco_models/pos_embed.py:110-157:
per head, dims 0..31 by y and 32..63 by x, each half as tokens * cos + rotate_half(tokens) * sin) -> taps -> train-mode BatchNorm1d over
all B * N tokens (``add_norm``) -> tokens_to_output('dense').  There is no class token and the final norm is never applied.

State dicts use the engine layout (mvp.backbone.croco_to_engine).  Runs in whatever dtype / device its inputs have (fp64 on CPU for the
goldens and tests).  Test infrastructure only."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import torch
import torch.nn.functional as F

from oracle import vit as ovit

StateDict = Dict[str, torch.Tensor]


def rope_tables(freq: float, rows: int, dtype=torch.float64) -> Tuple[torch.Tensor, torch.Tensor]:
    """RoPE2D.get_cos_sin (pos_embed.py:119-129) for D = 32: the angles are formed in fp32 as the reference forms them, cast to ``dtype``,
    and cos / sin taken there."""
    inv_freq = 1.0 / (freq ** (torch.arange(0, 32, 2).float() / 32))
    t = torch.arange(rows, dtype=inv_freq.dtype)
    freqs = torch.einsum("i,j->ij", t, inv_freq).to(dtype)
    freqs = torch.cat((freqs, freqs), dim=-1)
    return freqs.cos(), freqs.sin()


def rope1d(t: torch.Tensor, pos: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """t [B, H, N, 32], pos [N]: t * cos + rotate_half(t) * sin."""
    c, s = cos[pos][None, None], sin[pos][None, None]
    return t * c + torch.cat((-t[..., 16:], t[..., :16]), dim=-1) * s


def rope2d(t: torch.Tensor, hw: Tuple[int, int], cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """t [B, H, N, 64] over an h x w grid in row-major token order (y = n // w, x = n % w)."""
    h, w = hw
    n = torch.arange(h * w)
    return torch.cat((rope1d(t[..., :32], n // w, cos, sin), rope1d(t[..., 32:], n % w, cos, sin)), dim=-1)


def attention(sd: StateDict, prefix: str, x: torch.Tensor, heads: int, hw, tables) -> torch.Tensor:
    """croco_models/blocks.py:94-111."""
    B, N, C = x.shape
    d = C // heads
    qkv = F.linear(x, sd[prefix + "qkv.weight"], sd[prefix + "qkv.bias"]).reshape(B, N, 3, heads, d).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    if tables is not None:
        q, k = rope2d(q, hw, *tables), rope2d(k, hw, *tables)
    a = ((q @ k.transpose(-2, -1)) * (d ** -0.5)).softmax(dim=-1)
    return F.linear((a @ v).transpose(1, 2).reshape(B, N, C), sd[prefix + "proj.weight"], sd[prefix + "proj.bias"])


def block(sd: StateDict, i: int, x: torch.Tensor, heads: int, hw, tables, eps: float = 1e-6) -> torch.Tensor:
    p = f"blocks.{i}."
    C = x.shape[-1]
    y = F.layer_norm(x, (C,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
    x = x + attention(sd, p + "attn.", y, heads, hw, tables)
    y = F.layer_norm(x, (C,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
    return x + F.linear(F.gelu(F.linear(y, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])


def dense_features(sd: StateDict, images: torch.Tensor, layers: Sequence[int], *, pos_embed: str, img_size, patch: int = 16,
                   add_norm: bool = False, bn_affine=None, return_tokens: bool = False) -> List[torch.Tensor]:
    """One dense NCHW map per tap.  ``pos_embed``: 'cosine' (``sd['pos_embed']`` [1, n, C] is added) or 'RoPE<freq>'."""
    sd = {k: v.to(images.dtype) for k, v in sd.items()}
    img_size = (img_size, img_size) if isinstance(img_size, int) else tuple(img_size)
    images = F.interpolate(images, size=img_size, mode="bilinear", align_corners=False)
    h, w = img_size[0] // patch, img_size[1] // patch
    x = F.conv2d(images, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=patch).flatten(2).transpose(1, 2)
    heads = x.shape[-1] // 64
    tables = None
    if pos_embed == "cosine":
        x = x + sd["pos_embed"][0]
    else:
        tables = rope_tables(float(pos_embed[len("RoPE"):]), max(h, w), images.dtype)
    layers = list(layers)
    taps = []
    for i in range(max(layers) + 1):
        x = block(sd, i, x, heads, (h, w), tables)
        if i in layers:
            if add_norm:
                wgt, b = bn_affine[layers.index(i)] if bn_affine is not None else (None, None)
                taps.append(ovit.batchnorm_tokens_train(x, wgt, b))
            else:
                taps.append(x)
    if return_tokens:
        return taps
    return [ovit.tokens_to_output("dense", t, None, (h, w)) for t in taps]
