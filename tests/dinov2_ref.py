"""Torch restatement of the DINOv2 feature path (the reference's DINO wrapper with dino_name="dinov2", evals/models/dino.py:164-210,
around the torch.hub DinoVisionTransformer): center padding -> prepare_tokens_with_masks (patch embed, CLS, resampled pos-embed,
register tokens after CLS without pos-embed) -> blocks with LayerScale on both residual branches -> taps with train-mode BatchNorm1d
over ALL tokens (CLS and registers included) -> the last h*w tokens as the spatial map.

State dicts use the hub layout (``register_tokens``, ``blocks.i.ls1.gamma`` / ``ls2.gamma``), chunked / mask_token / norm keys already
dropped (mvp.backbone.dinov2_hub_to_engine).  Runs in whatever dtype / device its inputs have (fp64 on CPU for the goldens and tests).
Test infrastructure only."""
from __future__ import annotations

import math
from typing import Dict, List, Sequence

import torch
import torch.nn.functional as F

from oracle import vit as ovit

StateDict = Dict[str, torch.Tensor]


def interpolate_pos_encoding(pos_embed: torch.Tensor, d2: int, d3: int, patch: int, registers: bool) -> torch.Tensor:
    """DinoVisionTransformer.interpolate_pos_encoding: non-register models (interpolate_offset 0.1, no antialias) use the +0.1 scale
    factor — the DINO rule of oracle/vit.py; register models (offset 0, antialias) resample to ``size`` = the grid, antialiased."""
    N = pos_embed.shape[1] - 1
    npatch = (d2 // patch) * (d3 // patch)
    if npatch == N and d2 == d3:
        return pos_embed
    if not registers:
        return ovit.interpolate_pos_encoding(pos_embed, npatch, d2, d3, patch)
    dim = pos_embed.shape[-1]
    side = int(math.sqrt(N))
    grid = pos_embed[:, 1:].reshape(1, side, side, dim).permute(0, 3, 1, 2)
    grid = F.interpolate(grid, size=(d2 // patch, d3 // patch), mode="bicubic", antialias=True)
    return torch.cat((pos_embed[:, :1], grid.permute(0, 2, 3, 1).reshape(1, -1, dim)), dim=1)


def prepare_tokens(sd: StateDict, images: torch.Tensor, patch: int = 14) -> torch.Tensor:
    B, _, d2, d3 = images.shape
    x = F.conv2d(images, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=patch).flatten(2).transpose(1, 2)
    x = torch.cat((sd["cls_token"].expand(B, -1, -1), x), dim=1)
    reg = sd.get("register_tokens")
    x = x + interpolate_pos_encoding(sd["pos_embed"], d2, d3, patch, reg is not None)
    if reg is not None:
        x = torch.cat((x[:, :1], reg.expand(B, -1, -1), x[:, 1:]), dim=1)
    return x


def block(sd: StateDict, i: int, x: torch.Tensor, heads: int, eps: float = 1e-6) -> torch.Tensor:
    """NestedTensorBlock (eval): x + ls1(attn(norm1(x))), then x + ls2(mlp(norm2(x)))."""
    p = f"blocks.{i}."
    C = x.shape[-1]
    y = F.layer_norm(x, (C,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
    x = x + sd[p + "ls1.gamma"] * ovit.attention(sd, p + "attn.", y, heads)
    y = F.layer_norm(x, (C,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
    y = F.linear(F.gelu(F.linear(y, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
    return x + sd[p + "ls2.gamma"] * y


def dense_features(sd: StateDict, images: torch.Tensor, layers: Sequence[int], *, patch: int = 14, add_norm: bool = True,
                   output: str = "dense-cls", bn_affine=None, return_tokens: bool = False) -> List[torch.Tensor]:
    """The reference wrapper's forward for dinov2 (return_kqv False): a list with one output per tap (NCHW for dense / dense-cls)."""
    sd = {k: v.to(images.dtype) for k, v in sd.items()}
    heads = sd["cls_token"].shape[-1] // 64
    images = ovit.center_padding(images, patch)
    h, w = images.shape[-2] // patch, images.shape[-1] // patch
    x = prepare_tokens(sd, images, patch)
    layers = list(layers)
    taps = []
    for i in range(max(layers) + 1):
        x = block(sd, i, x, heads)
        if i in layers:
            j = layers.index(i)
            if add_norm:
                wgt, b = bn_affine[j] if bn_affine is not None else (None, None)
                taps.append(ovit.batchnorm_tokens_train(x, wgt, b))
            else:
                taps.append(x)
    if return_tokens:
        return taps
    return [ovit.tokens_to_output(output, t[:, -h * w:], t[:, 0], (h, w)) for t in taps]
