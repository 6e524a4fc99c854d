"""Torch restatement of the CLIP and SigLIP feature paths (the reference's wrappers, evals/models/clip.py:67-101 and siglip.py:58-93,
around open_clip's / timm's image towers): center padding -> patch convolution (CLIP: no bias) -> class embedding (CLIP only) ->
position table resized to the grid when its entry COUNT differs (bicubic, antialiased; the CLS entry kept apart) -> ln_pre (CLIP only)
-> pre-norm blocks with QuickGELU / erf GELU / tanh-GELU -> taps -> tokens_to_output.

``add_norm=True`` is this project's definition: train-mode per-channel BatchNorm1d over ALL tokens of the batch at each
tap, the DINO wrapper's rule — the reference's own add_norm lines cannot run.

State dicts use the engine layout (mvp.backbone.clip_to_engine / siglip_to_engine).  Runs in whatever dtype / device its inputs have
(fp64 on CPU for the goldens and tests).  Test infrastructure only."""
from __future__ import annotations

from typing import Dict, List, Sequence

import torch
import torch.nn.functional as F

from oracle import vit as ovit

StateDict = Dict[str, torch.Tensor]


def activation(name: str, x: torch.Tensor) -> torch.Tensor:
    if name == "quick_gelu":
        return x * torch.sigmoid(1.702 * x)
    if name == "gelu_tanh":
        return F.gelu(x, approximate="tanh")
    if name == "gelu":
        return F.gelu(x)
    raise ValueError(name)


def resize_pos_embed(pos: torch.Tensor, hw, has_cls: bool) -> torch.Tensor:
    """utils.py:12-52 on a [n, C] table."""
    c0 = 1 if has_cls else 0
    n = pos.shape[0] - c0
    if n == hw[0] * hw[1]:
        return pos
    side = int(n ** 0.5)
    grid = pos[c0:].reshape(1, side, side, -1).permute(0, 3, 1, 2)
    grid = F.interpolate(grid, hw, mode="bicubic", align_corners=False, antialias=True)
    return torch.cat((pos[:c0], grid.permute(0, 2, 3, 1).reshape(hw[0] * hw[1], -1)), dim=0)


def prepare_tokens(sd: StateDict, images: torch.Tensor, patch: int, eps: float, resize: bool = True) -> torch.Tensor:
    B = images.shape[0]
    x = F.conv2d(images, sd["patch_embed.proj.weight"], sd.get("patch_embed.proj.bias"), stride=patch)
    hw = tuple(x.shape[-2:])
    x = x.flatten(2).transpose(1, 2)
    has_cls = "cls_token" in sd
    if has_cls:
        x = torch.cat((sd["cls_token"].reshape(1, 1, -1).expand(B, -1, -1), x), dim=1)
    x = x + (resize_pos_embed(sd["pos_embed"][0], hw, has_cls) if resize else sd["pos_embed"][0])
    if "norm_pre.weight" in sd:
        x = F.layer_norm(x, (x.shape[-1],), sd["norm_pre.weight"], sd["norm_pre.bias"], eps)
    return x


def block(sd: StateDict, i: int, x: torch.Tensor, heads: int, eps: float, act: str) -> torch.Tensor:
    p = f"blocks.{i}."
    C = x.shape[-1]
    y = F.layer_norm(x, (C,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
    x = x + ovit.attention(sd, p + "attn.", y, heads)
    y = F.layer_norm(x, (C,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
    y = F.linear(activation(act, F.linear(y, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
    return x + y


def dense_features(sd: StateDict, images: torch.Tensor, layers: Sequence[int], *, patch: int, act: str, eps: float, output: str = "dense",
                   add_norm: bool = False, bn_affine=None, return_tokens: bool = False) -> List[torch.Tensor]:
    """One output per tap.  CLIP: eps 1e-5, act 'quick_gelu' / 'gelu'; SigLIP (no ``cls_token`` in ``sd``): eps 1e-6, act 'gelu_tanh'."""
    sd = {k: v.to(images.dtype) for k, v in sd.items()}
    has_cls = "cls_token" in sd
    heads = sd["pos_embed"].shape[-1] // 64
    images = ovit.center_padding(images, patch)
    h, w = images.shape[-2] // patch, images.shape[-1] // patch
    x = prepare_tokens(sd, images, patch, eps)
    layers = list(layers)
    taps = []
    for i in range(max(layers) + 1):
        x = block(sd, i, x, heads, eps, act)
        if i in layers:
            j = layers.index(i)
            if add_norm:
                wgt, b = bn_affine[j] if bn_affine is not None else (None, None)
                taps.append(ovit.batchnorm_tokens_train(x, wgt, b))
            else:
                taps.append(x)
    if return_tokens:
        return taps
    return [ovit.tokens_to_output(output, t[:, -h * w:], t[:, 0] if has_cls else None, (h, w)) for t in taps]
