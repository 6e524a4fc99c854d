"""Torch restatement of the BEiT v2 feature path (the reference's wrapper, evals/models/beit_v2.py:248-287, around
impl_utils/beit_model.py's VisionTransformer): bilinear resize (align_corners=False) to the model's image size -> patch convolution ->
class token, no position table -> pre-norm blocks (LayerNorm eps 1e-6, qkv with bias cat(q_bias, 0, v_bias), softmax(q k^T * scale +
bias[h]) with the block's own relative-position bias, LayerScale on both branches, erf GELU) -> ``fc_norm`` over ALL tokens -> the same
blocks AGAIN, taps taken in this second pass -> train-mode BatchNorm1d over all B * N tokens on the tap only (``add_norm``) -> dense
maps of the patch tokens.  The bias index is written out here per (query, key) pair, independently of mvp.vit.rel_pos_index.

State dicts use the engine layout (mvp.backbone.beit_to_engine).  Runs in whatever dtype its inputs have.  Test infrastructure only."""
from __future__ import annotations

from typing import Dict, List, Sequence

import torch
import torch.nn.functional as F

from oracle import vit as ovit

StateDict = Dict[str, torch.Tensor]


def dense_bias(table: torch.Tensor, gh: int, gw: int) -> torch.Tensor:
    """[rows, H] -> [H, N, N], N = 1 + gh * gw, pair by pair."""
    rows, H = table.shape
    assert rows == (2 * gh - 1) * (2 * gw - 1) + 3
    N = 1 + gh * gw
    out = torch.empty(H, N, N, dtype=table.dtype)
    for q in range(N):
        for k in range(N):
            if q == 0 and k == 0:
                r = rows - 1
            elif q == 0:
                r = rows - 3  # cls -> token
            elif k == 0:
                r = rows - 2  # token -> cls
            else:
                yq, xq, yk, xk = (q - 1) // gw, (q - 1) % gw, (k - 1) // gw, (k - 1) % gw
                r = (yq - yk + gh - 1) * (2 * gw - 1) + (xq - xk + gw - 1)
            out[:, q, k] = table[r]
    return out


def block(sd: StateDict, i: int, x: torch.Tensor, heads: int, bias: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    p = f"blocks.{i}."
    B, N, C = x.shape
    d = C // heads
    y = F.layer_norm(x, (C,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
    qkv = F.linear(y, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"]).reshape(B, N, 3, heads, d).permute(2, 0, 3, 1, 4)
    a = ((qkv[0] * d ** -0.5) @ qkv[1].transpose(-2, -1) + bias[None]).softmax(dim=-1)
    y = F.linear((a @ qkv[2]).transpose(1, 2).reshape(B, N, C), sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
    x = x + sd[p + "ls1.gamma"] * y
    y = F.layer_norm(x, (C,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
    y = F.linear(F.gelu(F.linear(y, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
    return x + sd[p + "ls2.gamma"] * y


def features(sd: StateDict, images: torch.Tensor, layers: Sequence[int], *, img_size, patch: int = 16, add_norm: bool = False,
             replay: bool = True, return_cls: bool = False, biases=None) -> List[torch.Tensor]:
    """One dense NCHW map per tap (``return_cls``: the un-normalised class token of the single tap instead)."""
    sd = {k: v.to(images.dtype) for k, v in sd.items()}
    img_size = (img_size, img_size) if isinstance(img_size, int) else tuple(img_size)
    images = F.interpolate(images, size=img_size, mode="bilinear", align_corners=False)
    gh, gw = img_size[0] // patch, img_size[1] // patch
    x = F.conv2d(images, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=patch).flatten(2).transpose(1, 2)
    C = x.shape[-1]
    heads = C // 64
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    x = torch.cat((sd["cls_token"].expand(x.shape[0], -1, -1), x), dim=1)
    if biases is None:
        biases = [dense_bias(sd[f"blocks.{i}.attn.rel_pos_bias_table"], gh, gw) for i in range(depth)]
    if replay:
        for i in range(depth):
            x = block(sd, i, x, heads, biases[i])
        x = F.layer_norm(x, (C,), sd["fc_norm.weight"], sd["fc_norm.bias"], 1e-6)
    layers = list(layers)
    taps = []
    for i in range(max(layers) + 1):
        x = block(sd, i, x, heads, biases[i])
        if i in layers:
            if len(layers) == 1 and return_cls:
                return [x[:, 0]]
            taps.append(ovit.batchnorm_tokens_train(x, None, None) if add_norm else x)
    return [t[:, 1:].permute(0, 2, 1).reshape(t.shape[0], C, gh, gw) for t in taps]
