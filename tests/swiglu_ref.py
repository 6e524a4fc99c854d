"""Torch restatement of DINOv2's SwiGLU models (ViT-g/14): the feature path of tests/dinov2_ref.py with SwiGLUFFNFused in the place
of the fc1 / GELU / fc2 MLP — x12 = w12(y); x1, x2 = x12.chunk(2, -1); w3(silu(x1) * x2) — and nothing else changed: the same
tokens, attention, LayerScale, taps and outputs, imported from dinov2_ref.py and oracle/vit.py.

State dicts use the hub layout as mvp.backbone.dinov2_hub_to_engine leaves it (``blocks.i.mlp.w12.*`` [2H, C], ``blocks.i.mlp.w3.*``
[C, H]).  Runs in whatever dtype its inputs have (fp64 on the CPU for the tests).  Test infrastructure only."""
from __future__ import annotations

from typing import List, Sequence

import torch
import torch.nn.functional as F

import dinov2_ref
from oracle import vit as ovit

StateDict = dinov2_ref.StateDict


def hidden_width(embed_dim: int) -> int:
    """SwiGLUFFNFused.__init__: hidden_features = (int(hidden_features * 2 / 3) + 7) // 8 * 8 with hidden_features = 4 C."""
    return (int(4 * embed_dim * 2 / 3) + 7) // 8 * 8


def gate(x12: torch.Tensor) -> torch.Tensor:
    """silu(x1) * x2 of x12 = x1 | x2."""
    x1, x2 = x12.chunk(2, dim=-1)
    return F.silu(x1) * x2


def ffn(sd: StateDict, prefix: str, y: torch.Tensor) -> torch.Tensor:
    """SwiGLUFFNFused.forward with the weights under ``prefix`` (``blocks.i.mlp.``)."""
    x12 = F.linear(y, sd[prefix + "w12.weight"], sd[prefix + "w12.bias"])
    return F.linear(gate(x12), sd[prefix + "w3.weight"], sd[prefix + "w3.bias"])


def block(sd: StateDict, i: int, x: torch.Tensor, heads: int, eps: float = 1e-6) -> torch.Tensor:
    """NestedTensorBlock (eval) with the SwiGLU FFN: x + ls1(attn(norm1(x))), then x + ls2(ffn(norm2(x)))."""
    p = f"blocks.{i}."
    C = x.shape[-1]
    y = F.layer_norm(x, (C,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
    x = x + sd[p + "ls1.gamma"] * ovit.attention(sd, p + "attn.", y, heads)
    y = F.layer_norm(x, (C,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
    return x + sd[p + "ls2.gamma"] * ffn(sd, p + "mlp.", y)


def dense_features(sd: StateDict, images: torch.Tensor, layers: Sequence[int], *, patch: int = 14, add_norm: bool = True,
                   output: str = "dense-cls", return_tokens: bool = False) -> List[torch.Tensor]:
    """dinov2_ref.dense_features for a SwiGLU state dict: one output per tap (NCHW for dense / dense-cls)."""
    sd = {k: v.to(images.dtype) for k, v in sd.items()}
    heads = sd["cls_token"].shape[-1] // 64
    images = ovit.center_padding(images, patch)
    h, w = images.shape[-2] // patch, images.shape[-1] // patch
    x = dinov2_ref.prepare_tokens(sd, images, patch)
    layers = list(layers)
    taps = []
    for i in range(max(layers) + 1):
        x = block(sd, i, x, heads)
        if i in layers:
            taps.append(ovit.batchnorm_tokens_train(x, None, None) if add_norm else x)
    if return_tokens:
        return taps
    return [ovit.tokens_to_output(output, t[:, -h * w:], t[:, 0], (h, w)) for t in taps]
