"""Goldens of the ConvNeXt / ConvNeXt V2 feature path (run on the CPU, no download): tests/golden/convnext_tiny_v1.npz,
convnext_tiny_v2.npz, convnext_mid.npz, convnext_full_sampled.npz.

The reference's module imports timm and open_clip; neither is needed: the trunk is transformers' ``ConvNextModel`` / ``ConvNextV2Model``
(the same architecture: 4x4 / 4 stem + LayerNorm, per stage LayerNorm + 2x2 / 2 convolution, blocks of depthwise 7x7, LayerNorm, fc1, erf GELU,
(V2: GRN), fc2, (V1: LayerScale), residual), built from a config and loaded, strict, with ``mvp.convnext.engine_to_hf`` of the seeded weights
of ``mvp.convnext.random_state_dict``.  Those weights REPLACE the module's own initialisation on purpose: transformers starts
``layer_scale_parameter`` at 1e-6 and GRN ``weight`` / ``bias`` at 0, with which every block is the identity to seven digits and GRN a
no-op.  LayerScale is uniform in +-[0.5, 1.5], GRN gamma / beta N(0, 1), LayerNorm weights / biases, convolution and linear biases O(1); the
generator checks that every block changes its input by more than 10 % in relative L2 and that every LayerNorm has eps == 1e-6.

Around the trunk the reference wrapper's forward is restated (evals/models/convnext.py:81-108): center_padding to a multiple of 16 (:82,
utils.py:55-72), out_hw = (H // 16, W // 16) (:83-84), the stem and the stages with the stage outputs tapped (:87-98; transformers'
``hidden_states[1:]`` are those outputs; no final norm, no head, add_norm off), 'dense' = F.interpolate(x, out_hw, mode="bilinear") (:103),
'gap' = x.mean(dim=(2, 3)) (:105).  The model runs in float64; everything is stored in fp32.

tiny (stored in full): widths 64/128/192/256, depths 1/1/2/1, B = 2, V1 and V2, at 48 x 80 (maps 12x20, 6x10, 3x5, 1x2: smaller than the 7x7
window, odd sides floored by the 2x2 / 2 convolutions) and 50 x 75 (padded to 64 x 80).
mid: widths 128/256/512/1024, depths 1/1/2/1, 64 x 96, B = 2, V1 and V2: 4096 sampled elements per tap.
full: ConvNeXt-B and V2-B (3/3/27/3) at 224^2, B = 2: 4096 sampled elements per stage output and of the last tap's dense map."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "midvision-probe_amd"))
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
sys.path.insert(0, os.path.join(REPO, "tests"))

from make_goldens import save_golden  # noqa: E402
from make_goldens_dinov2 import sample_index  # noqa: E402
from mvp import convnext as cnx  # noqa: E402

TINY = dict(widths=(64, 128, 192, 256), depths=(1, 1, 2, 1), sizes=((48, 80), (50, 75)), B=2, seed=91)
MID = dict(widths=(128, 256, 512, 1024), depths=(1, 1, 2, 1), sizes=((64, 96),), B=2, seed=92)
FULL = dict(widths=cnx.WIDTHS_B, depths=cnx.DEPTHS_B, sizes=((224, 224),), B=2, seed=93)


def images(cfg, size) -> torch.Tensor:
    return torch.randn(cfg["B"], 3, *size, generator=torch.Generator().manual_seed(cfg["seed"] + 100 + size[0]))


def state_dict(cfg, v2: bool):
    """The seeded weights of a fixture in the engine's layout."""
    return cnx.random_state_dict(cfg["widths"], cfg["depths"], v2=v2, seed=cfg["seed"] + (1000 if v2 else 0))


def checksums(sd) -> np.ndarray:
    last = max(int(k.split(".")[3]) for k in sd if k.startswith("stages.2.blocks."))
    keys = ["stem.0.weight", "stem.1.bias", "stages.1.downsample.1.weight", "stages.0.blocks.0.conv_dw.weight", f"stages.2.blocks.{last}.mlp.fc2.weight",
            "stages.3.blocks.0.norm.weight", "stages.3.blocks.0.mlp.grn.bias" if "stages.3.blocks.0.mlp.grn.bias" in sd else "stages.3.blocks.0.gamma"]
    return np.array([float(sd[k].double().abs().sum()) for k in keys])


def reference_model(cfg, sd, v2: bool):
    from transformers import ConvNextConfig, ConvNextModel, ConvNextV2Config, ConvNextV2Model

    Cfg, Model = (ConvNextV2Config, ConvNextV2Model) if v2 else (ConvNextConfig, ConvNextModel)
    net = Model(Cfg(hidden_sizes=list(cfg["widths"]), depths=list(cfg["depths"]), hidden_act="gelu", layer_norm_eps=1e-6))
    full = {k: v for k, v in net.state_dict().items() if k.startswith("layernorm.")}  # the pooled output's norm: never run on the tap path
    full.update(cnx.engine_to_hf(sd))
    net.load_state_dict(full, strict=True)
    n_ln = 0
    for mod in net.modules():
        if "LayerNorm" in type(mod).__name__:
            assert mod.eps == 1e-6, (type(mod).__name__, mod.eps)
            n_ln += 1
    assert n_ln == 1 + 3 + sum(cfg["depths"]) + 1, n_ln
    return net.double().eval()


def reference_outputs(cfg, sd, v2, size):
    """convnext.py:81-108 around the transformers trunk -> (stage outputs NCHW, out_hw, per-block relative change)."""
    net = reference_model(cfg, sd, v2)
    change = []

    def hook(mod, inp, out):
        change.append(float((out - inp[0]).norm() / inp[0].norm()))

    for stage in net.encoder.stages:
        for layer in stage.layers:
            layer.register_forward_hook(hook)
    x = images(cfg, size).double()
    _, _, h, w = x.shape
    dh, dw = h % 16, w % 16
    if dh or dw:  # utils.py:55-72
        ph, pw = 16 - dh, 16 - dw
        x = F.pad(x, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2))
    out_hw = (x.shape[-2] // 16, x.shape[-1] // 16)
    with torch.no_grad():
        hs = net(x, output_hidden_states=True).hidden_states
    assert len(hs) == 5 and len(change) == sum(cfg["depths"])
    assert min(change) > 0.1, f"a block changes its input by only {min(change):.3f} in relative L2: the fixture would not test it"
    return list(hs[1:]), out_hw, change


def golden_tiny(v2: bool):
    sd = state_dict(TINY, v2)
    out = {"checksums": checksums(sd)}
    for size in TINY["sizes"]:
        tag = f"s{size[0]}_"
        stages, out_hw, change = reference_outputs(TINY, sd, v2, size)
        out[tag + "images"] = images(TINY, size).numpy()
        out[tag + "block_change"] = np.array(change)
        for j, m in enumerate(stages):
            out[f"{tag}stage{j}"] = m.float().numpy()
            out[f"{tag}dense{j}"] = F.interpolate(m, out_hw, mode="bilinear").float().numpy()
            out[f"{tag}gap{j}"] = m.mean(dim=(2, 3)).float().numpy()
    save_golden("convnext_tiny_v2.npz" if v2 else "convnext_tiny_v1.npz", out)


def golden_sampled(name, cfg):
    out = {}
    for v2 in (False, True):
        tag = "v2_" if v2 else "v1_"
        sd = state_dict(cfg, v2)
        out[tag + "checksums"] = checksums(sd)
        (size,) = cfg["sizes"]
        stages, out_hw, change = reference_outputs(cfg, sd, v2, size)
        out[tag + "block_change"] = np.array(change)
        for j, m in enumerate(stages):
            m = m.float().numpy()
            out[f"{tag}stage{j}"] = m.reshape(-1)[sample_index(m.size)]
            out[f"{tag}stage{j}_shape"] = np.array(m.shape)
        d = F.interpolate(stages[-1], out_hw, mode="bilinear").float().numpy()
        out[tag + "dense3"] = d.reshape(-1)[sample_index(d.size)]
        out[tag + "dense3_shape"] = np.array(d.shape)
    save_golden(name, out)


if __name__ == "__main__":
    torch.manual_seed(0)
    golden_tiny(False)
    golden_tiny(True)
    golden_sampled("convnext_mid.npz", MID)
    golden_sampled("convnext_full_sampled.npz", FULL)
    print("wrote tests/golden/convnext_tiny_v1.npz, convnext_tiny_v2.npz, convnext_mid.npz, convnext_full_sampled.npz")
