"""Goldens of the CroCo and CroCo v2 feature paths (run on CPU, no download): tests/golden/croco_tiny.npz, croco_full_sampled.npz.

The model is the reference's own ``CroCoNet`` (evals/models/croco_models/croco.py), imported at generation time from the reference
checkout behind a stub package (its ``evals/models/__init__.py`` cannot be imported), built from the ``croco_kwargs`` of
``mvp.backbone.random_croco_state_dict`` and loaded with that dict's seeded encoder weights (decoder tensors the seeded dict does not carry
keep the model's own init: the encoder path never reads them).  Without the compiled cuRoPE2D the reference falls back to its own torch
``RoPE2D`` (pos_embed.py:110-157), which is what runs here.  Around the model the reference wrapper's ``forward`` is replayed
(croco.py:138-178): bilinear resize (align_corners=False) to the model's image size — the wrapper's literal 224 generalised to
``img_size`` —, ``patch_embed``, ``enc_pos_embed`` when the model has one, ``enc_blocks`` one by one with the patch positions, taps after
blocks n/4-1, n/2-1, 3n/4-1, n-1, without and with ``add_norm`` (a fresh train-mode BatchNorm1d over all B * N tokens), then
``tokens_to_output('dense')`` from the reference's evals/models/utils.py.  Everything in fp64.

Tiny fixtures stored in full (fp32): both position forms, ``img_size=(64, 96)`` (a non-square 4 x 6 grid: a y / x swap shows), C = 128,
2 heads, depth 4, images [2, 3, 80, 112]; plus weight checksums.  Full size: ViT-B/16 at 224^2, B = 2, both forms, 4096 sampled elements
per tap and each tap's shape."""
from __future__ import annotations

import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("MVP_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "midvision-probe_amd"))
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

from make_goldens import save_golden  # noqa: E402
from make_goldens_dinov2 import _reference_utils, sample_index  # noqa: E402,F401
from mvp import backbone as bb  # noqa: E402

# name -> (position form, seed)
TINY = {"croco": ("cosine", 51), "crocov2": ("RoPE100", 52)}
TINY_DIMS = dict(C=128, depth=4, img_size=(64, 96), size=(80, 112), B=2)
FULL = {"croco_b16": ("cosine", 61), "crocov2_b16": ("RoPE100", 62)}
FULL_SHAPE = (2, 224, 224)


def tiny_images() -> torch.Tensor:
    return torch.randn(TINY_DIMS["B"], 3, *TINY_DIMS["size"], generator=torch.Generator().manual_seed(7))


def tiny_state_dict(name: str):
    """The seeded weights of a tiny fixture in the published layout ({"model": ..., "croco_kwargs": ...})."""
    form, seed = TINY[name]
    return bb.random_croco_state_dict(TINY_DIMS["C"], TINY_DIMS["depth"], 16, TINY_DIMS["img_size"], pos_embed=form, seed=seed)


def full_state_dict(key: str):
    form, seed = FULL[key]
    return bb.random_croco_state_dict(768, 12, 16, 224, pos_embed=form, seed=seed)


def full_images() -> torch.Tensor:
    B, H, W = FULL_SHAPE
    return torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(B * 1000 + H + W + 9))


def checksums(ckpt) -> np.ndarray:
    sd = bb.croco_to_engine(ckpt)
    last = max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    keys = ["patch_embed.proj.weight", "patch_embed.proj.bias", "blocks.0.attn.qkv.weight", "blocks.0.attn.qkv.bias", f"blocks.{last}.mlp.fc2.weight", "blocks.1.norm2.bias"]
    keys += ["pos_embed"] if "pos_embed" in sd else []
    return np.array([float(sd[k].double().abs().sum()) for k in keys])


def _croconet():
    """The reference's CroCoNet class: croco_models is imported as a sub-package of a stub (the reference's evals.models package
    re-exports names that no longer exist)."""
    if "mvp_ref_models" not in sys.modules:
        stub = types.ModuleType("mvp_ref_models")
        stub.__path__ = [os.path.join(REF, "evals", "models")]
        sys.modules["mvp_ref_models"] = stub
    return importlib.import_module("mvp_ref_models.croco_models.croco").CroCoNet


def reference_model(ckpt):
    net = _croconet()(**ckpt["croco_kwargs"])
    res = net.load_state_dict(ckpt["model"], strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    assert all(k.startswith(("dec_blocks.", "dec_norm.", "decoder_embed.", "prediction_head.")) for k in res.missing_keys), res.missing_keys
    assert net.pos_embed == ckpt["croco_kwargs"]["pos_embed"] and (net.rope is None) == (net.pos_embed == "cosine")
    return net.double().eval()


def reference_features(ckpt, images: torch.Tensor, add_norm: bool = False):
    """croco.py:138-178 around the reference model: one dense map per tap (return_multilayer)."""
    ut = _reference_utils()
    net = reference_model(ckpt)
    P = net.patch_embed.patch_size[0]
    depth = len(net.enc_blocks)
    layers = [depth // 4 - 1, depth // 2 - 1, depth // 4 * 3 - 1, depth - 1]
    with torch.no_grad():
        images = F.interpolate(images.double(), size=net.patch_embed.img_size, mode="bilinear", align_corners=False)
        h, w = images.shape[-2] // P, images.shape[-1] // P
        x, pos = net.patch_embed(images)
        if net.enc_pos_embed is not None:
            x = x + net.enc_pos_embed[None, ...]
        embeds = []
        for i, blk in enumerate(net.enc_blocks):
            x = blk(x, pos)
            if i in layers:
                if add_norm:
                    bn = torch.nn.BatchNorm1d(x.shape[-1]).double().train()
                    embeds.append(bn(x.permute(0, 2, 1)).permute(0, 2, 1))
                else:
                    embeds.append(x)
        return [ut.tokens_to_output("dense", e, None, (h, w)) for e in embeds]


def golden_tiny():
    out = {"images": tiny_images().numpy()}
    for name in TINY:
        ckpt = tiny_state_dict(name)
        out[f"{name}_checksums"] = checksums(ckpt)
        for tag, norm in (("dense", False), ("norm", True)):
            for j, m in enumerate(reference_features(ckpt, tiny_images(), add_norm=norm)):
                out[f"{name}_{tag}_tap{j}"] = m.float().numpy()
    save_golden("croco_tiny.npz", out)


def golden_full():
    out = {}
    B, H, W = FULL_SHAPE
    for key in FULL:
        ckpt = full_state_dict(key)
        out[f"{key}_checksums"] = checksums(ckpt)
        for j, o in enumerate(reference_features(ckpt, full_images())):
            o = o.float().numpy()
            out[f"{key}_{B}x{H}x{W}_tap{j}"] = o.reshape(-1)[sample_index(o.size)]
            out[f"{key}_{B}x{H}x{W}_tap{j}_shape"] = np.array(o.shape)
    save_golden("croco_full_sampled.npz", out)


if __name__ == "__main__":
    torch.manual_seed(0)
    golden_tiny()
    golden_full()
    print("wrote tests/golden/croco_tiny.npz, tests/golden/croco_full_sampled.npz")
