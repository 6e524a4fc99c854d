"""Goldens of the SAM image-encoder feature path (run on CPU, no download): tests/golden/sam_tiny.npz, sam_mid.npz, sam_full_sampled.npz.

segment_anything is not needed: the model is transformers' ``SamVisionEncoder`` — the same architecture (windowed and global blocks,
``get_rel_pos`` with linear interpolation, the decomposed bias on the unscaled q, zero padding after norm1) — built small from a
``SamVisionConfig`` and loaded, strict, with ``mvp.backbone.engine_to_sam_hf`` of the seeded weights of
``mvp.backbone.random_sam_state_dict`` (plus the module's own neck tensors, which the forward below never runs).  Around it the reference
wrapper's ``forward`` is replayed (evals/models/sam.py:85-113): the bicubic resize of the position table when the size differs
(sam.py:70-83), the patch projection, ``+ pos_embed``, the layers one by one, taps after blocks n/4-1, n/2-1, 3n/4-1, n-1, NHWC -> NCHW.  The
sub-modules are called directly: the encoder's own ``forward`` rejects non-native sizes.  The model is in fp64, but transformers computes
its attention softmax in fp32 (``softmax(..., dtype=torch.float32)``), so these goldens are exact to about 1e-7 relative, not 1e-16 — far
inside the 1e-3 feature contract they serve.

tiny (stored in full, fp32): C = 128, 2 heads, depth 4, native grid 8 (image 128^2), window 3, global blocks 1 and 3; images
[2, 3, 80, 112]: a 5 x 7 grid — non-square, both dimensions padded to the window (5 -> 6, 7 -> 9), pad rows acting as keys, a bicubic table
resize, the global tables interpolated 15 -> 13 rows with gh != gw; plus, for windowed block 0 and global block 1, the module's own
``rel_h`` / ``rel_w`` of the first window / image and the expanded ``Rh`` / ``Rw``.
mid: the same widths, native grid 16, window 14, images 256^2 (16 -> 28: four windows of 196 per image), B = 2: 4096 sampled elements per tap.
full: ViT-B geometry (768, 12 heads, depth 12, native grid 64, window 14, global 2 / 5 / 8 / 11), B = 1, at 224^2 (one window; global
tables 127 -> 27) and 512^2 (grid 32: nine windows; global N = 1024): 4096 samples per tap and the tap shapes.  Weight checksums in each."""
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

from make_goldens import save_golden  # noqa: E402
from make_goldens_dinov2 import sample_index  # noqa: E402
from mvp import backbone as bb  # noqa: E402

TINY = dict(C=128, depth=4, native=8, window=3, global_idx=(1, 3), sizes=((80, 112),), B=2, seed=81)
MID = dict(C=128, depth=4, native=16, window=14, global_idx=(1, 3), sizes=((256, 256),), B=2, seed=82)
FULL = dict(C=768, depth=12, native=64, window=14, global_idx=(2, 5, 8, 11), sizes=((224, 224), (512, 512)), B=1, seed=83)


def images(cfg, size) -> torch.Tensor:
    return torch.randn(cfg["B"], 3, *size, generator=torch.Generator().manual_seed(cfg["seed"] + 100 + size[0]))


def state_dict(cfg):
    """The seeded weights of a fixture in the engine's layout."""
    return bb.random_sam_state_dict(cfg["C"], cfg["depth"], cfg["native"], cfg["window"], cfg["global_idx"], seed=cfg["seed"])


def checksums(sd) -> np.ndarray:
    last = max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    keys = ["pos_embed", "patch_embed.proj.weight", "blocks.0.attn.qkv.weight", "blocks.0.attn.qkv.bias", "blocks.0.attn.rel_pos_h", "blocks.1.attn.rel_pos_w",
            f"blocks.{last}.attn.rel_pos_h", f"blocks.{last}.mlp.fc2.weight", "blocks.1.norm1.bias"]
    return np.array([float(sd[k].double().abs().sum()) for k in keys])


def reference_model(cfg, sd):
    from transformers import SamVisionConfig
    from transformers.models.sam.modeling_sam import SamVisionEncoder

    c = SamVisionConfig(hidden_size=cfg["C"], num_hidden_layers=cfg["depth"], num_attention_heads=cfg["C"] // 64, image_size=16 * cfg["native"], patch_size=16,
                        window_size=cfg["window"], global_attn_indexes=list(cfg["global_idx"]), mlp_dim=4 * cfg["C"], output_channels=32)
    c._attn_implementation = "eager"
    net = SamVisionEncoder(c)
    full = {k: v for k, v in net.state_dict().items() if k.startswith("neck.")}
    full.update(bb.engine_to_sam_hf(sd))
    net.load_state_dict(full, strict=True)
    return net.double().eval()


def reference_outputs(cfg, sd, size, keep=()):
    """sam.py:85-113 around the transformers encoder -> (NCHW taps, {block: (rel_h, rel_w, Rh, Rw)} of the module's own attention)."""
    net = reference_model(cfg, sd)
    depth = cfg["depth"]
    layers = [depth // 4 - 1, depth // 2 - 1, depth // 4 * 3 - 1, depth - 1]
    kept, taps = {}, []
    with torch.no_grad():
        h, w = size[0] // 16, size[1] // 16
        pos = net.pos_embed.data
        if (h, w) != tuple(pos.shape[1:3]):
            pos = F.interpolate(pos.permute(0, 3, 1, 2), size=(h, w), mode="bicubic").permute(0, 2, 3, 1)  # sam.py:77-81
        x = net.patch_embed.projection(images(cfg, size).double()).permute(0, 2, 3, 1) + pos  # (patch_embed's own forward rejects non-native sizes)
        for i, layer in enumerate(net.layers):
            if i in keep:
                a = layer.attn
                y = layer.layer_norm1(x)
                if layer.window_size > 0:
                    y, _ = layer.window_partition(y, layer.window_size)
                Bp, hh, ww, _ = y.shape
                q = a.qkv(y).reshape(Bp, hh * ww, 3, a.num_attention_heads, -1).permute(2, 0, 3, 1, 4).reshape(3, Bp * a.num_attention_heads, hh * ww, -1)[0]
                Rh, Rw = a.get_rel_pos(hh, hh, a.rel_pos_h), a.get_rel_pos(ww, ww, a.rel_pos_w)
                rq = q.reshape(Bp * a.num_attention_heads, hh, ww, -1)
                kept[i] = (torch.einsum("bhwc,hkc->bhwk", rq, Rh)[:a.num_attention_heads], torch.einsum("bhwc,wkc->bhwk", rq, Rw)[:a.num_attention_heads], Rh, Rw)
            out = layer(x)
            x = out[0] if isinstance(out, (tuple, list)) else out
            if i in layers:
                taps.append(x.permute(0, 3, 1, 2).contiguous())
    return taps, kept


def golden(name, cfg, full_taps: bool):
    sd = state_dict(cfg)
    out = {"checksums": checksums(sd)}
    for size in cfg["sizes"]:
        tag = "" if len(cfg["sizes"]) == 1 else f"s{size[0]}_"
        taps, kept = reference_outputs(cfg, sd, size, keep=(0, 1) if full_taps else ())
        if full_taps:
            out["images"] = images(cfg, size).numpy()
        for j, m in enumerate(taps):
            m = m.float().numpy()
            if full_taps:
                out[f"{tag}tap{j}"] = m
            else:
                out[f"{tag}tap{j}"] = m.reshape(-1)[sample_index(m.size)]
                out[f"{tag}tap{j}_shape"] = np.array(m.shape)
        for i, (rel_h, rel_w, Rh, Rw) in kept.items():
            out[f"rel_h_block{i}"], out[f"rel_w_block{i}"] = rel_h.numpy(), rel_w.numpy()  # fp64 [H, h, w, k] of the first window / image
            # the module's tables are fp64 copies of fp32 weights: Rh / Rw in fp32 come from its own get_rel_pos run on the fp32 tables
            out[f"Rh_block{i}"] = _fp32_rel(sd, i, Rh.shape[0], "h").numpy()
            out[f"Rw_block{i}"] = _fp32_rel(sd, i, Rw.shape[0], "w").numpy()
            np.testing.assert_allclose(out[f"Rh_block{i}"], Rh.numpy(), rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(out[f"Rw_block{i}"], Rw.numpy(), rtol=1e-5, atol=1e-6)
    save_golden(name, out)


def _fp32_rel(sd, i, size, axis):
    """transformers' own get_rel_pos on the fp32 table of block i (the bits a fp32 model forms)."""
    from transformers.models.sam.modeling_sam import SamVisionAttention

    return SamVisionAttention.get_rel_pos(None, size, size, sd[f"blocks.{i}.attn.rel_pos_{axis}"].float())


if __name__ == "__main__":
    torch.manual_seed(0)
    golden("sam_tiny.npz", TINY, True)
    golden("sam_mid.npz", MID, False)
    golden("sam_full_sampled.npz", FULL, False)
    print("wrote tests/golden/sam_tiny.npz, sam_mid.npz, sam_full_sampled.npz")
