"""Goldens of the CLIP and SigLIP feature paths (run on CPU, no download): tests/golden/langimg_tiny.npz, langimg_full_sampled.npz.

The models are transformers' ``CLIPVisionModel`` / ``SiglipVisionModel`` built from configs (no fetch; open_clip and timm, which the
reference's wrappers build on, were not installed where this was written), loaded with the seeded weights of
``mvp.backbone.random_clip_state_dict`` / ``random_siglip_state_dict`` through the converters run backwards (-> engine layout ->
``engine_to_hf_clip`` / ``engine_to_hf_siglip``).  Around the model's own modules the reference's ``forward`` is replayed (clip.py:67-101):
patch convolution, class embedding, then ``resize_pos_embed``, ``center_padding`` and ``tokens_to_output`` imported from the reference's
evals/models/utils.py at generation time, ``pre_layrnorm``, then ``encoder.layers[i]`` one by one, taps after blocks n/4-1, n/2-1, 3n/4-1,
n-1, add_norm=False.  transformers' own ``interpolate_pos_encoding`` is NOT used (a different rule).  SigLIP (siglip.py:58-93) the same
without class embedding and ``ln_pre``: timm's ``resample_abs_pos_embed(num_prefix_tokens=0)`` is the reference's ``resize_pos_embed(has_cls_token=False)``
(bicubic, antialiased) up to its same-size test, for which the count rule is used (the issue's definition of 'resize_aa').

Tiny fixtures stored in full (fp32): C = 128, 2 heads, depth 4, B = 2 images of a ragged size (100 x 130): CLIP patch 16 / QuickGELU
(table 4 x 4), CLIP patch 14 / erf GELU (table 5 x 5), SigLIP patch 16 / tanh-GELU (table 4 x 4); every tap, ``dense`` and (CLIP)
``dense-cls``; plus weight checksums.  Full size, 4096 sampled elements per tap and each tap's shape: CLIP B/16 at 224^2 and 480 x 640,
CLIP L/14-336 at 224^2, SigLIP B/16 (384 table) at 224^2, SigLIP L/16 at 256^2."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "midvision-probe_amd"))
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

from make_goldens import save_golden  # noqa: E402
from make_goldens_dinov2 import _reference_utils, sample_index  # noqa: E402,F401
from mvp import backbone as bb  # noqa: E402

# name -> (family, patch, pos-table image size, activation, seed)
TINY = {"clip_p16_quick": ("clip", 16, 64, "quick_gelu", 21), "clip_p14_gelu": ("clip", 14, 70, "gelu", 22), "siglip_p16_tanh": ("siglip", 16, 64, "gelu_tanh", 23)}
TINY_DIMS = dict(C=128, depth=4, size=(100, 130), B=2)
EPS = {"clip": 1e-5, "siglip": 1e-6}
HF_ACT = {"quick_gelu": "quick_gelu", "gelu": "gelu", "gelu_tanh": "gelu_pytorch_tanh"}


def tiny_images() -> torch.Tensor:
    return torch.randn(TINY_DIMS["B"], 3, *TINY_DIMS["size"], generator=torch.Generator().manual_seed(6))


def tiny_state_dict(name: str):
    """The engine-layout weights of a tiny fixture."""
    fam, patch, img, _, seed = TINY[name]
    if fam == "clip":
        return bb.clip_to_engine(bb.random_clip_state_dict(TINY_DIMS["C"], TINY_DIMS["depth"], patch, img, seed=seed))
    return bb.siglip_to_engine(bb.random_siglip_state_dict(TINY_DIMS["C"], TINY_DIMS["depth"], patch, img, seed=seed))


def checksums(sd) -> np.ndarray:
    last = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks.")) - 1
    keys = ["pos_embed", "patch_embed.proj.weight", "blocks.0.attn.qkv.weight", f"blocks.{last}.mlp.fc2.weight", "blocks.1.norm2.bias"]
    keys += ["norm_pre.weight"] if "norm_pre.weight" in sd else ["patch_embed.proj.bias"]
    return np.array([float(sd[k].double().abs().sum()) for k in keys])


def hf_model(sd, fam: str, patch: int, act: str):
    from transformers import CLIPVisionConfig, CLIPVisionModel, SiglipVisionConfig, SiglipVisionModel

    C = sd["pos_embed"].shape[-1]
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    n = sd["pos_embed"].shape[1] - (1 if fam == "clip" else 0)
    kw = dict(hidden_size=C, intermediate_size=4 * C, num_hidden_layers=depth, num_attention_heads=C // 64, image_size=int(n ** 0.5) * patch,
              patch_size=patch, hidden_act=HF_ACT[act], layer_norm_eps=EPS[fam], attention_dropout=0.0)
    if fam == "clip":
        model, hf = CLIPVisionModel(CLIPVisionConfig(**kw)), bb.engine_to_hf_clip(sd)
    else:
        model, hf = SiglipVisionModel(SiglipVisionConfig(**kw)), bb.engine_to_hf_siglip(sd)
    if not hasattr(model, "vision_model"):  # (newer transformers: the vision model's keys carry no prefix)
        hf = {k[len("vision_model."):]: v for k, v in hf.items()}
    res = model.load_state_dict(hf, strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    assert all(k.split("vision_model.")[-1].split(".")[0] in ("post_layernorm", "head") or k.endswith("position_ids") for k in res.missing_keys), res.missing_keys
    return model.double().eval()


def reference_features(sd, fam: str, patch: int, act: str, images: torch.Tensor, outputs=("dense",)):
    """clip.py:67-101 / siglip.py:58-93 around the transformers model's own modules: {output: [one map per tap]}."""
    ut = _reference_utils()
    model = hf_model(sd, fam, patch, act)
    vm = getattr(model, "vision_model", model)
    images = ut.center_padding(images.double(), patch)
    out_hw = (images.shape[-2] // patch, images.shape[-1] // patch)
    depth = len(vm.encoder.layers)
    layers = [depth // 4 - 1, depth // 2 - 1, depth // 4 * 3 - 1, depth - 1]
    with torch.no_grad():
        x = vm.embeddings.patch_embedding(images)
        x_hw = tuple(x.shape[-2:])
        x = x.flatten(2).transpose(1, 2)
        if fam == "clip":
            x = torch.cat([vm.embeddings.class_embedding.expand(x.shape[0], 1, -1).to(x.dtype), x], dim=1)
            x = vm.pre_layrnorm(x + ut.resize_pos_embed(vm.embeddings.position_embedding.weight, x_hw).to(x.dtype))
        else:
            x = x + ut.resize_pos_embed(vm.embeddings.position_embedding.weight, x_hw, has_cls_token=False).to(x.dtype)
        embeds = []
        for i, blk in enumerate(vm.encoder.layers):
            x = blk(x, attention_mask=None)
            x = x[0] if isinstance(x, tuple) else x
            if i in layers:
                embeds.append(x)
        res = {}
        for o in outputs:
            if fam == "clip":
                res[o] = [ut.tokens_to_output(o, e[:, 1:], e[:, 0], out_hw) for e in embeds]
            else:
                res[o] = [ut.tokens_to_output(o, e, None, out_hw) for e in embeds]
    return res


# Full-size models: name -> (family, arch / checkpoint name, activation, seed, [(B, H, W), ...])
FULL = {"clip_b16": ("clip", "ViT-B-16", "quick_gelu", 31, [(2, 224, 224), (1, 480, 640)]),
        "clip_l14_336": ("clip", "ViT-L-14-336", "quick_gelu", 32, [(1, 224, 224)]),
        "siglip_b16_384": ("siglip", "vit_base_patch16_siglip_384", "gelu_tanh", 33, [(2, 224, 224)]),
        "siglip_l16_256": ("siglip", "vit_large_patch16_siglip_256", "gelu_tanh", 34, [(1, 256, 256)])}


def full_state_dict(key: str):
    fam, arch, _, seed, _ = FULL[key]
    if fam == "clip":
        C, depth, patch, img = bb.CLIP_ARCH[arch]
        return bb.clip_to_engine(bb.random_clip_state_dict(C, depth, patch, img, seed=seed)), patch
    C, depth, patch, img = bb.SIGLIP_ARCH[arch]
    return bb.siglip_to_engine(bb.random_siglip_state_dict(C, depth, patch, img, seed=seed)), patch


def full_images(B: int, H: int, W: int) -> torch.Tensor:
    return torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(B * 1000 + H + W + 7))


def golden_tiny():
    out = {"images": tiny_images().numpy()}
    for name, (fam, patch, _, act, _) in TINY.items():
        sd = tiny_state_dict(name)
        out[f"{name}_checksums"] = checksums(sd)
        res = reference_features(sd, fam, patch, act, tiny_images(), outputs=("dense", "dense-cls") if fam == "clip" else ("dense",))
        for o, maps in res.items():
            for j, m in enumerate(maps):
                out[f"{name}_{o}_tap{j}"] = m.float().numpy()
    save_golden("langimg_tiny.npz", out)


def golden_full():
    out = {}
    for key, (fam, _, act, _, shapes) in FULL.items():
        sd, patch = full_state_dict(key)
        out[f"{key}_checksums"] = checksums(sd)
        for (B, H, W) in shapes:
            for j, o in enumerate(reference_features(sd, fam, patch, act, full_images(B, H, W))["dense"]):
                o = o.float().numpy()
                out[f"{key}_{B}x{H}x{W}_tap{j}"] = o.reshape(-1)[sample_index(o.size)]
                out[f"{key}_{B}x{H}x{W}_tap{j}_shape"] = np.array(o.shape)
    save_golden("langimg_full_sampled.npz", out)


if __name__ == "__main__":
    torch.manual_seed(0)
    golden_tiny()
    golden_full()
    print("wrote tests/golden/langimg_tiny.npz, tests/golden/langimg_full_sampled.npz")
