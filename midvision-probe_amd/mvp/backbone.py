"""Shared machinery of the evals.models.* ViT wrappers: parameter containers with the
reference's state-dict key layout, checkpoint discovery (local files only — there is no
network), lazy construction of the HIP engine, and the tap / tokens_to_output glue.
"""
from __future__ import annotations

import math
import os
import warnings
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from . import lib, pipeline
from .vit import RangeAudit, TapGroups, TapOutputs, ViTEngine, parse_precision, tripped_sites


def default_precision() -> str:
    """MVP_PRECISION when set, else 'f16x2': the ViT blocks' GEMMs as two fp16 products over compensated fp16 pairs
    (include/mvp_hip.h, MVP_PREC_F16X2) — the feature error of 'bf16x3' (1.5e-5 ... 2.3e-5 on the reference's ViT-B/16 goldens, contract
    1e-3) at 2/3 of its matrix work; activations must stay within fp16's range (|LayerNorm output|, |attention output|, |GELU(fc1)| <= 65504).
    'bf16x3' (three bf16 products, fp32's exponent range) is what the ResNet trunk and the probes run either way; 'bf16' (one product)
    fails the 1e-3 feature contract."""
    return os.environ.get("MVP_PRECISION", "f16x2")


RANGE_GUARD_MODES = ("off", "auto", "warn", "raise", "fallback")


def range_guard_action(env: Optional[str], range_guard: Optional[str], from_file: bool, world: int) -> str:
    """What the f16x2 range guard of a ViT wrapper does — 'off', 'warn', 'raise' or 'fallback' — from MVP_F16_GUARD (``env``; None =
    unset = 'auto'), the wrapper's ``range_guard=`` keyword (None: the environment decides), whether its weights were read from a
    checkpoint file (``find_checkpoint`` hit) and the number of ranks.  'auto' arms the guard for weights from a file only — never for
    seeded random init or a ``weights=`` state dict — as 'fallback' on one rank and as 'raise' on several, so that ranks never
    silently run different arithmetic (no collective is spent on agreeing).  'warn' / 'raise' / 'fallback' arm it whatever the source."""
    mode = (range_guard if range_guard is not None else (env or "auto")).strip().lower()
    if mode not in RANGE_GUARD_MODES:
        raise ValueError(f"range guard {mode!r}: one of {', '.join(RANGE_GUARD_MODES)} (range_guard= / MVP_F16_GUARD)")
    if mode != "auto":
        return mode
    if not from_file:
        return "off"
    return "fallback" if world <= 1 else "raise"


def checkpoint_dir() -> str:
    return os.environ.get("MVP_CKPT_DIR", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "checkpoints"))


def find_checkpoint(*names: str) -> Optional[str]:
    for n in names:
        for ext in ("", ".pth", ".pth.tar", ".pt", ".safetensors"):
            p = os.path.join(checkpoint_dir(), n + ext)
            if os.path.isfile(p):
                return p
    return None


def load_checkpoint_file(path: str) -> Dict[str, torch.Tensor]:
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file

        return load_file(path)
    obj = torch.load(path, map_location="cpu", weights_only=True)
    for key in ("state_dict", "model", "teacher"):
        if isinstance(obj, dict) and key in obj and isinstance(obj[key], dict):
            obj = obj[key]
    return obj


def random_vit_state_dict(embed_dim=768, depth=12, mlp_ratio=4.0, patch=16, img=224, seed=0, in_chans=3) -> Dict[str, torch.Tensor]:
    """Seeded random init with the reference's statistics (trunc-normal 0.02 linears, zero
    biases, unit LayerNorm: ibot_transformers.py:293-309).  Used when no local checkpoint
    exists (BASELINE configs are random-init / synthetic by construction)."""
    g = torch.Generator().manual_seed(seed)

    def tn(*shape):
        t = torch.empty(*shape)
        torch.nn.init.trunc_normal_(t, std=0.02, a=-2.0, b=2.0, generator=g)
        return t

    hid = int(embed_dim * mlp_ratio)
    sd = {"cls_token": tn(1, 1, embed_dim), "pos_embed": tn(1, (img // patch) ** 2 + 1, embed_dim)}
    bound = 1.0 / math.sqrt(in_chans * patch * patch)
    sd["patch_embed.proj.weight"] = (torch.rand(embed_dim, in_chans, patch, patch, generator=g) * 2 - 1) * bound
    sd["patch_embed.proj.bias"] = (torch.rand(embed_dim, generator=g) * 2 - 1) * bound
    for i in range(depth):
        p = f"blocks.{i}."
        for n in ("norm1", "norm2"):
            sd[p + n + ".weight"], sd[p + n + ".bias"] = torch.ones(embed_dim), torch.zeros(embed_dim)
        sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"] = tn(3 * embed_dim, embed_dim), torch.zeros(3 * embed_dim)
        sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"] = tn(embed_dim, embed_dim), torch.zeros(embed_dim)
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = tn(hid, embed_dim), torch.zeros(hid)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = tn(embed_dim, hid), torch.zeros(embed_dim)
    sd["norm.weight"], sd["norm.bias"] = torch.ones(embed_dim), torch.zeros(embed_dim)
    return sd


DINOV2_ARCH = {  # model_name -> (embed_dim, depth, register tokens); heads = embed_dim / 64, patch 14, MLP ratio 4, pos-embed 37 x 37 (518 / 14)
    "vitb14": (768, 12, 0),
    "vitb14_reg": (768, 12, 4),
    "vitl14": (1024, 24, 0),
    "vitg14": (1536, 40, 0),
}
DINOV2_FFN = {"vitg14": "swiglu"}  # model_name -> the MLP of its blocks where it is not fc1 / GELU / fc2 ("mlp"): SwiGLUFFNFused, w3(silu(x1) * x2)
DINOV2_HUB_NAMES = {"vitb14": "dinov2_vitb14_pretrain", "vitb14_reg": "dinov2_vitb14_reg4_pretrain", "vitl14": "dinov2_vitl14_pretrain",
                    "vitg14": "dinov2_vitg14_pretrain"}


def swiglu_hidden(embed_dim: int, mlp_ratio: float = 4.0) -> int:
    """Hidden width H of DINOv2's SwiGLUFFNFused: (int(hidden_features * 2 / 3) + 7) // 8 * 8 with hidden_features = int(C * mlp_ratio);
    344 at C = 128, 512 at 192, 4096 at 1536."""
    return (int(int(embed_dim * mlp_ratio) * 2 / 3) + 7) // 8 * 8


def random_dinov2_state_dict(embed_dim=768, depth=12, registers=0, patch=14, pos_grid=37, seed=0, in_chans=3, ffn="mlp") -> Dict[str, torch.Tensor]:
    """Seeded random DINOv2 weights in the torch.hub key layout (used when no local checkpoint exists): the ViT statistics of
    random_vit_state_dict, a pos_grid x pos_grid pos-embed (518 / 14 = 37), random register tokens, LayerScale gammas drawn log-uniform
    over [1e-6, 1] (trained DINOv2 models keep gammas from ~1e-5 to ~1), plus mask_token and the final norm (loaded, unused here).
    ``ffn``: 'mlp' (fc1 / fc2, hidden 4C) or 'swiglu' (ViT-g/14: ``mlp.w12`` [2H, C] and ``mlp.w3`` [C, H], H = swiglu_hidden(C))."""
    if ffn not in ("mlp", "swiglu"):
        raise ValueError(f"ffn {ffn!r}: 'mlp' or 'swiglu'")
    g = torch.Generator().manual_seed(seed)

    def tn(*shape, std=0.02):
        t = torch.empty(*shape)
        torch.nn.init.trunc_normal_(t, std=std, a=-2.0 * std / 0.02, b=2.0 * std / 0.02, generator=g)
        return t

    def gamma():
        return torch.exp(torch.empty(embed_dim).uniform_(math.log(1e-6), 0.0, generator=g))

    hid = 4 * embed_dim
    sd = {"cls_token": tn(1, 1, embed_dim), "pos_embed": tn(1, pos_grid * pos_grid + 1, embed_dim), "mask_token": torch.zeros(1, embed_dim)}
    if registers:
        sd["register_tokens"] = tn(1, registers, embed_dim, std=0.5)
    bound = 1.0 / math.sqrt(in_chans * patch * patch)
    sd["patch_embed.proj.weight"] = (torch.rand(embed_dim, in_chans, patch, patch, generator=g) * 2 - 1) * bound
    sd["patch_embed.proj.bias"] = (torch.rand(embed_dim, generator=g) * 2 - 1) * bound
    for i in range(depth):
        p = f"blocks.{i}."
        for n in ("norm1", "norm2"):
            sd[p + n + ".weight"] = 1.0 + 0.1 * torch.randn(embed_dim, generator=g)
            sd[p + n + ".bias"] = 0.02 * torch.randn(embed_dim, generator=g)
        sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"] = tn(3 * embed_dim, embed_dim), tn(3 * embed_dim)
        sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"] = tn(embed_dim, embed_dim), tn(embed_dim)
        sd[p + "ls1.gamma"] = gamma()
        if ffn == "swiglu":
            glu = swiglu_hidden(embed_dim)
            sd[p + "mlp.w12.weight"], sd[p + "mlp.w12.bias"] = tn(2 * glu, embed_dim), tn(2 * glu)
            sd[p + "mlp.w3.weight"], sd[p + "mlp.w3.bias"] = tn(embed_dim, glu), tn(embed_dim)
        else:
            sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = tn(hid, embed_dim), tn(hid)
            sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = tn(embed_dim, hid), tn(embed_dim)
        sd[p + "ls2.gamma"] = gamma()
    sd["norm.weight"], sd["norm.bias"] = torch.ones(embed_dim), torch.zeros(embed_dim)
    return sd


def dinov2_hub_to_engine(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """A DINOv2 torch.hub state dict -> the keys the engine reads: chunked blocks (``blocks.<chunk>.<i>.``, block_chunks > 0) are
    flattened to ``blocks.<i>.``; ``mask_token`` (masked pre-training only) and the final ``norm.*`` (not on the tap path,
    dino.py:176-207) are dropped.  Every other key passes through under its own name, ViT-g/14's ``mlp.w12.*`` / ``mlp.w3.*`` included."""
    out = {}
    for k, v in sd.items():
        if k == "mask_token" or k.startswith("norm."):
            continue
        parts = k.split(".")
        if parts[0] == "blocks" and len(parts) > 3 and parts[1].isdigit() and parts[2].isdigit():
            k = ".".join(["blocks"] + parts[2:])
        out[k] = v
    return out


def hf_vitmae_to_fused(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """HF ViTMAEModel keys (embeddings.*, encoder.layer.i.attention.attention.{query,key,value},
    layernorm_before/after, intermediate.dense, output.dense) -> the fused DINO-style layout."""
    out = {}
    pre = "vit." if any(k.startswith("vit.") for k in sd) else ""
    g = lambda k: sd[pre + k]  # noqa: E731
    out["cls_token"] = g("embeddings.cls_token")
    out["pos_embed"] = g("embeddings.position_embeddings")
    out["patch_embed.proj.weight"] = g("embeddings.patch_embeddings.projection.weight")
    out["patch_embed.proj.bias"] = g("embeddings.patch_embeddings.projection.bias")
    i = 0
    while pre + f"encoder.layer.{i}.layernorm_before.weight" in sd:
        s, d = f"encoder.layer.{i}.", f"blocks.{i}."
        out[d + "norm1.weight"], out[d + "norm1.bias"] = g(s + "layernorm_before.weight"), g(s + "layernorm_before.bias")
        out[d + "norm2.weight"], out[d + "norm2.bias"] = g(s + "layernorm_after.weight"), g(s + "layernorm_after.bias")
        out[d + "attn.qkv.weight"] = torch.cat([g(s + f"attention.attention.{n}.weight") for n in ("query", "key", "value")], 0)
        out[d + "attn.qkv.bias"] = torch.cat([g(s + f"attention.attention.{n}.bias") for n in ("query", "key", "value")], 0)
        out[d + "attn.proj.weight"], out[d + "attn.proj.bias"] = g(s + "attention.output.dense.weight"), g(s + "attention.output.dense.bias")
        out[d + "mlp.fc1.weight"], out[d + "mlp.fc1.bias"] = g(s + "intermediate.dense.weight"), g(s + "intermediate.dense.bias")
        out[d + "mlp.fc2.weight"], out[d + "mlp.fc2.bias"] = g(s + "output.dense.weight"), g(s + "output.dense.bias")
        i += 1
    if pre + "layernorm.weight" in sd:
        out["norm.weight"], out["norm.bias"] = g("layernorm.weight"), g("layernorm.bias")
    return out


# ---------------------------------------------------------------- CLIP / SigLIP (language-supervised ViTs): architectures, random init, key layouts
CLIP_ARCH = {  # open_clip arch -> (embed_dim, depth, patch, image size); heads = embed_dim / 64, MLP ratio 4
    "ViT-B-16": (768, 12, 16, 224),
    "ViT-L-14": (1024, 24, 14, 224),
    "ViT-L-14-336": (1024, 24, 14, 336),
}
SIGLIP_ARCH = {  # timm model name -> (embed_dim, depth, patch, image size)
    "vit_base_patch16_siglip_224": (768, 12, 16, 224),
    "vit_base_patch16_siglip_384": (768, 12, 16, 384),
    "vit_large_patch16_siglip_256": (1024, 24, 16, 256),
    "vit_large_patch16_siglip_384": (1024, 24, 16, 384),
}


def _random_blocks(sd, prefix, names, embed_dim, depth, g):
    """Blocks with non-trivial LayerNorm affines and biases (as random_dinov2_state_dict), under the given key names."""
    def tn(*shape):
        t = torch.empty(*shape)
        torch.nn.init.trunc_normal_(t, std=0.02, a=-2.0, b=2.0, generator=g)
        return t

    hid = 4 * embed_dim
    for i in range(depth):
        p = f"{prefix}{i}."
        for n in (names["norm1"], names["norm2"]):
            sd[p + n + ".weight"] = 1.0 + 0.1 * torch.randn(embed_dim, generator=g)
            sd[p + n + ".bias"] = 0.02 * torch.randn(embed_dim, generator=g)
        sd[p + names["qkv_w"]], sd[p + names["qkv_b"]] = tn(3 * embed_dim, embed_dim), tn(3 * embed_dim)
        sd[p + names["proj"] + ".weight"], sd[p + names["proj"] + ".bias"] = tn(embed_dim, embed_dim), tn(embed_dim)
        sd[p + names["fc1"] + ".weight"], sd[p + names["fc1"] + ".bias"] = tn(hid, embed_dim), tn(hid)
        sd[p + names["fc2"] + ".weight"], sd[p + names["fc2"] + ".bias"] = tn(embed_dim, hid), tn(embed_dim)


_OPENCLIP_BLOCK = dict(norm1="ln_1", norm2="ln_2", qkv_w="attn.in_proj_weight", qkv_b="attn.in_proj_bias", proj="attn.out_proj", fc1="mlp.c_fc", fc2="mlp.c_proj")
_TIMM_BLOCK = dict(norm1="norm1", norm2="norm2", qkv_w="attn.qkv.weight", qkv_b="attn.qkv.bias", proj="attn.proj", fc1="mlp.fc1", fc2="mlp.fc2")


def random_clip_state_dict(embed_dim=768, depth=12, patch=16, img=224, seed=0, in_chans=3, out_dim=512) -> Dict[str, torch.Tensor]:
    """Seeded random CLIP image tower in open_clip's ``visual.*`` key layout (used when no local checkpoint exists): class embedding and
    position table at open_clip's scale (width ** -0.5), a bias-free patch convolution, ``ln_pre`` with gains spread around 1 and
    non-zero biases (so that it really acts), blocks with non-trivial LayerNorm affines and biases, plus ``ln_post`` and ``proj`` (loaded, unused here)."""
    g = torch.Generator().manual_seed(seed)
    scale = embed_dim ** -0.5
    sd = {"visual.class_embedding": scale * torch.randn(embed_dim, generator=g),
          "visual.positional_embedding": scale * torch.randn((img // patch) ** 2 + 1, embed_dim, generator=g)}
    bound = 1.0 / math.sqrt(in_chans * patch * patch)
    sd["visual.conv1.weight"] = (torch.rand(embed_dim, in_chans, patch, patch, generator=g) * 2 - 1) * bound
    sd["visual.ln_pre.weight"] = 1.0 + 0.25 * torch.randn(embed_dim, generator=g)
    sd["visual.ln_pre.bias"] = 0.05 * torch.randn(embed_dim, generator=g)
    _random_blocks(sd, "visual.transformer.resblocks.", _OPENCLIP_BLOCK, embed_dim, depth, g)
    sd["visual.ln_post.weight"], sd["visual.ln_post.bias"] = torch.ones(embed_dim), torch.zeros(embed_dim)
    sd["visual.proj"] = scale * torch.randn(embed_dim, out_dim, generator=g)
    return sd


def random_siglip_state_dict(embed_dim=768, depth=12, patch=16, img=224, seed=0, in_chans=3) -> Dict[str, torch.Tensor]:
    """Seeded random SigLIP image tower in timm's key layout: no class token, a position table of (img / patch) ** 2 entries, a patch
    convolution with bias, blocks with non-trivial LayerNorm affines and biases, plus the final ``norm`` and two ``attn_pool`` tensors
    (loaded, unused here)."""
    g = torch.Generator().manual_seed(seed)
    sd = {"pos_embed": 0.02 * torch.randn(1, (img // patch) ** 2, embed_dim, generator=g)}
    bound = 1.0 / math.sqrt(in_chans * patch * patch)
    sd["patch_embed.proj.weight"] = (torch.rand(embed_dim, in_chans, patch, patch, generator=g) * 2 - 1) * bound
    sd["patch_embed.proj.bias"] = (torch.rand(embed_dim, generator=g) * 2 - 1) * bound
    _random_blocks(sd, "blocks.", _TIMM_BLOCK, embed_dim, depth, g)
    sd["norm.weight"], sd["norm.bias"] = torch.ones(embed_dim), torch.zeros(embed_dim)
    sd["attn_pool.latent"] = 0.02 * torch.randn(1, 1, embed_dim, generator=g)
    sd["attn_pool.norm.weight"] = torch.ones(embed_dim)
    return sd


def _rename_blocks(out, sd, src_prefix, src_names, dst_prefix, dst_names):
    i = 0
    while f"{src_prefix}{i}.{src_names['norm1']}.weight" in sd:
        s, d = f"{src_prefix}{i}.", f"{dst_prefix}{i}."
        for n in ("norm1", "norm2", "proj", "fc1", "fc2"):
            for t in (".weight", ".bias"):
                out[d + dst_names[n] + t] = sd[s + src_names[n] + t]
        out[d + dst_names["qkv_w"]], out[d + dst_names["qkv_b"]] = sd[s + src_names["qkv_w"]], sd[s + src_names["qkv_b"]]
        i += 1
    return i


def openclip_to_engine(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """open_clip's CLIP state dict (``visual.*``; the bare image tower without the prefix too) -> the keys the engine reads.  ``ln_post``
    and ``proj`` (the projection head, not on the tap path: clip.py:67-101) and everything outside the image tower are dropped."""
    pre = "visual." if any(k.startswith("visual.") for k in sd) else ""
    v = {k[len(pre):]: t for k, t in sd.items() if k.startswith(pre)}
    out = {"cls_token": v["class_embedding"].reshape(1, 1, -1), "pos_embed": v["positional_embedding"].unsqueeze(0),
           "patch_embed.proj.weight": v["conv1.weight"], "norm_pre.weight": v["ln_pre.weight"], "norm_pre.bias": v["ln_pre.bias"]}
    _rename_blocks(out, v, "transformer.resblocks.", _OPENCLIP_BLOCK, "blocks.", _TIMM_BLOCK)
    return out


def engine_to_openclip(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The inverse of openclip_to_engine (``visual.*`` keys; no ``ln_post`` / ``proj``)."""
    out = {"class_embedding": sd["cls_token"].reshape(-1), "positional_embedding": sd["pos_embed"][0], "conv1.weight": sd["patch_embed.proj.weight"],
           "ln_pre.weight": sd["norm_pre.weight"], "ln_pre.bias": sd["norm_pre.bias"]}
    _rename_blocks(out, sd, "blocks.", _TIMM_BLOCK, "transformer.resblocks.", _OPENCLIP_BLOCK)
    return {"visual." + k: v for k, v in out.items()}


def _hf_layers_to_engine(out, g, has):
    i = 0
    while has(f"encoder.layers.{i}.layer_norm1.weight"):
        s, d = f"encoder.layers.{i}.", f"blocks.{i}."
        for a, b in (("layer_norm1", "norm1"), ("layer_norm2", "norm2"), ("self_attn.out_proj", "attn.proj"), ("mlp.fc1", "mlp.fc1"), ("mlp.fc2", "mlp.fc2")):
            out[d + b + ".weight"], out[d + b + ".bias"] = g(s + a + ".weight"), g(s + a + ".bias")
        out[d + "attn.qkv.weight"] = torch.cat([g(s + f"self_attn.{n}_proj.weight") for n in "qkv"], 0)
        out[d + "attn.qkv.bias"] = torch.cat([g(s + f"self_attn.{n}_proj.bias") for n in "qkv"], 0)
        i += 1


def _engine_layers_to_hf(out, sd):
    i = 0
    while f"blocks.{i}.norm1.weight" in sd:
        s, d = f"blocks.{i}.", f"vision_model.encoder.layers.{i}."
        for a, b in (("layer_norm1", "norm1"), ("layer_norm2", "norm2"), ("self_attn.out_proj", "attn.proj"), ("mlp.fc1", "mlp.fc1"), ("mlp.fc2", "mlp.fc2")):
            out[d + a + ".weight"], out[d + a + ".bias"] = sd[s + b + ".weight"], sd[s + b + ".bias"]
        for n, w, b in zip("qkv", sd[s + "attn.qkv.weight"].chunk(3, 0), sd[s + "attn.qkv.bias"].chunk(3, 0)):
            out[d + f"self_attn.{n}_proj.weight"], out[d + f"self_attn.{n}_proj.bias"] = w.contiguous(), b.contiguous()
        i += 1


def hf_clip_to_engine(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """transformers' CLIPVisionModel (or CLIPModel) keys -> the engine's; ``post_layernorm``, ``position_ids``, the projection and the text
    tower are dropped."""
    pre = next((p for p in ("vision_model.", "") if p + "embeddings.class_embedding" in sd), None)
    if pre is None:
        raise KeyError("not a transformers CLIP vision state dict (vision_model.embeddings.class_embedding missing)")
    g, has = (lambda k: sd[pre + k]), (lambda k: pre + k in sd)
    out = {"cls_token": g("embeddings.class_embedding").reshape(1, 1, -1), "pos_embed": g("embeddings.position_embedding.weight").unsqueeze(0),
           "patch_embed.proj.weight": g("embeddings.patch_embedding.weight"),
           "norm_pre.weight": g("pre_layrnorm.weight"), "norm_pre.bias": g("pre_layrnorm.bias")}
    _hf_layers_to_engine(out, g, has)
    return out


def engine_to_hf_clip(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The inverse of hf_clip_to_engine (CLIPVisionModel keys; no ``post_layernorm``)."""
    out = {"vision_model.embeddings.class_embedding": sd["cls_token"].reshape(-1), "vision_model.embeddings.position_embedding.weight": sd["pos_embed"][0],
           "vision_model.embeddings.patch_embedding.weight": sd["patch_embed.proj.weight"],
           "vision_model.pre_layrnorm.weight": sd["norm_pre.weight"], "vision_model.pre_layrnorm.bias": sd["norm_pre.bias"]}
    _engine_layers_to_hf(out, sd)
    return out


def hf_siglip_to_engine(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """transformers' SiglipVisionModel (or SiglipModel) keys -> the engine's; ``post_layernorm``, the attention-pool ``head`` and the text
    tower are dropped."""
    pre = next((p for p in ("vision_model.", "") if p + "embeddings.patch_embedding.weight" in sd), None)
    if pre is None:
        raise KeyError("not a transformers SigLIP vision state dict (vision_model.embeddings.patch_embedding.weight missing)")
    g, has = (lambda k: sd[pre + k]), (lambda k: pre + k in sd)
    out = {"pos_embed": g("embeddings.position_embedding.weight").unsqueeze(0),
           "patch_embed.proj.weight": g("embeddings.patch_embedding.weight"), "patch_embed.proj.bias": g("embeddings.patch_embedding.bias")}
    _hf_layers_to_engine(out, g, has)
    return out


def engine_to_hf_siglip(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The inverse of hf_siglip_to_engine (SiglipVisionModel keys; no ``post_layernorm`` / ``head``)."""
    out = {"vision_model.embeddings.position_embedding.weight": sd["pos_embed"][0],
           "vision_model.embeddings.patch_embedding.weight": sd["patch_embed.proj.weight"], "vision_model.embeddings.patch_embedding.bias": sd["patch_embed.proj.bias"]}
    _engine_layers_to_hf(out, sd)
    return out


def timm_siglip_to_engine(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """timm's SigLIP ViT keys are the engine's own; the attention pool (``attn_pool.*``) and the final ``norm.*`` — neither on the tap path
    (siglip.py:58-93) — are dropped."""
    return {k: v for k, v in sd.items() if not (k.startswith("attn_pool.") or k.startswith("norm."))}


def clip_to_engine(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Any of the CLIP layouts (open_clip, transformers, or already the engine's)."""
    if any(k.endswith("embeddings.class_embedding") for k in sd):
        return hf_clip_to_engine(sd)
    if "visual.conv1.weight" in sd or "conv1.weight" in sd:
        return openclip_to_engine(sd)
    return dict(sd)


def siglip_to_engine(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Any of the SigLIP layouts (timm, transformers)."""
    if any(k.endswith("embeddings.patch_embedding.weight") for k in sd):
        return hf_siglip_to_engine(sd)
    return timm_siglip_to_engine(sd)


# ---------------------------------------------------------------- CroCo / CroCo v2 (cross-view completion; plain ViT-B/16 encoders without a class token)
CROCO_CKPT_FILES = {"croco": "CroCo.pth", "crocov2": "CroCo_V2_ViTBase_BaseDecoder.pth"}  # the published files, looked for under MVP_CKPT_DIR
_CROCO_DROPPED = ("enc_norm.", "mask_token", "decoder_embed.", "dec_", "prediction_head.")  # never on the tap path (croco.py:150-178)


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def croco_model_dict(sd: Dict) -> Dict[str, torch.Tensor]:
    """The model's tensors out of the published layout ``{"model": ..., "croco_kwargs": ...}``, or the bare dict itself."""
    return sd["model"] if isinstance(sd.get("model"), dict) else sd


def croco_to_engine(sd: Dict) -> Dict[str, torch.Tensor]:
    """A CroCo / CroCo v2 checkpoint (the published ``{"model": ..., "croco_kwargs": ...}``, or the bare model dict; a dict already in
    the engine's layout passes through) -> the keys the engine reads: ``enc_blocks.i.*`` -> ``blocks.i.*``, ``patch_embed.proj.*`` kept,
    ``enc_pos_embed`` [n, C] -> ``pos_embed`` [1, n, C] (CroCo v1: the fixed sin-cos table without a CLS entry; RoPE models have none).
    Dropped: ``enc_norm.*`` (the final norm is never applied on the tap path), ``mask_token``, ``decoder_embed.*``, ``dec_*`` and
    ``prediction_head.*`` (the decoder)."""
    m = croco_model_dict(sd)
    if not any(k.startswith("enc_blocks.") for k in m):
        return dict(m)
    out = {}
    for k, v in m.items():
        if k.startswith(_CROCO_DROPPED):
            continue
        if k.startswith("enc_blocks."):
            out["blocks." + k[len("enc_blocks."):]] = v
        elif k == "enc_pos_embed":
            out["pos_embed"] = v.unsqueeze(0)
        elif k.startswith("patch_embed.proj."):
            out[k] = v
        else:
            raise KeyError(f"croco_to_engine: unexpected key {k!r}")
    return out


def engine_to_croco(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The inverse of croco_to_engine on the encoder's keys (no ``enc_norm`` / decoder)."""
    out = {}
    for k, v in sd.items():
        if k.startswith("blocks."):
            out["enc_blocks." + k[len("blocks."):]] = v
        elif k == "pos_embed":
            out["enc_pos_embed"] = v[0]
        else:
            out[k] = v
    return out


def random_croco_state_dict(embed_dim=768, depth=12, patch=16, img=224, pos_embed="cosine", seed=0, in_chans=3, dec_dim=None) -> Dict:
    """Seeded random CroCo weights in the published layout ``{"model": ..., "croco_kwargs": ...}`` (used when no local checkpoint exists).
    ``img``: the model's image size, an int or (height, width); ``pos_embed``: 'cosine' (CroCo v1: ``enc_pos_embed`` is the sin-cos table
    of ``get_2d_sincos_pos_embed(C, grid, 0)``, croco_models/pos_embed.py:22-69) or 'RoPE<freq>' (CroCo v2: no table).  Blocks with
    non-trivial LayerNorm affines and biases and Q / K projections large enough for peaked attention (with trunc-normal 0.02 weights the
    softmax is near uniform and a wrong position form moves the features by less than the 1e-3 feature contract), plus ``enc_norm``, ``mask_token`` and a few decoder tensors (loaded, unused here)."""
    g = torch.Generator().manual_seed(seed)
    ih, iw = _pair(img)
    grid = (ih // patch, iw // patch)
    dec = dec_dim or (512 if embed_dim == 768 else embed_dim // 2)
    kw = dict(img_size=(ih, iw) if ih != iw else ih, patch_size=patch, enc_embed_dim=embed_dim, enc_depth=depth, enc_num_heads=embed_dim // 64,
              dec_embed_dim=dec, dec_depth=1, dec_num_heads=max(1, dec // 64), pos_embed=pos_embed)
    m = {}
    bound = math.sqrt(6.0 / (in_chans * patch * patch + embed_dim))  # (xavier-uniform on the flattened patch weight, as MAE / CroCo)
    m["patch_embed.proj.weight"] = (torch.rand(embed_dim, in_chans, patch, patch, generator=g) * 2 - 1) * bound
    m["patch_embed.proj.bias"] = 0.02 * torch.randn(embed_dim, generator=g)
    if pos_embed == "cosine":
        m["enc_pos_embed"] = torch.from_numpy(sincos_pos_embed_2d(embed_dim, grid, add_cls_token=False)).float()
        m["dec_pos_embed"] = torch.from_numpy(sincos_pos_embed_2d(dec, grid, add_cls_token=False)).float()
    elif not pos_embed.startswith("RoPE"):
        raise NotImplementedError("Unknown pos_embed " + pos_embed)
    _random_blocks(m, "enc_blocks.", _TIMM_BLOCK, embed_dim, depth, g)
    for i in range(depth):  # Q and K rows at std 1.5 / sqrt(C): logits of a few units, attention peaked enough for the positions to matter
        m[f"enc_blocks.{i}.attn.qkv.weight"][:2 * embed_dim] *= 1.5 / (0.02 * math.sqrt(embed_dim))
    m["enc_norm.weight"], m["enc_norm.bias"] = torch.ones(embed_dim), torch.zeros(embed_dim)
    m["mask_token"] = torch.zeros(1, 1, dec)
    m["decoder_embed.weight"], m["decoder_embed.bias"] = 0.02 * torch.randn(dec, embed_dim, generator=g), torch.zeros(dec)
    m["dec_norm.weight"], m["dec_norm.bias"] = torch.ones(dec), torch.zeros(dec)
    m["prediction_head.weight"], m["prediction_head.bias"] = 0.02 * torch.randn(patch * patch * 3, dec, generator=g), torch.zeros(patch * patch * 3)
    return {"model": m, "croco_kwargs": kw}


# ---------------------------------------------------------------- BEiT v2 (ViT-B/16 with a per-block relative-position bias, no absolute position table)
BEIT_CKPT_FILE = "beit_v2_vitb16.pth"  # the published file, looked for under MVP_CKPT_DIR
_BEIT_SHARED_TABLE = "rel_pos_bias.relative_position_bias_table"


def beit_grid(n_rows: int, grid=None):
    """(gh, gw) a relative-position table of ``n_rows`` rows belongs to: ``grid`` when given (checked), else the square grid of that length."""
    if grid is not None:
        gh, gw = _pair(grid)
    else:
        gh = gw = (math.isqrt(max(n_rows - 3, 0)) + 1) // 2
    if (2 * gh - 1) * (2 * gw - 1) + 3 != n_rows:
        raise lib.MvpError(f"relative-position table of {n_rows} rows does not belong to a {gh} x {gw} grid ({(2 * gh - 1) * (2 * gw - 1) + 3} rows): "
                           "re-interpolating tables to another grid (the reference's scipy path) is not supported")
    return gh, gw


def beit_to_engine(sd: Dict) -> Dict[str, torch.Tensor]:
    """A BEiT v2 checkpoint (the published ``{"model": ...}``, or the bare dict; a dict already in the engine's layout passes through) ->
    the keys the engine reads: ``attn.q_bias`` / ``attn.v_bias`` -> ``attn.qkv.bias`` = cat(q_bias, 0, v_bias) (the K bias is zero,
    beit_model.py:152-162); ``gamma_1`` / ``gamma_2`` -> ``ls1.gamma`` / ``ls2.gamma``; ``attn.relative_position_bias_table`` ->
    ``attn.rel_pos_bias_table``, a shared ``rel_pos_bias.relative_position_bias_table`` expanded to every block (beit_state_dict.py:14-28).
    Dropped: every ``relative_position_index`` (recomputed), ``head.*`` and ``mask_token``."""
    m = sd["model"] if isinstance(sd.get("model"), dict) else sd
    if not any(k.endswith(("attn.q_bias", "gamma_1", "relative_position_bias_table")) for k in m):
        return dict(m)
    out = {}
    shared = m.get(_BEIT_SHARED_TABLE)
    for k, v in m.items():
        if "relative_position_index" in k or k.startswith("head.") or k == "mask_token" or k == _BEIT_SHARED_TABLE:
            continue
        if k.endswith("attn.v_bias"):
            continue
        if k.endswith("attn.q_bias"):
            p = k[:-len("q_bias")]
            out[p + "qkv.bias"] = torch.cat((v, torch.zeros_like(v), m[p + "v_bias"]))
        elif k.endswith(".gamma_1") or k.endswith(".gamma_2"):
            out[k[:-len("gamma_1")] + ("ls1.gamma" if k.endswith("1") else "ls2.gamma")] = v
        elif k.endswith("attn.relative_position_bias_table"):
            out[k[:-len("relative_position_bias_table")] + "rel_pos_bias_table"] = v
        else:
            out[k] = v
    if shared is not None:
        depth = 1 + max(int(k.split(".")[1]) for k in out if k.startswith("blocks."))
        for i in range(depth):
            out[f"blocks.{i}.attn.rel_pos_bias_table"] = shared.clone()
    return out


def engine_to_beit(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The inverse of beit_to_engine (per-block tables; no ``relative_position_index``, ``head`` or ``mask_token``).  The K third of
    ``attn.qkv.bias`` must be zero: the layout has no place for it."""
    out = {}
    for k, v in sd.items():
        if k.endswith("attn.qkv.bias"):
            q, kb, vb = v.chunk(3)
            if bool((kb != 0).any()):
                raise ValueError(f"{k}: a non-zero K bias cannot be written in BEiT's q_bias / v_bias layout")
            out[k[:-len("qkv.bias")] + "q_bias"], out[k[:-len("qkv.bias")] + "v_bias"] = q.clone(), vb.clone()
        elif k.endswith(".ls1.gamma") or k.endswith(".ls2.gamma"):
            out[k[:-len("ls1.gamma")] + ("gamma_1" if k.endswith("ls1.gamma") else "gamma_2")] = v
        elif k.endswith("attn.rel_pos_bias_table"):
            out[k[:-len("rel_pos_bias_table")] + "relative_position_bias_table"] = v
        else:
            out[k] = v
    return out


def random_beit_state_dict(embed_dim=768, depth=12, patch=16, img=224, seed=0, in_chans=3) -> Dict[str, torch.Tensor]:
    """Seeded random BEiT v2 weights in the ENGINE's layout (used when no local checkpoint exists; ``engine_to_beit`` gives the published
    one).  ``img``: an int or (height, width).  Blocks as random_dinov2_state_dict's (non-trivial LayerNorm affines and biases) with a zero
    K bias; relative-position tables ~ N(0, 1) per block, LayerScale gammas 0.1 (1 + 0.5 N(0, 1)), non-zero q / v biases — the reference
    initialises tables to zero and gammas to a constant, under which a wrong index or a swapped gamma would not show — and ``fc_norm``
    with gains spread around 1.  No ``pos_embed``."""
    g = torch.Generator().manual_seed(seed)
    ih, iw = _pair(img)
    gh, gw = ih // patch, iw // patch
    heads = embed_dim // 64
    sd = {"cls_token": 0.02 * torch.randn(1, 1, embed_dim, generator=g)}
    bound = 1.0 / math.sqrt(in_chans * patch * patch)
    sd["patch_embed.proj.weight"] = (torch.rand(embed_dim, in_chans, patch, patch, generator=g) * 2 - 1) * bound
    sd["patch_embed.proj.bias"] = (torch.rand(embed_dim, generator=g) * 2 - 1) * bound
    _random_blocks(sd, "blocks.", _TIMM_BLOCK, embed_dim, depth, g)
    for i in range(depth):
        p = f"blocks.{i}."
        sd[p + "attn.qkv.bias"][embed_dim:2 * embed_dim] = 0.0
        sd[p + "attn.rel_pos_bias_table"] = torch.randn((2 * gh - 1) * (2 * gw - 1) + 3, heads, generator=g)
        sd[p + "ls1.gamma"] = 0.1 * (1.0 + 0.5 * torch.randn(embed_dim, generator=g))
        sd[p + "ls2.gamma"] = 0.1 * (1.0 + 0.5 * torch.randn(embed_dim, generator=g))
    sd["fc_norm.weight"] = 1.0 + 0.1 * torch.randn(embed_dim, generator=g)
    sd["fc_norm.bias"] = 0.02 * torch.randn(embed_dim, generator=g)
    return sd


# ---------------------------------------------------------------- SAM image encoders (ViT-B / ViT-L: windowed attention, decomposed relative-position terms)
SAM_ARCH = {"vit_b": (768, 12, 12, (2, 5, 8, 11)), "vit_l": (1024, 24, 16, (5, 11, 17, 23)), "vit_h": (1280, 32, 16, (7, 15, 23, 31))}  # arch -> (C, depth, heads, global blocks); vit_h: head dim 80, refused
SAM_CKPT_FILES = {"vit_b": "sam_vit_b_01ec64.pth", "vit_l": "sam_vit_l_0b3195.pth", "vit_h": "sam_vit_h_4b8939.pth"}  # the published files, looked for under MVP_CKPT_DIR
_SAM_PUB = (("norm1", "norm1"), ("norm2", "norm2"), ("attn.qkv", "attn.qkv"), ("attn.proj", "attn.proj"), ("mlp.lin1", "mlp.fc1"), ("mlp.lin2", "mlp.fc2"))
_SAM_HF = (("layer_norm1", "norm1"), ("layer_norm2", "norm2"), ("attn.qkv", "attn.qkv"), ("attn.proj", "attn.proj"), ("mlp.lin1", "mlp.fc1"), ("mlp.lin2", "mlp.fc2"))


def _sam_blocks(out, g, has, src_blocks, names, dst_blocks, to_engine=True):
    i = 0
    while has(f"{src_blocks}{i}.{(names[0][0] if to_engine else names[0][1])}.weight"):
        sp, dp = f"{src_blocks}{i}.", f"{dst_blocks}{i}."
        for a, b in names:
            a, b = (a, b) if to_engine else (b, a)
            for t in (".weight", ".bias"):
                out[dp + b + t] = g(sp + a + t)
        for t in ("attn.rel_pos_h", "attn.rel_pos_w"):
            out[dp + t] = g(sp + t)
        i += 1
    return i


def sam_to_engine(sd: Dict) -> Dict[str, torch.Tensor]:
    """A SAM checkpoint -> the keys the engine reads.  Accepted: the published ``sam_vit_*.pth`` layout (``image_encoder.`` prefix or the
    bare encoder: ``blocks.i.{norm1, attn.qkv, attn.proj, attn.rel_pos_h, attn.rel_pos_w, norm2, mlp.lin1, mlp.lin2}``, ``patch_embed.proj``,
    ``pos_embed`` [1, S, S, C]), transformers' ``SamVisionEncoder`` layout (``vision_encoder.`` prefix or bare: ``layers.i.{layer_norm1,
    layer_norm2, attn.*, mlp.lin1, mlp.lin2}``, ``patch_embed.projection``), and the engine's own (``mlp.fc1`` / ``mlp.fc2``; passes
    through).  The neck (not used by the reference's forward), the prompt encoder and the mask decoder are ignored."""
    pre = next((p for p in ("image_encoder.", "vision_encoder.", "") if p + "pos_embed" in sd), None)
    if pre is None:
        raise KeyError("not a SAM image-encoder state dict (pos_embed missing)")
    g, has = (lambda k: sd[pre + k]), (lambda k: pre + k in sd)
    out = {"pos_embed": g("pos_embed")}
    if has("patch_embed.projection.weight"):
        out["patch_embed.proj.weight"], out["patch_embed.proj.bias"] = g("patch_embed.projection.weight"), g("patch_embed.projection.bias")
        n = _sam_blocks(out, g, has, "layers.", _SAM_HF, "blocks.")
    else:
        out["patch_embed.proj.weight"], out["patch_embed.proj.bias"] = g("patch_embed.proj.weight"), g("patch_embed.proj.bias")
        names = _SAM_PUB if has("blocks.0.mlp.lin1.weight") else tuple((b, b) for _, b in _SAM_PUB)
        n = _sam_blocks(out, g, has, "blocks.", names, "blocks.")
    if n == 0:
        raise KeyError("not a SAM image-encoder state dict (no blocks)")
    if out["pos_embed"].dim() != 4:
        raise KeyError(f"SAM pos_embed of shape {tuple(out['pos_embed'].shape)}: [1, S, S, C] expected")
    return out


def engine_to_sam_hf(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The inverse of sam_to_engine into transformers' ``SamVisionEncoder`` keys (no neck)."""
    out = {"pos_embed": sd["pos_embed"], "patch_embed.projection.weight": sd["patch_embed.proj.weight"], "patch_embed.projection.bias": sd["patch_embed.proj.bias"]}
    _sam_blocks(out, lambda k: sd[k], lambda k: k in sd, "blocks.", _SAM_HF, "layers.", to_engine=False)
    return out


def engine_to_sam(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The inverse of sam_to_engine into the published layout (``image_encoder.*``; no neck, prompt encoder or mask decoder)."""
    out = {"pos_embed": sd["pos_embed"], "patch_embed.proj.weight": sd["patch_embed.proj.weight"], "patch_embed.proj.bias": sd["patch_embed.proj.bias"]}
    _sam_blocks(out, lambda k: sd[k], lambda k: k in sd, "blocks.", _SAM_PUB, "blocks.", to_engine=False)
    return {"image_encoder." + k: v for k, v in out.items()}


def sam_block_windows(sd: Dict[str, torch.Tensor]) -> List[int]:
    """Per block of an engine-layout SAM state dict: 0 for a global block (its tables have 2 S0 - 1 rows, S0 = the pos_embed grid's side),
    else the window side w (2 w - 1 rows).  The checkpoint does not store global_attn_indexes: this is how they are recovered."""
    s0 = sd["pos_embed"].shape[1]
    out, i = [], 0
    while f"blocks.{i}.attn.rel_pos_h" in sd:
        side = (sd[f"blocks.{i}.attn.rel_pos_h"].shape[0] + 1) // 2
        out.append(0 if side == s0 else side)
        i += 1
    return out


def random_sam_state_dict(embed_dim=768, depth=12, native_grid=64, window=14, global_idx=(2, 5, 8, 11), seed=0, patch=16, in_chans=3) -> Dict[str, torch.Tensor]:
    """Seeded random SAM image-encoder weights in the ENGINE's layout (used when no local checkpoint exists; ``engine_to_sam`` /
    ``engine_to_sam_hf`` give the other two).  Blocks as random_dinov2_state_dict's (non-trivial LayerNorm affines and biases) with Q and K
    rows large enough for peaked attention (as random_croco_state_dict), relative-position tables ~ 0.5 N(0, 1) (2 * native_grid - 1 rows
    in the global blocks, 2 * window - 1 in the others; the reference initialises them to zero, under which a wrong index would not show),
    a [1, S, S, C] position table ~ 0.02 N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    sd = {"pos_embed": 0.02 * torch.randn(1, native_grid, native_grid, embed_dim, generator=g)}
    bound = 1.0 / math.sqrt(in_chans * patch * patch)
    sd["patch_embed.proj.weight"] = (torch.rand(embed_dim, in_chans, patch, patch, generator=g) * 2 - 1) * bound
    sd["patch_embed.proj.bias"] = (torch.rand(embed_dim, generator=g) * 2 - 1) * bound
    _random_blocks(sd, "blocks.", _TIMM_BLOCK, embed_dim, depth, g)
    for i in range(depth):
        p = f"blocks.{i}."
        sd[p + "attn.qkv.weight"][:2 * embed_dim] *= 1.5 / (0.02 * math.sqrt(embed_dim))
        rows = 2 * (native_grid if i in tuple(global_idx) else window) - 1
        sd[p + "attn.rel_pos_h"] = 0.5 * torch.randn(rows, 64, generator=g) / 8.0
        sd[p + "attn.rel_pos_w"] = 0.5 * torch.randn(rows, 64, generator=g) / 8.0
    return sd


def sincos_pos_embed_2d(embed_dim: int, grid_hw, add_cls_token: bool = True) -> np.ndarray:
    """evals/models/utils.py:75-102 + HF get_2d_sincos_pos_embed_from_grid (MAE): half of the
    channels encode the w coordinate ("w goes first"), half the h coordinate; each half is
    [sin | cos] of pos * 1/10000^(2i/D)."""
    gh, gw = grid_hw
    grid_h = np.arange(gh, dtype=np.float32)
    grid_w = np.arange(gw, dtype=np.float32)
    grid = np.stack(np.meshgrid(grid_w, grid_h), axis=0).reshape(2, 1, gh, gw)

    def one_dim(d, pos):
        omega = np.arange(d // 2, dtype=float) / (d / 2.0)
        omega = 1.0 / 10000 ** omega
        out = np.einsum("m,d->md", pos.reshape(-1), omega)
        return np.concatenate([np.sin(out), np.cos(out)], axis=1)

    emb = np.concatenate([one_dim(embed_dim // 2, grid[0]), one_dim(embed_dim // 2, grid[1])], axis=1)
    if add_cls_token:
        emb = np.concatenate([np.zeros([1, embed_dim]), emb], axis=0)
    return emb


class _Named(nn.Module):
    pass


class ViTParams(nn.Module):
    """Parameter container with the key layout of the DINO / iBOT / timm VisionTransformer
    (cls_token, pos_embed, patch_embed.proj, blocks.i.{norm1,attn.qkv,attn.proj,norm2,mlp.fc1,mlp.fc2}, norm)."""

    def __init__(self, sd: Dict[str, torch.Tensor]):
        super().__init__()
        for k, v in sd.items():
            parts = k.split(".")
            mod = self
            for p in parts[:-1]:
                if not hasattr(mod, p):
                    setattr(mod, p, _Named())
                mod = getattr(mod, p)
            mod.register_parameter(parts[-1], nn.Parameter(v.clone().float(), requires_grad=False))
        self.embed_dim = (sd["cls_token"] if "cls_token" in sd else sd["pos_embed"]).shape[-1] if ("cls_token" in sd or "pos_embed" in sd) else sd["patch_embed.proj.weight"].shape[0]
        self.depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))

    @property
    def blocks(self):
        return [getattr(self._modules["blocks"], str(i)) for i in range(self.depth)]


def multilayer_indices(n: int) -> List[int]:
    return [n // 4 - 1, n // 2 - 1, n // 4 * 3 - 1, n - 1]


class ViTBackbone(nn.Module):
    """Base of the ViT wrappers.  Subclasses set: self.<params_attr> (ViTParams), heads, ln_eps,
    pos_embed_mode, tap_input_of_block; and call _setup_taps()."""

    params_attr = "vit"
    heads = 12
    ln_eps = 1e-6
    pos_embed_mode = "dino"
    tap_input_of_block = False
    act = "gelu"  # after fc1: 'gelu' (erf), 'quick_gelu', 'gelu_tanh' (ViTEngine)
    rope_freq = None  # CroCo v2: RoPE<freq> on Q and K of every block (ViTEngine(rope_freq=...)); None: no rotation
    rel_pos_grid = None  # BEiT: (gh, gw) of the grid the blocks' relative-position bias tables belong to (ViTEngine(rel_pos_grid=...))
    replay_after_norm = False  # BEiT v2's wrapper: all blocks + fc_norm, then the tapped loop over the blocks again (ViTEngine.forward_taps)
    weights_from_file = False  # set by the wrappers' loaders when ``find_checkpoint`` hit: arms the range guard under 'auto'
    _range_guard = None  # the ``range_guard=`` keyword (None: MVP_F16_GUARD, default 'auto'); see ``range_guard_action``
    _guard_sig = None  # the engine signature the guard was last resolved for (None: never)
    _f16_report = None  # the last audit's table (``f16_range_report``)
    supports_pipelining = True  # per-slot buffers, tap-BN running-statistics updates deferred to the consumer (mvp/pipeline.py)
    graph_safe = True  # a pipelined forward launches only this library's kernels on fixed buffers: it can be captured in a hipGraph

    def supports_grouping(self) -> bool:
        """True when the pipeline may stack several batches into ONE forward (mvp/pipeline.py, ``group``): the dense / multilayer
        paths, whose ``forward`` ends in ``_finish(_extract(images))``.  The single-tap ``return_cls`` shortcuts return a bare
        token tensor and stay one batch per forward."""
        return not (len(self.multilayers) == 1 and getattr(self, "return_cls", False))

    def _setup_taps(self, feat_dim, layer, return_multilayer, add_norm, num_layers):
        multilayers = multilayer_indices(num_layers)
        if return_multilayer:
            self.feat_dim = [feat_dim] * 4
            self.multilayers = multilayers
        else:
            self.feat_dim = feat_dim
            self.multilayers = [multilayers[-1] if layer == -1 else layer]
        self.layer = "-".join(str(x) for x in self.multilayers)
        self.add_norm = add_norm

    # ---- engine management
    def _params(self) -> ViTParams:
        return getattr(self, self.params_attr)

    def _signature(self):
        return tuple((p.data_ptr(), p._version) for p in self._params().parameters()) + (self._precision, self.act, self.rope_freq, self.rel_pos_grid)

    def engine(self) -> ViTEngine:
        sig = self._signature()
        if getattr(self, "_engine_sig", None) != sig:
            params = self._params()
            dev = next(params.parameters()).device
            if dev.type != "cuda":
                raise lib.MvpError("backbone parameters are on the CPU: call model.to('cuda') — the HIP path has no CPU fallback")
            sd = {k: v for k, v in params.state_dict().items()}
            self._engine_obj = ViTEngine(sd, heads=self.heads, patch=self.patch_size, ln_eps=self.ln_eps, precision=self._precision,
                                         device=dev, pos_embed_mode=self.pos_embed_mode, act=self.act, rope_freq=self.rope_freq,
                                         rel_pos_grid=self.rel_pos_grid)
            self.n_prefix = self._engine_obj.n_prefix
            self._engine_sig = sig
        return self._engine_obj

    def set_precision(self, precision) -> None:
        self._precision = parse_precision(precision)

    # ---- f16x2 range guard
    def set_range_guard(self, range_guard: Optional[str]) -> None:
        """``range_guard``: None (MVP_F16_GUARD decides; 'auto' when unset) or one of RANGE_GUARD_MODES.  The guard is pending again."""
        if range_guard is not None:
            range_guard_action(None, range_guard, False, 1)  # (validates the name)
        self._range_guard, self._guard_sig = range_guard, None

    def range_guard_action(self) -> str:
        from . import dist

        return range_guard_action(os.environ.get("MVP_F16_GUARD"), self._range_guard, bool(self.weights_from_file), dist.world_size())

    def f16_range_report(self) -> Optional[List[dict]]:
        """The per-site table of the guard's audited forward (``RangeAudit.read()``), None while no audit has run."""
        return self._f16_report

    def _engine_images(self, images: torch.Tensor) -> torch.Tensor:
        """What ``forward(images)`` hands the engine: the wrapper's own preprocessing of a raw batch.  Here: the resize to ``fixed_size``
        of the K / Q / V path; wrappers whose forward resizes the batch or rebuilds a position table for its size (BEiT v2, CroCo,
        MoCo-v3, MAE) override this, and their forward calls it, so the guard audits exactly what the engine will be fed."""
        if getattr(self, "return_kqv", False):
            return self.preprocess_image(images)[0]
        return images

    def _guard_pending(self, images: torch.Tensor) -> Optional[str]:
        """The guard's action ('warn' / 'raise' / 'fallback') while it is armed and still pending for the current engine signature, else
        None.  Every call reads MVP_F16_GUARD and the world size; an armed guard also builds the engine signature (a tuple over all
        parameters, as ``engine()`` does on every forward).  Launches nothing; a pending guard on a capturing stream raises here."""
        action = self.range_guard_action()
        if action == "off" or not images.is_cuda or self._guard_sig == self._signature():
            return None
        if torch.cuda.is_current_stream_capturing():
            raise lib.MvpError("the f16x2 range guard is still pending and the stream is capturing: run one eager forward (or "
                               "model.resolve_range_guard(images)) before the capture")
        return action

    def resolve_range_guard(self, images: torch.Tensor) -> None:
        """``images``: a raw batch, as ``forward`` takes it.  While the range guard is armed and pending for the current engine signature:
        the wrapper's own preprocessing (``_engine_images``), then ONE extra audited forward over the result (no tap BN, so no state is
        touched) on the current stream, one synchronise of that stream, and the action — 'warn': a warning naming the first site with a
        saturated or non-finite fp16 half; 'raise': MvpError; 'fallback': the warning, then ``set_precision('bf16x3')`` (the engine is
        rebuilt at the next forward, as after any signature change).  The guard is resolved either way.  FeaturePipeline calls this on
        every batch it is given (pending only on the first); ``_extract`` / ``extract_kqv`` and the single-tap class-token shortcuts call
        ``_guard`` on the batch they are about to run.  Never inside a stream capture: a pending guard there raises before it launches
        anything, because it would have to synchronise."""
        action = self._guard_pending(images)
        if action is not None:
            self._audit_range(self._engine_images(images), action)

    def _guard(self, images: torch.Tensor) -> None:
        """``resolve_range_guard`` for a batch that is already what the engine is fed (the forward paths)."""
        action = self._guard_pending(images)
        if action is not None:
            self._audit_range(images, action)

    def _audit_range(self, images: torch.Tensor, action: str) -> None:
        sig = self._signature()
        eng = self.engine()
        audit = RangeAudit(eng)
        if audit.sites:
            if images.ndim == 3:
                images = images.unsqueeze(0)
            with torch.no_grad():
                eng.forward_taps(images, self.multilayers, bn=None, bn_mode=2, pack=False, tap_input_of_block=self.tap_input_of_block,
                                 replay_after_norm=bool(self.replay_after_norm), audit=audit)
            torch.cuda.current_stream().synchronize()
        report = audit.read()
        self._f16_report, self._guard_sig = report, sig
        bad = tripped_sites(report)
        if not bad:
            return
        first = bad[0]
        top = max((r["max_abs"] for r in report), key=lambda v: float("inf") if v != v else v)
        msg = (f"f16x2 range guard: {first['site']} holds {first['n_sat'] + first['n_nonfinite']} of {first['n_scanned']} values at or "
               f"beyond fp16's range (|v| >= 65504; {len(bad)} of {len(report)} sites tripped, max |v| over all sites = {top})")
        if action == "raise":
            raise lib.MvpError(msg + ": run this model with precision='bf16x3' (MVP_PRECISION=bf16x3)")
        if action == "fallback":
            warnings.warn(msg + ": falling back to precision='bf16x3'")
            self.set_precision("bf16x3")
            self._guard_sig = self._signature()  # (a bf16x3 engine has nothing to audit)
        else:
            warnings.warn(msg + ": the features are wrong; run this model with precision='bf16x3' (MVP_PRECISION=bf16x3)")

    # ---- forward glue (dino.py:164-210 / ibot.py:182-220 / mocov3.py:146-186 / mae.py:195-237)
    def _tap_bn(self):
        if not self.add_norm:
            return None, 2
        bns = [dict(weight=bn.weight, bias=bn.bias, running_mean=bn.running_mean, running_var=bn.running_var,
                    num_batches_tracked=bn.num_batches_tracked) for bn in self.batchnorms]
        return bns, (0 if self.training else 1)

    def _extract(self, images: torch.Tensor, n_spatial_from_grid: bool = True, want_cls: bool = False):
        if not images.is_cuda:
            raise lib.MvpError("images must be on the HIP device (no CPU fallback)")
        self._guard(images)
        eng = self.engine()
        bns, mode = self._tap_bn()
        with torch.no_grad():
            taps = eng.forward_taps(images, self.multilayers, bn=bns, bn_mode=mode, tap_input_of_block=self.tap_input_of_block,
                                    want_cls=want_cls or self.output in ("cls", "dense-cls"), groups=pipeline.current_groups(),
                                    **({"replay_after_norm": True} if self.replay_after_norm else {}))
            # (num_batches_tracked is incremented by the tap kernel's statistics pass: no extra launch)
        return taps

    def extract_kqv(self, images):
        """dino.py:82-139, ibot.py:128-180 (the same code in both wrappers): K / Q / V of the last attention layer (the output of its fused qkv projection), CLS row dropped,
        as [B, C, h*w] ("kqv": [B, 3C, h*w], k | q | v).  No centre padding on this path (the reference calls prepare_tokens directly;
        ``fixed_size`` is a multiple of the patch size in every config)."""
        if images.ndim == 3:
            images = images.unsqueeze(0)
        if images.ndim == 5:
            images = images.squeeze(0)
        if not images.is_cuda:
            raise lib.MvpError("images must be on the HIP device (no CPU fallback)")
        if images.shape[-2] % self.patch_size or images.shape[-1] % self.patch_size:
            raise ValueError("extract_kqv: the image size must be a multiple of the patch size (dino.py:105 has no padding on this path)")
        self._guard(images)
        with torch.no_grad():
            qkv = self.engine().last_block_qkv(images)
        bs, _, C3 = qkv.shape
        C = C3 // 3
        hw = (images.shape[-2] // self.patch_size) * (images.shape[-1] // self.patch_size)
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        pick = {"k": [k], "q": [q], "v": [v], "kqv": [k, q, v]}[self.mode_selected]
        return torch.cat([t[:, 1:].transpose(1, 2).reshape(bs, C, hw) for t in pick], dim=1)

    def preprocess_image(self, rgb_image):
        """dino.py:141-161, ibot.py:102-124: torchvision ``Resize((fixed_size, fixed_size))`` of a [C,H,W] / [B,C,H,W] tensor (bilinear, antialiased)."""
        from . import functional as MF

        x = rgb_image if rgb_image.ndim == 4 else rgb_image.unsqueeze(0)
        return MF.resize_antialias(x, (self.fixed_size, self.fixed_size)), self.fixed_size // self.patch_size, self.fixed_size // self.patch_size

    def _finish(self, taps: TapOutputs):
        """tokens_to_output (evals/models/utils.py:105-124) per tap.  'dense' is the kernel's own output; 'cls' is the
        (tap-normalised) CLS token the tap kernel emits next to the map; 'gap' / 'dense-cls' are shape glue on those.
        A grouped forward (TapGroups: one TapOutputs per batch) is finished batch by batch -> pipeline.GroupedFeatures."""
        if isinstance(taps, TapGroups):
            return pipeline.GroupedFeatures(self._finish(t) for t in taps)
        if self.output == "dense":
            outs = list(taps)
        elif self.output == "cls":
            outs = list(taps.cls)
        elif self.output == "gap":
            outs = [t.mean(dim=(2, 3)) for t in taps]
        elif self.output == "dense-cls":
            outs = [torch.cat((t, c[:, :, None, None].expand(-1, -1, t.shape[2], t.shape[3])), dim=1).contiguous() for t, c in zip(taps, taps.cls)]
        else:
            raise ValueError(f"unknown output type {self.output!r}")
        if self.output != "dense":
            return outs[0] if len(outs) == 1 else outs
        return taps[0] if len(taps) == 1 else taps
