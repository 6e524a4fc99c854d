"""Goldens of the BEiT v2 feature path (run on CPU, no download): tests/golden/beit_tiny.npz, beit_mid.npz, beit_full_sampled.npz.

The model is the reference's own ``VisionTransformer`` (evals/models/impl_utils/beit_model.py), imported at generation time from the
reference checkout behind a few-line ``timm`` stub (the module needs ``drop_path``, ``to_2tuple``, ``trunc_normal_`` and
``register_model`` from it, nothing else), built with the wrapper's keyword arguments (beit_v2.py:71-81) and loaded, strict, with
``mvp.backbone.engine_to_beit`` of the seeded weights of ``mvp.backbone.random_beit_state_dict`` (only the ``relative_position_index``
buffers are not in the dict).  Around the model the reference wrapper's ``forward`` is replayed (beit_v2.py:255-287): bilinear resize
(align_corners=False) to the model's image size — the wrapper's literal 224 generalised —, ``forward_features(...,
return_all_tokens=True)`` (all blocks, then ``fc_norm`` over all tokens), the blocks again, taps after blocks n/4-1, n/2-1, 3n/4-1,
n-1, without and with ``add_norm`` (a fresh train-mode BatchNorm1d over all B * N tokens, class token included), the class token of the
last block for ``return_cls``, and the reshape of the patch tokens into maps.  Everything in fp64.

tiny (stored in full, fp32): ``img_size=(64, 96)`` (a non-square 4 x 6 grid, N = 25: a y / x swap of the bias index shows), C = 128,
2 heads, depth 4, images [2, 3, 80, 112]; plus every block's table and its dense [H, N, N] bias as the reference's module computes it.
mid: 14 x 14 grid (N = 197), C = 128, 2 heads, depth 4, B = 2: table and dense bias of block 0 in full, 4096 sampled elements per tap.
full: ViT-B/16 at 224^2, B = 2: 4096 sampled elements per tap and each tap's shape.  Weight checksums in each."""
from __future__ import annotations

import importlib.util
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
from make_goldens_dinov2 import sample_index  # noqa: E402
from mvp import backbone as bb  # noqa: E402

TINY = dict(C=128, depth=4, img_size=(64, 96), size=(80, 112), B=2, seed=71)
MID = dict(C=128, depth=4, img_size=(224, 224), size=(200, 240), B=2, seed=72)
FULL = dict(C=768, depth=12, img_size=(224, 224), size=(224, 224), B=2, seed=73)


def images(cfg) -> torch.Tensor:
    return torch.randn(cfg["B"], 3, *cfg["size"], generator=torch.Generator().manual_seed(cfg["seed"] + 100))


def state_dict(cfg):
    """The seeded weights of a fixture in the engine's layout."""
    return bb.random_beit_state_dict(cfg["C"], cfg["depth"], 16, cfg["img_size"], seed=cfg["seed"])


def checksums(sd) -> np.ndarray:
    last = max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    keys = ["cls_token", "patch_embed.proj.weight", "blocks.0.attn.qkv.weight", "blocks.0.attn.qkv.bias", "blocks.0.attn.rel_pos_bias_table",
            f"blocks.{last}.attn.rel_pos_bias_table", f"blocks.{last}.ls2.gamma", "blocks.1.ls1.gamma", "fc_norm.weight", "fc_norm.bias"]
    return np.array([float(sd[k].double().abs().sum()) for k in keys])


def _beit_module():
    """The reference's beit_model module behind a stub of the four timm names it imports."""
    if "timm" not in sys.modules:
        timm, models, layers, registry = (types.ModuleType(n) for n in ("timm", "timm.models", "timm.models.layers", "timm.models.registry"))
        layers.drop_path = lambda x, drop_prob=0.0, training=False: x
        layers.to_2tuple = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
        layers.trunc_normal_ = lambda t, std=1.0, **kw: torch.nn.init.trunc_normal_(t, std=std)
        registry.register_model = lambda fn: fn
        timm.models, models.layers, models.registry = models, layers, registry
        sys.modules.update({"timm": timm, "timm.models": models, "timm.models.layers": layers, "timm.models.registry": registry})
    spec = importlib.util.spec_from_file_location("mvp_ref_beit_model", os.path.join(REF, "evals", "models", "impl_utils", "beit_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_model(cfg, sd):
    from functools import partial

    bm = _beit_module()
    net = bm.VisionTransformer(img_size=cfg["img_size"], patch_size=16, embed_dim=cfg["C"], depth=cfg["depth"], num_heads=cfg["C"] // 64, mlp_ratio=4,
                               norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),  # (beit_base_patch16_224's own arguments, at this fixture's size)
                               num_classes=0, drop_rate=0.0, use_mean_pooling=True, init_scale=0.001, use_rel_pos_bias=True, use_abs_pos_emb=False,
                               init_values=0.1, qkv_bias=True)  # beit_v2.py:71-81
    net.head = torch.nn.Identity()
    own = net.state_dict()
    full = dict(bb.engine_to_beit(sd))
    missing = sorted(set(own) - set(full))
    assert all(k.endswith("relative_position_index") for k in missing), missing
    full.update({k: own[k] for k in missing})
    net.load_state_dict(full, strict=True)
    assert net.pos_embed is None and net.rel_pos_bias is None
    return net.double().eval()


def reference_outputs(cfg, sd):
    """beit_v2.py:255-287 around the reference model -> dict(dense taps, normed taps, cls of the last block, per-block dense bias)."""
    net = reference_model(cfg, sd)
    depth = len(net.blocks)
    layers = [depth // 4 - 1, depth // 2 - 1, depth // 4 * 3 - 1, depth - 1]
    out = {"dense": [], "norm": []}
    with torch.no_grad():
        x = F.interpolate(images(cfg).double(), size=cfg["img_size"], mode="bilinear", align_corners=False)
        x = net.forward_features(x, return_all_tokens=True)
        for i, blk in enumerate(net.blocks):
            x = blk(x)
            if i in layers:
                bn = torch.nn.BatchNorm1d(x.shape[-1]).double().train()
                for tag, e in (("dense", x), ("norm", bn(x.permute(0, 2, 1)).permute(0, 2, 1))):
                    e = e[:, 1:]
                    b, n, c = e.shape
                    if cfg["img_size"][0] == cfg["img_size"][1]:
                        h = w = int(n ** 0.5)  # beit_v2.py:283
                    else:
                        h, w = cfg["img_size"][0] // 16, cfg["img_size"][1] // 16  # (the wrapper's square assumption, generalised)
                    out[tag].append(e.permute(0, 2, 1).contiguous().view(b, c, h, w))
        out["cls"] = x[:, 0]
        out["bias"] = []
        for blk in net.blocks:
            a = blk.attn
            n = a.window_size[0] * a.window_size[1] + 1
            out["bias"].append(a.relative_position_bias_table[a.relative_position_index.view(-1)].view(n, n, -1).permute(2, 0, 1).contiguous())
    return out


def golden(name, cfg, full_taps: bool, all_bias: bool):
    sd = state_dict(cfg)
    ref = reference_outputs(cfg, sd)
    out = {"checksums": checksums(sd)}
    if full_taps:
        out["images"] = images(cfg).numpy()
    for tag in ("dense", "norm"):
        for j, m in enumerate(ref[tag]):
            m = m.float().numpy()
            if full_taps:
                out[f"{tag}_tap{j}"] = m
            else:
                out[f"{tag}_tap{j}"] = m.reshape(-1)[sample_index(m.size)]
                out[f"{tag}_tap{j}_shape"] = np.array(m.shape)
    out["cls"] = ref["cls"].float().numpy()
    for i, b in enumerate(ref["bias"] if all_bias else ref["bias"][:1]):
        if all_bias or cfg["C"] == 128:
            out[f"bias_block{i}"] = b.float().numpy()
            out[f"table_block{i}"] = sd[f"blocks.{i}.attn.rel_pos_bias_table"].numpy()  # (the table the bias was expanded from)
    save_golden(name, out)


if __name__ == "__main__":
    torch.manual_seed(0)
    golden("beit_tiny.npz", TINY, True, True)
    golden("beit_mid.npz", MID, False, False)
    golden("beit_full_sampled.npz", FULL, False, False)
    print("wrote tests/golden/beit_tiny.npz, beit_mid.npz, beit_full_sampled.npz")
