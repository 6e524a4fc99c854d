"""CPU checks of the CLIP and SigLIP backbones: the fp64 restatement (tests/langimg_ref.py) against the transformers-built goldens, the
state-dict converters, the five choice files, the wrappers' surface, the C ABI's argument validation for the two new activations and the
relaxed LayerNorm contract, and the large-M GEMM kernels' register / scratch usage against the parent commit's recorded numbers."""
import ctypes as C
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import warnings

import numpy as np
import pytest
import torch
import yaml

from conftest import GOLDEN, PKG, REPO, load_golden, rel_l2

sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

REF_DIGESTS = json.load(open(os.path.join(GOLDEN, "reference_config_digests_langimg.json")))


def _quiet(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "no local checkpoint: seeded random init"
        return fn(*a, **kw)


# ------------------------------------------------------------------------------------------------ restatement vs goldens
@pytest.mark.parametrize("name", ["clip_p16_quick", "clip_p14_gelu", "siglip_p16_tanh"])
def test_restatement_matches_tiny_goldens(name):
    import langimg_ref
    import make_goldens_langimg as mg

    g = load_golden("langimg_tiny.npz")
    fam, patch, _, act, _ = mg.TINY[name]
    sd = mg.tiny_state_dict(name)
    np.testing.assert_allclose(mg.checksums(sd), g[f"{name}_checksums"], rtol=1e-9)
    assert np.array_equal(mg.tiny_images().numpy(), g["images"])
    for output in (("dense", "dense-cls") if fam == "clip" else ("dense",)):
        outs = langimg_ref.dense_features(sd, torch.from_numpy(g["images"]).double(), [0, 1, 2, 3], patch=patch, act=act, eps=mg.EPS[fam], output=output)
        for j, o in enumerate(outs):
            assert rel_l2(o.numpy(), g[f"{name}_{output}_tap{j}"]) < 1e-6, (output, j)


def _full_cases():
    import make_goldens_langimg as mg

    return [(key, shape) for key, v in mg.FULL.items() for shape in v[4]]


@pytest.mark.parametrize("key,shape", _full_cases())
def test_restatement_matches_full_size_sampled_goldens(key, shape):
    import langimg_ref
    import make_goldens_langimg as mg
    from mvp import backbone as bb

    g = load_golden("langimg_full_sampled.npz")
    fam, _, act, _, _ = mg.FULL[key]
    sd, patch = mg.full_state_dict(key)
    np.testing.assert_allclose(mg.checksums(sd), g[f"{key}_checksums"], rtol=1e-9)
    B, H, W = shape
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    outs = langimg_ref.dense_features(sd, mg.full_images(B, H, W).double(), bb.multilayer_indices(depth), patch=patch, act=act, eps=mg.EPS[fam])
    for j, o in enumerate(outs):
        tag = f"{key}_{B}x{H}x{W}_tap{j}"
        assert tuple(o.shape) == tuple(g[tag + "_shape"]), tag
        assert rel_l2(o.numpy().reshape(-1)[mg.sample_index(o.numel())], g[tag]) < 1e-6, tag


# ------------------------------------------------------------------------------------------------ converters
def _same(a, b):
    assert sorted(a) == sorted(b), (sorted(set(a) ^ set(b)))
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_clip_converters_round_trip_and_agree():
    from mvp import backbone as bb

    oc = bb.random_clip_state_dict(128, 4, 16, 64, seed=1)
    oc["logit_scale"] = torch.tensor(1.0)  # (outside the image tower)
    eng = bb.openclip_to_engine(oc)
    dropped = {k for k in oc if k.startswith("visual.")} - set(bb.engine_to_openclip(eng))
    assert dropped == {"visual.ln_post.weight", "visual.ln_post.bias", "visual.proj"}, dropped
    assert "patch_embed.proj.bias" not in eng and eng["cls_token"].shape == (1, 1, 128) and eng["pos_embed"].shape == (1, 17, 128)
    _same(bb.openclip_to_engine(bb.engine_to_openclip(eng)), eng)
    _same(bb.openclip_to_engine({k[len("visual."):]: v for k, v in oc.items() if k.startswith("visual.")}), eng)  # the bare tower
    hf = bb.engine_to_hf_clip(eng)
    assert "vision_model.encoder.layers.3.self_attn.k_proj.weight" in hf and "vision_model.pre_layrnorm.weight" in hf
    hf["vision_model.post_layernorm.weight"] = torch.ones(128)
    hf["vision_model.embeddings.position_ids"] = torch.arange(17)[None]
    _same(bb.hf_clip_to_engine(hf), eng)  # the same weights in either layout: equal engine dicts
    _same(bb.hf_clip_to_engine({k[len("vision_model."):]: v for k, v in hf.items()}), eng)
    _same(bb.clip_to_engine(hf), eng)
    _same(bb.clip_to_engine(oc), eng)
    _same(bb.clip_to_engine(eng), eng)


def test_siglip_converters_round_trip_and_agree():
    from mvp import backbone as bb

    tm = bb.random_siglip_state_dict(128, 4, 16, 64, seed=2)
    eng = bb.timm_siglip_to_engine(tm)
    assert set(tm) - set(eng) == {"norm.weight", "norm.bias", "attn_pool.latent", "attn_pool.norm.weight"}
    assert "cls_token" not in eng and eng["pos_embed"].shape == (1, 16, 128)
    hf = bb.engine_to_hf_siglip(eng)
    hf["vision_model.post_layernorm.bias"] = torch.zeros(128)
    hf["vision_model.head.probe"] = torch.zeros(1, 1, 128)
    _same(bb.hf_siglip_to_engine(hf), eng)
    _same(bb.siglip_to_engine(hf), eng)
    _same(bb.siglip_to_engine(tm), eng)
    _same(bb.hf_siglip_to_engine(bb.engine_to_hf_siglip(eng)), eng)


# ------------------------------------------------------------------------------------------------ choice files
@pytest.mark.parametrize("name", sorted(REF_DIGESTS))
def test_choice_files_match_reference_compose_and_instantiate(name):
    from mvp import config

    node = yaml.safe_load(open(os.path.join(config.CONFIG_DIR, "backbone", name + ".yaml")))
    assert hashlib.sha256(json.dumps(node, sort_keys=True).encode()).hexdigest() == REF_DIGESTS[name], node
    for entry in ("depth_training", "spair_correspondence"):
        cfg = config.compose(entry, [f"backbone={name}"])
        assert cfg["backbone"]["_target_"] == node["_target_"] and cfg["backbone"]["output"] == "dense"
    model = _quiet(config.instantiate, node, return_multilayer=True)
    assert type(model).__module__ == node["_target_"].rsplit(".", 1)[0]
    assert len(model.feat_dim) == 4 and model.output == "dense" and model.add_norm == bool(node.get("add_norm", False))
    assert model.patch_size == (14 if name == "clip_l14" else 16)
    assert model.act == {"clip_b16": "quick_gelu", "clip_b16_laion": "gelu", "clip_l14": "quick_gelu"}.get(name, "gelu_tanh")


def test_five_reference_choices_are_recorded():
    assert sorted(REF_DIGESTS) == ["clip_b16", "clip_b16_laion", "clip_l14", "siglip_b16", "siglip_l16"]


# ------------------------------------------------------------------------------------------------ wrapper surface
@pytest.mark.parametrize("arch", ["ViT-B-16", "ViT-L-14", "ViT-L-14-336"])
def test_clip_wrapper_surface(arch):
    """clip.py:22-65: checkpoint_name, feat_dim (always the four-entry list, doubled for dense-cls), multilayers, layer, patch_size, batchnorms."""
    from evals.models.clip import CLIP
    from mvp import backbone as bb

    Cw, depth, patch, img = bb.CLIP_ARCH[arch]
    m = _quiet(CLIP, arch=arch, return_multilayer=True, output="dense-cls")
    assert m.checkpoint_name == "clip_" + arch.replace("-", "").lower() + "openai"
    assert m.feat_dim == [2 * Cw] * 4 and m.multilayers == [depth // 4 - 1, depth // 2 - 1, depth // 4 * 3 - 1, depth - 1]
    assert m.layer == "-".join(str(x) for x in m.multilayers) and m.patch_size == patch and len(m.batchnorms) == 4
    assert m.vit.pos_embed.shape == (1, (img // patch) ** 2 + 1, Cw) and m.heads == Cw // 64 and m.ln_eps == 1e-5
    assert m.act == "quick_gelu" and m.pos_embed_mode == "resize_aa" and not hasattr(m.vit.patch_embed.proj, "bias")
    s = _quiet(CLIP, arch=arch, checkpoint="laion2b_s34b_b88k", layer=3)
    assert s.feat_dim == [Cw] * 4 and s.multilayers == [3] and s.layer == "3" and s.act == "gelu" and s.add_norm is False
    assert _quiet(CLIP, arch=arch).multilayers == [depth - 1]


@pytest.mark.parametrize("ck", ["vit_base_patch16_siglip_224", "vit_base_patch16_siglip_384", "vit_large_patch16_siglip_256", "vit_large_patch16_siglip_384"])
def test_siglip_wrapper_surface(ck):
    """siglip.py:23-56: feat_dim a list only with return_multilayer, no CLS token, outputs gap / dense only."""
    from evals.models.siglip import SigLIP
    from mvp import backbone as bb

    Cw, depth, patch, img = bb.SIGLIP_ARCH[ck]
    m = _quiet(SigLIP, checkpoint=ck, return_multilayer=True)
    assert m.checkpoint_name == ck and m.feat_dim == [Cw] * 4 and m.multilayers == [depth // 4 - 1, depth // 2 - 1, depth // 4 * 3 - 1, depth - 1]
    assert m.layer == "-".join(str(x) for x in m.multilayers) and m.patch_size == 16 and len(m.batchnorms) == 4
    assert m.embed_size == (img // 16, img // 16) and m.vit.pos_embed.shape == (1, (img // 16) ** 2, Cw) and not hasattr(m.vit, "cls_token")
    assert m.n_prefix == 0 and m.ln_eps == 1e-6 and m.act == "gelu_tanh" and m.pos_embed_mode == "resize_aa"
    s = _quiet(SigLIP, checkpoint=ck, output="gap", act="gelu", resize_pos_embeds=False)
    assert s.feat_dim == Cw and s.multilayers == [depth - 1] and s.act == "gelu" and s.pos_embed_mode == "fixed"
    for bad in ("cls", "dense-cls"):
        with pytest.raises(AssertionError):
            _quiet(SigLIP, checkpoint=ck, output=bad)


def test_wrappers_refuse_unknown_architectures():
    from evals.models.clip import CLIP
    from evals.models.siglip import SigLIP

    with pytest.raises(NotImplementedError):
        CLIP(arch="ViT-H-14")
    with pytest.raises(NotImplementedError):
        SigLIP(checkpoint="vit_so400m_patch14_siglip_384")
    with pytest.raises(ValueError):
        _quiet(SigLIP, checkpoint="vit_base_patch16_siglip_224", act="relu")


def test_local_checkpoint_in_either_clip_layout(tmp_path, monkeypatch):
    from evals.models.clip import CLIP
    from mvp import backbone as bb

    oc = bb.random_clip_state_dict(128, 4, 16, 64, seed=5)
    torch.save(oc, tmp_path / "clip_vitb16openai.pth")
    monkeypatch.setenv("MVP_CKPT_DIR", str(tmp_path))
    m = CLIP(return_multilayer=True)
    for k, v in bb.openclip_to_engine(oc).items():
        assert torch.equal(m.vit.state_dict()[k], v), k
    assert m.vit.depth == 4 and m.multilayers == [0, 1, 2, 3]


# ------------------------------------------------------------------------------------------------ C ABI
def _gemm(act, **kw):
    from mvp import lib

    g = lib.GemmArgs(a_hi=16, a_lo=16, w_hi=16, w_lo=16, out_f32=16, M=-1, N=64, K=64, lda=64, ldw=64, ldo=64, act=act, precision=3)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def test_new_activations_pass_validation_where_gelu_does():
    """Host-side argument checks only (mvp_gemm_route launches nothing): the two new values are routed exactly as MVP_ACT_GELU is, for the
    tile kernels and the large-M kernel, both precisions; an unknown value is MVP_EINVAL; the convolution, split-K and mask forms
    refuse the new values; mvp_gemm_bias_act_res itself rejects what the route rejects."""
    from mvp import lib

    so = lib.load()
    assert (lib.ACT_QUICK_GELU, lib.ACT_GELU_TANH) == (3, 4)
    hdr = open(os.path.join(REPO, "include", "mvp_hip.h")).read()
    assert re.search(r"#define MVP_ACT_QUICK_GELU 3\b", hdr) and re.search(r"#define MVP_ACT_GELU_TANH 4\b", hdr)
    for M, N, K, prec in ((333, 3072, 768, 3), (50000, 3072, 768, 3), (333, 3072, 768, 2), (50000, 3072, 768, 2)):
        routes = []
        for act in (lib.ACT_GELU, lib.ACT_QUICK_GELU, lib.ACT_GELU_TANH):
            r = lib.GemmRoute()
            assert so.mvp_gemm_route(C.byref(_gemm(act, M=M, N=N, K=K, lda=K, ldw=K, ldo=N, precision=prec)), C.byref(r)) == 0, (act, M, prec)
            routes.append(bytes(r))
        assert routes[0] == routes[1] == routes[2]
    r = lib.GemmRoute()
    for act in (5, -1, 99):
        assert so.mvp_gemm_route(C.byref(_gemm(act, M=64)), C.byref(r)) == -1
        assert so.mvp_gemm_bias_act_res(C.byref(_gemm(act, M=64)), None) == -1
        assert so.mvp_gemm_pp(C.byref(_gemm(act, M=64)), None) == -1
    for act in (lib.ACT_QUICK_GELU, lib.ACT_GELU_TANH):
        assert so.mvp_gemm_route(C.byref(_gemm(act, M=64)), C.byref(r)) == 0
        assert so.mvp_gemm_route(C.byref(_gemm(act, M=64, splitk=2)), C.byref(r)) == -1
        assert so.mvp_gemm_route(C.byref(_gemm(act, M=64, out_mask=16, ldm=64)), C.byref(r)) == -1
        assert so.mvp_gemm_route(C.byref(_gemm(act, M=64, act_after_res=1)), C.byref(r)) == -1
        assert so.mvp_gemm_route(C.byref(_gemm(act, M=64, conv=1)), C.byref(r)) == -1
        assert so.mvp_gemm_scaled(C.byref(lib.GemmScaledArgs(_gemm(act, M=64), None)), None) == -1  # (no scale: refused before any launch)
    assert so.mvp_gemm_route(C.byref(_gemm(lib.ACT_GELU, M=64, K=256, lda=256, ldw=256, splitk=2)), C.byref(r)) == 0  # (what erf GELU may still do)


def test_layernorm_needs_one_output():
    from mvp import lib

    so = lib.load()
    a = lib.LayerNormArgs(16, 16, 16, None, None, None, 4, 64, 1e-5, 0, 0)
    assert so.mvp_layernorm_fwd(C.byref(a), None) == -1
    hdr = open(os.path.join(REPO, "include", "mvp_hip.h")).read()
    assert "out_f32 == x is allowed" in hdr
    assert so.mvp_get_info is not None and lib.info().abi_version == 8


# ------------------------------------------------------------------------------------------------ code objects
def _kernel_resources(obj):
    tool = lambda n: shutil.which(n) or os.path.join("/opt/rocm/llvm/bin", n)  # noqa: E731
    out = {}
    with tempfile.TemporaryDirectory() as td:  # the device code object: the object's offload bundle (.hip_fatbin), unbundled for gfx950
        fb, co = os.path.join(td, "fatbin"), os.path.join(td, "co")
        subprocess.run([tool("llvm-objcopy"), f"--dump-section=.hip_fatbin={fb}", obj, os.path.join(td, "host.o")], check=True)
        subprocess.run([tool("clang-offload-bundler"), "--type=o", f"--input={fb}", f"--output={co}", "--unbundle",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True)
        notes = subprocess.run([tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    for block in notes.split(".name:")[1:]:
        name = block.split("\n", 1)[0].strip()
        get = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))  # noqa: E731
        out[name] = {"vgpr_count": get("vgpr_count"), "private_segment_fixed_size": get("private_segment_fixed_size")}
    return out


def test_large_m_kernels_keep_their_registers():
    """Every gemm_pp kernel symbol of the parent commit's code object (tests/golden/gemm_pp_resources.json: read once from a parent
    build, the same way) still exists, spills nothing and uses no more VGPRs; the new activations' own instantiations (kernel-argument
    types mvp_gemm_kact / mvp_gemm_kscaled_act) exist for every operand layout and both precisions, and spill nothing either."""
    parent = json.load(open(os.path.join(GOLDEN, "gemm_pp_resources.json")))
    now = _kernel_resources(os.path.join(PKG, "csrc", "build", "gemm_pp.o"))
    assert len(parent) == 24
    for name, was in parent.items():
        assert name in now, name
        assert now[name]["private_segment_fixed_size"] == 0 and was["private_segment_fixed_size"] == 0, name
        assert now[name]["vgpr_count"] <= was["vgpr_count"], (name, now[name], was)
    new = {n: v for n, v in now.items() if n not in parent}
    assert sum("13mvp_gemm_kactE" in n for n in new) == 8 and sum("20mvp_gemm_kscaled_actE" in n for n in new) == 8, sorted(new)
    for n, v in new.items():
        assert v["private_segment_fixed_size"] == 0, (n, v)
