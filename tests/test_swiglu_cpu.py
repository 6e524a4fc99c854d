"""CPU checks of the SwiGLU backbones and DINO ViT-B/8: the hidden-width rule, hub-layout checkpoints with ``mlp.w12`` / ``mlp.w3``
keys, the fp64 restatement (tests/swiglu_ref.py) against transformers' Dinov2SwiGLUFFN, the seeded generator's unchanged default, the
two choice files, the wrapper's constructors and refusal, and mvp_swiglu_fwd as declared, exported, bound, sized and validated."""
import ctypes as C
import hashlib
import os
import re
import warnings

import pytest
import torch
import yaml

import swiglu_ref
from conftest import REPO


def _dino(**kw):
    from evals.models.dino import DINO

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "no local checkpoint: seeded random init"
        return DINO(**kw)


def test_hidden_width_rule():
    from mvp import backbone as bb

    for c, h in ((128, 344), (192, 512), (1536, 4096), (384, 1024), (768, 2048)):
        assert bb.swiglu_hidden(c) == swiglu_ref.hidden_width(c) == h, c
    sd = bb.random_dinov2_state_dict(128, 2, 0, seed=1, ffn="swiglu")
    assert sd["blocks.1.mlp.w12.weight"].shape == (688, 128) and sd["blocks.1.mlp.w12.bias"].shape == (688,)
    assert sd["blocks.1.mlp.w3.weight"].shape == (128, 344) and sd["blocks.1.mlp.w3.bias"].shape == (128,)
    assert not any(".mlp.fc" in k for k in sd) and "blocks.1.ls2.gamma" in sd
    with pytest.raises(ValueError):
        bb.random_dinov2_state_dict(128, 2, 0, ffn="glu")
    assert bb.DINOV2_ARCH["vitg14"] == (1536, 40, 0) and bb.DINOV2_FFN == {"vitg14": "swiglu"}
    assert bb.DINOV2_HUB_NAMES["vitg14"] == "dinov2_vitg14_pretrain"


def test_hub_layout_round_trip_with_chunked_blocks(tmp_path, monkeypatch):
    """``blocks.<chunk>.<i>.mlp.w12.*`` / ``mlp.w3.*`` under MVP_CKPT_DIR with the hub's file name: flattened, nothing renamed or lost."""
    from mvp import backbone as bb

    sd = bb.random_dinov2_state_dict(128, 4, 0, seed=9, ffn="swiglu")
    chunked = {}
    for k, v in sd.items():
        m = re.match(r"blocks\.(\d+)\.(.*)", k)
        chunked[f"blocks.{int(m.group(1)) // 2}.{m.group(1)}.{m.group(2)}" if m else k] = v
    eng = bb.dinov2_hub_to_engine(chunked)
    assert set(eng) == {k for k in sd if k != "mask_token" and not k.startswith("norm.")}
    for k, v in eng.items():
        assert torch.equal(v, sd[k]), k
    torch.save(chunked, tmp_path / "dinov2_vitg14_pretrain.pth")
    monkeypatch.setenv("MVP_CKPT_DIR", str(tmp_path))
    m = _dino(dino_name="dinov2", model_name="vitg14", return_multilayer=True)
    got = m.vit.state_dict()
    assert m.vit.depth == 4 and m.multilayers == [0, 1, 2, 3] and m.n_prefix == 1
    for k in ("blocks.3.mlp.w12.weight", "blocks.3.mlp.w12.bias", "blocks.0.mlp.w3.weight", "blocks.2.mlp.w3.bias", "blocks.3.ls2.gamma"):
        assert torch.equal(got[k], sd[k]), k


def test_restated_ffn_matches_transformers_swiglu():
    """tests/swiglu_ref.py's FFN against transformers' Dinov2SwiGLUFFN (weights_in = w12, weights_out = w3) in fp64 on shared weights."""
    from transformers import Dinov2Config
    from transformers.models.dinov2.modeling_dinov2 import Dinov2SwiGLUFFN

    for c in (128, 192):
        hf = Dinov2SwiGLUFFN(Dinov2Config(hidden_size=c, mlp_ratio=4, num_attention_heads=c // 64, use_swiglu_ffn=True)).double()
        h = swiglu_ref.hidden_width(c)
        assert hf.weights_in.weight.shape == (2 * h, c) and hf.weights_out.weight.shape == (c, h)
        g = torch.Generator().manual_seed(c)
        sd = {"m.w12.weight": torch.randn(2 * h, c, generator=g, dtype=torch.float64) * 0.2, "m.w12.bias": torch.randn(2 * h, generator=g, dtype=torch.float64),
              "m.w3.weight": torch.randn(c, h, generator=g, dtype=torch.float64) * 0.2, "m.w3.bias": torch.randn(c, generator=g, dtype=torch.float64)}
        hf.load_state_dict({"weights_in.weight": sd["m.w12.weight"], "weights_in.bias": sd["m.w12.bias"],
                            "weights_out.weight": sd["m.w3.weight"], "weights_out.bias": sd["m.w3.bias"]}, strict=True)
        y = torch.randn(3, 7, c, generator=g, dtype=torch.float64)
        with torch.no_grad():
            ref = hf(y)
        got = swiglu_ref.ffn(sd, "m.", y)
        err = ((got - ref).abs().max() / ref.abs().max()).item()
        assert err < 1e-12, (c, err)


def test_default_generator_draws_what_the_parent_commit_drew():
    """random_dinov2_state_dict(128, 4, 4, seed=9) (ffn left at its default): key order and every tensor as before ``ffn=`` existed;
    the digest and sums below were taken on the commit before it."""
    from mvp import backbone as bb

    sd = bb.random_dinov2_state_dict(128, 4, 4, seed=9)
    assert len(sd) == 64 and not any(".w12." in k or ".w3." in k for k in sd)
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.numpy().tobytes())
    assert h.hexdigest() == "2113b3adaa012c0b30e64cd28559d80e016536ff77f0dfa33fd924ff69a71a8b"
    sums = {"pos_embed": (12.1546397432856, 2801.2340962359967), "blocks.0.mlp.fc1.weight": (5.215352534882005, 1045.618759585151),
            "blocks.3.ls2.gamma": (11.389015929198194, 11.389015929198194), "blocks.3.mlp.fc2.bias": (-0.04952040276839398, 1.8656993782205973),
            "register_tokens": (-3.872349697165191, 203.37398933432996)}
    for k, (s, a) in sums.items():
        assert sd[k].double().sum().item() == s and sd[k].double().abs().sum().item() == a, k
    # the same seed with ffn="swiglu": identical up to the first MLP draw
    glu = bb.random_dinov2_state_dict(128, 4, 4, seed=9, ffn="swiglu")
    for k in ("pos_embed", "register_tokens", "blocks.0.attn.proj.bias", "blocks.0.ls1.gamma"):
        assert torch.equal(glu[k], sd[k]), k


@pytest.mark.parametrize("name,dino_name,model_name,like,output", [("dinov2_g14", "dinov2", "vitg14", "dinov2_l14", "dense-cls"),
                                                                     ("dino_b8", "dino", "vitb8", "dino_b16", "dense")])
def test_choice_files_compose(name, dino_name, model_name, like, output):
    """The reference reaches both models through ``backbone.model_name=`` overrides of these files' siblings: each new file is its
    sibling with only ``model_name`` changed, and composes under the training and the correspondence entry points."""
    from mvp import config

    node = yaml.safe_load(open(os.path.join(config.CONFIG_DIR, "backbone", name + ".yaml")))
    sibling = yaml.safe_load(open(os.path.join(config.CONFIG_DIR, "backbone", like + ".yaml")))
    assert node == {**sibling, "model_name": model_name} and node["dino_name"] == dino_name
    for entry in ("depth_training", "spair_correspondence"):
        cfg = config.compose(entry, [f"backbone={name}"])
        assert cfg["backbone"]["dino_name"] == dino_name and cfg["backbone"]["model_name"] == model_name and cfg["backbone"]["output"] == output


def test_dino_vitb8_constructs_with_patch_8():
    m = _dino(dino_name="dino", model_name="vitb8", return_multilayer=True)
    assert m.patch_size == 8 and m.vit.embed_dim == 768 and m.heads == 12 and m.vit.depth == 12
    assert m.vit.pos_embed.shape == (1, 28 * 28 + 1, 768) and m.multilayers == [2, 5, 8, 11] and m.checkpoint_name == "dino_vitb8"
    kqv = _dino(dino_name="dino", model_name="vitb8", return_kqv=True, mode_selected="kqv")
    assert kqv.return_kqv and kqv.patch_size == 8
    # ViT-B/16 draws what it drew: the generator's patch argument is the model's own
    from mvp import backbone as bb

    b16 = _dino(dino_name="dino", model_name="vitb16")
    assert torch.equal(b16.vit.state_dict()["pos_embed"], bb.random_vit_state_dict(seed=0)["pos_embed"]) and b16.patch_size == 16


def test_dinov2_vitg14_constructs_from_weights_and_refuses_without():
    from mvp import backbone as bb

    sd = bb.random_dinov2_state_dict(1536, 2, ffn="swiglu")
    m = _dino(dino_name="dinov2", model_name="vitg14", weights=sd, output="dense-cls", return_multilayer=True)
    assert m.heads == 24 and m.vit.embed_dim == 1536 and m.patch_size == 14 and m.n_prefix == 1 and m.feat_dim == [3072] * 4
    assert m.vit.state_dict()["blocks.1.mlp.w12.weight"].shape == (8192, 1536) and m.vit.state_dict()["blocks.1.mlp.w3.weight"].shape == (1536, 4096)
    assert bb.multilayer_indices(bb.DINOV2_ARCH["vitg14"][1]) == [9, 19, 29, 39]
    with pytest.raises(NotImplementedError, match="SwiGLU"):
        _dino(dino_name="dinov2", model_name="vitg14")
    with pytest.raises(NotImplementedError):
        _dino(dino_name="dinov2", model_name="vitb16")
    with pytest.raises(NotImplementedError):
        _dino(dino_name="dino", model_name="vitb14")


# ------------------------------------------------------------------------------------------------ C ABI
EINVAL, P = -1, 0x10000


def test_swiglu_export_abi():
    from mvp import lib, ops

    so = lib.load()
    assert hasattr(so, "mvp_swiglu_fwd") and lib.SYMBOLS["mvp_swiglu_fwd"] is lib.SwigluArgs
    assert so.mvp_sizeof(b"mvp_swiglu_args") == C.sizeof(lib.SwigluArgs) == 56 and lib.STRUCTS["mvp_swiglu_args"] is lib.SwigluArgs
    assert lib.info().abi_version == 8 and callable(ops.swiglu)
    header = open(os.path.join(REPO, "include", "mvp_hip.h")).read()
    assert "Added within 8: mvp_swiglu_fwd" in header and "#define MVP_ABI_VERSION 8" in header and "struct mvp_swiglu_args {" in header


def test_swiglu_argument_checks():
    """Validation precedes any launch.  (No well-formed call is made here: it would launch.)"""
    from mvp import lib

    fn = lib.load().mvp_swiglu_fwd

    def code(**kw):
        a = dict(h12=P, out_hi=P, out_lo=P, out_f32=P, M=5, H=344, ld_in=688, ld_out=384, out_layout=0, out_f16=0)
        a.update(kw)
        return fn(C.byref(lib.SwigluArgs(**a)), None)

    assert fn(None, None) == EINVAL and code(h12=None) == EINVAL
    assert code(out_hi=None, out_lo=None, out_f32=None) == EINVAL  # no output at all
    assert code(out_hi=None) == EINVAL  # a lo half without its hi half
    assert code(M=0) == EINVAL and code(M=-2) == EINVAL
    assert code(H=0, ld_in=0, ld_out=0) == EINVAL and code(H=340, ld_in=680) == EINVAL and code(H=-8) == EINVAL  # H % 8
    assert code(ld_in=684) == EINVAL and code(ld_in=690) == EINVAL and code(ld_in=-688) == EINVAL  # < 2H; not % 4
    assert code(ld_out=336) == EINVAL and code(ld_out=348) == EINVAL  # < H; not % 8
    assert code(out_layout=1, ld_out=360) == EINVAL and code(out_layout=2) == EINVAL and code(out_layout=-1) == EINVAL  # A_ILV32 needs % 32
    assert code(out_f16=2) == EINVAL and code(out_f16=1, out_lo=None) == EINVAL  # the fp16 pair has no one-product form
    for ptr in ("h12", "out_hi", "out_lo", "out_f32"):
        assert code(**{ptr: P + 8}) == EINVAL, ptr  # 16-byte alignment
    assert code(M=1 << 22, H=4096, ld_in=8192, ld_out=4096) == EINVAL  # M * ld_out / 8 = 2^31
    assert code(M=(1 << 22) + 5, H=8, ld_in=16, ld_out=4096) == EINVAL
