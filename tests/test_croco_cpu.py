"""CPU checks of the CroCo and CroCo v2 backbones: the fp64 restatement (tests/croco_ref.py) against the goldens built from the
reference's own CroCoNet, the checkpoint converter, the two choice files, the wrappers' surface, the engine's RoPE tables and the C ABI's
argument validation for mvp_rope2d_qkv (no launch, no GPU)."""
import ctypes as C
import hashlib
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch
import yaml

from conftest import GOLDEN, REPO, load_golden, rel_l2

sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

REF_DIGESTS = json.load(open(os.path.join(GOLDEN, "reference_config_digests_croco.json")))


def _quiet(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "no local checkpoint: seeded random init"
        return fn(*a, **kw)


# ------------------------------------------------------------------------------------------------ restatement vs goldens
@pytest.mark.parametrize("name", ["croco", "crocov2"])
def test_restatement_matches_tiny_goldens(name):
    """Both position forms on the non-square 4 x 6 grid, every tap, without and with add_norm."""
    import croco_ref
    import make_goldens_croco as mg
    from mvp import backbone as bb

    g = load_golden("croco_tiny.npz")
    ckpt = mg.tiny_state_dict(name)
    np.testing.assert_allclose(mg.checksums(ckpt), g[f"{name}_checksums"], rtol=1e-9)
    assert np.array_equal(mg.tiny_images().numpy(), g["images"])
    assert tuple(g["images"].shape) == (2, 3, 80, 112) and tuple(g[f"{name}_dense_tap0"].shape) == (2, 128, 4, 6)
    kw = dict(pos_embed=mg.TINY[name][0], img_size=mg.TINY_DIMS["img_size"])
    for tag, norm in (("dense", False), ("norm", True)):
        outs = croco_ref.dense_features(bb.croco_to_engine(ckpt), torch.from_numpy(g["images"]).double(), [0, 1, 2, 3], add_norm=norm, **kw)
        for j, o in enumerate(outs):
            assert rel_l2(o.numpy(), g[f"{name}_{tag}_tap{j}"]) < 1e-6, (tag, j)


def test_restatement_tells_the_axes_apart():
    """Swapping which half of a head takes y and which takes x moves the features far beyond the goldens' tolerance."""
    import croco_ref
    import make_goldens_croco as mg
    from mvp import backbone as bb

    g = load_golden("croco_tiny.npz")
    sd = bb.croco_to_engine(mg.tiny_state_dict("crocov2"))
    x = torch.from_numpy(g["images"]).double()
    orig = croco_ref.rope2d

    def swapped(t, hw, cos, sin):  # x angles on dims 0..31, y angles on dims 32..63
        n = torch.arange(hw[0] * hw[1])
        return torch.cat((croco_ref.rope1d(t[..., :32], n % hw[1], cos, sin), croco_ref.rope1d(t[..., 32:], n // hw[1], cos, sin)), dim=-1)

    try:
        croco_ref.rope2d = swapped
        out = croco_ref.dense_features(sd, x, [3], pos_embed="RoPE100", img_size=mg.TINY_DIMS["img_size"])[0]
    finally:
        croco_ref.rope2d = orig
    assert rel_l2(out.numpy(), g["crocov2_dense_tap3"]) > 1e-3


@pytest.mark.parametrize("key", ["croco_b16", "crocov2_b16"])
def test_restatement_matches_full_size_sampled_goldens(key):
    import croco_ref
    import make_goldens_croco as mg
    from mvp import backbone as bb

    g = load_golden("croco_full_sampled.npz")
    ckpt = mg.full_state_dict(key)
    np.testing.assert_allclose(mg.checksums(ckpt), g[f"{key}_checksums"], rtol=1e-9)
    B, H, W = mg.FULL_SHAPE
    outs = croco_ref.dense_features(bb.croco_to_engine(ckpt), mg.full_images().double(), [2, 5, 8, 11], pos_embed=mg.FULL[key][0], img_size=224)
    for j, o in enumerate(outs):
        tag = f"{key}_{B}x{H}x{W}_tap{j}"
        assert tuple(o.shape) == tuple(g[tag + "_shape"]) == (2, 768, 14, 14), tag
        assert rel_l2(o.numpy().reshape(-1)[mg.sample_index(o.numel())], g[tag]) < 1e-6, tag


# ------------------------------------------------------------------------------------------------ converter
def _same(a, b):
    assert sorted(a) == sorted(b), sorted(set(a) ^ set(b))
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("form", ["cosine", "RoPE100"])
def test_converter_on_the_published_layout(form):
    from mvp import backbone as bb

    ckpt = bb.random_croco_state_dict(128, 4, 16, (64, 96), pos_embed=form, seed=1)
    assert sorted(ckpt) == ["croco_kwargs", "model"] and ckpt["croco_kwargs"]["pos_embed"] == form and ckpt["croco_kwargs"]["img_size"] == (64, 96)
    m = ckpt["model"]
    eng = bb.croco_to_engine(ckpt)
    _same(bb.croco_to_engine(m), eng)  # the bare model dict
    _same(bb.croco_to_engine(eng), eng)  # already the engine's layout
    dropped = set(m) - set(bb.engine_to_croco(eng))
    expect = {"enc_norm.weight", "enc_norm.bias", "mask_token", "decoder_embed.weight", "decoder_embed.bias", "dec_norm.weight", "dec_norm.bias",
              "prediction_head.weight", "prediction_head.bias"} | ({"dec_pos_embed"} if form == "cosine" else set())
    assert dropped == expect, dropped ^ expect
    assert all(k.startswith(("blocks.", "patch_embed.proj.")) or k == "pos_embed" for k in eng) and "cls_token" not in eng
    assert ("pos_embed" in eng) == (form == "cosine")
    if form == "cosine":
        assert eng["pos_embed"].shape == (1, 24, 128) and torch.equal(eng["pos_embed"][0], m["enc_pos_embed"])
    assert torch.equal(eng["blocks.3.mlp.fc2.weight"], m["enc_blocks.3.mlp.fc2.weight"]) and eng["blocks.0.attn.qkv.bias"].shape == (384,)
    _same(bb.croco_to_engine(bb.engine_to_croco(eng)), eng)  # round trip
    with pytest.raises(KeyError):
        bb.croco_to_engine({**m, "something_else": torch.zeros(1)})


def test_sincos_table_is_the_reference_formula():
    """get_2d_sincos_pos_embed(C, grid, 0) (croco_models/pos_embed.py:22-69) restated here: meshgrid with w first, the first half of the
    channels from the first grid, each half [sin | cos] of pos / 10000^(2i / (C/2))."""
    from mvp import backbone as bb

    Cw, gh, gw = 128, 4, 6
    m = bb.random_croco_state_dict(Cw, 1, 16, (gh * 16, gw * 16), pos_embed="cosine", seed=0)["model"]
    grid = np.stack(np.meshgrid(np.arange(gw, dtype=np.float32), np.arange(gh, dtype=np.float32)), axis=0).reshape(2, -1)
    omega = 1.0 / 10000 ** (np.arange(Cw // 4, dtype=float) / (Cw / 4.0))
    halves = [np.concatenate([np.sin(np.outer(p, omega)), np.cos(np.outer(p, omega))], axis=1) for p in grid]
    ref = torch.from_numpy(np.concatenate(halves, axis=1)).float()
    assert torch.equal(m["enc_pos_embed"], ref) and ref.shape == (24, Cw)
    assert not torch.equal(ref[1], ref[gw])  # (one step in x is not one step in y)


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
    assert type(model).__module__ == node["_target_"].rsplit(".", 1)[0] and type(model).__name__ == node["_target_"].rsplit(".", 1)[1]
    assert model.feat_dim == [768] * 4 and model.output == "dense" and model.add_norm is True and model.return_cls is False
    assert model.rope_freq == (None if name == "croco_b16" else 100.0)


def test_two_reference_choices_are_recorded():
    assert sorted(REF_DIGESTS) == ["croco_b16", "crocov2_b16"]


# ------------------------------------------------------------------------------------------------ wrapper surface
@pytest.mark.parametrize("v2", [False, True])
def test_wrapper_surface(v2):
    """croco.py:20-72 / crocov2.py: checkpoint_name, feat_dim, multilayers, layer, patch_size, batchnorms; no class token; the position form."""
    from evals.models.croco import CROCO
    from evals.models.crocov2 import CROCOV2
    from mvp import backbone as bb

    cls = CROCOV2 if v2 else CROCO
    m = _quiet(cls, return_multilayer=True)
    assert m.checkpoint_name == ("crocov2_vitb16_dense" if v2 else "croco_vitb16_dense")
    assert m.feat_dim == [768] * 4 and m.multilayers == [2, 5, 8, 11] and m.layer == "2-5-8-11" and m.patch_size == 16 and len(m.batchnorms) == 4
    assert m.heads == 12 and m.ln_eps == 1e-6 and m.act == "gelu" and m.n_prefix == 0 and m.img_size == (224, 224) and m.arch == "vit"
    assert not hasattr(m.model, "cls_token") and not hasattr(m.model, "enc_norm") and m.model.depth == 12
    assert m.pos_form == ("RoPE100" if v2 else "cosine") and m.rope_freq == (100.0 if v2 else None) and m.pos_embed_mode == "fixed"
    assert hasattr(m.model, "pos_embed") != v2
    if not v2:
        assert m.model.pos_embed.shape == (1, 196, 768)
    s = _quiet(cls, layer=3, output="dense")  # (``layer`` is accepted and, as in the reference, not used)
    assert s.feat_dim == 768 and s.multilayers == [11] and s.layer == "11" and len(s.batchnorms) == 1 and s.add_norm is False
    assert bb.CROCO_CKPT_FILES == {"croco": "CroCo.pth", "crocov2": "CroCo_V2_ViTBase_BaseDecoder.pth"}
    with pytest.raises(AssertionError):
        cls(model_name="vitl16")


@pytest.mark.parametrize("v2", [False, True])
def test_return_kqv_is_refused(v2):
    from evals.models.croco import CROCO
    from evals.models.crocov2 import CROCOV2

    with pytest.raises(NotImplementedError, match="return_kqv"):
        (CROCOV2 if v2 else CROCO)(return_kqv=True)


def test_position_form_comes_from_the_checkpoint(tmp_path, monkeypatch):
    """``croco_kwargs["pos_embed"]`` wins over the class's own form; a local file in the published layout is found under MVP_CKPT_DIR;
    ``img_size`` may be a pair."""
    from evals.models.croco import CROCO
    from evals.models.crocov2 import CROCOV2
    from mvp import backbone as bb

    rope = bb.random_croco_state_dict(128, 4, 16, (64, 96), pos_embed="RoPE100", seed=5)
    cos = bb.random_croco_state_dict(128, 4, 16, 64, pos_embed="cosine", seed=6)
    m = CROCO(weights=rope, return_multilayer=True)
    assert m.rope_freq == 100.0 and m.pos_form == "RoPE100" and m.img_size == (64, 96) and m.multilayers == [0, 1, 2, 3] and m.feat_dim == [128] * 4
    m = CROCOV2(weights=cos)
    assert m.rope_freq is None and m.model.pos_embed.shape == (1, 16, 128) and m.img_size == (64, 64)
    with pytest.raises(NotImplementedError):
        CROCO(weights={"model": cos["model"], "croco_kwargs": {**cos["croco_kwargs"], "pos_embed": "learned"}})
    torch.save(rope, tmp_path / "CroCo_V2_ViTBase_BaseDecoder.pth")
    monkeypatch.setenv("MVP_CKPT_DIR", str(tmp_path))
    m = CROCOV2(return_multilayer=True)
    for k, v in bb.croco_to_engine(rope).items():
        assert torch.equal(m.model.state_dict()[k], v), k
    assert m.model.depth == 4 and m.rope_freq == 100.0 and m.img_size == (64, 96)
    with pytest.warns(UserWarning, match="CroCo.pth"):
        CROCO()  # (no CroCo.pth there: seeded random init, nothing fetched)


# ------------------------------------------------------------------------------------------------ C ABI
def _rope(**kw):
    from mvp import lib

    a = lib.Rope2dQkvArgs(qkv=64, out_hi=64, out_lo=64, cos_tab=64, sin_tab=64, M=32, N=16, H=2, n_prefix=1, gh=3, gw=5, tab_rows=5,
                          ld_in=384, ld_out=384, precision=3, v_format=0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_rope2d_struct_and_export():
    from mvp import lib

    so = lib.load()
    assert lib.SYMBOLS["mvp_rope2d_qkv"] is lib.Rope2dQkvArgs and hasattr(so, "mvp_rope2d_qkv")
    assert so.mvp_sizeof(b"mvp_rope2d_qkv_args") == C.sizeof(lib.Rope2dQkvArgs) == 88
    hdr = open(os.path.join(REPO, "include", "mvp_hip.h")).read()
    assert "struct mvp_rope2d_qkv_args {" in hdr and "Added within 8: mvp_rope2d_qkv" in hdr and lib.info().abi_version == 8
    assert "SEPARATE multiplies" in hdr  # (the header says which arithmetic form the rotation is)


@pytest.mark.parametrize("bad", [dict(qkv=None), dict(out_hi=None), dict(out_lo=None), dict(cos_tab=None), dict(sin_tab=None), dict(M=33), dict(N=17, M=34),
                                 dict(gh=5, gw=3, tab_rows=4), dict(tab_rows=4), dict(ld_in=380), dict(ld_out=376), dict(ld_in=386), dict(ld_out=388),
                                 dict(qkv=68), dict(out_hi=72), dict(out_lo=66), dict(cos_tab=68), dict(precision=1, v_format=1), dict(precision=1, v_format=2),
                                 dict(precision=2), dict(v_format=3), dict(H=0), dict(n_prefix=-1, gh=17, gw=1, tab_rows=17)])
def test_rope2d_refusals_before_any_launch(bad):
    """Every MVP_EINVAL case of include/mvp_hip.h; the host checks run before the launch, so nothing here touches a device (the valid
    argument set is never launched either)."""
    from mvp import lib

    assert lib.load().mvp_rope2d_qkv(C.byref(_rope(**bad)), None) == -1, bad


# ------------------------------------------------------------------------------------------------ engine tables
class _NoDevice:
    """ViTEngine.rope_for without an engine: the table arithmetic only."""

    def __init__(self, freq):
        self.rope_freq, self.device, self._rope = freq, torch.device("cpu"), {}


@pytest.mark.parametrize("grid", [(14, 14), (4, 6), (30, 40), (6, 4)])
def test_engine_rope_tables_are_bit_equal_to_the_reference_formula(grid):
    """RoPE2D.get_cos_sin (croco_models/pos_embed.py:119-129) for D = 32, freq 100, seq_len = max(gh, gw), evaluated here in fp32 on the CPU."""
    from mvp import vit

    gh, gw = grid
    cos, sin = vit.ViTEngine.rope_for(_NoDevice(100.0), gh, gw)
    D, base, seq_len = 32, 100.0, max(gh, gw)
    inv_freq = 1.0 / (base ** (torch.arange(0, D, 2).float() / D))
    t = torch.arange(seq_len, dtype=inv_freq.dtype)
    freqs = torch.einsum("i,j->ij", t, inv_freq).to(torch.float32)
    freqs = torch.cat((freqs, freqs), dim=-1)
    assert cos.dtype == torch.float32 and cos.shape == (seq_len, 32) and cos.is_contiguous() and sin.is_contiguous()
    assert torch.equal(cos, freqs.cos()) and torch.equal(sin, freqs.sin())
    assert torch.equal(cos[0], torch.ones(32)) and torch.equal(sin[0], torch.zeros(32)) and torch.equal(cos[:, :16], cos[:, 16:])
