"""CPU checks of the BEiT v2 backbone: the engine's dense expansion of the relative-position tables against the reference module's own
(bit for bit), the fp64 restatement (tests/beit_ref.py) against the goldens built from the reference's VisionTransformer, the checkpoint
converter, the choice file, the wrapper's surface, and the C ABI of mvp_attention_bias_fwd with its argument validation (no launch, no
GPU)."""
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

REF_DIGESTS = json.load(open(os.path.join(GOLDEN, "reference_config_digests_beit.json")))


def _quiet(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "no local checkpoint: seeded random init"
        return fn(*a, **kw)


# ------------------------------------------------------------------------------------------------ the dense bias
@pytest.mark.parametrize("name,grid,blocks", [("beit_tiny.npz", (4, 6), 4), ("beit_mid.npz", (14, 14), 1)])
def test_dense_bias_equals_the_reference_modules_bit_for_bit(name, grid, blocks):
    """mvp.vit.dense_rel_pos_bias of the fixtures' tables == the [H, N, N] array the reference's Attention module forms, on the non-square
    4 x 6 grid (a y / x swap shows) and on 14 x 14; the padding columns are zero; tests/beit_ref.dense_bias (pair by pair) agrees."""
    import beit_ref
    import make_goldens_beit as mg
    from mvp import vit

    g = load_golden(name)
    cfg = mg.TINY if name == "beit_tiny.npz" else mg.MID
    sd = mg.state_dict(cfg)
    np.testing.assert_allclose(mg.checksums(sd), g["checksums"], rtol=1e-9)
    N = 1 + grid[0] * grid[1]
    for i in range(blocks):
        table = torch.from_numpy(g[f"table_block{i}"])  # (stored: the comparison below is bit for bit on any machine)
        np.testing.assert_allclose(sd[f"blocks.{i}.attn.rel_pos_bias_table"].numpy(), table.numpy(), rtol=1e-6, atol=1e-7)
        dense = vit.dense_rel_pos_bias(table, *grid)
        want = torch.from_numpy(g[f"bias_block{i}"])
        assert dense.shape == (2, N, 64 * ((N + 63) // 64)) and dense.dtype == torch.float32
        assert torch.equal(dense[:, :, :N], want) and not bool(dense[:, :, N:].any())
        if grid == (4, 6):
            assert torch.equal(beit_ref.dense_bias(table, *grid), want)
            swapped = vit.dense_rel_pos_bias(table, grid[1], grid[0])  # (the same table length: the mistake the explicit grid prevents)
            assert not torch.equal(swapped[:, :, :N], want)
    with pytest.raises(Exception, match="grid"):
        vit.dense_rel_pos_bias(sd["blocks.0.attn.rel_pos_bias_table"], grid[0] + 1, grid[1])


def test_rel_pos_index_corners():
    from mvp import vit

    idx = vit.rel_pos_index(4, 6)
    n = 7 * 11 + 3
    assert idx.shape == (25, 25) and int(idx[0, 0]) == n - 1 and bool((idx[0, 1:] == n - 3).all()) and bool((idx[1:, 0] == n - 2).all())
    assert int(idx[1, 1]) == 3 * 11 + 5 and int(idx[2, 1]) == 3 * 11 + 6 and int(idx[1 + 6, 1]) == 4 * 11 + 5  # one step in x, one in y
    assert int(idx[1:, 1:].min()) == 0 and int(idx[1:, 1:].max()) == n - 4


# ------------------------------------------------------------------------------------------------ restatement vs goldens
def test_restatement_matches_tiny_goldens():
    import beit_ref
    import make_goldens_beit as mg

    g = load_golden("beit_tiny.npz")
    sd = mg.state_dict(mg.TINY)
    x = torch.from_numpy(g["images"]).double()
    for tag, norm in (("dense", False), ("norm", True)):
        outs = beit_ref.features(sd, x, [0, 1, 2, 3], img_size=mg.TINY["img_size"], add_norm=norm)
        for j, o in enumerate(outs):
            assert o.shape == (2, 128, 4, 6)
            assert rel_l2(o.numpy(), g[f"{tag}_tap{j}"]) < 1e-6, (tag, j)
    cls = beit_ref.features(sd, x, [3], img_size=mg.TINY["img_size"], return_cls=True)[0]
    assert rel_l2(cls.numpy(), g["cls"]) < 1e-6
    # the quirk is visible: without the first pass + fc_norm the taps are far from the goldens
    once = beit_ref.features(sd, x, [3], img_size=mg.TINY["img_size"], replay=False)[0]
    assert rel_l2(once.numpy(), g["dense_tap3"]) > 1e-2


def test_restatement_matches_mid_goldens():
    import beit_ref
    import make_goldens_beit as mg
    from make_goldens_dinov2 import sample_index

    g = load_golden("beit_mid.npz")
    sd = mg.state_dict(mg.MID)
    outs = beit_ref.features(sd, mg.images(mg.MID).double(), [0, 1, 2, 3], img_size=mg.MID["img_size"])
    for j, o in enumerate(outs):
        o = o.numpy()
        assert tuple(g[f"dense_tap{j}_shape"]) == o.shape == (2, 128, 14, 14)
        assert rel_l2(o.reshape(-1)[sample_index(o.size)], g[f"dense_tap{j}"]) < 1e-6, j


# ------------------------------------------------------------------------------------------------ converter
def _same(a, b):
    assert sorted(a) == sorted(b), (sorted(set(a) ^ set(b)))
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_converter_round_trip_and_layouts():
    from mvp import backbone as bb

    sd = bb.random_beit_state_dict(128, 4, 16, (64, 96), seed=3)
    assert "pos_embed" not in sd and sd["blocks.0.attn.rel_pos_bias_table"].shape == (7 * 11 + 3, 2)
    assert bool((sd["blocks.2.attn.qkv.bias"][128:256] == 0).all()) and bool((sd["blocks.2.attn.qkv.bias"][:128] != 0).any())
    assert float(sd["blocks.0.attn.rel_pos_bias_table"].std()) > 0.5 and float(sd["blocks.0.ls1.gamma"].std()) > 0.01
    pub = bb.engine_to_beit(sd)
    assert "blocks.0.attn.q_bias" in pub and "blocks.0.attn.v_bias" in pub and "blocks.0.gamma_1" in pub and "blocks.0.gamma_2" in pub
    assert "blocks.0.attn.relative_position_bias_table" in pub and not any("qkv.bias" in k or "ls1" in k or "rel_pos_bias_table" in k for k in pub)
    _same(bb.beit_to_engine(pub), sd)  # the bare dict
    _same(bb.beit_to_engine({"model": pub}), sd)  # the published wrapper
    _same(bb.beit_to_engine(sd), sd)  # already the engine's layout
    extra = dict(pub)
    extra.update({"blocks.0.attn.relative_position_index": torch.zeros(25, 25, dtype=torch.long), "head.weight": torch.zeros(3, 128),
                  "head.bias": torch.zeros(3), "mask_token": torch.zeros(1, 1, 128)})
    _same(bb.beit_to_engine({"model": extra}), sd)
    with pytest.raises(ValueError, match="K bias"):
        bad = dict(sd)
        bad["blocks.0.attn.qkv.bias"] = torch.ones(384)
        bb.engine_to_beit(bad)


def test_shared_table_expands_to_every_block():
    from mvp import backbone as bb

    sd = bb.random_beit_state_dict(128, 4, 16, 64, seed=4)
    pub = {k: v for k, v in bb.engine_to_beit(sd).items() if not k.endswith("relative_position_bias_table")}
    shared = torch.randn(7 * 7 + 3, 2, generator=torch.Generator().manual_seed(1))
    pub["rel_pos_bias.relative_position_bias_table"] = shared
    pub["rel_pos_bias.relative_position_index"] = torch.zeros(17, 17, dtype=torch.long)
    eng = bb.beit_to_engine({"model": pub})
    assert not any(k.startswith("rel_pos_bias.") for k in eng)
    for i in range(4):
        assert torch.equal(eng[f"blocks.{i}.attn.rel_pos_bias_table"], shared)
    assert eng["blocks.0.attn.rel_pos_bias_table"].data_ptr() != eng["blocks.1.attn.rel_pos_bias_table"].data_ptr()


def test_wrong_grid_tables_are_refused():
    from evals.models.beit_v2 import BEiTV2
    from mvp import backbone as bb
    from mvp.lib import MvpError

    assert bb.beit_grid(27 * 27 + 3) == (14, 14) and bb.beit_grid(7 * 11 + 3, (4, 6)) == (4, 6)
    with pytest.raises(MvpError, match="re-interpolating"):
        bb.beit_grid(7 * 11 + 3)  # not a square grid's length
    with pytest.raises(MvpError, match="re-interpolating"):
        bb.beit_grid(27 * 27 + 3, (16, 16))
    sd = bb.random_beit_state_dict(128, 4, 16, (64, 96), seed=5)
    with pytest.raises(MvpError, match="re-interpolating"):
        BEiTV2(weights=sd)  # a 4 x 6 table without img_size
    assert BEiTV2(weights=sd, img_size=(96, 64)).rel_pos_grid == (6, 4)  # (the same table length: only the caller knows the grid)
    with pytest.raises(MvpError, match="re-interpolating"):
        BEiTV2(weights=sd, img_size=(64, 64))
    sd["blocks.2.attn.rel_pos_bias_table"] = torch.zeros(5 * 5 + 3, 2)
    with pytest.raises(MvpError, match="re-interpolating"):
        BEiTV2(weights=sd, img_size=(64, 96))


# ------------------------------------------------------------------------------------------------ choice file, wrapper surface
def test_choice_file_matches_reference_compose_and_instantiate():
    from mvp import config

    assert sorted(REF_DIGESTS) == ["beit-v2_vitb16"]
    node = yaml.safe_load(open(os.path.join(config.CONFIG_DIR, "backbone", "beit-v2_vitb16.yaml")))
    assert hashlib.sha256(json.dumps(node, sort_keys=True).encode()).hexdigest() == REF_DIGESTS["beit-v2_vitb16"], node
    for entry in ("depth_training", "spair_correspondence"):
        cfg = config.compose(entry, ["backbone=beit-v2_vitb16"])
        assert cfg["backbone"]["_target_"] == "evals.models.beit_v2.BEiTV2" and cfg["backbone"]["output"] == "dense"
    model = _quiet(config.instantiate, node, return_multilayer=True)
    assert type(model).__name__ == "BEiTV2" and model.feat_dim == [768] * 4 and model.add_norm is True and model.return_cls is False
    assert model.rel_pos_grid == (14, 14) and model.replay_after_norm is True


def test_wrapper_surface():
    """beit_v2.py:17-67: checkpoint_name, feat_dim, multilayers, layer, patch_size, batchnorms; class token, no position table."""
    import evals.models
    from evals.models.beit_v2 import BEiTV2
    from mvp import backbone as bb

    assert evals.models.BEiTV2 is BEiTV2
    m = _quiet(BEiTV2, return_multilayer=True)
    assert m.checkpoint_name == "$beit_v2$_beit_vitb16_dense_2-5-8-11"
    assert m.feat_dim == [768] * 4 and m.multilayers == [2, 5, 8, 11] and m.layer == "2-5-8-11" and m.patch_size == 16 and len(m.batchnorms) == 4
    assert m.heads == 12 and m.ln_eps == 1e-6 and m.act == "gelu" and m.n_prefix == 1 and m.img_size == (224, 224) and m.arch == "vit"
    assert hasattr(m.model, "cls_token") and hasattr(m.model, "fc_norm") and not hasattr(m.model, "pos_embed") and m.model.depth == 12
    assert m.model.blocks[0].attn.rel_pos_bias_table.shape == (732, 12)
    s = _quiet(BEiTV2, model_name="vitb16", layer=3, output="gap")  # (``layer`` and ``output`` are accepted and, as in the reference, not used)
    assert s.feat_dim == 768 and s.multilayers == [11] and s.layer == "11" and len(s.batchnorms) == 1 and s.add_norm is False and s.output == "gap"
    assert s.checkpoint_name == "$beit_v2$_vitb16_gap_11"
    assert bb.BEIT_CKPT_FILE == "beit_v2_vitb16.pth"
    t = BEiTV2(weights=bb.random_beit_state_dict(128, 4, 16, (64, 96), seed=1), img_size=(64, 96), return_multilayer=True)
    assert t.rel_pos_grid == (4, 6) and t.img_size == (64, 96) and t.multilayers == [0, 1, 2, 3] and t.feat_dim == [128] * 4
    assert t.supports_grouping() and not BEiTV2(weights=bb.random_beit_state_dict(128, 4, 16, 64, seed=1), return_cls=True).supports_grouping()
    with pytest.raises(AssertionError):
        BEiTV2(arch="beit_vitl16")


def test_return_kqv_is_refused():
    from evals.models.beit_v2 import BEiTV2

    with pytest.raises(NotImplementedError, match="return_kqv"):
        BEiTV2(return_kqv=True)


def test_local_checkpoint_is_found(tmp_path, monkeypatch):
    from evals.models.beit_v2 import BEiTV2
    from mvp import backbone as bb

    sd = bb.random_beit_state_dict(128, 4, 16, 64, seed=9)
    torch.save({"model": bb.engine_to_beit(sd)}, tmp_path / "beit_v2_vitb16.pth")
    monkeypatch.setenv("MVP_CKPT_DIR", str(tmp_path))
    m = BEiTV2()
    assert m.rel_pos_grid == (4, 4) and m.model.depth == 4
    assert torch.equal(m.model.blocks[1].attn.rel_pos_bias_table, sd["blocks.1.attn.rel_pos_bias_table"])
    assert torch.equal(m.model.blocks[3].attn.qkv.bias, sd["blocks.3.attn.qkv.bias"])


# ------------------------------------------------------------------------------------------------ C ABI
def test_attention_bias_abi():
    from mvp import lib

    so = lib.load()
    assert hasattr(so, "mvp_attention_bias_fwd") and lib.SYMBOLS["mvp_attention_bias_fwd"] is lib.AttentionBiasArgs
    assert so.mvp_sizeof(b"mvp_attention_bias_args") == C.sizeof(lib.AttentionBiasArgs) == C.sizeof(lib.AttentionArgs) + 24
    assert so.mvp_sizeof(b"mvp_attention_args") == C.sizeof(lib.AttentionArgs)
    assert lib.info().abi_version == 8
    assert lib.STRUCTS["mvp_attention_bias_args"] is lib.AttentionBiasArgs
    header = open(os.path.join(REPO, "include", "mvp_hip.h")).read()
    assert "Added within 8: mvp_attention_bias_fwd" in header and "struct mvp_attention_bias_args {" in header
    assert "#define MVP_ABI_VERSION 8" in header


def test_attention_bias_argument_checks():
    """Every MVP_EINVAL of mvp_attention_bias_fwd: the host checks run before any launch, so fake (aligned, non-NULL) addresses do."""
    from mvp import lib

    fn = lib.load().mvp_attention_bias_fwd
    EINVAL = -1
    B, N, H = 1, 197, 2
    Cw = H * 64
    P = 0x10000

    def code(bias=P, ld=256, hs=None, att=None, **kw):
        f = dict(qkv_hi=P, qkv_lo=P, out_hi=P, out_lo=P, B=B, N=N, H=H, ld_qkv=3 * Cw, ld_out=Cw, scale=0.125, precision=lib.PREC_BF16X3,
                 out_layout=lib.PAIR_SEPARATE, v_format=0, out_f16=0)
        f.update(kw)
        a = lib.AttentionBiasArgs(lib.AttentionArgs(**f), bias, N * ld if hs is None else hs, ld)
        return fn(C.byref(a), None)

    assert fn(None, None) == EINVAL
    # everything mvp_attention_fwd rejects
    assert code(qkv_hi=None) == EINVAL and code(out_hi=None) == EINVAL and code(qkv_lo=None) == EINVAL and code(out_lo=None) == EINVAL
    assert code(B=0) == EINVAL and code(N=0) == EINVAL and code(H=0) == EINVAL
    assert code(ld_qkv=3 * Cw + 4) == EINVAL and code(ld_out=Cw + 2) == EINVAL and code(ld_qkv=3 * Cw - 8) == EINVAL and code(ld_out=Cw - 4) == EINVAL
    assert code(v_format=3) == EINVAL and code(precision=lib.PREC_BF16, v_format=1) == EINVAL and code(precision=lib.PREC_BF16, out_f16=1) == EINVAL
    assert code(out_layout=lib.PAIR_A_ILV32, ld_out=Cw) == EINVAL and code(precision=lib.PREC_BF16, out_layout=lib.PAIR_A_ILV32, ld_out=2 * Cw) == EINVAL
    assert code(precision=99) == EINVAL
    # the bias itself
    assert code(bias=None) == EINVAL and code(bias=P + 4) == EINVAL and code(bias=P + 8) == EINVAL
    assert code(ld=258) == EINVAL and code(ld=197) == EINVAL and code(ld=200) == EINVAL and code(ld=252) == EINVAL  # % 4, < 64 * ceil(N / 64)
    assert code(hs=N * 256 - 4) == EINVAL and code(hs=N * 256 + 2) == EINVAL
    assert code(N=64, ld=60) == EINVAL and code(N=65, ld=64) == EINVAL and code(N=257, ld=256) == EINVAL
