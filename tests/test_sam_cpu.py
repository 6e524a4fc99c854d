"""CPU checks of the SAM image-encoder backbone: the fp64 restatement (tests/sam_ref.py) against the goldens built from transformers'
SamVisionEncoder, the checkpoint converters, the window index tables, the host ``get_rel_pos`` against the module's own (bit for bit), the
wrapper's surface, the choice files, and the C ABI of mvp_gather_rows / mvp_relpos_terms / mvp_attention_relpos_fwd with their argument
validation (no launch, no GPU)."""
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

REF_DIGESTS = json.load(open(os.path.join(GOLDEN, "reference_config_digests_sam.json")))


def _quiet(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "no local checkpoint: seeded random init"
        return fn(*a, **kw)


def _layers(depth):
    return [depth // 4 - 1, depth // 2 - 1, depth // 4 * 3 - 1, depth - 1]


# ------------------------------------------------------------------------------------------------ the oracle against the goldens
@pytest.mark.parametrize("name", ["sam_tiny.npz", "sam_mid.npz", "sam_full_sampled.npz"])
def test_oracle_reproduces_the_goldens(name):
    """tests/sam_ref.forward in fp64 == the transformers module's taps to 2e-6 relative L2 (the goldens are stored in fp32 and the module
    computes its softmax in fp32: ~1e-7 each)."""
    import make_goldens_sam as mg
    import sam_ref
    from make_goldens_dinov2 import sample_index

    cfg = {"sam_tiny.npz": mg.TINY, "sam_mid.npz": mg.MID, "sam_full_sampled.npz": mg.FULL}[name]
    g = load_golden(name)
    sd = mg.state_dict(cfg)
    np.testing.assert_allclose(mg.checksums(sd), g["checksums"], rtol=1e-9)
    for size in cfg["sizes"]:
        tag = "" if len(cfg["sizes"]) == 1 else f"s{size[0]}_"
        outs, kept = sam_ref.forward(sd, mg.images(cfg, size), _layers(cfg["depth"]), keep_blocks=(0, 1) if name == "sam_tiny.npz" else ())
        assert len(outs) == 4
        for j, o in enumerate(outs):
            o = o.numpy()
            want = g[f"{tag}tap{j}"]
            if name == "sam_tiny.npz":
                assert o.shape == want.shape == (2, 128, 5, 7)
                got = o
            else:
                assert tuple(g[f"{tag}tap{j}_shape"]) == o.shape
                got = o.reshape(-1)[sample_index(o.size)]
            assert rel_l2(got, want) < 2e-6, (name, size, j, rel_l2(got, want))
        for i, k in kept.items():  # block 0 windowed (first window), block 1 global (first image)
            H = cfg["C"] // 64
            # (block 1 sees block 0's output, which carries the module's fp32 softmax: the same 2e-6 as the taps)
            assert rel_l2(k["rel_h"][:1].reshape(H, *k["rel_h"].shape[2:]).numpy(), g[f"rel_h_block{i}"]) < 2e-6
            assert rel_l2(k["rel_w"][:1].reshape(H, *k["rel_w"].shape[2:]).numpy(), g[f"rel_w_block{i}"]) < 2e-6


def test_host_rel_pos_equals_the_modules_bit_for_bit():
    """mvp.vit.sam_rel_pos on the fixture's fp32 tables == the module's own get_rel_pos: the windowed block's [3, 3, 64] (no interpolation)
    and the global block's [5, 5, 64] / [7, 7, 64] (15 rows interpolated to 9 / 13; gh != gw)."""
    import make_goldens_sam as mg
    from mvp import vit

    g, sd = load_golden("sam_tiny.npz"), mg.state_dict(mg.TINY)
    for i, (sh, sw) in ((0, (3, 3)), (1, (5, 7))):
        Rh, Rw = vit.sam_rel_pos(sh, sh, sd[f"blocks.{i}.attn.rel_pos_h"]), vit.sam_rel_pos(sw, sw, sd[f"blocks.{i}.attn.rel_pos_w"])
        assert Rh.dtype == torch.float32 and Rh.shape == (sh, sh, 64) and Rw.shape == (sw, sw, 64)
        assert torch.equal(Rh, torch.from_numpy(g[f"Rh_block{i}"])) and torch.equal(Rw, torch.from_numpy(g[f"Rw_block{i}"]))


# ------------------------------------------------------------------------------------------------ index tables
@pytest.mark.parametrize("gh,gw,w", [(5, 7, 3), (16, 16, 14), (14, 14, 14), (28, 28, 14)])
def test_window_index_tables(gh, gw, w):
    """partition and un-partition are inverse on the real rows, -1 exactly on the pad rows, and the partition is segment_anything's
    (pad, view, permute) order."""
    from mvp import vit

    B = 2
    part, unpart = vit.sam_window_index(B, gh, gw, w)
    nwh, nww = -(-gh // w), -(-gw // w)
    assert part.dtype == unpart.dtype == torch.int32 and part.shape == (B * nwh * nww * w * w,) and unpart.shape == (B * gh * gw,)
    assert int((part < 0).sum()) == B * (nwh * w * nww * w - gh * gw)
    live = part >= 0
    assert torch.equal(unpart[part[live].long()].long(), torch.arange(part.numel())[live])
    assert torch.equal(part[unpart.long()].long(), torch.arange(B * gh * gw))
    ids = torch.arange(B * gh * gw, dtype=torch.float32).reshape(B, gh, gw, 1) + 1  # 0 marks padding
    x = torch.nn.functional.pad(ids, (0, 0, 0, nww * w - gw, 0, nwh * w - gh))
    win = x.view(B, nwh, w, nww, w, 1).permute(0, 1, 3, 2, 4, 5).reshape(-1)
    assert torch.equal(win.long() - 1, part.long())
    if (gh, gw, w) == (14, 14, 14):
        assert nwh * nww == 1 and torch.equal(part.long(), torch.arange(B * 196))


# ------------------------------------------------------------------------------------------------ converters
def test_converters_round_trip_and_block_types():
    from mvp import backbone as bb

    sd = bb.random_sam_state_dict(128, 4, 8, 3, (1, 3), seed=5)
    assert sd["pos_embed"].shape == (1, 8, 8, 128) and sd["blocks.0.attn.rel_pos_h"].shape == (5, 64) and sd["blocks.1.attn.rel_pos_w"].shape == (15, 64)
    assert bb.sam_block_windows(sd) == [3, 0, 3, 0]
    pub = bb.engine_to_sam(sd)
    assert "image_encoder.blocks.2.mlp.lin1.weight" in pub and "image_encoder.patch_embed.proj.bias" in pub
    pub.update({"image_encoder.neck.0.weight": torch.zeros(4, 128, 1, 1), "prompt_encoder.pe_layer.x": torch.zeros(2), "mask_decoder.iou_token.weight": torch.zeros(1, 4)})
    hf = bb.engine_to_sam_hf(sd)
    assert "layers.3.layer_norm2.bias" in hf and "patch_embed.projection.weight" in hf
    hf_pref = {"vision_encoder." + k: v for k, v in hf.items()}
    hf_pref["vision_encoder.neck.conv1.weight"] = torch.zeros(4, 128, 1, 1)
    bare = {k[len("image_encoder."):]: v for k, v in pub.items() if k.startswith("image_encoder.")}
    for src in (pub, hf, hf_pref, bare, sd):
        back = bb.sam_to_engine(src)
        assert sorted(back) == sorted(sd)
        assert all(torch.equal(back[k], sd[k]) for k in sd)
    with pytest.raises(KeyError):
        bb.sam_to_engine({"cls_token": torch.zeros(1)})


def test_vit_h_is_refused():
    from evals.models.sam import SAM
    from mvp import backbone as bb
    from mvp.lib import MvpError

    with pytest.raises(MvpError, match="head_dim 64"):
        SAM("vit_h", weights=bb.random_sam_state_dict(1280, 2, 4, 3, (1,), seed=1))
    with pytest.raises(KeyError):
        SAM("vit_x")


# ------------------------------------------------------------------------------------------------ wrapper surface, choice files
def test_wrapper_surface():
    import evals.models
    from evals.models.sam import SAM
    from mvp import backbone as bb

    assert evals.models.SAM is SAM
    m = _quiet(SAM, "vit_b", return_multilayer=True)
    assert m.checkpoint_name == "sam_vit_b" and m.patch_size == 16 and m.image_size == (1024, 1024)
    assert m.feat_dim == [768] * 4 and m.multilayers == [2, 5, 8, 11] and m.layer == "2-5-8-11" and len(m.batchnorms) == 4 and m.add_norm is False
    assert m.heads == 12 and m.ln_eps == 1e-6 and m.act == "gelu" and m.n_prefix == 0 and m.pos_embed_mode == "sam"
    assert m.block_windows == [14, 14, 0, 14, 14, 0, 14, 14, 0, 14, 14, 0] and m.vit.blocks[2].attn.rel_pos_h.shape == (127, 64)
    assert not hasattr(m.vit, "neck") and not hasattr(m.vit, "cls_token") and m.supports_grouping()
    s = SAM("vit_b", output="gap", layer=1, weights=bb.random_sam_state_dict(128, 4, 8, 3, (1, 3), seed=2))
    assert s.feat_dim == 128 and s.multilayers == [1] and s.layer == "1" and s.output == "gap" and s.image_size == (128, 128) and s.heads == 2
    assert bb.SAM_CKPT_FILES["vit_b"] == "sam_vit_b_01ec64.pth" and bb.SAM_CKPT_FILES["vit_l"] == "sam_vit_l_0b3195.pth"
    with pytest.raises(NotImplementedError, match="add_norm"):
        SAM("vit_b", add_norm=True)
    with pytest.raises(AssertionError):
        SAM("vit_b", output="cls")
    with pytest.raises(AssertionError, match="100, 128"):
        s(torch.zeros(1, 3, 100, 128))


def test_local_checkpoint_is_found(tmp_path, monkeypatch):
    from evals.models.sam import SAM
    from mvp import backbone as bb

    sd = bb.random_sam_state_dict(128, 4, 8, 3, (1, 3), seed=9)
    torch.save(bb.engine_to_sam(sd), tmp_path / "sam_vit_l_0b3195.pth")
    monkeypatch.setenv("MVP_CKPT_DIR", str(tmp_path))
    m = SAM("vit_l")
    assert m.vit.depth == 4 and torch.equal(m.vit.blocks[1].attn.rel_pos_w, sd["blocks.1.attn.rel_pos_w"]) and m.checkpoint_name == "sam_vit_l"
    assert torch.equal(m.vit.blocks[3].mlp.fc2.weight, sd["blocks.3.mlp.fc2.weight"])


def test_choice_files_match_reference_compose_and_instantiate():
    from mvp import config

    assert sorted(REF_DIGESTS) == ["sam_base", "sam_large"]
    for name, arch, C_, depth in (("sam_base", "vit_b", 768, 12), ("sam_large", "vit_l", 1024, 24)):
        node = yaml.safe_load(open(os.path.join(config.CONFIG_DIR, "backbone", name + ".yaml")))
        assert hashlib.sha256(json.dumps(node, sort_keys=True).encode()).hexdigest() == REF_DIGESTS[name], node
        for entry in ("depth_training", "spair_correspondence"):
            cfg = config.compose(entry, [f"backbone={name}"])
            assert cfg["backbone"]["_target_"] == "evals.models.sam.SAM" and cfg["backbone"]["arch"] == arch
    model = _quiet(config.instantiate, node, return_multilayer=True)
    assert type(model).__name__ == "SAM" and model.feat_dim == [1024] * 4 and model.multilayers == [5, 11, 17, 23] and model.heads == 16


# ------------------------------------------------------------------------------------------------ C ABI
def test_sam_exports_abi():
    from mvp import lib

    so = lib.load()
    for sym, st, cname in (("mvp_gather_rows", lib.GatherRowsArgs, b"mvp_gather_rows_args"), ("mvp_relpos_terms", lib.RelposTermsArgs, b"mvp_relpos_terms_args"),
                           ("mvp_attention_relpos_fwd", lib.AttentionRelposArgs, b"mvp_attention_relpos_args")):
        assert hasattr(so, sym) and lib.SYMBOLS[sym] is st
        assert so.mvp_sizeof(cname) == C.sizeof(st) and lib.STRUCTS[cname.decode()] is st
    assert C.sizeof(lib.AttentionRelposArgs) == C.sizeof(lib.AttentionArgs) + 32  # pointer, int64, three ints, padded to 8
    assert so.mvp_sizeof(b"mvp_attention_args") == C.sizeof(lib.AttentionArgs) and so.mvp_sizeof(b"mvp_attention_bias_args") == C.sizeof(lib.AttentionBiasArgs)
    assert lib.info().abi_version == 8
    header = open(os.path.join(REPO, "include", "mvp_hip.h")).read()
    assert "Added within 8: mvp_gather_rows" in header and "#define MVP_ABI_VERSION 8" in header
    for n in ("mvp_gather_rows_args", "mvp_relpos_terms_args", "mvp_attention_relpos_args"):
        assert f"struct {n} {{" in header


EINVAL, P = -1, 0x10000


def test_gather_rows_argument_checks():
    from mvp import lib

    fn = lib.load().mvp_gather_rows

    def code(**kw):
        f = dict(in_hi=P, in_lo=P, out_hi=2 * P, out_lo=2 * P, idx=3 * P, rows=10, rows_in=8, cols=128, ld_in=128, ld_out=128)
        f.update(kw)
        return fn(C.byref(lib.GatherRowsArgs(**f)), None)

    assert fn(None, None) == EINVAL
    assert code(in_hi=None) == EINVAL and code(out_hi=None) == EINVAL and code(idx=None) == EINVAL
    assert code(in_lo=None) == EINVAL and code(out_lo=None) == EINVAL
    assert code(rows=0) == EINVAL and code(rows_in=0) == EINVAL and code(cols=0) == EINVAL and code(cols=124) == EINVAL
    assert code(ld_in=120) == EINVAL and code(ld_out=120) == EINVAL and code(ld_in=132) == EINVAL and code(ld_out=132) == EINVAL
    assert code(in_hi=P + 8) == EINVAL and code(in_lo=P + 2) == EINVAL and code(out_hi=P + 4) == EINVAL and code(out_lo=P + 8) == EINVAL and code(idx=P + 2) == EINVAL
    assert code(rows=1 << 30, cols=1024, ld_in=1024, ld_out=1024) == EINVAL


def test_relpos_terms_argument_checks():
    from mvp import lib

    fn = lib.load().mvp_relpos_terms
    H, N = 2, 15
    C3 = 3 * H * 64

    def code(**kw):
        f = dict(qkv=P, out_hi=P, out_lo=P, rel=P, rh=P, rw=P, rel_bh_stride=N * 8, M=2 * N, N=N, H=H, Qh=3, Qw=5, Kh=3, Kw=5, ld_in=C3, ld_out=C3, ld_rel=8,
                 precision=lib.PREC_BF16X3, v_format=0)
        f.update(kw)
        return fn(C.byref(lib.RelposTermsArgs(**f)), None)

    assert fn(None, None) == EINVAL
    for k in ("qkv", "out_hi", "out_lo", "rel", "rh", "rw"):
        assert code(**{k: None}) == EINVAL, k
    for k in ("qkv", "out_hi", "out_lo", "rel", "rh", "rw"):
        assert code(**{k: P + 8}) == EINVAL, k
    assert code(M=0) == EINVAL and code(N=0) == EINVAL and code(H=0) == EINVAL and code(M=2 * N + 1) == EINVAL
    assert code(Qh=5, Qw=5) == EINVAL and code(Qh=0) == EINVAL and code(Kh=0) == EINVAL and code(Kw=0) == EINVAL
    assert code(ld_rel=4) == EINVAL and code(ld_rel=10) == EINVAL and code(rel_bh_stride=N * 8 - 1) == EINVAL
    assert code(ld_in=C3 - 4) == EINVAL and code(ld_out=C3 - 8) == EINVAL and code(ld_in=C3 + 2) == EINVAL and code(ld_out=C3 + 4) == EINVAL
    assert code(precision=99) == EINVAL and code(precision=lib.PREC_F16X2) == EINVAL and code(v_format=3) == EINVAL and code(v_format=-1) == EINVAL
    assert code(precision=lib.PREC_BF16, v_format=1) == EINVAL
    assert code(H=257, ld_in=3 * 257 * 64, ld_out=3 * 257 * 64) == EINVAL  # the Q row of a token in LDS: H <= 256


def test_attention_relpos_argument_checks():
    """Every MVP_EINVAL of mvp_attention_relpos_fwd: the host checks run before any launch, so fake (aligned, non-NULL) addresses do."""
    from mvp import lib

    fn = lib.load().mvp_attention_relpos_fwd
    B, N, H = 1, 196, 2
    Cw = H * 64

    def code(rel=P, ld=28, hs=None, Kh=14, Kw=14, **kw):
        f = dict(qkv_hi=P, qkv_lo=P, out_hi=P, out_lo=P, B=B, N=N, H=H, ld_qkv=3 * Cw, ld_out=Cw, scale=0.125, precision=lib.PREC_BF16X3,
                 out_layout=lib.PAIR_SEPARATE, v_format=0, out_f16=0)
        f.update(kw)
        a = lib.AttentionRelposArgs(lib.AttentionArgs(**f), rel, f["N"] * ld if hs is None else hs, ld, Kh, Kw)
        return fn(C.byref(a), None)

    assert fn(None, None) == EINVAL
    # everything mvp_attention_fwd rejects
    assert code(qkv_hi=None) == EINVAL and code(out_hi=None) == EINVAL and code(qkv_lo=None) == EINVAL and code(out_lo=None) == EINVAL
    assert code(B=0) == EINVAL and code(N=0) == EINVAL and code(H=0) == EINVAL
    assert code(ld_qkv=3 * Cw + 4) == EINVAL and code(ld_out=Cw + 2) == EINVAL and code(ld_qkv=3 * Cw - 8) == EINVAL and code(ld_out=Cw - 4) == EINVAL
    assert code(v_format=3) == EINVAL and code(precision=lib.PREC_BF16, v_format=1) == EINVAL and code(precision=lib.PREC_BF16, out_f16=1) == EINVAL
    assert code(out_layout=lib.PAIR_A_ILV32, ld_out=Cw) == EINVAL and code(precision=99) == EINVAL
    # the decomposed bias itself
    assert code(rel=None) == EINVAL and code(rel=P + 2) == EINVAL
    assert code(Kh=0) == EINVAL and code(Kw=0) == EINVAL and code(Kh=14, Kw=13) == EINVAL and code(N=197) == EINVAL and code(Kh=-14, Kw=-14) == EINVAL
    assert code(ld=27) == EINVAL and code(hs=N * 28 - 1) == EINVAL
    assert code(N=1 << 16, Kh=256, Kw=256, ld=1 << 14) == EINVAL
