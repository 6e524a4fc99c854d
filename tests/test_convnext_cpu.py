"""CPU checks of the ConvNeXt / ConvNeXt V2 backbone: the fp64 restatement (tests/convnext_ref.py) against the goldens built from
transformers' ConvNextModel / ConvNextV2Model, the checkpoint-layout converters, the wrapper's surface, the choice files, the kernel-test
fixtures' conditioning, and the C ABI of mvp_dwconv7_ln_fwd / mvp_grn_stats / mvp_grn_apply with their argument validation (no launch, no GPU)."""
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

REF_DIGESTS = json.load(open(os.path.join(GOLDEN, "reference_config_digests_convnext.json")))
CHOICES = {"convnext_in22k": ("convnext_base", "in22k", "cnxt_b_in22k", False),
           "convnext_fcmae": ("convnext_base", "fcmae_ft_in22k_in1k_384", "cnxt_b_fcmae_ft_in22k_in1k_384", True),
           "clip_convnext": ("convnext_base_w", "laion2b_s13b_b82k", "cnxt_b_w_laion2b_s13b_b82k", False),
           "clip_convnext_augreg": ("convnext_base_w", "laion2b_s13b_b82k_augreg", "cnxt_b_w_laion2b_s13b_b82k_augreg", False)}


def _quiet(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "no local checkpoint: seeded random init"
        return fn(*a, **kw)


# ------------------------------------------------------------------------------------------------ the oracle against the goldens
@pytest.mark.parametrize("v2", [False, True])
def test_oracle_reproduces_the_tiny_goldens(v2):
    """tests/convnext_ref in fp64 == the transformers module's stage outputs and the restated wrapper outputs to 2e-6 relative L2 (the
    goldens are stored in fp32: ~1e-7); every block of the fixture changes its input by more than 10 %."""
    import convnext_ref as ref
    import make_goldens_convnext as mg

    g = load_golden("convnext_tiny_v2.npz" if v2 else "convnext_tiny_v1.npz")
    sd = mg.state_dict(mg.TINY, v2)
    np.testing.assert_allclose(mg.checksums(sd), g["checksums"], rtol=1e-9)
    for size, shapes in zip(mg.TINY["sizes"], (((12, 20), (6, 10), (3, 5), (1, 2)), ((16, 20), (8, 10), (4, 5), (2, 2)))):
        tag = f"s{size[0]}_"
        img = torch.from_numpy(g[tag + "images"])
        assert torch.equal(img, mg.images(mg.TINY, size))
        change = []
        stages = ref.trunk(sd, ref.center_padding(img.double()), block_change=change)
        assert min(change) > 0.1 and min(g[tag + "block_change"]) > 0.1
        np.testing.assert_allclose(change, g[tag + "block_change"], rtol=1e-6)
        for j, s in enumerate(stages):
            assert tuple(s.shape) == (2, mg.TINY["widths"][j]) + shapes[j] == g[f"{tag}stage{j}"].shape
            assert rel_l2(s.numpy(), g[f"{tag}stage{j}"]) < 2e-6, (size, j)
        for output in ("dense", "gap"):
            outs = ref.wrapper_forward(sd, img, (0, 1, 2, 3), output)
            for j, o in enumerate(outs):
                assert o.shape == g[f"{tag}{output}{j}"].shape and rel_l2(o.numpy(), g[f"{tag}{output}{j}"]) < 2e-6, (size, output, j)
        assert tuple(outs[0].shape) == (2, 64)
        (last,) = ref.wrapper_forward(sd, img, (3,), "dense")
        assert tuple(last.shape) == (2, 256, shapes[0][0] // 4, shapes[0][1] // 4)


@pytest.mark.parametrize("name", ["convnext_mid.npz", "convnext_full_sampled.npz"])
def test_oracle_reproduces_the_sampled_goldens(name):
    import convnext_ref as ref
    import make_goldens_convnext as mg
    from make_goldens_dinov2 import sample_index

    cfg = {"convnext_mid.npz": mg.MID, "convnext_full_sampled.npz": mg.FULL}[name]
    g = load_golden(name)
    (size,) = cfg["sizes"]
    for v2 in (False, True):
        tag = "v2_" if v2 else "v1_"
        sd = mg.state_dict(cfg, v2)
        np.testing.assert_allclose(mg.checksums(sd), g[tag + "checksums"], rtol=1e-9)
        assert min(g[tag + "block_change"]) > 0.1 and len(g[tag + "block_change"]) == sum(cfg["depths"])
        stages = ref.trunk(sd, mg.images(cfg, size).double())
        for j, s in enumerate(stages):
            s = s.numpy()
            assert tuple(g[f"{tag}stage{j}_shape"]) == s.shape
            assert rel_l2(s.reshape(-1)[sample_index(s.size)], g[f"{tag}stage{j}"]) < 2e-6, (name, v2, j)
        (d,) = ref.wrapper_forward(sd, mg.images(cfg, size), (3,), "dense")
        d = d.numpy()
        assert tuple(g[tag + "dense3_shape"]) == d.shape == (cfg["B"], cfg["widths"][3], size[0] // 16, size[1] // 16)
        assert rel_l2(d.reshape(-1)[sample_index(d.size)], g[tag + "dense3"]) < 2e-6


def test_kernel_fixtures_have_no_ill_conditioned_rows():
    """LayerNorm amplifies an error of its input by 1 / sigma: no row of a random dwconv fixture may have sigma below 1e-3 of its RMS."""
    import convnext_ref as ref

    for Cdim in ref.DW_CHANNELS:
        for H, W in ref.DW_SIZES:
            x, w, b, _, _ = ref.dwconv_fixture(Cdim, H, W)
            assert ref.row_sigma_ratio(x, w, b) > ref.SIGMA_FLOOR, (Cdim, H, W)
    x, w, b, _, _ = ref.dwconv_fixture(64, 9, 13, ldx=80)
    assert x.shape[-1] == 80 and ref.row_sigma_ratio(x, w, b) > ref.SIGMA_FLOOR


def test_oracle_pieces():
    """The oracle's own pieces against first principles: a tap outside the image is zero; GRN of an all-zero image is finite."""
    import convnext_ref as ref

    x, w, b, gamma, beta = ref.dwconv_fixture(32, 3, 5, B=1)
    y = ref.dwconv7(x, w, b)
    want = b.double().clone()
    for ky in range(7):
        for kx in range(7):
            yy, xx = 0 + ky - 3, 4 + kx - 3
            if 0 <= yy < 3 and 0 <= xx < 5:
                want += w[:, ky, kx].double() * x[0, yy, xx].double()
    np.testing.assert_allclose(y[0, 0, 4].numpy(), want.numpy(), rtol=1e-12, atol=1e-12)
    h = torch.randn(2, 15, 64)
    h[1] = 0
    G, N = ref.grn_stats(h)
    out = ref.grn_apply(h, N, torch.randn(64), torch.randn(64))
    assert torch.isfinite(out).all() and float(G[1].abs().max()) == 0.0 and float(N[1].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ checkpoint layouts
@pytest.mark.parametrize("v2", [False, True])
def test_both_checkpoint_layouts_map_to_the_same_engine_tensors(v2):
    from mvp import convnext as cnx

    sd = cnx.random_state_dict((64, 128, 192, 256), (1, 1, 2, 1), v2=v2, seed=5)
    hf = cnx.engine_to_hf(sd)
    assert "embeddings.patch_embeddings.weight" in hf and "encoder.stages.2.layers.1.pwconv2.bias" in hf
    assert ("encoder.stages.0.layers.0.grn.weight" in hf) == v2 and ("encoder.stages.0.layers.0.layer_scale_parameter" in hf) == (not v2)
    if v2:
        assert tuple(hf["encoder.stages.3.layers.0.grn.bias"].shape) == (1, 1, 1, 1024)
    timm = cnx.engine_to_timm(sd)
    clip = cnx.engine_to_timm(sd, "visual.trunk.")
    clip.update({"visual.trunk.head.norm.weight": torch.ones(256), "visual.head.proj.weight": torch.ones(4, 256), "logit_scale": torch.ones(()),
                 "text_projection": torch.ones(4, 4)})
    timm.update({"head.fc.weight": torch.ones(10, 256), "head.norm.bias": torch.zeros(256), "norm_pre.weight": torch.ones(256)})
    prefixed = {("convnextv2." if v2 else "convnext.") + k: v for k, v in hf.items()}
    prefixed["classifier.weight"] = torch.ones(10, 256)
    for other in (hf, timm, clip, prefixed):
        eng = cnx.to_engine(other)
        assert set(eng) == set(sd)
        for k in sd:
            assert torch.equal(eng[k].reshape(-1), sd[k].reshape(-1)), k
    assert cnx.arch_of(cnx.to_engine(hf)) == ([64, 128, 192, 256], [1, 1, 2, 1], v2)
    with pytest.raises(ValueError):
        cnx.to_engine({"blocks.0.attn.qkv.weight": torch.ones(3, 3)})


def test_hf_module_loads_the_converted_weights_strictly():
    """engine_to_hf's keys are exactly transformers' (minus the pooled output's norm), for both versions."""
    import make_goldens_convnext as mg

    for v2 in (False, True):
        net = mg.reference_model(mg.TINY, mg.state_dict(mg.TINY, v2), v2)
        assert type(net).__name__ == ("ConvNextV2Model" if v2 else "ConvNextModel")


# ------------------------------------------------------------------------------------------------ the wrapper's surface
def _tiny_weights(v2=False):
    from mvp import convnext as cnx

    return cnx.random_state_dict((64, 128, 192, 256), (1, 1, 2, 1), v2=v2, seed=7)


def test_constructor_surface():
    import inspect

    from evals.models import ConvNext
    from evals.models.convnext import ConvNext as Direct

    assert ConvNext is Direct
    sig = inspect.signature(ConvNext.__init__)
    assert list(sig.parameters)[1:7] == ["arch", "checkpoint", "output", "layer", "return_multilayer", "add_norm"]
    d = {k: v.default for k, v in sig.parameters.items() if k != "self"}
    assert d == dict(arch="convnext_base_w", checkpoint="laion2b_s13b_b82k", output="dense", layer=-1, return_multilayer=False, add_norm=False,
                     weights=None, precision=None, init_seed=0)
    m = ConvNext(weights=_tiny_weights())
    assert m.checkpoint_name == "cnxt_b_w_laion2b_s13b_b82k" and m.patch_size == 16 and m.output == "dense"
    assert m.feat_dim == 256 and m.multilayers == [3] and m.layer == "3" and not m.v2 and len(m.batchnorms) == 4
    m = ConvNext("convnext_base", "in22k", layer=1, output="gap", weights=_tiny_weights())
    assert m.checkpoint_name == "cnxt_b_in22k" and m.feat_dim == 128 and m.multilayers == [1] and m.layer == "1"
    m = ConvNext("convnext_base", "fcmae_ft_in22k_in1k_384", return_multilayer=True, weights=_tiny_weights(True))
    assert m.checkpoint_name == "cnxt_b_fcmae_ft_in22k_in1k_384" and m.feat_dim == [64, 128, 192, 256] and m.multilayers == [0, 1, 2, 3]
    assert m.layer == "0-1-2-3" and m.v2
    m = ConvNext("convnext_base", "in22k", layer=0, weights=_tiny_weights())
    assert m.feat_dim == 64 and m.layer == "0"


def test_random_init_is_convnext_b():
    from evals.models import ConvNext

    with pytest.warns(UserWarning, match="seeded random init"):
        m = ConvNext("convnext_base", "fcmae_ft_in22k_in1k_384", return_multilayer=True)
    assert m.feat_dim == [128, 256, 512, 1024] and m.depths == [3, 3, 27, 3] and m.v2
    assert tuple(m.visual.stages._modules["2"].blocks._modules["26"].mlp.grn.weight.shape) == (2048,)


def test_refused_arguments():
    from evals.models import ConvNext
    from mvp import lib

    with pytest.raises(ValueError):
        ConvNext("convnext_base", "in1k", weights=_tiny_weights())
    with pytest.raises(ValueError):
        ConvNext("convnext_large", "in22k", weights=_tiny_weights())
    with pytest.raises(NotImplementedError, match="add_norm"):
        ConvNext("convnext_base", "in22k", add_norm=True, weights=_tiny_weights())
    with pytest.raises(AssertionError):
        ConvNext("convnext_base", "in22k", output="cls", weights=_tiny_weights())
    with pytest.raises(AssertionError):
        ConvNext("convnext_base", "in22k", layer=4, weights=_tiny_weights())
    m = ConvNext("convnext_base", "in22k", weights=_tiny_weights())
    with pytest.raises(lib.MvpError, match="no CPU fallback"):
        m(torch.zeros(1, 3, 64, 64))


def test_weights_from_the_checkpoint_directory(tmp_path, monkeypatch):
    from evals.models import ConvNext
    from mvp import convnext as cnx

    sd = _tiny_weights()
    torch.save(cnx.engine_to_timm(sd, "visual.trunk."), tmp_path / "convnext_base_w_laion2b_s13b_b82k_augreg.pth")
    torch.save(cnx.engine_to_hf(_tiny_weights(True)), tmp_path / "convnextv2_base.fcmae_ft_in22k_in1k_384.pth")
    monkeypatch.setenv("MVP_CKPT_DIR", str(tmp_path))
    m = ConvNext(checkpoint="laion2b_s13b_b82k_augreg")
    assert m.depths == [1, 1, 2, 1] and torch.equal(m.visual.stages._modules["2"].blocks._modules["1"].gamma, sd["stages.2.blocks.1.gamma"])
    m = ConvNext("convnext_base", "fcmae_ft_in22k_in1k_384")
    assert m.v2 and m.widths == [64, 128, 192, 256]


def test_choice_files_match_reference_compose_and_instantiate():
    from mvp import config

    assert sorted(REF_DIGESTS) == sorted(CHOICES)
    for name, (arch, ckpt, ckpt_name, v2) in CHOICES.items():
        node = yaml.safe_load(open(os.path.join(config.CONFIG_DIR, "backbone", name + ".yaml")))
        assert hashlib.sha256(json.dumps(node, sort_keys=True).encode()).hexdigest() == REF_DIGESTS[name], node
        for entry in ("depth_training", "spair_correspondence"):
            cfg = config.compose(entry, [f"backbone={name}"])
            assert cfg["backbone"]["_target_"] == "evals.models.convnext.ConvNext" and cfg["backbone"]["arch"] == arch
            assert cfg["backbone"]["checkpoint"] == ckpt
        model = config.instantiate(node, return_multilayer=True, weights=_tiny_weights(v2))
        assert type(model).__name__ == "ConvNext" and model.checkpoint_name == ckpt_name and model.v2 == v2
        assert model.feat_dim == [64, 128, 192, 256] and model.multilayers == [0, 1, 2, 3]


# ------------------------------------------------------------------------------------------------ C ABI
EINVAL, P = -1, 0x10000


def test_convnext_exports_abi():
    from mvp import lib

    so = lib.load()
    for sym, st, cname in (("mvp_dwconv7_ln_fwd", lib.Dwconv7LnArgs, b"mvp_dwconv7_ln_args"), ("mvp_grn_stats", lib.GrnArgs, b"mvp_grn_args"),
                           ("mvp_grn_apply", lib.GrnArgs, b"mvp_grn_args")):
        assert hasattr(so, sym) and lib.SYMBOLS[sym] is st
        assert so.mvp_sizeof(cname) == C.sizeof(st) and lib.STRUCTS[cname.decode()] is st
    assert lib.info().abi_version == 8
    header = open(os.path.join(REPO, "include", "mvp_hip.h")).read()
    assert "Added within 8: mvp_dwconv7_ln_fwd" in header and "#define MVP_ABI_VERSION 8" in header
    for n in ("mvp_dwconv7_ln_args", "mvp_grn_args"):
        assert f"struct {n} {{" in header
    # the workspace query: fp64 partial sums, one per (image, slab of >= 64 rows up to 64 slabs, channel)
    q = so.mvp_grn_workspace_bytes
    assert q(3, 2, 256) == 3 * 1 * 256 * 8 and q(3, 200, 4096) == 3 * 4 * 4096 * 8 and q(16, 3136, 512) == 16 * 49 * 512 * 8
    assert q(1, 100000, 8) == 64 * 8 * 8 and q(0, 4, 8) == 0


def test_dwconv7_ln_argument_checks():
    """Validation precedes any launch: C = 48 (not a multiple of 32), C = 4096 (beyond 2048) and H = 0 are MVP_EINVAL, as are NULL
    operands, a pixel stride below C and an unknown layout.  (No well-formed call is made here: it would launch.)"""
    from mvp import lib

    fn = lib.load().mvp_dwconv7_ln_fwd

    def code(**kw):
        a = dict(x=P, weight=P, bias=P, gamma=P, beta=P, out_hi=P, out_lo=P, B=2, H=5, W=7, C=64, ldx=64, eps=1e-6)
        a.update(kw)
        return fn(C.byref(lib.Dwconv7LnArgs(**a)), None)

    assert code(C=48, ldx=48) == EINVAL
    assert code(C=4096, ldx=4096) == EINVAL
    assert code(H=0) == EINVAL
    assert code(C=0, ldx=0) == EINVAL and code(C=16, ldx=16) == EINVAL and code(W=0) == EINVAL and code(B=0) == EINVAL and code(H=-3) == EINVAL
    assert code(ldx=32) == EINVAL and code(ldx=66) == EINVAL
    assert code(out_layout=2) == EINVAL and code(out_layout=-1) == EINVAL
    assert code(out_hi=None, out_lo=None) == EINVAL  # no output at all
    for ptr in ("x", "weight", "bias", "gamma", "beta"):
        assert code(**{ptr: None}) == EINVAL, ptr
    assert fn(None, None) == EINVAL


def test_grn_argument_checks():
    from mvp import lib

    so = lib.load()

    def args(**kw):
        a = dict(h=P, gamma=P, beta=P, G=P, N=P, out_hi=P, out_lo=P, workspace=P, workspace_bytes=1 << 30, B=3, HW=15, C4=768)
        a.update(kw)
        return C.byref(lib.GrnArgs(**a))

    for fn in (so.mvp_grn_stats, so.mvp_grn_apply):
        assert fn(args(C4=100), None) == EINVAL and fn(args(C4=0), None) == EINVAL and fn(args(HW=0), None) == EINVAL and fn(args(B=0), None) == EINVAL
        assert fn(args(h=None), None) == EINVAL and fn(args(N=None), None) == EINVAL
        assert fn(None, None) == EINVAL
    assert so.mvp_grn_stats(args(workspace_bytes=3 * 768 * 8 - 1), None) == EINVAL
    assert so.mvp_grn_stats(args(workspace=None), None) == EINVAL and so.mvp_grn_stats(args(G=None), None) == EINVAL
    assert so.mvp_grn_stats(args(workspace=P + 4), None) == EINVAL
    assert so.mvp_grn_apply(args(gamma=None), None) == EINVAL and so.mvp_grn_apply(args(out_hi=None, out_lo=None), None) == EINVAL
    assert so.mvp_grn_apply(args(out_layout=1, C4=776), None) == EINVAL and so.mvp_grn_apply(args(out_layout=2), None) == EINVAL
