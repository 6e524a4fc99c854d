"""CLIP and SigLIP backbones on the HIP path: QuickGELU / tanh-GELU through every GEMM kernel family against fp64 (same bits from each),
the in-place fp32 LayerNorm (CLIP's ln_pre), whole models through the wrappers against the transformers-built goldens and the fp64
restatement in tests/langimg_ref.py, activation outliers, grouped and pipelined forwards without a prefix row (SigLIP: n_prefix = 0),
and this project's add_norm definition."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import langimg_ref
from conftest import REPO, load_golden, rel_l2

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(REPO, "tests", "golden"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _gemm_args(ap, wp, bias, M, N, K, prec, pol, act, out_f32=None, out_pair=None, f16_col0=0):
    from mvp import lib, ops

    ilv = pol == "pp_ilv"
    ai, wi = (ops.interleave_pair(ap), ops.interleave_pair(wp)) if ilv else (None, None)
    oh, ol = out_pair if out_pair is not None else (None, None)
    a = lib.GemmArgs(lib.ptr(ai if ilv else ap[0]), None if ilv else lib.ptr(ap[1]), lib.ptr(wi if ilv else wp[0]), None if ilv else lib.ptr(wp[1]),
                     lib.ptr(bias), None, lib.ptr(out_f32), lib.ptr(oh), lib.ptr(ol), M, N, K, 2 * K if ilv else K, 2 * K if ilv else K, N, N, N,
                     act, prec, 0, 0, 0, 0)
    a.pair_layout = 3 if ilv else 0
    a.out_f16_col0 = f16_col0
    # tile: the tile kernels (universal epilogue); guarded: the row-guarded epilogue; pp: the large-M kernel (shared-chip rule: >= 96 tiles)
    a.tile_policy = {"tile": lib.TILES_NO_PP, "guarded": lib.TILES_NO_PP | lib.TILES_NO_UNI, "pp": lib.TILES_SHARED, "pp_ilv": 0}[pol]
    return a, (ai, wi)


def _pair_value(pair, f16):
    """fp64 value of a pair output: bf16 hi + lo, or the compensated fp16 activation pair (hi + (lo - hi / 8) / 8)."""
    if f16:
        hi, lo = pair[0].view(torch.float16).double(), pair[1].view(torch.float16).double()
        return hi + (lo - hi / 8) / 8
    return pair[0].double() + pair[1].double()


@pytest.mark.parametrize("prec_name", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("act_name", ["quick_gelu", "gelu_tanh"])
@pytest.mark.parametrize("shape", [(333, 3072, 768), (2000, 4096, 1024), (25000, 768, 768)])
def test_activation_gemm_vs_fp64(dev, prec_name, act_name, shape):
    """Y = act(A W^T + bias) for fc1-like shapes: a ragged tile-kernel shape, a second tile shape, a large-M shape (25000 rows = 294
    tiles of 256^2, ragged too); tile kernels (universal and row-guarded epilogues) and the large-M kernel on separate and interleaved
    operands; fp32 output and pair output (fc1's form: the bf16 pair for bf16x3, the compensated fp16 pair of out_f16_col0 = -1 for
    f16x2).  Relative L2 against fp64 under test_layerscale_gemm_vs_fp64's bound for these precisions (2e-5); the same bits from every
    kernel family; and through mvp_gemm_scaled with a unit scale the same bits again."""
    from mvp import lib, ops, vit

    M, N, K = shape
    prec = vit.parse_precision(prec_name)
    act = vit.ACTIVATIONS[act_name]
    g = torch.Generator().manual_seed(M + N + prec + act)
    a = torch.randn(M, K, generator=g).to(dev)
    w = (torch.randn(N, K, generator=g) * 2.0 * K ** -0.5).to(dev)  # pre-activations of a few units: both tails of the sigmoid
    bias = torch.randn(N, generator=g).to(dev)
    if prec == lib.PREC_F16X2:
        ap, wp = ops.split_f16_comp(a), ops.f16x2_weight(w)
    else:
        ap, wp = ops.split_bf16(a, prec), ops.split_bf16(w, prec)
    ref = langimg_ref.activation(act_name, a.double() @ w.double().t() + bias.double())
    so = lib.load()
    tol = 2e-5
    f16 = prec == lib.PREC_F16X2
    first = {}
    ones = torch.ones(N, device=dev)
    for pol in ["tile", "guarded", "pp", "pp_ilv"]:
        out = torch.full((M, N), float("nan"), device=dev)
        args, keep = _gemm_args(ap, wp, bias, M, N, K, prec, pol, act, out_f32=out)
        lib.check((so.mvp_gemm_pp if pol == "pp_ilv" else so.mvp_gemm_bias_act_res)(C.byref(args), lib.stream_ptr()), pol)
        pair = ops.empty_pair((M, N), lib.PREC_BF16X3, dev)
        args, keep2 = _gemm_args(ap, wp, bias, M, N, K, prec, pol, act, out_pair=pair, f16_col0=-1 if f16 else 0)
        lib.check((so.mvp_gemm_pp if pol == "pp_ilv" else so.mvp_gemm_bias_act_res)(C.byref(args), lib.stream_ptr()), pol)
        outs = torch.full((M, N), float("nan"), device=dev)
        args, keep3 = _gemm_args(ap, wp, bias, M, N, K, prec, pol, act, out_f32=outs)
        lib.check(so.mvp_gemm_scaled(C.byref(lib.GemmScaledArgs(args, lib.ptr(ones))), lib.stream_ptr()), pol)
        torch.cuda.synchronize()
        e32 = ((out.double() - ref).norm() / ref.norm()).item()
        epair = ((_pair_value(pair, f16) - ref).norm() / ref.norm()).item()
        print(f"\n[{act_name} gemm {prec_name} {shape} {pol}] rel-L2 vs fp64: fp32 out {e32:.2e}, pair out {epair:.2e}")
        assert e32 < tol and epair < tol, (pol, e32, epair)
        assert torch.equal(outs, out), pol
        if first:
            assert torch.equal(out, first["o"]), pol
            assert torch.equal(pair[0], first["p"][0]) and torch.equal(pair[1], first["p"][1]), pol
        else:
            first = {"o": out, "p": pair}


@pytest.mark.parametrize("act_name", ["quick_gelu", "gelu_tanh", "gelu"])
def test_activation_pointwise_error_vs_fp64(dev, act_name):
    """The activation alone: identity weights and inputs on the grid k / 2048 over [-12, 12] (15 significant bits: exact as a bf16 pair,
    so the pre-activation is the input exactly).  Bound: the sigmoid forms take five roundings — the argument product, v_exp_f32 (1 ulp),
    the add, v_rcp_f32 (1 ulp), the final product — at most 3.5 x 2^-23 relative on |y| <= 12: 5e-6 absolute.  (DESIGN.md records what is
    measured.)"""
    from mvp import ops, vit

    M = K = N = 256
    k = torch.round(torch.linspace(-24576, 24576, M * K, dtype=torch.float64))
    xs = (k / 2048).float().reshape(M, K)
    pair = ops.split_bf16(xs.to(dev))
    assert torch.equal((pair[0].float() + pair[1].float()).cpu(), xs)
    out = torch.empty(M, N, device=dev)
    ops.gemm(pair, ops.split_bf16(torch.eye(K).to(dev)), M, N, K, out_f32=out, act=vit.ACTIVATIONS[act_name], splitk=1)
    torch.cuda.synchronize()
    err = (out.double().cpu() - langimg_ref.activation(act_name, xs.double())).abs().max().item()
    print(f"\n[{act_name}] max |error| vs fp64 over [-12, 12]: {err:.2e}")
    assert err < 5e-6, err


def test_activation_gemm_refusals(dev):
    from mvp import lib

    so = lib.load()
    x = torch.zeros(64 * 64, device=dev)
    m = torch.zeros(64 * 64, dtype=torch.uint8, device=dev)
    for act in (lib.ACT_QUICK_GELU, lib.ACT_GELU_TANH):
        a = lib.GemmArgs(lib.ptr(x), lib.ptr(x), lib.ptr(x), lib.ptr(x), None, None, lib.ptr(x), None, None, 64, 64, 64, 64, 64, 64, 64, 64,
                         act, lib.PREC_BF16X3, 0, 0, 0, 0)
        a.out_mask, a.ldm = lib.ptr(m), 64
        assert so.mvp_gemm_bias_act_res(C.byref(a), None) == -1
    a = lib.GemmArgs(lib.ptr(x), lib.ptr(x), lib.ptr(x), lib.ptr(x), None, None, lib.ptr(x), None, None, 64, 64, 64, 64, 64, 64, 64, 64,
                     5, lib.PREC_BF16X3, 0, 0, 0, 0)
    assert so.mvp_gemm_bias_act_res(C.byref(a), None) == -1


@pytest.mark.parametrize("shape", [(1000, 768), (333, 1024), (64, 128)])
def test_layernorm_in_place_and_pair_path(dev, shape):
    """mvp_layernorm_fwd with out_hi = NULL and out_f32 == x against torch's layer_norm in fp64; the pair output of a run with
    out_f32 set equals the pair output of a run without it, bit for bit."""
    from mvp import lib, ops

    M, Cc = shape
    g = torch.Generator().manual_seed(M)
    x = (torch.randn(M, Cc, generator=g) * 3 + 0.5).to(dev)
    gam, bet = (1 + 0.3 * torch.randn(Cc, generator=g)).to(dev), torch.randn(Cc, generator=g).to(dev)
    ref = F.layer_norm(x.double(), (Cc,), gam.double(), bet.double(), 1e-5)
    p0, p1 = ops.empty_pair((M, Cc), lib.PREC_BF16X3, dev), ops.empty_pair((M, Cc), lib.PREC_BF16X3, dev)
    o32 = torch.empty(M, Cc, device=dev)
    ops.layernorm(x, gam, bet, p0, M, Cc, 1e-5)
    ops.layernorm(x, gam, bet, p1, M, Cc, 1e-5, out_f32=o32)
    xi = x.clone()
    ops.layernorm(xi, gam, bet, None, M, Cc, 1e-5, out_f32=xi)
    torch.cuda.synchronize()
    assert torch.equal(p0[0], p1[0]) and torch.equal(p0[1], p1[1])
    assert torch.equal(xi, o32)
    err = ((xi.double() - ref).norm() / ref.norm()).item()
    print(f"\n[layernorm in place {shape}] rel-L2 vs fp64 {err:.2e}")
    assert err < 1e-6, err


# ------------------------------------------------------------------------------------------------ whole models
def _clip(sd, dev, precision, act, patch_arch="ViT-B-16", **kw):
    from evals.models.clip import CLIP

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = CLIP(arch=patch_arch, checkpoint="openai" if act == "quick_gelu" else "other", weights=sd, precision=precision, **kw)
    return m.to(dev)


def _siglip(sd, dev, precision, act="gelu_tanh", checkpoint="vit_base_patch16_siglip_224", **kw):
    from evals.models.siglip import SigLIP

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = SigLIP(checkpoint=checkpoint, weights=sd, precision=precision, act=act, **kw)
    return m.to(dev)


def _errs(outs, refs):
    errs = []
    for o, r in zip(outs, refs):
        r = torch.as_tensor(r)
        assert tuple(o.shape) == tuple(r.shape), (o.shape, r.shape)
        errs.append(((o.double().cpu() - r.double()).norm() / r.double().norm()).item())
    return errs


@pytest.mark.parametrize("precision", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("name", ["clip_p16_quick", "clip_p14_gelu", "siglip_p16_tanh"])
def test_tiny_models_vs_goldens_and_restatement(dev, precision, name):
    """C = 128, 2 heads, depth 4, a ragged image size: every tap against the transformers-built golden and the fp64 restatement, under
    the 1e-3 feature contract."""
    import make_goldens_langimg as mg

    g = load_golden("langimg_tiny.npz")
    fam, patch, _, act, _ = mg.TINY[name]
    sd = mg.tiny_state_dict(name)
    images = torch.from_numpy(g["images"])
    for output in (("dense", "dense-cls") if fam == "clip" else ("dense",)):
        m = (_clip(sd, dev, precision, act, output=output, return_multilayer=True) if fam == "clip"
             else _siglip(sd, dev, precision, act, output=output, return_multilayer=True))
        assert m.multilayers == [0, 1, 2, 3] and m.patch_size == patch
        with torch.no_grad():
            outs = m(images.to(dev))
        eg = _errs(outs, [g[f"{name}_{output}_tap{j}"] for j in range(4)])
        ref = langimg_ref.dense_features(sd, images.double(), m.multilayers, patch=patch, act=act, eps=m.ln_eps, output=output)
        er = _errs(outs, ref)
        print(f"\n[{name} {output} {precision}] rel-L2 per tap vs golden: " + " ".join(f"{e:.2e}" for e in eg) + " | vs fp64 restatement: " + " ".join(f"{e:.2e}" for e in er))
        assert max(eg) < 1e-3 and max(er) < 1e-3, (eg, er)


def _full_cases():
    import make_goldens_langimg as mg

    return [(key, shape) for key, v in mg.FULL.items() for shape in v[4]]


@pytest.mark.parametrize("precision", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("key,shape", _full_cases())
def test_full_size_models_vs_sampled_goldens(dev, precision, key, shape):
    import make_goldens_langimg as mg

    g = load_golden("langimg_full_sampled.npz")
    fam, arch, act, _, _ = mg.FULL[key]
    sd, patch = mg.full_state_dict(key)
    B, H, W = shape
    m = (_clip(sd, dev, precision, act, patch_arch=arch, return_multilayer=True) if fam == "clip"
         else _siglip(sd, dev, precision, act, checkpoint=arch, return_multilayer=True))
    with torch.no_grad():
        outs = m(mg.full_images(B, H, W).to(dev))
    errs = []
    for j, o in enumerate(outs):
        tag = f"{key}_{B}x{H}x{W}_tap{j}"
        assert tuple(o.shape) == tuple(g[tag + "_shape"]), tag
        errs.append(rel_l2(o.cpu().numpy().reshape(-1)[mg.sample_index(o.numel())], g[tag]))
    print(f"\n[{key} {precision} {shape}] rel-L2 per tap vs sampled golden: " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < 1e-3, errs


def test_clip_with_activation_outliers_vs_restatement(dev):
    """Large ln_pre gains on a few channels (trained CLIP models carry large-magnitude channels in the residual stream): bf16x3 and
    f16x2 against the fp64 restatement, and the f16x2 range check stays silent."""
    from mvp import backbone as bb

    sd = bb.clip_to_engine(bb.random_clip_state_dict(768, 12, 16, 224, seed=41))
    sd["norm_pre.weight"][[7, 300]] = 60.0
    sd["norm_pre.bias"][[7, 300]] = 5.0
    images = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(3))
    ref = langimg_ref.dense_features(sd, images.double(), [2, 5, 8, 11], patch=16, act="quick_gelu", eps=1e-5)
    for precision in ("bf16x3", "f16x2"):
        m = _clip(sd, dev, precision, "quick_gelu", return_multilayer=True)
        m.engine().check_f16_range = True
        with torch.no_grad():
            outs = m(images.to(dev))
        errs = _errs(outs, ref)
        print(f"\n[clip outliers {precision}] rel-L2 per tap vs fp64 restatement: " + " ".join(f"{e:.2e}" for e in errs))
        assert max(errs) < 1e-3, errs


@pytest.mark.parametrize("fam", ["clip", "siglip"])
def test_grouped_forward_equals_single_batches(dev, fam):
    """Two batches stacked into one forward (the large-M kernel's QuickGELU / tanh-GELU instantiations, interleaved operands) give each
    batch exactly the bits of its own forward (tile kernels); SigLIP: no prefix row."""
    from mvp import backbone as bb

    if fam == "clip":
        m = _clip(bb.random_clip_state_dict(768, 12, 16, 224, seed=4), dev, "f16x2", "quick_gelu", return_multilayer=True)
    else:
        m = _siglip(bb.random_siglip_state_dict(768, 12, 16, 224, seed=4), dev, "f16x2", return_multilayer=True)
    eng = m.engine()
    assert eng.n_prefix == (1 if fam == "clip" else 0)
    imgs = torch.randn(32, 3, 224, 224, generator=torch.Generator().manual_seed(9)).to(dev)
    cls = fam == "clip"
    with torch.no_grad():
        grouped = eng.forward_taps(imgs, m.multilayers, bn=None, bn_mode=2, pack=False, want_cls=cls, groups=2)
        for gidx in range(2):
            single = eng.forward_taps(imgs[16 * gidx:16 * (gidx + 1)].contiguous(), m.multilayers, bn=None, bn_mode=2, pack=False, want_cls=cls)
            for a, b in zip(grouped[gidx], single):
                assert torch.equal(a, b), gidx
            for a, b in zip(grouped[gidx].cls, single.cls):
                assert torch.equal(a, b), gidx


def test_siglip_refuses_cls(dev):
    from mvp import backbone as bb, lib

    m = _siglip(bb.random_siglip_state_dict(128, 4, 16, 64, seed=1), dev, "bf16x3", return_multilayer=True)
    with pytest.raises(lib.MvpError, match="no CLS token"):
        m.engine().forward_taps(torch.randn(1, 3, 64, 64, device=dev), m.multilayers, bn=None, bn_mode=2, want_cls=True)


def _build(dev, sd, precision="f16x2"):
    from evals.models.probes import DepthHead
    from evals.utils.optim import cosine_decay_linear_warmup
    from mvp.optim import FlatAdamW

    model = _siglip(sd, dev, precision, return_multilayer=True, add_norm=True)
    torch.manual_seed(11)
    probe = DepthHead(feat_dim=model.feat_dim, head_type="linear", kernel_size=1, prediction_type="bindepth", min_depth=0.001, max_depth=10).to(dev)
    opt = FlatAdamW([{"params": probe.parameters(), "lr": 1e-3}])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda e: cosine_decay_linear_warmup(e, 100, 10))
    return model, probe, opt, sched


def test_siglip_span_pipeline_with_graphs_is_bit_identical_to_serial(dev):
    """SigLIP B/16 (no prefix row: 196 rows per image), B = 16 at 224^2: forwards over spans of 24 images with graph replay and grouped
    tap BN — losses, probe weights, AdamW state and tap-BN running statistics equal the one-batch-at-a-time loop's bit for bit."""
    from evals.utils.losses import DepthLoss
    from mvp import backbone as bb
    from mvp.pipeline import FeaturePipeline, pipelined_features, rows_per_image
    from mvp.train import train_depth_step

    sd = bb.random_siglip_state_dict(768, 12, 16, 224, seed=13)
    n, B, span = 5, 16, 24
    bs = []
    for s in range(n):
        g = torch.Generator().manual_seed(700 + s)
        bs.append({"image": torch.randn(B, 3, 224, 224, generator=g).to(dev), "depth": (torch.rand(B, 1, 224, 224, generator=g) * 9.0 + 0.05).to(dev)})
    loss_fn = DepthLoss()

    def state(model, opt, losses):
        torch.cuda.synchronize()
        bn = [torch.cat([b.running_mean, b.running_var]).cpu().numpy() for b in model.batchnorms]
        return (torch.stack(losses).cpu().numpy(), opt.flat_param.cpu().numpy().copy(), opt.exp_avg_sq.cpu().numpy().copy(), bn,
                [int(b.num_batches_tracked) for b in model.batchnorms])

    model, probe, opt, sched = _build(dev, sd)
    assert model.n_prefix == 0 and rows_per_image(224, 224, 16, 0) == 196
    losses = [train_depth_step(model, probe, opt, sched, loss_fn, b["image"], b["depth"].clone()) for b in bs]
    ref = state(model, opt, losses)

    model, probe, opt, sched = _build(dev, sd)
    pipe = FeaturePipeline(model, 2, graphs=True, group=2, span=span)
    losses = []
    for b, f in pipelined_features(model, bs, pipe=pipe):
        losses.append(train_depth_step(model, probe, opt, sched, loss_fn, None, b["depth"].clone(), feats=f))
    assert pipe.span == span and all(e["graph"] is not None for e in pipe._graphs.values())
    got = state(model, opt, losses)
    for i in range(3):
        np.testing.assert_array_equal(got[i], ref[i])
    for a, b in zip(got[3], ref[3]):
        np.testing.assert_array_equal(a, b)
    assert got[4] == ref[4] == [n] * 4


@pytest.mark.parametrize("fam", ["clip", "siglip"])
def test_add_norm_train_mode_vs_restatement(dev, fam):
    """add_norm=True: train-mode per-channel BatchNorm1d over all tokens of the batch at each tap — outputs and the
    updated running statistics against the fp64 restatement."""
    import make_goldens_langimg as mg

    name = "clip_p16_quick" if fam == "clip" else "siglip_p16_tanh"
    _, patch, _, act, _ = mg.TINY[name]
    sd = mg.tiny_state_dict(name)
    images = mg.tiny_images()
    m = (_clip(sd, dev, "bf16x3", act, return_multilayer=True, add_norm=True) if fam == "clip"
         else _siglip(sd, dev, "bf16x3", act, return_multilayer=True, add_norm=True))
    m.train()
    g = torch.Generator().manual_seed(8)
    aff = []
    for bn in m.batchnorms:
        bn.weight.data.copy_((1 + 0.2 * torch.randn(128, generator=g)).to(dev))
        bn.bias.data.copy_((0.1 * torch.randn(128, generator=g)).to(dev))
        aff.append((bn.weight.detach().double().cpu(), bn.bias.detach().double().cpu()))
    with torch.no_grad():
        outs = m(images.to(dev))
    kw = dict(patch=patch, act=act, eps=m.ln_eps)
    ref = langimg_ref.dense_features(sd, images.double(), m.multilayers, add_norm=True, bn_affine=aff, **kw)
    errs = _errs(outs, ref)
    print(f"\n[{fam} add_norm train] rel-L2 per tap vs fp64 restatement: " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < 1e-3, errs
    toks = langimg_ref.dense_features(sd, images.double(), m.multilayers, return_tokens=True, **kw)
    for bn, t in zip(m.batchnorms, toks):
        flat = t.reshape(-1, t.shape[-1])
        mean, var = flat.mean(0), flat.var(0, unbiased=True)
        assert rel_l2(bn.running_mean.cpu().numpy(), (0.1 * mean).numpy()) < 1e-3
        assert rel_l2(bn.running_var.cpu().numpy(), (0.9 + 0.1 * var).numpy()) < 1e-3
        assert int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("name", ["clip_b16", "clip_b16_laion", "clip_l14", "siglip_b16", "siglip_l16"])
def test_choice_file_builds_a_model_whose_linear_probe_step_trains(dev, name):
    """``backbone=<name>`` composed into depth_training, instantiated with return_multilayer (train_depth.py:564-567), two steps of the
    linear depth probe through mvp.train at 224^2: finite losses, the second lower than the first on the same batch, weights moved."""
    from evals.models.probes import DepthHead
    from evals.utils.losses import DepthLoss
    from mvp import config
    from mvp.optim import FlatAdamW
    from mvp.train import train_depth_step

    cfg = config.compose("depth_training", [f"backbone={name}"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = config.instantiate(cfg["backbone"], return_multilayer=True).to(dev)
    torch.manual_seed(3)
    probe = DepthHead(feat_dim=model.feat_dim, head_type="linear", kernel_size=1, prediction_type="bindepth", min_depth=0.001, max_depth=10).to(dev)
    opt = FlatAdamW([{"params": probe.parameters(), "lr": 1e-3}])
    g = torch.Generator().manual_seed(1)
    img = torch.randn(4, 3, 224, 224, generator=g).to(dev)
    tgt = (torch.rand(4, 1, 224, 224, generator=g) * 9.0 + 0.05).to(dev)
    w0 = probe.head.conv.weight.detach().clone()
    losses = [train_depth_step(model, probe, opt, None, DepthLoss(), img, tgt.clone()).item() for _ in range(2)]
    print(f"\n[{name}] linear-probe losses: {losses[0]:.5f} -> {losses[1]:.5f}")
    assert all(np.isfinite(losses)) and losses[1] < losses[0], losses
    assert not torch.equal(probe.head.conv.weight.detach(), w0)
    assert model.add_norm == bool(cfg["backbone"].get("add_norm", False))
