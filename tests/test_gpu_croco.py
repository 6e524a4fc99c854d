"""CroCo and CroCo v2 backbones on the HIP path: the 2-D RoPE kernel (mvp_rope2d_qkv) against the qkv GEMM's own pair output (identity
tables: bit for bit) and against fp64 per element in every output form, its refusals; whole models through the wrappers against the
goldens built from the reference's CroCoNet and the fp64 restatement in tests/croco_ref.py; grouped, span-pipelined and graph-replayed
forwards; the two choice files."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest
import torch

import croco_ref
from conftest import REPO, load_golden, rel_l2

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

# (precision of the qkv GEMM, v_format) -> the GEMM's out_f16_col0 for C' = 2 * H * 64
FORMS = [("bf16x3", 0), ("bf16x3", 1), ("f16x2", 2)]
H, GH, GW = 2, 3, 5
C3 = 3 * H * 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _decode(pair, v_format):
    """fp64 value of every column of a [M, 3 * H * 64] pair in the forms of ``v_format`` (as _pair_value in test_gpu_langimg.py, per third):
    bf16 pair hi + lo; V under v_format >= 1: fp16 hi + bf16 lo; Q under 2: the compensated activation pair hi + (lo - hi / 8) / 8; K under 2:
    the compensated weight-side pair hi + lo / 8 (fp16 halves)."""
    hi, lo = pair[0][:, :C3], pair[1][:, :C3]
    bb_ = hi.double() + lo.double()
    h16, l16 = hi.view(torch.float16).double(), lo.view(torch.float16).double()
    out = bb_.clone()
    Cq = H * 64
    if v_format >= 1:
        out[:, 2 * Cq:] = h16[:, 2 * Cq:] + lo.double()[:, 2 * Cq:]
    if v_format == 2:
        out[:, :Cq] = h16[:, :Cq] + (l16[:, :Cq] - h16[:, :Cq] / 8) / 8
        out[:, Cq:2 * Cq] = h16[:, Cq:2 * Cq] + l16[:, Cq:2 * Cq] / 8
    return out


def _tables(dev, rows, identity=False):
    if identity:
        return torch.ones(rows, 32, device=dev), torch.zeros(rows, 32, device=dev)
    cos, sin = croco_ref.rope_tables(100.0, rows, torch.float32)
    return cos.contiguous().to(dev), sin.contiguous().to(dev)


def _rope(qkv, out, tabs, N, n_prefix, gh, gw, v_format, ld_out=None):
    from mvp import lib, ops

    ops.rope2d_qkv(qkv, out, tabs[0], tabs[1], qkv.shape[0], N, H, n_prefix, gh, gw, lib.PREC_BF16X3, v_f16=v_format >= 1, qk_f16=v_format == 2, ld_out=ld_out)


@pytest.mark.parametrize("n_prefix", [0, 1])
@pytest.mark.parametrize("prec_name,v_format", FORMS)
def test_rope_identity_tables_reproduce_the_gemm_pair_bit_for_bit(dev, prec_name, v_format, n_prefix):
    """cos = 1, sin = 0: the kernel's pair output is the pair the qkv GEMM writes from the same operands with the matching out_f16_col0 —
    one definition of each 16-bit form.  The fp32 input is the same GEMM's out_f32."""
    from mvp import lib, ops, vit

    B, K = 2, 128
    N = n_prefix + GH * GW
    M = B * N
    prec = vit.parse_precision(prec_name)
    g = torch.Generator().manual_seed(100 + v_format + n_prefix)
    a = torch.randn(M, K, generator=g).to(dev)
    w = (torch.randn(C3, K, generator=g) * K ** -0.5).to(dev)
    bias = torch.randn(C3, generator=g).to(dev)
    ap, wp = (ops.split_f16_comp(a), ops.f16x2_weight(w)) if prec == lib.PREC_F16X2 else (ops.split_bf16(a, prec), ops.split_bf16(w, prec))
    col0 = {0: 0, 1: 2 * H * 64, 2: -2 * H * 64}[v_format]
    want = ops.empty_pair((M, C3), lib.PREC_BF16X3, dev)
    f32 = torch.empty(M, C3, device=dev)
    ops.gemm(ap, wp, M, C3, K, bias=bias, out=want, precision=prec, f16_col0=col0)
    ops.gemm(ap, wp, M, C3, K, bias=bias, out_f32=f32, precision=prec)
    got = ops.empty_pair((M, C3), lib.PREC_BF16X3, dev)
    _rope(f32, got, _tables(dev, max(GH, GW), identity=True), N, n_prefix, GH, GW, v_format)
    torch.cuda.synchronize()
    assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16)) and torch.equal(got[1].view(torch.int16), want[1].view(torch.int16))
    assert (_decode(got, v_format) - f32.double()).abs().max().item() < 1e-3  # (and the GEMM really wrote those forms)


@pytest.mark.parametrize("n_prefix", [0, 1])
@pytest.mark.parametrize("pad", [0, 64])
@pytest.mark.parametrize("v_format", [0, 1, 2])
def test_rope_rotation_vs_fp64_per_element(dev, v_format, pad, n_prefix):
    """RoPE100 tables on a 3 x 5 grid, B = 2, H = 2, every output form, dense rows and ld_out > 3C.  Per element
        |decoded - exact| <= 2^-16 |exact| + 2^-22 (|a| + |b|) + 2^-24,   a, b the two inputs of that rotation:
    derived, not measured — the three forms are documented at <= 2^-17 relative (include/mvp_hip.h), the fp32 rotation (two products, one
    sum) costs a few ulp of |a| + |b|, the absolute term covers fp16 lo halves below the normal range when the rotation cancels.
    Prefix rows and the V third equal the identity-table run bit for bit (not rotated); swapping gh and gw changes Q and K."""
    from mvp import lib, ops

    B = 2
    N = n_prefix + GH * GW
    M = B * N
    g = torch.Generator().manual_seed(7 + v_format + pad + n_prefix)
    qkv = (torch.randn(M, C3, generator=g) * 2.0).to(dev)
    ld = C3 + pad
    tabs = _tables(dev, max(GH, GW))

    def run(t, gh, gw):
        out = (torch.full((M, ld), 7.0, dtype=torch.bfloat16, device=dev), torch.full((M, ld), 7.0, dtype=torch.bfloat16, device=dev))
        _rope(qkv, out, t, N, n_prefix, gh, gw, v_format, ld_out=ld)
        return out

    got, ident, swapped = run(tabs, GH, GW), run(_tables(dev, max(GH, GW), identity=True), GH, GW), run(tabs, GW, GH)
    torch.cuda.synchronize()
    for o in got:
        assert torch.equal(o[:, C3:], torch.full((M, pad), 7.0, dtype=torch.bfloat16, device=dev))  # the padding columns stay untouched
    # exact rotation in fp64 from the fp32 inputs and tables
    x = qkv.double().cpu().reshape(B, N, 3, H, 2, 2, 16)  # [.., which, head, axis (y | x), half (d < 16 | d >= 16), 16]
    cos, sin = tabs[0].double().cpu(), tabs[1].double().cpu()
    p = torch.arange(GH * GW)
    pos = torch.stack((p // GW, p % GW), dim=1)  # [hw, 2]: (y, x)
    c = cos[pos].reshape(GH * GW, 2, 2, 16)[None, :, None, None]  # [1, hw, 1, 1, axis, half, 16]
    s = sin[pos].reshape(GH * GW, 2, 2, 16)[None, :, None, None]
    exact, other = x.clone(), torch.zeros_like(x)
    t = x[:, n_prefix:, :2]
    partner = torch.stack((-t[..., 1, :], t[..., 0, :]), dim=-2)  # rotate_half
    exact[:, n_prefix:, :2] = t * c + partner * s
    other[:, n_prefix:, :2] = partner.abs()
    exact, a_abs, b_abs = exact.reshape(M, C3), x.abs().reshape(M, C3), other.reshape(M, C3)
    dec = _decode(got, v_format).cpu()
    bound = 2.0 ** -16 * exact.abs() + 2.0 ** -22 * (a_abs + b_abs) + 2.0 ** -24
    ratio = ((dec - exact).abs() / bound).max().item()
    print(f"\n[rope2d v_format={v_format} ld_out={ld} n_prefix={n_prefix}] max |decoded - exact| / bound = {ratio:.3f}")
    assert ratio <= 1.0, ratio
    rows = torch.arange(M).reshape(B, N)
    pre, grid = rows[:, :n_prefix].reshape(-1).to(dev), rows[:, n_prefix:].reshape(-1).to(dev)
    Cq = H * 64
    for k in range(2):
        gi, ii, si = got[k].view(torch.int16), ident[k].view(torch.int16), swapped[k].view(torch.int16)
        assert torch.equal(gi[pre], ii[pre])  # prefix rows: not rotated
        assert torch.equal(gi[:, 2 * Cq:C3], ii[:, 2 * Cq:C3]) and torch.equal(si[:, 2 * Cq:C3], ii[:, 2 * Cq:C3])  # V untouched
    assert not torch.equal(got[0][grid][:, :2 * Cq], ident[0][grid][:, :2 * Cq])  # (the rotation acts)
    assert not torch.equal(got[0][grid][:, :2 * Cq], swapped[0][grid][:, :2 * Cq])  # the axis order: 3 x 5 is not 5 x 3
    # token 1 of the grid sits at (y, x) = (0, 1): its y halves (angle 0) pass through, its x halves do not
    r1 = int(grid[1])
    ycols = torch.arange(2 * Cq).reshape(-1, 2, 32)[:, 0].reshape(-1).to(dev)
    assert torch.equal(got[0][r1, ycols].view(torch.int16), ident[0][r1, ycols].view(torch.int16))


def test_rope_refusals_launch_nothing(dev):
    """Every MVP_EINVAL case of include/mvp_hip.h with real device buffers: refused on the host, the output keeps its fill."""
    from mvp import lib

    so = lib.load()
    N, M = 1 + GH * GW, 2 * (1 + GH * GW)
    qkv = torch.zeros(M + 1, C3 + 8, device=dev)
    hi, lo = (torch.full((M + 1, C3 + 8), 3.0, dtype=torch.bfloat16, device=dev) for _ in range(2))
    cos, sin = _tables(dev, 8)
    p = lib.ptr

    def args(**kw):
        a = lib.Rope2dQkvArgs(p(qkv), p(hi), p(lo), p(cos), p(sin), M, N, H, 1, GH, GW, 8, C3, C3, lib.PREC_BF16X3, 0)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    bad = [dict(qkv=None), dict(out_hi=None), dict(out_lo=None), dict(cos_tab=None), dict(sin_tab=None), dict(M=M + 1), dict(N=N + 1, M=2 * (N + 1)),
           dict(n_prefix=0), dict(tab_rows=4), dict(gh=GW, gw=GH, tab_rows=4), dict(ld_in=C3 - 4), dict(ld_out=C3 - 8), dict(ld_in=C3 + 2), dict(ld_out=C3 + 4),
           dict(qkv=p(qkv) + 4), dict(out_hi=p(hi) + 8), dict(out_lo=p(lo) + 2), dict(cos_tab=p(cos) + 4), dict(sin_tab=p(sin) + 8),
           dict(precision=lib.PREC_BF16, v_format=1), dict(precision=lib.PREC_BF16, v_format=2), dict(precision=lib.PREC_F16X2), dict(v_format=3), dict(v_format=-1)]
    for kw in bad:
        assert so.mvp_rope2d_qkv(C.byref(args(**kw)), lib.stream_ptr()) == -1, kw
    assert so.mvp_rope2d_qkv(None, lib.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert bool((hi == 3.0).all()) and bool((lo == 3.0).all())


# ------------------------------------------------------------------------------------------------ whole models
def _model(name, sd, dev, precision, **kw):
    from evals.models.croco import CROCO
    from evals.models.crocov2 import CROCOV2

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = (CROCOV2 if name.startswith("crocov2") else CROCO)(weights=sd, precision=precision, **kw)
    return m.to(dev)


def _errs(outs, refs):
    errs = []
    for o, r in zip(outs, refs):
        r = torch.as_tensor(r)
        assert tuple(o.shape) == tuple(r.shape), (o.shape, r.shape)
        errs.append(((o.double().cpu() - r.double()).norm() / r.double().norm()).item())
    return errs


@pytest.mark.parametrize("add_norm", [False, True])
@pytest.mark.parametrize("precision", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("name", ["croco", "crocov2"])
def test_tiny_models_vs_goldens_and_restatement(dev, name, precision, add_norm):
    """C = 128, 2 heads, depth 4, images [2, 3, 80, 112] resized to the model's 64 x 96 (a 4 x 6 grid): every tap against the golden built
    from the reference's CroCoNet and against the fp64 restatement, under the 1e-3 feature contract; add_norm = train-mode BatchNorm1d
    over all B * N tokens."""
    import make_goldens_croco as mg
    from mvp import backbone as bb

    g = load_golden("croco_tiny.npz")
    ckpt = mg.tiny_state_dict(name)
    images = torch.from_numpy(g["images"])
    m = _model(name, ckpt, dev, precision, return_multilayer=True, add_norm=add_norm)
    m.train()
    assert m.multilayers == [0, 1, 2, 3] and m.img_size == (64, 96) and (m.rope_freq == 100.0) == (name == "crocov2")
    with torch.no_grad():
        outs = m(images.to(dev))
    assert m.engine().n_prefix == 0 and (m.engine().pos_embed is None) == (name == "crocov2")
    eg = _errs(outs, [g[f"{name}_{'norm' if add_norm else 'dense'}_tap{j}"] for j in range(4)])
    ref = croco_ref.dense_features(bb.croco_to_engine(ckpt), images.double(), m.multilayers, pos_embed=mg.TINY[name][0], img_size=m.img_size, add_norm=add_norm)
    er = _errs(outs, ref)
    print(f"\n[{name} {precision} add_norm={add_norm}] rel-L2 per tap vs golden: " + " ".join(f"{e:.2e}" for e in eg) + " | vs fp64 restatement: " + " ".join(f"{e:.2e}" for e in er))
    assert max(eg) < 1e-3 and max(er) < 1e-3, (eg, er)


def test_return_cls_is_the_first_patch_token(dev):
    """croco.py:175-176: ``embeds[0][:, 0]`` of the single tap — there is no class token."""
    import make_goldens_croco as mg

    g = load_golden("croco_tiny.npz")
    m = _model("crocov2", mg.tiny_state_dict("crocov2"), dev, "bf16x3", return_cls=True)
    with torch.no_grad():
        out = m(torch.from_numpy(g["images"]).to(dev))
    assert tuple(out.shape) == (2, 128) and m.multilayers == [3]
    assert rel_l2(out.cpu().numpy(), g["crocov2_dense_tap3"][:, :, 0, 0]) < 1e-3


@pytest.mark.parametrize("precision", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("key", ["croco_b16", "crocov2_b16"])
def test_full_size_models_vs_sampled_goldens(dev, key, precision):
    import make_goldens_croco as mg

    g = load_golden("croco_full_sampled.npz")
    B, Hh, Ww = mg.FULL_SHAPE
    m = _model(key, mg.full_state_dict(key), dev, precision, return_multilayer=True)
    with torch.no_grad():
        outs = m(mg.full_images().to(dev))
    errs = []
    for j, o in enumerate(outs):
        tag = f"{key}_{B}x{Hh}x{Ww}_tap{j}"
        assert tuple(o.shape) == tuple(g[tag + "_shape"]), tag
        errs.append(rel_l2(o.cpu().numpy().reshape(-1)[mg.sample_index(o.numel())], g[tag]))
    print(f"\n[{key} {precision}] rel-L2 per tap vs sampled golden: " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < 1e-3, errs


@pytest.mark.parametrize("name", ["croco", "crocov2"])
def test_grouped_forward_equals_single_batches(dev, name):
    """Two batches of 16 stacked into one forward (the large-M GEMM kernel, the rotation over 6272 rows) give each batch exactly the bits
    of its own forward (tile kernels, 3136 rows)."""
    from mvp import backbone as bb

    m = _model(name, bb.random_croco_state_dict(768, 12, 16, 224, pos_embed="RoPE100" if name == "crocov2" else "cosine", seed=4), dev, "f16x2",
               return_multilayer=True)
    eng = m.engine()
    assert eng.n_prefix == 0 and (eng.rope_freq == 100.0) == (name == "crocov2")
    imgs = torch.randn(32, 3, 224, 224, generator=torch.Generator().manual_seed(9)).to(dev)
    with torch.no_grad():
        grouped = eng.forward_taps(imgs, m.multilayers, bn=None, bn_mode=2, pack=False, groups=2)
        for gidx in range(2):
            single = eng.forward_taps(imgs[16 * gidx:16 * (gidx + 1)].contiguous(), m.multilayers, bn=None, bn_mode=2, pack=False)
            for a, b in zip(grouped[gidx], single):
                assert torch.equal(a, b), gidx


def _build(dev, sd, precision="f16x2"):
    from evals.models.probes import DepthHead
    from evals.utils.optim import cosine_decay_linear_warmup
    from mvp.optim import FlatAdamW

    model = _model("crocov2", sd, dev, precision, return_multilayer=True, add_norm=True)
    torch.manual_seed(11)
    probe = DepthHead(feat_dim=model.feat_dim, head_type="linear", kernel_size=1, prediction_type="bindepth", min_depth=0.001, max_depth=10).to(dev)
    opt = FlatAdamW([{"params": probe.parameters(), "lr": 1e-3}])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda e: cosine_decay_linear_warmup(e, 100, 10))
    return model, probe, opt, sched


def test_crocov2_span_pipeline_with_graphs_is_bit_identical_to_serial(dev):
    """CroCo v2 B/16 (196 rows per image, RoPE in every block), B = 16 at 224^2: forwards over spans of 24 images with graph replay and
    grouped tap BN — losses, probe weights, AdamW state and tap-BN running statistics equal the one-batch-at-a-time loop's bit for bit."""
    from evals.utils.losses import DepthLoss
    from mvp import backbone as bb
    from mvp.pipeline import FeaturePipeline, pipelined_features
    from mvp.train import train_depth_step

    sd = bb.random_croco_state_dict(768, 12, 16, 224, pos_embed="RoPE100", seed=13)
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
    losses = [train_depth_step(model, probe, opt, sched, loss_fn, b["image"], b["depth"].clone()) for b in bs]
    ref = state(model, opt, losses)

    model, probe, opt, sched = _build(dev, sd)
    pipe = FeaturePipeline(model, 2, graphs=True, group=2, span=span)
    losses = []
    for b, f in pipelined_features(model, bs, pipe=pipe):
        losses.append(train_depth_step(model, probe, opt, sched, loss_fn, None, b["depth"].clone(), feats=f))
    assert pipe.span == span and all(e["graph"] is not None for e in pipe._graphs.values())
    assert model.engine().rope_freq == 100.0 and model.engine()._rope
    got = state(model, opt, losses)
    for i in range(3):
        np.testing.assert_array_equal(got[i], ref[i])
    for a, b in zip(got[3], ref[3]):
        np.testing.assert_array_equal(a, b)
    assert got[4] == ref[4] == [n] * 4


@pytest.mark.parametrize("name", ["croco_b16", "crocov2_b16"])
def test_choice_file_builds_a_model_whose_linear_probe_step_trains(dev, name):
    """``backbone=<name>`` composed into depth_training, instantiated with return_multilayer (train_depth.py:564-567), two steps of the
    linear depth probe through mvp.train at 224^2: finite losses, the second lower than the first on the same batch, weights moved.

    The learning rate is 1e-5, not the 1e-3 of the language-image test.  AdamW's first step moves every weight by lr against its gradient's
    sign, which lowers the loss to first order by lr * |grad|_1; that is only a guarantee while the step stays in the linear regime.  A
    logit moves by at most lr * |x|_1, and |x|_1 is about 0.8 * 3072 for these tap-normalised features (unit variance, 4 x 768 channels):
    2.5 at 1e-3, far outside it, 0.025 at 1e-5, inside it.  The reference's own CroCoNet, DepthHead, DepthLoss and torch.optim.AdamW on
    the CPU, same seeds and batch, give 9.55349 -> 9.58610 (up) at 1e-3 and 9.55349 -> 9.55243 at 1e-5 for croco_b16, 9.55213 -> 9.55130
    at 1e-5 for crocov2_b16: the expected drop of 1e-4 relative is a hundred times the fp32 rounding of the loss."""
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
    opt = FlatAdamW([{"params": probe.parameters(), "lr": 1e-5}])
    g = torch.Generator().manual_seed(1)
    img = torch.randn(4, 3, 224, 224, generator=g).to(dev)
    tgt = (torch.rand(4, 1, 224, 224, generator=g) * 9.0 + 0.05).to(dev)
    w0 = probe.head.conv.weight.detach().clone()
    losses = [train_depth_step(model, probe, opt, None, DepthLoss(), img, tgt.clone()).item() for _ in range(2)]
    print(f"\n[{name}] linear-probe losses: {losses[0]:.5f} -> {losses[1]:.5f}")
    assert all(np.isfinite(losses)) and losses[1] < losses[0], losses
    assert not torch.equal(probe.head.conv.weight.detach(), w0)
    assert model.add_norm is True and (model.rope_freq == 100.0) == (name == "crocov2_b16")
