"""DINOv2 backbones (ViT-B/14, B/14 with registers, L/14) on the HIP path: the LayerScale GEMM epilogue (mvp_gemm_scaled) of every
kernel family against fp64, the padded patch gather (mvp_patch_gather_ld) against conv2d, the prefix rows (mvp_prefix_rows), and whole
models through the DINO wrapper against the fp64 restatement in tests/dinov2_ref.py."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import dinov2_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _operands(a, w, prec):
    from mvp import lib, ops

    if prec == lib.PREC_F16X2:
        return ops.split_f16_comp(a), ops.f16x2_weight(w)
    return ops.split_bf16(a, prec), ops.split_bf16(w, prec)


def _args(ap, wp, bias, res, out, M, N, K, prec, pol):
    from mvp import lib, ops

    ilv = pol == "pp_ilv"
    ai, wi = (ops.interleave_pair(ap), ops.interleave_pair(wp)) if ilv else (None, None)
    a = lib.GemmArgs(lib.ptr(ai if ilv else ap[0]), None if ilv else lib.ptr(ap[1]), lib.ptr(wi if ilv else wp[0]), None if ilv else lib.ptr(wp[1]),
                     lib.ptr(bias), lib.ptr(res), lib.ptr(out), None, None, M, N, K, 2 * K if ilv else K, 2 * K if ilv else K, N, N, N,
                     lib.ACT_NONE, prec, 0, 0, 0, 0)
    a.pair_layout = 3 if ilv else 0
    # tile: the tile kernels (universal epilogue); guarded: the row-guarded epilogue; pp: the large-M kernel (shared-chip rule: >= 96 tiles)
    a.tile_policy = {"tile": lib.TILES_NO_PP, "guarded": lib.TILES_NO_PP | lib.TILES_NO_UNI, "pp": lib.TILES_SHARED, "pp_ilv": 0}[pol]
    return a, (ai, wi)


@pytest.mark.parametrize("prec_name", ["bf16x3", "f16x2", "bf16"])
@pytest.mark.parametrize("shape", [(333, 768, 768), (2000, 1024, 4096), (25000, 768, 768)])
def test_layerscale_gemm_vs_fp64(dev, prec_name, shape):
    """Y = gamma * (A W^T + bias) (+ residual) for the proj / fc2 shapes of B/14 and L/14: tile kernels (universal and row-guarded
    epilogues), the large-M kernel on separate and interleaved operands (25000 rows = 294 tiles of 256^2: two rounds of the persistent
    tile loop), ragged M.  gamma log-uniform over [1e-6, 2]: per-column relative error against fp64; every kernel family gives the same bits;
    gamma = 1 gives exactly the bits of the unscaled GEMM."""
    from mvp import lib, vit

    M, N, K = shape
    prec = vit.parse_precision(prec_name)
    g = torch.Generator().manual_seed(M + N + prec)
    a = torch.randn(M, K, generator=g).to(dev)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(dev)
    bias, res = torch.randn(N, generator=g).to(dev), torch.randn(M, N, generator=g).to(dev)
    gamma = torch.exp(torch.empty(N).uniform_(math.log(1e-6), math.log(2.0), generator=g)).to(dev)
    ones = torch.ones(N, device=dev)
    ap, wp = _operands(a, w, prec)
    ref = (a.double() @ w.double().t() + bias.double()) * gamma.double()
    so = lib.load()
    tol = 1e-2 if prec == lib.PREC_BF16 else 2e-5
    pols = ["tile", "guarded"] + ([] if prec == lib.PREC_BF16 else ["pp", "pp_ilv"])
    first = {}
    for pol in pols:
        for use_res in (False, True):
            out = torch.full((M, N), float("nan"), device=dev)
            args, keep = _args(ap, wp, bias, res if use_res else None, out, M, N, K, prec, pol)
            lib.check(so.mvp_gemm_scaled(C.byref(lib.GemmScaledArgs(args, lib.ptr(gamma))), lib.stream_ptr()), pol)
            torch.cuda.synchronize()
            r = ref + res.double() if use_res else ref
            if use_res:
                err = ((out.double() - r).norm() / r.norm()).item()
            else:  # per column: a tiny gamma must not hide a wrong column
                err = (((out.double() - r).norm(dim=0) / r.norm(dim=0)).square().mean().sqrt()).item()
            if pol == "tile":
                print(f"\n[layerscale gemm {prec_name} {shape} residual={use_res}] rel err vs fp64: {err:.2e}")
            assert err < tol, (pol, use_res, err)
            if (use_res, "o") in first:
                assert torch.equal(out, first[(use_res, "o")]), (pol, use_res)
            else:
                first[(use_res, "o")] = out
        # gamma == 1: the bits of mvp_gemm_bias_act_res
        o1, o0 = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)
        args, keep = _args(ap, wp, bias, res, o1, M, N, K, prec, pol)
        lib.check(so.mvp_gemm_scaled(C.byref(lib.GemmScaledArgs(args, lib.ptr(ones))), lib.stream_ptr()), pol)
        args0, keep0 = _args(ap, wp, bias, res, o0, M, N, K, prec, pol)
        lib.check((so.mvp_gemm_pp if pol == "pp_ilv" else so.mvp_gemm_bias_act_res)(C.byref(args0), lib.stream_ptr()), pol)
        torch.cuda.synchronize()
        assert torch.equal(o1, o0), pol


def test_layerscale_gemm_refuses_split_and_stream_k(dev):
    from mvp import lib

    so = lib.load()
    x = torch.zeros(64 * 64, device=dev)
    a = lib.GemmArgs(lib.ptr(x), lib.ptr(x), lib.ptr(x), lib.ptr(x), None, None, lib.ptr(x), None, None, 64, 64, 64, 64, 64, 64, 64, 64,
                     lib.ACT_NONE, lib.PREC_BF16X3, 0, 0, 0, 0)
    for sk in (2, -1):
        a.splitk = sk
        assert so.mvp_gemm_scaled(C.byref(lib.GemmScaledArgs(a, lib.ptr(x))), None) == -1
    a.splitk = 0
    assert so.mvp_gemm_scaled(C.byref(lib.GemmScaledArgs(a, None)), None) == -1


@pytest.mark.parametrize("hw", [(224, 224), (70, 99), (141, 55)])
def test_padded_patch_gather_and_patch_embed_vs_conv2d(dev, hw):
    """P = 14: gather into rows of 608 (588 + zero tail), GEMM against zero-padded weights == conv2d of the center-padded images."""
    from mvp import lib, ops

    H, W = hw
    B, P, Cout = 2, 14, 256
    g = torch.Generator().manual_seed(H * W)
    img = torch.randn(B, 3, H, W, generator=g)
    wt = torch.randn(Cout, 3, P, P, generator=g) * 0.05
    bias = torch.randn(Cout, generator=g)
    from oracle import vit as ovit

    padded = ovit.center_padding(img.double(), P)
    gh, gw = padded.shape[-2] // P, padded.shape[-1] // P
    ph, pw = padded.shape[-2] - H, padded.shape[-1] - W
    ref = F.conv2d(padded, wt.double(), bias.double(), stride=P).flatten(2).transpose(1, 2).reshape(-1, Cout)
    ldk = 608
    pair = ops.empty_pair((B * gh * gw, ldk), lib.PREC_BF16X3, dev)
    pair[0].fill_(1.0)
    pair[1].fill_(1.0)
    ops.patch_gather_ld(img.to(dev), pair, P, gh, gw, ph // 2, pw // 2, ldk)
    torch.cuda.synchronize()
    assert not pair[0][:, 588:].any() and not pair[1][:, 588:].any()
    cols = F.unfold(padded, P, stride=P).transpose(1, 2).reshape(-1, 588)
    assert ((pair[0][:, :588].double() + pair[1][:, :588].double()).cpu() - cols).abs().max().item() <= 2 ** -16 * cols.abs().max().item()
    wp = ops.split_bf16(F.pad(wt.reshape(Cout, -1), (0, ldk - 588)).to(dev))
    out = torch.empty(B * gh * gw, Cout, device=dev)
    ops.gemm(pair, wp, B * gh * gw, Cout, ldk, bias=bias.to(dev), out_f32=out)
    torch.cuda.synchronize()
    err = ((out.double().cpu() - ref).norm() / ref.norm()).item()
    assert err < 2e-5, err


def test_prefix_rows(dev):
    from mvp import ops

    B, N, Cc, R = 3, 20, 192, 4
    g = torch.Generator().manual_seed(7)
    cls, pos0, reg = torch.randn(Cc, generator=g).to(dev), torch.randn(Cc, generator=g).to(dev), torch.randn(R, Cc, generator=g).to(dev)
    x = torch.randn(B * N, Cc, generator=g).to(dev)
    want = x.clone().view(B, N, Cc)
    want[:, 0] = cls + pos0
    want[:, 1:1 + R] = reg
    ops.prefix_rows(cls, pos0, reg, x, B, N, Cc)
    torch.cuda.synchronize()
    assert torch.equal(x.view(B, N, Cc), want)


def _model(name, sd, precision, dev, **kw):
    import warnings

    from evals.models.dino import DINO

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = DINO(dino_name="dinov2", model_name=name, output="dense-cls", return_multilayer=True, add_norm=True, weights=sd,
                 precision=precision, **kw)
    return m.to(dev)


def _check_model(dev, name, sd, images, precision, tol=1e-3, label=""):
    from mvp import backbone as bb

    m = _model(name, sd, precision, dev)
    with torch.no_grad():
        outs = m(images.to(dev))
    ref = dinov2_ref.dense_features(bb.dinov2_hub_to_engine(sd), images.double(), m.multilayers)
    errs = []
    for o, r in zip(outs, ref):
        assert o.shape == r.shape, (o.shape, r.shape)
        errs.append(((o.double().cpu() - r).norm() / r.norm()).item())
    print(f"\n[dinov2 {label or name} {precision} {tuple(images.shape)}] rel-L2 per tap vs fp64 oracle: " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < tol, errs
    return m


@pytest.mark.parametrize("precision", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("R", [0, 4])
def test_tiny_dinov2_vs_oracle(dev, precision, R):
    """C = 128, 2 heads, depth 4, P = 14, R register tokens, a ragged image size (center padding, resampled 37x37 pos-embed)."""
    from mvp import backbone as bb

    sd = bb.random_dinov2_state_dict(128, 4, R, seed=3 + R)
    images = torch.randn(3, 3, 100, 130, generator=torch.Generator().manual_seed(5))
    _check_model(dev, "vitb14_reg" if R else "vitb14", sd, images, precision, label=f"tiny R={R}")


@pytest.mark.parametrize("precision", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("name,size,B", [("vitb14", (224, 224), 2), ("vitb14_reg", (224, 224), 2), ("vitl14", (224, 224), 1),
                                         ("vitb14", (480, 640), 1), ("vitb14_reg", (480, 640), 1)])
def test_dinov2_models_vs_oracle(dev, precision, name, size, B):
    """Full-size B/14, B/14-reg (N = 257 / 261 tokens at 224^2: the streaming attention kernel) and L/14 (C = 1024, 24 blocks)."""
    from mvp import backbone as bb

    C, depth, R = bb.DINOV2_ARCH[name]
    sd = bb.random_dinov2_state_dict(C, depth, R, seed=11)
    images = torch.randn(B, 3, *size, generator=torch.Generator().manual_seed(B + size[1]))
    m = _check_model(dev, name, sd, images, precision)
    assert m.multilayers == ([5, 11, 17, 23] if name == "vitl14" else [2, 5, 8, 11])


def test_dinov2_with_activation_outliers_vs_oracle(dev):
    """A few very large residual-stream channels (trained ViTs carry such outliers): scaled-up LayerScale on one channel of fc2."""
    from mvp import backbone as bb

    sd = bb.random_dinov2_state_dict(768, 12, 4, seed=21)
    for i in range(12):
        sd[f"blocks.{i}.ls2.gamma"][[7, 300]] = 40.0
        sd[f"blocks.{i}.mlp.fc2.bias"][[7, 300]] = 2.0
    images = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(2))
    _check_model(dev, "vitb14_reg", sd, images, "bf16x3", label="outliers")
    _check_model(dev, "vitb14_reg", sd, images, "f16x2", label="outliers")


def test_dinov2_grouped_forward_equals_single_batches(dev):
    """Two batches stacked into one forward (M = 2 x 16 x 261 rows: the large-M kernel with the LayerScale epilogue and interleaved
    operands) give each batch exactly the bits of its own forward (tile kernels)."""
    from mvp import backbone as bb

    sd = bb.random_dinov2_state_dict(768, 12, 4, seed=4)
    m = _model("vitb14_reg", sd, "f16x2", dev)
    eng = m.engine()
    imgs = torch.randn(32, 3, 224, 224, generator=torch.Generator().manual_seed(9)).to(dev)
    with torch.no_grad():
        grouped = eng.forward_taps(imgs, m.multilayers, bn=None, bn_mode=2, pack=False, want_cls=True, groups=2)
        for gidx in range(2):
            single = eng.forward_taps(imgs[16 * gidx:16 * (gidx + 1)].contiguous(), m.multilayers, bn=None, bn_mode=2, pack=False, want_cls=True)
            for a, b in zip(grouped[gidx], single):
                assert torch.equal(a, b), gidx
            for a, b in zip(grouped[gidx].cls, single.cls):
                assert torch.equal(a, b), gidx
