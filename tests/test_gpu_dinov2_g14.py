"""DINOv2 with the SwiGLU MLP (ViT-g/14) and DINO ViT-B/8 on the HIP engine against fp64: tiny SwiGLU models whose hidden width needs
padding (344 -> 384) or not (512), the true width (C = 1536, 24 heads, H = 4096) at depth 4, the pipelined loop against the serial
one bit for bit, and patch-8 models (tiny, and the real geometry at N = 785) with ``extract_kqv``.  Contract: relative L2 per tap
<= 1e-3 (the GELU models measure about 2e-5)."""
import functools
import warnings

import pytest
import torch

import swiglu_ref
from oracle import vit as ovit

pytestmark = pytest.mark.gpu

TOL = 1e-3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _dino(dev, **kw):
    from evals.models.dino import DINO

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return DINO(**kw).to(dev)


def _rel(o, r):
    return ((o.double().cpu() - r).norm() / r.norm()).item()


# ------------------------------------------------------------------------------------------------ SwiGLU
@functools.lru_cache(maxsize=None)
def _glu_case(C, depth, R, B, H, W):
    """(hub-layout weights, images, fp64 reference per tap) of one SwiGLU case: computed once, shared by both precisions."""
    from mvp import backbone as bb

    sd = bb.random_dinov2_state_dict(C, depth, R, seed=C + R, ffn="swiglu")
    images = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(B + W))
    layers = bb.multilayer_indices(depth)
    with torch.no_grad():
        ref = swiglu_ref.dense_features(bb.dinov2_hub_to_engine(sd), images.double(), layers)
    return sd, images, layers, ref


def _check_glu(dev, precision, C, depth, R, B, H, W):
    sd, images, layers, ref = _glu_case(C, depth, R, B, H, W)
    # (the wrapper takes the registers' position rule from the model name; the SwiGLU MLP from the weights)
    m = _dino(dev, dino_name="dinov2", model_name="vitb14_reg" if R else "vitg14", output="dense-cls", return_multilayer=True, add_norm=True,
              weights=sd, precision=precision)
    assert m.multilayers == layers and m.heads == C // 64
    with torch.no_grad():
        outs = m(images.to(dev))
    eng = m.engine()
    Hh = swiglu_ref.hidden_width(C)
    assert eng.act_name == "swiglu" and eng.swiglu_h == Hh and eng.hidden == -(-Hh // 64) * 64 and eng.fc1_out == 2 * Hh
    errs = []
    for o, r in zip(outs, ref):
        assert o.shape == r.shape, (o.shape, r.shape)
        errs.append(_rel(o, r))
    print(f"\n[swiglu C={C} depth={depth} R={R} {precision} {tuple(images.shape)}] rel-L2 per tap vs fp64: " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= TOL, errs
    return m


@pytest.mark.parametrize("precision", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("hw", [(70, 99), (224, 224)])
@pytest.mark.parametrize("C,R", [(128, 0), (192, 4)])
def test_tiny_swiglu_models_vs_fp64(dev, precision, hw, C, R):
    """C = 128: H = 344, padded to 384 columns, C and the row counts too small for the interleaved operands; C = 192 with four register
    tokens: H = 512, no padding.  B = 2, a ragged size (center padding, resampled position table) and 224^2."""
    m = _check_glu(dev, precision, C, 4, R, 2, *hw)
    assert m.engine().hidden == (384 if C == 128 else 512) and m.n_prefix == 1 + R


@pytest.mark.parametrize("precision", ["bf16x3", "f16x2"])
def test_true_width_swiglu_vs_fp64(dev, precision):
    """ViT-g/14's width (C = 1536, 24 heads, H = 4096) at depth 4, B = 1, 224^2."""
    m = _check_glu(dev, precision, 1536, 4, 0, 1, 224, 224)
    assert m.heads == 24 and m.engine().hidden == 4096


def test_f16_range_check_covers_the_gate_output(dev, monkeypatch):
    """MVP_CHECK_F16_RANGE=1: a gate output beyond fp16's range (a huge w12 bias on one value column) is reported, by name."""
    from mvp import backbone as bb, lib

    sd = dict(_glu_case(128, 4, 0, 2, 70, 99)[0])
    b = sd["blocks.0.mlp.w12.bias"].clone()
    b[0], b[344] = 300.0, 300.0  # gate and value of hidden column 0: silu(300) * 300 = 9e4
    sd["blocks.0.mlp.w12.bias"] = b
    monkeypatch.setenv("MVP_CHECK_F16_RANGE", "1")
    m = _dino(dev, dino_name="dinov2", model_name="vitg14", return_multilayer=True, weights=sd, precision="f16x2")
    with pytest.raises(lib.MvpError, match="block 0: SwiGLU gate output"):
        with torch.no_grad():
            m(torch.zeros(1, 3, 28, 28, device=dev))
    assert bb.swiglu_hidden(128) == 344


def test_swiglu_pipelined_loop_is_bit_identical_to_serial(dev):
    """Five batches of three images of the C = 192 model: spans of four images (every forward but the first starts inside a batch: carry
    stores), grouped tap BN, graph replay — features and tap-BN running statistics equal the one-batch-at-a-time loop's bit for bit."""
    from mvp import backbone as bb
    from mvp.pipeline import FeaturePipeline, pipelined_features
    from mvp.train import extract_features

    sd = bb.random_dinov2_state_dict(192, 4, 4, seed=31, ffn="swiglu")
    n, B, span = 5, 3, 4
    bs = [{"image": torch.randn(B, 3, 70, 98, generator=torch.Generator().manual_seed(900 + s)).to(dev)} for s in range(n)]

    def build():
        return _dino(dev, dino_name="dinov2", model_name="vitb14_reg", output="dense-cls", return_multilayer=True, add_norm=True, weights=sd,
                     precision="f16x2")

    def bn_state(m):
        return [torch.cat([b.running_mean, b.running_var]).cpu() for b in m.batchnorms] + [torch.tensor([int(b.num_batches_tracked) for b in m.batchnorms])]

    model = build()
    ref = [[f.clone() for f in extract_features(model, b["image"])] for b in bs]
    torch.cuda.synchronize()
    ref_bn = bn_state(model)

    model = build()
    pipe = FeaturePipeline(model, 2, graphs=True, group=2, span=span)
    got = []
    for b, f in pipelined_features(model, bs, pipe=pipe):
        got.append([t.clone() for t in f])
    torch.cuda.synchronize()
    assert pipe.span == span and len(got) == n
    for g, r in zip(got, ref):
        assert len(g) == len(r) == 4
        for a, c in zip(g, r):
            assert torch.equal(a, c)
    for a, c in zip(bn_state(model), ref_bn):
        assert torch.equal(a, c)


# ------------------------------------------------------------------------------------------------ DINO ViT-B/8
@functools.lru_cache(maxsize=None)
def _b8_case(C, depth, B, H, W):
    sd = ovit.make_vit_weights(C, depth, patch=8, img=224, seed=C + depth)
    images = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(H + W))
    layers = ovit.multilayer_indices(depth)
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        ref = ovit.vit_dense_features(sd64, images.double(), layers, heads=C // 64, patch=8)
    return sd, sd64, images, layers, ref


def _check_b8(dev, precision, C, depth, B, H, W):
    sd, _, images, layers, ref = _b8_case(C, depth, B, H, W)
    m = _dino(dev, dino_name="dino", model_name="vitb8", return_multilayer=True, add_norm=True, weights=sd, precision=precision)
    assert m.patch_size == 8 and m.multilayers == layers
    with torch.no_grad():
        outs = m(images.to(dev))
    errs = [_rel(o, r) for o, r in zip(outs, ref)]
    assert all(o.shape == r.shape for o, r in zip(outs, ref))
    print(f"\n[dino vitb8 C={C} depth={depth} {precision} {tuple(images.shape)}] rel-L2 per tap vs fp64 oracle: " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= TOL, errs
    return m


@pytest.mark.parametrize("precision", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("hw", [(64, 72), (224, 224)])
def test_tiny_patch8_model_vs_oracle(dev, precision, hw):
    """C = 128, depth 4, a 28 x 28 position table: 64 x 72 (an 8 x 9 grid, resampled table) and 224^2 (N = 785, the table as it is)."""
    _check_b8(dev, precision, 128, 4, 2, *hw)


@pytest.mark.parametrize("precision", ["bf16x3", "f16x2"])
def test_patch8_extract_kqv_vs_oracle(dev, precision):
    """``extract_kqv`` (k | q | v of the last block's fused projection, CLS row dropped) of the tiny patch-8 model at 64 x 72."""
    sd, sd64, images, _, _ = _b8_case(128, 4, 2, 64, 72)
    m = _dino(dev, dino_name="dino", model_name="vitb8", return_kqv=True, mode_selected="kqv", weights=sd, precision=precision)
    got = m.extract_kqv(images.to(dev))
    with torch.no_grad():
        q, k, v = ovit.last_block_qkv(sd64, images.double(), heads=2, patch=8)
    ref = torch.cat([t[:, 1:].transpose(1, 2) for t in (k, q, v)], dim=1)
    assert got.shape == ref.shape == (2, 3 * 128, 72)
    err = _rel(got, ref)
    print(f"\n[dino vitb8 extract_kqv {precision}] rel-L2 vs fp64 oracle {err:.2e}")
    assert err <= TOL, err


@pytest.mark.parametrize("precision", ["bf16x3", "f16x2"])
def test_vitb8_real_geometry_vs_oracle(dev, precision):
    """ViT-B/8 as published: C = 768, depth 12, B = 1 at 224^2 (N = 785 tokens)."""
    m = _check_b8(dev, precision, 768, 12, 1, 224, 224)
    assert m.heads == 12 and m.multilayers == [2, 5, 8, 11]
