"""DINOv2 on the paths a training run takes: attention at the token counts DINOv2 produces (N = 257 / 261 at 224^2, up to 321) in all
four forms against fp64; the pipelined loop (spans that cut batches, carry stores, hipGraph replay) for B/14 with registers
(n_prefix = 5) against the serial loop, bit for bit; and the linear-probe training step on B/14-reg taps against the oracle."""
import numpy as np
import pytest
import torch

import dinov2_ref
from conftest import rel_l2
from test_gpu_kernels import _bf16_round, _qk_thirds_as_f16_comp, _v_third_as_f16_bf16

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("form", ["bf16x3", "bf16x3_vf16", "bf16x3_vf16_qk16", "bf16"])
@pytest.mark.parametrize("N", [257, 261, 300, 320, 321])
def test_attention_past_256_tokens_vs_fp64(dev, form, N):
    """softmax(Q K^T / 8) V at N = 257 / 261 (DINOv2 B/14 and B/14-reg at 224^2) and around the 320-token edge, 12 heads, B = 3: the bf16
    pair, the fp16 probabilities with V as fp16 + bf16 (VF16), Q.K^T in two f16 products, and plain bf16 (same bounds as test_attention)."""
    from mvp import lib, ops
    from mvp.vit import parse_precision

    B, H = 3, 12
    qk16, vf16 = form.endswith("_qk16"), "_vf16" in form
    pr = parse_precision(form.replace("_qk16", "").replace("_vf16", ""))
    C = H * 64
    g = torch.Generator().manual_seed(N)
    qkv = torch.randn(B * N, 3 * C, generator=g)
    qkv[:, :C] *= 2.0
    qp = ops.split_bf16(qkv.to(dev), pr)
    if vf16:
        qp = _v_third_as_f16_bf16(qp, C)
    if qk16:
        qp = _qk_thirds_as_f16_comp(qp, C)
    src = (_bf16_round(qkv) if pr == lib.PREC_BF16 else qkv).double()
    t = src.reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    ref = (((t[0] @ t[1].transpose(-2, -1)) * 0.125).softmax(-1) @ t[2]).transpose(1, 2).reshape(B * N, C)
    out = ops.empty_pair((B * N, C), lib.PREC_BF16X3, dev)
    out[0].fill_(float("nan"))
    out[1].fill_(float("nan"))
    ops.attention(qp, out, B, N, H, 0.125, pr, v_f16=vf16, qk_f16=qk16)
    torch.cuda.synchronize()
    got = (out[0].float() + out[1].float()).cpu()
    assert torch.isfinite(got).all()
    tol = (3e-4 if vf16 else 6e-5) if pr == lib.PREC_BF16X3 else 4e-3
    err = rel_l2(got.numpy(), ref.numpy())
    print(f"\n[attention {form} N={N}] rel-L2 vs fp64 {err:.2e} (bound {tol:.0e})")
    assert err < tol, (N, form, err)


def _build(dev, sd, precision="f16x2"):
    import warnings

    from evals.models.dino import DINO
    from evals.models.probes import DepthHead
    from evals.utils.optim import cosine_decay_linear_warmup
    from mvp.optim import FlatAdamW

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = DINO(dino_name="dinov2", model_name="vitb14_reg", output="dense-cls", return_multilayer=True, add_norm=True, weights=sd,
                     precision=precision).to(dev)
    torch.manual_seed(11)
    probe = DepthHead(feat_dim=model.feat_dim, head_type="linear", kernel_size=1, prediction_type="bindepth", min_depth=0.001, max_depth=10).to(dev)
    opt = FlatAdamW([{"params": probe.parameters(), "lr": 1e-3}])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda e: cosine_decay_linear_warmup(e, 100, 10))
    return model, probe, opt, sched


def _batches(dev, n, B, hw=(224, 224)):
    out = []
    for s in range(n):
        g = torch.Generator().manual_seed(700 + s)
        out.append({"image": torch.randn(B, 3, *hw, generator=g).to(dev), "depth": (torch.rand(B, 1, *hw, generator=g) * 9.0 + 0.05).to(dev)})
    return out


def _state(model, opt, losses):
    torch.cuda.synchronize()
    bn = [torch.cat([b.running_mean, b.running_var]).cpu().numpy() for b in model.batchnorms]
    return (torch.stack(losses).cpu().numpy(), opt.flat_param.cpu().numpy().copy(), opt.exp_avg_sq.cpu().numpy().copy(), bn,
            [int(b.num_batches_tracked) for b in model.batchnorms])


def test_dinov2_reg_span_pipeline_with_graphs_is_bit_identical_to_serial(dev):
    """B/14-reg (5 prefix rows per image), B = 16 at 224^2: forwards over spans of 24 images (every other forward starts with the 8
    images of a batch the previous span cut: carry stores of [taps, 8 x 261, 768] rows), graph replay, grouped tap BN — losses, probe
    weights, AdamW state and tap-BN running statistics equal the one-batch-at-a-time loop's bit for bit."""
    from evals.utils.losses import DepthLoss
    from mvp import backbone as bb
    from mvp.pipeline import FeaturePipeline, pipelined_features, rows_per_image, span_patterns
    from mvp.train import train_depth_step

    sd = bb.random_dinov2_state_dict(768, 12, 4, seed=13)
    n, B, span = 5, 16, 24
    bs = _batches(dev, n, B)
    loss_fn = DepthLoss()

    model, probe, opt, sched = _build(dev, sd)
    assert model.n_prefix == 5 and rows_per_image(224, 224, 14, model.n_prefix) == 261
    losses = [train_depth_step(model, probe, opt, sched, loss_fn, b["image"], b["depth"].clone()) for b in bs]
    ref = _state(model, opt, losses)

    model, probe, opt, sched = _build(dev, sd)
    pipe = FeaturePipeline(model, 2, graphs=True, group=2, span=span)
    losses = []
    for b, f in pipelined_features(model, bs, pipe=pipe):
        losses.append(train_depth_step(model, probe, opt, sched, loss_fn, None, b["depth"].clone(), feats=f))
    assert pipe.span == span and all(e["graph"] is not None for e in pipe._graphs.values())
    assert sorted((k[0], k[-1].carry) for k in pipe._graphs) == sorted(span_patterns(span, B))
    got = _state(model, opt, losses)
    np.testing.assert_array_equal(got[0], ref[0])
    np.testing.assert_array_equal(got[1], ref[1])
    np.testing.assert_array_equal(got[2], ref[2])
    for a, r in zip(got[3], ref[3]):
        np.testing.assert_array_equal(a, r)
    assert got[4] == ref[4] == [n] * 4


@pytest.mark.parametrize("precision", ["bf16x3", "f16x2"])
def test_dinov2_reg_linear_probe_step_vs_oracle(dev, precision):
    """backbone=dinov2_b14_reg (dense-cls, multilayer, train-mode tap BN) -> DepthHead(linear, k = 1, bindepth) -> bilinear -> DepthLoss ->
    backward -> FlatAdamW, B = 3 at 224^2, two steps: loss of each step and the updated probe weights against the oracle (fp64 DINOv2
    features of tests/dinov2_ref.py, oracle probe / loss / AdamW)."""
    from evals.utils.losses import DepthLoss
    from mvp import backbone as bb
    from mvp.train import train_depth_step
    from oracle import train as otrain

    sd = bb.random_dinov2_state_dict(768, 12, 4, seed=17)
    model, probe, opt, sched = _build(dev, sd, precision)
    psd = {k: v.detach().cpu().clone() for k, v in probe.state_dict().items()}
    eng_sd = bb.dinov2_hub_to_engine(sd)

    class DinoV2Trainer(otrain.DepthProbeTrainer):
        def features(self, images):
            with torch.no_grad():
                return [f.float() for f in dinov2_ref.dense_features(eng_sd, images.double(), self.layers, output="dense-cls")]

    ref = DinoV2Trainer(eng_sd, psd, layers=model.multilayers, heads=12, patch=14, lr=1e-3, max_step=100, warmup_step=10)
    loss_fn = DepthLoss()
    for step in range(2):
        images, tgt = otrain.synthetic_depth_batch(3, 224, 224, rank=0, step=step)
        l_ref = ref.step(images, tgt.clone())
        l_hip = train_depth_step(model, probe, opt, sched, loss_fn, images.to(dev), tgt.to(dev)).item()
        print(f"\n[dinov2_b14_reg linear step {step} {precision}] loss hip={l_hip:.6f} oracle={l_ref:.6f}")
        assert abs(l_hip - l_ref) < 1e-4 * abs(l_ref), (step, l_hip, l_ref)
    for n, p in probe.state_dict().items():
        if n not in ref.probe_sd:
            continue
        err = rel_l2(p.detach().cpu().numpy(), ref.probe_sd[n].detach().numpy())
        print(f"  updated {n}: rel-L2 vs oracle {err:.2e}")
        assert err < 1e-4, (n, err)


@pytest.mark.parametrize("precision", ["bf16x3", "f16x2"])
def test_full_size_models_vs_sampled_goldens(dev, precision):
    """The HIP models against the sampled outputs of transformers' Dinov2Model / Dinov2WithRegistersModel (reference wrapper glue, hub
    pos-embed rule; tests/golden/make_goldens_dinov2.py): B/14 and B/14-reg at 224^2 (B = 2) and 480 x 640 (B = 1), L/14 at 224^2."""
    import os
    import sys
    import warnings

    from conftest import REPO, load_golden
    from evals.models.dino import DINO
    from mvp import backbone as bb

    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import make_goldens_dinov2 as mg

    g = load_golden("dinov2_full_sampled.npz")
    for key, (model_name, seed, shapes) in mg.FULL.items():
        C, depth, R = bb.DINOV2_ARCH[model_name]
        sd = bb.random_dinov2_state_dict(C, depth, R, seed=seed)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = DINO(dino_name="dinov2", model_name=model_name, output="dense-cls", return_multilayer=True, add_norm=True, weights=sd,
                     precision=precision).to(dev)
        for (B, H, W) in shapes:
            with torch.no_grad():
                outs = m(mg.full_images(B, H, W).to(dev))
            errs = []
            for j, o in enumerate(outs):
                tag = f"{key}_{B}x{H}x{W}_tap{j}"
                assert tuple(o.shape) == tuple(g[tag + "_shape"]), tag
                errs.append(rel_l2(o.float().cpu().numpy().reshape(-1)[mg.sample_index(o.numel())], g[tag]))
            print(f"\n[{key} {B}x{H}x{W} {precision}] rel-L2 vs sampled goldens per tap: " + " ".join(f"{e:.2e}" for e in errs))
            assert max(errs) < 1e-3, (key, B, H, W, errs)
