"""ConvNeXt / ConvNeXt V2 on the GPU: the engine (mvp/convnext.py) and the wrapper (evals/models/convnext.py) against the goldens made
with transformers' ConvNextModel / ConvNextV2Model (tests/golden/make_goldens_convnext.py), relative L2 <= 1e-3 per tap (README's feature
contract; every error is printed); a linear-probe and a DPT-probe training step on ConvNeXt features against the CPU oracle; the
train_depth.py entry point with either probe."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden, rel_l2

sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

pytestmark = pytest.mark.gpu

TOL = 1e-3
PKG = os.path.join(REPO, "midvision-probe_amd")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _wrapper(sd, v2, dev, **kw):
    from evals.models.convnext import ConvNext

    arch, ckpt = ("convnext_base", "fcmae_ft_in22k_in1k_384") if v2 else ("convnext_base", "in22k")
    return ConvNext(arch, ckpt, weights=sd, **kw).to(dev)


@pytest.mark.parametrize("v2", [False, True])
def test_tiny_engine_and_wrapper_against_the_goldens(dev, v2):
    """Widths 64/128/192/256, depths 1/1/2/1, B = 2.  48 x 80: maps 12x20 ... 1x2 (smaller than the 7x7 window; odd sides floored by the
    2x2 / 2 convolutions).  50 x 75: center_padding to 64 x 80 inside the stem's gather.  Stage outputs, then the wrapper's dense / gap
    outputs for all four taps and for layer 0 and 3 alone."""
    import make_goldens_convnext as mg
    from mvp.convnext import ConvNeXtEngine

    g = load_golden("convnext_tiny_v2.npz" if v2 else "convnext_tiny_v1.npz")
    sd = mg.state_dict(mg.TINY, v2)
    eng = ConvNeXtEngine(sd, mg.TINY["depths"], mg.TINY["widths"], precision="bf16x3", device=dev)
    assert eng.v2 == v2
    f16 = ConvNeXtEngine(sd, mg.TINY["depths"], mg.TINY["widths"], precision="f16x2", device=dev)
    from mvp import lib

    assert f16.pr == lib.PREC_BF16X3  # an f16x2 request falls back, as ResNetEngine's does
    for size in mg.TINY["sizes"]:
        tag = f"s{size[0]}_"
        img = torch.from_numpy(g[tag + "images"]).to(dev)
        taps = eng.forward_taps(img, [0, 1, 2, 3], pad_to=16)
        errs = [rel_l2(t.cpu().numpy(), g[f"{tag}stage{j}"]) for j, t in enumerate(taps)]
        print(f"[convnext tiny v{2 if v2 else 1} {size}] stage errors {['%.2e' % e for e in errs]}")
        assert [tuple(t.shape) for t in taps] == [g[f"{tag}stage{j}"].shape for j in range(4)]
        assert max(errs) <= TOL, errs
        (only2,) = eng.forward_taps(img, [2], pad_to=16)  # stops after stage 2
        assert torch.equal(only2, taps[2])
        for output in ("dense", "gap"):
            m = _wrapper(sd, v2, dev, output=output, return_multilayer=True, precision="bf16x3")
            outs = m(img)
            errs = [rel_l2(o.cpu().numpy(), g[f"{tag}{output}{j}"]) for j, o in enumerate(outs)]
            print(f"[convnext tiny v{2 if v2 else 1} {size}] {output} errors {['%.2e' % e for e in errs]}")
            assert [tuple(o.shape) for o in outs] == [g[f"{tag}{output}{j}"].shape for j in range(4)]
            assert max(errs) <= TOL, (output, errs)
            for layer in (0, 3):
                one = _wrapper(sd, v2, dev, output=output, layer=layer, precision="bf16x3")(img)
                assert torch.is_tensor(one) and rel_l2(one.cpu().numpy(), g[f"{tag}{output}{layer}"]) <= TOL, (output, layer)
        last = _wrapper(sd, v2, dev)(img)  # layer = -1, dense, the default precision
        assert rel_l2(last.cpu().numpy(), g[f"{tag}dense3"]) <= TOL


@pytest.mark.parametrize("name", ["convnext_mid.npz", "convnext_full_sampled.npz"])
@pytest.mark.parametrize("v2", [False, True])
def test_sampled_goldens(dev, name, v2):
    """mid: the real widths 128 ... 1024 (K = 1024, N = 4096 GEMMs) with depths 1/1/2/1 at 64 x 96; full: ConvNeXt-B / V2-B (3/3/27/3)
    at 224^2, B = 2 — sampled elements of every stage output and of the wrapper's dense map of the last tap."""
    import make_goldens_convnext as mg
    from make_goldens_dinov2 import sample_index

    cfg = {"convnext_mid.npz": mg.MID, "convnext_full_sampled.npz": mg.FULL}[name]
    g = load_golden(name)
    tag = "v2_" if v2 else "v1_"
    sd = mg.state_dict(cfg, v2)
    np.testing.assert_allclose(mg.checksums(sd), g[tag + "checksums"], rtol=1e-9)
    (size,) = cfg["sizes"]
    img = mg.images(cfg, size).to(dev)
    m = _wrapper(sd, v2, dev, return_multilayer=True, precision="bf16x3")
    assert m.depths == list(cfg["depths"]) and m.widths == list(cfg["widths"])
    taps = m.engine().forward_taps(img, [0, 1, 2, 3], pad_to=16)
    errs = []
    for j, t in enumerate(taps):
        t = t.cpu().numpy()
        assert tuple(g[f"{tag}stage{j}_shape"]) == t.shape
        errs.append(rel_l2(t.reshape(-1)[sample_index(t.size)], g[f"{tag}stage{j}"]))
    d = m(img)[3].cpu().numpy()
    assert tuple(g[tag + "dense3_shape"]) == d.shape
    errs.append(rel_l2(d.reshape(-1)[sample_index(d.size)], g[tag + "dense3"]))
    print(f"[convnext {name} v{2 if v2 else 1}] stage 0-3 and dense errors {['%.2e' % e for e in errs]}")
    assert max(errs) <= TOL, errs


def test_linear_probe_step_on_convnext_features_vs_oracle(dev):
    """One linear bindepth probe step on the four dense ConvNeXt maps (tiny size, 64 x 96 images -> 4 x 6 maps of 64 + 128 + 192 + 256
    channels): features <= 1e-3, loss 1e-4, prediction within the depth-RMSE 1e-2 contract, gradients against the CPU oracle
    (oracle/train.py with the fp64 trunk of tests/convnext_ref.py as its feature extractor)."""
    import convnext_ref as ref
    import make_goldens_convnext as mg
    from evals.models.probes import DepthHead
    from evals.utils.losses import DepthLoss
    from mvp import functional as MF
    from mvp.optim import FlatAdamW
    from mvp.train import extract_features
    from oracle import probes as oprobes
    from oracle import train as otrain

    sd = mg.state_dict(mg.TINY, False)
    widths = list(mg.TINY["widths"])
    psd = oprobes.make_linear_head_weights(widths, 256, 1, seed=3)
    images, tgt = otrain.synthetic_depth_batch(3, 64, 96, rank=0, step=0)

    class Trainer(otrain.DepthProbeTrainer):
        def features(self, images):
            return [f.float() for f in ref.wrapper_forward(sd, images, (0, 1, 2, 3), "dense")]

    tr = Trainer({"cls_token": torch.zeros(1, 1, 8)}, psd, max_step=100, warmup_step=10)
    feats_ref = tr.features(images)
    loss_ref, pred_ref = tr.forward_loss(feats_ref, tgt.clone())
    loss_ref.backward()

    model = _wrapper(sd, False, dev, return_multilayer=True, precision="bf16x3")
    probe = DepthHead(feat_dim=model.feat_dim, head_type="linear", kernel_size=1, prediction_type="bindepth", precision="bf16x3")
    probe.load_state_dict(psd, strict=True)
    probe = probe.to(dev)
    opt = FlatAdamW([{"params": probe.parameters(), "lr": 5e-4}])
    opt.zero_grad()
    feats = extract_features(model, images.to(dev))
    ferr = [rel_l2(f.cpu().numpy(), fr.numpy()) for f, fr in zip(feats, feats_ref)]
    pred = MF.interpolate(probe(feats), size=tgt.shape[-2:], mode="bilinear")
    loss = DepthLoss()(pred, tgt.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    rmse = (pred.detach().cpu() - pred_ref.detach()).pow(2).mean().sqrt().item() / pred_ref.detach().abs().mean().item()
    gw = rel_l2(probe.head.conv.weight.grad.cpu().numpy(), tr.probe_sd["head.conv.weight"].grad.numpy())
    gb = rel_l2(probe.head.conv.bias.grad.cpu().numpy(), tr.probe_sd["head.conv.bias"].grad.numpy())
    print(f"[convnext linear probe] feature errors {['%.2e' % e for e in ferr]}  loss {loss.item():.6f} vs {loss_ref.item():.6f}  "
          f"depth RMSE rel {rmse:.2e}  grad W / b {gw:.2e} / {gb:.2e}")
    assert max(ferr) <= TOL
    assert abs(loss.item() - loss_ref.item()) < 1e-4 * abs(loss_ref.item())
    assert rmse < 1e-2
    assert gw < 1e-3 and gb < 1e-3


@pytest.mark.timeout(900)
def test_train_depth_entrypoint_with_convnext(tmp_path):
    """`python train_depth.py backbone=convnext_in22k probe=depth_linear` on the synthetic dataset, two steps (seeded random ConvNeXt-B:
    no checkpoint directory)."""
    env = dict(os.environ, MVP_CKPT_DIR=str(tmp_path / "none"))
    args = ["backbone=convnext_in22k", "probe=depth_linear", f"output_dir={tmp_path}/result", "dataset.image_size=[64,96]", "dataset.num_batches=2",
            "batch_size=2", "optimizer=one_epoch", "num_workers=0"]
    p = subprocess.run([sys.executable, os.path.join(PKG, "train_depth.py")] + args, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-4000:]
    assert "SA valid loss" in out and "results ->" in out and "saved" in out


def test_dpt_probe_step_on_convnext_features_vs_oracle(dev):
    """The DPT probe on four ConvNeXt taps of DIFFERENT widths (64 / 128 / 192 / 256 channels at one 4 x 6 resolution: mvp/dpt.py takes
    per-tap widths): loss, prediction within the depth-RMSE 1e-2 contract, and every parameter gradient against the CPU oracle.  Gradient
    bounds as tests/test_gpu_dpt.py::test_dpt_probe_fwd_bwd_vs_oracle: against the plain oracle a few ReLU gates differ, hence rel-L2 5e-2
    plus a direction check."""
    import convnext_ref as ref
    import make_goldens_convnext as mg
    from evals.models.probes import DepthHead
    from evals.utils.losses import DepthLoss
    from mvp import functional as MF
    from mvp.train import extract_features
    from oracle import probes as oprobes
    from oracle import train as otrain

    sd = mg.state_dict(mg.TINY, True)
    widths, Hd = list(mg.TINY["widths"]), 128
    psd = oprobes.make_dpt_weights(widths, 256, hidden=Hd, k=3, seed=5)
    images, tgt = otrain.synthetic_depth_batch(2, 64, 96, rank=0, step=1)

    class Trainer(otrain.DepthProbeTrainer):
        def features(self, images):
            return [f.float() for f in ref.wrapper_forward(sd, images, (0, 1, 2, 3), "dense")]

    tr = Trainer({"cls_token": torch.zeros(1, 1, 8)}, psd, head_type="dpt", k=3, max_step=100, warmup_step=10)
    loss_ref, pred_ref = tr.forward_loss(tr.features(images), tgt.clone())
    loss_ref.backward()

    model = _wrapper(sd, True, dev, return_multilayer=True, precision="bf16x3")
    assert model.feat_dim == widths
    probe = DepthHead(feat_dim=model.feat_dim, head_type="dpt", prediction_type="bindepth", hidden_dim=Hd, kernel_size=3, precision="bf16x3")
    probe.load_state_dict(psd, strict=True)
    probe = probe.to(dev)
    feats = extract_features(model, images.to(dev))
    pred = MF.interpolate(probe(feats), size=tgt.shape[-2:], mode="bilinear")
    loss = DepthLoss()(pred, tgt.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    rmse = (pred.detach().cpu() - pred_ref.detach()).pow(2).mean().sqrt().item() / pred_ref.detach().abs().mean().item()
    worst = 0.0
    for n, p in probe.named_parameters():
        e = rel_l2(p.grad.cpu().numpy(), tr.probe_sd[n].grad.numpy())
        worst = max(worst, e)
        a64, b64 = p.grad.double().cpu().flatten(), tr.probe_sd[n].grad.double().flatten()
        assert e < 5e-2 and 1 - float(a64 @ b64 / (a64.norm() * b64.norm())) < 2e-3, (n, e)
    print(f"[convnext dpt probe] loss {loss.item():.6f} vs {loss_ref.item():.6f}  depth RMSE rel {rmse:.2e}  worst param-grad rel-L2 {worst:.2e}")
    assert abs(loss.item() - loss_ref.item()) < 1e-3 * abs(loss_ref.item())
    assert rmse < 1e-2


@pytest.mark.timeout(900)
def test_train_depth_entrypoint_with_convnext_dpt(tmp_path):
    """The multilayer DPT probe on ConvNeXt-B's four stage widths (feat_dim = [128, 256, 512, 1024], one resolution), two steps."""
    env = dict(os.environ, MVP_CKPT_DIR=str(tmp_path / "none"))
    args = ["backbone=convnext_in22k", "+backbone.return_multilayer=True", "probe=depth_dpt", "probe.hidden_dim=128", f"output_dir={tmp_path}/result",
            "dataset.image_size=[64,96]", "dataset.num_batches=2", "batch_size=2", "optimizer=one_epoch", "num_workers=0"]
    p = subprocess.run([sys.executable, os.path.join(PKG, "train_depth.py")] + args, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-4000:]
    assert "SA valid loss" in out and "results ->" in out and "saved" in out
