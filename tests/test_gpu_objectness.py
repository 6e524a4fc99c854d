"""BinaryHead / TaskonomyHead, train_objectness_step, validation() and the entry script on the GPU, against what the reference recorded
(tests/golden/objectness.npz) and the fp64 restatement (tests/objectness_ref.py).

The linear trunks are compared with the golden itself; the multiscale and DPT trunks, which the HIP path runs at widths that are multiples
of 128 only, with the CPU oracle + the restatement at width 128 (``_wide_case``).

Bounds.  The trunks are held to rel-L2 1e-4 by tests/test_gpu_dpt.py; BatchNorm divides by the batch spread, which amplifies a
relative error of the trunk by rms / sigma of its output, a factor stored with every golden case (1.0 .. 1.3, asserted <= 1 / 0.3 by the
generator).  Forward, eval forward and loss: 1e-4 x that factor.  Parameter gradients of the linear cases: GRAD_TOL of
tests/test_gpu_probe.py x the factor.  Trajectory: losses rtol 1e-4, final weights rel-L2 1e-4 (test_train_step_tiny_vs_reference_golden's
bounds) x the factor."""
import csv
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import objectness_ref as R
from conftest import PKG, load_golden, rel_l2
from test_gpu_probe import GRAD_TOL

pytestmark = pytest.mark.gpu

CASES = [("lin_k1", "linear", 1), ("lin_k3", "linear", 3), ("ms_k1", "multiscale", 1), ("dpt_k3", "dpt", 3)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g():
    return load_golden("objectness.npz")


def _sd(g, case):
    pre = f"{case}__sd__"
    return {k[len(pre):]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith(pre)}


def _probe(g, case, dev, cls=None, **kw):
    from evals.models.probes import BinaryHead

    probe = (cls or BinaryHead)(feat_dim=[8] * 4, hidden_dim=16, precision="bf16x3", **kw)
    probe.load_state_dict(_sd(g, case), strict=True)  # the reference's state dict, keys unchanged
    return probe.to(dev)


def _wide_case(g, case, head_type, k):
    """The multiscale and DPT trunks run on the HIP path with feature and hidden widths that are multiples of 128 only, which the golden's
    tiny widths (8 and 16) are not, and weights of that width do not fit a committed fixture.  For these two trunks the expected values
    are therefore computed here, at width 128: the trunk by the CPU oracle in fp64 (oracle/probes.py, pinned to the reference's modules
    by tests/golden/probes*.npz), the tail by the fp64 restatement (pinned to the reference's BinaryHead at the golden's widths, these
    two trunks included, by tests/test_objectness_cpu.py).  Same seeded conditioning as the golden generator: every conv weight of the
    trunk is doubled until sigma >= 0.3 rms of the pre-BatchNorm map, with and without the last conv's bias.  The oracle's DPT returns
    the UPSAMPLED map, so its statistics are the reference's: the running variance checks the n = 4 P correction."""
    import torch.nn.functional as F

    from oracle import probes as oprobes

    W = 128
    gen = torch.Generator().manual_seed(97 + k)
    feats = [torch.randn(2, W, 4, 4, generator=gen) for _ in range(4)]
    mask = torch.from_numpy(g["mask"])
    if head_type == "multiscale":
        sd, last, trunk = oprobes.make_multiscale_weights([W] * 4, 1, hidden=W, k=k, seed=51), "head.conv_out.2", oprobes.multiscale_head
    else:
        sd, last, trunk = oprobes.make_dpt_weights([W] * 4, 1, hidden=W, k=k, seed=52), "head.out_conv.2", lambda s_, f_: oprobes.dpt_head(s_, f_, k)
    for _ in range(8):
        x = trunk({n: v.double() for n, v in sd.items()}, [f.double() for f in feats])
        sigma = x.var(unbiased=False).sqrt()
        amp = float(torch.maximum(x.pow(2).mean().sqrt(), (x - sd[last + ".bias"].double()).pow(2).mean().sqrt()) / sigma)
        if amp <= 1.0 / 0.3:
            break
        sd = {n: (v * 2.0 if n.endswith(".weight") else v) for n, v in sd.items()}
    assert amp <= 1.0 / 0.3, amp
    bn = dict(weight=np.array([1.3]), bias=np.array([-0.2]), running_mean=np.array([0.05]), running_var=np.array([0.8]))
    sd.update({f"batch_norm.{n}": torch.tensor(v, dtype=torch.float32) for n, v in bn.items()})
    sd["batch_norm.num_batches_tracked"] = torch.tensor(0)
    xn = x.numpy()
    f = R.bn_act_fwd(xn, bn["weight"], bn["bias"], bn["running_mean"], bn["running_var"])
    y = torch.from_numpy(f["y"]).requires_grad_(True)
    pred = F.interpolate(y, size=mask.shape[-2:], mode="bilinear")
    pred.backward(torch.from_numpy(R.bce_grad(pred.detach().numpy(), mask.numpy())))
    b = R.bn_act_bwd(xn, y.grad.numpy(), bn["weight"], bn["bias"])
    e = R.bn_act_fwd(xn, bn["weight"], bn["bias"], f["running_mean"], f["running_var"], training=False)
    out = {f"{case}__amp": amp, f"{case}__out": f["y"], f"{case}__loss": R.bce(pred.detach().numpy(), mask.numpy()), f"{case}__eval_out": e["y"],
           f"{case}__after__running_mean": f["running_mean"], f"{case}__after__running_var": f["running_var"], f"{case}__after__num_batches_tracked": 1,
           f"{case}__grad__batch_norm.weight": b["grad_gamma"], f"{case}__grad__batch_norm.bias": b["grad_beta"],
           f"{case}__name": f"snorm_{head_type}_k{k}", "feats": [t.numpy() for t in feats], "mask": g["mask"]}
    return out, sd, W


@pytest.mark.parametrize("case,head_type,k", CASES)
def test_binary_head_matches_reference(dev, g, case, head_type, k):
    from evals.models.probes import BinaryHead, TaskonomyHead
    from mvp import functional as MF

    wide = None
    if head_type != "linear":
        g, wide, width = _wide_case(g, case, head_type, k)
    amp = float(g[f"{case}__amp"])
    tol = 1e-4 * amp
    feats = [torch.from_numpy(f).to(dev) for f in g["feats"]]
    mask = torch.from_numpy(g["mask"]).to(dev)
    # TaskonomyHead is the same body with output_dim = 1 by default: run it for one case instead of BinaryHead
    if wide is not None:
        probe = BinaryHead(feat_dim=[width] * 4, hidden_dim=width, precision="bf16x3", head_type=head_type, kernel_size=k, output_dim=1)
        probe.load_state_dict(wide, strict=True)
        probe = probe.to(dev)
    elif case == "lin_k3":
        probe = _probe(g, case, dev, cls=TaskonomyHead, head_type=head_type, kernel_size=k)
    else:
        probe = _probe(g, case, dev, head_type=head_type, kernel_size=k, output_dim=1)
    assert probe.name == str(g[f"{case}__name"]) and probe.training
    y = probe(feats)
    loss = MF.bce_loss(MF.interpolate(y, size=mask.shape[-2:], mode="bilinear"), mask)
    MF.backward(loss)
    torch.cuda.synchronize()
    figs = {"out": rel_l2(y.detach().cpu().numpy(), g[f"{case}__out"]), "loss": abs(float(loss) - float(g[f"{case}__loss"])) / float(g[f"{case}__loss"])}
    assert tuple(y.shape) == g[f"{case}__out"].shape
    bn = probe.batch_norm
    # the DPT case normalises before the nearest x2: its running_var must carry the count of the upsampled map (n = 4 P)
    np.testing.assert_allclose(bn.running_mean.cpu().numpy(), g[f"{case}__after__running_mean"], rtol=1e-4)
    np.testing.assert_allclose(bn.running_var.cpu().numpy(), g[f"{case}__after__running_var"], rtol=1e-4)
    assert int(bn.num_batches_tracked) == int(g[f"{case}__after__num_batches_tracked"]) == 1
    gtol = GRAD_TOL * amp
    for n in ("weight", "bias"):
        figs[f"grad bn.{n}"] = rel_l2(getattr(bn, n).grad.cpu().numpy(), g[f"{case}__grad__batch_norm.{n}"])
        assert figs[f"grad bn.{n}"] <= gtol, figs
    if head_type == "linear":
        gw = g[f"{case}__grad__head.conv.weight"]
        figs["grad conv.weight"] = rel_l2(probe.head.conv.weight.grad.cpu().numpy(), gw)
        # the gradient of a bias in front of a train-mode BatchNorm is exactly zero (the reference stores 1e-9 of rounding): held
        # absolutely, against the scale of the weight gradient, which is the same sum over pixels weighted by unit-size features
        figs["grad conv.bias / |grad conv.weight|"] = float(np.abs(probe.head.conv.bias.grad.cpu().numpy()).max() / np.linalg.norm(gw))
        assert figs["grad conv.weight"] <= gtol and figs["grad conv.bias / |grad conv.weight|"] <= gtol, figs
    probe.eval()
    with torch.no_grad():
        ye = probe(feats)
    figs["eval_out"] = rel_l2(ye.cpu().numpy(), g[f"{case}__eval_out"])
    assert int(bn.num_batches_tracked) == 1  # eval mode updates nothing
    print(f"{case}: rms/sigma {amp:.3f} " + " ".join(f"{k_}={v:.2e}" for k_, v in figs.items()))
    assert figs["out"] <= tol and figs["loss"] <= tol and figs["eval_out"] <= tol, figs


def test_two_channel_tanh_and_raw_forms(dev, g):
    from evals.models.probes import BinaryHead

    feats = [torch.from_numpy(f).to(dev) for f in g["feats"]]
    probe = _probe(g, "od2", dev, head_type="linear", kernel_size=1)  # BinaryHead's default output_dim = 2
    y = probe(feats)
    assert rel_l2(y.detach().cpu().numpy(), g["od2__out"]) <= 1e-4 * float(g["od2__amp"])
    np.testing.assert_allclose(probe.batch_norm.running_var.cpu().numpy(), g["od2__after__running_var"], rtol=1e-4)
    probe = _probe(g, "tanh", dev, head_type="linear", kernel_size=1, output_dim=1, pred_type="tanh")
    yt = probe(feats)
    assert rel_l2(yt.detach().cpu().numpy(), g["tanh__out"]) <= 1e-4
    raw = BinaryHead(feat_dim=[8] * 4, head_type="linear", kernel_size=1, output_dim=1, pred_type="logits", precision="bf16x3")
    raw.load_state_dict(_sd(g, "tanh"), strict=True)
    yr = raw.to(dev)(feats)
    assert rel_l2(np.tanh(yr.detach().cpu().numpy().astype(np.float64)), g["tanh__out"]) <= 1e-4


def test_train_objectness_step_trajectory_vs_reference(dev, g):
    """The drop-in loop body (BinaryHead -> interpolate -> bce_loss -> backward -> FlatAdamW -> LambdaLR) reproduces the reference's
    8-step trajectory."""
    from evals.utils.optim import cosine_decay_linear_warmup
    from mvp.optim import FlatAdamW
    from mvp.train import train_objectness_step

    amp = float(g["traj__amp"])
    probe = _probe(g, "traj", dev, head_type="linear", kernel_size=1, output_dim=1)
    opt = FlatAdamW([{"params": probe.parameters(), "lr": 5e-4}])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda e: cosine_decay_linear_warmup(e, 30, 2))
    losses = []
    for s in range(8):
        feats = [torch.from_numpy(f).to(dev) for f in g["traj__feats"][s]]
        loss = train_objectness_step(None, probe, opt, sched, None, torch.from_numpy(g["traj__masks"][s]).to(dev), feats=feats)
        losses.append(loss.item())
    print("trajectory losses rel", np.abs(np.array(losses) / g["traj__losses"] - 1).max())
    np.testing.assert_allclose(losses, g["traj__losses"], rtol=1e-4 * amp)
    lr_sum = sum(5e-4 * cosine_decay_linear_warmup(e, 30, 2) for e in range(8))
    for n, p in probe.state_dict().items():
        ref = g[f"traj__final__{n}"]
        if n == "head.conv.bias":
            # gradient exactly zero (the batch mean absorbs a constant): AdamW steps on the sign of rounding noise, about one learning
            # rate per step, in the reference as here.  Not reproducible, only bounded (tests/test_objectness_cpu.py has the argument).
            assert abs(p.item() - ref.item()) <= 2 * lr_sum
        elif n == "batch_norm.running_mean":
            np.testing.assert_allclose(p.cpu().numpy(), ref, atol=2 * lr_sum + 1e-4 * amp * np.abs(ref).max())  # carries that bias
        elif n == "batch_norm.num_batches_tracked":
            assert int(p) == int(ref) == 8
        else:
            e = rel_l2(p.cpu().numpy(), ref)
            print("final", n, e)
            assert e <= 1e-4 * amp, (n, e)


class _TinyBackbone(torch.nn.Module):
    """Stands in for a frozen backbone: four 8-channel maps at a quarter of the resolution (average pooling and fixed mixes)."""

    feat_dim = [8] * 4

    def forward(self, images):
        x = torch.nn.functional.avg_pool2d(images, 4)
        base = torch.cat([x, x * x, x[:, :2] * 0.5], dim=1)
        return [base * (1.0 + 0.25 * i) + 0.1 * i for i in range(4)]


def test_validation_equals_the_restatement(dev, g):
    """Two seeded batches: whole-batch counts, equal weight per batch, probe left in train mode (its running statistics move)."""
    from evals.datasets.synthetic import SyntheticVOC
    from mvp import functional as MF
    from mvp.objectness import validation

    probe = _probe(g, "lin_k1", dev, head_type="linear", kernel_size=1, output_dim=1)
    model = _TinyBackbone().to(dev).eval()
    ds = SyntheticVOC("test", num_samples=5, fixed_size=32, seed=1)
    loader = torch.utils.data.DataLoader(ds, batch_size=3, shuffle=False)  # batches of 3 and 2
    avg = validation(model, probe, loader)
    assert probe.training and int(probe.batch_norm.num_batches_tracked) == 2
    want, n = {k: 0.0 for k in avg}, 0
    probe2 = _probe(g, "lin_k1", dev, head_type="linear", kernel_size=1, output_dim=1)
    for batch in loader:
        with torch.no_grad():
            pred = MF.interpolate(probe2(model(batch["original_image"].to(dev))), size=(32, 32), mode="bilinear").cpu().numpy()
        m = R.metrics(*R.counts(pred.reshape(1, -1), batch["gt_binary_mask"].numpy().reshape(1, -1))[0])
        n += 1
        for k in want:
            want[k] = (want[k] * (n - 1) + m[k]) / n
    assert set(avg) == {"F-measure", "IoU", "Accuracy", "CorLoc"}
    assert {k: repr(float(v)) for k, v in avg.items()} == {k: repr(float(v)) for k, v in want.items()}, (avg, want)


def _run(args, cwd):
    p = subprocess.run([sys.executable, os.path.join(PKG, "train_generic_objectness.py")] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-4000:]
    return out


@pytest.mark.timeout(900)
def test_entry_script_trains_validates_and_reloads(tmp_path):
    """`python train_generic_objectness.py ...` as a fresh child process: one epoch of three batches on a small backbone and image."""
    args = ["backbone=dino_b16", "probe.hidden_dim=128", "dataset.fixed_size=64", "dataset.num_samples=6", "batch_size=2", "optimizer=one_epoch",
            "num_workers=0", f"output_dir={tmp_path}/result", "model_name=tiny_run"]
    out = _run(args, str(tmp_path))
    m = re.search(r"epoch 0 train loss ([0-9.einf+-]+|nan)", out)
    assert m and np.isfinite(float(m.group(1))), out[-2000:]
    rows = list(csv.reader(open(tmp_path / "result" / "trained_objectness" / "final_results_summary_voc.csv")))
    assert rows[0] == ["Model Name", "Test Avg F-measure", "Test Avg IoU", "Test Avg Accuracy", "Test Avg CorLoc"]
    assert len(rows) == 2 and rows[1][0] == "tiny_run" and all(0.0 <= float(v) <= 1.0 for v in rows[1][1:]) and len(rows[1]) == 5
    ck = re.search(r"saved (\S+ckpt\.pth)", out).group(1)
    assert os.path.isfile(ck)
    blob = torch.load(ck, map_location="cpu", weights_only=True)
    assert {"batch_norm.weight", "batch_norm.running_var", "batch_norm.num_batches_tracked", "head.out_conv.2.weight"} <= set(blob["probe"])
    test_line = re.search(r"^test .*$", out, flags=re.M).group(0)
    # is_eval=True ckpt_path=...: nothing trained or saved, the same four metrics (validation normalises with batch statistics)
    out2 = _run(args + ["is_eval=True", f"ckpt_path={ck}"], str(tmp_path))
    assert "saved" not in out2 and "epoch 0" not in out2
    assert re.search(r"^test .*$", out2, flags=re.M).group(0) == test_line
    assert len(list(csv.reader(open(tmp_path / "result" / "trained_objectness" / "final_results_summary_voc.csv")))) == 3
