"""Taskonomy probing end to end on the GPU: train_taskonomy_step against the reference's recorded three-step trajectory
(tests/golden/taskonomy.npz) and a torch-autograd restatement on a DPT probe, DeviceTaskTransform against the host transforms,
validation() against the restatement image by image, the pipelined loop against the serial one, and the entry script.

Bounds.  Trajectory: losses rtol 1e-4, final weights rel-L2 1e-4 — tests/test_gpu_objectness.py's trajectory bounds; the fixture's
margin (every valid pixel at least 10 x 1e-4 x rms(pred) away from the L1 kink at every step) makes the sign pattern of the
gradient the reference's.  DPT step: parameter gradients within GRAD_TOL of tests/test_gpu_probe.py, the same margin checked on its
inputs."""
import csv
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import taskonomy_ref as R
from conftest import PKG, load_golden, rel_l2
from test_gpu_probe import GRAD_TOL

pytestmark = pytest.mark.gpu

MARGIN = 10 * 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g():
    return load_golden("taskonomy.npz")


def _golden_probe(g, dev):
    from evals.models.probes import TaskonomyHead

    probe = TaskonomyHead(feat_dim=[8] * 4, head_type="linear", kernel_size=1, pred_type="vanilla", output_dim=3, precision="bf16x3")
    pre = "traj__sd__"
    probe.load_state_dict({k[len(pre):]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith(pre)}, strict=True)
    return probe.to(dev)


def test_train_taskonomy_step_trajectory_vs_reference(dev, g):
    from evals.utils.optim import cosine_decay_linear_warmup
    from mvp.optim import FlatAdamW
    from mvp.train import train_taskonomy_step

    assert float(g["traj__margin"]) >= MARGIN
    probe = _golden_probe(g, dev)
    opt = FlatAdamW([{"params": probe.parameters(), "lr": 5e-4}])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda e: cosine_decay_linear_warmup(e, 30, 2))
    losses = []
    for s in range(3):
        feats = [torch.from_numpy(f).to(dev) for f in g["traj__feats"][s]]
        target, valid = torch.from_numpy(g["traj__targets"][s]).to(dev), torch.from_numpy(g["traj__valids"][s]).to(dev)
        w0 = probe.head.conv.weight.detach().clone()
        loss = train_taskonomy_step(None, probe, opt, sched, None, target, valid, feats=feats)
        losses.append(loss.item())
        if s == 0:
            # channel 2 of the three-channel head is not used by the two-channel target: a gradient of exactly zero, and AdamW's
            # decoupled weight decay alone moves it (w <- w (1 - lr wd) with lr = the first step's 5e-4 x schedule(0))
            assert float(probe.head.conv.weight.grad[2].abs().max()) == 0.0 and float(probe.head.conv.bias.grad[2]) == 0.0
            assert float((probe.head.conv.weight.grad[:2].abs().max())) > 0.0
            lr0 = 5e-4 * cosine_decay_linear_warmup(0, 30, 2)
            assert torch.allclose(probe.head.conv.weight.detach()[2], w0[2] * (1 - lr0 * 0.01), rtol=1e-6, atol=0)
    print("trajectory losses", losses, "rel", np.abs(np.array(losses) / g["traj__losses"] - 1).max())
    np.testing.assert_allclose(losses, g["traj__losses"], rtol=1e-4)
    for n, p in probe.state_dict().items():
        e = rel_l2(p.cpu().numpy(), g[f"traj__final__{n}"])
        print("final", n, e)
        assert e <= 1e-4, (n, e)


def test_output_dim_below_the_target_is_refused(dev, g):
    from mvp.train import train_taskonomy_step

    probe = _golden_probe(g, dev)
    feats = [torch.from_numpy(f).to(dev) for f in g["traj__feats"][0]]
    opt = torch.optim.SGD(probe.parameters(), lr=0.1)
    with pytest.raises(ValueError, match="output channels"):
        train_taskonomy_step(None, probe, opt, None, None, torch.zeros(2, 4, 24, 24, device=dev), torch.ones(2, 1, 24, 24, dtype=torch.bool, device=dev),
                             feats=feats)


def test_dpt_step_equals_torch_autograd(dev):
    """One step's loss and parameter gradients of TaskonomyHead(dpt, k = 3, vanilla, 3 channels) on a 2-channel target against the CPU
    oracle's DPT + the restated loss under torch autograd, on the same weights."""
    from evals.models.probes import TaskonomyHead
    from mvp import functional as MF
    from oracle import probes as oprobes

    C, B, h, w = 128, 2, 3, 4
    gen = torch.Generator().manual_seed(2024)
    feats = [torch.randn(B, C, h, w, generator=gen) for _ in range(4)]
    H, W = 40, 56
    sd = oprobes.make_dpt_weights([C] * 4, 3, hidden=C, k=3, seed=61)
    sd_r = {n: t.clone().double().requires_grad_(True) for n, t in sd.items()}
    low = oprobes.dpt_head(sd_r, [f.double() for f in feats], 3)
    valid = torch.rand(B, 1, H, W, generator=gen) < 0.9
    # a target that keeps clear of the prediction: the L1 kink further than the margin from every valid pixel
    with torch.no_grad():
        pred0 = torch.nn.functional.interpolate(low[:, :2], size=(H, W), mode="bilinear", align_corners=False)
        rms = float(pred0.pow(2).mean().sqrt())
        sign = torch.where(torch.rand(B, 2, H, W, generator=gen) < 0.5, -1.0, 1.0).double()
        target = (pred0 + sign * rms * (0.05 + torch.rand(B, 2, H, W, generator=gen).double())).float()
    assert R.margin(pred0, target, valid) >= MARGIN
    loss_r, _ = R.step_loss(low, target.double(), valid)
    loss_r.backward()
    probe = TaskonomyHead(feat_dim=[C] * 4, head_type="dpt", hidden_dim=C, kernel_size=3, pred_type="vanilla", output_dim=3, precision="bf16x3")
    probe.load_state_dict(sd, strict=True)
    probe = probe.to(dev)
    out = probe([f.to(dev) for f in feats])
    assert tuple(out.shape) == tuple(low.shape)
    pred = MF.interpolate(out[:, :2], size=(H, W), mode="bilinear", align_corners=False)
    loss = MF.masked_l1_loss(pred, target.to(dev), valid.to(dev))
    MF.backward(loss)
    torch.cuda.synchronize()
    assert rel_l2(out.detach().cpu().numpy(), low.detach().numpy()) < 1e-4
    assert abs(float(loss.detach()) - float(loss_r.detach())) <= 1e-4 * abs(float(loss_r.detach()))
    worst = 0.0
    for n, p in probe.named_parameters():
        ref = sd_r[n].grad.numpy()
        if n.startswith("head.out_conv.2."):
            assert float(p.grad[2:].abs().max()) == 0.0 and float(np.abs(ref[2:]).max()) == 0.0  # the unused third channel
        e = rel_l2(p.grad.cpu().numpy(), ref)
        worst = max(worst, e)
        print(f"dpt step grad {n}: rel-L2 {e:.2e}")
    print(f"dpt step: loss hip {float(loss.detach()):.8f} autograd {float(loss_r.detach()):.8f}, worst parameter-gradient rel-L2 {worst:.2e} (bound {GRAD_TOL})")
    assert worst <= GRAD_TOL


def _loader(task, n, hw, bs, raw):
    from evals.datasets.synthetic import SyntheticTaskonomy

    return torch.utils.data.DataLoader(SyntheticTaskonomy("test", task, n, hw, raw=raw, seed=3), batch_size=bs, shuffle=False)


@pytest.mark.parametrize("task,hw", [("principal_curvature", (32, 48)), ("normal", (30, 34)), ("reshading", (32, 32)), ("depth_euclidean", (32, 48)),
                                     ("edge_texture", (18, 23)), ("keypoints2d", (16, 16))])
def test_device_transform_equals_the_host_transform(dev, task, hw):
    from mvp.prefetch import DevicePrefetcher
    from mvp.taskonomy import DeviceTaskTransform
    from test_gpu_augment_kernels import jitter_tolerance

    tol = jitter_tolerance()  # the augment kernel's normalise tolerance
    got = list(DeviceTaskTransform(DevicePrefetcher(_loader(task, 5, hw, 2, True), dev), task))
    want = list(_loader(task, 5, hw, 2, False))
    assert len(got) == len(want) == 3
    for a, b in zip(got, want):
        assert set(a) == {"rgb", task, "mask_valid"}
        assert np.array_equal(a[task].cpu().numpy().view(np.uint32), b[task].numpy().view(np.uint32))
        assert a["mask_valid"].dtype == torch.uint8 and np.array_equal(a["mask_valid"].cpu().numpy().astype(bool), b["mask_valid"].numpy())
        err = float((a["rgb"].cpu().double() - b["rgb"].double()).abs().max())
        assert tuple(a["rgb"].shape) == tuple(b["rgb"].shape) and err <= tol, err


class _TinyBackbone(torch.nn.Module):
    """Stands in for a frozen backbone: four 8-channel maps at a quarter of the resolution (average pooling and fixed mixes)."""

    feat_dim = [8] * 4

    def forward(self, images):
        x = torch.nn.functional.avg_pool2d(images, 4)
        base = torch.cat([x, x * x, x[:, :2] * 0.5], dim=1)
        return [base * (1.0 + 0.25 * i) + 0.1 * i for i in range(4)]


@pytest.mark.parametrize("task", ["principal_curvature", "normal", "depth_euclidean"])
def test_validation_equals_the_restatement(dev, g, task):
    """Five images in batches of 2, 2, 1: the mean over IMAGES of the per-image metrics, probe in eval mode and put back."""
    from mvp import functional as MF
    from mvp.prefetch import DevicePrefetcher
    from mvp.taskonomy import DeviceTaskTransform, metric_keys, target_channels, validation

    probe = _golden_probe(g, dev)
    model = _TinyBackbone().to(dev).eval()
    avg = validation(model, probe, DeviceTaskTransform(DevicePrefetcher(_loader(task, 5, (32, 48), 2, True), dev), task), task)
    assert probe.training and list(avg) == metric_keys(task)
    ct = target_channels(task)
    rows = []
    # the same device batches (test_device_transform_equals_the_host_transform holds them to the host transforms): the prediction the
    # restatement sees is the one validation() saw, bit for bit
    for batch in DeviceTaskTransform(DevicePrefetcher(_loader(task, 5, (32, 48), 2, True), dev), task):
        with torch.no_grad():
            pred = MF.interpolate(probe(model(batch["rgb"]))[:, :ct], size=(32, 48), mode="bilinear").cpu()
        target, valid = batch[task].cpu(), batch["mask_valid"].cpu()
        for i in range(pred.shape[0]):  # image by image
            form = "curvature" if task == "principal_curvature" else "reshading"
            sums = R.metric_sums(pred[i:i + 1], target[i:i + 1], valid[i:i + 1], form)
            rows.append(R.curvature_metrics(sums) if form == "curvature" else R.reshading_metrics(sums))
    assert len(rows) == 5
    for k in avg:
        want = float(np.mean([float(r[k]) for r in rows]))
        # the sums are fp64 in another order (1e-12) and the per-image values pass through fp32 once (6e-8)
        assert abs(avg[k] - want) <= 1e-6 * max(abs(want), 1e-12), (k, avg[k], want)


def test_pipelined_loop_equals_the_serial_loop(dev, g):
    from evals.utils.optim import cosine_decay_linear_warmup
    from mvp.optim import FlatAdamW
    from mvp.pipeline import pipelined_features
    from mvp.prefetch import DevicePrefetcher
    from mvp.taskonomy import DeviceTaskTransform
    from mvp.train import train_taskonomy_step

    task = "principal_curvature"
    model = _TinyBackbone().to(dev).eval()
    results = []
    for pipelined in (False, True):
        probe = _golden_probe(g, dev)
        opt = FlatAdamW([{"params": probe.parameters(), "lr": 5e-4}])
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda e: cosine_decay_linear_warmup(e, 30, 2))
        batches = DeviceTaskTransform(DevicePrefetcher(_loader(task, 6, (32, 48), 2, True), dev), task)
        losses = []
        for _ in range(2):
            if pipelined:
                for batch, feats in pipelined_features(model, batches, image_key="rgb", probe=probe):
                    losses.append(train_taskonomy_step(model, probe, opt, sched, None, batch[task], batch["mask_valid"], feats=feats).item())
            else:
                for batch in batches:
                    losses.append(train_taskonomy_step(model, probe, opt, sched, batch["rgb"], batch[task], batch["mask_valid"]).item())
        opt.finish_pending()
        torch.cuda.synchronize()
        results.append((losses, {n: p.detach().cpu().numpy().tobytes() for n, p in probe.state_dict().items()}))
    assert len(results[0][0]) == 6 and all(np.isfinite(results[0][0]))
    assert [repr(v) for v in results[0][0]] == [repr(v) for v in results[1][0]]
    assert results[0][1] == results[1][1]


def _run(args, cwd):
    p = subprocess.run([sys.executable, os.path.join(PKG, "train_taskonomy.py")] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-4000:]
    return out


@pytest.mark.timeout(900)
def test_entry_script_trains_validates_and_reloads(tmp_path):
    """`python train_taskonomy.py ...` as a fresh child process: one epoch of three batches on a small backbone and image."""
    from mvp.taskonomy import metric_keys

    args = ["backbone=dino_b16", "+probe.hidden_dim=128", "dataset.image_size=[64,64]", "dataset.num_samples=6", "batch_size=2", "optimizer=one_epoch",
            "num_workers=0", f"output_dir={tmp_path}/result", "experiment_model=tiny_run"]
    out = _run(args, str(tmp_path))
    m = re.search(r"epoch 0 train loss ([0-9.einf+-]+|nan)", out)
    assert m and np.isfinite(float(m.group(1))), out[-2000:]
    path = tmp_path / "result" / "result" / "taskonomy-principal_curvature" / "results.csv"
    rows = list(csv.reader(open(path)))
    assert rows[0] == ["Model Name"] + metric_keys("principal_curvature") and "δ1.25_avg" in rows[0]
    assert len(rows) == 2 and rows[1][0] == "tiny_run" and all(np.isfinite(float(v)) for v in rows[1][1:]) and len(rows[1]) == 11
    ck = re.search(r"saved (\S+ckpt\.pth)", out).group(1)
    assert os.path.isfile(ck) and ck.endswith("_principal_curvature/ckpt.pth") and "taskonomy_exps" in ck
    blob = torch.load(ck, map_location="cpu", weights_only=True)
    assert "head.out_conv.2.weight" in blob["probe"] and blob["probe"]["head.out_conv.2.weight"].shape[0] == 3
    test_line = re.search(r"^test .*$", out, flags=re.M).group(0)
    # is_eval=True ckpt_path=...: nothing trained or saved, the same metrics (the probe is validated in eval mode)
    out2 = _run(args + ["is_eval=True", f"ckpt_path={ck}"], str(tmp_path))
    assert "saved" not in out2 and "epoch 0" not in out2
    assert re.search(r"^test .*$", out2, flags=re.M).group(0) == test_line
    assert len(list(csv.reader(open(path)))) == 3
