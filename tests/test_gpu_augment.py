"""mvp.augment.DeviceAugment end to end on the GPU: raw uint8 samples (SyntheticNYURaw) -> DataLoader -> DevicePrefetcher -> the two
augmentation launches -> the reference's batch dict, against tests/augment_ref.py applied with sample_params of the same seed; the
stream ordering against the pipelined frozen forward (train() == the same loop forced serial, bit for bit); the entry script."""
import csv
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import augment_ref
from test_gpu_augment_kernels import jitter_tolerance, normalised

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "midvision-probe_amd")
HW = (64, 96)


def _loader(n=10, B=4, hw=HW):
    from torch.utils.data import DataLoader

    from evals.datasets import SyntheticNYURaw

    return DataLoader(SyntheticNYURaw("train", num_samples=n, image_size=hw), B, shuffle=False, num_workers=0)


def _augmented(loader, **kw):
    from mvp.augment import DeviceAugment
    from mvp.prefetch import DevicePrefetcher

    kw.setdefault("image_mean", "imagenet")
    kw.setdefault("seed", 7)
    return DeviceAugment(DevicePrefetcher(loader, torch.device("cuda:0")), **kw)


def _collect(it):
    out = [{k: v.cpu() if torch.is_tensor(v) else v for k, v in b.items()} for b in it]
    torch.cuda.synchronize()
    return out


def test_batches_honour_the_contract_and_equal_the_reference():
    loader = _loader()
    aug = _augmented(loader)
    assert len(aug) == len(loader) == 3 and not hasattr(aug, "consumer_lag")
    got = _collect(aug)
    host = list(loader)
    tol = jitter_tolerance()
    assert [b["image"].shape[0] for b in got] == [4, 4, 2]
    jittered = cropped = 0
    for i, (g, h) in enumerate(zip(got, host)):
        B = h["image"].shape[0]
        assert set(g) == {"image", "depth", "snorm", "segmentation"}
        assert g["image"].shape == (B, 3, *HW) and g["depth"].shape == (B, 1, *HW) and g["snorm"].shape == (B, 3, *HW)
        assert g["image"].dtype == g["depth"].dtype == g["snorm"].dtype == torch.float32
        assert g["segmentation"].dtype == torch.int64 and torch.equal(g["segmentation"], h["segmentation"])
        params = aug.params_for(0, i, B, *HW)
        ref_img, ref_dep, ref_sn, tie = augment_ref.apply(h["image"], h["depth"], h["snorm"], params, HW, "imagenet")
        assert not tie.any()  # rotateflip is off, as in the reference's NYU path
        assert torch.equal(g["depth"], ref_dep) and torch.equal(g["snorm"], ref_sn)  # a pure gather
        assert torch.equal(g["depth"] == 0, ref_dep == 0) and (g["depth"] == 0).any()
        for b in range(B):  # no new values appear
            assert torch.isin(g["depth"][b], h["depth"][b]).all() and torch.isin(g["snorm"][b], h["snorm"][b]).all()
        err = float((g["image"].double() - ref_img).abs().max())
        print(f"[augment e2e] batch {i}: image max abs err {err:.3e} (tolerance {tol:.3e})")
        assert err <= tol
        from mvp.augment import unpack_params

        es = unpack_params(params)
        jittered += sum(e["jitter"] for e in es)
        cropped += sum(e["box"] != (0, 0, HW[1], HW[0]) for e in es)
    assert jittered >= 5 and 1 <= cropped <= 9  # the draws do augment: p = 0.8 and 0.5 over ten images


def test_same_seed_same_bits_and_epochs_differ():
    loader = _loader()
    a = _collect(_augmented(loader))
    b = _collect(_augmented(loader))
    assert all(torch.equal(x[k], y[k]) for x, y in zip(a, b) for k in x)
    aug = _augmented(loader)
    first = _collect(aug)
    second = _collect(aug)  # a pass without set_epoch advances the epoch: single-process training does not repeat its draws
    assert all(torch.equal(x[k], y[k]) for x, y in zip(a, first) for k in x)
    assert not all(torch.equal(x["image"], y["image"]) for x, y in zip(first, second))
    aug.set_epoch(0)
    again = _collect(aug)
    assert all(torch.equal(x[k], y[k]) for x, y in zip(first, again) for k in x)
    aug.sampler.set_epoch(1)  # what train() calls on a loader
    assert all(torch.equal(x[k], y[k]) for x, y in zip(second, _collect(aug)) for k in x)
    other = _collect(_augmented(loader, seed=8))
    assert not all(torch.equal(x["image"], y["image"]) for x, y in zip(a, other))
    rank1 = _collect(_augmented(loader, rank=1))
    assert not all(torch.equal(x["image"], y["image"]) for x, y in zip(a, rank1))


def test_augment_off_is_plain_normalisation():
    loader = _loader(n=6)
    for mean in ("imagenet", "clip", None):
        got = _collect(_augmented(loader, augment=False, image_mean=mean))
        for g, h in zip(got, loader):
            assert torch.equal(g["image"], normalised(h["image"], mean)) and torch.equal(g["depth"], h["depth"])
            assert torch.equal(g["snorm"], h["snorm"]) and torch.equal(g["segmentation"], h["segmentation"])


def test_rotateflip_draws_reach_the_kernel():
    loader = _loader(n=8)
    aug = _augmented(loader, rotateflip=True, seed=3)
    got = _collect(aug)
    host = list(loader)
    tol = jitter_tolerance()
    for i, (g, h) in enumerate(zip(got, host)):
        params = aug.params_for(0, i, h["image"].shape[0], *HW)
        ref_img, ref_dep, ref_sn, tie = augment_ref.apply(h["image"], h["depth"], h["snorm"], params, HW, "imagenet")
        ok = ~tie
        assert torch.equal(g["depth"][:, 0][ok], ref_dep[:, 0][ok])
        keep = ok.unsqueeze(1).expand_as(ref_sn)
        assert torch.equal(g["snorm"][keep], ref_sn[keep])
        assert float((g["image"].double() - ref_img)[keep].abs().max()) <= tol


def _build(dev):
    from evals.models.dino import DINO
    from evals.models.probes import DepthHead
    from evals.utils.optim import cosine_decay_linear_warmup
    from mvp.optim import FlatAdamW
    from oracle import vit as ovit

    model = DINO(return_multilayer=True, add_norm=True, weights=ovit.make_vit_weights(embed_dim=128, depth=4, seed=1)).to(dev)
    torch.manual_seed(11)
    probe = DepthHead(feat_dim=model.feat_dim, head_type="linear", kernel_size=1, prediction_type="bindepth", min_depth=0.001, max_depth=10).to(dev)
    opt = FlatAdamW([{"params": probe.parameters(), "lr": 1e-3}])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda e: cosine_decay_linear_warmup(e, 100, 10))
    return model, probe, opt, sched


def test_train_over_the_augmented_loader_matches_the_serial_loop(monkeypatch):
    """Two epochs of train() with the forwards of the next batches in flight on side streams while the augmentation launches of later
    batches are issued on the caller's stream, against the same loop forced serial (MVP_INFLIGHT=1): the same losses and weights, bit
    for bit — the side-stream forward never reads an image the augmentation has not finished, and no buffer is recycled under it."""
    from evals.utils.losses import DepthLoss
    from mvp.train import train

    dev = torch.device("cuda:0")
    loader = _loader(n=22, B=4, hw=(64, 64))

    def run():
        model, probe, opt, sched = _build(dev)
        hist = train(model, probe, _augmented(loader, seed=5), opt, sched, 2, True, DepthLoss())
        opt.finish_pending()
        torch.cuda.synchronize()
        return hist, opt.flat_param.cpu().numpy().copy(), model.batchnorms[2].running_var.cpu().numpy().copy()

    monkeypatch.setenv("MVP_INFLIGHT", "1")
    ref = run()
    monkeypatch.delenv("MVP_INFLIGHT")
    got = run()
    assert len(ref[0]) == 2 and all(np.isfinite(ref[0])) and ref[0][0] != ref[0][1]
    assert got[0] == ref[0]
    np.testing.assert_array_equal(got[1], ref[1])
    np.testing.assert_array_equal(got[2], ref[2])


@pytest.mark.timeout(900)
def test_train_depth_entrypoint_with_the_augmented_choice(tmp_path):
    args = ["backbone=dino_b16", "+backbone.return_multilayer=True", "probe=depth_linear", "dataset=synthetic_aug", "dataset.image_size=[64,64]",
            "dataset.num_batches=3", "batch_size=2", "optimizer=one_epoch", "num_workers=0", f"output_dir={tmp_path}/result"]
    p = subprocess.run([sys.executable, os.path.join(PKG, "train_depth.py")] + args, cwd=str(tmp_path), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-4000:]
    assert "SA valid loss" in out and "results ->" in out and "saved" in out
    files = glob.glob(str(tmp_path / "result" / "result" / "depth" / "*.csv"))
    assert len(files) == 1
    rows = list(csv.reader(open(files[0])))
    assert len(rows) == 2 and os.path.isfile(rows[1][-1])
    assert float(rows[1][rows[0].index("rmse SA")]) > 0


@pytest.mark.timeout(900)
def test_train_snorm_entrypoint_with_the_augmented_choice(tmp_path):
    """The normals go through the same gather as the image; the validation batch of the raw loader is normalised on the device."""
    args = ["backbone=dino_b16", "+backbone.return_multilayer=True", "probe=snorm_dpt", "probe.hidden_dim=128", "dataset=synthetic_aug",
            "dataset.image_size=[64,64]", "dataset.num_batches=3", "batch_size=2", "optimizer=one_epoch", "num_workers=0",
            f"output_dir={tmp_path}/result"]
    p = subprocess.run([sys.executable, os.path.join(PKG, "train_snorm.py")] + args, cwd=str(tmp_path), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-4000:]
    assert "epoch 0 train loss" in out and "valid d1" in out and "saved" in out
