"""CPU checks of the pixel-level 2AFC baselines (csrc/pixelsim.hip, mvp/percept.py, evals/models/pixel_metrics.py,
evals/utils/losses.py): the fp64 definition of tests/pixelsim_ref.py against the reference's recorded outputs (tests/golden/ssim.npz),
the window, the ABI boundary of mvp_pixel_score, the config choices, the synthetic dataset and the refusals."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import pixelsim_ref as ref
from conftest import PKG, REPO

CASES = ["noise_1x1x7x9", "smooth_2x3x5x5", "noise_1x2x13x12", "smooth_2x3x24x20"]


@pytest.mark.parametrize("case", CASES)
def test_fp64_restatement_equals_the_recorded_reference(golden, case):
    z = golden("ssim.npz")
    a, b = torch.from_numpy(z[f"{case}__a"]), torch.from_numpy(z[f"{case}__b"])
    assert float(a.min()) >= 0 and float(a.max()) <= 1 and torch.equal((a * 255).round() / 255, a)  # the 8-bit grid
    per = ref.ssim(a, b)
    err = float((per - torch.from_numpy(z[f"{case}__per64"])).abs().max())
    err_all = abs(float(per.mean()) - float(z[f"{case}__all64"]))  # one image size: the mean of the per-image means is the global mean
    print(f"{case}: |ssim64 - recorded fp64| = {err:.2e} per image, {err_all:.2e} averaged")
    assert err <= 1e-12 and err_all <= 1e-12
    # the fp32 restatement is the reference's fp32 evaluation up to the order of the last mean
    assert float((ref.ssim_fp32(a, b).double() - torch.from_numpy(z[f"{case}__per32"]).double()).abs().max()) <= 2.0 ** -22


def test_window_is_the_references_to_the_bit(golden):
    from evals.utils import losses

    rec = torch.from_numpy(golden("ssim.npz")["window"])
    assert rec.shape == (1, 1, 11, 11) and rec.dtype == torch.float32
    assert torch.equal(losses.create_window(11, 1), rec) and torch.equal(ref.window2d(), rec[0, 0])
    w3 = losses.create_window(11, 3)
    assert w3.shape == (3, 1, 11, 11) and w3.is_contiguous() and all(torch.equal(w3[c], rec[0]) for c in range(3))
    g = losses.gaussian(11, 1.5)
    assert g.dtype == torch.float32 and torch.equal(g, ref.window1d()) and torch.equal(g.unsqueeze(1).mm(g.unsqueeze(0)), rec[0, 0])
    # the eleven literals the kernel holds
    src = open(os.path.join(PKG, "csrc", "pixelsim.hip")).read()
    body = re.search(r"PX_G\[PX_TAPS\] = \{(.*?)\};", src, flags=re.S).group(1)
    lits = [float.fromhex(v.rstrip("f")) for v in re.findall(r"0x[0-9a-f.]+p-?\d+f", body)]
    assert len(lits) == 11 and torch.equal(torch.tensor(lits, dtype=torch.float64), g.double())


def test_symbols_are_exported_declared_and_bound():
    from mvp import lib, ops, percept

    header = open(os.path.join(REPO, "include", "mvp_hip.h")).read()
    so = lib.load()
    for name in ("mvp_pixel_score", "mvp_pixel_score_workspace_bytes"):
        assert re.search(r"^\s*(?:int|int64_t)\s+" + name + r"\s*\(", header, flags=re.M), name
        assert name in lib.SYMBOLS and hasattr(so, name)
    assert lib.SYMBOLS["mvp_pixel_score"] is lib.PixelScoreArgs and lib.STRUCTS["mvp_pixel_score_args"] is lib.PixelScoreArgs
    assert "struct mvp_pixel_score_args {" in header and so.mvp_sizeof(b"mvp_pixel_score_args") == ctypes.sizeof(lib.PixelScoreArgs)
    assert "Added within 8: mvp_pixel_score" in header and lib.info().abi_version == 8
    assert ops.PIXEL_METRICS == {"psnr": 0, "ssim": 1} and callable(ops.pixel_score) and callable(percept.score_pixel_triplets)


def _args(**kw):
    """Arguments mvp_pixel_score accepts up to the launch (never launched here): fake 16-byte aligned addresses."""
    from mvp import lib

    base = dict(ref=4096, left=8192, right=12288, label=256, sim=512, pred=1024, counts=2048, workspace=16384, ld=3 * 20 * 40,
                B=2, C=3, H=20, W=40, metric=1, accumulate=0)
    base.update(kw)
    base.setdefault("workspace_bytes", max(16, lib.load().mvp_pixel_score_workspace_bytes(base["B"], base["C"], base["H"], base["W"],
                                                                                          base["metric"])))
    return lib.PixelScoreArgs(**base)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("bad", [
    dict(ref=None), dict(left=None), dict(right=None), dict(sim=None), dict(pred=None),
    dict(label=None),                       # counts without label
    dict(B=0), dict(B=-1), dict(C=0), dict(C=-3), dict(H=0), dict(H=-1), dict(W=0), dict(W=-2),
    dict(ld=3 * 20 * 40 - 1),               # ld < C * H * W
    dict(C=2, H=32768, W=32768, ld=1 << 31, workspace_bytes=1 << 40),  # C * H * W = 2^31 > 2^31 - 1
    dict(C=1 << 20, H=1 << 20, W=1 << 20, ld=1 << 62, workspace_bytes=1 << 40),
    dict(metric=2), dict(metric=-1),
    dict(workspace=None), dict(workspace=16384 + 4), dict(workspace_bytes="short"), dict(workspace_bytes=0),
    dict(counts=2048 + 4),
], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()) if isinstance(d, dict) else str(d))
def test_bad_arguments_return_einval(bad, metric):
    from mvp import lib

    so = lib.load()
    bad = dict(bad)
    bad.setdefault("metric", metric)
    if bad.get("workspace_bytes") == "short":
        bad["workspace_bytes"] = so.mvp_pixel_score_workspace_bytes(2, 3, 20, 40, metric) - 1
    assert so.mvp_pixel_score(ctypes.byref(_args(**bad)), None) == -1
    assert so.mvp_pixel_score(None, None) == -1


def test_workspace_bytes():
    from mvp import lib

    ws = lib.load().mvp_pixel_score_workspace_bytes
    for m in (0, 1):
        for B, C, H, W in [(0, 3, 8, 8), (-1, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, 0), (1, -3, 8, 8), (1, 3, -8, -8),
                           (1, 2, 32768, 32768), (1, 1 << 20, 1 << 20, 1 << 20), (1, 1 << 30, 2, 1)]:
            assert ws(B, C, H, W, m) == 0, (B, C, H, W, m)
        for shape in [(1, 1, 1, 1), (2, 3, 5, 5), (16, 3, 224, 224), (16, 3, 512, 512), (3, 3, 33, 31), (1, 1, 1, (1 << 31) - 1)]:
            n = ws(*shape, m)
            assert n > 0 and n % 8 == 0, (shape, m, n)
    assert ws(1, 3, 8, 8, 2) == 0 and ws(1, 3, 8, 8, -1) == 0
    # SSIM: 16 bytes per (triplet, channel, 16 x 32 tile); PSNR: 16 bytes per (triplet, chunk of >= 4096 elements), <= 1024 chunks
    assert ws(1, 1, 1, 1, 1) == 16 and ws(2, 3, 16, 32, 1) == 2 * 3 * 16 and ws(2, 3, 17, 33, 1) == 2 * 3 * 4 * 16
    assert ws(16, 3, 224, 224, 1) == 16 * 3 * 14 * 7 * 16
    assert ws(1, 1, 1, 1, 0) == 16 and ws(2, 1, 64, 64, 0) == 2 * 16 and ws(2, 1, 64, 65, 0) == 2 * 2 * 16
    assert ws(16, 3, 224, 224, 0) == 16 * 37 * 16 and ws(1, 3, 4096, 4096, 0) == 768 * 16  # 65536-element chunks


@pytest.mark.parametrize("name", ["psnr", "ssim"])
def test_choice_files_compose_and_instantiate_without_a_device(name):
    from mvp import config

    cfg = config.compose("model_percepture", [f"backbone={name}", "backbone.return_cls=True", f"dataset.preprocess={name.upper()}",
                                              f"experiment_model={name}"])
    assert cfg["dataset"]["preprocess"] == name.upper() and cfg["experiment_model"] == name
    assert config.compose("model_percepture")["dataset"]["preprocess"] == "DEFAULT"
    model = config.instantiate(cfg["backbone"])
    assert isinstance(model, torch.nn.Module) and list(model.parameters()) == [] and list(model.buffers()) == []
    assert model.arch == "metric" and model.metric == name and model.checkpoint_name == f"${name}$" and model.preprocess == name.upper()
    from evals.models import PSNR, SSIM
    from evals.models.pixel_metrics import PixelMetric

    assert type(model) is {"psnr": PSNR, "ssim": SSIM}[name] and isinstance(model, PixelMetric)
    type(model)(return_cls=True, return_multilayer=True, output="gap", layer=3)  # accepted, ignored
    ds = config.instantiate(cfg["dataset"], split="test")
    assert ds.preprocess == name.upper() and float(ds[0][0].min()) >= 0.0 and float(ds[0][0].max()) <= 1.0


@pytest.mark.parametrize("seed", [0, 3, 11])
def test_default_items_are_what_they_were(seed):
    """The formula of the dataset before it had ``preprocess``, restated."""
    from mvp.percept import SyntheticTwoAFC

    for ds in (SyntheticTwoAFC(5, image_size=(6, 9), seed=seed), SyntheticTwoAFC(5, image_size=(6, 9), seed=seed, preprocess="DEFAULT")):
        for i in range(5):
            g = torch.Generator().manual_seed(seed * 7919 + i)
            r = torch.randn(3, 6, 9, generator=g)
            near = r + 0.05 * torch.randn(3, 6, 9, generator=g)
            far = torch.randn(3, 6, 9, generator=g)
            p = int(torch.randint(0, 2, (1,), generator=g))
            left, right = (far, near) if p == 1 else (near, far)
            got = ds[i]
            assert torch.equal(got[0], r) and torch.equal(got[1], left) and torch.equal(got[2], right)
            assert isinstance(got[3], np.float32) and got[3] == p and got[4] == i
    with pytest.raises(ValueError, match="preprocess"):
        SyntheticTwoAFC(2, preprocess="CLIP")


@pytest.mark.parametrize("pre", ["SSIM", "PSNR"])
@pytest.mark.parametrize("size", [24, (48, 40)])
def test_eight_bit_items_grid_determinism_and_margins(pre, size):
    from mvp.percept import SyntheticTwoAFC

    ds = SyntheticTwoAFC(32, image_size=size, seed=0, preprocess=pre)
    items = [ds[i] for i in range(32)]
    hw = (size, size) if isinstance(size, int) else size
    for i, (r, left, right, p, idx) in enumerate(items):
        for t in (r, left, right):
            assert t.shape == (3, *hw) and t.dtype == torch.float32
            assert float(t.min()) >= 0.0 and float(t.max()) <= 1.0 and torch.equal((t * 255).round() / 255, t)
        assert isinstance(p, np.float32) and p in (0.0, 1.0) and idx == i
    again = SyntheticTwoAFC(40, image_size=size, seed=0, preprocess=pre)  # (seed, i) alone: not the length, not the order of access
    for i in (31, 0, 7):
        assert all(torch.equal(torch.as_tensor(a), torch.as_tensor(b)) for a, b in zip(again[i], items[i]))
    other = SyntheticTwoAFC(32, image_size=size, seed=1, preprocess=pre)
    assert not torch.equal(other[0][0], items[0][0]) and not torch.equal(items[1][0], items[0][0])
    assert torch.equal(SyntheticTwoAFC(1, image_size=size, preprocess="SSIM")[0][0], SyntheticTwoAFC(1, image_size=size, preprocess="PSNR")[0][0])
    r, left, right = (torch.stack([it[k] for it in items]) for k in range(3))
    p = torch.tensor([float(it[3]) for it in items])
    assert set(p.tolist()) == {0.0, 1.0}
    for metric, margin in (("ssim", 1e-3), ("psnr", 1e-2)):
        sim, pred = ref.score(r, left, right, metric)
        gap = torch.where(p == 1, sim[:, 1] - sim[:, 0], sim[:, 0] - sim[:, 1])  # near minus far
        print(f"{pre} {size} {metric}: near - far between {float(gap.min()):.4g} and {float(gap.max()):.4g}")
        assert (gap >= margin).all(), gap  # every item: none is excused
        assert torch.equal(pred.float(), p)  # the label is the closer side


def test_losses_ssim_refuses_what_is_not_compiled_in():
    from evals.utils import losses

    x = torch.rand(1, 3, 8, 8)
    with pytest.raises(NotImplementedError, match="11"):
        losses.ssim(x, x, window_size=7)
    with pytest.raises(NotImplementedError, match="11"):
        losses.SSIM(window_size=7)
    with pytest.raises(NotImplementedError, match="forward only"):
        losses.ssim(x.clone().requires_grad_(), x)
    with pytest.raises(Exception, match="no CPU fallback"):
        losses.ssim(x, x)  # host tensors
    assert losses.SSIM().window_size == 11 and losses.SSIM(size_average=False).size_average is False


def test_score_pixel_triplets_refusals_on_the_host():
    from mvp import lib, percept

    x = torch.rand(2, 3, 8, 8)
    with pytest.raises(lib.MvpError, match="no CPU fallback"):
        percept.score_pixel_triplets(x, x, x, "ssim")
    with pytest.raises(ValueError, match="metric"):
        percept.score_pixel_triplets(x, x, x, "lpips")


@pytest.mark.parametrize("name", ["psnr", "ssim"])
def test_predict_batch_without_a_device_says_so(name, monkeypatch):
    from evals.models import pixel_metrics
    from mvp import lib, percept

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    ds = percept.SyntheticTwoAFC(2, image_size=8, preprocess=name.upper())
    model = {"psnr": pixel_metrics.PSNR, "ssim": pixel_metrics.SSIM}[name]()
    with pytest.raises(lib.MvpError, match="no CPU fallback"):
        percept.predict_batch(model, torch.utils.data.DataLoader(ds, 2), output_dir=None)


def test_psnr_definition_at_the_edges():
    a = torch.zeros(1, 1, 2, 2)
    assert ref.psnr(a, a).tolist() == [math.inf] and float(ref.psnr(a, a + 1.0)) == 0.0
    assert abs(float(ref.psnr(a, a + 0.1)) - 20.0) < 1e-5  # mse 0.01 (fp32 0.1)
    sim, pred = ref.score(a, a, a, "psnr")
    assert pred.tolist() == [1]  # two +inf
