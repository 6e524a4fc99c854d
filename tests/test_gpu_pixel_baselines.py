"""The pixel-level baselines through the Python surface on the GPU (mvp/percept.py: predict_batch and score_pixel_triplets,
evals/models/pixel_metrics.py, evals/utils/losses.py: ssim / SSIM) against the fp64 definition of tests/pixelsim_ref.py and the
reference's recorded outputs (tests/golden/ssim.npz).  The comparison of predictions is exact: every triplet's two fp64 scores differ
by at least 1e-3 SSIM, resp. 1e-2 dB (asserted), which the kernel's error bounds cannot turn."""
import pytest
import torch

import pixelsim_ref as ref
import twoafc_ref
from test_gpu_percept import _count_device_to_host, _loader, _SomeLabelsFlipped, _vit

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MARGIN = {"ssim": 1e-3, "psnr": 1e-2}
EPS = 2.0 ** -23
CASES = ["noise_1x1x7x9", "smooth_2x3x5x5", "noise_1x2x13x12", "smooth_2x3x24x20"]


def _model(metric):
    from evals.models.pixel_metrics import PSNR, SSIM

    return {"psnr": PSNR, "ssim": SSIM}[metric]()


def _expected(metric, loader):
    """(results, counts) by the fp64 definition, batch by batch."""
    results, counts = [], [0, 0, 0, 0]
    for img_ref, img_left, img_right, p, ids in loader:
        sim64, pred64 = ref.score(img_ref, img_left, img_right, metric)
        assert ((sim64[:, 0] - sim64[:, 1]).abs() >= MARGIN[metric]).all(), sim64  # every triplet: none is excused
        results += [{"id": int(i), "gt": float(g), "prediction": int(q)} for i, g, q in zip(ids, p, pred64)]
        counts = [a + b for a, b in zip(counts, ref.counts(p, pred64))]
    return results, counts


@pytest.mark.parametrize("metric", ["ssim", "psnr"])
def test_predict_batch_ragged_last_batch_one_transfer(metric, monkeypatch):
    from mvp import percept

    # items 0, 7 and 22 get the wrong label, so that FP and FN occur and the four metrics differ
    ds = _SomeLabelsFlipped(percept.SyntheticTwoAFC(24, image_size=48, preprocess="SSIM"), flipped=(0, 7, 22))
    model = _model(metric)
    want, counts = _expected(metric, _loader(ds, 5))  # batches of 5, 5, 5, 5, 4
    calls, to_host = [], percept._to_host
    monkeypatch.setattr(percept, "_to_host", lambda t: (calls.append(tuple(t.shape)), to_host(t))[1])
    with _count_device_to_host() as seen:
        results, metrics, errors = percept.predict_batch(model, _loader(ds, 5), output_dir=None)
    assert len(calls) == 1 and len(seen) == 1, (calls, seen)  # predictions and counts of the whole shard in one transfer, after the loop
    assert errors == [] and results == want and [r["id"] for r in results] == list(range(24))
    assert metrics == percept.metrics_from_counts(*counts) == twoafc_ref.metrics(counts)
    assert metrics == percept.compute_metrics([r["gt"] for r in results], [r["prediction"] for r in results])
    assert sum(counts) == 24 and counts[1] > 0 and counts[2] > 0 and metrics["accuracy"] == 21 / 24, (counts, metrics)


@pytest.mark.parametrize("metric", ["ssim", "psnr"])
def test_module_forward_is_column_zero_of_the_op(metric):
    from mvp import percept

    ds = percept.SyntheticTwoAFC(3, image_size=(20, 36), preprocess="PSNR")
    r, left, right = (torch.stack([ds[i][k] for i in range(3)]).to(DEV) for k in range(3))
    sim, pred = percept.score_pixel_triplets(r, left, right, metric)
    model = _model(metric).to(DEV)
    got = model(r, left)
    assert got.shape == (3,) and got.dtype == torch.float32 and got.is_cuda and got.grad_fn is None
    assert torch.equal(got.view(torch.int32), sim[:, 0].contiguous().view(torch.int32))
    assert torch.equal(model(r, right).view(torch.int32), sim[:, 1].contiguous().view(torch.int32))
    sim64, pred64 = ref.score(r.cpu(), left.cpu(), right.cpu(), metric)
    assert torch.equal(pred.cpu().long(), pred64)


@pytest.mark.parametrize("case", CASES)
def test_losses_ssim_against_the_recorded_reference(golden, case):
    from evals.utils import losses
    from mvp import percept

    z = golden("ssim.npz")
    a, b = torch.from_numpy(z[f"{case}__a"]), torch.from_numpy(z[f"{case}__b"])
    per64, all64 = torch.from_numpy(z[f"{case}__per64"]), float(z[f"{case}__all64"])
    e_ref = float((torch.from_numpy(z[f"{case}__per32"]).double() - per64).abs().max())  # the reference's own fp32 run, recorded
    e_ref = max(e_ref, float((ref.ssim_fp32(a, b).double() - per64).abs().max()))
    bound = max(4 * e_ref, 4 * EPS)
    ad, bd = a.to(DEV), b.to(DEV)
    per = losses.ssim(ad, bd, size_average=False)
    mean = losses.ssim(ad, bd)
    assert per.shape == per64.shape and per.dtype == torch.float32 and per.is_cuda and per.grad_fn is None
    assert mean.shape == () and mean.dtype == torch.float32 and mean.grad_fn is None
    err, err_mean = float((per.cpu().double() - per64).abs().max()), abs(float(mean) - all64)
    print(f"{case}: |ssim - recorded fp64| = {err:.3e} per image, {err_mean:.3e} averaged; bound {bound:.3e} ({err / bound:.3f}, "
          f"{err_mean / bound:.3f})")
    assert err <= bound and err_mean <= bound
    col0 = percept.score_pixel_triplets(ad, bd, bd, "ssim")[0][:, 0].contiguous()
    assert torch.equal(per.view(torch.int32), col0.view(torch.int32))
    for module, want in ((losses.SSIM(size_average=False), per), (losses.SSIM(), mean)):
        got = module(ad, bd)
        assert torch.equal(got.reshape(-1).view(torch.int32), want.reshape(-1).view(torch.int32))
    with pytest.raises(NotImplementedError, match="forward only"):
        losses.ssim(ad.clone().requires_grad_(), bd)


def test_backbone_path_is_unchanged_by_the_metric_branch():
    """dino_b16-shaped ViT through the same predict_batch: its predictions are those of score_triplets on the stacked forward."""
    from mvp import percept

    ds = percept.SyntheticTwoAFC(6, image_size=(64, 96), seed=2)
    model = _vit()
    assert model.arch == "vit"
    want = []
    model.eval()
    for img_ref, img_left, img_right, p, ids in _loader(ds, 4):
        B = img_ref.shape[0]
        with torch.no_grad():
            feats = model(torch.cat((img_ref, img_left, img_right)).to(DEV)).float().contiguous()
        _, pred = percept.score_triplets(feats[:B], feats[B:2 * B], feats[2 * B:])
        want += [{"id": int(i), "gt": float(g), "prediction": int(q)} for i, g, q in zip(ids, p, pred.cpu())]
    results, metrics, errors = percept.predict_batch(model, _loader(ds, 4), output_dir=None)
    assert errors == [] and results == want
    assert metrics == percept.compute_metrics([r["gt"] for r in results], [r["prediction"] for r in results])


@pytest.mark.parametrize("metric", ["ssim", "psnr"])
def test_entry_script_runs_the_baseline_unchanged(metric, tmp_path, monkeypatch):
    """evaluate_model_percepture.py in-process with the documented overrides: the script itself knows nothing of the baselines."""
    import csv
    import sys

    from conftest import PKG

    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.syspath_prepend(PKG)
    sys.modules.pop("evaluate_model_percepture", None)
    import evaluate_model_percepture as script

    results, metrics, errors = script.main([f"backbone={metric}", f"dataset.preprocess={metric.upper()}", f"experiment_model={metric}",
                                            "batch_size=4", "dataset.num_triplets=6", "dataset.image_size=[20,36]",
                                            f"output_dir={tmp_path}/out"])
    assert errors == [] and [r["id"] for r in results] == list(range(6))
    assert all(r["prediction"] == int(r["gt"]) for r in results) and metrics["accuracy"] == 1.0  # near / far: margins >= 0.4 SSIM, 9 dB
    rows = list(csv.reader(open(tmp_path / "out" / "final_results_summary.csv")))
    assert len(rows) == 2 and rows[1][0] == metric and float(rows[1][1]) == 1.0
