"""The Python surface of the 2AFC perceptual-similarity evaluation on the GPU (mvp/percept.py, evaluate_model_percepture.py) against
the fp64 definition of tests/twoafc_ref.py, applied on the CPU to the features that ``model(stacked)`` itself returned for the same
batches.  The comparison of predictions is exact: every triplet's two fp64 similarities differ by at least 1e-3 (asserted; the
dataset seeds were chosen with the CPU oracles of the two backbones), which the kernel's 2^-23 cannot turn.  World size 1 only: the
merge of several ranks is covered on the CPU (tests/test_percept_cpu.py)."""
import contextlib
import csv
import os
import sys

import pytest
import torch

import twoafc_ref as ref
from conftest import PKG

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MARGIN = 1e-3


class _SomeLabelsFlipped(torch.utils.data.Dataset):
    """The labels of the listed items inverted: a perfect model is then wrong on those, so that FP and FN occur and the four metrics
    differ."""

    def __init__(self, ds, flipped=()):
        self.ds, self.flipped = ds, set(flipped)

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, i):
        a, b, c, p, idx = self.ds[i]
        return a, b, c, (type(p)(1 - p) if i in self.flipped else p), idx


def _vit(**kw):
    from evals.models.dino import DINO
    from oracle import vit as ovit

    kw.setdefault("return_cls", True)
    return DINO(weights=ovit.make_vit_weights(embed_dim=128, depth=4, seed=1), **kw).to(DEV)


def _loader(ds, batch_size):
    return torch.utils.data.DataLoader(ds, batch_size, shuffle=False, drop_last=False)


def _expected(model, loader):
    """(results, counts) by the fp64 definition from the model's own features, batch by batch."""
    model.eval()
    results, counts = [], [0, 0, 0, 0]
    for img_ref, img_left, img_right, p, ids in loader:
        B = img_ref.shape[0]
        with torch.no_grad():
            feats = model(torch.cat((img_ref, img_left, img_right)).to(DEV)).float().cpu()
        sim64, pred64 = ref.score(feats[:B], feats[B:2 * B], feats[2 * B:])
        assert ((sim64[:, 0] - sim64[:, 1]).abs() >= MARGIN).all(), sim64  # every triplet: none is excused
        results += [{"id": int(i), "gt": float(g), "prediction": int(q)} for i, g, q in zip(ids, p, pred64)]
        counts = [a + b for a, b in zip(counts, ref.counts(p, pred64))]
    return results, counts


@contextlib.contextmanager
def _count_device_to_host():
    """Counts every call that brings a DEVICE tensor's values to the host through the tensor API, ``host.copy_(device)`` included."""
    seen, saved = [], {}

    def wrap(name):
        orig = getattr(torch.Tensor, name)
        saved[name] = torch.Tensor.__dict__.get(name)  # None: inherited from the C base class

        def f(self, *a, **k):
            out = orig(self, *a, **k)
            if self.is_cuda and not (torch.is_tensor(out) and out.is_cuda):
                seen.append((name, tuple(self.shape)))
            if name == "copy_" and not self.is_cuda and a and torch.is_tensor(a[0]) and a[0].is_cuda:
                seen.append((name, tuple(self.shape)))  # host.copy_(device)
            return out

        setattr(torch.Tensor, name, f)

    for name in ("cpu", "item", "tolist", "numpy", "to", "copy_", "__bool__", "__int__", "__float__", "__index__"):
        wrap(name)
    try:
        yield seen
    finally:
        for name, own in saved.items():
            if own is None:
                delattr(torch.Tensor, name)
            else:
                setattr(torch.Tensor, name, own)


def test_vit_class_token_route_ragged_last_batch_one_transfer():
    from mvp import percept

    # seed 2: labels 1 0 0 1 0 0 1 1 0 1; items 0 (1 -> 0: a false positive), 1 and 5 (0 -> 1: false negatives) get the wrong label
    ds = _SomeLabelsFlipped(percept.SyntheticTwoAFC(10, image_size=(64, 96), seed=2), flipped=(0, 1, 5))
    model = _vit()
    assert model.arch == "vit" and model.heads == 2
    want, counts = _expected(model, _loader(ds, 4))  # batches of 4, 4, 2
    with _count_device_to_host() as seen:
        results, metrics, errors = percept.predict_batch(model, _loader(ds, 4), output_dir=None)
    assert len(seen) == 1, seen  # predictions and counts of the whole shard in one transfer, after the loop
    assert errors == [] and results == want and [r["id"] for r in results] == list(range(10))
    assert metrics == ref.metrics(counts) == percept.compute_metrics([r["gt"] for r in results], [r["prediction"] for r in results])
    assert counts == [4, 1, 2, 3] and len({round(v, 6) for v in metrics.values()}) == 4, (counts, metrics)
    assert not model.training


def test_resnet_pooled_route():
    import warnings

    from evals.models.dino_res50 import DINO_RESNET
    from mvp import percept

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (no local checkpoint: seeded random init)
        model = DINO_RESNET(fixed_size=64, init_seed=0).to(DEV)
    ds = percept.SyntheticTwoAFC(4, image_size=64, seed=1)
    model.eval()
    with torch.no_grad():
        probe = model(torch.stack([ds[0][0]] * 3).to(DEV))
    assert model.arch != "vit" and probe.shape == (3, 2048, 2, 2)  # HW = 4
    want, counts = _expected(model, _loader(ds, 2))
    results, metrics, errors = percept.predict_batch(model, _loader(ds, 2), output_dir=None)
    assert errors == [] and results == want and metrics == ref.metrics(counts)
    assert {r["prediction"] for r in results} == {0, 1}


def test_device_log_grows_and_keeps_what_it_holds():
    """Growing replaces the buffer: the views of one reserve() are those of the buffer after it, and what the old one held moves."""
    from mvp.percept import _DeviceLog

    log = _DeviceLog(1, torch.device(DEV))
    want_counts, want_preds = [0, 0, 0, 0], []
    for k, vals in enumerate(([0, 1], [1, 1, 0], [0, 0, 1, 0, 1, 1])):  # capacity 2: the second and the third reserve grow
        pred, counts = log.reserve(len(vals))  # the order predict_batch uses: both views from one call, then the writes
        pred.copy_(torch.tensor(vals, dtype=torch.int32, device=DEV))
        counts.add_(torch.tensor([1, 2, 3, k], device=DEV))
        want_counts = [a + b for a, b in zip(want_counts, [1, 2, 3, k])]
        want_preds += vals
    assert log.fetch() == (want_counts, want_preds)


def test_predict_batch_keeps_every_batchs_counts_when_the_log_grows(monkeypatch):
    """A plain list of batches has no length to size the log from; with a starting capacity of 2 every batch of 4 outgrows it.  The
    metrics come from the device counts, the results from the device predictions: they must tell the same story."""
    from mvp import percept

    monkeypatch.setattr(percept, "_LOG_CAPACITY", 2)
    ds = _SomeLabelsFlipped(percept.SyntheticTwoAFC(10, image_size=(64, 96), seed=2), flipped=(0, 1, 5))
    model = _vit()
    want, counts = _expected(model, _loader(ds, 4))
    results, metrics, errors = percept.predict_batch(model, list(_loader(ds, 4)), output_dir=None)
    assert errors == [] and results == want and counts == [4, 1, 2, 3]
    assert metrics == ref.metrics(counts) == percept.compute_metrics([r["gt"] for r in results], [r["prediction"] for r in results])


def test_score_triplets_refuses_images_that_are_not_dense():
    """Also for B = 1, where the stride between images says nothing."""
    from mvp import percept

    g = torch.Generator().manual_seed(8)
    for B in (1, 2):
        x = torch.randn(B, 8, 3, 5, generator=g).to(DEV)
        cl = x.contiguous(memory_format=torch.channels_last)
        assert cl.shape == x.shape and not cl[0].is_contiguous()
        with pytest.raises(ValueError, match="contiguous"):
            percept.score_triplets(cl, cl, cl)
        wide = torch.randn(B, 16, generator=g).to(DEV)[:, ::2]  # [B, 8] with a stride of 2 inside the row
        with pytest.raises(ValueError, match="contiguous"):
            percept.score_triplets(wide, wide, wide)
        sim, pred = percept.score_triplets(x, x, x)
        assert torch.equal(sim.cpu(), torch.ones(B, 2)) and pred.tolist() == [1] * B


def test_cosine_similarity_batch_is_the_fp64_cosine():
    from mvp import percept

    g = torch.Generator().manual_seed(6)
    a, b = torch.randn(9, 130, generator=g), torch.randn(9, 130, generator=g)
    b[:3] = a[:3] * 2.5
    got = percept.cosine_similarity_batch(a.to(DEV), b.to(DEV))
    assert got.shape == (9,) and got.dtype == torch.float32 and got.is_cuda
    err = float((got.cpu().double() - ref.cosine(a, b)).abs().max())
    print(f"cosine_similarity_batch: max |sim - sim64| = {err:.3e}")
    assert err <= 2.0 ** -23
    with pytest.raises(Exception, match="device"):
        percept.cosine_similarity_batch(a, b)


@pytest.mark.parametrize("kw", [dict(return_cls=False), dict(return_cls=True, return_multilayer=True)], ids=["no_cls", "multilayer"])
def test_misconfigured_backbone_raises(kw):
    from mvp import percept

    ds = percept.SyntheticTwoAFC(2, image_size=(64, 96), seed=0)
    with pytest.raises(ValueError, match="return_cls=True"):
        percept.predict_batch(_vit(**kw), _loader(ds, 2), output_dir=None)


def test_bad_labels_raise():
    from mvp import percept

    class Half(_SomeLabelsFlipped):
        def __getitem__(self, i):
            a, b, c, p, idx = self.ds[i]
            return a, b, c, type(p)(0.5), idx

    with pytest.raises(ValueError, match="0 / 1"):
        percept.predict_batch(_vit(), _loader(Half(percept.SyntheticTwoAFC(2, image_size=(64, 96))), 2), output_dir=None)


def test_entry_script_writes_the_csv_row(tmp_path, monkeypatch, capsys):
    """evaluate_model_percepture.py in-process on the synthetic config, the tiny weights found as a local checkpoint."""
    from oracle import vit as ovit

    torch.save(ovit.make_vit_weights(embed_dim=128, depth=4, seed=1), tmp_path / "dino_vitb16.pth")
    monkeypatch.setenv("MVP_CKPT_DIR", str(tmp_path))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.syspath_prepend(PKG)
    sys.modules.pop("evaluate_model_percepture", None)
    import evaluate_model_percepture as script

    args = ["backbone=dino_b16", "backbone.return_cls=True", "experiment_model=dino_b16", "batch_size=4", "wandb.use=True",
            "dataset.num_triplets=6", "dataset.image_size=[64,96]", "dataset.seed=2", f"output_dir={tmp_path}/out"]
    results, metrics, errors = script.main(args)
    assert errors == [] and [r["id"] for r in results] == list(range(6))
    assert all(r["prediction"] == int(r["gt"]) for r in results) and metrics["accuracy"] == 1.0  # near / far triplets, margins >= 0.04
    assert "Test metrics" in capsys.readouterr().out
    rows = list(csv.reader(open(tmp_path / "out" / "final_results_summary.csv")))
    assert rows[0] == ["Model Name", "Test Accuracy", "Test F1-Score", "Test Precision", "Test Recall"]
    assert len(rows) == 2 and rows[1][0] == "dino_b16"
    assert [float(v) for v in rows[1][1:]] == [metrics[k] for k in ("accuracy", "f1_score", "precision", "recall")]
    script.main(args)
    assert len(list(csv.reader(open(tmp_path / "out" / "final_results_summary.csv")))) == 3  # appended, header once
