"""CPU checks of the 2AFC perceptual-similarity evaluation (mvp/percept.py, evaluate_model_percepture.py, csrc/twoafc.hip): the ABI
boundary of mvp_twoafc_score, the metrics against values written out from their definitions, the config, the synthetic dataset, the
sharding and the CSV row."""
import csv
import ctypes
import os
import re

import pytest
import torch

import twoafc_ref as ref
from conftest import REPO


def test_symbols_are_exported_declared_and_bound():
    from mvp import lib

    header = open(os.path.join(REPO, "include", "mvp_hip.h")).read()
    so = lib.load()
    for name in ("mvp_twoafc_score", "mvp_twoafc_workspace_bytes"):
        assert re.search(r"^\s*(?:int|int64_t)\s+" + name + r"\s*\(", header, flags=re.M), name
        assert name in lib.SYMBOLS and hasattr(so, name)
    assert lib.SYMBOLS["mvp_twoafc_score"] is lib.TwoafcArgs and lib.STRUCTS["mvp_twoafc_args"] is lib.TwoafcArgs
    assert "struct mvp_twoafc_args {" in header and so.mvp_sizeof(b"mvp_twoafc_args") == ctypes.sizeof(lib.TwoafcArgs)
    assert lib.info().abi_version == 8
    from mvp import ops, percept

    assert callable(ops.twoafc_score) and callable(percept.cosine_similarity_batch)


def _args(**kw):
    """Arguments mvp_twoafc_score accepts up to the launch (never launched here): fake 16-byte aligned addresses."""
    from mvp import lib

    so = lib.load()
    base = dict(ref=4096, left=8192, right=12288, label=256, sim=512, pred=1024, counts=2048, workspace=16384, ld=65 * 49,
                B=3, C=65, HW=49, accumulate=0)
    base["workspace_bytes"] = so.mvp_twoafc_workspace_bytes(3, 65, 49)
    base.update(kw)
    return lib.TwoafcArgs(**base)


@pytest.mark.parametrize("bad", [
    dict(ref=None), dict(left=None), dict(right=None), dict(sim=None), dict(pred=None),
    dict(label=None),                       # counts without label
    dict(B=0), dict(B=-1), dict(C=0), dict(C=-3), dict(HW=0), dict(HW=-1),
    dict(ld=65 * 49 - 1),                   # ld < C * HW
    dict(C=65536, HW=32768, ld=1 << 31, workspace_bytes=1 << 40),  # C * HW = 2^31 > 2^31 - 1
    dict(workspace=None), dict(workspace=16384 + 4), dict(workspace_bytes=3 * 40 - 1), dict(workspace_bytes=0),
    dict(counts=2048 + 4),
], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_bad_arguments_return_einval(bad):
    from mvp import lib

    so = lib.load()
    assert so.mvp_twoafc_workspace_bytes(3, 65, 49) == 3 * 40  # (one chunk: the short-workspace cases above are one byte short)
    assert so.mvp_twoafc_score(ctypes.byref(_args(**bad)), None) == -1
    assert so.mvp_twoafc_score(None, None) == -1


def test_workspace_bytes():
    from mvp import lib

    ws = lib.load().mvp_twoafc_workspace_bytes
    for B, C, HW in [(0, 8, 1), (-1, 8, 1), (1, 0, 1), (1, 8, 0), (1, -8, 4), (1, 65536, 32768), (1, 1 << 30, 2)]:
        assert ws(B, C, HW) == 0, (B, C, HW)
    assert ws(1, 1, 1) == 40 and ws(16, 768, 1) == 16 * 40 and ws(1, 1, (1 << 31) - 1) == 40
    assert ws(16, 2048, 225) == 16 * 108 * 40   # ceil(4096 / 225) = 19 channels at least: 108 chunks of 19
    assert ws(2, 8200, 1) == 2 * 3 * 40 and ws(3, 300, 49) == 3 * 4 * 40 and ws(2, 600, 64) == 2 * 10 * 40
    assert ws(1, 1 << 20, 64) == 256 * 40       # the cap on the chunks of one triplet


def test_metrics_from_counts_against_the_definitions():
    from mvp.percept import compute_metrics, metrics_from_counts

    # general: TP 3, FP 1, FN 2, TN 4 -> accuracy 7/10, precision 3/4, recall 3/5, F1 = 2 * 3 / (2 * 3 + 1 + 2) = 6/9
    m = metrics_from_counts(3, 1, 2, 4)
    assert set(m) == {"accuracy", "f1_score", "precision", "recall"}
    assert m == {"accuracy": 0.7, "f1_score": 6 / 9, "precision": 0.75, "recall": 0.6}
    assert abs(m["f1_score"] - 2 * 0.75 * 0.6 / (0.75 + 0.6)) < 1e-15
    # no predicted positives: precision 0 / 0 -> 0.0, recall 0 / 2, F1 0 / 2
    assert metrics_from_counts(0, 0, 2, 3) == {"accuracy": 0.6, "f1_score": 0.0, "precision": 0.0, "recall": 0.0}
    # no actual positives: recall 0 / 0 -> 0.0, precision 0 / 2
    assert metrics_from_counts(0, 2, 0, 3) == {"accuracy": 0.6, "f1_score": 0.0, "precision": 0.0, "recall": 0.0}
    # all correct
    assert metrics_from_counts(4, 0, 0, 5) == {"accuracy": 1.0, "f1_score": 1.0, "precision": 1.0, "recall": 1.0}
    # only negatives, all correct: every positive-class ratio is 0 / 0
    assert metrics_from_counts(0, 0, 0, 5) == {"accuracy": 1.0, "f1_score": 0.0, "precision": 0.0, "recall": 0.0}
    assert metrics_from_counts(0, 0, 0, 0) == {"accuracy": 0.0, "f1_score": 0.0, "precision": 0.0, "recall": 0.0}
    gt = [1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    pr = [1, 1, 1, 0, 0, 1, 0, 0, 0, 0]
    assert compute_metrics(gt, pr) == m == ref.metrics(ref.counts(torch.tensor(gt), torch.tensor(pr)))
    with pytest.raises(ValueError, match="0 / 1"):
        compute_metrics([0.0, 0.5], [0, 1])
    with pytest.raises(ValueError):
        compute_metrics([0.0, 1.0], [0])


def test_metrics_agree_with_sklearn():
    sk = pytest.importorskip("sklearn.metrics")
    from mvp.percept import compute_metrics

    g = torch.Generator().manual_seed(4)
    gt = torch.randint(0, 2, (57,), generator=g).tolist()
    pr = torch.randint(0, 2, (57,), generator=g).tolist()
    m = compute_metrics(gt, pr)
    want = {"accuracy": sk.accuracy_score(gt, pr), "f1_score": sk.f1_score(gt, pr), "precision": sk.precision_score(gt, pr),
            "recall": sk.recall_score(gt, pr)}
    assert all(abs(m[k] - want[k]) < 1e-12 for k in want), (m, want)


def test_config_composes_with_the_readme_overrides():
    from mvp import config

    cfg = config.compose("model_percepture", ["backbone=dino_b16", "backbone.return_cls=True"])
    assert cfg["backbone"]["_target_"] == "evals.models.dino.DINO" and cfg["backbone"]["return_cls"] is True
    assert cfg["dataset"]["_target_"] == "mvp.percept.SyntheticTwoAFC"
    assert cfg["batch_size"] == 16 and cfg["system"] == {"random_seed": 8, "num_gpus": 1, "port": 12355} and cfg["note"] == ""
    assert cfg["experiment_name"] == "SSL_Model_Percepture" and cfg["experiment_model"] == "dinov2_b14" and cfg["output_dir"] == "result"
    assert cfg["wandb"]["use"] in (True, False) and "optimizer" in cfg and "probe" in cfg
    default = config.compose("model_percepture")
    assert default["backbone"]["_target_"] == "evals.models.dino.DINO" and default["backbone"]["dino_name"] == "dinov2"
    assert default["backbone"]["return_cls"] is False  # the script's override turns it on, as in the reference's README
    assert config.compose("model_percepture", ["wandb.use=True", "dataset.num_triplets=5"])["dataset"]["num_triplets"] == 5


def test_synthetic_twoafc_item_contract_determinism_and_labels():
    import numpy as np

    from evals.datasets.builder import build_loader
    from mvp import config
    from mvp.percept import SyntheticTwoAFC

    ds = SyntheticTwoAFC(12, image_size=(16, 24), seed=3)
    assert len(ds) == 12
    labels = []
    for i in range(12):
        img_ref, img_left, img_right, p, idx = ds[i]
        assert img_ref.shape == img_left.shape == img_right.shape == (3, 16, 24) and img_ref.dtype == torch.float32
        assert isinstance(p, np.float32) and p in (0.0, 1.0) and isinstance(idx, int) and idx == i
        near, far = (img_right, img_left) if p == 1 else (img_left, img_right)
        assert float((near - img_ref).abs().max()) < 0.5 < float((far - img_ref).abs().max())  # p = 1: the right one is the close one
        labels.append(float(p))
    assert set(labels) == {0.0, 1.0}
    again, other = SyntheticTwoAFC(12, image_size=(16, 24), seed=3), SyntheticTwoAFC(12, image_size=(16, 24), seed=4)
    for a, b in zip(ds[5], again[5]):
        assert torch.equal(torch.as_tensor(a), torch.as_tensor(b))
    assert not torch.equal(ds[5][0], other[5][0]) and not torch.equal(ds[5][0], ds[6][0])
    assert SyntheticTwoAFC(2)[0][0].shape == (3, 224, 224)
    with pytest.raises(IndexError):
        ds[12]
    # through the builder, from the config file: the reference's batch contract
    node = config.compose("model_percepture", ["dataset.num_triplets=5", "dataset.image_size=8"])["dataset"]
    batches = list(build_loader(node, "test", 2))
    assert [len(b[4]) for b in batches] == [2, 2, 1]
    img_ref, img_left, img_right, p, ids = batches[0]
    assert img_ref.shape == img_left.shape == img_right.shape == (2, 3, 8, 8) and p.dtype == torch.float32 and ids.tolist() == [0, 1]


@pytest.mark.parametrize("world", [1, 2, 3])
def test_sharding_covers_every_batch_once_and_merged_counts_equal_unsharded(world):
    from mvp import percept

    n, bs = 23, 4  # 6 batches, the last one of 3
    g = torch.Generator().manual_seed(9)
    gt = torch.randint(0, 2, (n,), generator=g).float().tolist()
    pr = torch.randint(0, 2, (n,), generator=g).tolist()
    batches = [list(range(s, min(s + bs, n))) for s in range(0, n, bs)]
    shards = [percept.shard_batches(len(batches), r, world) for r in range(world)]
    assert sorted(b for s in shards for b in s) == list(range(len(batches)))
    assert all(s == list(range(r, len(batches), world)) for r, s in enumerate(shards))
    parts = []
    for r, s in enumerate(shards):
        rows = [(b, [{"id": i, "gt": gt[i], "prediction": pr[i]} for i in batches[b]]) for b in s]
        mine = [i for b in s for i in batches[b]]
        parts.append((rows, percept.counts_from_labels([gt[i] for i in mine], [pr[i] for i in mine]), [f"rank {r}"] if r == 1 else []))
    results, counts, errors = percept.merge_shards(parts)
    assert [d["id"] for d in results] == list(range(n))  # loader order, every triplet once
    assert tuple(counts) == percept.counts_from_labels(gt, pr) == tuple(ref.counts(torch.tensor(gt), torch.tensor(pr)))
    assert sum(counts) == n and errors == (["rank 1"] if world > 1 else [])
    assert percept.metrics_from_counts(*counts) == percept.compute_metrics(gt, pr)


def test_csv_header_and_row(tmp_path):
    from mvp import percept, results

    m = percept.metrics_from_counts(3, 1, 2, 4)
    path = str(tmp_path / "out" / "final_results_summary.csv")
    for name in ("dino_b16", "dinov2_b14"):
        results.append_result_csv(path, percept.CSV_HEADER, [name] + [m[k] for k in percept.METRIC_NAMES])
    rows = list(csv.reader(open(path)))
    assert rows[0] == ["Model Name", "Test Accuracy", "Test F1-Score", "Test Precision", "Test Recall"]
    assert len(rows) == 3 and rows[1][0] == "dino_b16" and rows[2][0] == "dinov2_b14"
    assert [float(v) for v in rows[1][1:]] == [0.7, 6 / 9, 0.75, 0.6]
