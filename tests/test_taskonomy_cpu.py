"""Taskonomy probing without a GPU: the host transforms and tests/taskonomy_ref.py against tests/golden/taskonomy.npz (recorded from
the reference's own functions by tests/golden/make_goldens_taskonomy.py), the dataset / builder / config surface, and the argument
checks of the three exports (which run before any launch)."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch
import yaml

import taskonomy_ref as R
from conftest import GOLDEN, load_golden

DIGESTS = json.load(open(os.path.join(GOLDEN, "reference_config_digests_taskonomy.json")))
SIZES = [(4, 4), (7, 9), (8, 8), (13, 37), (64, 64)]
METRIC_CASES = [("curv_rand", "curvature"), ("curv_rand2", "curvature"), ("curv_ties", "curvature"), ("resh_rand", "reshading"),
                ("resh_rand2", "reshading"), ("resh_ties", "reshading")]


@pytest.fixture(scope="module")
def g():
    return load_golden("taskonomy.npz")


@pytest.mark.parametrize("hw", SIZES)
def test_host_transforms_equal_the_goldens(g, hw):
    from evals.datasets.transforms import make_valid_mask, task_transform

    H, W = hw
    raw, want = g[f"mask_{H}x{W}__raw"], g[f"mask_{H}x{W}__valid"]
    for m, w in zip(raw, want):
        got = task_transform(torch.from_numpy(m), "mask_valid")
        assert got.dtype == torch.bool and tuple(got.shape) == (1, H, W) and np.array_equal(got.numpy(), w)
    batch = make_valid_mask(torch.from_numpy(raw.astype(np.float32) / np.float32(255)).unsqueeze(1))  # the [b, c, h, w] form
    assert np.array_equal(batch.numpy(), want)
    u16, out = g[f"u16_{H}x{W}__raw"], g[f"u16_{H}x{W}__out"]
    assert u16.dtype == np.uint16
    for src in (u16, torch.from_numpy(u16.view(np.int16))):  # a decoder's array, and the int16 bit patterns a torch batch carries
        got = task_transform(src, "keypoints2d")
        assert got.dtype == torch.float32 and np.array_equal(got.numpy().view(np.uint32), out.view(np.uint32))


def test_host_clamp_tasks_and_channel_crop():
    from evals.datasets.transforms import task_transform

    maxx = np.float32(8000.0 / 65535.0)
    raw = np.array([[0, 1, 7999, 8000], [8001, 40000, 65535, 4000]], dtype=np.uint16)
    want = np.minimum(raw.astype(np.float32) / np.float32(65535.0), maxx) / maxx
    for task in ("depth_euclidean", "depth_zbuffer"):
        got = task_transform(raw, task).numpy()
        assert np.array_equal(got[0], want) and got.max() == 1.0 and got[0, 0, 0] == 0.0
    raw = np.array([[0, 16383, 16384, 65535]], dtype=np.uint16)
    got = task_transform(raw, "edge_texture").numpy()[0, 0]
    assert got[0] == 0.0 and got[1] < 1.0 and got[2] == 1.0 and got[3] == 1.0
    rgb = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3) * 14
    for task, ct in (("principal_curvature", 2), ("curvature", 2), ("reshading", 1), ("normal", 3)):
        got = task_transform(rgb, task)
        assert tuple(got.shape) == (ct, 2, 3)
        assert np.array_equal(got.numpy(), (rgb.astype(np.float32) / np.float32(255)).transpose(2, 0, 1)[:ct])
    for task in ("edge_occlusion", "segment_semantic", "class_object"):
        with pytest.raises(NotImplementedError):
            task_transform(rgb, task)
    with pytest.raises(ValueError):
        task_transform(rgb, "no_such_task")


@pytest.mark.parametrize("case", ["l1_a", "l1_b", "l1_c", "l1_none", "l1_allinvalid"])
def test_masked_l1_restatement_reproduces_the_golden(g, case):
    pred, tgt = torch.from_numpy(g[f"{case}__pred"]), torch.from_numpy(g[f"{case}__target"])
    mask = torch.from_numpy(g[f"{case}__mask"]) if g[f"{case}__mask"].size else None
    got = float(R.masked_l1(pred.double(), tgt.double(), mask))
    want = float(g[f"{case}__loss64"])
    if case == "l1_allinvalid":
        assert np.isnan(got) and np.isnan(want) and np.isnan(float(g[f"{case}__loss32"]))
        return
    assert abs(got - want) <= 1e-12 * abs(want), (got, want)
    assert abs(float(g[f"{case}__loss32"]) - want) <= 1e-6 * abs(want)  # the reference's own fp32 sum


@pytest.mark.parametrize("case,form", METRIC_CASES)
def test_metric_restatement_reproduces_the_golden(g, case, form):
    pred, tgt, valid = (torch.from_numpy(g[f"{case}__{k}"]) for k in ("pred", "target", "valid"))
    keys = R.CURV_KEYS if form == "curvature" else R.RESH_KEYS
    table, dist = g[f"{case}__table"], g[f"{case}__absrel_dist"]
    sums = R.metric_sums(pred[:, :2] if form == "curvature" else pred, tgt, valid, form)
    mine = R.curvature_metrics(sums) if form == "curvature" else R.reshading_metrics(sums)
    nv = np.maximum(sums[..., 1].numpy(), 1.0)  # [B, C]
    assert np.array_equal(sums[..., 1].numpy(), g[f"{case}__nvalid"])
    # counts: the reference's fp32 quotient count / n determines the count (n < 2^24)
    for c in range(sums.shape[1]):
        names = [f"δ{t}_k{c + 1}" for t in ("1.25", "2.5", "3.75")] if form == "curvature" else keys[1:]
        for j, k in enumerate(names):
            want = np.rint(table[keys.index(k)] * nv[:, c])
            assert np.array_equal(want, sums[:, c, 2 + j].numpy()), (k, want, sums[:, c, 2 + j])
    for k in keys[1:]:
        assert np.allclose(mine[k].numpy(), table[keys.index(k)], rtol=2e-7, atol=0), k
    got, want = mine["AbsRel"].numpy(), table[0]
    assert np.array_equal(np.isnan(got), np.isnan(want))  # NaN exactly where the reference has it
    ok = ~np.isnan(want)
    zero = ok & (want == 0)
    assert np.all(got[zero] == 0)
    fin = ok & ~zero
    assert np.all(np.abs(got[fin] - want[fin]) <= 4 * dist[fin] * np.abs(got[fin])), (got, want, dist)
    if case.endswith("ties"):
        assert np.isnan(want[1]) and np.isnan(want[2]) and want[3] == 0 and np.isfinite(want[0])


def test_tie_pixels_are_not_counted(g):
    """The recorded ties: fp32 quotients that land on the threshold itself."""
    pred, tgt, valid = (torch.from_numpy(g[f"curv_ties__{k}"]) for k in ("pred", "target", "valid"))
    _, ratio, _ = R.metric_terms(pred[:, :2], tgt, valid, "curvature")
    assert [float(ratio[0, 0, 0, j]) for j in range(3)] == [1.25, 2.5, 1.25]
    assert np.isinf(float(ratio[0, 0, 0, 3])) and np.isnan(float(ratio[0, 1, 0, 2]))  # gt 0 against 0.3, and against 0
    assert float(ratio[0, 1, 0, 3]) < 0  # a negative ratio counts as under every threshold: the reference's quirk
    pred, tgt, valid = (torch.from_numpy(g[f"resh_ties__{k}"]) for k in ("pred", "target", "valid"))
    _, ratio, _ = R.metric_terms(pred, tgt, valid, "reshading")
    assert float(ratio[0, 0, 0, 0]) == float(np.float32(1.1**3)) and not bool(ratio[0, 0, 0, 0] < 1.1**3)


def test_builder_builds_task_nodes_with_the_item_contract():
    from evals.datasets import build_loader
    from evals.datasets.taskonomy import Taskonomy, TaskonomyDataset

    node = {"task": "reshading", "name": "taskonomy", "raw": True, "image_mean": "imagenet", "num_samples": 5, "image_size": [12, 16]}
    b = next(iter(build_loader(node, "test", 2)))
    assert set(b) == {"rgb", "reshading", "mask_valid"}
    assert b["rgb"].dtype == torch.uint8 and tuple(b["rgb"].shape) == (2, 12, 16, 3)
    assert b["reshading"].dtype == torch.uint8 and tuple(b["reshading"].shape) == (2, 12, 16, 1) and tuple(b["mask_valid"].shape) == (2, 12, 16)
    node = dict(node, task="depth", _target_="evals.datasets.synthetic.SyntheticTaskonomy")
    ld = build_loader(node, "test", 2)
    assert isinstance(ld.dataset, TaskonomyDataset) and ld.dataset.task == "depth" and len(ld.dataset) == 5
    b = next(iter(ld))
    assert set(b) == {"rgb", "depth", "mask_valid"}
    assert b["rgb"].dtype == torch.float32 and tuple(b["rgb"].shape) == (2, 3, 12, 16)
    assert b["depth"].dtype == torch.float32 and tuple(b["depth"].shape) == (2, 1, 12, 16) and float(b["depth"].max()) == 1.0
    assert b["mask_valid"].dtype == torch.bool and tuple(b["mask_valid"].shape) == (2, 1, 12, 16)
    with pytest.raises(NotImplementedError, match="GaussianBlur"):
        build_loader(dict(node, task="edge_occlusion"), "test", 2)
    with pytest.raises(NotImplementedError, match="datasets"):
        Taskonomy("a", "b", "train", "normal")


@pytest.mark.parametrize("task", ["principal_curvature", "normal", "reshading", "depth_euclidean", "edge_texture", "keypoints3d"])
def test_synthetic_taskonomy_is_deterministic_and_shaped(task):
    from evals.datasets.synthetic import SyntheticTaskonomy
    from evals.datasets.transforms import task_transform
    from mvp.taskonomy import TASKS

    a, b = SyntheticTaskonomy("train", task, 4, (40, 48)), SyntheticTaskonomy("train", task, 4, (40, 48))
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k])
    assert not torch.equal(a[1]["rgb"], a[2]["rgb"]) and not torch.equal(a[1][task], SyntheticTaskonomy("test", task, 4, (40, 48))[1][task])
    s = a[3]
    assert s[task].dtype == (torch.uint8 if TASKS[task]["bits"] == 8 else torch.int16)
    bad = (s["mask_valid"] != 255).float().mean()
    assert 0.02 < float(bad) < 0.25 and set(s["mask_valid"].unique().tolist()) == {0, 255}
    assert int((s[task] == 0).sum()) > 0  # exact zeros
    cooked = SyntheticTaskonomy("train", task, 4, (40, 48), raw=False)[3]
    assert torch.equal(cooked[task], task_transform(s[task], task)) and tuple(cooked[task].shape) == (TASKS[task]["channels"], 40, 48)
    grown = (~cooked["mask_valid"]).float().mean()
    assert float(grown) > float(bad)  # the blobs cross block borders: growing them to 4 x 4 blocks invalidates more
    with pytest.raises(IndexError):
        a[4]


def _digest(node):
    return hashlib.sha256(json.dumps(node, sort_keys=True).encode()).hexdigest()


def test_configs_match_the_reference_and_compose():
    from mvp import config

    node = yaml.safe_load(open(os.path.join(config.CONFIG_DIR, "probe", "taskonomy_dpt.yaml")))
    assert _digest(node) == DIGESTS["probe/taskonomy_dpt"], node
    probe = config.instantiate(node, feat_dim=[768] * 4)
    assert type(probe).__name__ == "TaskonomyHead" and probe.name == "snorm_dpt_k3_UA" and not hasattr(probe, "batch_norm")
    root = yaml.safe_load(open(os.path.join(config.CONFIG_DIR, "taskonomy_training.yaml")))
    assert {"dataset": "synthetic_taskonomy"} in root["defaults"] and root["system"]["num_gpus"] == 1
    root["defaults"] = [({"dataset": None} if isinstance(d, dict) and "dataset" in d else d) for d in root["defaults"]]
    root["system"]["num_gpus"] = None
    assert _digest(root) == DIGESTS["taskonomy_training(dataset, system.num_gpus blanked)"], root
    cfg = config.compose("taskonomy_training", ["batch_size=4", "dataset.task=reshading"])
    assert cfg["probe"]["_target_"] == "evals.models.probes.TaskonomyHead" and cfg["probe"]["output_dim"] == 3
    assert cfg["optimizer"]["n_epochs"] == 15 and cfg["batch_size"] == 4 and cfg["backbone"]["model_name"] == "vitb14"
    ds = cfg["dataset"]
    assert ds["task"] == "reshading" and ds["name"] == "taskonomy" and ds["raw"] is True and ds["image_mean"] == "imagenet"
    assert "_target_" not in ds


def test_cpu_tensors_are_refused():
    from evals.utils.losses import MaskedL1Loss
    from evals.utils.metrics import evaluate_curvature_absrel, evaluate_reshading_absrel_and_delta
    from mvp import lib

    p, t, m = torch.rand(1, 2, 4, 4), torch.rand(1, 2, 4, 4), torch.ones(1, 1, 4, 4, dtype=torch.bool)
    with pytest.raises(lib.MvpError, match="device tensors"):
        MaskedL1Loss()(p, t, m)
    with pytest.raises(lib.MvpError, match="device tensors"):
        evaluate_curvature_absrel(p, t, m)
    with pytest.raises(lib.MvpError, match="device tensors"):
        evaluate_reshading_absrel_and_delta(p[:, :1], t[:, :1], m)


def test_exports_are_registered_and_check_their_arguments():
    from mvp import lib

    for name, st in (("mvp_task_prepare", "mvp_task_prepare_args"), ("mvp_masked_l1_fwd_bwd", "mvp_masked_l1_args"),
                     ("mvp_task_metrics", "mvp_task_metrics_args")):
        assert lib.SYMBOLS[name] is lib.STRUCTS[st]
    so = lib.load()
    ok = dict(target_raw=16, mask_raw=16, target=16, valid=16, B=1, H=4, W=4, Cs=3, Ct=2, bits=8)
    for bad in (dict(H=3), dict(W=3), dict(Cs=1), dict(bits=12), dict(mask_raw=None), dict(bits=16), dict(clamp_max=-1.0), dict(B=0)):
        assert so.mvp_task_prepare(ctypes.byref(lib.TaskPrepareArgs(**dict(ok, **bad))), None) == -1, bad
    ok = dict(pred=16, target=16, valid=16, loss=16, workspace=16, workspace_bytes=40960, B=1, C=2, Cm=1, HW=8)
    for bad in (dict(Cm=3), dict(workspace_bytes=40959), dict(loss=None), dict(HW=0), dict(workspace=20)):
        assert so.mvp_masked_l1_fwd_bwd(ctypes.byref(lib.MaskedL1Args(**dict(ok, **bad))), None) == -1, bad
    ok = dict(pred=16, target=16, valid=16, out=16, workspace=16, workspace_bytes=40960, B=1, C=2, Cm=2, HW=8, form=0)
    for bad in (dict(form=2), dict(B=513, C=2), dict(out=None), dict(Cm=0), dict(out=20)):
        assert so.mvp_task_metrics(ctypes.byref(lib.TaskMetricsArgs(**dict(ok, **bad))), None) == -1, bad
