"""CPU checks of the MaskCut evaluation: the fp64 oracle (tests/maskcut_ref.py) against what the reference's own code gave on the
same fixtures (tests/golden/maskcut.npz, recorded by tests/golden/make_goldens_maskcut.py), the metric formulas, the config, the
Python layer's refusals and the host-side argument checks of the four exports (they run before any launch).

Tolerances.  tau: the affinity tolerance AFF_TOL = 9.6e-5 of tests/test_gpu_maskcut_kernels.py (sklearn stops on a tolerance and
reads fp32 affinities; the oracle iterates to the fixed point in fp64).  W: equal except where |A - tau| <= 2 AFF_TOL.  Eigenvector:
the reference's is scipy's generalised eigh(D - W, D), the oracle's numpy's eigh of S; both are accurate to ~1e-15 / gap, compared at
1e-7 relative to max |v| after the sign convention."""
import ctypes
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import maskcut_ref as ref
from conftest import GOLDEN, load_golden

AFF_TOL = 9.6e-5


@functools.lru_cache(maxsize=None)
def oracle(name):
    f, lab, h, w, P = ref.fixture(name)
    return f, h, w, P, ref.maskcut(f, h, w, P)


@functools.lru_cache(maxsize=None)
def gold():
    return load_golden("maskcut.npz")


def _passes(name):
    return [k for k in range(2) if f"{name}/{k}/tau" in gold()]


@pytest.mark.parametrize("name", list(ref.FIXTURES))
def test_oracle_against_the_reference_goldens(name):
    f, h, w, P, out = oracle(name)
    g = gold()
    N = h * w
    assert _passes(name) == list(range(P if (h == w or P == 1) else 1))
    for k in _passes(name):
        ps = out["passes"][k]
        assert abs(ps["tau"] - float(g[f"{name}/{k}/tau"])) <= AFF_TOL
        W_on = np.unpackbits(g[f"{name}/{k}/W_on"])[:N * N].reshape(N, N).astype(bool)
        near = np.abs(ps["A"] - ps["tau"]) <= 2 * AFF_TOL
        assert near.mean() <= 1e-3 and np.array_equal(W_on[~near], ps["B"][~near])
        clean = ~near.any(axis=1)
        assert np.allclose(g[f"{name}/{k}/d"][clean], ps["d"][clean], rtol=1e-12, atol=0)  # (the reference sums the N weights of a row one by one)
        if near.any():
            continue  # a different W: the eigenvectors are not comparable
        raw = g[f"{name}/{k}/eigvec"]
        v = ref.fix_sign(raw)
        assert np.abs(v - ps["v"]).max() <= 1e-7 * np.abs(ps["v"]).max()
        flipped = bool(np.abs(v - raw).max() > 0)
        bip_raw = g[f"{name}/{k}/bipartition"].astype(bool)
        mine = ref.bipartition(-ps["v"] if flipped else ps["v"])  # the oracle's vector in the reference's (LAPACK's) sign
        assert np.array_equal(mine, bip_raw)
        assert ref.corners(mine, h, w) == int(g[f"{name}/{k}/nc"])
        if ref.seed_margin(ps["v"], ps["reverse"]) > 1e-9:  # (two fp64 solvers: a plateau of v has no definite arg-extremum)
            assert ps["seed"] == int(g[f"{name}/{k}/seed"])
        assert np.array_equal(g[f"{name}/{k}/component"].astype(bool), ps["mask"] if k == 0 else _raw_component(ps, h, w))
        if k >= 1:
            prev = out["passes"][k - 1]
            assert np.array_equal(g[f"{name}/{k}/painting"].astype(bool).reshape(h, w), prev["painted"])  # (recorded as [1, h, w])
            assert np.array_equal(g[f"{name}/{k}/zero_cols"], prev["painted"].reshape(-1))


def _raw_component(ps, h, w):
    """The seed's component before the rejection rule of passes >= 2 (detect_box knows nothing of it)."""
    sd = np.zeros((h, w), dtype=bool)
    sd[np.unravel_index(ps["seed"], (h, w))] = True
    return ref.flood(sd, ps["bip"])


def test_every_fixture_has_the_property_it_is_there_for():
    gaps = {n: [ps["gap"] for ps in oracle(n)[4]["passes"]] for n in ref.FIXTURES}
    assert gaps["8x8"][0] < 1e-4 and all(g[0] > 0.05 for n, g in gaps.items() if n != "8x8")
    assert 0.05 < gaps["9x13"][0] < 0.3 and gaps["32x32"][0] < 0.1
    for n in ("9x13", "32x32", "8x8"):
        out = oracle(n)[4]
        assert len(out["masks"]) == 2 and all(m.sum() > 0 for m in out["masks"]) and not (out["masks"][0] & out["masks"][1]).any()
    for n in ref.FIXTURES:  # the prediction is the labelled objects, so the metrics of the synthetic run mean something
        f, lab, h, w, P = ref.fixture(n)
        tp, fp, fn, tn = ref.counts(oracle(n)[4]["union"], lab > 0)
        assert tp / (tp + fp + fn) > 0.8, n


def test_flood_fill_and_holes_against_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.RandomState(3)
    for h, w in ((1, 9), (9, 1), (7, 11), (16, 16)):
        for _ in range(5):
            m = rng.rand(h, w) < 0.55
            assert np.array_equal(ref.fill_holes(m), ndimage.binary_fill_holes(m))
            lab, n = ndimage.label(m)
            for y, x in zip(*np.nonzero(m)):
                sd = np.zeros((h, w), dtype=bool)
                sd[y, x] = True
                assert np.array_equal(ref.flood(sd, m), lab == lab[y, x])


def test_eigenvector_and_threshold_against_scipy_and_sklearn():
    linalg = pytest.importorskip("scipy.linalg")
    cluster = pytest.importorskip("sklearn.cluster")
    for name in ("5x7", "9x13", "16x16"):
        ps = oracle(name)[4]["passes"][0]
        W = np.where(ps["B"], 1.0, ref.EPS)
        D = np.diag(W.sum(axis=1))
        assert np.allclose(np.diag(D), ps["d"], rtol=1e-12, atol=0)
        lam, vec = linalg.eigh(D - W, D, subset_by_index=[1, 2])
        assert abs(lam[0] - ps["lam"]) <= 1e-10
        assert np.abs(ref.fix_sign(vec[:, 0]) - ps["v"]).max() <= 1e-9 * np.abs(ps["v"]).max()
        km = cluster.KMeans(n_clusters=2, n_init=10, random_state=0).fit(ps["A"].reshape(-1, 1))
        assert abs(float(np.mean(km.cluster_centers_)) - ps["tau"]) <= AFF_TOL


def test_residual_of_the_oracle_vector_is_zero_and_bits_round_trip():
    ps = oracle("9x13")[4]["passes"][1]
    lam, res = ref.residual(ps["B"], ps["d"], ps["v"])
    assert abs(lam - ps["lam"]) <= 1e-12 and res <= 1e-12
    assert np.array_equal(ref.unpack_bits(ref.pack_bits(ps["B"]), 117), ps["B"])


def test_metric_formulas_are_the_reference_scripts():
    """tests/golden/objectness.npz holds the reference script's numbers for recorded masks (the trained probe's validation uses the
    same five helpers as evaluate_generic_objectness.py:50-177)."""
    from mvp.maskcut import METRICS, metrics_from_counts

    rng = np.random.RandomState(0)
    for _ in range(20):
        p, g = rng.rand(12, 12) < 0.4, rng.rand(12, 12) < 0.5
        tp, fp, fn, tn = ref.counts(p, g)
        # the script's formulas written out (evaluate_generic_objectness.py:72-74, 93, 120, 146, 175)
        precision, recall = tp / (tp + fp + 1e-6), tp / (tp + fn + 1e-6)
        want = {"F-measure": 1.09 * precision * recall / (0.09 * precision + recall + 1e-6), "IoU": tp / ((p | g).sum() + 1e-6),
                "Accuracy": (p == g).sum() / p.size, "CorLoc": 1 if tp / ((p | g).sum() + 1e-6) >= 0.5 else 0}
        got, mine = metrics_from_counts(tp, fp, fn, tn), ref.metrics_from_counts(tp, fp, fn, tn)
        for k in METRICS:
            assert abs(got[k] - want[k]) <= 1e-12 and abs(mine[k] - want[k]) <= 1e-12
    empty = metrics_from_counts(0, 0, 0, 144)
    assert empty["F-measure"] == 0.0 and empty["IoU"] == 0.0 and empty["Accuracy"] == 1.0 and empty["CorLoc"] == 0


def test_config_is_the_references_but_for_the_documented_keys():
    """configs/objectness_eval.yaml against the reference's file as parsed (its digest is recorded, not its text)."""
    import yaml

    from conftest import PKG
    from mvp import config

    own = yaml.safe_load(open(os.path.join(PKG, "configs", "objectness_eval.yaml")))
    as_ref = json.loads(json.dumps(own))
    rec = json.load(open(os.path.join(GOLDEN, "reference_config_digest_objectness_eval.json")))
    theirs = rec["reference_values"]  # the four values this package's file changes (its header comment says why)
    as_ref["system"]["num_gpus"] = theirs["num_gpus"]
    as_ref["wandb"]["use"] = theirs["wandb_use"]
    as_ref["defaults"][2] = {"dataset": theirs["dataset"]}
    as_ref["output_dir"] = theirs["output_dir"]
    assert hashlib.sha256(json.dumps(as_ref, sort_keys=True).encode()).hexdigest() == rec["objectness_eval"]
    cfg = config.compose("objectness_eval", ["backbone=dino_b16", "backbone.return_kqv=true", "dataset=synthetic_voc"])
    assert cfg["backbone"]["_target_"] == "evals.models.dino.DINO" and cfg["backbone"]["return_kqv"] is True
    assert cfg["dataset"]["_target_"] == "evals.datasets.synthetic.SyntheticVOC" and cfg["batch_size"] == 16


def test_python_layer_refusals():
    import torch

    from evals.models.maskcut_processor import MaskCutProcessor
    from mvp import lib, maskcut

    with pytest.raises(NotImplementedError, match="crf"):
        MaskCutProcessor(backbone=None, crf=True)
    with pytest.raises(ValueError, match="N <= 1024"):
        maskcut.check_sizes(64, 1025)
    with pytest.raises(ValueError, match="N <= 1024"):
        MaskCutProcessor(backbone=None, patch_size=8, fixed_size=480)  # 60 x 60 cells
    with pytest.raises(ValueError, match="C <= 4096"):
        maskcut.check_sizes(4097, 900)
    with pytest.raises(ValueError, match="N <= 1024"):
        maskcut.maskcut_batch(torch.zeros(1, 8, 33 * 33), 33, 33, [1])
    with pytest.raises(lib.MvpError, match="device tensor"):
        maskcut._need(torch.zeros(2), torch.float32, (2,), "x")
    p = MaskCutProcessor(backbone=None, patch_size=16, tau=0.15, fixed_size=480)
    assert p.patch_size == 16 and p.fixed_size == 480 and p.crf is False
    assert maskcut.CSV_HEADER[:9] == ["Model Name", "Train Avg F-measure", "Train Avg IoU", "Train Avg Accuracy", "Train Avg CorLoc",
                                      "Test Avg F-measure", "Test Avg IoU", "Test Avg Accuracy", "Test Avg CorLoc"]
    assert maskcut.CSV_HEADER[9] == "n_fallback" and len(maskcut.CSV_HEADER) == 10


# ----------------------------------------------------------------------------- MVP_EINVAL, every condition the header names, once each
P8, P4, P1 = 4096, 4100, 4097  # fake pointers: 8-byte aligned, 4-byte aligned only, odd (nothing is launched on a rejected call)


def _einval(fn, args):
    from mvp import lib

    return getattr(lib.load(), fn)(ctypes.byref(args), None) == -1


def _aff(**kw):
    from mvp import lib

    so = lib.load()
    base = dict(feats=P8, painted=P8, active=P8, A=P8, sums=P8, workspace=P8, workspace_bytes=so.mvp_ncut_workspace_bytes(2, 900), ldf=900,
                Bimg=2, C=768, N=900)
    base.update(kw)
    return lib.NcutAffinityArgs(**base)


@pytest.mark.parametrize("bad", [dict(feats=0), dict(A=0), dict(sums=0), dict(workspace=0), dict(Bimg=0), dict(Bimg=65536), dict(N=0),
                                 dict(N=1025), dict(C=0), dict(C=4097), dict(ldf=899), dict(feats=P1), dict(A=P1), dict(sums=P4),
                                 dict(workspace=P4), dict(workspace_bytes=8)])
def test_affinity_einval(bad):
    assert _einval("mvp_ncut_affinity", _aff(**bad))


def test_workspace_query():
    from mvp import lib

    so = lib.load()
    assert so.mvp_ncut_workspace_bytes(2, 900) == 2 * 900 * 4 + 2 * 15 * 15 * 16
    assert so.mvp_ncut_workspace_bytes(1, 35) == 144 + 16  # 140 bytes of norms rounded up to 8
    assert so.mvp_ncut_workspace_bytes(1, 1025) == 0 and so.mvp_ncut_workspace_bytes(0, 900) == 0


def _thr(**kw):
    from mvp import lib

    base = dict(A=P8, sums=P8, active=0, tau=P8, bits=P8, deg=P8, rounds=P8, Bimg=2, N=900, max_rounds=64)
    base.update(kw)
    return lib.NcutThresholdArgs(**base)


@pytest.mark.parametrize("bad", [dict(A=0), dict(sums=0), dict(tau=0), dict(bits=0), dict(deg=0), dict(Bimg=0), dict(N=1025), dict(N=0),
                                 dict(max_rounds=0), dict(A=P1), dict(bits=P1), dict(rounds=P1), dict(sums=P4), dict(tau=P4), dict(deg=P4)])
def test_threshold_einval(bad):
    assert _einval("mvp_ncut_threshold", _thr(**bad))


def _fie(**kw):
    from mvp import lib

    base = dict(bits=P8, deg=P8, active=0, v=P8, residual=P8, iters=P8, converged=P8, Bimg=2, N=900, max_iters=100, r_tol=1e-6, mix_tol=1e-3)
    base["lambda"] = P8
    base.update(kw)
    return lib.NcutFiedlerArgs(**base)


@pytest.mark.parametrize("bad", [dict(bits=0), dict(deg=0), dict(v=0), {"lambda": 0}, dict(residual=0), dict(iters=0), dict(converged=0),
                                 dict(Bimg=0), dict(N=1025), dict(max_iters=0), dict(r_tol=0.0), dict(mix_tol=-1.0), dict(bits=P1), dict(v=P1),
                                 dict(iters=P1), dict(deg=P4), {"lambda": P4}, dict(residual=P4)])
def test_fiedler_einval(bad):
    assert _einval("mvp_ncut_fiedler", _fie(**bad))


def _par(**kw):
    from mvp import lib

    base = dict(v=P8, prev_mask=P8, active=0, pass_mask=P8, painted=P8, union_mask=P8, seed=P8, Bimg=2, h=30, w=30, use_prev=1)
    base.update(kw)
    return lib.NcutPartitionArgs(**base)


@pytest.mark.parametrize("bad", [dict(v=0), dict(pass_mask=0), dict(painted=0), dict(union_mask=0), dict(seed=0), dict(prev_mask=0),
                                 dict(h=0), dict(w=0), dict(h=33, w=32), dict(Bimg=0), dict(Bimg=65536), dict(v=P1), dict(seed=P1)])
def test_partition_einval(bad):
    assert _einval("mvp_ncut_partition", _par(**bad))
