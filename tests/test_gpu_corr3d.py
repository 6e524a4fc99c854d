"""The Python surface of the NAVI 3-D correspondence evaluation on the GPU (mvp/corr3d.py, evals/utils/correspondence.py,
evaluate_navi_correspondence.py) against the fp64 definition of tests/corr3d_ref.py.  Bounds as in tests/test_gpu_knn.py:
delta = 4 * max|D32 - D64| with D32 torch's fp32 CPU evaluation of the same formula (bicubic upsampling included)."""
import csv
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import _navi_rank as NR
import corr3d_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "midvision-probe_amd")


@pytest.fixture(scope="module")
def pair():
    """C = 64 maps of 6 x 6, xyz grids of 24 x 24 whose masks have holes; the fp64 reference of the full problem, computed once."""
    g = torch.Generator().manual_seed(31)
    f0, f1 = torch.randn(64, 6, 6, generator=g), torch.randn(64, 6, 6, generator=g)
    x0, x1 = torch.rand(3, 24, 24, generator=g) + 0.2, torch.rand(3, 24, 24, generator=g) + 0.2
    x0[2][torch.rand(24, 24, generator=g) < 0.3] = 0.0
    x1[2][torch.rand(24, 24, generator=g) < 0.3] = 0.0
    r = ref.estimate_correspondence_xyz(f0, f1, x0, x1, 10 ** 6)
    up32 = lambda f: torch.nn.functional.interpolate(f[None], size=(24, 24), mode="bicubic")[0].reshape(64, -1).t()  # noqa: E731
    delta = 4 * float((ref.distance_matrix(up32(f0), up32(f1), torch.float32).double() - r["D"]).abs().max())
    assert 1e-8 < delta < 2e-5
    return f0, f1, x0, x1, r, delta


@pytest.mark.parametrize("num_corr", [50, 1000])  # below and above the number of valid cells of view 0
def test_estimate_correspondence_xyz(pair, num_corr):
    from evals.utils.correspondence import estimate_correspondence_xyz
    from mvp import corr3d

    f0, f1, x0, x1, r, delta = pair
    n_valid = int(r["valid_0"].sum())
    assert 50 < n_valid < 576
    dev = [t.to(DEV) for t in (f0, f1, x0, x1)]
    xyz0, xyz1, dist, uv0, uv1 = [t.cpu() for t in estimate_correspondence_xyz(*dev, num_corr=num_corr)]
    n = min(num_corr, n_valid)
    assert len(xyz0) == len(xyz1) == len(dist) == len(uv0) == len(uv1) == n
    assert (dist[:-1] >= dist[1:]).all()  # sorted descending
    # the cells behind the results: pixel centres -> grid indices; gathered xyz / uv are the grids' own values there, bit for bit
    flat0, flat1 = x0.permute(1, 2, 0).reshape(-1, 3), x1.permute(1, 2, 0).reshape(-1, 3)
    centres = ref.get_grid(24, 24).permute(1, 2, 0).reshape(-1, 3)[:, :2].float()
    idx0 = uv0[:, 1].floor().long() * 24 + uv0[:, 0].floor().long()
    idx1 = uv1[:, 1].floor().long() * 24 + uv1[:, 0].floor().long()
    assert torch.equal(centres[idx0], uv0) and torch.equal(centres[idx1], uv1)
    assert torch.equal(flat0[idx0], xyz0) and torch.equal(flat1[idx1], xyz1)
    assert len(set(idx0.tolist())) == n and r["valid_0"][idx0].all() and r["valid_1"][idx1].all()
    m = corr3d.match_grids(*dev, num_corr=num_corr)
    assert int(m["count"]) == n and torch.equal(m["idx0"][:n].cpu(), idx0) and torch.equal(m["idx1"][:n].cpu(), idx1)
    # per row: the weight within the first-order bound of 1 - d1 / d2, the neighbour the fp64 one wherever its gap is clear
    d64, w64, nn64 = r["dist"][idx0], r["all_weight"][idx0], r["nn"][idx0]
    bound = 4 * delta / d64[:, 1].clamp(min=1e-9)
    assert ((dist.double() - w64).abs() <= bound).all()
    clear = (d64[:, 1] - d64[:, 0]) > 2 * delta
    assert torch.equal(idx1[clear], nn64[clear])
    all_gap = (r["dist"][:, 1] - r["dist"][:, 0])[r["valid_0"]]
    assert (all_gap <= 2 * delta).double().mean() <= 0.01  # (over every valid row of the problem: the exemption hides nothing)
    # the selection: every selected weight reaches the fp64 k-th weight up to its row's bound
    kth = torch.sort(r["all_weight"][r["valid_0"]], descending=True).values[n - 1]
    assert (dist.double() >= kth - bound).all()
    if n == n_valid:
        assert set(idx0.tolist()) == set(torch.nonzero(r["valid_0"])[:, 0].tolist())


def _clear_topk(weights, k, margin):
    """The fp64 top-k of ``weights`` is decided by more than ``margin`` at every rank down to the one that falls out."""
    s = torch.sort(weights, descending=True).values[:k + 1]
    return bool(((s[:-1] - s[1:]) > margin).all())


def test_get_correspondences_ratio_test_forms():
    from evals.utils.correspondence import get_correspondences_ratio_test

    g = torch.Generator().manual_seed(41)
    P1, P2 = torch.randn(200, 64, generator=g), torch.randn(230, 64, generator=g)
    D = ref.distance_matrix(P1, P2)
    delta = 4 * float((ref.distance_matrix(P1, P2, torch.float32).double() - D).abs().max())
    i12, d12 = ref.two_nearest(D)
    i21, d21 = ref.two_nearest(D.t().contiguous())
    w12, w21 = ref.ratio_weight(d12), ref.ratio_weight(d21)
    b12, b21 = 4 * delta / d12[:, 1], 4 * delta / d21[:, 1]
    assert _clear_topk(w12, 30, 2 * float(b12.max())) and _clear_topk(w12, 20, 2 * float(b12.max())) and _clear_topk(w21, 20, 2 * float(b21.max()))
    assert _clear_topk(d12[:, 0], 30, 2 * delta)
    dev1, dev2 = P1.to(DEV), P2.to(DEV)

    a1, a2, aw = [t.cpu() for t in get_correspondences_ratio_test(dev1, dev2, 30)]
    s, t, w = ref.topk_matches(w12, i12[:, 0], 30)
    assert torch.equal(a1, s) and torch.equal(a2, t) and ((aw.double() - w).abs() <= b12[s]).all()

    # ratio_test=False: the weight is the nearest distance itself, so the LARGEST nearest distances are kept (reference quirk)
    a1, a2, aw = [t.cpu() for t in get_correspondences_ratio_test(dev1, dev2, 30, ratio_test=False)]
    s, t, w = ref.topk_matches(d12[:, 0], i12[:, 0], 30)
    assert torch.equal(a1, s) and torch.equal(a2, t) and ((aw.double() - w).abs() <= delta).all()
    assert w[0] == d12[:, 0].max()

    # bidirectional: num_corres // 2 each way, P1 -> P2 first; the second half's P1 indices are the neighbours of its P2 queries
    a1, a2, aw = [t.cpu() for t in get_correspondences_ratio_test(dev1, dev2, 41, bidirectional=True)]
    s12, t12, v12 = ref.topk_matches(w12, i12[:, 0], 20)
    s21, t21, v21 = ref.topk_matches(w21, i21[:, 0], 20)
    assert len(a1) == len(a2) == len(aw) == 40
    assert torch.equal(a1, torch.cat((s12, t21))) and torch.equal(a2, torch.cat((t12, s21)))
    assert ((aw.double() - torch.cat((v12, v21))).abs() <= torch.cat((b12[s12], b21[s21]))).all()


def _reference_numbers(stub, ds, num_corr, scale):
    """evaluate_dataset by the fp64 definition, from the stub's features."""
    e3, e2, Rs = [], [], []
    for i in range(len(ds)):
        it = ds[i]
        x0 = torch.nn.functional.interpolate(it["xyz_grid_0"][None], scale_factor=scale, mode="nearest")[0]
        x1 = torch.nn.functional.interpolate(it["xyz_grid_1"][None], scale_factor=scale, mode="nearest")[0]
        r = ref.estimate_correspondence_xyz(stub.features(it["image_0"]), stub.features(it["image_1"]), x0, x1, num_corr)
        p01 = ref.transform(x0.permute(1, 2, 0).reshape(-1, 3)[r["idx0"]], it["Rt_01"])
        p1 = x1.permute(1, 2, 0).reshape(-1, 3)[r["idx1"]].double()
        e3.append((p01 - p1).norm(dim=1))
        e2.append((ref.project(p01, it["intrinsics_1"]) - ref.project(p1, it["intrinsics_1"])).norm(dim=1))
        Rs.append(it["Rt_01"][:3, :3])
    return ref.recalls(e3, e2, torch.stack(Rs))


def test_evaluate_dataset_with_ground_truth_features_equals_the_fp64_definition():
    """Features that are a projection of the true 3-D point make nearby cells nearly parallel (nearest cosine distances of 1e-5 to
    1e-4), where the RANKING by 1 - d1 / d2 is decided below fp32 resolution — torch's own fp32 CPU evaluation of the reference
    formulas already gives another 2 cm recall than fp64 at num_corr = 60 (73.75 against 73.33).  So every valid cell is selected
    (num_corr above their number): the recalls then depend on the nearest neighbours alone, which are decided well above delta."""
    from mvp import corr3d

    ds = NR.dataset(4)
    stub = NR.GroundTruthFeatures(ds)
    want = _reference_numbers(stub, ds, 4096, NR.SCALE)
    got = corr3d.evaluate_dataset(stub.to(DEV), ds, 4096, NR.SCALE, False, batch_size=4)
    print("fp64", want, "\ngpu ", got)
    assert len(got) == 10 and all(isinstance(v, float) for v in got)
    assert got[1] == pytest.approx(want[1], abs=1e-9) and got[4] == pytest.approx(want[4], abs=1e-9)  # 2 cm and 25 px recalls
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9, equal_nan=True)
    assert 20.0 < got[1] <= 100.0 and got[0] <= got[1] <= got[2] and got[3] <= got[4] <= got[5]
    assert math.isnan(got[9]) and sum(not math.isnan(v) for v in got[6:]) >= 2  # three angle bins filled, the last one empty


def test_evaluate_dataset_pipelined_equals_strictly_serial_forwards(monkeypatch):
    """Forwards kept in flight (mvp.pipeline) against MVP_INFLIGHT=1 (every forward inline on the caller's stream), a fresh wrapper
    each: the ten numbers bit for bit.  And against a plain loop of the public functions, two separate forwards per batch."""
    from mvp import corr3d
    from mvp import functional as MF

    ds = NR.dataset()
    monkeypatch.delenv("MVP_INFLIGHT", raising=False)
    piped = corr3d.evaluate_dataset(NR.build_vit(DEV), ds, NR.NUM_CORR, NR.SCALE, False, batch_size=NR.BATCH)
    monkeypatch.setenv("MVP_INFLIGHT", "1")
    serial = corr3d.evaluate_dataset(NR.build_vit(DEV), ds, NR.NUM_CORR, NR.SCALE, False, batch_size=NR.BATCH)
    assert all(a == b or (math.isnan(a) and math.isnan(b)) for a, b in zip(piped, serial)), (piped, serial)

    model = NR.build_vit(DEV)
    e3, e2, Rs = [], [], []
    for s in range(0, len(ds), NR.BATCH):
        items = [ds[i] for i in range(s, min(s + NR.BATCH, len(ds)))]
        with torch.no_grad():
            f0 = model(torch.stack([it["image_0"] for it in items]).to(DEV)).clone()
            f1 = model(torch.stack([it["image_1"] for it in items]).to(DEV)).clone()
        for j, it in enumerate(items):
            x0 = MF.interpolate(it["xyz_grid_0"][None].to(DEV), scale_factor=NR.SCALE, mode="nearest")[0]
            x1 = MF.interpolate(it["xyz_grid_1"][None].to(DEV), scale_factor=NR.SCALE, mode="nearest")[0]
            c0, c1, _, _, _ = corr3d.estimate_correspondence_xyz(f0[j], f1[j], x0, x1, NR.NUM_CORR)
            Rt, K = it["Rt_01"].to(DEV), it["intrinsics_1"].to(DEV)
            c01 = corr3d.transform_points_Rt(c0, Rt[:3, :4])
            e3.append((c01 - c1).norm(p=2, dim=1).cpu())
            e2.append((corr3d.project_3dto2d(c01, K) - corr3d.project_3dto2d(c1, K)).norm(p=2, dim=1).cpu())
            Rs.append(it["Rt_01"][:3, :3])
    loop = corr3d.summarize(e3, e2, torch.stack(Rs))
    assert all(a == b or (math.isnan(a) and math.isnan(b)) for a, b in zip(piped, loop)), (piped, loop)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_with_sharded_batches_equal_one_rank(tmp_path):
    from mvp import corr3d

    one = corr3d.evaluate_dataset(NR.build_vit(DEV), NR.dataset(), NR.NUM_CORR, NR.SCALE, False, batch_size=NR.BATCH)
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   MVP_DIST_BACKEND="gloo", MVP_FORCE_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "_navi_rank.py"), str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        assert p.returncode == 0, o.decode(errors="replace")[-3000:]
    for r in range(2):
        got = np.load(os.path.join(tmp_path, f"navi{r}.npz"))
        assert int(got["world"]) == 2 and str(got["backend"]) == "gloo"
        np.testing.assert_array_equal(got["numbers"], np.array(one, dtype=np.float64))


def test_navi_entrypoint_writes_the_reference_csv_row(tmp_path):
    args = ["backbone=dino_b16", "image_size=128", "num_instances=2", "num_corr=50", f"output_dir={tmp_path}/out"]
    p = subprocess.run([sys.executable, os.path.join(PKG, "evaluate_navi_correspondence.py")] + args, cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-4000:]
    assert "3D Recall (0.02m)" in out and "Bin Rec 30-60°" in out
    rows = list(csv.reader(open(tmp_path / "out" / "navi_correspondence_final.csv")))
    assert len(rows) == 2
    assert rows[0] == ["Time", "Model Checkpoint", "Patch Size", "Layer", "Output", "Num Correspondences", "Scale Factor", "Dataset",
                       "3D Recall (0.01m)", "3D Recall (0.02m)", "3D Recall (0.05m)", "2D Recall (5px)", "2D Recall (25px)", "2D Recall (50px)",
                       "Bin Rec 0-30°", "Bin Rec 30-60°", "Bin Rec 60-90°", "Bin Rec 90-120°"]
    assert len(rows[1]) == len(rows[0]) and rows[1][4] == "dense" and rows[1][5] == "50" and rows[1][6] == "0.25" and rows[1][7] == "synthetic_navi"
    assert all(0.0 <= float(v) <= 100.0 for v in rows[1][8:14])
