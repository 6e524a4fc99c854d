"""The Python surface of the ScanNet pair correspondence evaluation on the GPU (mvp/corr3d.py, evals/utils/correspondence.py,
render_scannet_correspondence.py) against the fp64 definition of tests/corr_depth_ref.py.  Bounds as in tests/test_gpu_corr3d.py:
delta = 4 * max|D32 - D64| with D32 torch's fp32 CPU evaluation of the same formulas (back-projection and sampling included).

Neighbour identity is only checked where the depth grid is 2 x the feature map: from 3 x on, zero padding followed by the L2
normalisation makes whole border rows / columns exact duplicates of their neighbours, and the nearest among duplicates is decided by
fp32 noise in the reference too."""
import csv
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import _scannet_rank as SR
import corr3d_ref as ref3
import corr_depth_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "midvision-probe_amd")


@pytest.fixture(scope="module")
def pair():
    """C = 64 maps of 12 x 16, depth maps of 24 x 32 (2 x) with 30 % holes; the fp64 reference of the full problem, computed once."""
    g = torch.Generator().manual_seed(31)
    f0, f1 = torch.randn(64, 12, 16, generator=g), torch.randn(64, 12, 16, generator=g)
    d0, d1 = torch.rand(1, 24, 32, generator=g) * 2 + 0.5, torch.rand(1, 24, 32, generator=g) * 2 + 0.5
    d0[0][torch.rand(24, 32, generator=g) < 0.3] = 0.0
    d1[0][torch.rand(24, 32, generator=g) < 0.3] = 0.0
    K = torch.tensor([[23.0, 0.0, 17.2], [0.0, 24.5, 10.8], [0.0, 0.0, 1.0]])
    r = ref.estimate_correspondence_depth(f0, f1, d0, d1, K, 10 ** 6)
    r32 = ref.estimate_correspondence_depth(f0, f1, d0, d1, K, 10 ** 6, torch.float32)
    delta = 4 * float((r32["D"].double() - r["D"]).abs().max())
    assert 1e-8 < delta < 2e-5
    return f0, f1, d0, d1, K, r, delta


@pytest.mark.parametrize("num_corr", [50, 10 ** 6])  # below and above the number of valid cells of view 0
def test_estimate_correspondence_depth(pair, num_corr):
    from evals.utils.correspondence import estimate_correspondence_depth, grid_to_pointcloud
    from mvp import corr3d

    f0, f1, d0, d1, K, r, delta = pair
    n_valid = int(r["valid_0"].sum())
    assert 50 < n_valid < 768
    dev = [t.to(DEV) for t in (f0, f1, d0, d1)]
    keep = [t.clone() for t in (f0, f1, d0, d1, K)]
    xyz0, xyz1, dist = [t.cpu() for t in estimate_correspondence_depth(*dev, K, num_corr=num_corr)]
    assert all(torch.equal(a, b) for a, b in zip(keep, (f0, f1, d0, d1, K))) and all(torch.equal(a.cpu(), b) for a, b in zip(dev, keep))
    n = min(num_corr, n_valid)
    assert len(xyz0) == len(xyz1) == len(dist) == n
    assert (dist[:-1] >= dist[1:]).all()  # sorted descending
    # the cells behind the results: gathered xyz are the back-projected grids' own rows at the selected cells, bit for bit
    m = corr3d.match_depth(*dev, K, num_corr=num_corr)
    assert len(m["idx0"]) == min(num_corr, 768) and int(m["count"]) == n
    idx0, idx1 = m["idx0"][:n].cpu(), m["idx1"][:n].cpu()
    flat0 = grid_to_pointcloud(K.inverse().to(DEV), dev[2]).cpu()
    flat1 = grid_to_pointcloud(K.inverse().to(DEV), dev[3]).cpu()
    assert flat0.shape == flat1.shape == (768, 3)
    assert torch.equal(flat0[idx0], xyz0) and torch.equal(flat1[idx1], xyz1) and torch.equal(m["dist"][:n].cpu(), dist)
    np.testing.assert_allclose(flat0.double().numpy(), r["xyz_0"].numpy(), rtol=2e-6, atol=1e-6)
    np.testing.assert_allclose(flat1.double().numpy(), r["xyz_1"].numpy(), rtol=2e-6, atol=1e-6)
    assert len(set(idx0.tolist())) == n and r["valid_0"][idx0].all() and r["valid_1"][idx1].all()
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


def test_sample_pointcloud_features_is_the_transposed_view_and_leaves_its_arguments(pair):
    from evals.utils.correspondence import sample_pointcloud_features

    f0, _, d0, _, K, r, _ = pair
    pc = r["xyz_0"].float()
    args = [f0.to(DEV), K.to(DEV), pc.to(DEV)]
    got = sample_pointcloud_features(*args, (24, 32))
    assert got.shape == (768, 64) and got.t().is_contiguous()
    assert torch.equal(args[0].cpu(), f0) and torch.equal(args[1].cpu(), K) and torch.equal(args[2].cpu(), pc)
    S32 = ref.sample_pointcloud_features(f0, K, pc, (24, 32), torch.float32)
    ds = 4 * float((S32.double() - r["f0"]).abs().max())
    assert 1e-8 < ds < 1e-4
    assert (got.cpu().double() - r["f0"]).abs().max() <= ds
    assert torch.equal(sample_pointcloud_features(args[0], K, args[2], (24, 32)), got)  # a host K gives the same bits


def reference_pairs(stub, ds, num_corr, scale):
    """evaluate_scannet by the fp64 definition, from the stub's features: per pair the error vectors (3-D, 2-D) of the selected
    correspondences, and the same for the SECOND nearest target of every selected row whose neighbour is not decided in fp32
    (gap <= 2 delta) — what an fp32 evaluation may legitimately report instead."""
    out = []
    for i in range(len(ds)):
        it = ds[i]
        deps = torch.nn.functional.interpolate(torch.stack((it["depth_0"], it["depth_1"])), scale_factor=scale, mode="nearest")
        K = it["K"].clone()
        K[:2, :] *= scale
        fa, fb = stub.features(it["rgb_0"]), stub.features(it["rgb_1"])
        r = ref.estimate_correspondence_depth(fa, fb, deps[0], deps[1], K, num_corr)
        r32 = ref.estimate_correspondence_depth(fa, fb, deps[0], deps[1], K, num_corr, torch.float32)
        delta = 4 * float((r32["D"].double() - r["D"]).abs().max())

        def errors(idx0, idx1):
            p01 = ref3.transform(r["xyz_0"][idx0], it["Rt_1"])
            p1 = r["xyz_1"][idx1]
            return (p01 - p1).norm(dim=1), (ref3.project(p01, K) - ref3.project(p1, K)).norm(dim=1)

        e3, e2 = errors(r["idx0"], r["idx1"])
        gap = (r["dist"][:, 1] - r["dist"][:, 0])[r["idx0"]]
        unclear = r["idx0"][gap <= 2 * delta]
        second = ref3.two_nearest(r["D"][unclear], r["valid_1"])[0][:, 1]
        a3, a2 = errors(unclear, second)
        out.append({"e3": e3, "e2": e2, "alt3": a3, "alt2": a2, "unclear": (gap <= 2 * delta), "R": it["Rt_1"][:3, :3], "n_valid": int(r["valid_0"].sum())})
    return out


def thresholds_are_clear(pairs):
    """No error within 1e-4 relative of any of the 15 thresholds, and an undecided neighbour's alternative falls on the same side."""
    for p in pairs:
        for e, alt, ths in ((p["e2"], p["alt2"], ref.PX_THRESH), (p["e3"], p["alt3"], ref.M_THRESH)):
            for th in ths:
                if ((e - th).abs() <= 1e-4 * th).any() or ((alt - th).abs() <= 1e-4 * th).any():
                    return False
                if not torch.equal(e[p["unclear"]] < th, alt < th):
                    return False
    return True


def test_evaluate_scannet_with_ground_truth_features_equals_the_fp64_definition():
    """Features that are a projection of the true 3-D point: 128 x 160 images, patch 8, scale 0.25 -> features 16 x 20, depth
    32 x 40 (2 x).  Every valid cell is selected (num_corr above their number), so the recalls depend on the nearest neighbours
    alone.  First, on the fp64 reference alone: no correspondence error lies within 1e-4 relative of a threshold (and where the
    neighbour itself is not decided in fp32, the runner-up's error falls on the same side of every threshold) — that is how the
    dataset seed was chosen — so an fp32 evaluation has to give the same 19 numbers."""
    from mvp import corr3d

    ds = SR.dataset(3, seed=SR.GT_SEED)
    stub = SR.GroundTruthFeatures(ds)
    pairs = reference_pairs(stub, ds, 4096, SR.SCALE)
    assert all(0 < p["n_valid"] < 1280 and len(p["e3"]) == p["n_valid"] for p in pairs)
    assert thresholds_are_clear(pairs)
    want = ref.recalls([p["e3"] for p in pairs], [p["e2"] for p in pairs], torch.stack([p["R"] for p in pairs]))
    got = corr3d.evaluate_scannet(stub.to(DEV), ds, 4096, SR.SCALE, False)
    print("fp64", want, "\ngpu ", got, "\nundecided neighbours per pair", [int(p["unclear"].sum()) for p in pairs])
    assert len(got) == 19 and all(isinstance(v, float) for v in got)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9, equal_nan=True)
    assert sum(not math.isnan(v) for v in got[15:]) >= 2  # at least two angle bins filled
    assert all(a <= b for a, b in zip(got[:6], got[1:7])) and all(a <= b for a, b in zip(got[7:14], got[8:15]))  # monotone in the threshold
    assert got[9] > 50.0  # the 5 cm recall


def _same(a, b):
    return all(x == y or (math.isnan(x) and math.isnan(y)) for x, y in zip(a, b))


def test_evaluate_scannet_pipelined_equals_strictly_serial_forwards(monkeypatch):
    """Forwards kept in flight (mvp.pipeline) against MVP_INFLIGHT=1 (every forward inline on the caller's stream), a fresh wrapper
    each: the 19 numbers bit for bit.  And against a plain loop of the public functions, one forward per stacked pair."""
    from mvp import corr3d
    from mvp import functional as MF

    ds = SR.dataset()
    monkeypatch.delenv("MVP_INFLIGHT", raising=False)
    piped = corr3d.evaluate_scannet(SR.build_vit(DEV), ds, SR.NUM_CORR, SR.SCALE, False)
    monkeypatch.setenv("MVP_INFLIGHT", "1")
    serial = corr3d.evaluate_scannet(SR.build_vit(DEV), ds, SR.NUM_CORR, SR.SCALE, False)
    assert len(piped) == 19 and _same(piped, serial), (piped, serial)

    model = SR.build_vit(DEV)
    e3, e2, Rs = [], [], []
    for i in range(len(ds)):
        it = ds[i]
        with torch.no_grad():
            feats = model(torch.stack((it["rgb_0"], it["rgb_1"])).to(DEV)).clone()
        deps = MF.interpolate(torch.stack((it["depth_0"], it["depth_1"])).to(DEV), scale_factor=SR.SCALE, mode="nearest")
        K = it["K"].clone()
        K[:2, :] *= SR.SCALE
        c0, c1, _ = corr3d.estimate_correspondence_depth(feats[0], feats[1], deps[0], deps[1], K, SR.NUM_CORR)
        Rt, Kd = it["Rt_1"][:3, :4].to(DEV), K.to(DEV)
        c01 = corr3d.transform_points_Rt(c0, Rt)
        e3.append((c01 - c1).norm(p=2, dim=1).cpu())
        e2.append((corr3d.project_3dto2d(c01, Kd) - corr3d.project_3dto2d(c1, Kd)).norm(p=2, dim=1).cpu())
        Rs.append(it["Rt_1"][:3, :3])
    loop = corr3d.summarize_scannet(e3, e2, torch.stack(Rs))
    assert _same(piped, loop), (piped, loop)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_with_sharded_pairs_equal_one_rank(tmp_path):
    from mvp import corr3d

    one = corr3d.evaluate_scannet(SR.build_vit(DEV), SR.dataset(), SR.NUM_CORR, SR.SCALE, False)
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   MVP_DIST_BACKEND="gloo", MVP_FORCE_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "_scannet_rank.py"), str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        assert p.returncode == 0, o.decode(errors="replace")[-3000:]
    for r in range(2):
        got = np.load(os.path.join(tmp_path, f"scannet{r}.npz"))
        assert int(got["world"]) == 2 and str(got["backend"]) == "gloo"
        np.testing.assert_array_equal(got["numbers"], np.array(one, dtype=np.float64))


def test_scannet_entrypoint_writes_the_reference_csv_row(tmp_path):
    args = ["backbone=dino_b16", "image_height=128", "image_width=160", "num_instances=2", "num_corr=50", f"output_dir={tmp_path}/out"]
    p = subprocess.run([sys.executable, os.path.join(PKG, "render_scannet_correspondence.py")] + args, cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-4000:]
    assert "3D Recall (0.02m)" in out and "2D Recall (15px)" in out and "Bin Rec 30-60°" in out
    rows = list(csv.reader(open(tmp_path / "out" / "scannet_correspondence_final.csv")))
    assert len(rows) == 2
    assert rows[0] == ["Time", "Model Checkpoint", "Patch Size", "Layer", "Output", "Dataset", "Num Correspondences", "Scale Factor",
                       "2D Recall (1px)", "2D Recall (2px)", "2D Recall (5px)", "2D Recall (15px)", "2D Recall (25px)", "2D Recall (35px)",
                       "2D Recall (50px)", "3D Recall (0.01m)", "3D Recall (0.02m)", "3D Recall (0.05m)", "3D Recall (0.1m)", "3D Recall (0.2m)",
                       "3D Recall (0.3m)", "3D Recall (0.4m)", "3D Recall (0.5m)", "Bin Rec 0-30°", "Bin Rec 30-60°", "Bin Rec 60-90°",
                       "Bin Rec 90-120°"]
    assert len(rows[0]) == 27 and len(rows[1]) == 27
    assert rows[1][4] == "dense" and rows[1][5] == "synthetic_scannet" and rows[1][6] == "50" and rows[1][7] == "0.25"
    assert all(0.0 <= float(v) <= 100.0 for v in rows[1][8:23])
    assert sum(not math.isnan(float(v)) for v in rows[1][23:]) == 2  # two pairs, two angle bins: the bin columns hold recalls
