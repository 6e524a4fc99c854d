"""CPU checks of the ScanNet pairs' depth path: the fp64 definition the GPU tests use (tests/corr_depth_ref.py) reproduces goldens
recorded from the reference's own functions (tests/golden/make_goldens_corr_depth.py) and equals torch's fp64 grid_sample, error_auc
matches its golden, mvp_pointcloud_sample validates its arguments before any launch, SyntheticScanNetPairs is geometrically exact
and deterministic, the config composes and evals.utils.correspondence exports the reference's names."""
import ctypes
import math

import numpy as np
import pytest
import torch

import corr3d_ref as ref3
import corr_depth_ref as ref
from conftest import load_golden


@pytest.fixture(scope="module")
def G():
    return {k: torch.from_numpy(v) for k, v in load_golden("corr_depth.npz").items()}


def _clear_topk(weights, k, margin):
    """The fp64 top-k of ``weights`` is decided by more than ``margin`` at every rank down to the one that falls out."""
    s = torch.sort(weights, descending=True).values[:k + 1]
    return bool(((s[:-1] - s[1:]) > margin).all())


def test_fp64_back_projection_and_sampling_reproduce_the_reference(G):
    K = G["K"]
    pts = ref.grid_to_pointcloud(K.inverse(), G["e2e_depth_0"])
    assert pts.shape == (12 * 16, 3) == G["g2p_points"].shape
    np.testing.assert_allclose(pts.numpy(), G["g2p_points"].numpy(), rtol=2e-6, atol=1e-6)
    assert (G["g2p_points"][G["e2e_depth_0"].reshape(-1) == 0] == 0).all()  # a hole back-projects to the origin
    # the sampling case: inside, border band, outside, z = 0 and z < 0; bound from the fp32 evaluation of the same formulas
    pc, feat = G["samp_pc"], G["samp_feat"]
    S64 = ref.sample_pointcloud_features(feat, K, pc, (12, 16))
    S32 = ref.sample_pointcloud_features(feat, K, pc, (12, 16), torch.float32)
    delta = 4 * float((S32.double() - S64).abs().max())
    assert 1e-8 < delta < 1e-4
    assert (G["samp_out"].double() - S64).abs().max() <= delta
    x, y, ok = ref.sample_positions(K, pc, (6, 8), (12, 16))
    assert 10 < int(ok.sum()) < 50 and not ok[40:46].any() and (pc[40:43, 2] == 0).all() and (pc[43:46, 2] < 0).all()
    assert (S64[~ok] == 0).all() and (G["samp_out"][~ok] == 0).all()
    band = ok & ((x < 0) | (x > 7) | (y < 0) | (y > 5))
    assert int(band.sum()) >= 4 and (S64[band].abs().max(dim=1).values > 0).all()


def test_fp64_sampling_equals_torch_fp64_grid_sample(G):
    g = torch.Generator().manual_seed(3)
    K = G["K"].double()
    feat = torch.randn(7, 5, 9, generator=g, dtype=torch.float64)
    pc = torch.randn(400, 3, generator=g, dtype=torch.float64)
    pc[:, 2] = pc[:, 2].abs() + 0.3
    pc[:8, 2] = 0.0
    pc[8:16, 2] = -1.0
    H, W = 12, 16
    for cloud in (pc, ref.grid_to_pointcloud(K.inverse(), torch.rand(1, H, W, generator=g, dtype=torch.float64) + 0.5)):
        uvd = cloud @ K.t()
        uv = uvd[:, :2] / uvd[:, 2:3].clamp(min=1e-9)
        uv = torch.stack((2 * uv[:, 0] / W - 1, 2 * uv[:, 1] / H - 1), dim=1)
        want = torch.nn.functional.grid_sample(feat[None], uv[None, None], mode="bilinear", padding_mode="zeros", align_corners=False)[0, :, 0].t()
        got = ref.sample_pointcloud_features(feat, K, cloud, (H, W))
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=1e-11)


@pytest.mark.parametrize("case,num_corr", [("a", 40), ("b", 1000)])
def test_fp64_definition_reproduces_the_reference_end_to_end(G, case, num_corr):
    """estimate_correspondence_depth of the reference (faiss replaced by its definition while recording) against the grid-index form:
    the same cells in the same order, the reference's fp32 weights within fp32 rounding of the fp64 ones."""
    from mvp import corr3d

    K, f0, f1, d0, d1 = G["K"], G["e2e_feat_0"], G["e2e_feat_1"], G["e2e_depth_0"], G["e2e_depth_1"]
    r = ref.estimate_correspondence_depth(f0, f1, d0, d1, K, num_corr)
    r32 = ref.estimate_correspondence_depth(f0, f1, d0, d1, K, num_corr, torch.float32)
    delta = 4 * float((r32["D"].double() - r["D"]).abs().max())
    v0 = r["valid_0"]
    n_valid = int(v0.sum())
    assert 0.15 < 1 - n_valid / 192 < 0.35 and 0.15 < 1 - int(r["valid_1"].sum()) / 192 < 0.35
    assert torch.equal(v0, d0.reshape(-1) > 0)
    bound = 4 * delta / r["dist"][v0][:, 1]
    assert 1e-8 < delta < 2e-5
    assert _clear_topk(r["all_weight"][v0], 40, 2 * float(bound.max()))  # how the recording's seed was chosen
    n = min(num_corr, n_valid)
    assert len(r["idx0"]) == n == len(G[f"e2e_{case}_dist"])
    # the reference's compacted fp32 clouds are the back-projected grids' own rows (the package's fp32 torch plumbing, on the CPU here)
    flat0 = corr3d.grid_to_pointcloud(K.inverse(), d0)
    flat1 = corr3d.grid_to_pointcloud(K.inverse(), d1)
    np.testing.assert_allclose(flat0.double().numpy(), r["xyz_0"].numpy(), rtol=2e-6, atol=1e-6)
    if case == "a":
        assert torch.equal(flat0[r["idx0"]], G["e2e_a_xyz0"]) and torch.equal(flat1[r["idx1"]], G["e2e_a_xyz1"])
        np.testing.assert_allclose(r["weight"].numpy(), G["e2e_a_dist"].numpy(), rtol=0, atol=float(bound.max()))
    else:
        # every valid cell is selected; below rank 40 the ORDER of near-equal weights is fp32's to decide, so rows are matched by cell
        key = lambda a, b: sorted(zip(map(tuple, a.tolist()), map(tuple, b.tolist())))  # noqa: E731
        assert key(flat0[r["idx0"]], flat1[r["idx1"]]) == key(G["e2e_b_xyz0"], G["e2e_b_xyz1"])
        assert torch.equal(flat0[r["idx0"][:40]], G["e2e_b_xyz0"][:40])
        np.testing.assert_allclose(r["weight"].numpy(), G["e2e_b_dist"].numpy(), rtol=0, atol=float(bound.max()))
    assert (r["valid_0"][r["idx0"]]).all() and (r["valid_1"][r["idx1"]]).all()


def test_error_auc_and_exports(G):
    from evals.utils import correspondence as C
    from mvp import corr3d, lib

    got = C.error_auc(G["auc_errors"].tolist(), G["auc_thresholds"].tolist())
    np.testing.assert_allclose(np.array(got), G["auc_out"].numpy(), rtol=1e-12, atol=0)
    assert len(got) == 3 and 0 < got[0] < got[1] < got[2] < 1
    for name in ("grid_to_pointcloud", "sample_pointcloud_features", "estimate_correspondence_depth", "error_auc"):
        assert getattr(C, name) is getattr(corr3d, name)
    assert torch.equal(C.grid_to_pointcloud(G["K"].inverse(), G["e2e_depth_0"]), G["g2p_points"])
    # the hot path has no CPU fallback
    with pytest.raises(lib.MvpError):
        C.sample_pointcloud_features(G["samp_feat"], G["K"], G["samp_pc"], (12, 16))
    with pytest.raises(lib.MvpError):
        C.estimate_correspondence_depth(G["e2e_feat_0"], G["e2e_feat_1"], G["e2e_depth_0"], G["e2e_depth_1"], G["K"])


def test_pointcloud_sample_abi_struct_and_einval():
    from mvp import lib

    so = lib.load()
    assert so.mvp_sizeof(b"mvp_pointcloud_sample_args") == ctypes.sizeof(lib.PointcloudSampleArgs) == 72
    assert lib.STRUCTS["mvp_pointcloud_sample_args"] is lib.PointcloudSampleArgs
    assert lib.SYMBOLS["mvp_pointcloud_sample"] is lib.PointcloudSampleArgs
    assert lib.info().abi_version == 8
    ok = dict(feat=256, pc=256, K=256, out=256, valid=256, C=4, fh=3, fw=5, N=8, H=6, W=10, ld_out=8)

    def rc(**kw):
        return so.mvp_pointcloud_sample(ctypes.byref(lib.PointcloudSampleArgs(**{**ok, **kw})), None)

    assert so.mvp_pointcloud_sample(None, None) == -1
    for field in ("feat", "pc", "K", "out"):
        assert rc(**{field: None}) == -1, field
    for field in ("C", "fh", "fw", "N", "H", "W", "ld_out"):
        assert rc(**{field: 0}) == -1 and rc(**{field: -2}) == -1, field
    assert rc(ld_out=7) == -1
    assert rc(N=(1 << 24) + 1, ld_out=(1 << 24) + 1) == -1


def test_synthetic_scannet_pairs_are_exact_and_deterministic():
    """A view-0 depth pixel, back-projected, moved by Rt_1 and projected with K, lands in some pixel of view 1.  Where that pixel has
    a reading and shows the same wall, its depth is the wall plane met by the ray through ITS centre (no interpolation): with the
    plane n . X = h through the moved point (n = the wall's axis in camera 1's frame), depth_1 = h / (n . K^-1 (c + 0.5, r + 0.5, 1))."""
    from mvp import corr3d

    H, W = 60, 84
    ds = corr3d.SyntheticScanNetPairs(num_pairs=6, image_height=H, image_width=W, seed=11)
    assert len(ds) == 6 and ds.name == "synthetic_scannet"
    angles, shares = [], []
    for i in range(len(ds)):
        it = ds[i]
        assert set(it) == {"uid", "class_id", "sequence_id", "frame_0", "frame_1", "K", "rgb_0", "rgb_1", "depth_0", "depth_1", "Rt_0", "Rt_1"}
        assert it["uid"] == i and isinstance(it["frame_0"], int) and isinstance(it["sequence_id"], str)
        assert it["rgb_0"].shape == it["rgb_1"].shape == (3, H, W) and it["depth_0"].shape == it["depth_1"].shape == (1, H, W)
        assert it["K"].shape == (3, 3) and it["Rt_0"].shape == it["Rt_1"].shape == (4, 4) and torch.equal(it["Rt_0"], torch.eye(4))
        assert all(it[k].dtype == torch.float32 for k in ("K", "rgb_0", "depth_0", "Rt_1"))
        again = ds[i]
        assert all(torch.equal(it[k], again[k]) if torch.is_tensor(it[k]) else it[k] == again[k] for k in it)
        K = it["K"].double()
        assert K[0, 0] != K[1, 1] and abs(K[0, 2] - W / 2) > 1 and abs(K[1, 2] - H / 2) > 1 and H != W
        geo = ds.geometry(i)
        for v in (0, 1):
            d = it[f"depth_{v}"][0]
            full = geo[f"xyz_{v}"][..., 2]
            hole = d == 0
            assert hole.float().mean() < 0.6 and (d >= 0).all() and d.max() <= ds.max_range
            assert hole[full > ds.max_range].all()                                   # the range limit ...
            assert int((hole & (full <= ds.max_range)).sum()) >= int(0.08 * H) * int(0.08 * W)  # ... and the rectangles (each at least that large)
            np.testing.assert_allclose(d[~hole].numpy(), full[~hole].numpy(), rtol=1e-6)
            assert it[f"rgb_{v}"].abs().max() <= 1 and it[f"rgb_{v}"].std() > 0.05
        d0, d1 = it["depth_0"][0].double(), it["depth_1"][0].double()
        p0 = ref.grid_to_pointcloud(K.inverse(), d0[None])
        keep0 = p0[:, 2] > 0
        p1 = ref3.transform(p0, it["Rt_1"])
        uv = ref3.project(p1, K)
        pix = uv.floor().long()
        inside = keep0 & (p1[:, 2] > 0) & (pix[:, 0] >= 0) & (pix[:, 0] < W) & (pix[:, 1] >= 0) & (pix[:, 1] < H)
        px, py = pix[:, 0].clamp(0, W - 1), pix[:, 1].clamp(0, H - 1)
        same = inside & (d1[py, px] > 0) & (geo["wall_1"][py, px] == geo["wall_0"].reshape(-1))
        axis = geo["wall_0"].reshape(-1) // 2
        n = geo["R_1"].t()[axis]                       # the wall's room axis in camera 1's frame: column `axis` of R_1
        h = (n * p1).sum(1)
        centre = torch.stack((px + 0.5, py + 0.5, torch.ones_like(px)), dim=1).double() @ K.inverse().t()
        want = h / (n * centre).sum(1)
        rel = ((d1[py, px] - want).abs() / want.abs())[same]
        assert rel.max() <= 1e-4, float(rel.max())
        shares.append(float(same.double().mean()))
        angles.append(float(ref3.rotation_angle(it["Rt_1"][None, :3, :3]) * 180 / math.pi))
        R = it["Rt_1"][:3, :3].double()
        np.testing.assert_allclose((R @ R.t()).numpy(), np.eye(3), atol=1e-6)
        assert it["Rt_1"][:3, 3].norm() > 0.02
    print("share of view-0 pixels checked against depth_1, per pair:", [f"{s:.2f}" for s in shares])
    assert sum(shares) / len(shares) > 0.20
    assert [int(a // 30) for a in angles] == [0, 1, 2, 0, 1, 2], angles
    other = corr3d.SyntheticScanNetPairs(num_pairs=6, image_height=H, image_width=W, seed=12)[0]
    assert not torch.equal(other["rgb_0"], ds[0]["rgb_0"])


def test_scannet_config_composes():
    from mvp import config, corr3d

    cfg = config.compose("scannet_correspondence", ["num_instances=3", "image_height=64"])
    assert cfg["random_seed"] == 8 and cfg["scale_factor"] == 0.25 and cfg["num_corr"] == 1000 and cfg["multilayer"] is False
    assert cfg["model_name"] == "dino_b16" and cfg["image_height"] == 64 and cfg["image_width"] == 640 and cfg["num_instances"] == 3
    assert "output_dir" in cfg and cfg["backbone"]["_target_"].endswith("DINO")
    ds = config.instantiate(cfg["dataset"], num_pairs=3, image_height=64, image_width=80, seed=8)
    assert isinstance(ds, corr3d.SyntheticScanNetPairs) and len(ds) == 3 and ds.name == "synthetic_scannet"
    assert len(corr3d.SCANNET_CSV_HEADER) == 27 and len(corr3d.SCANNET_RESULT_NAMES) == 19
