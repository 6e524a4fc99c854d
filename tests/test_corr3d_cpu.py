"""CPU checks of the NAVI 3-D correspondence path: the fp64 definition the GPU tests use (tests/corr3d_ref.py) reproduces goldens
recorded from the reference's own functions (tests/golden/make_goldens_corr3d.py), the device-free functions of mvp.corr3d do
too, SyntheticNAVI is geometrically exact and deterministic, and the new ABI entry validates its arguments before any launch."""
import ctypes
import math

import numpy as np
import pytest
import torch

import corr3d_ref as ref
from conftest import load_golden


@pytest.fixture(scope="module")
def G():
    return {k: torch.from_numpy(v) for k, v in load_golden("corr3d.npz").items()}


def test_fp64_definition_reproduces_the_reference_functions(G):
    np.testing.assert_allclose(ref.ratio_weight(G["ratio_in"].double()).numpy(), G["ratio_out"].numpy(), rtol=0, atol=2e-7)
    assert (G["ratio_out"][:4] == 0).all() and (G["ratio_out"][4:8] == 1 - 1e-9 / G["ratio_in"][4:8, 1].clamp(min=1e-9)).all()
    for k in (7, 200):
        s, t, v = ref.topk_matches(G["topk_w"].double(), G["topk_idx"], k)
        assert torch.equal(s, G[f"topk{k}_src"]) and torch.equal(t, G[f"topk{k}_tgt"]) and torch.equal(v.float(), G[f"topk{k}_val"])
        assert len(s) == min(k, 50)
    np.testing.assert_allclose(ref.get_grid(5, 7).numpy(), G["grid_5x7"].numpy(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(ref.project(G["proj_xyz"], G["proj_K"]).numpy(), G["proj_uv"].numpy(), rtol=2e-6, atol=1e-4)
    np.testing.assert_allclose(ref.transform(G["tf_pts"], G["tf_Rt"]).numpy(), G["tf_fwd"].numpy(), rtol=0, atol=2e-6)
    np.testing.assert_allclose(ref.transform(G["tf_pts"], G["tf_Rt"], inverse=True).numpy(), G["tf_inv"].numpy(), rtol=0, atol=2e-6)
    np.testing.assert_allclose(ref.transform(ref.transform(G["tf_pts"], G["tf_Rt"]), G["tf_Rt"], inverse=True).numpy(), G["tf_pts"].numpy(), atol=1e-6)
    # acos near 1 amplifies the fp32 rounding of the trace: sqrt(2 * 3 * 2^-24) ~ 6e-4 rad at the identity
    np.testing.assert_allclose(ref.rotation_angle(G["so3_R"]).numpy(), G["so3_angle"].numpy(), rtol=0, atol=1e-3)
    b, gb = ref.binned_mean(G["bin_y"], G["bin_x"], [0, 30, 60, 90, 120]), G["bin_out"]
    assert torch.isnan(gb[2]) and torch.isnan(b[2])
    np.testing.assert_allclose(b[[0, 1, 3]].numpy(), gb[[0, 1, 3]].numpy(), rtol=0, atol=1e-6)


@pytest.mark.parametrize("case,num_corr,ratio_test", [("a", 40, True), ("b", 1000, True), ("c", 40, False)])
def test_fp64_definition_reproduces_the_reference_end_to_end(G, case, num_corr, ratio_test):
    """estimate_correspondence_xyz of the reference (faiss replaced by its definition while recording) against the grid-index form:
    the same cells in the same order, the reference's fp32 weights within fp32 rounding of the fp64 ones."""
    x0, x1 = G["e2e_xyz_0"], G["e2e_xyz_1"]
    r = ref.estimate_correspondence_xyz(G["e2e_feat_0"], G["e2e_feat_1"], x0, x1, num_corr, ratio_test)
    n = min(num_corr, int((x0[2] > 0).sum()))
    assert len(r["idx0"]) == n == len(G[f"e2e_{case}_dist"])
    flat0, flat1 = x0.permute(1, 2, 0).reshape(-1, 3), x1.permute(1, 2, 0).reshape(-1, 3)
    uv = ref.get_grid(12, 12).permute(1, 2, 0).reshape(-1, 3)[:, :2].float()
    assert torch.equal(flat0[r["idx0"]], G[f"e2e_{case}_xyz0"]) and torch.equal(flat1[r["idx1"]], G[f"e2e_{case}_xyz1"])
    assert torch.equal(uv[r["idx0"]], G[f"e2e_{case}_uv0"]) and torch.equal(uv[r["idx1"]], G[f"e2e_{case}_uv1"])
    np.testing.assert_allclose(r["weight"].numpy(), G[f"e2e_{case}_dist"].numpy(), rtol=0, atol=5e-6)
    assert (r["valid_0"][r["idx0"]]).all() and (r["valid_1"][r["idx1"]]).all()


def test_device_free_functions_of_the_package_match_the_goldens(G):
    from evals.utils import correspondence as C
    from evals.utils import transformations as T
    from mvp import corr3d, lib

    assert torch.equal(C.calculate_ratio_test(G["ratio_in"]), G["ratio_out"])
    s, t, v = C.get_topk_matches(G["topk_w"], G["topk_idx"], 7)
    assert torch.equal(s, G["topk7_src"]) and torch.equal(t, G["topk7_tgt"]) and torch.equal(v, G["topk7_val"])
    assert torch.equal(C.get_grid(5, 7), G["grid_5x7"])
    assert torch.equal(C.project_3dto2d(G["proj_xyz"], G["proj_K"]), G["proj_uv"])
    assert torch.equal(T.transform_points_Rt(G["tf_pts"], G["tf_Rt"]), G["tf_fwd"])
    assert torch.equal(T.transform_points_Rt(G["tf_pts"], G["tf_Rt"], inverse=True), G["tf_inv"])
    assert torch.equal(T.so3_rotation_angle(G["so3_R"]), G["so3_angle"])
    np.testing.assert_allclose(T.so3_relative_angle(G["so3_R"], G["so3_R"]).numpy(), 0.0, atol=1e-3)
    out = torch.stack(C.compute_binned_performance(G["bin_y"], G["bin_x"], [0, 30, 60, 90, 120]))
    assert torch.equal(out[[0, 1, 3]], G["bin_out"][[0, 1, 3]]) and torch.isnan(out[2])
    with pytest.raises(ValueError):
        T.so3_rotation_angle(torch.eye(3)[None] * 2.0)   # trace 6
    with pytest.raises(ValueError):
        T.so3_rotation_angle(torch.zeros(1, 3, 4))
    # the hot path has no CPU fallback
    f = torch.randn(8, 5)
    with pytest.raises(lib.MvpError):
        corr3d.knn_ratio(f, f)
    with pytest.raises(lib.MvpError):
        C.get_correspondences_ratio_test(f.t(), f.t(), 3)
    with pytest.raises(lib.MvpError):
        C.estimate_correspondence_xyz(torch.randn(8, 2, 2), torch.randn(8, 2, 2), torch.rand(3, 4, 4), torch.rand(3, 4, 4))
    with pytest.raises(NotImplementedError):
        C.get_correspondences_ratio_test(f.t(), f.t(), 3, metric="euclidean")


def test_synthetic_navi_is_exact_and_deterministic():
    """A view-0 surface point moved by Rt_01 lies where view 1 saw the surface: it projects (intrinsics_1) into some pixel, and that
    pixel's own xyz_1 — the hit of the ray through the pixel CENTRE — is the same surface seen at most half a pixel diagonal away:
    |difference| <= z * (sqrt(2) / 2) / f / cos(slant).  Checked where the surface faces camera 1 with cos(slant) >= 0.3, with the
    bound 4 z / f (2.4 z / f from the formula, the rest for the curvature over that footprint)."""
    from mvp import corr3d

    ds = corr3d.SyntheticNAVI(num_pairs=5, image_size=96, seed=11)
    assert len(ds) == 5
    angles = []
    for i in range(len(ds)):
        it = ds[i]
        assert set(it) >= {"image_0", "image_1", "xyz_grid_0", "xyz_grid_1", "Rt_01", "intrinsics_1"}
        S = 96
        assert it["image_0"].shape == it["image_1"].shape == it["xyz_grid_0"].shape == it["xyz_grid_1"].shape == (3, S, S)
        assert it["Rt_01"].shape == (4, 4) and it["intrinsics_1"].shape == (3, 3)
        again = ds[i]
        assert all(torch.equal(it[k], again[k]) for k in it)  # deterministic per (seed, index)
        for v in (0, 1):
            xyz, img = it[f"xyz_grid_{v}"], it[f"image_{v}"]
            m = xyz[2] > 0
            assert 0.05 < m.float().mean() < 0.9
            assert (xyz[:, ~m] == 0).all() and (img[:, ~m] == 0).all() and img[:, m].abs().max() > 0.1
            # every hit is the pixel-centre ray scaled by its depth: the grid back-projects to itself
            uv = ref.project(xyz.permute(1, 2, 0)[m], it["intrinsics_1"])
            np.testing.assert_allclose(uv.numpy(), ref.get_grid(S, S).permute(1, 2, 0)[m][:, :2].numpy(), atol=2e-3)
        geo = ds.geometry(i)
        m0 = it["xyz_grid_0"][2] > 0
        p1 = ref.transform(it["xyz_grid_0"].permute(1, 2, 0)[m0], it["Rt_01"])
        np.testing.assert_allclose((p1 - geo["centre_1"]).norm(dim=1).numpy(), geo["radius"], atol=1e-6)  # still on the sphere
        normal = (p1 - geo["centre_1"]) / geo["radius"]
        cos = -(normal * p1).sum(1) / p1.norm(dim=1)
        pix = ref.project(p1, it["intrinsics_1"]).floor().long()
        keep = (cos >= 0.3) & (pix >= 0).all(1) & (pix < S).all(1)
        assert keep.sum() > 100
        x1 = it["xyz_grid_1"][:, pix[keep, 1], pix[keep, 0]].t().double()
        assert (x1[:, 2] > 0).all()  # visible there
        assert ((x1 - p1[keep]).norm(dim=1) <= 4 * p1[keep, 2] / geo["focal"]).all()
        angles.append(float(ref.rotation_angle(it["Rt_01"][None, :3, :3]) * 180 / math.pi))
        R = it["Rt_01"][:3, :3].double()
        np.testing.assert_allclose((R @ R.t()).numpy(), np.eye(3), atol=1e-6)
    assert len({int(a // 30) for a in angles}) >= 2 and max(angles) < 120, angles
    other = corr3d.SyntheticNAVI(num_pairs=5, image_size=96, seed=12)[0]
    assert not torch.equal(other["image_0"], ds[0]["image_0"])


def _ws_bytes(C, N0, N1):
    """include/mvp_hip.h: fp32 rows + fp16 pair of both views (C padded to 32), then 4 candidates of 8 bytes per query and target slice."""
    Cpad = -(-C // 32) * 32
    qt, tt = -(-N0 // 128), -(-N1 // 128)
    want = max(1, min(tt, -(-512 // qt)))
    tps = -(-tt // want)
    return (N0 + N1) * Cpad * 8 + (-(-tt // tps)) * N0 * 32


def test_knn_abi_struct_workspace_and_einval():
    from mvp import lib

    so = lib.load()
    assert so.mvp_sizeof(b"mvp_knn_ratio_args") == ctypes.sizeof(lib.KnnRatioArgs) == 96
    assert lib.STRUCTS["mvp_knn_ratio_args"] is lib.KnnRatioArgs and lib.SYMBOLS["mvp_knn_ratio"] is lib.KnnRatioArgs
    assert lib.info().abi_version == 8
    assert so.mvp_knn_workspace_bytes(64, 300, 333) == _ws_bytes(64, 300, 333) == 352896
    assert so.mvp_knn_workspace_bytes(768, 16384, 16384) == _ws_bytes(768, 16384, 16384) == 203423744
    assert so.mvp_knn_workspace_bytes(40, 1, 2) == _ws_bytes(40, 1, 2) == 3 * 64 * 8 + 32
    for bad in ((0, 4, 4), (64, 0, 4), (64, 4, 1), (16385, 4, 4), (-1, 4, 4), (64, -3, 4)):
        assert so.mvp_knn_workspace_bytes(*bad) == 0

    need = so.mvp_knn_workspace_bytes(64, 8, 8)
    ok = dict(src_feat=256, tgt_feat=256, nn_idx=256, dist=256, weight=256, n_valid=256, workspace=256, workspace_bytes=need, C=64, N0=8, N1=8)

    def rc(**kw):
        return so.mvp_knn_ratio(ctypes.byref(lib.KnnRatioArgs(**{**ok, **kw})), None)

    assert so.mvp_knn_ratio(None, None) == -1
    for field in ("src_feat", "tgt_feat", "nn_idx", "dist", "weight", "n_valid", "workspace"):
        assert rc(**{field: None}) == -1, field
    assert rc(C=0) == -1 and rc(C=-4) == -1 and rc(C=16385) == -1
    assert rc(N0=0) == -1 and rc(N0=-1) == -1 and rc(N1=1) == -1 and rc(N1=0) == -1
    assert rc(workspace_bytes=need - 1) == -1 and rc(workspace_bytes=0) == -1
    assert rc(workspace=264) == -1 and rc(workspace=260) == -1  # not 16-byte aligned
    assert rc(N0=16, workspace_bytes=need) == -1                # the workspace of a smaller problem
