"""Records tests/golden/corr3d.npz from the reference's own pure functions on seeded inputs:

    python tests/golden/make_goldens_corr3d.py <path to a checkout of the reference>

evals/utils/correspondence.py imports faiss at module level (not installable here): a placeholder module satisfies the import and
``faiss_knn`` is replaced, while recording, by what it is defined to return — an exact brute-force squared-L2 search (fp64, ties to
the lowest index).  Everything else is the reference's code, unmodified, read only while this script runs."""
import os
import sys
import types

import numpy as np
import torch


def _import_reference(root):
    fake = types.ModuleType("faiss")
    fake.StandardGpuResources = lambda: None
    contrib = types.ModuleType("faiss.contrib")
    tu = types.ModuleType("faiss.contrib.torch_utils")
    fake.contrib, contrib.torch_utils = contrib, tu
    sys.modules.update({"faiss": fake, "faiss.contrib": contrib, "faiss.contrib.torch_utils": tu})
    sys.path.insert(0, root)
    import evals.utils.correspondence as rc
    import evals.utils.transformations as rt

    def exact_knn(query, target, k):
        d = torch.cdist(query.double(), target.double()) ** 2
        dist, index = torch.sort(d, dim=1, stable=True)
        return dist[:, :k].float(), index[:, :k]

    rc.faiss_knn = exact_knn
    return rc, rt


def main():
    rc, rt = _import_reference(os.path.abspath(sys.argv[1]))
    g = torch.Generator().manual_seed(20240611)
    out = {}

    d = torch.rand(64, 2, generator=g).sort(dim=1).values
    d[:4] = 0.0            # both clamps
    d[4:8, 0] = 0.0        # the first clamp only
    d[8:10] = 1e-10
    out["ratio_in"], out["ratio_out"] = d, rc.calculate_ratio_test(d)

    w = torch.randn(50, generator=g)
    idx = torch.randperm(80, generator=g)[:50]
    for k in (7, 200):
        s, t, v = rc.get_topk_matches(w, idx, k)
        out[f"topk{k}_src"], out[f"topk{k}_tgt"], out[f"topk{k}_val"] = s, t, v
    out["topk_w"], out["topk_idx"] = w, idx

    out["grid_5x7"] = rc.get_grid(5, 7)

    xyz = torch.randn(40, 3, generator=g)
    xyz[:, 2] = xyz[:, 2].abs() + 0.3
    xyz[:3, 2] = 0.0       # the clamp of the divisor
    xyz[3, 2] = -0.5
    K = torch.tensor([[300.0, 0.0, 128.0], [0.0, 310.0, 120.0], [0.0, 0.0, 1.0]])
    out["proj_xyz"], out["proj_K"], out["proj_uv"] = xyz, K, rc.project_3dto2d(xyz, K)

    A = torch.randn(6, 3, 3, generator=g, dtype=torch.float64)
    R = torch.linalg.qr(A).Q
    R = R * torch.linalg.det(R).sign()[:, None, None]
    R = torch.cat([R, torch.eye(3, dtype=torch.float64)[None]]).float()
    Rt = torch.eye(4)
    Rt[:3, :3], Rt[:3, 3] = R[0], torch.tensor([0.1, -0.2, 0.3])
    pts = torch.randn(30, 3, generator=g)
    out["tf_Rt"], out["tf_pts"] = Rt, pts
    out["tf_fwd"], out["tf_inv"] = rt.transform_points_Rt(pts, Rt), rt.transform_points_Rt(pts, Rt, inverse=True)
    out["so3_R"], out["so3_angle"] = R, rt.so3_rotation_angle(R)

    y = torch.rand(12, generator=g)
    x = torch.tensor([5.0, 10, 29.9, 30, 45, 59, 95, 100, 119, 120, 0, 31])  # nothing in [60, 90)
    out["bin_y"], out["bin_x"] = y, x
    out["bin_out"] = torch.stack(rc.compute_binned_performance(y, x, [0, 30, 60, 90, 120]))

    C, fh, h = 16, 5, 12
    f0, f1 = torch.randn(C, fh, fh, generator=g), torch.randn(C, fh, fh, generator=g)
    x0, x1 = torch.rand(3, h, h, generator=g) + 0.2, torch.rand(3, h, h, generator=g) + 0.2
    x0[2][torch.rand(h, h, generator=g) < 0.25] = 0.0
    x1[2][torch.rand(h, h, generator=g) < 0.25] = 0.0
    out["e2e_feat_0"], out["e2e_feat_1"], out["e2e_xyz_0"], out["e2e_xyz_1"] = f0, f1, x0, x1
    for name, n, rtest in (("a", 40, True), ("b", 1000, True), ("c", 40, False)):
        res = rc.estimate_correspondence_xyz(f0, f1, x0, x1, num_corr=n, ratio_test=rtest)
        for key, v in zip(("xyz0", "xyz1", "dist", "uv0", "uv1"), res):
            out[f"e2e_{name}_{key}"] = v

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "corr3d.npz")
    np.savez_compressed(path, **{k: v.detach().cpu().numpy() for k, v in out.items()})
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
