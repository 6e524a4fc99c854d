"""Records tests/golden/corr_depth.npz from the reference's own grid_to_pointcloud, sample_pointcloud_features,
estimate_correspondence_depth and error_auc on seeded inputs:

    python tests/golden/make_goldens_corr_depth.py <path to a checkout of the reference>

faiss is stood in for as in make_goldens_corr3d.py (a placeholder module for the import, ``faiss_knn`` replaced by the exact
brute-force search it is defined to return).  Everything else is the reference's code, unmodified, read only while this script runs.
SEED was picked so that the fp64 top-40 of the end-to-end case is decided by more than the fp32 weight bound at every rank
(tests/test_corr_depth_cpu.py asserts it)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_goldens_corr3d import _import_reference  # noqa: E402

SEED = 20240628


def inputs(seed=SEED):
    """The seeded inputs (also used to search the seed): C = 16, feats 6 x 8, depth 12 x 16 (k = 2) with about 25 % holes."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    K = torch.tensor([[11.5, 0.0, 8.6], [0.0, 12.25, 5.4], [0.0, 0.0, 1.0]])  # fx != fy, off-centre principal point, for 12 x 16
    out["K"] = K
    f0, f1 = torch.randn(16, 6, 8, generator=g), torch.randn(16, 6, 8, generator=g)
    d0, d1 = torch.rand(1, 12, 16, generator=g) * 2 + 0.5, torch.rand(1, 12, 16, generator=g) * 2 + 0.5
    d0[0][torch.rand(12, 16, generator=g) < 0.25] = 0.0
    d1[0][torch.rand(12, 16, generator=g) < 0.25] = 0.0
    out["e2e_feat_0"], out["e2e_feat_1"], out["e2e_depth_0"], out["e2e_depth_1"] = f0, f1, d0, d1
    # the sampling case: points whose projections fall inside, on the border band and outside the 12 x 16 image, z = 0 and z < 0
    pc = torch.randn(60, 3, generator=g)
    pc[:, 2] = pc[:, 2].abs() + 0.4
    pc[:20, :2] *= 0.3     # mostly inside
    uv_edge = torch.tensor([[0.2, 0.3], [15.9, 11.8], [0.4, 6.0], [8.0, 11.7], [-0.5, 3.0], [16.4, 5.0], [3.0, -0.6], [-3.0, 4.0], [7.0, 14.0]])
    z = torch.rand(len(uv_edge), generator=g) + 0.5
    pc[20:20 + len(uv_edge)] = (torch.cat((uv_edge, torch.ones(len(uv_edge), 1)), dim=1) * z[:, None]) @ K.inverse().t()
    pc[40:43, 2] = 0.0
    pc[43:46, 2] = -0.7
    out["samp_pc"], out["samp_feat"] = pc, torch.randn(16, 6, 8, generator=g)
    out["auc_errors"] = torch.rand(50, generator=g) * 0.3
    out["auc_thresholds"] = torch.tensor([0.05, 0.1, 0.2])
    return out


def main():
    rc, _ = _import_reference(os.path.abspath(sys.argv[1]))
    out = inputs()
    K = out["K"]
    out["g2p_points"] = rc.grid_to_pointcloud(K.inverse(), out["e2e_depth_0"])
    out["samp_out"] = rc.sample_pointcloud_features(out["samp_feat"], K.clone(), out["samp_pc"].clone(), (12, 16))
    for name, n in (("a", 40), ("b", 1000)):
        res = rc.estimate_correspondence_depth(out["e2e_feat_0"], out["e2e_feat_1"], out["e2e_depth_0"], out["e2e_depth_1"], K.clone(), num_corr=n)
        for key, v in zip(("xyz0", "xyz1", "dist"), res):
            out[f"e2e_{name}_{key}"] = v
    out["auc_out"] = torch.tensor(rc.error_auc(out["auc_errors"].tolist(), out["auc_thresholds"].tolist()), dtype=torch.float64)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "corr_depth.npz")
    np.savez_compressed(path, **{k: v.detach().cpu().numpy() for k, v in out.items()})
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
