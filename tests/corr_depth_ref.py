"""Plain-torch definition of the ScanNet pairs' depth path (test infrastructure; CPU), fp64 unless a dtype is given.  Written from
the formulas, with explicit corner arithmetic (no grid_sample):

    back-projection   P[r * W + c] = K^-1 (depth[r, c] * (c + 0.5, r + 0.5, 1))
    projection        uvd = K p,  u = uvd.x / max(uvd.z, 1e-9),  v = uvd.y / max(uvd.z, 1e-9)
    sampling          x = u * fw / W - 0.5,  y = v * fh / H - 0.5;  S[n, c] = sum over the corners (floor / floor + 1 of x and y) of
                      w_corner * feat[c, yc, xc];  a corner outside the map contributes 0;  a point whose x or y is not finite or
                      lies outside (-1, fw) x (-1, fh) gives exactly 0
    matching          tests/corr3d_ref.py (cosine distance, two nearest over the valid targets, ratio weight, top-k) on whole grids
                      with valid = z > 0, indices = GRID indices

The goldens of tests/golden/corr_depth.npz (recorded from the reference's own functions) pin this definition in
tests/test_corr_depth_cpu.py; the GPU tests then compare the kernel and the package with it."""
import math

import torch

import corr3d_ref as ref3

PX_THRESH = (1, 2, 5, 15, 25, 35, 50)
M_THRESH = (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5)


def grid_to_pointcloud(K_inv, depth, dtype=torch.float64):
    """depth [1, H, W] -> [H * W, 3]."""
    _, H, W = depth.shape
    grid = ref3.get_grid(H, W).to(dtype)
    return (K_inv.to(dtype) @ (depth.to(dtype) * grid).reshape(3, H * W)).t()


def sample_positions(K, pc, feat_hw, image_shape, dtype=torch.float64):
    """(x, y, ok): the sampling position of every point in feature-map texels and whether it yields anything at all."""
    (fh, fw), (H, W) = feat_hw, image_shape
    uvd = pc.to(dtype) @ K.to(dtype).t()
    z = uvd[:, 2].clamp(min=1e-9)
    x = uvd[:, 0] / z * fw / W - 0.5
    y = uvd[:, 1] / z * fh / H - 0.5
    ok = torch.isfinite(x) & torch.isfinite(y) & (x > -1) & (x < fw) & (y > -1) & (y < fh)
    return x, y, ok


def sample_pointcloud_features(feats, K, pc, image_shape, dtype=torch.float64):
    """feats [C, fh, fw], pc [N, 3] -> S [N, C] in ``dtype`` (fp64: the definition; fp32: the reference arithmetic)."""
    f = feats.to(dtype)
    C, fh, fw = f.shape
    x, y, ok = sample_positions(K, pc, (fh, fw), image_shape, dtype)
    x, y = torch.where(ok, x, torch.zeros_like(x)), torch.where(ok, y, torch.zeros_like(y))
    x0, y0 = x.floor(), y.floor()
    tx, ty = x - x0, y - y0
    out = torch.zeros(pc.shape[0], C, dtype=dtype)
    for dx, dy, w in ((0, 0, (1 - tx) * (1 - ty)), (1, 0, tx * (1 - ty)), (0, 1, (1 - tx) * ty), (1, 1, tx * ty)):
        xc, yc = x0 + dx, y0 + dy
        inb = ok & (xc >= 0) & (xc <= fw - 1) & (yc >= 0) & (yc <= fh - 1)
        vals = f[:, yc.clamp(0, fh - 1).long(), xc.clamp(0, fw - 1).long()].t()
        out += torch.where(inb[:, None], w[:, None] * vals, torch.zeros_like(vals))
    return out


def estimate_correspondence_depth(feat_0, feat_1, depth_0, depth_1, K, num_corr, dtype=torch.float64):
    """Grid-index form of the reference function.  K_inv is the fp32 host inverse the reference takes.  Returns dict(idx0, idx1, weight
    (sorted descending), all_weight [H*W], nn [H*W], dist [H*W, 2], D [H*W, H*W], valid_0, valid_1, xyz_0, xyz_1, f0, f1);
    selections have length min(num_corr, valid cells of view 0)."""
    K_inv = K.float().inverse()
    xyz_0, xyz_1 = grid_to_pointcloud(K_inv, depth_0, dtype), grid_to_pointcloud(K_inv, depth_1, dtype)
    v0, v1 = xyz_0[:, 2] > 0, xyz_1[:, 2] > 0
    f0 = sample_pointcloud_features(feat_0, K, xyz_0, depth_0.shape[-2:], dtype)
    f1 = sample_pointcloud_features(feat_1, K, xyz_1, depth_1.shape[-2:], dtype)
    if dtype != torch.float64:
        return {"D": ref3.distance_matrix(f0, f1, dtype), "f0": f0, "f1": f1}
    nn, d, wgt, _ = ref3.knn_ratio(f0, f1, v0, v1)
    k = min(num_corr, int(v0.sum()))
    sel_w, sel = torch.topk(wgt, k=k)
    return {"idx0": sel, "idx1": nn[sel], "weight": sel_w, "all_weight": wgt, "nn": nn, "dist": d, "D": ref3.distance_matrix(f0, f1),
            "valid_0": v0, "valid_1": v1, "xyz_0": xyz_0, "xyz_1": xyz_1, "f0": f0, "f1": f1}


def recalls(err_3d, err_2d, R_gt):
    """The 19 numbers from per-pair fp64 error vectors: 2-D recalls, 3-D recalls, the 2 cm recall per relative-angle bin."""
    a3, a2 = torch.cat(err_3d), torch.cat(err_2d)
    out = [100.0 * (a2 < th).double().mean().item() for th in PX_THRESH]
    out += [100.0 * (a3 < th).double().mean().item() for th in M_THRESH]
    ang = ref3.rotation_angle(R_gt) * 180.0 / math.pi
    rec = torch.stack([(e < 0.02).double().mean() for e in err_3d])
    return out + [100.0 * float(v) for v in ref3.binned_mean(rec, ang, [0, 30, 60, 90, 120])]
