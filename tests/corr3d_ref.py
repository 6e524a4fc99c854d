"""Plain-torch fp64 definition of the NAVI 3-D correspondence path (test infrastructure; CPU).  Written from the formulas:

    x^ = x / max(|x|, 1e-12)                       D[i, j] = 1 - <q^_i, t^_j>
    nearest / second nearest of query i = the two smallest D[i, j] over the valid targets j, ties to the lowest j
    weight = 1 - max(d1, 1e-9) / max(d2, 1e-9)     top-k = the k largest weights
    transform X -> X R^T + t,  projection (K X)_xy / max((K X)_z, 1e-9),  angle = acos(clamp((tr R - 1) / 2, -1, 1))

The goldens of tests/golden/corr3d.npz (recorded from the reference's own functions) pin this definition in
tests/test_corr3d_cpu.py; the GPU tests then compare the kernels with it."""
import math

import torch


def normalize(x, dtype=torch.float64):
    x = x.to(dtype)
    return x / x.norm(dim=-1, keepdim=True).clamp(min=1e-12)


def distance_matrix(q, t, dtype=torch.float64):
    """q [N0, C], t [N1, C] (un-normalised) -> D [N0, N1] in ``dtype`` (fp64: the definition; fp32: the reference arithmetic)."""
    return 1 - normalize(q, dtype) @ normalize(t, dtype).t()


def two_nearest(D, valid_t=None):
    """D [N0, N1] -> (idx [N0, 2], d [N0, 2]) of the two smallest distances per row over the valid targets, ties to the lowest index.
    (A stable ascending sort keeps equal values in index order.)"""
    D = D.clone()
    if valid_t is not None:
        D[:, ~valid_t.bool()] = math.inf
    d, idx = torch.sort(D, dim=1, stable=True)
    return idx[:, :2], d[:, :2]


def ratio_weight(d):
    d = d.clamp(min=1e-9)
    return 1 - d[..., 0] / d[..., 1].clamp(min=1e-9)


def knn_ratio(q, t, valid_q=None, valid_t=None):
    """-> (nn_idx [N0] int64, dist [N0, 2], weight [N0], n_valid (2,)) with the ABI's conventions for invalid rows."""
    N0, N1 = q.shape[0], t.shape[0]
    vq = torch.ones(N0, dtype=torch.bool) if valid_q is None else valid_q.bool()
    vt = torch.ones(N1, dtype=torch.bool) if valid_t is None else valid_t.bool()
    idx, d = two_nearest(distance_matrix(q, t), vt)
    w = ratio_weight(d)
    dead = ~vq if int(vt.sum()) >= 2 else torch.ones(N0, dtype=torch.bool)
    nn = idx[:, 0].clone()
    nn[dead] = -1
    d = d.clone()
    d[dead] = math.inf
    w = w.clone()
    w[dead] = -math.inf
    return nn, d, w, (int(vq.sum()), int(vt.sum()))


def topk_matches(weights, idx, k):
    k = min(k, weights.shape[-1])
    w, src = torch.topk(weights, k=k, dim=-1)
    return src, idx[src], w


def get_grid(H, W):
    xs = (torch.arange(W, dtype=torch.float64) + 0.5).view(1, W).expand(H, W)
    ys = (torch.arange(H, dtype=torch.float64) + 0.5).view(H, 1).expand(H, W)
    return torch.stack((xs, ys, torch.ones(H, W, dtype=torch.float64)), dim=0)


def project(xyz, K):
    uvd = xyz.double() @ K.double().t()
    return uvd[:, :2] / uvd[:, 2:3].clamp(min=1e-9)


def transform(points, Rt, inverse=False):
    R, t = Rt[:3, :3].double(), Rt[:3, 3].double()
    return (points.double() - t) @ R if inverse else points.double() @ R.t() + t


def rotation_angle(R):
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    return torch.acos(((tr.double() - 1) / 2).clamp(-1, 1))


def binned_mean(y, x, bins):
    out = []
    for lo, hi in zip(bins[:-1], bins[1:]):
        m = (x >= lo) & (x < hi)
        out.append(y[m].double().mean() if m.any() else torch.tensor(math.nan, dtype=torch.float64))
    return torch.stack(out)


def bicubic_up(feat, h, w):
    """torch's own bicubic (align_corners=False, A = -0.75) in fp64: what the reference's nn_F.interpolate computes."""
    return torch.nn.functional.interpolate(feat[None].double(), size=(h, w), mode="bicubic")[0]


def estimate_correspondence_xyz(feat_0, feat_1, xyz_0, xyz_1, num_corr, ratio_test=True):
    """Grid-index form of the reference function: returns dict(idx0, idx1, weight (sorted descending), all_weight [h*w], nn [h*w],
    D [h*w, h*w], valid_0, valid_1); selections have length min(num_corr, valid cells of view 0)."""
    _, h, w = xyz_0.shape
    f0 = bicubic_up(feat_0, h, w).reshape(feat_0.shape[0], -1).t()
    f1 = bicubic_up(feat_1, h, w).reshape(feat_1.shape[0], -1).t()
    v0, v1 = (xyz_0[2] > 0).reshape(-1), (xyz_1[2] > 0).reshape(-1)
    nn, d, wgt, _ = knn_ratio(f0, f1, v0, v1)
    if not ratio_test:
        wgt = torch.where(nn >= 0, d[:, 0], wgt)
    k = min(num_corr, int(v0.sum()))
    sel_w, sel = torch.topk(wgt, k=k)
    return {"idx0": sel, "idx1": nn[sel], "weight": sel_w, "all_weight": wgt, "nn": nn, "dist": d, "D": distance_matrix(f0, f1),
            "valid_0": v0, "valid_1": v1, "f0": f0, "f1": f1}


def recalls(err_3d, err_2d, R_gt):
    """The ten numbers from per-pair fp64 error vectors."""
    a3, a2 = torch.cat(err_3d), torch.cat(err_2d)
    out = [100.0 * (a3 < th).double().mean().item() for th in (0.01, 0.02, 0.05)]
    out += [100.0 * (a2 < th).double().mean().item() for th in (5, 25, 50)]
    ang = rotation_angle(R_gt) * 180.0 / math.pi
    rec = torch.stack([(e < 0.02).double().mean() for e in err_3d])
    return out + [100.0 * float(v) for v in binned_mean(rec, ang, [0, 30, 60, 90, 120])]
