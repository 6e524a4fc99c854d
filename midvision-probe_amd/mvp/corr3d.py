"""NAVI / ScanNet 3-D correspondence hot path (evaluate_navi_correspondence.py:121-223, evals/utils/correspondence.py:26-131,
193-277, evals/utils/transformations.py).

``knn_ratio`` runs the fused HIP path (mvp_knn_ratio: L2-normalise, MFMA top-candidates, exact fp32 refine, ratio test) on whole
grids with validity masks; indices are GRID indices (the reference compacts with a boolean mask, which preserves order, so the
correspondences are the same and nothing has to be synchronised to size a compacted tensor).  Everything else in this module is
few-line device-tensor plumbing with the reference's names, signatures and return values."""
from __future__ import annotations

import numpy as np
import torch

from . import functional as MF
from . import lib, ops

RESULT_NAMES = ["3D Recall (0.01m)", "3D Recall (0.02m)", "3D Recall (0.05m)", "2D Recall (5px)", "2D Recall (25px)", "2D Recall (50px)",
                "Bin Rec 0-30°", "Bin Rec 30-60°", "Bin Rec 60-90°", "Bin Rec 90-120°"]
CSV_HEADER = ["Time", "Model Checkpoint", "Patch Size", "Layer", "Output", "Num Correspondences", "Scale Factor", "Dataset"] + RESULT_NAMES


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise lib.MvpError("mvp.corr3d needs device tensors (no CPU fallback)")


# ----------------------------------------------------------------------------------------------- kernel wrapper
def knn_ratio(feat_0: torch.Tensor, feat_1: torch.Tensor, valid_0: torch.Tensor = None, valid_1: torch.Tensor = None):
    """feat_0 [C, ...] / feat_1 [C, ...]: fp32 device maps, channel-major, un-normalised (trailing dimensions are flattened to N0 / N1);
    valid_* optional masks over those positions.  Returns, on the device and without a sync,
    (nn_idx int32 [N0], dist fp32 [N0, 2], weight fp32 [N0], n_valid int32 [2]) as include/mvp_hip.h defines them."""
    _need_cuda(feat_0, feat_1, valid_0, valid_1)
    f0 = feat_0.detach().reshape(feat_0.shape[0], -1).contiguous().float()
    f1 = feat_1.detach().reshape(feat_1.shape[0], -1).contiguous().float()
    if f0.shape[0] != f1.shape[0]:
        raise ValueError(f"feature widths differ: {f0.shape[0]} vs {f1.shape[0]}")
    C, N0 = f0.shape
    N1 = f1.shape[1]
    v0 = None if valid_0 is None else valid_0.reshape(-1).ne(0).to(torch.uint8).contiguous()
    v1 = None if valid_1 is None else valid_1.reshape(-1).ne(0).to(torch.uint8).contiguous()
    if (v0 is not None and v0.numel() != N0) or (v1 is not None and v1.numel() != N1):
        raise ValueError("a valid mask does not match its feature map")
    dev = f0.device
    nn_idx = torch.empty(N0, dtype=torch.int32, device=dev)
    dist = torch.empty(N0, 2, dtype=torch.float32, device=dev)
    weight = torch.empty(N0, dtype=torch.float32, device=dev)
    n_valid = torch.empty(2, dtype=torch.int32, device=dev)
    nbytes = int(lib.load().mvp_knn_workspace_bytes(C, N0, N1))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    ops.knn_ratio(f0, f1, v0, v1, nn_idx, dist, weight, n_valid, ws, C, N0, N1)
    return nn_idx, dist, weight, n_valid


# ----------------------------------------------------------------------------------------------- reference-named functions
def calculate_ratio_test(dists: torch.Tensor) -> torch.Tensor:
    """correspondence.py:106-121: dists [..., 2] -> 1 - max(d1, 1e-9) / max(d2, 1e-9)."""
    dists = dists.clamp(min=1e-9)
    return 1 - dists[..., 0] / dists[..., 1].clamp(min=1e-9)


def get_topk_matches(dists, idx, num_corres: int):
    """correspondence.py:125-129."""
    num_corres = min(num_corres, dists.shape[-1])
    dist, idx_source = torch.topk(dists, k=num_corres, dim=-1)
    return idx_source, idx[idx_source], dist


def get_correspondences_ratio_test(P1_F, P2_F, num_corres, metric="cosine", bidirectional=False, ratio_test=True):
    """correspondence.py:63-102 on point features P1_F [N1, F], P2_F [N2, F] (every point valid): (idx into P1, idx into P2, weight).
    ``ratio_test=False`` weights by the nearest distance itself, so the top-k keeps the LARGEST distances (a quirk of the reference,
    kept).  ``bidirectional``: num_corres // 2 in each direction, concatenated."""
    if metric != "cosine":
        raise NotImplementedError("metric='euclidean' has no caller in the reference and is not built")
    _need_cuda(P1_F, P2_F)

    def one_way(a, b, k):
        nn_idx, dist, weight, _ = knn_ratio(a.t(), b.t())
        w = weight if ratio_test else dist[:, 0]
        return get_topk_matches(w, nn_idx.long(), k)

    if not bidirectional:
        return one_way(P1_F, P2_F, num_corres)
    m12_idx1, m12_idx2, m12_dist = one_way(P1_F, P2_F, num_corres // 2)
    m21_idx2, m21_idx1, m21_dist = one_way(P2_F, P1_F, num_corres // 2)
    return torch.cat((m12_idx1, m21_idx1), dim=-1), torch.cat((m12_idx2, m21_idx2), dim=-1), torch.cat((m12_dist, m21_dist), dim=-1)


def get_grid(H: int, W: int) -> torch.Tensor:
    """correspondence.py:132-144: [3, H, W] = (x, y, 1) of the pixel centres."""
    xs = torch.linspace(0.5, W - 0.5, W).view(1, W).repeat(H, 1)
    ys = torch.linspace(0.5, H - 0.5, H).view(H, 1).repeat(1, W)
    return torch.stack((xs, ys, torch.ones_like(xs)), dim=0)


def project_3dto2d(xyz, K_mat):
    """correspondence.py:193-196."""
    uvd = xyz @ K_mat.transpose(-1, -2)
    return uvd[:, :2] / uvd[:, 2:3].clamp(min=1e-9)


def compute_binned_performance(y, x, x_bins):
    """correspondence.py:266-277: mean of y over each [x_bins[i], x_bins[i + 1]); an empty bin is nan."""
    out = []
    for i in range(len(x_bins) - 1):
        mask = (x >= x_bins[i]) * (x < x_bins[i + 1])
        out.append(y[mask].mean())
    return out


def transform_points_Rt(points: torch.Tensor, viewpoint: torch.Tensor, inverse: bool = False):
    """transformations.py:27-36; points [..., n, 3]."""
    R = viewpoint[..., :3, :3]
    t = viewpoint[..., None, :3, 3]
    if inverse:
        return (points - t) @ R
    return points @ R.transpose(-2, -1) + t


def so3_rotation_angle(R: torch.Tensor, eps: float = 1e-4) -> torch.Tensor:
    """transformations.py:47-63."""
    _, dim1, dim2 = R.shape
    if dim1 != 3 or dim2 != 3:
        raise ValueError("Input has to be a batch of 3x3 Tensors.")
    rot_trace = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    if ((rot_trace < -1.0 - eps) + (rot_trace > 3.0 + eps)).any():
        raise ValueError("A matrix has trace outside valid range [-1-eps,3+eps].")
    return torch.acos(((rot_trace - 1.0) * 0.5).clamp(min=-1, max=1))


def so3_relative_angle(R1: torch.Tensor, R2: torch.Tensor, eps: float = 1e-4):
    """transformations.py:39-44."""
    return so3_rotation_angle(torch.bmm(R1, R2.permute(0, 2, 1)), eps=eps)


# ----------------------------------------------------------------------------------------------- one pair, on the device
def match_grids(feat_0, feat_1, xyz_grid_0, xyz_grid_1, num_corr=500, ratio_test=True):
    """The body of estimate_correspondence_xyz (correspondence.py:235-263) without a host sync.  Returns a dict of device tensors of
    the STATIC length k = min(num_corr, h * w): idx0 / idx1 (grid indices, int64), xyz0 / xyz1 [k, 3], dist [k] (the weights, sorted
    descending), uv0 / uv1 [k, 2], and count (0-d int64) = min(num_corr, valid cells of view 0) — entries from ``count`` on are
    padding (weight -inf).  With fewer than two valid cells in view 1 nothing can be matched and count is 0."""
    _need_cuda(feat_0, feat_1, xyz_grid_0, xyz_grid_1)
    _, h, w = xyz_grid_0.shape
    up0 = MF.interpolate(feat_0[None].float(), size=(h, w), mode="bicubic")[0]
    up1 = MF.interpolate(feat_1[None].float(), size=(h, w), mode="bicubic")[0]
    valid_0 = xyz_grid_0[2] > 0
    valid_1 = xyz_grid_1[2] > 0
    nn_idx, dist, weight, n_valid = knn_ratio(up0, up1, valid_0, valid_1)
    if not ratio_test:
        weight = torch.where(nn_idx >= 0, dist[:, 0], weight)  # invalid queries keep -inf
    k = min(int(num_corr), h * w)
    c_dist, idx0 = torch.topk(weight, k=k, dim=-1)
    idx1 = nn_idx.long()[idx0].clamp(min=0)  # padding entries point at cell 0 (never reported: count)
    uvd = get_grid(h, w).to(xyz_grid_0).permute(1, 2, 0).reshape(h * w, 3)
    xyz_0 = xyz_grid_0.permute(1, 2, 0).reshape(h * w, 3)
    xyz_1 = xyz_grid_1.permute(1, 2, 0).reshape(h * w, 3)
    nv = n_valid.long()
    count = torch.where(nv[1] >= 2, nv[0].clamp(max=k), torch.zeros_like(nv[0]))
    return {"idx0": idx0, "idx1": idx1, "xyz0": xyz_0[idx0], "xyz1": xyz_1[idx1], "dist": c_dist, "uv0": uvd[idx0][:, :2],
            "uv1": uvd.to(xyz_grid_1)[idx1][:, :2], "count": count}


def estimate_correspondence_xyz(feat_0, feat_1, xyz_grid_0, xyz_grid_1, num_corr=500, ratio_test=True):
    """correspondence.py:235-263: feat_* [C, fh, fw], xyz_grid_* [3, h, w] -> (c_xyz0, c_xyz1, c_dist, c_uv0, c_uv1), each of length
    min(num_corr, valid cells of view 0), ordered by descending weight.  One host sync, to trim."""
    m = match_grids(feat_0, feat_1, xyz_grid_0, xyz_grid_1, num_corr, ratio_test)
    n = int(m["count"])
    return m["xyz0"][:n], m["xyz1"][:n], m["dist"][:n], m["uv0"][:n], m["uv1"][:n]


# ----------------------------------------------------------------------------------------------- the dataset loop
def _collate(items):
    return {k: torch.stack([torch.as_tensor(it[k]) for it in items]) for k in ("image_0", "image_1", "xyz_grid_0", "xyz_grid_1", "Rt_01", "intrinsics_1")}


def evaluate_dataset(model, dataset, num_corr, scale_factor, multilayer, batch_size=4, rank: int = 0, world: int = 1):
    """evaluate_navi_correspondence.py:121-223 -> the ten numbers of ``RESULT_NAMES`` (Python floats; recalls in %, an empty angle bin
    is nan).  Loader batches of ``batch_size`` pairs in dataset order; per batch ``model(image_0)`` then ``model(image_1)``, two
    separate forwards kept in flight by mvp.pipeline (each equal, bit for bit, to the serial call); the per-pair matching stays on
    the device and the error vectors are fetched once at the end.  With world > 1 the BATCHES are sharded (mvp.spair.shard_pairs over
    batch indices: a wrapper whose train-mode tap BN couples the images of a forward then sees the same batches at any world size)
    and gathered with one all_gather_object."""
    from .pipeline import pipelined_features
    from .spair import shard_pairs

    dev = torch.device("cuda", torch.cuda.current_device())
    n = len(dataset)
    batches = [list(range(s, min(s + batch_size, n))) for s in range(0, n, batch_size)]
    mine = shard_pairs(len(batches), rank, world)

    def forwards():
        for b in mine:
            batch = {k: v.to(dev, non_blocking=True) for k, v in _collate([dataset[i] for i in batches[b]]).items()}
            yield {"image": batch["image_0"].float(), "meta": (b, 0, batch)}
            yield {"image": batch["image_1"].float(), "meta": (b, 1, batch)}

    import os

    graphs = True if (world > 1 and os.environ.get("MVP_PIPELINE_GRAPHS") is None) else None  # no collective in flight in this loop (mvp/spair.py)
    pending, feat_0 = [], None
    for item, feats in pipelined_features(model, forwards(), graphs=graphs):
        f = torch.cat(list(feats), dim=1) if isinstance(feats, (list, tuple)) else feats.clone()  # a copy: the slot's buffer is reused
        b, view, batch = item["meta"]
        if view == 0:
            feat_0 = f
            continue
        xyz_0 = MF.interpolate(batch["xyz_grid_0"].float(), scale_factor=scale_factor, mode="nearest")
        xyz_1 = MF.interpolate(batch["xyz_grid_1"].float(), scale_factor=scale_factor, mode="nearest")
        Rt = batch["Rt_01"].float()[:, :3, :4]
        K = batch["intrinsics_1"].float()
        for j, i in enumerate(batches[b]):
            m = match_grids(feat_0[j], f[j], xyz_0[j], xyz_1[j], num_corr)
            xyz0in1 = transform_points_Rt(m["xyz0"], Rt[j])
            err3d = (xyz0in1 - m["xyz1"]).norm(p=2, dim=1)
            err2d = (project_3dto2d(xyz0in1, K[j]) - project_3dto2d(m["xyz1"], K[j])).norm(p=2, dim=1)
            pending.append((i, err3d, err2d, m["count"], Rt[j, :3, :3]))
    outs = [(i, e3[:int(c)].cpu(), e2[:int(c)].cpu(), R.cpu()) for i, e3, e2, c, R in pending]  # the loop's only syncs
    if world > 1:
        import torch.distributed as dist

        gathered = [None] * world
        dist.all_gather_object(gathered, outs)
        outs = sorted((o for part in gathered for o in part), key=lambda o: o[0])  # dataset order, as the reference's single loop
    return summarize([o[1] for o in outs], [o[2] for o in outs], torch.stack([o[3] for o in outs]))


def summarize(err_3d, err_2d, R_gt):
    """evaluate_navi_correspondence.py:196-223 from per-pair error vectors (the reference stacks them, which needs equal lengths;
    here pairs with fewer than num_corr valid cells simply contribute fewer correspondences) and R_gt [n, 3, 3]."""
    all3, all2 = torch.cat(err_3d).float(), torch.cat(err_2d).float()
    # (means of 0 / 1 in fp64: the reference's fp32 mean rounds count / n in the 7th digit; it prints two decimals)
    out = [100.0 * (all3 < th).double().mean().item() for th in (0.01, 0.02, 0.05)]
    out += [100.0 * (all2 < th).double().mean().item() for th in (5, 25, 50)]
    rel_ang = so3_rotation_angle(R_gt) * 180.0 / np.pi
    rec_2cm = torch.stack([(e < 0.02).double().mean() for e in err_3d])
    out += [float(v) * 100.0 for v in compute_binned_performance(rec_2cm, rel_ang, [0, 30, 60, 90, 120])]
    return out


# ----------------------------------------------------------------------------------------------- synthetic NAVI-shaped pairs
class SyntheticNAVI(torch.utils.data.Dataset):
    """NAVI-shaped pair instances (the keys evaluate_navi_correspondence.py:143-166 reads): image_0 / image_1 [3, S, S],
    xyz_grid_0 / xyz_grid_1 [3, S, S] (camera-frame point per pixel, z = 0 outside the object), Rt_01 [4, 4] (camera 0 -> camera 1),
    intrinsics_1 [3, 3].  The object is one textured sphere (random radius, position and texture per pair) seen from two cameras
    whose relative rotation is 15, 45 or 75 degrees (+- 10) about a random axis: both views are ray-cast analytically at the pixel
    centres, so xyz, masks and the pose are exact by construction, and a convex object has no self-occlusion beyond facing away."""

    name = "synthetic_navi"

    def __init__(self, num_pairs=8, image_size=512, seed=0, patch=16):
        self.n, self.S, self.seed, self.patch = int(num_pairs), int(image_size), int(seed), int(patch)

    def __len__(self):
        return self.n

    @staticmethod
    def _cast(S, f, centre, radius):
        """Pixel-centre rays against the sphere: xyz [S, S, 3] float64 (0 where missed) and the hit mask."""
        c = (torch.arange(S, dtype=torch.float64) + 0.5 - S / 2) / f
        d = torch.stack((c.view(1, S).expand(S, S), c.view(S, 1).expand(S, S), torch.ones(S, S, dtype=torch.float64)), dim=-1)
        a = (d * d).sum(-1)
        b = (d * centre).sum(-1)
        disc = b * b - a * ((centre * centre).sum() - radius * radius)
        hit = disc > 0
        t = (b - disc.clamp(min=0).sqrt()) / a  # the near intersection
        return torch.where(hit[..., None], d * t[..., None], torch.zeros_like(d)), hit

    def _scene(self, i):
        """(generator, focal length, radius, sphere centre in camera 0 / camera 1, R, t) of pair i."""
        g = torch.Generator().manual_seed(self.seed * 7919 + int(i))
        f = 1.2 * self.S
        r = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64)  # noqa: E731
        radius = 0.10 + 0.04 * r(1).item()
        c0 = torch.tensor([0.02 * (r(1).item() - 0.5), 0.02 * (r(1).item() - 0.5), 0.50 + 0.05 * r(1).item()], dtype=torch.float64)
        c1 = torch.tensor([0.02 * (r(1).item() - 0.5), 0.02 * (r(1).item() - 0.5), 0.50 + 0.05 * r(1).item()], dtype=torch.float64)
        angle = np.deg2rad(15.0 + 30.0 * (int(i) % 3) + 20.0 * (r(1).item() - 0.5))
        axis = torch.randn(3, generator=g, dtype=torch.float64)
        axis = axis / axis.norm()
        Kx = torch.tensor([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]], dtype=torch.float64)
        R = torch.eye(3, dtype=torch.float64) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)  # Rodrigues
        return g, f, radius, c0, c1, R, c1 - R @ c0

    def geometry(self, i):
        """The scene behind pair i (tests): focal length in pixels, sphere radius and centre in each camera's frame (float64)."""
        _, f, radius, c0, c1, _, _ = self._scene(i)
        return {"focal": f, "radius": radius, "centre_0": c0, "centre_1": c1}

    def __getitem__(self, i):
        g, f, radius, c0, c1, R, t = self._scene(i)
        S = self.S
        r = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64)  # noqa: E731
        Rt = torch.eye(4, dtype=torch.float64)
        Rt[:3, :3], Rt[:3, 3] = R, t
        xyz_0, hit_0 = self._cast(S, f, c0, radius)
        xyz_1, hit_1 = self._cast(S, f, c1, radius)
        # texture: a few random plane waves of the object-frame position (camera-0 axes, origin at the sphere's centre)
        freq = (r(6, 3) - 0.5) * 2 * 60.0
        phase = r(6, 3) * 2 * np.pi
        amp = r(6, 3) + 0.2

        def texture(obj, hit):
            img = (amp[None, None] * torch.sin((obj @ freq.t())[..., None] + phase[None, None])).sum(-2)  # [S, S, 6 waves, 3] -> [S, S, 3]
            return torch.where(hit[..., None], img, torch.zeros_like(img)).permute(2, 0, 1).float()

        obj_0 = xyz_0 - c0
        obj_1 = (xyz_1 - t) @ R - c0  # camera 1 -> camera 0 (transform_points_Rt(inverse=True)), then to the object frame
        K = torch.tensor([[f, 0, S / 2], [0, f, S / 2], [0, 0, 1]], dtype=torch.float32)
        return {"image_0": texture(obj_0, hit_0), "image_1": texture(obj_1, hit_1),
                "xyz_grid_0": xyz_0.permute(2, 0, 1).float(), "xyz_grid_1": xyz_1.permute(2, 0, 1).float(),
                "Rt_01": Rt.float(), "intrinsics_1": K}
