"""NAVI / ScanNet 3-D correspondence hot path (evaluate_navi_correspondence.py:121-223, evals/utils/correspondence.py:26-131,
193-277, evals/utils/transformations.py).

``knn_ratio`` runs the fused HIP path (mvp_knn_ratio: L2-normalise, MFMA top-candidates, exact fp32 refine, ratio test) on whole
grids with validity masks; indices are GRID indices (the reference compacts with a boolean mask, which preserves order, so the
correspondences are the same and nothing has to be synchronised to size a compacted tensor).  The ScanNet pairs' depth path
(render_scannet_correspondence.py, correspondence.py:147-232) puts mvp_pointcloud_sample in front of it: each view's depth map is
back-projected, the dense features are sampled at the points' projections (zero-padded bilinear) straight into the channel-major
map the search reads.  Everything else in this module is few-line device-tensor plumbing with the reference's names, signatures
and return values."""
from __future__ import annotations

import numpy as np
import torch

from . import evalloop
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
def _select(weight, nn_idx, n_valid, num_corr):
    """The selection both match_* functions end in: (weights [k] sorted descending, idx0, idx1, count) of the k = min(num_corr, queries)
    heaviest queries (a STATIC length); count (0-d int64) = min(k, valid queries), 0 with fewer than two valid candidates."""
    k = min(int(num_corr), weight.shape[0])
    c_dist, idx0 = torch.topk(weight, k=k, dim=-1)
    idx1 = nn_idx.long()[idx0].clamp(min=0)  # padding entries point at cell 0 (never reported: count)
    nv = n_valid.long()
    count = torch.where(nv[1] >= 2, nv[0].clamp(max=k), torch.zeros_like(nv[0]))
    return c_dist, idx0, idx1, count


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
    c_dist, idx0, idx1, count = _select(weight, nn_idx, n_valid, num_corr)
    uvd = get_grid(h, w).to(xyz_grid_0).permute(1, 2, 0).reshape(h * w, 3)
    xyz_0 = xyz_grid_0.permute(1, 2, 0).reshape(h * w, 3)
    xyz_1 = xyz_grid_1.permute(1, 2, 0).reshape(h * w, 3)
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
    the device and the error vectors are fetched once at the end.  With world > 1 the BATCHES are sharded (evalloop.shard over batch
    indices: a wrapper whose train-mode tap BN couples the images of a forward then sees the same batches at any world size), the
    rows gathered once and sorted by pair index."""
    dev = torch.device("cuda", torch.cuda.current_device())
    n = len(dataset)
    batches = [list(range(s, min(s + batch_size, n))) for s in range(0, n, batch_size)]
    mine = evalloop.shard(len(batches), rank, world)

    def forwards():
        for b in mine:
            batch = {k: v.to(dev, non_blocking=True) for k, v in _collate([dataset[i] for i in batches[b]]).items()}
            yield {"image": batch["image_0"].float(), "meta": (b, 0, batch)}
            yield {"image": batch["image_1"].float(), "meta": (b, 1, batch)}

    pending, feat_0 = [], None
    for item, f in evalloop.features(model, forwards(), world):
        b, view, batch = item["meta"]
        if view == 0:
            feat_0 = f.clone()  # view 0 is kept across the next forward, which may reuse the buffer f is a view of
            continue
        xyz_0 = MF.interpolate(batch["xyz_grid_0"].float(), scale_factor=scale_factor, mode="nearest")
        xyz_1 = MF.interpolate(batch["xyz_grid_1"].float(), scale_factor=scale_factor, mode="nearest")
        Rt = batch["Rt_01"].float()[:, :3, :4]
        K = batch["intrinsics_1"].float()
        for j, i in enumerate(batches[b]):
            m = match_grids(feat_0[j], f[j], xyz_0[j], xyz_1[j], num_corr)
            pending.append((i, *_pair_errors(m, Rt[j], K[j]), m["count"], Rt[j, :3, :3]))
    outs = evalloop.in_index_order(evalloop.gather_parts(_fetch(pending), world))
    return summarize([o[1] for o in outs], [o[2] for o in outs], torch.stack([o[3] for o in outs]))


def _pair_errors(m, Rt, K):
    """(err3d, err2d), each [k], of a match dict: view 0's points moved into camera 1 by Rt [3, 4] against view 1's points, in metres
    and, projected by K, in pixels.  On the device, no sync; entries from m["count"] on are padding."""
    xyz0in1 = transform_points_Rt(m["xyz0"], Rt)
    err3d = (xyz0in1 - m["xyz1"]).norm(p=2, dim=1)
    err2d = (project_3dto2d(xyz0in1, K) - project_3dto2d(m["xyz1"], K)).norm(p=2, dim=1)
    return err3d, err2d


def _fetch(pending):
    """Rows (pair index, err3d, err2d, count, R_gt) of a finished loop -> host rows with the errors trimmed to ``count``: the loop's
    only host syncs, after its last forward has been issued.  (R_gt: a device slice for NAVI, already on the host for ScanNet.)"""
    return [(i, e3[:int(c)].cpu(), e2[:int(c)].cpu(), R.cpu()) for i, e3, e2, c, R in pending]


def _recalls(err, thresholds):
    """Recall in % at each threshold (means of 0 / 1 in fp64: the reference's fp32 mean rounds count / n in the 7th digit; it prints
    two decimals)."""
    return [100.0 * (err < th).double().mean().item() for th in thresholds]


def _angle_bin_recalls(err_3d, R_gt):
    """The pairs' 2 cm recall in %, averaged per 30-degree bin of the relative rotation angle up to 120 (an empty bin is nan)."""
    rel_ang = so3_rotation_angle(R_gt) * 180.0 / np.pi
    rec_2cm = torch.stack([(e < 0.02).double().mean() for e in err_3d])
    return [float(v) * 100.0 for v in compute_binned_performance(rec_2cm, rel_ang, [0, 30, 60, 90, 120])]


def summarize(err_3d, err_2d, R_gt):
    """evaluate_navi_correspondence.py:196-223 from per-pair error vectors (the reference stacks them, which needs equal lengths;
    here pairs with fewer than num_corr valid cells simply contribute fewer correspondences) and R_gt [n, 3, 3]: 3-D recalls, 2-D
    recalls, angle bins."""
    all3, all2 = torch.cat(err_3d).float(), torch.cat(err_2d).float()
    return _recalls(all3, (0.01, 0.02, 0.05)) + _recalls(all2, (5, 25, 50)) + _angle_bin_recalls(err_3d, R_gt)


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


# ----------------------------------------------------------------------------------------------- ScanNet pairs: the depth path
SCANNET_PX_THRESH = (1, 2, 5, 15, 25, 35, 50)
SCANNET_M_THRESH = (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5)
SCANNET_RESULT_NAMES = ([f"2D Recall ({t}px)" for t in SCANNET_PX_THRESH] + [f"3D Recall ({t}m)" for t in SCANNET_M_THRESH]
                        + ["Bin Rec 0-30°", "Bin Rec 30-60°", "Bin Rec 60-90°", "Bin Rec 90-120°"])
SCANNET_CSV_HEADER = ["Time", "Model Checkpoint", "Patch Size", "Layer", "Output", "Dataset", "Num Correspondences", "Scale Factor"] + SCANNET_RESULT_NAMES


def grid_to_pointcloud(K_inv, depth, grid=None):
    """correspondence.py:147-161: depth [1, H, W] -> [H * W, 3], the pixel centres back-projected by K_inv (row-major grid order; a
    depth hole, value 0, becomes the point 0)."""
    _, H, W = depth.shape
    if grid is None:
        grid = get_grid(H, W).to(depth)
    points = (depth * grid).reshape(3, H * W)
    return (K_inv.to(depth) @ points).permute(1, 0)


def _pointcloud_sample(feats, K, pc, image_shape, want_valid=False):
    """mvp_pointcloud_sample -> (out [C, N] fp32, valid uint8 [N] or None), on the device, no sync."""
    _need_cuda(feats, pc)
    H, W = (int(v) for v in image_shape)
    f = feats.detach().contiguous().float()
    p = pc.detach().contiguous().float()
    if f.dim() != 3 or p.dim() != 2 or p.shape[1] != 3:
        raise ValueError(f"expected feats [C, fh, fw] and pc [N, 3], got {tuple(f.shape)} and {tuple(p.shape)}")
    Kd = K.detach().to(device=f.device, dtype=torch.float32).contiguous()
    C, fh, fw = f.shape
    N = p.shape[0]
    out = torch.empty(C, N, dtype=torch.float32, device=f.device)
    valid = torch.empty(N, dtype=torch.uint8, device=f.device) if want_valid else None
    ops.pointcloud_sample(f, p, Kd, out, valid, C, fh, fw, N, H, W, N)
    return out, valid


def sample_pointcloud_features(feats, K, pc, image_shape):
    """correspondence.py:164-176: feats [C, fh, fw], pc [N, 3], image_shape (H, W) of the grid K projects into -> [N, C], the
    zero-padded bilinear samples at the points' projections (the .t() view of the kernel's channel-major [C, N] output).  The
    arguments are not modified (the reference normalises uv in place, on its own temporary)."""
    return _pointcloud_sample(feats, K, pc, image_shape)[0].t()


def match_depth(feat_0, feat_1, depth_0, depth_1, K, num_corr=500, K_inv=None):
    """The body of estimate_correspondence_depth (correspondence.py:218-232) on whole grids, without a host sync when K is a host
    tensor (its inverse is then taken on the host, as the reference does) or when K_inv is given.  Returns a dict of device tensors
    of the STATIC length k = min(num_corr, H * W): idx0 / idx1 (GRID indices, int64; the reference's compaction by z > 0 preserves
    order, so the correspondences are the same), xyz0 / xyz1 [k, 3], dist [k] (the weights, sorted descending) and count (0-d
    int64) = min(num_corr, valid cells of view 0); entries from ``count`` on are padding (weight -inf)."""
    _need_cuda(feat_0, feat_1, depth_0, depth_1)
    if K_inv is None:
        K_inv = K.detach().cpu().inverse()  # a device K costs one sync here
    xyz_0 = grid_to_pointcloud(K_inv, depth_0.float()).contiguous()
    xyz_1 = grid_to_pointcloud(K_inv, depth_1.float()).contiguous()
    f0, valid_0 = _pointcloud_sample(feat_0, K, xyz_0, depth_0.shape[-2:], want_valid=True)
    f1, valid_1 = _pointcloud_sample(feat_1, K, xyz_1, depth_1.shape[-2:], want_valid=True)
    nn_idx, dist, weight, n_valid = knn_ratio(f0, f1, valid_0, valid_1)
    c_dist, idx0, idx1, count = _select(weight, nn_idx, n_valid, num_corr)
    return {"idx0": idx0, "idx1": idx1, "xyz0": xyz_0[idx0], "xyz1": xyz_1[idx1], "dist": c_dist, "count": count}


def estimate_correspondence_depth(feat_0, feat_1, depth_0, depth_1, K, num_corr=500):
    """correspondence.py:218-232: feat_* [C, fh, fw], depth_* [1, H, W], K [3, 3] -> (corr_xyz0, corr_xyz1, corr_dist), each of
    length min(num_corr, points of view 0 with z > 0), ordered by descending weight.  One host sync, to trim."""
    m = match_depth(feat_0, feat_1, depth_0, depth_1, K, num_corr)
    n = int(m["count"])
    return m["xyz0"][:n], m["xyz1"][:n], m["dist"][:n]


def error_auc(errors, thresholds):
    """correspondence.py:199-215 (host numpy): area under the recall-over-error curve up to each threshold, over the threshold."""
    errors = [0] + sorted(list(errors))
    recall = list(np.linspace(0, 1, len(errors)))
    trapezoid = getattr(np, "trapezoid", None) or np.trapz
    aucs = []
    for thr in thresholds:
        last_index = np.searchsorted(errors, thr)
        y = recall[:last_index] + [recall[last_index - 1]]
        x = errors[:last_index] + [thr]
        aucs.append(trapezoid(y, x) / thr)
    return aucs


def evaluate_scannet(model, dataset, num_corr, scale_factor, multilayer, rank: int = 0, world: int = 1):
    """render_scannet_correspondence.py:188-274 over EVERY pair -> the 19 numbers of ``SCANNET_RESULT_NAMES`` (Python floats; recalls
    in %, an empty angle bin is nan).  One forward per pair on the stacked [rgb_0, rgb_1] (the reference's batch of 2: a wrapper
    whose tap BN runs in train mode sees both views together), kept in flight by mvp.pipeline; depths resized by ``scale_factor``
    (nearest), K[:2] scaled and inverted on the host; the matching stays on the device and the error vectors are fetched once at
    the end.  With world > 1 the pairs are sharded (evalloop.shard) and the rows gathered once."""
    dev = torch.device("cuda", torch.cuda.current_device())
    mine = evalloop.shard(len(dataset), rank, world)

    def forwards():
        for i in mine:
            it = dataset[i]
            rgbs = torch.stack((it["rgb_0"], it["rgb_1"]), dim=0).float().to(dev, non_blocking=True)
            yield {"image": rgbs, "meta": (i, it)}

    pending = []
    for item, f in evalloop.features(model, forwards(), world):
        f = f.clone()  # the copy this loop has always made, kept so that nothing changes (SPair's, which consumes f the same way, has none)
        i, it = item["meta"]
        deps = torch.stack((it["depth_0"], it["depth_1"]), dim=0).float().to(dev, non_blocking=True)
        deps = MF.interpolate(deps, scale_factor=scale_factor, mode="nearest")
        K_host = it["K"].clone().float()
        K_host[:2, :] *= scale_factor
        K_mat, K_inv = K_host.to(dev), K_host.inverse().to(dev)
        Rt = it["Rt_1"].float()[:3, :4].to(dev)
        m = match_depth(f[0], f[1], deps[0], deps[1], K_mat, num_corr, K_inv=K_inv)
        pending.append((i, *_pair_errors(m, Rt, K_mat), m["count"], it["Rt_1"].float()[:3, :3]))
    outs = evalloop.in_index_order(evalloop.gather_parts(_fetch(pending), world))
    return summarize_scannet([o[1] for o in outs], [o[2] for o in outs], torch.stack([o[3] for o in outs]))


def summarize_scannet(err_3d, err_2d, R_gt):
    """render_scannet_correspondence.py:248-274 from per-pair error vectors (concatenated, as ``summarize`` does: the reference stacks
    them, which needs equal lengths) and R_gt [n, 3, 3]: 2-D recalls, 3-D recalls, then the 2 cm recall per relative-angle bin."""
    all3, all2 = torch.cat(err_3d).float(), torch.cat(err_2d).float()
    return _recalls(all2, SCANNET_PX_THRESH) + _recalls(all3, SCANNET_M_THRESH) + _angle_bin_recalls(err_3d, R_gt)


# ----------------------------------------------------------------------------------------------- synthetic ScanNet-shaped pairs
class SyntheticScanNetPairs(torch.utils.data.Dataset):
    """ScanNet-pairs-shaped instances (the keys of the reference's ScanNetPairsDataset.__getitem__): uid, class_id, sequence_id,
    frame_0, frame_1, K [3, 3], rgb_0 / rgb_1 [3, H, W], depth_0 / depth_1 [1, H, W] (metres along the optical axis, 0 = no
    reading), Rt_0 (identity) and Rt_1 [4, 4] (camera 0 -> camera 1).  The scene is the inside of a textured axis-aligned box room
    (camera 0 stands in it with a yaw and a slight tilt); both cameras are ray-cast analytically at the pixel centres (slab test
    from the inside), so depth and pose are exact by construction.  fx != fy and the principal point is off-centre; the relative
    rotation is 15, 45 or 75 degrees (+- 10, cycling with the index) about a nearly vertical axis through a point in front of
    camera 0, so the translation grows with it and the views keep common walls.  Depth holes, as a ScanNet sensor gives them: two
    rectangles per view and everything beyond ``max_range``."""

    name = "synthetic_scannet"
    max_range = 2.6

    def __init__(self, num_pairs=8, image_height=480, image_width=640, seed=0):
        self.n, self.H, self.W, self.seed = int(num_pairs), int(image_height), int(image_width), int(seed)

    def __len__(self):
        return self.n

    def intrinsics(self):
        H, W = self.H, self.W
        return torch.tensor([[0.90 * W, 0, 0.5 * W + 0.031 * W], [0, 0.93 * W, 0.5 * H - 0.027 * H], [0, 0, 1]], dtype=torch.float64)

    @staticmethod
    def _rodrigues(axis, angle):
        axis = axis / axis.norm()
        Kx = torch.tensor([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]], dtype=torch.float64)
        return torch.eye(3, dtype=torch.float64) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)

    def _scene(self, i):
        """(generator, box lo / hi [3] in the room frame, room -> camera rotations R0 / R1, camera centres c0 / c1 in the room frame,
        R and t of camera 0 -> camera 1) of pair i (float64)."""
        g = torch.Generator().manual_seed(self.seed * 7919 + int(i))
        r = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64)  # noqa: E731
        lo = -torch.tensor([1.3, 1.0, 1.2], dtype=torch.float64) - 0.4 * r(3)
        hi = torch.tensor([1.5, 1.1, 1.9], dtype=torch.float64) + 0.4 * r(3)
        up = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
        R0 = self._rodrigues(up + 0.3 * (r(3) - 0.5), np.deg2rad(70.0 * (r(1).item() - 0.5)))  # camera 0: a yaw, slightly tilted
        c0 = (r(3) - 0.5) * torch.tensor([0.8, 0.3, 0.8], dtype=torch.float64)
        angle = np.deg2rad(15.0 + 30.0 * (int(i) % 3) + 20.0 * (r(1).item() - 0.5))
        R = self._rodrigues((up + 0.15 * (r(3) - 0.5)) * (1.0 if r(1).item() < 0.5 else -1.0), angle)
        R1 = R @ R0
        # camera 1 swings about a point 1.2 m in front of camera 0 (so that a large rotation still leaves common walls), kept inside the room
        pivot = c0 + 1.2 * R0[2]
        c1 = pivot - (0.9 + 0.3 * r(1).item()) * R1[2] + (r(3) - 0.5) * torch.tensor([0.2, 0.1, 0.2], dtype=torch.float64)
        c1 = torch.minimum(torch.maximum(c1, lo + 0.3), hi - 0.3)
        return g, lo, hi, R0, R1, c0, c1, R, R1 @ (c0 - c1)

    def _cast(self, R, centre, lo, hi):
        """Pixel-centre rays of a camera (room -> camera rotation R, centre in the room frame) against the box from the inside:
        camera-frame xyz [H, W, 3], room-frame hit points [H, W, 3] and the wall id (2 * axis + (1 if the high wall)) [H, W]."""
        H, W = self.H, self.W
        K = self.intrinsics()
        u = ((torch.arange(W, dtype=torch.float64) + 0.5 - K[0, 2]) / K[0, 0]).view(1, W).expand(H, W)
        v = ((torch.arange(H, dtype=torch.float64) + 0.5 - K[1, 2]) / K[1, 1]).view(H, 1).expand(H, W)
        d_cam = torch.stack((u, v, torch.ones(H, W, dtype=torch.float64)), dim=-1)
        d = d_cam @ R  # room frame: R^T d_cam
        plane = torch.where(d > 0, hi.expand_as(d), lo.expand_as(d))
        t_axis = torch.where(d != 0, (plane - centre) / torch.where(d != 0, d, torch.ones_like(d)), torch.full_like(d, float("inf")))
        t, axis = t_axis.min(dim=-1)
        wall = 2 * axis + (torch.gather(d, -1, axis[..., None])[..., 0] > 0).long()
        return d_cam * t[..., None], centre + d * t[..., None], wall

    def geometry(self, i):
        """The scene behind pair i, without holes (tests): box lo / hi, the room -> camera rotations R_v and centres centre_v, R and t
        of Rt_1, and per view v the camera-frame points xyz_v [H, W, 3], the room-frame hits room_v and the wall ids wall_v."""
        _, lo, hi, R0, R1, c0, c1, R, t = self._scene(i)
        x0, r0, w0 = self._cast(R0, c0, lo, hi)
        x1, r1, w1 = self._cast(R1, c1, lo, hi)
        return {"lo": lo, "hi": hi, "R": R, "t": t, "R_0": R0, "R_1": R1, "centre_0": c0, "centre_1": c1, "xyz_0": x0, "xyz_1": x1,
                "room_0": r0, "room_1": r1, "wall_0": w0, "wall_1": w1}

    def __getitem__(self, i):
        g = self._scene(i)[0]
        geo = self.geometry(i)
        H, W = self.H, self.W
        r = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64)  # noqa: E731
        # texture: a few random plane waves of the room-frame position, a different mix per wall
        freq = (r(6, 3) - 0.5) * 2 * 14.0
        phase = r(6, 3) * 2 * np.pi
        amp = r(6, 3) + 0.2
        wall_gain = 0.5 + r(6, 3)
        out = {"uid": int(i), "class_id": "ScanNet_synthetic", "sequence_id": f"room{self.seed:04d}_{int(i):02d}", "frame_0": 0, "frame_1": 1,
               "K": self.intrinsics().float()}
        for v in (0, 1):
            room, wall = geo[f"room_{v}"], geo[f"wall_{v}"]
            img = (amp[None, None] * torch.sin((room @ freq.t())[..., None] + phase[None, None])).sum(-2) * wall_gain[wall] / 3.0
            depth = geo[f"xyz_{v}"][..., 2].clone()
            depth[depth > self.max_range] = 0.0
            for _ in range(2):
                hh, ww = int(H * (0.08 + 0.12 * r(1).item())), int(W * (0.08 + 0.12 * r(1).item()))
                y0, x0 = int((H - hh) * r(1).item()), int((W - ww) * r(1).item())
                depth[y0:y0 + hh, x0:x0 + ww] = 0.0
            out[f"rgb_{v}"] = img.permute(2, 0, 1).float().clamp(-1, 1)
            out[f"depth_{v}"] = depth[None].float()
        Rt = torch.eye(4, dtype=torch.float64)
        Rt[:3, :3], Rt[:3, 3] = geo["R"], geo["t"]
        out["Rt_0"], out["Rt_1"] = torch.eye(4).float(), Rt.float()
        return out
