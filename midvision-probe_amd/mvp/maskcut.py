"""Training-free object discovery with MaskCut (reference: evals/models/maskcut_processor.py, evaluate_generic_objectness.py):
normalised cuts on the thresholded patch affinity of a frozen backbone's last-layer keys, scored against the VOC masks.

The reference runs, per image and per object, a device-to-host copy of the affinity matrix, sklearn KMeans(2) on its N^2 entries, a
dense scipy eigh and ndimage.label.  Here a pass is four launches batched over the images of a batch (csrc/maskcut.hip): the affinity
on the fp32-input MFMA, a deterministic 2-means threshold that leaves a bit matrix, an eigen-solver that keeps that bit matrix in LDS,
and the partition / painting step.  ``max(num_objects)`` passes are issued back to back without a host sync, images with fewer
objects idle through an ``active`` byte; the union is upsampled to the mask and counted by mvp_binary_counts.  One transfer per batch
brings the [B, 4] counts and the ``converged`` bytes.  With ``refine="dense_crf"`` every pass's mask then goes through the reference's
post-processing at pixel level (mvp/densecrf.py: dense CRF, hole filling, IoU rule, union) before it is counted.  An image whose
solve did not converge on the device (near-degenerate lambda_2 ~ lambda_3) is done again with torch.linalg.eigh on S in fp64 on the host, re-entering at the partition launch; how many
did is reported (``n_fallback``).  Deviations from the reference: INTEGRATION.md."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch

from . import densecrf
from . import functional as MF
from . import lib, ops
from .objectness import METRICS, metrics_from_counts

MAX_N, MAX_C = 1024, 4096    # what the kernels cover (include/mvp_hip.h)
EPS = 1e-5                   # the reference's off-weight of the thresholded affinity
R_TOL = 2e-6                 # convergence: |S y - theta y| <= R_TOL (MaskCut: the fp32 floor of the iteration times a margin)
MIX_TOL = 1e-3               # ... and <= MIX_TOL * (theta_2 - theta_3): the admixture of the neighbouring eigenvector
MAX_ITERS = 1000
LLOYD_ROUNDS = 64
REFINE_MODES = ("none", "dense_crf")
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CSV_HEADER = ["Model Name", "Train Avg F-measure", "Train Avg IoU", "Train Avg Accuracy", "Train Avg CorLoc", "Test Avg F-measure",
              "Test Avg IoU", "Test Avg Accuracy", "Test Avg CorLoc", "n_fallback"]


def check_sizes(C: int, N: int) -> None:
    if not 0 < N <= MAX_N:
        raise ValueError(f"maskcut: {N} grid cells; the LDS-resident solver covers N <= {MAX_N} (480^2 at patch 16 is 900)")
    if not 0 < C <= MAX_C:
        raise ValueError(f"maskcut: {C} feature channels; the affinity kernel covers C <= {MAX_C}")


class _Buffers:
    """Everything a batch of passes needs on the device, allocated once per (B, N)."""

    def __init__(self, B: int, N: int, dev):
        NW = (N + 31) // 32
        f64, i32, u8 = torch.float64, torch.int32, torch.uint8
        self.B, self.N, self.NW = B, N, NW
        self.A = torch.empty(B, N, N, dtype=torch.float32, device=dev)
        self.sums = torch.empty(B, 2, dtype=f64, device=dev)
        self.ws = torch.empty(max(1, ops.ncut_workspace_bytes(B, N) // 8), dtype=f64, device=dev)
        self.tau = torch.empty(B, dtype=f64, device=dev)
        self.bits = torch.empty(B, N, NW, dtype=i32, device=dev)
        self.deg = torch.empty(B, N, dtype=f64, device=dev)
        self.rounds = torch.empty(B, dtype=i32, device=dev)
        self.v = torch.empty(B, N, dtype=torch.float32, device=dev)
        self.lam = torch.empty(B, dtype=f64, device=dev)
        self.res = torch.empty(B, dtype=f64, device=dev)
        self.iters = torch.empty(B, dtype=i32, device=dev)
        self.mask = torch.zeros(B, N, dtype=u8, device=dev)
        self.painted = torch.zeros(B, N, dtype=u8, device=dev)
        self.union = torch.zeros(B, N, dtype=u8, device=dev)
        self.seed = torch.empty(B, dtype=i32, device=dev)


def _need(t: torch.Tensor, dtype, shape, name: str) -> None:
    if not t.is_cuda:
        raise lib.MvpError(f"maskcut: {name} must be a device tensor (no CPU fallback)")
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"maskcut: {name} must be a contiguous {dtype} tensor of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")


def affinity(feats: torch.Tensor, buf: _Buffers, painted: Optional[torch.Tensor] = None, active: Optional[torch.Tensor] = None) -> None:
    B, C, N = feats.shape
    check_sizes(C, N)
    _need(feats, torch.float32, (buf.B, C, buf.N), "feats")
    ops.ncut_affinity(feats, buf.A, buf.sums, buf.ws, B, C, N, painted=painted, active=active)


def threshold(buf: _Buffers, active=None) -> None:
    ops.ncut_threshold(buf.A, buf.sums, buf.tau, buf.bits, buf.deg, buf.B, buf.N, LLOYD_ROUNDS, rounds=buf.rounds, active=active)


def fiedler(buf: _Buffers, converged: torch.Tensor, active=None, max_iters: int = MAX_ITERS, r_tol: float = R_TOL,
            mix_tol: float = MIX_TOL) -> None:
    _need(converged, torch.uint8, (buf.B,), "converged")
    ops.ncut_fiedler(buf.bits, buf.deg, buf.v, buf.lam, buf.res, buf.iters, converged, buf.B, buf.N, max_iters, r_tol, mix_tol, active=active)


def partition(buf: _Buffers, h: int, w: int, use_prev: bool, active=None) -> None:
    if h * w != buf.N:
        raise ValueError(f"maskcut: grid {h} x {w} against {buf.N} cells")
    ops.ncut_partition(buf.v, buf.mask, buf.painted, buf.union, buf.seed, buf.B, h, w, prev_mask=buf.mask, use_prev=use_prev, active=active)


def host_eigenvector(bits: torch.Tensor, deg: torch.Tensor, N: int) -> torch.Tensor:
    """The fallback solve of ONE image: torch.linalg.eigh on S = D^-1/2 W D^-1/2 in fp64 on the host -> v = D^-1/2 y_2 [N] fp32 with the
    sign convention (the entry of largest |v| positive, the lowest index on ties)."""
    b = bits.cpu().to(torch.int64) & 0xFFFFFFFF
    B = ((b.unsqueeze(-1) >> torch.arange(32)) & 1).reshape(N, -1)[:, :N].to(torch.float64)
    d = deg.cpu().double()
    s = d.rsqrt()
    S = (B + EPS * (1.0 - B)) * s[:, None] * s[None, :]
    _, U = torch.linalg.eigh(S)
    v = U[:, -2] * s
    k = int(torch.argmax(v.abs()))
    if v[k] < 0:
        v = -v
    return v.float()


def keep_crf_input(crf_inputs: torch.Tensor, p: int, buf: _Buffers, act: torch.Tensor) -> None:
    """The reference's ``bipartition_masked`` of pass p on the grid (maskcut_processor.py:278-286): the pass's mask minus the cells of the
    earlier passes' inputs, for the images with a set ``act`` byte -> crf_inputs[:, p] ([B, P, N] bytes); the other images keep theirs."""
    cur = buf.mask
    if p:
        cur = cur * (1 - crf_inputs[:, :p].amax(dim=1))
    a = act.view(-1, 1)
    crf_inputs[:, p] = cur * a + crf_inputs[:, p] * (1 - a)


def maskcut_batch(feats: torch.Tensor, h: int, w: int, num_objects: Sequence[int], *, max_iters: int = MAX_ITERS, r_tol: float = R_TOL,
                  mix_tol: float = MIX_TOL, buf: Optional[_Buffers] = None, keep_passes: bool = False,
                  crf_inputs: Optional[torch.Tensor] = None):
    """The pass loop of maskcut_forward for a batch.  feats [B, C, h*w] fp32 on the device (extract_kqv's layout), num_objects per
    image.  Issues max(num_objects) passes of the four launches without a host sync and returns
    (buf, converged [P, B] uint8 on the device, active [P, B] uint8 on the device[, per-pass copies]); buf.union holds the prediction on
    the grid (holes filled).  ``finish_fallbacks`` then repairs the images whose solve did not converge.  ``crf_inputs``: a zeroed
    [B, P, h*w] byte tensor that receives every pass's CRF input (``keep_crf_input``; refinement only)."""
    if feats.dim() != 3:
        raise ValueError(f"maskcut: feats must be [B, C, h*w], got {tuple(feats.shape)}")
    B, C, N = feats.shape
    check_sizes(C, N)
    if h * w != N:
        raise ValueError(f"maskcut: grid {h} x {w} against {N} feature columns")
    if len(num_objects) != B or min(int(k) for k in num_objects) < 1:
        raise ValueError("maskcut: one num_objects >= 1 per image")
    feats = feats.detach().contiguous().float()
    dev = feats.device
    buf = buf if (buf is not None and buf.B == B and buf.N == N) else _Buffers(B, N, dev)
    buf.painted.zero_()
    buf.mask.zero_()
    buf.union.zero_()
    P = max(int(k) for k in num_objects)
    act_host = torch.tensor([[1 if p < int(k) else 0 for k in num_objects] for p in range(P)], dtype=torch.uint8)
    active = act_host.to(dev, non_blocking=True)
    converged = torch.ones(P, B, dtype=torch.uint8, device=dev)
    kept: List[Dict[str, torch.Tensor]] = []
    for p in range(P):
        act = active[p]
        affinity(feats, buf, painted=buf.painted if p else None, active=act)
        threshold(buf, active=act)
        fiedler(buf, converged[p], active=act, max_iters=max_iters, r_tol=r_tol, mix_tol=mix_tol)
        partition(buf, h, w, use_prev=p >= 1, active=act)
        if crf_inputs is not None:
            keep_crf_input(crf_inputs, p, buf, act)
        if keep_passes:
            kept.append({k: getattr(buf, k).clone() for k in ("A", "sums", "tau", "bits", "deg", "rounds", "v", "lam", "res", "iters", "mask",
                                                              "painted", "union", "seed")})
    return (buf, converged, active, kept) if keep_passes else (buf, converged, active)


def finish_fallbacks(feats: torch.Tensor, h: int, w: int, num_objects: Sequence[int], buf: _Buffers, converged_host: torch.Tensor,
                     crf_inputs: Optional[torch.Tensor] = None) -> int:
    """Run again, pass by pass (with a host sync per pass) and with the host solve wherever the device does not converge, every image
    that has a clear ``converged`` byte in one of its passes; the other images idle and keep their results.  -> number of host solves."""
    B, N = buf.B, buf.N
    todo = [b for b in range(B) if any(int(converged_host[p, b]) == 0 for p in range(int(num_objects[b])))]
    if not todo:
        return 0
    dev = buf.v.device
    feats = feats.detach().contiguous().float()
    sel = torch.zeros(B, dtype=torch.uint8)
    sel[todo] = 1
    idx = torch.tensor(todo, device=dev)
    buf.painted[idx] = 0
    buf.mask[idx] = 0
    buf.union[idx] = 0
    if crf_inputs is not None:
        crf_inputs[idx] = 0
    n_fallback = 0
    conv = torch.ones(B, dtype=torch.uint8, device=dev)
    for p in range(max(int(num_objects[b]) for b in todo)):
        act_host = torch.tensor([1 if (sel[b] and p < int(num_objects[b])) else 0 for b in range(B)], dtype=torch.uint8)
        act = act_host.to(dev)
        affinity(feats, buf, painted=buf.painted if p else None, active=act)
        threshold(buf, active=act)
        conv.fill_(1)
        fiedler(buf, conv, active=act)
        conv_host = conv.cpu()
        for b in todo:
            if act_host[b] and not int(conv_host[b]):
                buf.v[b].copy_(host_eigenvector(buf.bits[b], buf.deg[b], N))
                n_fallback += 1
        partition(buf, h, w, use_prev=p >= 1, active=act)
        if crf_inputs is not None:
            keep_crf_input(crf_inputs, p, buf, act)
    return n_fallback


def upsampled_counts(union: torch.Tensor, h: int, w: int, gt: torch.Tensor) -> torch.Tensor:
    """[B, 4] int64 TP / FP / FN / TN on the device of the grid prediction, nearest-upsampled to the mask's size, against gt [B, 1, H, W]."""
    B = union.shape[0]
    H, W = gt.shape[-2:]
    with torch.no_grad():
        up = MF.interpolate(union.view(B, 1, h, w).float(), size=(H, W), mode="nearest")  # maskcut_processor.py:279-283
    g = gt.detach().reshape(B, H * W).contiguous().float()
    counts = torch.empty(B, 4, dtype=torch.int64, device=union.device)
    ops.binary_counts(up.reshape(B, H * W).contiguous(), g, counts, B, H * W, 0.5)
    return counts


def quantise_rgb(images: torch.Tensor, rgb: Optional[torch.Tensor]) -> torch.Tensor:
    """The uint8 image the CRF sees, [B, 3, H, W]: round(255 rgb) of ``rgb`` in [0, 1], or of ``images`` with the ImageNet normalisation undone."""
    if rgb is None:
        mean = torch.tensor(IMAGENET_MEAN, device=images.device, dtype=torch.float32).view(1, 3, 1, 1)
        std = torch.tensor(IMAGENET_STD, device=images.device, dtype=torch.float32).view(1, 3, 1, 1)
        rgb = images.float() * std + mean
    elif tuple(rgb.shape) != tuple(images.shape):
        raise ValueError(f"MaskCutProcessor: rgb {tuple(rgb.shape)} against images {tuple(images.shape)}")
    return torch.round(255.0 * rgb.float()).clamp_(0.0, 255.0).to(torch.uint8)


class MaskCutProcessor:
    """The reference's MaskCutProcessor on the HIP path.  It takes the dataset's tensors (``original_image``: already fixed_size^2 and
    normalised) instead of opening image files.  ``refine="dense_crf"`` runs the reference's post-processing of every pass (dense CRF with
    exact message passing, hole filling, IoU rule, union: mvp/densecrf.py) and scores at pixel level; ``refine="none"`` (the default)
    scores the patch grid.  The reference's ``crf`` flag is not how the refinement is selected: ``crf=True`` raises."""

    def __init__(self, backbone, feature_extractor_fn=None, patch_size: int = 16, tau: float = 0.15, fixed_size: int = 480, crf: bool = False,
                 refine: str = "none"):
        if crf:
            raise NotImplementedError("MaskCutProcessor(crf=True): the pydensecrf post-processing of the reference (host side, approximate) is "
                                      'not part of this port; pass refine="dense_crf" for the exact dense CRF on the device '
                                      "(INTEGRATION.md, MaskCut deviations)")
        if refine not in REFINE_MODES:
            raise ValueError(f"MaskCutProcessor: refine must be one of {REFINE_MODES}, got {refine!r}")
        self.refine = refine
        self.backbone = backbone
        self.feature_extractor_fn = feature_extractor_fn if feature_extractor_fn is not None else self.default_feature_extractor
        self.patch_size, self.fixed_size = int(patch_size), int(fixed_size)
        self.tau = tau  # kept for the signature: the reference overwrites it with the 2-means threshold (maskcut_processor.py:94)
        self.crf = False
        self._buf: Optional[_Buffers] = None
        check_sizes(1, (self.fixed_size // self.patch_size) ** 2)

    def default_feature_extractor(self, image_tensor: torch.Tensor) -> torch.Tensor:
        """[B, C, h*w] keys of the last attention layer (the backbone is configured with return_kqv=True)."""
        with torch.no_grad():
            return self.backbone(image_tensor)

    def maskcut_forward(self, feats: torch.Tensor, dims, num_pseudo_masks: Sequence[int]):
        """The pass loop for a batch -> (buffers, converged [P, B] uint8 on the device); buffers.union [B, h*w] is the prediction on the
        grid, holes filled.  feats [B, C, h*w], one num_pseudo_masks per image."""
        h, w = int(dims[0]), int(dims[1])
        self._buf, converged, _ = maskcut_batch(feats, h, w, num_pseudo_masks, buf=self._buf)
        return self._buf, converged

    def process_batch(self, images: torch.Tensor, gt: torch.Tensor, num_objects: Sequence[int], rgb: Optional[torch.Tensor] = None):
        """images [B, 3, S, S] on the device, gt [B, 1, H, W] 0 / 1 -> (per-image metric dicts, n_fallback).  ``rgb`` [B, 3, S, S] in [0, 1]:
        the image the dense CRF sees (refinement only; without it the ImageNet normalisation of ``images`` is undone)."""
        if images.shape[-1] % self.patch_size or images.shape[-2] % self.patch_size:
            raise ValueError("MaskCutProcessor: the image size must be a multiple of the patch size")
        if self.refine != "none":
            return self._process_batch_refined(images, gt, num_objects, rgb)
        h, w = images.shape[-2] // self.patch_size, images.shape[-1] // self.patch_size
        feats = self.feature_extractor_fn(images)
        if feats.dim() != 3 or feats.shape[-1] != h * w:
            raise ValueError(f"MaskCutProcessor: the backbone must return [B, C, {h * w}] key features (return_kqv=True), got {tuple(feats.shape)}")
        feats = feats.detach().contiguous().float()
        buf, converged = self.maskcut_forward(feats, (h, w), num_objects)
        counts = upsampled_counts(buf.union, h, w, gt)
        # the one transfer of the batch: the counts and the converged bytes in one buffer
        P, B = converged.shape
        host = torch.cat([counts.reshape(-1), converged.reshape(-1).to(torch.int64)]).cpu()
        conv_host = host[4 * B:].reshape(P, B)
        n_fallback = finish_fallbacks(feats, h, w, num_objects, buf, conv_host)
        if n_fallback:
            host = upsampled_counts(buf.union, h, w, gt).reshape(-1).cpu()
        rows = [metrics_from_counts(*host[4 * b:4 * b + 4].tolist()) for b in range(B)]
        return [{k: r[k] for k in METRICS} for r in rows], n_fallback

    def _features(self, images: torch.Tensor):
        h, w = images.shape[-2] // self.patch_size, images.shape[-1] // self.patch_size
        feats = self.feature_extractor_fn(images)
        if feats.dim() != 3 or feats.shape[-1] != h * w:
            raise ValueError(f"MaskCutProcessor: the backbone must return [B, C, {h * w}] key features (return_kqv=True), got {tuple(feats.shape)}")
        return feats.detach().contiguous().float(), h, w

    def refined_union(self, images: torch.Tensor, num_objects: Sequence[int], rgb: Optional[torch.Tensor] = None):
        """The pass loop, the fallbacks and the refinement -> (union [B, H, W] uint8 at pixel level, per-pass CRF inputs [B, P, H, W] uint8,
        active [B, P] uint8, n_fallback), all on the device; the first is a view of mvp.densecrf's buffers."""
        feats, h, w = self._features(images)
        B = feats.shape[0]
        H, W = images.shape[-2:]
        P = max(int(k) for k in num_objects)
        grid_inputs = torch.zeros(B, P, h * w, dtype=torch.uint8, device=feats.device)
        self._buf, converged, active = maskcut_batch(feats, h, w, num_objects, buf=self._buf, crf_inputs=grid_inputs)
        n_fallback = finish_fallbacks(feats, h, w, num_objects, self._buf, converged.cpu(), crf_inputs=grid_inputs)
        with torch.no_grad():
            up = MF.interpolate(grid_inputs.view(B, P, h, w).float(), size=(H, W), mode="nearest")  # maskcut_processor.py:279-283
        inputs = up.to(torch.uint8)
        pass_active = active.t().contiguous()
        union, _, _ = densecrf.refine_and_union(quantise_rgb(images, rgb), inputs, pass_active)
        return union, inputs, pass_active, n_fallback

    def _process_batch_refined(self, images, gt, num_objects, rgb):
        B = images.shape[0]
        H, W = images.shape[-2:]
        if tuple(gt.shape[-2:]) != (H, W):
            raise ValueError(f"MaskCutProcessor(refine={self.refine!r}): gt {tuple(gt.shape)} must have the image's size {H} x {W}")
        union, _, _, n_fallback = self.refined_union(images, num_objects, rgb)
        counts = torch.empty(B, 4, dtype=torch.int64, device=union.device)
        ops.binary_counts(union.reshape(B, H * W).float(), gt.detach().reshape(B, H * W).contiguous().float(), counts, B, H * W, 0.5)
        host = counts.reshape(-1).cpu()
        rows = [metrics_from_counts(*host[4 * b:4 * b + 4].tolist()) for b in range(B)]
        return [{k: r[k] for k in METRICS} for r in rows], n_fallback


def predict(processor: MaskCutProcessor, dataset, batch_size: int = 16, device=None):
    """evaluate_generic_objectness.py:180-279 without files, wandb or plots -> (average metrics, n_fallback, n_images)."""
    dev = device or torch.device("cuda", torch.cuda.current_device())
    avg = {k: 0.0 for k in METRICS}
    n, n_fallback = 0, 0
    for i0 in range(0, len(dataset), batch_size):
        items = [dataset[i] for i in range(i0, min(i0 + batch_size, len(dataset)))]
        images = torch.stack([it["original_image"] for it in items]).to(dev)
        gt = torch.stack([it["gt_binary_mask"] for it in items]).to(dev)
        rgb = None
        if processor.refine != "none" and "original_image_rgb" in items[0]:
            rgb = torch.stack([it["original_image_rgb"] for it in items]).to(dev)
        rows, nf = processor.process_batch(images, gt, [int(it["num_objects"]) for it in items], rgb)
        n_fallback += nf
        for r in rows:  # the reference's running average, image by image
            n += 1
            for k in avg:
                avg[k] = (avg[k] * (n - 1) + r[k]) / n
    if n == 0:
        raise ValueError("predict(): empty dataset")
    return avg, n_fallback, n
