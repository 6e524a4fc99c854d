"""Dense-CRF refinement of binary masks (reference: evals/models/crf.py::densecrf and the post-processing loop of
maskcut_processor.py:376-404), with the fully connected CRF's message passing evaluated exactly on the device (csrc/densecrf.hip).

The model is the one written out in include/mvp_hip.h ("Dense CRF").  With two labels one field per object is kept (Q_0 = 1 - Q_1):
per image the two kernels filter the ones field (-> the symmetric normalisers n) and n itself once, and per mean-field iteration
n * Q_1 of all objects as the fields of one pass, so the weight of a pixel pair is computed once for up to eight objects.  Nothing
here synchronises with the host.  pydensecrf evaluates the same two sums approximately on a permutohedral lattice; this is the exact
evaluation (MaskCut deviations)."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import lib, ops

MAX_ITER = 10                                    # crf.py
POS_W, POS_XY_STD = 7.0, 3.0
BI_W, BI_XY_STD, BI_RGB_STD = 10.0, 50.0, 5.0
MAX_FIELDS = 8                                   # fields of one filter pass (include/mvp_hip.h)
MAX_PASSES = 64                                  # masks per image of mvp_mask_finish
MAX_MASK_WORDS = 32768                           # H * ceil(W / 32): the bit-packed mask of mvp_mask_finish in LDS


class _Buffers:
    """Everything a refinement needs on the device, allocated once per (B, F, H, W)."""

    def __init__(self, B: int, F: int, H: int, W: int, dev):
        N = H * W
        f32, u8 = torch.float32, torch.uint8
        self.n_g, self.n_b = torch.empty(B, N, dtype=f32, device=dev), torch.empty(B, N, dtype=f32, device=dev)
        self.m_g, self.m_b = torch.empty(B, N, dtype=f32, device=dev), torch.empty(B, N, dtype=f32, device=dev)
        self.f_g, self.f_b, self.q, self.x_g, self.x_b = (torch.empty(B, F, N, dtype=f32, device=dev) for _ in range(5))
        self.map = torch.zeros(B, F, N, dtype=u8, device=dev)
        self.refined = torch.zeros(B, F, N, dtype=u8, device=dev)
        self.kept = torch.ones(B, F, dtype=u8, device=dev)
        self.union = torch.zeros(B, N, dtype=u8, device=dev)


_CACHE: Dict[Tuple, _Buffers] = {}


def _buffers(B: int, F: int, H: int, W: int, dev) -> _Buffers:
    key = (B, F, H, W, str(dev))
    if key not in _CACHE:
        _CACHE[key] = _Buffers(B, F, H, W, dev)
    return _CACHE[key]


def _need(t: torch.Tensor, dtype, ndim: int, name: str) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise lib.MvpError(f"densecrf: {name} must be a device tensor (no CPU fallback)")
    if t.dtype != dtype or t.dim() != ndim:
        raise ValueError(f"densecrf: {name} must be a {ndim}-d {dtype} tensor, got {t.dtype} {tuple(t.shape)}")


def mean_field(rgb_hwc: torch.Tensor, planes: torch.Tensor, active: Optional[torch.Tensor] = None, iters: int = MAX_ITER) -> _Buffers:
    """rgb_hwc [B, H, W, 3] uint8, planes [B, F, H, W] fp32 in [0, 1] (the foreground logit plane of crf.py: the mask, or its bilinear
    resize) -> the cached buffers with q [B, F, H W] = Q_1 after ``iters`` iterations and map = [Q_1 > Q_0].  ``active``: [B] bytes."""
    _need(rgb_hwc, torch.uint8, 4, "rgb")
    _need(planes, torch.float32, 4, "planes")
    B, F, H, W = planes.shape
    if tuple(rgb_hwc.shape) != (B, H, W, 3):
        raise ValueError(f"densecrf: rgb {tuple(rgb_hwc.shape)} against planes {tuple(planes.shape)}")
    if iters < 0 or F < 1:
        raise ValueError("densecrf: iters >= 0 and at least one field")
    rgb, planes = rgb_hwc.contiguous(), planes.contiguous()
    N = H * W
    buf = _buffers(B, F, H, W, planes.device)
    g_xy, b_xy, b_rgb = 1.0 / POS_XY_STD ** 2, 1.0 / BI_XY_STD ** 2, 1.0 / BI_RGB_STD ** 2
    ops.crf_filter(rgb, buf.n_g, B, 1, H, W, g_xy, 0.0, active=active)             # K_g 1
    ops.crf_filter(rgb, buf.n_b, B, 1, H, W, b_xy, b_rgb, active=active)           # K_b 1
    ops.crf_update("normalise", buf.n_g, buf.n_b, B, 1, N, active=active)
    ops.crf_filter(rgb, buf.m_g, B, 1, H, W, g_xy, 0.0, inp=buf.n_g, active=active)    # K_g n_g
    ops.crf_filter(rgb, buf.m_b, B, 1, H, W, b_xy, b_rgb, inp=buf.n_b, active=active)  # K_b n_b
    stride = F * N
    for f0 in range(0, F, MAX_FIELDS):
        fc = min(MAX_FIELDS, F - f0)
        q, x_g, x_b, f_g, f_b, mp = (t[:, f0:] for t in (buf.q, buf.x_g, buf.x_b, buf.f_g, buf.f_b, buf.map))
        common = dict(mask=planes[:, f0:], q=q, x_g=x_g, x_b=x_b, map_out=mp, stride=stride, active=active)
        ops.crf_update("init", buf.n_g, buf.n_b, B, fc, N, **common)
        for _ in range(iters):
            ops.crf_filter(rgb, f_g, B, fc, H, W, g_xy, 0.0, inp=x_g, in_stride=stride, out_stride=stride, active=active)
            ops.crf_filter(rgb, f_b, B, fc, H, W, b_xy, b_rgb, inp=x_b, in_stride=stride, out_stride=stride, active=active)
            ops.crf_update("step", buf.n_g, buf.n_b, B, fc, N, ones_g=buf.m_g, ones_b=buf.m_b, filt_g=f_g, filt_b=f_b, w_g=POS_W, w_b=BI_W,
                           **common)
    return buf


def _hwc(rgb_u8: torch.Tensor) -> torch.Tensor:
    _need(rgb_u8, torch.uint8, 4, "rgb_u8")
    if rgb_u8.shape[1] != 3:
        raise ValueError(f"densecrf: rgb_u8 must be [B, 3, H, W], got {tuple(rgb_u8.shape)}")
    return rgb_u8.permute(0, 2, 3, 1).contiguous()


def densecrf_batch(rgb_u8: torch.Tensor, masks: torch.Tensor, active: Optional[torch.Tensor] = None, iters: int = MAX_ITER):
    """rgb_u8 [B, 3, H, W] uint8, masks [B, F, H, W] uint8 (0 / 1; all F objects of an image share its filter passes)
    -> (Q_fg [B, F, H, W] fp32, map [B, F, H, W] uint8).  Images with a zero ``active`` byte keep whatever the buffers held."""
    _need(masks, torch.uint8, 4, "masks")
    B, F, H, W = masks.shape
    buf = mean_field(_hwc(rgb_u8), masks.float(), active, iters)
    return buf.q.view(B, F, H, W).clone(), buf.map.view(B, F, H, W).clone()


def refine_and_union(rgb_u8: torch.Tensor, masks: torch.Tensor, pass_active: Optional[torch.Tensor] = None, iters: int = MAX_ITER):
    """The reference's loop over an image's bipartitions (maskcut_processor.py:376-404) for a batch: dense CRF, hole filling, the IoU
    rule against the CRF's input, the union and its hole filling.  masks [B, P, H, W] uint8, pass_active optional [B, P] bytes (a pass an
    image does not have) -> (union [B, H, W] uint8, refined [B, P, H, W] uint8, kept [B, P] uint8), views of the cached buffers."""
    _need(masks, torch.uint8, 4, "masks")
    B, P, H, W = masks.shape
    if P > MAX_PASSES or H * ((W + 31) // 32) > MAX_MASK_WORDS:
        raise ValueError(f"densecrf: {P} passes of {H} x {W}; the finish step covers {MAX_PASSES} passes and H * ceil(W / 32) <= {MAX_MASK_WORDS}")
    masks = masks.contiguous()
    buf = mean_field(_hwc(rgb_u8), masks.float(), None, iters)
    if pass_active is not None:
        _need(pass_active, torch.uint8, 2, "pass_active")
        pass_active = pass_active.contiguous()
    ops.mask_finish(buf.map, masks, buf.refined, B, P, H, W, kept=buf.kept, union_mask=buf.union, active=pass_active)
    return buf.union.view(B, H, W), buf.refined.view(B, P, H, W), buf.kept
