"""The oracle of the dense-CRF refinement: the model of include/mvp_hip.h ("Dense CRF") by brute force, N x N kernel matrices in fp64
numpy (or in fp32, to measure what the number format alone costs), and the post-processing of the reference's process_image with
scipy.ndimage.binary_fill_holes and the IoU rule on integer counts.  Also the fixtures the CRF tests share."""
import functools

import numpy as np
from scipy import ndimage

MAX_ITER = 10
POS_W, POS_XY_STD = 7.0, 3.0
BI_W, BI_XY_STD, BI_RGB_STD = 10.0, 50.0, 5.0


def kernel_matrices(rgb, dtype=np.float64):
    """rgb [H, W, 3] uint8 -> (K_g, K_b) [N, N], both with the diagonal (j = i) included."""
    H, W = rgb.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]
    y, x = yy.reshape(-1).astype(dtype), xx.reshape(-1).astype(dtype)
    d2 = (y[:, None] - y[None, :]) ** 2 + (x[:, None] - x[None, :]) ** 2
    c = rgb.reshape(-1, 3).astype(dtype)
    c2 = np.zeros_like(d2)
    for k in range(3):
        c2 += (c[:, None, k] - c[None, :, k]) ** 2
    two = dtype(2.0)
    K_g = np.exp(-d2 / (two * dtype(POS_XY_STD) ** 2))
    K_b = np.exp(-d2 / (two * dtype(BI_XY_STD) ** 2) - c2 / (two * dtype(BI_RGB_STD) ** 2))
    return K_g.astype(dtype), K_b.astype(dtype)


def normaliser(K):
    return (K.sum(axis=1) + K.dtype.type(1e-20)) ** K.dtype.type(-0.5)


def softmax2(a):
    a = a - a.max(axis=1, keepdims=True)
    e = np.exp(a)
    return e / e.sum(axis=1, keepdims=True)


def mean_field(kernels, plane, iters=MAX_ITER):
    """kernels = (K_g, K_b), plane [H, W] = the foreground logit plane m in [0, 1] -> Q [N, 2] after ``iters`` iterations."""
    K_g, K_b = kernels
    dt = K_g.dtype.type
    m = plane.reshape(-1).astype(K_g.dtype)
    p = softmax2(np.stack([dt(1.0) - m, m], axis=1))
    U = -np.log(np.maximum(p, dt(1e-5)))
    n_g, n_b = normaliser(K_g), normaliser(K_b)
    Q = p.copy()
    for _ in range(iters):
        f_g = n_g[:, None] * (K_g @ (n_g[:, None] * Q))
        f_b = n_b[:, None] * (K_b @ (n_b[:, None] * Q))
        Q = softmax2(-U + dt(POS_W) * f_g + dt(BI_W) * f_b)
    return Q


def map_of(Q, shape):
    return (Q[:, 1] > Q[:, 0]).reshape(shape)


def resize_plane(mask, H, W):
    """crf.py's F.interpolate(mode="bilinear") of the foreground logit plane (align_corners=False), in fp64."""
    import torch
    import torch.nn.functional as F

    t = torch.from_numpy(np.asarray(mask, dtype=np.float64))[None, None]
    return F.interpolate(t, size=(H, W), mode="bilinear")[0, 0].numpy()


def densecrf(rgb, mask, iters=MAX_ITER, dtype=np.float64):
    """evals/models/crf.py::densecrf -> (MAP [H, W] bool, Q_1 [H, W])."""
    H, W = rgb.shape[:2]
    plane = np.asarray(mask, dtype=np.float64) if mask.shape == (H, W) else resize_plane(mask, H, W)
    Q = mean_field(kernel_matrices(rgb, dtype), plane, iters)
    return map_of(Q, (H, W)), Q[:, 1].reshape(H, W)


def fill_holes(mask):
    return ndimage.binary_fill_holes(np.asarray(mask) != 0)


def keeps(refined, ref):
    """The IoU rule on integer counts: dropped iff 2 |A & B| < |A | B|; an empty union keeps the mask."""
    a, b = np.asarray(refined) != 0, np.asarray(ref) != 0
    return not (2 * int((a & b).sum()) < int((a | b).sum()))


def refine_chain(rgb, inputs, iters=MAX_ITER):
    """maskcut_processor.py:376-404 for one image: inputs = the per-pass CRF inputs [H, W] 0 / 1
    -> (union [H, W] bool, per pass: (Q_1, refined, kept))."""
    H, W = rgb.shape[:2]
    kernels = kernel_matrices(rgb)
    union = np.zeros((H, W), dtype=bool)
    passes = []
    for m in inputs:
        Q = mean_field(kernels, np.asarray(m, dtype=np.float64), iters)
        filled = fill_holes(map_of(Q, (H, W)))
        kept = keeps(filled, m)
        refined = filled if kept else np.zeros_like(filled)
        union |= refined
        passes.append((Q[:, 1].reshape(H, W), refined, kept))
    return fill_holes(union), passes


# ------------------------------------------------------------------------------------------------ fixtures
def true_mask(S):
    y, x = np.mgrid[0:S, 0:S].astype(np.float64)
    return ((y - 0.45 * S) / (0.27 * S)) ** 2 + ((x - 0.55 * S) / (0.22 * S)) ** 2 <= 1.0


def input_mask(S):
    """The true mask's 8-pixel block average > 0.3, rolled one cell along x, back at pixel size."""
    blocks = true_mask(S).reshape(S // 8, 8, S // 8, 8).mean(axis=(1, 3)) > 0.3
    return np.kron(np.roll(blocks, 1, axis=1), np.ones((8, 8), dtype=bool)).astype(np.uint8)


def image(kind, S, seed=0):
    rng = np.random.default_rng(seed)
    t = true_mask(S)
    if kind == "flat":
        base = np.where(t[..., None], np.array([200, 120, 60]), np.array([40, 90, 160]))
        return (base + rng.integers(-4, 5, size=(S, S, 3))).astype(np.uint8)
    if kind == "noisy":  # SyntheticVOC's texture: uniform noise, the object half a range brighter
        rgb = rng.uniform(0.0, 0.5, size=(S, S, 3)) + 0.5 * t[..., None]
        return np.round(255.0 * rgb).clip(0, 255).astype(np.uint8)
    raise ValueError(kind)


FIXTURES = [("noisy", 48), ("noisy", 64), ("flat", 48), ("flat", 64)]


@functools.lru_cache(None)
def fixture(kind, S):
    """(rgb [S, S, 3] uint8, input mask [S, S] uint8, true mask [S, S] bool, oracle Q [N, 2] fp64, fp32-oracle Q [N, 2])."""
    rgb, m = image(kind, S), input_mask(S)
    Q64 = mean_field(kernel_matrices(rgb), m.astype(np.float64))
    Q32 = mean_field(kernel_matrices(rgb, np.float32), m.astype(np.float64))
    for a in (rgb, m, Q64, Q32):
        a.setflags(write=False)
    return rgb, m, true_mask(S), Q64, Q32


def iou(a, b):
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    return float((a & b).sum()) / float((a | b).sum())
