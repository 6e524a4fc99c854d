"""fp64 oracle of the MaskCut evaluation (reference: evals/models/maskcut_processor.py, evaluate_generic_objectness.py), numpy only:
one function per step of a pass and one for the pass loop, with the same deterministic threshold rule and eigenvector sign convention
as the kernels (MaskCut deviations) and its own flood fill for components and holes.  numpy.linalg.eigh on
S = D^-1/2 W D^-1/2 plays the role of scipy.linalg.eigh(D - W, D)."""
import numpy as np

EPS = 1e-5


# ----------------------------------------------------------------------------- fixtures
def make_labels(h, w, n_objects, clean=False):
    """Background 0 and n_objects rectangles 1.., placed left to right away from the corners (where the grid allows it)."""
    lab = np.zeros((h, w), dtype=np.int64)
    if h == 1 or w == 1:
        n = h * w
        a = lab.reshape(-1)
        seg = max(1, n // (2 * n_objects + 1))
        for k in range(n_objects):
            a[(2 * k + 1) * seg:(2 * k + 2) * seg] = k + 1
        return a.reshape(h, w)
    y0, y1 = max(1, h // 4), max(2, h - h // 4)
    span = w - 2
    seg = max(1, span // (2 * n_objects))
    for k in range(n_objects):
        x0 = 1 + 2 * k * seg + (0 if clean else seg // 4)
        x1 = min(w - 1, x0 + seg + (seg // 2 if k == 0 else 0))
        yy0 = y0 + (k % 2) * (0 if clean else max(0, (y1 - y0) // 4))
        lab[yy0:y1, x0:x1] = k + 1
    return lab


# name -> (h, w, C, objects, seed, noise, ramp, clean); what each is for: tests/test_gpu_maskcut_kernels.py
FIXTURES = {
    "5x7": (5, 7, 24, 1, 11, 1.0, 0.3, False),
    "9x13": (9, 13, 40, 2, 17, 1.25, 0.3, False),
    "16x16": (16, 16, 64, 1, 13, 1.0, 0.3, False),
    "32x32": (32, 32, 64, 2, 14, 1.0, 0.3, False),
    "30x30": (30, 30, 768, 1, 15, 2.5, 0.3, False),
    "8x8": (8, 8, 32, 2, 16, 0.0, 0.0, True),
}


def fixture(name):
    """-> (feats [C, N] fp32, labels [h, w], h, w, objects)"""
    h, w, C, P, seed, noise, ramp, clean = FIXTURES[name]
    f, lab = make_feats(h, w, C, P, seed, noise=noise, ramp=ramp, clean=clean)
    return f, lab, h, w, P


def make_feats(h, w, C, n_objects, seed, noise=1.0, ramp=0.3, clean=False):
    """features = prototype[label] + noise + a smooth ramp, seeded -> (feats [C, N] fp32, labels [h, w]).  clean: orthogonal
    prototypes, no noise and no ramp (cleanly separated components: lambda_2 ~ lambda_3)."""
    rng = np.random.RandomState(seed)
    lab = make_labels(h, w, n_objects, clean)
    if clean:
        proto = np.eye(n_objects + 1, C)
        f = proto[lab.reshape(-1)].T.copy()
        return f.astype(np.float32), lab
    proto = rng.randn(n_objects + 1, C)
    proto /= np.linalg.norm(proto, axis=1, keepdims=True)
    yy, xx = np.mgrid[0:h, 0:w]
    rdir = rng.randn(2, C) / np.sqrt(C)
    f = proto[lab.reshape(-1)].T
    f = f + noise * rng.randn(C, h * w) / np.sqrt(C)
    f = f + ramp * (rdir[0][:, None] * (yy.reshape(-1) / max(1, h - 1) - 0.5) + rdir[1][:, None] * (xx.reshape(-1) / max(1, w - 1) - 0.5))
    return f.astype(np.float32), lab


# ----------------------------------------------------------------------------- steps
def affinity(feats, painted=None):
    """get_masked_affinity_matrix + F.normalize + F^T F in fp64.  feats [C, N]; painted [N] (0 / 1) zeroes columns."""
    f = np.asarray(feats, dtype=np.float64)
    nrm = np.maximum(np.sqrt((f * f).sum(axis=0)), 1e-12)
    f = f / nrm
    if painted is not None:
        f = f * (1.0 - (np.asarray(painted).reshape(-1) != 0).astype(np.float64))
    return f.T @ f


def lloyd_tau(A, max_rounds=64):
    """The fixed point of Lloyd's iteration for two centres started from mean -+ std -> (tau, rounds)."""
    a = np.asarray(A, dtype=np.float64).reshape(-1)
    M = a.size
    mean = a.sum() / M
    sd = np.sqrt(max((a * a).sum() / M - mean * mean, 0.0))
    c0, c1 = mean - sd, mean + sd
    prev, rounds = -1, 0
    for r in range(max_rounds):
        up = a > 0.5 * (c0 + c1)
        cnt = int(up.sum())
        rounds = r + 1
        if cnt == 0 or cnt == M:
            break
        c1, c0 = a[up].sum() / cnt, a[~up].sum() / (M - cnt)
        if cnt == prev:
            break
        prev = cnt
    return 0.5 * (c0 + c1), rounds


def threshold(A, tau):
    """-> (B bool [N, N], d [N]) with W = B + eps (1 - B), d = W 1."""
    B = np.asarray(A) > tau
    cnt = B.sum(axis=1).astype(np.float64)
    return B, cnt + EPS * (B.shape[0] - cnt)


def pack_bits(B):
    """Row-major bit matrix [N, ceil(N / 32)] uint32, bit j & 31 of word j >> 5."""
    N = B.shape[0]
    NW = (N + 31) // 32
    pad = np.zeros((N, NW * 32), dtype=np.uint64)
    pad[:, :N] = B
    return (pad.reshape(N, NW, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def unpack_bits(bits, N):
    b = np.asarray(bits).astype(np.uint32)
    return (((b[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(b.shape[0], -1)[:, :N]).astype(bool)


def normalised(B, d):
    W = np.where(B, 1.0, EPS)
    s = 1.0 / np.sqrt(d)
    return W * s[:, None] * s[None, :]


def fix_sign(v):
    """The entry of largest |v| positive, the lowest index on ties."""
    k = int(np.argmax(np.abs(v)))
    return -v if v[k] < 0 else v


def fiedler(B, d):
    """-> dict(v, lam, gap, theta): the second-smallest generalised eigenvector of (D - W) v = lam D v, v = D^-1/2 y with |y| = 1 and
    the sign convention; gap = theta_2 - theta_3 of S."""
    S = normalised(B, d)
    w, U = np.linalg.eigh(S)
    y = U[:, -2]
    v = fix_sign(y / np.sqrt(d))
    return {"v": v, "lam": 1.0 - w[-2], "theta": w[-2], "gap": w[-2] - w[-3] if len(w) > 2 else w[-2] + 1.0}


def residual(B, d, v):
    """(lam, residual) of an output vector v as the kernel reports them: y = D^1/2 v / |.|, theta = y^T S y, |S y - theta y|."""
    y = np.sqrt(d) * np.asarray(v, dtype=np.float64)
    y = y / np.linalg.norm(y)
    s = 1.0 / np.sqrt(d)
    x = s * y
    Sy = s * ((1.0 - EPS) * (B.astype(np.float64) @ x) + EPS * x.sum())
    th = float(y @ Sy)
    return 1.0 - th, float(np.linalg.norm(Sy - th * y))


def flood(seeds, open_):
    """Cells of ``open_`` 4-connected to a seed cell (seeds inside open_)."""
    h, w = open_.shape
    reach = np.zeros((h, w), dtype=bool)
    stack = [(int(y), int(x)) for y, x in zip(*np.nonzero(seeds & open_))]
    for y, x in stack:
        reach[y, x] = True
    while stack:
        y, x = stack.pop()
        for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= yy < h and 0 <= xx < w and open_[yy, xx] and not reach[yy, xx]:
                reach[yy, xx] = True
                stack.append((yy, xx))
    return reach


def fill_holes(mask):
    """ndimage.binary_fill_holes: the complement of the background 4-connected to the border."""
    m = np.asarray(mask).astype(bool)
    border = np.zeros_like(m)
    border[0, :] = border[-1, :] = True
    border[:, 0] = border[:, -1] = True
    return ~flood(border, ~m)


def bipartition(v):
    v = np.asarray(v, dtype=np.float64)
    return v > v.sum() / v.size


def corners(bip, h, w):
    b = bip.reshape(h, w)
    return int(b[0, 0]) + int(b[0, -1]) + int(b[-1, 0]) + int(b[-1, -1])


def partition(v, h, w, painted, prev=None, use_prev=False):
    """One pass after the eigenvector -> dict(mask, painted, union, seed, nc, reverse, bip); masks are bool [h, w]."""
    v = np.asarray(v, dtype=np.float64)
    bip = bipartition(v)
    seed0 = int(np.argmax(np.abs(v)))
    nc = corners(bip, h, w)
    reverse = nc >= 3 or not bip[seed0]
    if reverse:
        bip = ~bip
        seed = int(np.argmin(v))
    else:
        seed = int(np.argmax(v))
    sd = np.zeros((h, w), dtype=bool)
    sd[np.unravel_index(seed, (h, w))] = True
    mask = flood(sd, bip.reshape(h, w))
    if use_prev:
        p = np.asarray(prev).reshape(h, w).astype(bool)
        inter, uni = int((mask & p).sum()), int((mask | p).sum())
        if 2 * inter > uni or mask.sum() / h / w <= 0.01:
            mask = np.zeros((h, w), dtype=bool)
    painted = np.asarray(painted).reshape(h, w).astype(bool) | mask
    return {"mask": mask, "painted": painted, "union": fill_holes(painted), "seed": seed, "nc": nc, "reverse": bool(reverse),
            "bip": bip.reshape(h, w)}


def seed_margin(v, reverse):
    """How far the seed's value is ahead of the runner-up, relative to max |v|: a solver whose error is below half of it finds the same seed."""
    s = np.sort(-np.asarray(v, dtype=np.float64) if reverse else np.asarray(v, dtype=np.float64))
    return float((s[-1] - s[-2]) / np.abs(s).max()) if s.size > 1 else 1.0


def maskcut(feats, h, w, num_objects):
    """The pass loop of maskcut_forward + the union with filled holes -> dict(union, masks, passes)."""
    painted = np.zeros((h, w), dtype=bool)
    prev, masks, passes = None, [], []
    out = None
    for i in range(num_objects):
        A = affinity(feats, painted.reshape(-1))
        tau, rounds = lloyd_tau(A)
        B, d = threshold(A, tau)
        e = fiedler(B, d)
        out = partition(e["v"], h, w, painted, prev, use_prev=i >= 1)
        painted, prev = out["painted"], out["mask"]
        masks.append(out["mask"])
        passes.append({"A": A, "tau": tau, "rounds": rounds, "B": B, "d": d, **e, **out})
    return {"union": out["union"], "masks": masks, "passes": passes}


# ----------------------------------------------------------------------------- metrics
def counts(pred, gt):
    p, g = np.asarray(pred).astype(bool), np.asarray(gt).astype(bool)
    return int((p & g).sum()), int((p & ~g).sum()), int((~p & g).sum()), int((~p & ~g).sum())


def metrics_from_counts(tp, fp, fn, tn, beta=0.3):
    """evaluate_generic_objectness.py:50-177 from the confusion counts of one image."""
    precision, recall = tp / (tp + fp + 1e-6), tp / (tp + fn + 1e-6)
    b2 = beta ** 2
    iou = tp / (tp + fp + fn + 1e-6)
    return {"F-measure": (1 + b2) * (precision * recall) / (b2 * precision + recall + 1e-6), "IoU": iou,
            "Accuracy": (tp + tn) / (tp + fp + fn + tn), "CorLoc": 1 if iou >= 0.5 else 0}


def upsample_nearest(mask, H, W):
    """F.interpolate(mode="nearest") of a [h, w] mask to [H, W]: source index floor(dst * in / out)."""
    m = np.asarray(mask)
    h, w = m.shape
    return m[(np.arange(H) * h) // H][:, (np.arange(W) * w) // W]
