"""fp64 reference of the resampling kernels (csrc/resize.hip) for tests/test_gpu_resize.py, checked on its own by
tests/test_resize_ref_cpu.py.  Plain numpy / torch; nothing is imported from ``mvp``.

Resampling is separable and linear, so one axis is a matrix: ``W[o, i]`` is the weight of input index i in output index o.

    forward(X, Wy, Wx) = Wy X Wx^T          adjoint(G, Wy, Wx) = Wy^T G Wx

``axis_matrix`` builds W with ATen's definitions (area_pixel_compute_source_index; cubic A = -0.75 with taps clamped onto the border,
where they add up); ``aa_axis_matrix`` is the stretched, renormalised triangle of _upsample_bilinear2d_aa.  The source coordinate is
evaluated in fp64, EXCEPT for nearest: the choice of an index is discontinuous, so the index is computed in ATen's fp32 arithmetic
(one fp32 multiply, then floor).  torch's float64 nearest picks other indices (9 of 8200 outputs for 25 -> 8200), so an fp64 nearest
reference would be wrong about what the kernel has to return.  Nearest has no ``align_corners`` form (torch raises ValueError).

Each builder also returns the support ``S`` (0/1): the taps the definition names for an output index, whether or not their weight
happens to be zero, for ANY coordinate within |ds| of the fp64 one (|ds| as below, with the axis' own length).  Away from integer
coordinates that is the fp64 tap set.  Where the fp64 coordinate sits on an integer (align_corners 83 -> 20 ends on 82 exactly) fp32
may land just below it and name the neighbour on the other side with a weight of up to D |ds|; that neighbour's value is then part
of what the element may legitimately see, so it belongs to the footprint F and to n_terms.  (The first GPU run of these tests showed
it: an input row that no output touches in fp64 received 7.2e-6 from one that fp32 places 5e-6 below the integer; ATen's own fp32
kernels do the same.)

The bound (``bound``), per output element, from the reference alone.  u = 2^-24 is fp32's unit roundoff.

  * The kernel's source coordinate takes at most 3 fp32 roundings (the scale, its product with o or o + 0.5, the subtraction of
    0.5) of values no larger than the axis, and the subtraction of the floor adds one more of the same size:
    |ds| <= 4 u max(Hi, Wi).
  * A weight is a polynomial of the coordinate's fraction with |dw/ds| <= D.  D = 1 for bilinear and for the antialiased triangle
    (its argument is scaled by inv <= 1).  Bicubic: the near piece 1.25 x^3 - 2.25 x^2 + 1 has the derivative 3.75 x^2 - 4.5 x,
    largest in magnitude on [0, 1] at x = 0.6: 1.35; the far piece -0.75 (t^3 - 5 t^2 + 8 t - 4) has -0.75 (3 t^2 - 10 t + 8),
    at most 0.75 on [1, 2].  D = 1.5 is used for all.  Evaluating the polynomial (or the renormalising division) adds at most
    8 u.  So |dw| <= 1.5 * 4 u max(Hi, Wi) + 8 u = u (6 max(Hi, Wi) + 8).
  * A product of two weights, both <= 1 in magnitude, moves by at most twice that: u (12 max + 16).
  * Every product-and-add into the accumulator adds u of the running sum: n_terms u in all.
  * Each of these is relative to |input|, so the element's error is at most  u (12 max(Hi, Wi) + 16 + n_terms) F  with
    F = the sum of |input| over the element's footprint:  Sy |X| Sx^T  forward,  Sy^T |G| Sx  adjoint, and
    n_terms = (Sy 1)(Sx 1)^T (or the transposed sums for the adjoint).

        bound = 2 u (12 max(Hi, Wi) + 16 + n_terms) F

    The factor 2 is the only margin.  Nearest forward is a copy: the bound is 0 (exact equality).  Nearest adjoint is a sum of
    n_terms inputs with weight 1: bound = 2 u n_terms F.

``make_input`` keeps the base signal positive and within [0.7, 3.6] (a ramp plus noise, scaled per plane so that a read from the
wrong plane shows): no footprint sums to nearly nothing, so every element's bound is a statement about that element.  Its few large
values sit where the coordinate is far from an integer (a tap weight near 0.5).

``CASES`` lists every GPU case (one table for the GPU test and for the CPU sensitivity test), ``cand_window`` emulates the
kernel's fp32 candidate window so that the CPU test can assert that a case reaches the route its docstring names.
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

U = 2.0 ** -24
MODES = ("nearest", "bilinear", "bicubic")
MUTATIONS = ("shift", "nofold")  # of a builder; the adjoint's window mutations are ``shorten``
SPIKE = 4096.0
TINY = 1e-9  # a weight below this is fp64 noise of a coordinate that sits on an integer, not a tap


# ------------------------------------------------------------------------------------------------ one axis
def _scale64(align: bool, n_in: int, n_out: int, sf: float) -> float:
    if align:
        return (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    return 1.0 / sf if sf > 0 else n_in / n_out


def _put(W, S, o, idx, w, n_in, fold):
    """Add weight w of tap idx to row o; an index outside the axis is clamped onto the border (fold) or dropped."""
    inside = (idx >= 0) & (idx < n_in)
    if fold:
        idx = np.clip(idx, 0, n_in - 1)
    else:
        o, idx, w = o[inside], idx[inside], w[inside]
    np.add.at(W, (o, idx), w)
    S[o, idx] = 1.0


def axis_matrix(mode: str, align: bool, n_in: int, n_out: int, sf: float = 0.0, mutate: Optional[str] = None):
    """W [n_out, n_in] fp64 and its support S.  ``mutate``: None, or a deliberately wrong variant for the sensitivity checks:
    'shift' moves every tap index up by one, 'nofold' drops the taps that fall outside the axis instead of folding them onto
    the border."""
    assert mode in MODES and mutate in (None,) + MUTATIONS
    W = np.zeros((n_out, n_in))
    S = np.zeros((n_out, n_in))
    o = np.arange(n_out)
    sh = 1 if mutate == "shift" else 0
    fold = mutate != "nofold"
    if mode == "nearest":
        assert not align, "nearest has no align_corners form"
        scale32 = np.float32(1.0) / np.float32(sf) if sf > 0 else np.float32(n_in) / np.float32(n_out)
        idx = np.minimum(np.floor(o.astype(np.float32) * scale32).astype(np.int64), n_in - 1)
        _put(W, S, o, idx + sh, np.ones(n_out), n_in, True)
        return W, S
    scale = _scale64(align, n_in, n_out, sf)
    if mutate is None:  # the support: the taps of every coordinate within ds of the fp64 one
        ds = 4.0 * U * n_in
        for d in (-ds, ds):
            _axis_taps(mode, align, scale, o, n_in, d, np.zeros_like(W), S, 0, True)
    _axis_taps(mode, align, scale, o, n_in, 0.0, W, S, sh, fold)
    return W, S


def _axis_taps(mode, align, scale, o, n_in, ds, W, S, sh, fold):
    """Bilinear / bicubic taps of the coordinate moved by ds, added to W and marked in S."""
    if mode == "bilinear":
        s = np.maximum((scale * o if align else scale * (o + 0.5) - 0.5) + ds, 0.0)
        i0 = np.minimum(s.astype(np.int64), n_in - 1)
        l1 = s - i0
        _put(W, S, o, i0 + sh, 1.0 - l1, n_in, True)
        _put(W, S, o, i0 + 1 + sh, l1, n_in, fold)
        return
    s = (scale * o if align else scale * (o + 0.5) - 0.5) + ds
    fl = np.floor(s)
    x = s - fl
    i = fl.astype(np.int64)
    A = -0.75

    def near(t):
        return ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0

    def far(t):
        return ((A * t - 5.0 * A) * t + 8.0 * A) * t - 4.0 * A

    for k, w in enumerate((far(x + 1.0), near(x), near(1.0 - x), far(2.0 - x))):
        _put(W, S, o, i - 1 + k + sh, w, n_in, fold)


def aa_axis_matrix(n_in: int, n_out: int, mutate: Optional[str] = None):
    """The antialiased triangle of _upsample_bilinear2d_aa (align_corners = False, sizes given): scale = in / out, support =
    max(scale, 1), taps renormalised over the part of the window that lies inside the axis.  'nofold' normalises by the whole
    window instead (the mass cut off by the border is lost), 'shift' moves every tap index up by one."""
    W = np.zeros((n_out, n_in))
    S = np.zeros((n_out, n_in))
    scale = n_in / n_out
    support = max(scale, 1.0)
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    sh = 1 if mutate == "shift" else 0
    ds = 4.0 * U * n_in
    for o in range(n_out):
        center = scale * (o + 0.5)
        if mutate is None:  # the support: the windows of every centre within ds of the fp64 one
            for c in (center - ds, center + ds):
                S[o, max(int(math.floor(c - support + 0.5)), 0):min(int(math.floor(c + support + 0.5)), n_in)] = 1.0
        lo_all, hi_all = int(math.floor(center - support + 0.5)), int(math.floor(center + support + 0.5))
        lo, hi = max(lo_all, 0), min(hi_all, n_in)
        j = np.arange(lo_all, hi_all)
        w = np.maximum(1.0 - np.abs((j - center + 0.5) * inv), 0.0)
        inside = (j >= lo) & (j < hi)
        total = w.sum() if mutate == "nofold" else w[inside].sum()
        idx = np.clip(j[inside] + sh, 0, n_in - 1)
        np.add.at(W[o], idx, w[inside] / total)
        S[o, idx] = 1.0
    return W, S


def shorten(W: np.ndarray, end: str) -> np.ndarray:
    """The adjoint's window of every input index (the outputs with a weight on it) shortened by one at its 'lo' or 'hi' end."""
    W = W.copy()
    for i in range(W.shape[1]):
        nz = np.flatnonzero(np.abs(W[:, i]) > TINY)
        if nz.size:
            W[nz[0] if end == "lo" else nz[-1], i] = 0.0
    return W


# ------------------------------------------------------------------------------------------------ two axes
def forward(X, Wy, Wx):
    """X [P, Hi, Wi] fp64 -> [P, Ho, Wo]."""
    return Wy @ X @ Wx.T


def adjoint(G, Wy, Wx):
    """G [P, Ho, Wo] fp64 -> [P, Hi, Wi]."""
    return Wy.T @ G @ Wx


def to_cl(x, B, C):
    """planar [B * C, H, W] -> channels-last [B, H, W, C]."""
    return x.reshape(B, C, x.shape[-2], x.shape[-1]).permute(0, 2, 3, 1).contiguous()


def from_cl(x):
    """channels-last [B, H, W, C] -> planar [B * C, H, W]."""
    B, H, W, C = x.shape
    return x.permute(0, 3, 1, 2).reshape(B * C, H, W).contiguous()


def forward_cl(X, Wy, Wx):
    B, _, _, C = X.shape
    return to_cl(forward(from_cl(X), Wy, Wx), B, C)


def adjoint_cl(G, Wy, Wx):
    B, _, _, C = G.shape
    return to_cl(adjoint(from_cl(G), Wy, Wx), B, C)


def bound(direction: str, mode: str, src, Sy, Sx, Hi: int, Wi: int):
    """Per-element bound of the module docstring.  ``direction`` 'fwd' (src = X [P, Hi, Wi]) or 'bwd' (src = G [P, Ho, Wo]);
    ``mode`` one of MODES or 'aa'."""
    a = src.abs()
    if direction == "fwd":
        F = forward(a, Sy, Sx)
        n = torch.outer(Sy.sum(1), Sx.sum(1))
    else:
        F = adjoint(a, Sy, Sx)
        n = torch.outer(Sy.sum(0), Sx.sum(0))
    if mode == "nearest":
        return torch.zeros_like(F) if direction == "fwd" else 2.0 * U * n * F
    return 2.0 * U * (12.0 * max(Hi, Wi) + 16.0 + n) * F


def worst(err, bnd):
    """(largest err / bound ratio, its index); 0 / 0 counts as 0 and x / 0 as inf."""
    r = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    k = int(torch.argmax(r))
    return float(r.flatten()[k]), tuple(int(v) for v in np.unravel_index(k, tuple(r.shape)))


def rel_l2(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------ the kernel's windows
def cand_window(mode: str, align: bool, n_in: int, n_out: int, sf: float = 0.0) -> np.ndarray:
    """Width of the adjoint's candidate window of every input index, with the kernel's own fp32 arithmetic (cand_range).  Only
    used to assert which branch a case reaches: cached (<= 64 rows, <= 24 columns channels-last) or not."""
    f = np.float32
    if align:
        scale = f(n_in - 1) / f(n_out - 1) if n_out > 1 else f(0)
    else:
        scale = f(1) / f(sf) if sf > 0 else f(n_in) / f(n_out)
    if scale <= 0:
        return np.full(n_in, n_out)
    r = f(2) if mode == "bicubic" else f(1)
    off = f(0) if (align or mode == "nearest") else f(0.5)
    i = np.arange(n_in).astype(f)
    lo = np.maximum(0, np.floor((i - r + off) / scale - off).astype(np.int64) - 1)
    hi = np.minimum(n_out - 1, np.ceil((i + r + off) / scale - off).astype(np.int64) + 1)
    lo[0], hi[-1] = 0, n_out - 1
    return hi - lo + 1


# ------------------------------------------------------------------------------------------------ the cases
@dataclass(frozen=True)
class Case:
    group: str
    P: int                      # planes; the batch B when channels-last
    Hi: int
    Wi: int
    Ho: int
    Wo: int
    mode: str                   # one of MODES, or 'aa'
    align: bool = False
    C: int = 0                  # > 0: channels-last with C channels
    sf: Tuple[float, float] = (0.0, 0.0)

    @property
    def id(self):
        s = f"{self.group}-{self.mode}{'-align' if self.align else ''}-{self.P}x{self.Hi}x{self.Wi}-to-{self.Ho}x{self.Wo}"
        if self.C:
            s += f"-C{self.C}"
        if self.sf != (0.0, 0.0):
            s += f"-sf{self.sf[0]:g}x{self.sf[1]:g}"
        return s

    @property
    def planes(self):
        return self.P * max(self.C, 1)

    @property
    def directions(self):
        return ("fwd",) if self.mode == "aa" else ("fwd", "bwd")


FIVE = (("nearest", False), ("bilinear", False), ("bilinear", True), ("bicubic", False), ("bicubic", True))


def _cases():
    c = []
    for Wo in (1, 2, 3, 17, 128, 129, 300):                                              # a
        c += [Case("a", 3, 4, 7, 5, Wo, m, al) for m, al in FIVE]
    c.append(Case("b", 260, 8, 8, 256, 129, "bilinear"))                                  # b
    for hi, wi, ho, wo in ((20, 28, 83, 114), (3, 300, 7, 700), (83, 114, 20, 28)):       # c
        c += [Case("c", 2, hi, wi, ho, wo, m, al) for m, al in FIVE]
    c += [Case("d", 2, 7, 5, 112, 9, "bicubic"), Case("d", 2, 7, 5, 112, 9, "bicubic", True),  # d
          Case("d", 2, 4, 5, 128, 9, "bilinear"), Case("d", 2, 4, 5, 128, 9, "bilinear", True),
          Case("d", 2, 4, 5, 128, 9, "nearest"), Case("d", 1, 14, 14, 224, 224, "bicubic")]
    c += [Case("e", 8200, 8, 3, 16, 6, "bicubic"), Case("e", 8200, 8, 3, 16, 6, "bilinear")]  # e
    for wi, wo in ((2048, 8192), (2050, 8200)):                                           # f
        c += [Case("f", 1, 3, wi, 5, wo, m, al) for m, al in FIVE]
    c.append(Case("g", 1, 130, 2050, 131, 8200, "bilinear"))                              # g
    for C in (4, 8, 132):                                                                 # h
        c += [Case("h", 2, 5, 7, 20, 28, m, al, C) for m, al in FIVE]
        c += [Case("h", 2, 6, 6, 36, 36, "bicubic", False, C), Case("h", 2, 6, 6, 30, 30, "bicubic", False, C),
              Case("h", 2, 4, 4, 44, 44, "bilinear", False, C), Case("h", 2, 4, 4, 44, 44, "nearest", False, C)]
    c += [Case("h", 2, 36, 36, 6, 6, m, al, 8) for m, al in FIVE]
    c += [Case("i", 1, 260, 260, 130, 130, "bilinear", False, 128), Case("i", 1, 130, 130, 260, 260, "bilinear", False, 128)]  # i
    for hi, wi, ho, wo in ((1, 1, 5, 7), (1, 9, 4, 9), (6, 1, 6, 5), (7, 9, 1, 1), (7, 9, 1, 4), (7, 9, 3, 1), (6, 9, 6, 9),
                           (12, 40, 40, 12)):                                             # j
        c += [Case("j", 2, hi, wi, ho, wo, m, al) for m, al in FIVE]
    for sf in ((2.5, 2.5), (1.5, 0.5), (4.0, 4.0)):                                       # k
        ho, wo = int(7 * sf[0]), int(9 * sf[1])
        c += [Case("k", 6, 7, 9, ho, wo, m, al, 0, sf) for m, al in FIVE[:4]]
    c += [Case("l", 2, 530, 300, 7, 224, "aa"), Case("l", 2, 96, 150, 1, 64, "aa"), Case("l", 2, 64, 64, 64, 64, "aa"),  # l
          Case("l", 2, 64, 48, 96, 20, "aa"), Case("l", 2, 9, 9, 2, 2, "aa")]
    return c


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def matrices(case: Case, mutate: Optional[str] = None):
    """(Wy, Sy, Wx, Sx) of a case as fp64 torch tensors; ``mutate`` is applied to both axes (the kernels share one tap
    function between the axes, so a mistake in it shows on both)."""
    if case.mode == "aa":
        m = aa_axis_matrix(case.Hi, case.Ho, mutate) + aa_axis_matrix(case.Wi, case.Wo, mutate)
    else:
        m = (axis_matrix(case.mode, case.align, case.Hi, case.Ho, case.sf[0], mutate)
             + axis_matrix(case.mode, case.align, case.Wi, case.Wo, case.sf[1], mutate))
    return tuple(torch.from_numpy(a) for a in m)


def _base(planes, H, W, seed):
    """1 + a ramp + uniform noise in [0.7, 1.8], times 1, 1.5 or 2 by plane: positive and bounded away from zero."""
    rng = np.random.default_rng(seed)
    y = np.arange(H, dtype=np.float64)[:, None] / max(H - 1, 1)
    x = np.arange(W, dtype=np.float64)[None, :] / max(W - 1, 1)
    a = 1.0 + 0.3 * y + 0.2 * x + rng.uniform(-0.3, 0.3, size=(planes, H, W))
    return a * (1.0 + 0.5 * (np.arange(planes) % 3))[:, None, None]


def _edge(W, end):
    """(o, i): the window end of the input index whose end weight is closest to 0.5 (a weak-but-visible tap whose coordinate
    is far from an integer)."""
    best = None
    for i in range(W.shape[1]):
        nz = np.flatnonzero(np.abs(W[:, i]) > TINY)
        if nz.size:
            o = nz[0] if end == "lo" else nz[-1]
            d = abs(abs(W[o, i]) - 0.5)
            if best is None or d < best[0]:
                best = (d, int(o), i)
    return best[1], best[2]


def _mid(W, i):
    """The output index whose weight on input i (or on the nearest input index that has any weight) is closest to 0.5."""
    live = np.flatnonzero((np.abs(W) > TINY).any(axis=0))
    i = int(live[np.argmin(np.abs(live - i))])
    col = np.abs(W[:, i])
    col = np.where(col > TINY, np.abs(col - 0.5), np.inf)
    return int(np.argmin(col))


def make_input(case: Case, which: str) -> torch.Tensor:
    """The fp32 input of a case in planar form: 'x' [planes, Hi, Wi] for the forward, 'g' [planes, Ho, Wo] for the adjoint.
    'g' carries four values of SPIKE in plane 0, one on each end of one adjoint window per axis: a weak tap dropped at the end of
    a wide window is then larger than the bound of the element that loses it.  'x' carries two in the antialiased cases, whose
    windows are wide in the forward direction: one in the middle and one under the corner output.  All positions come from the reference matrices."""
    if which == "x":
        a = _base(case.planes, case.Hi, case.Wi, zlib.crc32(case.id.encode()))
        if case.mode == "aa":
            a[0, case.Hi // 2, case.Wi // 2] = SPIKE
            Wy, _, Wx, _ = (m.numpy() for m in matrices(case))
            a[0, int(np.argmax(Wy[0])), int(np.argmax(Wx[0]))] = SPIKE  # the peak tap of the corner output, whose windows the border cuts
    else:
        a = _base(case.planes, case.Ho, case.Wo, zlib.crc32(case.id.encode()) + 1)
        Wy, _, Wx, _ = (m.numpy() for m in matrices(case))
        for end in ("lo", "hi"):
            oy, iy = _edge(Wy, end)
            a[0, oy, _mid(Wx, case.Wi // 2)] = SPIKE
            ox, ix = _edge(Wx, end)
            a[0, _mid(Wy, case.Hi // 2), ox] = SPIKE
    return torch.from_numpy(a.astype(np.float32))


def reference(case: Case, direction: str, src: torch.Tensor, mats=None):
    """(ref, bound) of one direction, planar fp64, for the fp32 input ``src`` (planar)."""
    Wy, Sy, Wx, Sx = mats if mats is not None else matrices(case)
    s = src.double()
    ref = forward(s, Wy, Wx) if direction == "fwd" else adjoint(s, Wy, Wx)
    return ref, bound(direction, case.mode, s, Sy, Sx, case.Hi, case.Wi)
