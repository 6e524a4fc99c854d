"""The resampling reference of the GPU tests (tests/resize_ref.py) checked on its own, without a GPU:

  * its axis matrices against torch over a sweep of sizes, both ``align_corners`` settings and explicit scale factors (bilinear,
    bicubic and antialiased against F.interpolate on float64 to 1e-12; nearest against F.interpolate on float32, exactly);
  * its adjoint against autograd on float64;
  * the emulated candidate windows: every case of the GPU test reaches the branch its docstring names;
  * sensitivity: for every case of the GPU test, references built from deliberately wrong matrices differ from the true one by
    more than 4 x the bound on at least one element, so a kernel with that mistake could not pass;
  * the wrapper refuses ``align_corners`` with nearest, as torch does.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resize_ref as rr

SIZES = list(range(1, 41)) + [56, 83, 112, 224, 480]


def _torch_axis(n_in, n_out, dtype, **kw):
    """The matrix F.interpolate applies along H, read off the identity image (W keeps its size, which every mode maps to itself)."""
    x = torch.eye(n_in, dtype=dtype).reshape(1, 1, n_in, n_in)
    if "scale_factor" in kw:
        kw = dict(kw, scale_factor=(kw["scale_factor"], 1.0))
    else:
        kw = dict(kw, size=(n_out, n_in))
    return F.interpolate(x, **kw)[0, 0].contiguous()


@pytest.mark.parametrize("mode,align", [("bilinear", False), ("bilinear", True), ("bicubic", False), ("bicubic", True)])
def test_axis_matrix_matches_torch_float64(mode, align):
    worst = 0.0
    for n_in in SIZES:
        for n_out in SIZES:
            W, S = rr.axis_matrix(mode, align, n_in, n_out)
            ref = _torch_axis(n_in, n_out, torch.float64, mode=mode, align_corners=align).numpy()
            worst = max(worst, float(np.abs(W - ref).max()))
            assert np.abs(W - ref).max() <= 1e-12, (mode, align, n_in, n_out)
            assert ((W != 0) <= (S == 1)).all() and S.sum(1).max() <= (3 if mode == "bilinear" else 5)  # (one more where the coordinate is an integer)
            assert np.abs(W.sum(1) - 1).max() <= 1e-12
    print(f"\n[resize-ref] {mode} align={align}: max |W - torch| = {worst:.2e} over {len(SIZES) ** 2} size pairs")


def test_nearest_matrix_matches_torch_float32_exactly():
    for n_in in SIZES:
        for n_out in SIZES:
            W, S = rr.axis_matrix("nearest", False, n_in, n_out)
            ref = _torch_axis(n_in, n_out, torch.float32, mode="nearest").double().numpy()
            assert np.array_equal(W, ref) and np.array_equal(S, W), (n_in, n_out)
    # the pairs at which torch's own float64 path picks other indices: the reference has to follow fp32
    for n_in, n_out in ((25, 8200), (530, 480)):
        W, _ = rr.axis_matrix("nearest", False, n_in, n_out)
        assert np.array_equal(W, _torch_axis(n_in, n_out, torch.float32, mode="nearest").double().numpy())


def test_aa_matrix_matches_torch_float64():
    for n_in in SIZES:
        for n_out in SIZES:
            W, S = rr.aa_axis_matrix(n_in, n_out)
            ref = _torch_axis(n_in, n_out, torch.float64, mode="bilinear", align_corners=False, antialias=True).numpy()
            assert np.abs(W - ref).max() <= 1e-12, (n_in, n_out)
            assert ((W != 0) <= (S == 1)).all()


@pytest.mark.parametrize("sf", [2.5, 1.5, 0.5, 4.0])
@pytest.mark.parametrize("mode", rr.MODES)
def test_scale_factor_axis_matches_torch(mode, sf):
    """With a scale factor the coordinate uses 1 / sf, not in / out (they differ whenever in * sf is not an integer)."""
    for n_in in (2, 3, 7, 9, 13, 30):
        n_out = int(n_in * sf)
        W, _ = rr.axis_matrix(mode, False, n_in, n_out, sf)
        if mode == "nearest":
            assert np.array_equal(W, _torch_axis(n_in, n_out, torch.float32, mode=mode, scale_factor=sf).double().numpy())
        else:
            ref = _torch_axis(n_in, n_out, torch.float64, mode=mode, scale_factor=sf, align_corners=False).numpy()
            assert np.abs(W - ref).max() <= 1e-12, (n_in, sf)


@pytest.mark.parametrize("mode,align", rr.FIVE)
@pytest.mark.parametrize("sf", [None, 2.5, (1.5, 0.5)])
def test_forward_and_adjoint_match_torch_and_autograd(mode, align, sf):
    g = torch.Generator().manual_seed(5)
    dt = torch.float32 if mode == "nearest" else torch.float64
    x = torch.randn(2, 3, 7, 9, generator=g, dtype=dt).requires_grad_(True)
    kw = dict(size=(10, 23)) if sf is None else dict(scale_factor=sf)
    if mode != "nearest":
        kw["align_corners"] = align
    y = F.interpolate(x, mode=mode, **kw)
    gy = torch.randn(y.shape, generator=g, dtype=dt)
    y.backward(gy)
    sfs = (0.0, 0.0) if sf is None else (sf, sf) if not isinstance(sf, tuple) else sf
    Wy, _ = rr.axis_matrix(mode, align, 7, y.shape[2], sfs[0])
    Wx, _ = rr.axis_matrix(mode, align, 9, y.shape[3], sfs[1])
    Wy, Wx = torch.from_numpy(Wy), torch.from_numpy(Wx)
    tol = 1e-5 if mode == "nearest" else 1e-12  # (fp32 sums of torch's own nearest backward)
    assert float((rr.forward(x.detach().double().flatten(0, 1), Wy, Wx) - y.detach().double().flatten(0, 1)).abs().max()) <= (0 if mode == "nearest" else tol)
    assert float((rr.adjoint(gy.double().flatten(0, 1), Wy, Wx) - x.grad.double().flatten(0, 1)).abs().max()) <= tol
    # channels-last forms: the same operator on permuted data
    xc = rr.to_cl(x.detach().double().flatten(0, 1), 2, 3)
    assert torch.equal(rr.from_cl(xc), x.detach().double().flatten(0, 1))
    assert torch.equal(rr.forward_cl(xc, Wy, Wx), rr.to_cl(rr.forward(rr.from_cl(xc), Wy, Wx), 2, 3))
    assert torch.equal(rr.adjoint_cl(rr.to_cl(gy.double().flatten(0, 1), 2, 3), Wy, Wx), rr.to_cl(rr.adjoint(gy.double().flatten(0, 1), Wy, Wx), 2, 3))


# ------------------------------------------------------------------------------------------------ routes
def _wy(c):
    return rr.cand_window(c.mode, c.align, c.Hi, c.Ho, c.sf[0])


def _wx(c):
    return rr.cand_window(c.mode, c.align, c.Wi, c.Wo, c.sf[1])


def test_cases_reach_the_routes_they_name():
    """The grid arithmetic and the candidate windows (the kernel's own fp32 expressions) behind the table of test_gpu_resize.py."""
    by = {}
    for c in rr.CASES:
        by.setdefault(c.group, []).append(c)
    assert sorted(by) == list("abcdefghijkl")
    # a: cw_log2 = 0, 1, 2, 5, 7, 8, 8 and the ox += cw loop at Wo = 300 > 256
    assert sorted({c.Wo for c in by["a"]}) == [1, 2, 3, 17, 128, 129, 300]
    # b: rb = 256 >> 8 = 1 row per block, rows = planes * Ho > the 65536-block cap
    (b,) = by["b"]
    assert b.Wo > 128 and b.planes * b.Ho == 66560 > 65536
    # c: cached (ny <= 64) with every ny % 4, and rows wider than one sweep of 256 lanes
    rem = set()
    for c in by["c"]:
        w = _wy(c)
        assert w.max() <= 64
        rem |= {int(v) % 4 for v in w}
    assert rem == {0, 1, 2, 3}
    assert any(c.Wo > 256 and c.Wi > 256 for c in by["c"])
    # d: uncached rows (ny > 64) mixed with cached edge rows in one launch
    got = {c.id: _wy(c) for c in by["d"]}
    w = got["d-bicubic-2x7x5-to-112x9"]
    assert sorted(set(w.tolist())) == [42, 58, 68] and w.min() <= 64 < w.max()
    assert got["d-bicubic-align-2x7x5-to-112x9"].max() == 78
    assert got["d-bilinear-align-2x4x5-to-128x9"].max() == 87 and got["d-bilinear-2x4x5-to-128x9"].max() > 64
    assert got["d-nearest-2x4x5-to-128x9"].max() > 64
    assert got["d-bicubic-1x14x14-to-224x224"].max() == 68 and got["d-bicubic-1x14x14-to-224x224"].min() <= 64
    # e: rows = planes * Hi = 65600 > 65536 blocks, cached (the LDS weights are rewritten on the second trip)
    for c in by["e"]:
        assert c.planes * c.Hi == 65600 and _wy(c).max() <= 64
    # f: Wo = 8192 is the last width of the LDS row buffer, 8200 the first shape of the fallback kernel in the table
    assert sorted({c.Wo for c in by["f"]}) == [8192, 8200]
    # g: fallback, 8192 blocks * 32 elements = 262144 per sweep; the element count is no multiple of 32 (nor of 8)
    (g,) = by["g"]
    n = g.planes * g.Hi * g.Wi
    assert g.Wo > 8192 and n == 266500 > 262144 and n % 32 and n % 8
    # h: C4 = 1, 2, 33; register cache (nx <= 24) hit and miss
    assert sorted({c.C for c in by["h"]}) == [4, 8, 132]
    hx = {c.id: int(_wx(c).max()) for c in by["h"] if c.C == 8}
    assert hx["h-bicubic-2x6x6-to-36x36-C8"] == 28 and hx["h-bicubic-2x6x6-to-30x30-C8"] == 23
    assert hx["h-bilinear-2x4x4-to-44x44-C8"] == 25 and hx["h-nearest-2x4x4-to-44x44-C8"] > 24
    assert hx["h-bicubic-2x5x7-to-20x28-C8"] <= 24
    # i: more float4 than 8192 blocks * 256 lanes, on the output side one way and the input side the other
    for c in by["i"]:
        assert max(c.Hi * c.Wi, c.Ho * c.Wo) * c.P * (c.C // 4) == 2163200 > 8192 * 256
    # j: the scale is 0 under align_corners at one output -> the whole axis is the window
    assert int(rr.cand_window("bilinear", True, 7, 1)[0]) == 1 and int(rr.cand_window("bicubic", True, 9, 1).max()) == 1
    # k: scale factors whose 1 / sf is not in / out
    assert any(c.sf[0] and c.Hi / c.Ho != 1.0 / c.sf[0] for c in by["k"])


# ------------------------------------------------------------------------------------------------ sensitivity
# (case id, direction, mutation) at which NO input can show the mutation within the bound.  A wrong reference differs by
# sum_j dW_j x_j and the bound is k sum_j |x_j| over the footprint with k = 2 u (12 max(Hi, Wi) + 16 + n_terms), so as long as dW stays
# inside the footprint the ratio is at most max_j |dW_j| / k, whatever the input (``_reach``).  530 x 300 -> 7 x 224 antialiased: a
# window of 151 rows x 3 columns makes every weight about 1 / 100 (the corner output's largest is 0.0150 x 0.697), the lost border mass
# changes it by 2.1e-3, and k = 7.9e-4 (12 x 530 + 16 + 228 terms): 2.7, short of 4.  The bound follows from its derivation and is not
# narrowed for this case; the smaller antialiased cases (9 -> 2, 96 -> 1, 64 x 48 -> 96 x 20) do resolve the same mutation.  Listed, not skipped: the test asserts that this entry is
# out of reach of every input and that every other mutation of every case is caught.
OUT_OF_REACH = {("l-aa-2x530x300-to-7x224", "fwd", "nofold")}


def _reach(case, direction, mats, mut):
    """max over elements of (largest |change of a two-axis weight| of the element) / (bound of a unit input on that tap): the most
    any input could make of the mutation, relative to the bound."""
    Wy, Sy, Wx, Sx = mats
    My, Mx = mut
    if direction == "bwd":
        Wy, Sy, Wx, Sx, My, Mx = Wy.T, Sy.T, Wx.T, Sx.T, My.T, Mx.T
    ny, nx = Sy.sum(1), Sx.sum(1)
    best = 0.0
    for oy in range(Wy.shape[0]):
        d = (Wy[oy][None, :, None] * Wx[:, None, :] - My[oy][None, :, None] * Mx[:, None, :]).abs()
        outside = (Sy[oy][None, :, None] * Sx[:, None, :]) == 0  # a weight on an input outside the footprint: no bound covers it
        d = torch.where(outside & (d > 0), torch.full_like(d, float("inf")), d).amax(dim=(1, 2))
        k = 2.0 * rr.U * ((12.0 * max(case.Hi, case.Wi) + 16.0 if case.mode != "nearest" else 0.0) + ny[oy] * nx)
        best = max(best, float((d / k.clamp_min(1e-300)).max()))
    return best


@pytest.mark.parametrize("cid", [c.id for c in rr.CASES])
def test_bound_is_tight_enough_to_catch_a_wrong_kernel(cid):
    case = rr.BY_ID[cid]
    true = rr.matrices(case)
    Wy, Sy, Wx, Sx = true
    muts = {}
    for m in rr.MUTATIONS:
        My, _, Mx, _ = rr.matrices(case, m)
        if not (torch.equal(My, Wy) and torch.equal(Mx, Wx)):  # (e.g. no tap is clamped: 'nofold' is the same operator)
            muts[m] = (My, Mx)
    applicable = 0
    for direction in case.directions:
        src = rr.make_input(case, "x" if direction == "fwd" else "g")
        ref, bnd = rr.reference(case, direction, src, true)
        assert bool((bnd >= 0).all()) and bool(torch.isfinite(ref).all())
        todo = dict(muts)
        if direction == "bwd":
            for end in ("lo", "hi"):
                todo[f"window-{end}"] = (torch.from_numpy(rr.shorten(Wy.numpy(), end)), torch.from_numpy(rr.shorten(Wx.numpy(), end)))
        for name, (My, Mx) in todo.items():
            applicable += 1
            s = src.double()
            wrong = rr.forward(s, My, Mx) if direction == "fwd" else rr.adjoint(s, My, Mx)
            ratio, where = rr.worst((wrong - ref).abs(), bnd)
            key = (cid, direction, name)
            if key in OUT_OF_REACH:
                assert _reach(case, direction, true, (My, Mx)) < 4.0, f"{key}: within reach of some input, take it off the list"
                continue
            assert ratio > 4.0, f"{cid} {direction} '{name}': the wrong reference is within {ratio:.2f} x the bound everywhere (worst at {where})"
    assert applicable >= len(case.directions)


# ------------------------------------------------------------------------------------------------ the wrapper
@pytest.mark.parametrize("align", [False, True])
def test_interpolate_refuses_align_corners_with_nearest(align):
    """torch raises ValueError there; the kernel would take (in - 1) / (out - 1) as the nearest scale, which torch never computes."""
    from mvp import functional as MF

    x = torch.zeros(1, 1, 4, 4)
    with pytest.raises(ValueError):
        F.interpolate(x, size=(8, 8), mode="nearest", align_corners=align)
    with pytest.raises(ValueError, match="align_corners"):
        MF.interpolate(x, size=(8, 8), mode="nearest", align_corners=align)
