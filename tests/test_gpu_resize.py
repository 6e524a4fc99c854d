"""The resampling kernels (csrc/resize.hip) against fp64, one output element at a time.  tests/resize_ref.py has the reference, the
case table and the bound  2 u (12 max(Hi, Wi) + 16 + n_terms) x (sum of |input| over the element's footprint),  derived there from
fp32's roundings alone; tests/test_resize_ref_cpu.py checks that reference against torch, that each case reaches the branch named
here, and that a wrong kernel (a tap index off by one, border taps dropped, an adjoint window one short) could not pass.

  a  forward planar: every column-tile width cw = 2^0 .. 2^8 and the ox += cw loop
  b  forward planar: a second trip of the grid-stride loop
  c  adjoint by rows, row weights cached in LDS: every ny % 4, rows wider than one sweep of the 256 lanes
  d  adjoint by rows, windows wider than the cache (ny > 64) next to cached edge rows in one launch
  e  adjoint by rows: a second trip of the grid-stride loop (the LDS buffers are reused)
  f  Wo = 8192, the last width the row buffer holds, and 8200, the first shape of the fallback kernel
  g  the fallback kernel: a second trip and a tail that is no multiple of 8 lanes
  h  channels-last, forward and adjoint: C / 4 = 1, 2, 33; the register cache of column weights hit and missed
  i  channels-last: a second trip of the grid-stride loop, forward and adjoint
  j  degenerate axes: length 1 in or out, in == out, one axis growing while the other shrinks
  k  explicit scale factors through ops.resize and functional.interpolate
  l  the antialiased forward
  m  argument checks

Every launch writes into a slice of a larger buffer prefilled with a NaN bit pattern, 64 floats of guard on either side (the slice
stays 16-byte aligned for the float4 kernels): afterwards the slice is all finite and the guards are untouched.  Every launch is
repeated and must give the same bits (gather form, no atomics).  Each case prints its worst error / bound ratio, where it fell and the
whole-tensor rel-L2; profiles/resize_element_error.txt keeps those figures.

Nearest has no align_corners form (torch raises), so "all modes, both aligns" is nearest, bilinear x 2, bicubic x 2.  Not covered: the
int64_t index instantiation of the channels-last kernels, which needs 2^31 float4 (32 GiB) in one tensor; nothing smaller reaches it."""
import ctypes

import pytest
import torch

import resize_ref as rr

pytestmark = pytest.mark.gpu

GUARD = 64
NAN_BITS = 0x7FC0BEEF
EINVAL = -1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _guarded(n, dev):
    """(whole int32 buffer of NaN bit patterns, its float32 slice [GUARD, GUARD + n))."""
    whole = torch.full((n + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device=dev)
    dst = whole[GUARD:GUARD + n].view(torch.float32)
    assert dst.data_ptr() % 16 == 0
    return whole, dst


def _guards_intact(whole, n):
    return bool((whole[:GUARD] == NAN_BITS).all()) and bool((whole[GUARD + n:] == NAN_BITS).all())


def _mode(case):
    from mvp import lib

    return {"nearest": lib.RESIZE_NEAREST, "bilinear": lib.RESIZE_BILINEAR, "bicubic": lib.RESIZE_BICUBIC, "aa": lib.RESIZE_BILINEAR}[case.mode]


def _launch(case, direction, src, dst, through_ops=False):
    from mvp import lib, ops

    if through_ops:
        ops.resize(src, dst, case.P, case.Hi, case.Wi, case.Ho, case.Wo, _mode(case), align_corners=case.align, channels_last=case.C > 0,
                   Cdim=case.C, scale_h=case.sf[0], scale_w=case.sf[1], backward=direction == "bwd")
        return
    a = lib.ResizeArgs(lib.ptr(src), lib.ptr(dst), case.P, case.Hi, case.Wi, case.Ho, case.Wo, _mode(case), int(case.align), int(case.C > 0),
                       case.C, case.sf[0], case.sf[1])
    lib.call("mvp_resize_aa_fwd" if case.mode == "aa" else "mvp_resize_bwd" if direction == "bwd" else "mvp_resize_fwd", a)


def _run(case, direction, dev, through_ops=False):
    """One direction of one case: launch twice into guarded NaN buffers, then compare element by element.  Returns (src, got), both
    planar on the CPU."""
    src = rr.make_input(case, "x" if direction == "fwd" else "g")
    H, W = (case.Ho, case.Wo) if direction == "fwd" else (case.Hi, case.Wi)
    n = case.planes * H * W
    s = (rr.to_cl(src, case.P, case.C) if case.C else src).contiguous().to(dev)
    (w1, d1), (w2, d2) = _guarded(n, dev), _guarded(n, dev)
    _launch(case, direction, s, d1, through_ops)
    _launch(case, direction, s, d2, through_ops)
    torch.cuda.synchronize()
    label = f"{case.id} {direction}"
    assert bool(torch.isfinite(d1).all()), f"{label}: an element of dst was not written, or NaN / inf was computed"
    assert _guards_intact(w1, n) and _guards_intact(w2, n), f"{label}: a write outside dst"
    assert torch.equal(w1, w2), f"{label}: two launches differ"
    got = d1.cpu()
    got = rr.from_cl(got.view(case.P, H, W, case.C)) if case.C else got.view(case.planes, H, W)
    ref, bnd = rr.reference(case, direction, src)
    err = (got.double() - ref).abs()
    ratio, where = rr.worst(err, bnd)
    print(f"\n[resize-elem] {label}: worst err/bound {ratio:.3f} at (plane, y, x) = {where}, err {float(err[where]):.3e}, bound {float(bnd[where]):.3e}, "
          f"rel-L2 {rr.rel_l2(got.double(), ref):.3e}")
    assert ratio <= 1.0, (f"{label}: |got - ref| = {float(err[where]):.3e} > bound {float(bnd[where]):.3e} at (plane, y, x) = {where} "
                          f"(got {float(got[where])!r}, ref {float(ref[where])!r})")
    return src, got


def _both(case, dev, **kw):
    return {d: _run(case, d, dev, **kw) for d in case.directions}


def _ids(group):
    return [c.id for c in rr.CASES if c.group == group]


# ------------------------------------------------------------------------------------------------ planar
@pytest.mark.parametrize("cid", _ids("a"))
def test_a_forward_planar_column_tiles(dev, cid):
    """resize_fwd_planar with cw_log2 = 0, 1, 2, 5, 7, 8, 8 for Wo = 1, 2, 3, 17, 128, 129, 300 (the smallest power of two >= Wo, capped
    at 256): rb = 256 >> cw_log2 rows per block from 256 down to 1, lanes past Wo idle (3, 17, 129), and at Wo = 300 > 256 a second
    pass of the ox += cw loop.  4 x 7 -> 5 x Wo, 3 planes: 15 rows, so one partly filled block whenever rb > 15."""
    _both(rr.BY_ID[cid], dev)


@pytest.mark.parametrize("cid", _ids("b"))
def test_b_forward_planar_second_trip(dev, cid):
    """Wo = 129 gives cw_log2 = 8, rb = 1 row per block; rows = 260 planes x 256 = 66560 > the 65536-block cap, so blocks 0 .. 1023
    take a second trip of the row loop (row += gridDim.x * rb) into planes 256 .. 259."""
    _both(rr.BY_ID[cid], dev)


@pytest.mark.parametrize("cid", _ids("c"))
def test_c_adjoint_rows_cached(dev, cid):
    """resize_bwd_planar_rows with every candidate window ny <= ADJ_ROWS = 64 (row weights in LDS): 20 x 28 -> 83 x 114, 3 x 300 ->
    7 x 700 and 83 x 114 -> 20 x 28 give ny % 4 = 0, 1, 2, 3 between them (the 4-row unrolled loop and its remainder), and 300 -> 700
    has Wo and Wi > 256, so both the row sweep (ox += 256) and the column sweep (ix += 256) loop."""
    _both(rr.BY_ID[cid], dev)


@pytest.mark.parametrize("cid", _ids("d"))
def test_d_adjoint_rows_uncached(dev, cid):
    """ny > ADJ_ROWS = 64: the row weights are recomputed per lane instead of read from LDS.  Bicubic 7 -> 112 rows has windows of
    42 / 58 (edge rows, cached) and 68 (inner rows, not) in one launch, 78 under align_corners; bilinear and nearest 4 -> 128 reach 87;
    bicubic 14 x 14 -> 224 x 224, the B/16 token grid to the image, has 68."""
    _both(rr.BY_ID[cid], dev)


@pytest.mark.parametrize("cid", _ids("e"))
def test_e_adjoint_rows_second_trip(dev, cid):
    """rows = 8200 planes x Hi 8 = 65600 > the 65536-block cap: blocks 0 .. 63 run a second trip and overwrite the LDS row weights
    and the row buffer of their first."""
    _both(rr.BY_ID[cid], dev)


@pytest.mark.parametrize("cid", _ids("f"))
def test_f_row_buffer_limit_and_fallback(dev, cid):
    """Wo = 8192 = ADJ_WO fills the LDS row buffer of resize_bwd_planar_rows to its last float; Wo = 8200 > ADJ_WO launches
    resize_bwd_planar instead (8 lanes per input element, candidate rows strided by 8, a shuffle reduction).  The forward of both
    runs 33 passes of the ox += 256 loop."""
    _both(rr.BY_ID[cid], dev)


@pytest.mark.parametrize("cid", _ids("g"))
def test_g_fallback_second_trip_and_tail(dev, cid):
    """resize_bwd_planar on 130 x 2050 = 266500 input elements: 8192 blocks x 32 elements = 262144 per sweep, so 4356 elements take a
    second trip, and 266500 is no multiple of 32 (nor of 8): the last block's groups of 8 lanes are partly past the end."""
    _both(rr.BY_ID[cid], dev)


# ------------------------------------------------------------------------------------------------ channels-last
@pytest.mark.parametrize("cid", _ids("h"))
def test_h_channels_last(dev, cid):
    """resize_fwd_cl / resize_bwd_cl with C4 = C / 4 = 1, 2 and 33 (one float4 per pixel; a non-power-of-two divisor).  Column windows
    of the adjoint: 5 x 7 -> 20 x 28 and 6 -> 30 (23 columns) stay within ADJ_MAXW = 24 registers; bicubic 6 -> 36 (28) and bilinear /
    nearest 4 -> 44 (25) do not and recompute the weights in the loop; 36 x 36 -> 6 x 6 has windows of 1 .. 3."""
    _both(rr.BY_ID[cid], dev)


@pytest.mark.parametrize("cid", _ids("i"))
def test_i_channels_last_second_trip(dev, cid):
    """260 x 260 x 128 channels = 2163200 float4 > 8192 blocks x 256 lanes = 2097152: the adjoint of 260 -> 130 and the forward of
    130 -> 260 each take a second trip of the float4 loop (the other direction of each case fits in one)."""
    _both(rr.BY_ID[cid], dev)


# ------------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("cid", _ids("j"))
def test_j_degenerate_axes(dev, cid):
    """Hi or Wi = 1 (every tap clamps onto index 0); Ho or Wo = 1, where align_corners makes the scale 0 and cand_range returns the
    whole axis; in == out, where bilinear and bicubic without align_corners must return the input bit for bit (weights exactly 1 and 0);
    12 x 40 -> 40 x 12, one axis up while the other goes down."""
    case = rr.BY_ID[cid]
    res = _both(case, dev)
    if (case.Hi, case.Wi) == (case.Ho, case.Wo) and not case.align:
        src, got = res["fwd"]
        assert torch.equal(got.view(torch.int32), src.view(torch.int32)), f"{cid}: in == out is not the identity"


@pytest.mark.parametrize("cid", _ids("k"))
def test_k_scale_factors_through_ops(dev, cid):
    """ops.resize with scale_h / scale_w given: 7 x 9 by 2.5 (-> 17 x 22, 1 / sf = 0.4 where in / out = 0.412 and 0.409), by
    (1.5, 0.5) (-> 10 x 4: 0.667 against 0.7, 2 against 2.25) and by 4.  align_corners ignores the factor."""
    _both(rr.BY_ID[cid], dev, through_ops=True)


@pytest.mark.parametrize("mode,align", [("nearest", None), ("bilinear", False), ("bilinear", True), ("bicubic", False)])
@pytest.mark.parametrize("sf", [2.5, (1.5, 0.5), 4])
def test_k_interpolate_wrapper(dev, mode, align, sf):
    """functional.interpolate: the output size is floor(in x sf), the factor reaches the kernel, fp16 and non-contiguous inputs are
    made contiguous fp32 first, and the gradient is the reference adjoint of the gradient that came in."""
    from mvp import functional as MF

    sfs = (float(sf), float(sf)) if not isinstance(sf, tuple) else sf
    case = rr.Case("k", 6, 7, 9, int(7 * sfs[0]), int(9 * sfs[1]), mode, bool(align), 0, sfs)
    kw = {} if align is None else dict(align_corners=align)
    wide = torch.zeros(2, 3, 7, 18)
    wide[..., ::2] = rr.make_input(case, "x").view(2, 3, 7, 9)
    x = wide.to(dev)[..., ::2]
    assert not x.is_contiguous()
    x.requires_grad_(True)
    out = MF.interpolate(x, scale_factor=sf, mode=mode, **kw)
    gy = rr.make_input(case, "g")
    out.backward(gy.view(out.shape).to(dev))
    torch.cuda.synchronize()
    assert tuple(out.shape) == (2, 3, case.Ho, case.Wo)
    for name, direction, got, src in (("out", "fwd", out.detach(), x.detach().cpu().flatten(0, 1)), ("grad", "bwd", x.grad, gy)):
        ref, bnd = rr.reference(case, direction, src)
        err = (got.cpu().flatten(0, 1).double() - ref).abs()
        ratio, where = rr.worst(err, bnd)
        print(f"\n[resize-elem] interpolate {case.id} {name}: worst err/bound {ratio:.3f} at (plane, y, x) = {where}")
        assert ratio <= 1.0, f"interpolate {case.id} {name}: {float(err[where]):.3e} > {float(bnd[where]):.3e} at (plane, y, x) = {where}"
    # fp16 in: the values the kernel sees are the fp16 values, exactly
    x16 = x.detach().half()
    out16 = MF.interpolate(x16, scale_factor=sf, mode=mode, **kw)
    torch.cuda.synchronize()
    ref, bnd = rr.reference(case, "fwd", x16.float().cpu().flatten(0, 1))
    ratio, where = rr.worst((out16.cpu().flatten(0, 1).double() - ref).abs(), bnd)
    assert out16.dtype == torch.float32 and ratio <= 1.0, f"interpolate fp16 {case.id}: ratio {ratio:.3f} at {where}"


@pytest.mark.parametrize("cid", _ids("l"))
def test_l_antialiased_forward(dev, cid):
    """resize_aa_fwd_planar: 530 x 300 -> 7 x 224 (windows of 151 rows x 3 columns, cut by the border at the first and last output);
    96 x 150 -> 1 x 64 (one output row whose window is the whole axis); 64 x 64 -> 64 x 64 (support 1, a single tap of weight 1: the
    identity, exact); 64 x 48 -> 96 x 20 (one axis up, where the filter is plain bilinear, the other down); 9 x 9 -> 2 x 2."""
    case = rr.BY_ID[cid]
    src, got = _both(case, dev)["fwd"]
    if (case.Hi, case.Wi) == (case.Ho, case.Wo):
        assert torch.equal(got.view(torch.int32), src.view(torch.int32)), f"{cid}: in == out is not the identity"


# ------------------------------------------------------------------------------------------------ argument checks
def _args(dev, **kw):
    from mvp import lib

    src = torch.ones(2 * 4 * 4 * 8, device=dev)
    whole, dst = _guarded(2 * 8 * 8 * 8, dev)
    f = dict(src=lib.ptr(src), dst=lib.ptr(dst), planes=2, Hi=4, Wi=4, Ho=8, Wo=8, mode=lib.RESIZE_BILINEAR, align_corners=0, channels_last=0,
             C=0, scale_h=0.0, scale_w=0.0)
    f.update(kw)
    return lib.ResizeArgs(*[f[name] for name, _ in lib.ResizeArgs._fields_]), src, whole


BAD = [dict(channels_last=1, C=6), dict(channels_last=1, C=0), dict(channels_last=1, C=-4), dict(mode=3), dict(mode=-1), dict(planes=0),
       dict(Hi=0), dict(Wi=0), dict(Ho=0), dict(Wo=0), dict(Wo=-1), dict(src=None), dict(dst=None)]
BAD_AA = [dict(align_corners=1), dict(channels_last=1, C=8), dict(scale_h=2.0), dict(scale_w=2.0), dict(mode=0), dict(mode=2)]


@pytest.mark.parametrize("fn,bad", [(f, b) for f in ("mvp_resize_fwd", "mvp_resize_bwd", "mvp_resize_aa_fwd") for b in BAD]
                         + [("mvp_resize_aa_fwd", b) for b in BAD_AA], ids=lambda v: v if isinstance(v, str) else ",".join(f"{k}={x}" for k, x in v.items()))
def test_m_argument_checks(dev, fn, bad):
    """validate(): MVP_EINVAL for a channel count that is no positive multiple of 4 under channels-last, an unknown mode, a dimension
    <= 0, a null src or dst; mvp_resize_aa_fwd also for align_corners, channels-last, a scale factor or a mode other than bilinear.
    Nothing is launched: dst keeps its prefill.  The same arguments without the fault are accepted."""
    from mvp import lib

    so = lib.load()
    good, src, whole = _args(dev)
    assert getattr(so, fn)(ctypes.byref(good), lib.stream_ptr()) == 0
    a, src2, whole2 = _args(dev, **bad)
    assert getattr(so, fn)(ctypes.byref(a), lib.stream_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert bool((whole2 == NAN_BITS).all()), "a refused call wrote to dst"
    assert _guards_intact(whole, 2 * 8 * 8 * 8)
