"""The ConvNeXt kernels (csrc/convnext.hip) against fp64, element by element, on the same fp32 inputs (tests/convnext_ref.py).

mvp_dwconv7_ln_fwd — the tolerance is measured, not chosen: the yardstick of a fixture is the maximum error of torch's own fp32 CPU
evaluation (F.conv2d(groups=C) + F.layer_norm) against fp64 on that fixture; the kernel's fp32 copy may err by at most 4 x that (another
summation order over 49 taps and C channels), the pair output by that plus 2^-16 relative (hi + lo carries a value to 2^-17).  Rows with
sigma below 1e-3 of their RMS are not in the random fixtures (tests/test_convnext_cpu.py checks the generator).  Every figure is printed
before it is asserted (pytest -s shows them; DESIGN.md §4 records one run).

mvp_grn_stats / mvp_grn_apply — G and N to 1e-6 relative (fp64 partial sums, one rounding to fp32, one fp32 divide); the applied output to
2^-16 of the magnitude of its terms |gamma h N| + |beta| + |h| (fp32 roundings of each term are relative to that term, and the pair adds 2^-17)."""
import pytest
import torch

import convnext_ref as R

pytestmark = pytest.mark.gpu

PAIR = 2.0 ** -16
MARGIN = 4.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _pair_value(hi, lo, f16=False):
    """fp64 value of a pair: bf16 hi + lo, or the compensated fp16 form hi + (lo - hi / 8) / 8 (include/mvp_hip.h)."""
    if f16:
        h, l = hi.view(torch.float16).double(), lo.view(torch.float16).double()
        return h + (l - h / 8.0) / 8.0
    return hi.double() + lo.double()


def _run_dwconv(dev, x, w, b, gamma, beta, Cdim, *, layout="separate", f16=False, want_f32=True, eps=R.EPS):
    """One launch on NaN-filled outputs -> (pair value fp64 [B, H, W, C] on the CPU, fp32 copy or None, raw output tensors)."""
    from mvp import ops

    B, H, W, ldx = x.shape
    M = B * H * W
    xd, wd, bd, gd, ed = (t.to(dev).contiguous() for t in (x, w, b, gamma, beta))
    nan16 = lambda *s: torch.full(s, float("nan"), dtype=torch.bfloat16, device=dev)  # noqa: E731
    f32 = torch.full((M, Cdim), float("nan"), dtype=torch.float32, device=dev) if want_f32 else None
    if layout == "ilv32":
        out = ops.IlvPair(M, Cdim, dev)
        out.t.fill_(float("nan"))
    else:
        out = (nan16(M, Cdim), nan16(M, Cdim))
    ops.dwconv7_ln(xd, wd, bd, gd, ed, out, B, H, W, Cdim, eps, ldx=ldx, out_f32=f32, out_f16=f16)
    torch.cuda.synchronize()
    raw = (out.t,) if layout == "ilv32" else out
    hi, lo = out.separate() if layout == "ilv32" else out
    val = _pair_value(hi.cpu(), lo.cpu(), f16).reshape(B, H, W, Cdim)
    return val, (f32.cpu().reshape(B, H, W, Cdim) if want_f32 else None), tuple(t.clone() for t in raw) + ((f32.clone(),) if want_f32 else ())


def _check(tag, val, f32, ref, yard, floor=0.0):
    """The two bounds of the module docstring; prints the figures first.  ``floor``: an absolute term for the fp16 pair form, whose halves
    have fp16's subnormal spacing (2^-24 below 6.1e-5): hi is then wrong by up to 2^-25 and lo / 8 repairs it to 2^-25 / 8."""
    assert torch.isfinite(val).all() and (f32 is None or torch.isfinite(f32).all()), tag
    e_pair = float(((val - ref).abs() - PAIR * ref.abs() - floor).max())
    line = f"[dwconv7_ln] {tag}: torch fp32 max err {yard:.3e}  tol {MARGIN * yard:.3e}  pair excess over 2^-16|ref| {e_pair:.3e}"
    if f32 is not None:
        e32 = float((f32.double() - ref).abs().max())
        gap = float((((val - f32.double()).abs() - floor).clamp_min(0.0) / f32.double().abs().clamp_min(1e-30)).max())
        line += f"  fp32 copy max err {e32:.3e}  pair vs copy max rel {gap:.3e}"
    print(line)
    assert e_pair <= MARGIN * yard, (tag, e_pair, yard)
    if f32 is not None:
        assert e32 <= MARGIN * yard, (tag, e32, yard)
        assert gap <= PAIR, (tag, gap)


@pytest.mark.parametrize("hw", R.DW_SIZES)
@pytest.mark.parametrize("Cdim", R.DW_CHANNELS)
def test_dwconv7_ln_against_fp64(dev, Cdim, hw):
    """Every channel count x map size, B = 2: pair + fp32 copy against fp64, and a second launch gives the same bits."""
    H, W = hw
    x, w, b, gamma, beta = R.dwconv_fixture(Cdim, H, W)
    ref, yard = R.dwconv_yardstick(x, w, b, gamma, beta)
    val, f32, raw = _run_dwconv(dev, x, w, b, gamma, beta, Cdim)
    _check(f"C={Cdim} {H}x{W}", val, f32, ref, yard)
    _, _, raw2 = _run_dwconv(dev, x, w, b, gamma, beta, Cdim)
    for a, c in zip(raw, raw2):
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32),
                           c.view(torch.int16) if c.dtype == torch.bfloat16 else c.view(torch.int32))


def test_dwconv7_ln_pixel_stride_beyond_c(dev):
    """ldx > C: the filler columns (NaN here) are never read into a result."""
    x, w, b, gamma, beta = R.dwconv_fixture(64, 9, 13, ldx=80)
    x[..., 64:] = float("nan")
    ref, yard = R.dwconv_yardstick(x, w, b, gamma, beta)
    val, f32, _ = _run_dwconv(dev, x, w, b, gamma, beta, 64)
    _check("C=64 9x13 ldx=80", val, f32, ref, yard)


@pytest.mark.parametrize("form", ["ilv32", "f16", "pair_only", "f32_only"])
def test_dwconv7_ln_output_forms(dev, form):
    """The interleaved layout, the compensated fp16 pair (2^-16 holds for it as well: hi carries 11 bits, lo / 8 the next 11; plus
    2^-28 absolute for elements in fp16's subnormal range), and each output alone — the same bounds."""
    from mvp import ops

    Cdim, H, W = 192, 9, 13
    x, w, b, gamma, beta = R.dwconv_fixture(Cdim, H, W, seed=1)
    ref, yard = R.dwconv_yardstick(x, w, b, gamma, beta)
    if form == "f32_only":
        f32 = torch.full((2 * H * W, Cdim), float("nan"), dtype=torch.float32, device=dev)
        ops.dwconv7_ln(*(t.to(dev) for t in (x, w, b, gamma, beta)), None, 2, H, W, Cdim, R.EPS, out_f32=f32)
        e32 = float((f32.cpu().double().reshape(ref.shape) - ref).abs().max())
        print(f"[dwconv7_ln] f32 only: max err {e32:.3e}  tol {MARGIN * yard:.3e}")
        assert e32 <= MARGIN * yard
        return
    val, f32, _ = _run_dwconv(dev, x, w, b, gamma, beta, Cdim, layout="ilv32" if form == "ilv32" else "separate", f16=form == "f16",
                              want_f32=form != "pair_only")
    _check(f"C={Cdim} {H}x{W} {form}", val, f32, ref, yard, floor=2.0 ** -28 if form == "f16" else 0.0)


@pytest.mark.parametrize("Cdim,hw", [(64, (3, 5)), (192, (7, 7)), (1024, (1, 2))])
def test_dwconv7_ln_images_do_not_leak(dev, Cdim, hw):
    """Image 1 holds values 1e4 times those of image 0: image 0 of the B = 2 result equals the B = 1 result bit for bit (row H - 1 of
    image 0 never reads row 0 of image 1)."""
    H, W = hw
    x, w, b, gamma, beta = R.dwconv_fixture(Cdim, H, W, B=1, seed=2)
    x2 = torch.cat([x, x * 1e4], dim=0)
    _, f1, raw1 = _run_dwconv(dev, x, w, b, gamma, beta, Cdim)
    _, f2, raw2 = _run_dwconv(dev, x2, w, b, gamma, beta, Cdim)
    M = H * W
    for a, c in zip(raw1, raw2):
        ai, ci = (t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) for t in (a, c))
        assert torch.equal(ai, ci[:M]), (Cdim, hw)
    ref, yard = R.dwconv_yardstick(x, w, b, gamma, beta)
    assert float((f1.double() - ref).abs().max()) <= MARGIN * yard


@pytest.mark.parametrize("Cdim", [32, 192, 1536])
def test_dwconv7_ln_constant_rows(dev, Cdim):
    """All channels and taps equal (dyadic values, so every sum is exact in fp32 and in torch's evaluation alike): the variance is 0 and the
    output is beta to within the tolerance, with no NaN."""
    B, H, W = 2, 5, 9
    x = torch.full((B, H, W, Cdim), 0.5)
    w = torch.full((Cdim, 7, 7), 0.125)
    b = torch.full((Cdim,), 0.25)
    g = torch.Generator().manual_seed(Cdim)
    gamma, beta = 0.5 + torch.rand(Cdim, generator=g), torch.randn(Cdim, generator=g)
    ref, yard = R.dwconv_yardstick(x, w, b, gamma, beta)
    assert float((ref - beta.double()).abs().max()) < 1e-12
    val, f32, _ = _run_dwconv(dev, x, w, b, gamma, beta, Cdim)
    want = beta.double().expand_as(ref)
    _check(f"C={Cdim} constant rows", val, f32, want, yard)


# ------------------------------------------------------------------------------------------------ GRN
@pytest.mark.parametrize("HW,C4", [(2, 256), (15, 768), (200, 4096)])
def test_grn_stats_and_apply(dev, HW, C4):
    from mvp import ops

    B = 3
    g = torch.Generator().manual_seed(HW * 7 + C4)
    h = torch.randn(B, HW, C4, generator=g) * (0.5 + torch.rand(C4, generator=g) * 2.0)
    h[1] = 0.0  # an all-zero image: finite through the + 1e-6
    gamma, beta = torch.randn(C4, generator=g), torch.randn(C4, generator=g)
    Gr, Nr = R.grn_stats(h)
    ref = R.grn_apply(h, Nr, gamma, beta)
    scale = (gamma.double() * (h.double() * Nr[:, None, :])).abs() + beta.double().abs() + h.double().abs()
    hd, gd, bd = h.to(dev), gamma.to(dev), beta.to(dev)
    runs = []
    for _ in range(2):
        G = torch.full((B, C4), float("nan"), device=dev)
        N = torch.full((B, C4), float("nan"), device=dev)
        ws = torch.full((ops.grn_workspace_bytes(B, HW, C4) // 8,), float("nan"), dtype=torch.float64, device=dev)
        out = (torch.full((B * HW, C4), float("nan"), dtype=torch.bfloat16, device=dev), torch.full((B * HW, C4), float("nan"), dtype=torch.bfloat16, device=dev))
        f32 = torch.full((B * HW, C4), float("nan"), device=dev)
        ops.grn_stats(hd, G, N, ws, B, HW, C4)
        ops.grn_apply(hd, N, gd, bd, out, B, HW, C4, out_f32=f32)  # (no host synchronisation in between)
        torch.cuda.synchronize()
        runs.append((G.cpu(), N.cpu(), out[0].cpu(), out[1].cpu(), f32.cpu()))
    G, N, hi, lo, f32 = runs[0]
    for t in (G, N, hi.float(), lo.float(), f32):
        assert torch.isfinite(t).all()
    eG = float(((G.double() - Gr).abs() / Gr.clamp_min(1e-300)).max())
    eN = float(((N.double() - Nr).abs() / Nr.clamp_min(1e-300)).max())
    val = (hi.double() + lo.double()).reshape(B, HW, C4)
    eo = float(((val - ref).abs() / scale.clamp_min(1e-300)).max())
    e32 = float(((f32.double().reshape(B, HW, C4) - ref).abs() / scale.clamp_min(1e-300)).max())
    print(f"[grn] HW={HW} C4={C4}: G max rel {eG:.3e}  N max rel {eN:.3e}  applied pair / fp32, relative to the terms: {eo:.3e} / {e32:.3e}")
    assert float(G[1].abs().max()) == 0.0 and float(N[1].abs().max()) == 0.0
    assert torch.equal(f32.reshape(B, HW, C4)[1], beta.expand(HW, C4))  # gamma (0 * 0) + beta + 0
    assert eG <= 1e-6 and eN <= 1e-6
    assert eo <= PAIR and e32 <= PAIR
    for a, c in zip(runs[0], runs[1]):
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32),
                           c.view(torch.int16) if c.dtype == torch.bfloat16 else c.view(torch.int32))


def test_grn_apply_interleaved_layout(dev):
    from mvp import ops

    B, HW, C4 = 2, 15, 256
    g = torch.Generator().manual_seed(5)
    h, gamma, beta = torch.randn(B, HW, C4, generator=g), torch.randn(C4, generator=g), torch.randn(C4, generator=g)
    hd = h.to(dev)
    G, N = torch.empty(B, C4, device=dev), torch.empty(B, C4, device=dev)
    ws = torch.empty(ops.grn_workspace_bytes(B, HW, C4) // 8, dtype=torch.float64, device=dev)
    ops.grn_stats(hd, G, N, ws, B, HW, C4)
    sep = ops.empty_pair((B * HW, C4), 3, dev)
    ilv = ops.IlvPair(B * HW, C4, dev)
    ops.grn_apply(hd, N, gamma.to(dev), beta.to(dev), sep, B, HW, C4)
    ops.grn_apply(hd, N, gamma.to(dev), beta.to(dev), ilv, B, HW, C4)
    hi, lo = ilv.separate()
    assert torch.equal(hi.view(torch.int16), sep[0].view(torch.int16)) and torch.equal(lo.view(torch.int16), sep[1].view(torch.int16))
