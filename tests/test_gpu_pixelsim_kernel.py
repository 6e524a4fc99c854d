"""mvp_pixel_score (csrc/pixelsim.hip) against the fp64 definition of tests/pixelsim_ref.py.

PSNR bound: |sim - psnr64| <= 2^-23 max(1, |psnr64|).  The kernel takes differences (exact), squares and sums in fp64, which leaves
about n 2^-53 relative on the mse and 4.3 n 2^-53 dB on the score; the one rounding to fp32 costs half an ulp, 2^-24 relative; the bound
leaves a factor 2.

SSIM bound, per case: max(4 e_ref, 4 x 2^-23), e_ref = the largest error against the fp64 definition of the SAME formula evaluated by
torch in fp32 (pixelsim_ref.ssim_fp32, the reference's own arithmetic) on the same inputs, computed here on the host.  4 is the
project's margin for a legitimately different summation order; the floor is that factor on one fp32 epsilon, for the cases where torch's
error happens to land near zero.

Measured on an MI355X (the maxima over the 120 cases of test_scores_predictions_and_counts): PSNR |err| <= 1.42e-6 dB = 0.46 x its
bound; SSIM |err| <= 2.98e-8 = 0.063 x its bound on noise and <= 1.70e-7 = 0.047 x its bound on smooth images (the kernel filters and
forms the map in fp64: what is left is the one rounding to fp32 and the window, which it applies separably where the reference's is
the fp32-rounded outer product), where the bounds are 4.8e-7 ... 2.3e-5.

Predictions are compared on every row; the fp64 margin between the near and the far side is asserted for every row (>= 1e-3 SSIM,
>= 1e-2 dB), so that no rounding within the bounds can turn a comparison.  The seeds of the inputs were chosen on the CPU with the
fp64 definition."""
import functools
import math

import pytest
import torch

import pixelsim_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 2.0 ** -23
MARGIN = {"ssim": 1e-3, "psnr": 1e-2}
TH, TW = 16, 32  # the SSIM tile of csrc/pixelsim.hip
# the issue's shapes, then this file's own: the tile size - 1, + 0, + 1 in each dimension (one tile exactly; one row / one column more
# starts a second tile that holds a single line of pixels)
SHAPES = [(1, 1, 1, 1), (2, 3, 5, 5), (2, 1, 6, 17), (2, 3, 11, 11), (1, 3, 12, 13), (3, 3, 33, 31), (2, 3, 64, 65), (2, 4, 40, 100),
          (2, 1, 7, 300), (1, 2, 130, 9),
          (1, 1, TH - 1, TW - 1), (1, 2, TH, TW), (1, 1, TH + 1, TW + 1), (1, 1, TH - 1, TW + 1), (1, 1, TH + 1, TW - 1)]
FAMILIES = ["noise", "smooth"]
SEED = {}  # (shape, family) -> seed, where seed 0 does not give every row its margin (none needed so far)


def q8(x):
    return (x.clamp(0.0, 1.0) * 255.0).round() / 255.0


def make_images(B, C, H, W, family, seed=0):
    """-> (ref, near, far) [B, C, H, W] fp32 on the 8-bit grid: near = clamp(ref + 0.03 n), far = clamp(ref + 0.15 n)."""
    g = torch.Generator().manual_seed(100000 * seed + 1000 * FAMILIES.index(family) + 131 * B + 31 * C + 7 * H + W)
    if family == "noise":
        r = torch.rand(B, C, H, W, generator=g)
    else:
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        ph = torch.rand(B, C, 1, 1, generator=g) * 6.28
        r = 0.5 + 0.3 * torch.sin(0.11 * xx + 0.07 * yy + ph) + 0.02 * torch.randn(B, C, H, W, generator=g)
    r = q8(r)
    n = torch.randn(B, C, H, W, generator=g)
    return r, q8(r + 0.03 * n), q8(r + 0.15 * n), g


@functools.lru_cache(maxsize=None)
def make_case(shape, family):
    """-> (ref, left, right, label [B], {metric: (sim64 [B, 2], pred64 [B], bound [B, 2])}).  The sides alternate per row."""
    B = shape[0]
    r, near, far, g = make_images(*shape, family, SEED.get((shape, family), 0))
    side = torch.arange(B) % 2 == 0  # True: left is the near one
    left = torch.where(side[:, None, None, None], near, far)
    right = torch.where(side[:, None, None, None], far, near)
    label = torch.randint(0, 2, (B,), generator=g).float()
    return r, left, right, label, {m: expected(r, left, right, m, side) for m in ("psnr", "ssim")}


def bounds(r, left, right, metric, sim64):
    if metric == "psnr":
        return EPS * sim64.abs().clamp_min(1.0)
    err = torch.stack([(ref.ssim_fp32(r, x).double() - sim64[:, k]).abs() for k, x in enumerate((left, right))])
    e_ref = float(err[torch.isfinite(err)].max())  # (a row with a NaN pixel has no error to speak of)
    return torch.full_like(sim64, max(4 * e_ref, 4 * EPS))


def expected(r, left, right, metric, side=None):
    sim64, pred64 = ref.score(r, left, right, metric)
    if side is not None:
        gap = torch.where(side, sim64[:, 0] - sim64[:, 1], sim64[:, 1] - sim64[:, 0])  # near minus far
        assert (gap >= MARGIN[metric]).all(), (metric, gap)  # every row: none is excused
        assert torch.equal(pred64, torch.where(side, 0, 1))
    return sim64, pred64, bounds(r, left, right, metric, sim64)


def run(r, left, right, metric, label=None, counts=None, accumulate=False, gap=0, one_allocation=True, shift=0):
    """One ABI call on [B, C, H, W] host tensors -> (sim [B, 2], pred [B]) on the host.  The three operands are slices of one
    [3B, ld] allocation (or three allocations), ld = C H W + gap with the gap filled with NaN; ``shift``: floats by which every base
    address is moved off its alignment."""
    from mvp import ops

    B, C, H, W = r.shape
    n = C * H * W
    ld = n + gap
    if one_allocation:
        buf = torch.full((3 * B * ld + shift,), math.nan, dtype=torch.float32, device=DEV)[shift:].view(3 * B, ld)
        parts = [buf[:B], buf[B:2 * B], buf[2 * B:]]
    else:
        parts = [torch.full((B * ld + shift,), math.nan, dtype=torch.float32, device=DEV)[shift:].view(B, ld) for _ in range(3)]
    for dst, src in zip(parts, (r, left, right)):
        dst[:, :n] = src.reshape(B, n).to(DEV)
    sim = torch.full((B, 2), -7.0, dtype=torch.float32, device=DEV)
    pred = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(max(1, ops.pixel_score_workspace_bytes(B, C, H, W, metric) // 8), dtype=torch.float64, device=DEV)
    ops.pixel_score(parts[0], parts[1], parts[2], sim, pred, ws, B, C, H, W, ld, metric, label=None if label is None else label.to(DEV),
                    counts=counts, accumulate=accumulate)
    return sim.cpu(), pred.cpu()


def ratio(sim, sim64, bound):
    """(largest error, largest error / bound) over the finite expected entries."""
    err = (sim.double() - sim64).abs()
    return float(err.max()), float((err / bound).max())


@pytest.mark.parametrize("gap", [0, 5])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("metric", ["psnr", "ssim"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_scores_predictions_and_counts(shape, metric, family, gap):
    r, left, right, label, want = make_case(shape, family)
    sim64, pred64, bound = want[metric]
    counts = torch.full((4,), -99, dtype=torch.int64, device=DEV)
    sim, pred = run(r, left, right, metric, label=label, counts=counts, gap=gap)
    err, rel = ratio(sim, sim64, bound)
    print(f"{metric} {family} (B, C, H, W) = {shape}, ld = C H W + {gap}: max |sim - sim64| = {err:.3e} = {rel:.3f} x bound "
          f"({float(bound.max()):.3e})")
    assert torch.isfinite(sim).all() and rel <= 1.0
    assert torch.equal(pred.long(), pred64)
    assert counts.cpu().tolist() == ref.counts(label, pred64)


@pytest.mark.parametrize("metric", ["psnr", "ssim"])
@pytest.mark.parametrize("shape", [(6, 3, 12, 13), (6, 1, 33, 31)], ids=lambda s: "x".join(map(str, s)))
def test_rows_with_chosen_content(shape, metric):
    """Row 0: left bitwise equal to right.  1: left bitwise equal to the reference image.  2: all three images zero.  3: a NaN pixel in
    left.  4: values scaled to [-2, 3] (nothing is clamped).  5: a plain row."""
    r, left, right, _, _ = make_case(shape, "smooth")
    r, left, right = r.clone(), left.clone(), right.clone()
    C, H, W = shape[1:]
    right[0] = left[0]
    left[1] = r[1]
    r[2], left[2], right[2] = 0.0, 0.0, 0.0
    left[3, C // 2, H - 1, W // 2] = math.nan
    for t in (r, left, right):
        t[4] = t[4] * 5.0 - 2.0
    assert float(r[4].min()) < -0.5 and float(r[4].max()) > 1.5  # x -> 5 x - 2 takes [0, 1] to [-2, 3]: well outside [0, 1]
    sim64, pred64, bound = expected(r, left, right, metric)
    plain = [4, 5]
    assert ((sim64[plain, 0] - sim64[plain, 1]).abs() >= MARGIN[metric]).all(), sim64
    sim, pred = run(r, left, right, metric)
    top = 1.0 if metric == "ssim" else math.inf
    assert sim[0, 0].view(torch.int32) == sim[0, 1].view(torch.int32) and pred[0] == 1
    assert abs(float(sim[0, 0]) - float(sim64[0, 0])) <= float(bound[0, 0])
    assert float(sim[1, 0]) == top and pred[1] == 0 and abs(float(sim[1, 1]) - float(sim64[1, 1])) <= float(bound[1, 1])
    assert float(sim[2, 0]) == top and float(sim[2, 1]) == top and pred[2] == 1
    assert math.isnan(float(sim[3, 0])) and pred[3] == 1 and abs(float(sim[3, 1]) - float(sim64[3, 1])) <= float(bound[3, 1])
    err, rel = ratio(sim[plain], sim64[plain], bound[plain])
    print(f"{metric} {shape}: max |sim - sim64| on the scaled / plain rows = {err:.3e} = {rel:.3f} x bound")
    assert torch.isfinite(sim[plain]).all() and rel <= 1.0
    assert torch.equal(pred[plain].long(), pred64[plain])


@pytest.mark.parametrize("metric", ["psnr", "ssim"])
def test_call_forms_give_the_same_bits(metric):
    """Three allocations against slices of one; every base address one float off its alignment (PSNR then takes dword loads);
    the same call twice."""
    for shape in [(2, 4, 40, 100), (3, 3, 33, 31)]:  # 16-byte loads at the first, never at the second (C H W = 3069)
        r, left, right, _, want = make_case(shape, "noise")
        a = run(r, left, right, metric)
        for other in (run(r, left, right, metric, one_allocation=False), run(r, left, right, metric, shift=1),
                      run(r, left, right, metric, one_allocation=False, shift=1, gap=5), run(r, left, right, metric)):
            assert torch.equal(a[0].view(torch.int32), other[0].view(torch.int32)) and torch.equal(a[1], other[1])
        assert torch.equal(a[1].long(), want[metric][1])


@pytest.mark.parametrize("metric", ["psnr", "ssim"])
def test_counts_accumulate_over_calls_and_need_a_label(metric):
    from mvp import lib

    cases = [make_case((3, 3, 33, 31), "noise"), make_case((2, 3, 5, 5), "smooth"), make_case((2, 4, 40, 100), "noise"),
             make_case((3, 3, 33, 31), "smooth")]
    counts = torch.full((4,), 12345, dtype=torch.int64, device=DEV)
    want = [0, 0, 0, 0]
    for i, (r, left, right, label, exp) in enumerate(cases):
        run(r, left, right, metric, label=label, counts=counts, accumulate=i > 0)  # the first call overwrites the sentinel
        want = [a + b for a, b in zip(want, ref.counts(label, exp[metric][1]))]
        assert counts.cpu().tolist() == want
    assert sum(want) == 10
    r, left, right, label, exp = cases[0]
    run(r, left, right, metric, label=label, counts=counts)  # without accumulate: overwritten
    assert counts.cpu().tolist() == ref.counts(label, exp[metric][1])
    sentinel = torch.full((4,), -5, dtype=torch.int64, device=DEV)
    with pytest.raises(lib.MvpError, match="invalid argument"):
        run(r, left, right, metric, label=None, counts=sentinel)
    assert sentinel.cpu().tolist() == [-5] * 4
