"""mvp_twoafc_score (csrc/twoafc.hip) against the fp64 definition of tests/twoafc_ref.py.

Bound: |sim - sim64| <= 2^-23 absolute.  The kernel's fp64 chain (pooled sums, dot products, squared norms, square roots, division)
is off by at most about n * 2^-53 relative to |a| |b| for n <= 2^24 terms, i.e. below 2^-29 of a value of magnitude <= 1; the single
rounding of that value to fp32 adds at most 2^-25.  The sum is below 2^-24; the bound leaves a factor 2 on top.

Predictions are compared on every row whose fp64 similarities differ by at least 1e-3 (asserted for every row outside the chosen tie
rows: the inputs are built that way), where a 2^-23 error cannot turn the comparison."""
import functools
import math

import pytest
import torch

import twoafc_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BOUND = 2.0 ** -23
MARGIN = 1e-3
# the issue's shapes, then this file's own: three that cut the channels into several chunks (a ragged last chunk, the class-token
# form, the 16-byte form) and three whose rows are long enough for 32 and 64 lanes per row (the issue's stop at 16) and for more than
# one full pass per lane
SHAPES = [(1, 1, 1), (3, 63, 1), (2, 64, 1), (2, 65, 1), (16, 768, 1), (5, 1024, 1),
          (1, 1, 4), (3, 65, 49), (17, 130, 4), (2, 2048, 225), (2, 7, 3),
          (3, 300, 49), (2, 8200, 1), (2, 600, 64),
          (2, 5, 300), (2, 3, 1001), (1, 2, 4100)]


@functools.lru_cache(maxsize=None)
def make_case(B, C, HW, seed=0):
    """-> (ref, left, right [B, C, HW] fp32, label [B], sim64 [B, 2], pred64 [B]).  One side is the reference image scaled per channel
    row by 1 + 0.3 u (plus noise when there are enough channels to carry it), the other the NEGATED image scaled by 0.5 + u (plus
    noise): similarities near +1 and below 0.9, also for C = 1, where a cosine can only be +-1."""
    g = torch.Generator().manual_seed(1000 * seed + 31 * B + 7 * C + HW)
    r = torch.randn(B, C, HW, generator=g)
    n_close = 0.2 if C >= 16 else 0.0
    n_far = 0.5 if C >= 16 else (0.3 if C > 1 else 0.0)
    close = r * (1 + 0.3 * torch.rand(B, C, 1, generator=g)) + n_close * torch.randn(B, C, HW, generator=g)
    far = -r * (0.5 + torch.rand(B, C, 1, generator=g)) + n_far * torch.randn(B, C, HW, generator=g)
    side = (torch.arange(B) + seed) % 2 == 0  # True: left is the close one
    left = torch.where(side[:, None, None], close, far)
    right = torch.where(side[:, None, None], far, close)
    label = torch.randint(0, 2, (B,), generator=g).float()
    sim64, pred64 = ref.score(r, left, right)
    assert ((sim64[:, 0] - sim64[:, 1]).abs() >= MARGIN).all(), sim64  # every row: none is excused
    assert torch.equal(pred64, torch.where(side, 0, 1))
    return r, left, right, label, sim64, pred64


def run(r, left, right, label=None, counts=None, accumulate=False, gap=0, one_allocation=True):
    """One ABI call on [B, C, HW] host tensors -> (sim [B, 2], pred [B]) on the host.  The three operands are slices of one
    [3B, ld] allocation (or three allocations), ld = C * HW + gap with the gap filled with NaN."""
    from mvp import ops

    B, C, HW = r.shape
    ld = C * HW + gap
    if one_allocation:
        buf = torch.full((3 * B, ld), math.nan, dtype=torch.float32, device=DEV)
        parts = [buf[:B], buf[B:2 * B], buf[2 * B:]]
    else:
        parts = [torch.full((B, ld), math.nan, dtype=torch.float32, device=DEV) for _ in range(3)]
    for dst, src in zip(parts, (r, left, right)):
        dst[:, :C * HW] = src.reshape(B, C * HW).to(DEV)
    sim = torch.full((B, 2), -7.0, dtype=torch.float32, device=DEV)
    pred = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(max(1, ops.twoafc_workspace_bytes(B, C, HW) // 8), dtype=torch.float64, device=DEV)
    ops.twoafc_score(parts[0], parts[1], parts[2], sim, pred, ws, B, C, HW, ld, label=None if label is None else label.to(DEV),
                     counts=counts, accumulate=accumulate)
    return sim.cpu(), pred.cpu()


@pytest.mark.parametrize("gap", [0, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_similarities_predictions_and_counts(shape, gap):
    r, left, right, label, sim64, pred64 = make_case(*shape)
    counts = torch.full((4,), -99, dtype=torch.int64, device=DEV)
    sim, pred = run(r, left, right, label=label, counts=counts, gap=gap)
    err = float((sim.double() - sim64).abs().max())
    print(f"(B, C, HW) = {shape}, ld = C HW + {gap}: max |sim - sim64| = {err:.3e} = {err / BOUND:.3f} x 2^-23")
    assert torch.isfinite(sim).all() and err <= BOUND
    assert torch.equal(pred.long(), pred64)
    assert counts.cpu().tolist() == ref.counts(label, pred64)


def test_three_allocations_equal_slices_of_one():
    r, left, right, label, _, _ = make_case(3, 65, 49)
    a = run(r, left, right, one_allocation=True)
    b = run(r, left, right, one_allocation=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("C,HW", [(65, 1), (33, 5), (40, 4)])
def test_rows_with_chosen_content(C, HW):
    """Row 0: left bitwise equal to right.  1: an all-zero reference.  2: pooled norms of 5e-9, below both clamps.  3: entries near 1e18
    (fp32 squares would be inf).  4: a NaN in left.  5: a plain row."""
    r, left, right, _, _, _ = (t.clone() if t.dim() == 3 else t for t in make_case(6, C, HW, seed=3))
    right[0] = left[0]
    r[1] = 0.0
    for t in (r, left, right):
        t[2] *= (5e-9 / ref.pool(t[2:3]).norm()).float()
        t[3] *= 1e18
    left[4, C // 2, HW - 1] = math.nan
    sim64, pred64 = ref.score(r, left, right)
    plain = [2, 3, 5]
    assert all(float(ref.pool(t[2:3]).norm()) < 1e-8 for t in (r, left, right))
    assert ((sim64[plain, 0] - sim64[plain, 1]).abs() >= MARGIN).all(), sim64
    sim, pred = run(r, left, right)
    assert sim[0, 0].view(torch.int32) == sim[0, 1].view(torch.int32) and pred[0] == 1 and abs(float(sim[0, 0]) - float(sim64[0, 0])) <= BOUND
    assert sim[1, 0] == 0.0 and sim[1, 1] == 0.0 and pred[1] == 1
    assert math.isnan(float(sim[4, 0])) and pred[4] == 1 and abs(float(sim[4, 1]) - float(sim64[4, 1])) <= BOUND
    err = float((sim[plain].double() - sim64[plain]).abs().max())
    print(f"C = {C}, HW = {HW}: max |sim - sim64| on the tiny / 1e18 / plain rows = {err:.3e} = {err / BOUND:.3f} x 2^-23")
    assert torch.isfinite(sim[plain]).all() and err <= BOUND
    assert torch.equal(pred[plain].long(), pred64[plain])


def test_counts_accumulate_over_calls_and_need_a_label():
    from mvp import lib

    cases = [make_case(17, 130, 4), make_case(5, 1024, 1), make_case(3, 65, 49)]
    counts = torch.full((4,), 12345, dtype=torch.int64, device=DEV)
    want = [0, 0, 0, 0]
    for i, (r, left, right, label, _, pred64) in enumerate(cases):
        run(r, left, right, label=label, counts=counts, accumulate=i > 0)  # the first call overwrites the sentinel
        want = [a + b for a, b in zip(want, ref.counts(label, pred64))]
        assert counts.cpu().tolist() == want
    assert sum(want) == 25 and min(want) > 0  # every one of TP, FP, FN, TN occurs
    # no label: counts may not be passed (MVP_EINVAL before anything is launched) and what it holds stays
    r, left, right, _, sim64, pred64 = cases[2]
    sentinel = torch.full((4,), -5, dtype=torch.int64, device=DEV)
    with pytest.raises(lib.MvpError, match="invalid argument"):
        run(r, left, right, label=None, counts=sentinel)
    sim, pred = run(r, left, right, label=None, counts=None)
    assert sentinel.cpu().tolist() == [-5] * 4 and counts.cpu().tolist() == want
    assert torch.equal(pred.long(), pred64) and float((sim.double() - sim64).abs().max()) <= BOUND


def test_two_calls_give_the_same_bits():
    r, left, right, label, _, _ = make_case(2, 2048, 225)
    a = run(r, left, right, gap=5)
    b = run(r, left, right, gap=5)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
