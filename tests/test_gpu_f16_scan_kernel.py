"""mvp_f16_range_scan against its CPU restatement (tests/f16_scan_ref.py), all four words with exact equality: both layouts, row
strides with a gap, a column window inside a wider array, every planted content, accumulation into one record and run-to-run
repeatability.  Everything the kernel must not read — the gap columns, the lo blocks of the interleaved layout, the columns beside
the window — is filled with saturated and NaN bits, so a stray read shows in every word."""
import functools

import pytest
import torch

from f16_scan_ref import ilv32, scan_record

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8), (1, 32), (3, 96), (64, 64), (257, 160), (1, 3072), (5, 4096), (70001, 32)]  # 70 001 rows: more than the grid cap
CONTENTS = ["clean", "first", "last", "col7_col8", "neg_sat", "below_sat", "inf_nan", "all_sat"]
PAD = 24  # gap columns behind the window (ld = cols + 24)
SAT, NSAT, BELOW, INF, NINF, NAN = 0x7BFF, 0xFBFF - 0x10000, 0x7BFE, 0x7C00, 0xFC00 - 0x10000, 0x7E00


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _hi(rows, cols, content):
    """The hi words [rows, cols] as int16 on the CPU: fp16 noise of N(0, 30^2) (far inside the range), then the plants.  Built once per
    case, shared, never modified."""
    g = torch.Generator().manual_seed(7 * rows + cols)
    hi = (torch.randn(rows, cols, generator=g) * 30.0).half().view(torch.int16).clone()
    if content == "first":
        hi[0, 0] = SAT
    elif content == "last":
        hi[rows - 1, cols - 1] = SAT
    elif content == "col7_col8":  # across a 16-byte vector boundary (a 1 x 8 problem has column 7 only)
        hi[0, 7] = SAT
        if cols > 8:
            hi[rows - 1, 8] = NAN
    elif content == "neg_sat":
        hi[rows // 2, cols // 2] = NSAT
    elif content == "below_sat":  # 65472: the largest finite value that is NOT flagged
        hi[rows // 2, cols - 1] = BELOW
    elif content == "inf_nan":
        hi[0, cols - 1] = INF
        hi[rows - 1, 0] = NAN
        hi[rows // 2, cols // 2] = NINF
    elif content == "all_sat":
        hi[:] = SAT
        hi[:, 1::2] = NSAT
    return hi


def _poison(rows, cols):
    """What surrounds the scanned words: alternating saturated and NaN bits."""
    t = torch.full((rows, cols), SAT, dtype=torch.int16)
    t[:, 1::2] = NAN
    return t


def _stored(hi, layout, pad, left=0):
    """(array as stored, col0) for the window ``hi``: ``left`` poisoned pair columns in front of it, ``pad`` behind it; separate: the
    hi array alone (row stride left + cols + pad), interleaved: hi | lo per 32 columns with poisoned lo blocks and 2 * pad poisoned
    words at the end of every row (row stride 2 (left + cols) + 2 pad)."""
    rows, cols = hi.shape
    wide = torch.cat([_poison(rows, left), hi], dim=1) if left else hi
    if layout == "separate":
        return torch.cat([wide, _poison(rows, pad)], dim=1).contiguous() if pad else wide.contiguous(), left
    t = ilv32(wide, _poison(rows, left + cols))
    return (torch.cat([t, _poison(rows, 2 * pad)], dim=1).contiguous() if pad else t), left


def _run(dev, stored, layout, rows, cols, col0, record=None):
    from mvp import ops

    t = stored.to(dev).view(torch.bfloat16)
    if layout == "ilv":
        pair = ops.IlvPair.__new__(ops.IlvPair)  # an interleaved pair over the test's own array (row stride = its width)
        pair.rows, pair.cols, pair.t = rows, t.shape[1] // 2, t
    else:
        pair = (t, None)
    if record is None:
        record = torch.zeros(4, dtype=torch.int32, device=dev).view(torch.uint32)
    ops.f16_range_scan(pair, rows, cols, record, col0=col0)
    return record


def _words(record):
    return (record.view(torch.int32).cpu().to(torch.int64) & 0xFFFFFFFF).tolist()


CASES = [(r, c, layout, pad) for r, c in SHAPES for layout in ("separate", "ilv") for pad in (0, PAD) if layout == "separate" or c % 32 == 0]


@pytest.mark.parametrize("rows, cols, layout, pad", CASES)
def test_record_matches_the_restatement(dev, rows, cols, layout, pad):
    """Every content of one (shape, layout, ld): the four words are the restatement's, n_scanned == rows * cols, and the poisoned
    surroundings appear in no word (clean noise gives n_sat == n_nonfinite == 0 and a maximum below 0x7BFF)."""
    for content in CONTENTS:
        hi = _hi(rows, cols, content)
        stored, col0 = _stored(hi, layout, pad)
        got = _words(_run(dev, stored, layout, rows, cols, col0))
        want = scan_record(hi)
        assert want[3] == rows * cols
        if content == "clean":
            assert want[1] == want[2] == 0 and 0 < want[0] < SAT
        if content == "below_sat":
            assert want[:3] == [BELOW, 0, 0]
        if content == "all_sat":
            assert want[:3] == [SAT, rows * cols, 0]
        assert got == want, (content, got, want)


@pytest.mark.parametrize("layout", ["separate", "ilv"])
@pytest.mark.parametrize("rows, cols", [(3, 96), (257, 160), (5, 4096)])
def test_window_inside_a_wider_array(dev, rows, cols, layout):
    """col0 = 64: the window starts two interleave blocks into rows whose first 64 and last 24 pair columns are poisoned."""
    for content in ("clean", "first", "last", "inf_nan"):
        hi = _hi(rows, cols, content)
        stored, col0 = _stored(hi, layout, PAD, left=64)
        assert col0 == 64
        assert _words(_run(dev, stored, layout, rows, cols, col0)) == scan_record(hi), content


def test_q_k_window_of_a_wider_pair(dev):
    """The Q / K site: the first 2C columns of a [M, 3C] array, whose V third is poisoned."""
    M, C = 50, 128
    hi = _hi(M, 2 * C, "last")
    stored = torch.cat([hi, _poison(M, C)], dim=1).contiguous()
    assert _words(_run(dev, stored, "separate", M, 2 * C, 0)) == scan_record(hi)


@pytest.mark.parametrize("layout", ["separate", "ilv"])
def test_two_launches_accumulate_and_a_second_run_repeats(dev, layout):
    a, b = _hi(257, 160, "inf_nan"), _hi(64, 64, "all_sat")
    recs = []
    for _ in range(2):
        rec = _run(dev, _stored(a, layout, PAD)[0], layout, 257, 160, 0)
        first = _words(rec)
        rec = _run(dev, _stored(b, layout, 0)[0], layout, 64, 64, 0, record=rec)
        assert first == scan_record(a)
        recs.append(_words(rec))
    assert recs[0] == scan_record(b, accumulate=scan_record(a))
    assert recs[0] == recs[1]
    big = _hi(70001, 32, "all_sat")  # every workgroup adds to every word: the atomics' arrival order does not show
    st = _stored(big, layout, PAD)[0]
    assert _words(_run(dev, st, layout, 70001, 32, 0)) == _words(_run(dev, st, layout, 70001, 32, 0)) == scan_record(big)


def test_wrapper_refuses_windows_outside_the_operand(dev):
    from mvp import lib, ops

    t = torch.zeros(4, 64, dtype=torch.bfloat16, device=dev)
    rec = torch.zeros(4, dtype=torch.int32, device=dev).view(torch.uint32)
    for rows, cols, col0 in ((5, 64, 0), (4, 72, 0), (4, 32, 40), (4, 12, 0)):
        with pytest.raises(lib.MvpError):
            ops.f16_range_scan((t, None), rows, cols, rec, col0=col0)
    assert _words(rec) == [0, 0, 0, 0]
