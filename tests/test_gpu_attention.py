"""The attention kernels (csrc/attention.hip) against fp64, one query row at a time (tests/attention_ref.py has the reference, the
rounding model and the budget derived from it):

  a  token counts at which the LAST tile's code changes shape, both sides of the resident / streaming switch, a full last streaming tile
  b  the persistent ring of the resident kernel: every slot offset, a wrap, unequal pair counts per workgroup — against fp64 and,
     bit for bit, against two-image launches of the same rows
  c  padded strides (ld_qkv, ld_out) with guard columns and rows
  d  out_f16 = 1, separate and interleaved; the argument checks
  e  the softmax's range: uniform rows, one dominant key in the first / last tile, a one-hot row, maxima that climb just under and
     just over the deferral threshold tile after tile; scales other than 1/8

Every output is prefilled with NaN bit patterns, and every bound is computed from the reference: 4 x the model's worst row error plus
2^-22 x the largest exponent argument, with the whole-tensor bounds of test_attention kept as caps."""
import ctypes

import pytest
import torch

import attention_ref as ar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _prec(form):
    from mvp import lib

    return lib.PREC_BF16 if form == "bf16" else lib.PREC_BF16X3


def _pack(qkv, C, form):
    from mvp import ops

    return ar.pack(qkv, C, form, split=ops.split_bf16)


def _nan_pair(rows, cols, dev):
    hi = torch.full((rows, cols), float("nan"), dtype=torch.bfloat16, device=dev)
    return hi, hi.clone()


def _attend(qp, out, B, N, H, scale, form, **kw):
    from mvp import ops

    ops.attention(qp, out, B, N, H, scale, _prec(form), v_f16="_vf16" in form, qk_f16=form.endswith("_qk16"), **kw)
    torch.cuda.synchronize()


def _launch(qp, B, N, H, scale, form, dev):
    """One dense launch into a NaN-filled bf16 pair -> (hi, lo)."""
    out = _nan_pair(B * N, H * 64, dev)
    _attend(qp, out, B, N, H, scale, form)
    return out


def _pair_value(out):
    return out[0].double() + out[1].double()


def _check(case, got_rows, label, extra=0.0):
    """Per-row bound (+ ``extra``) and whole-tensor cap of one case; prints the figures, names the worst (b, h, q)."""
    got = ar.heads(got_rows, case.B, case.N, case.H)
    assert bool(torch.isfinite(got).all()), f"{label}: non-finite output (an element was not written, or NaN / inf was computed)"
    err = ar.row_err(got, case.ref, case.v)
    e, where = ar.worst(err)
    me, mwhere = ar.worst(case.model_err)
    whole = ar.rel_l2(got, case.ref)
    print(f"\n[attn-row] {label}: model {me:.3e} at {mwhere}, kernel {e:.3e} at (b, h, q) = {where}, bound {case.bound + extra:.3e}, "
          f"max exp2 arg {float(case.smax.max()):.1f}, rel-L2 {whole:.3e}")
    assert e <= case.bound + extra, f"{label}: row error {e:.3e} > bound {case.bound + extra:.3e} at (b, h, q) = {where} (model {me:.3e})"
    assert whole < ar.CAPS[case.form], f"{label}: rel-L2 {whole:.3e} over the whole tensor, cap {ar.CAPS[case.form]:.0e}; worst row (b, h, q) = {where}"
    return err


def _randn(shape, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(shape, generator=g, device=dev, dtype=torch.float32)


def _head_view(x, B, N, H):
    """ar.heads of a column slice, as a view to write through."""
    v = ar.heads(x, B, N, H)
    assert v.data_ptr() == x.data_ptr()
    return v


def _sentinel(rows, cols, dev, salt):
    """A bf16-typed array holding an int16 pattern that no kernel would write by accident."""
    i = torch.arange(rows * cols, device=dev, dtype=torch.int64)
    return ((i * 40503 + salt) % 65536 - 32768).to(torch.int16).view(rows, cols).view(torch.bfloat16)


def _bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ a. token-count edges
EDGE_N = [1, 15, 16, 17, 32, 33, 48, 49, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256, 257, 383, 384, 385]


@pytest.mark.parametrize("form", ar.FORMS)
@pytest.mark.parametrize("N", EDGE_N)
def test_token_count_edges_per_row_vs_fp64(dev, form, N):
    """nsub = min(4, (N - key0 + 15) >> 4) at every value, the skipped P.V halves, the key mask at the first and last key of a 16-key
    sub-tile, 255 / 256 (resident) against 257 (streaming), a full last streaming tile (384).  V of image b, head h is scaled and
    offset differently, so a read across an image or head boundary is a gross row error."""
    B, H = 2, 2
    C = H * 64
    qkv = _randn((B * N, 3 * C), 1000 + N, dev)
    qkv[:, :C] *= 2.0
    v = _head_view(qkv[:, 2 * C:], B, N, H)
    for b in range(B):
        for h in range(H):
            v[b, h] = v[b, h] * ((1 + b) * (1 + h)) + (3 * b + 5 * h)
    qp = _pack(qkv, C, form)
    case = ar.reference(qp, B, N, H, 0.125, form)
    out = _launch(qp, B, N, H, 0.125, form, dev)
    _check(case, _pair_value(out), f"a edges {form} N={N}")


# ------------------------------------------------------------------------------------------------ b. persistent ring
RING = [(f, n) for f in ("bf16x3", "bf16x3_vf16_qk16") for n in (40, 70, 150, 193)] + [("bf16", 40), ("bf16", 70)]


@pytest.mark.parametrize("form,N", RING, ids=[f"{f}-N{n}" for f, n in RING])
def test_persistent_ring_every_slot_and_wrap(dev, form, N):
    """B * H >= (nkt + 2) * cu_count * per_cu + 3 pairs (the first multiple of H = 3 there: the count itself is one only where
    (nkt + 2) * cu_count * per_cu is): every workgroup walks nkt + 2 or nkt + 3 pairs, so every s0 = (nkt * i) % (nkt + 1) occurs and
    wraps, and the workgroups end after unequal counts.  Every pair against fp64; the first and last two images bit-identical to a
    two-image launch, where no pair is computed by a ring iteration i >= 1."""
    from mvp import lib

    H, nkt = 3, ar.nkt_of(N)
    C = H * 64
    cus = int(lib.info().cu_count)
    assert cus > 0
    pairs = ar.ring_pairs(nkt, form, cus)
    B = -(-pairs // H)
    assert B * H >= pairs and B * H % (cus * ar.per_cu(nkt, form)) != 0 and B * H // (cus * ar.per_cu(nkt, form)) == nkt + 2
    qkv = _randn((B * N, 3 * C), 2000 + N, dev)
    qkv[:, :C] *= 2.0
    qp = _pack(qkv, C, form)
    del qkv
    out = _launch(qp, B, N, H, 0.125, form, dev)
    for name, r0 in (("first", 0), ("last", (B - 2) * N)):
        sub = tuple(None if t is None else t[r0:r0 + 2 * N] for t in qp)
        two = _launch(sub, 2, N, H, 0.125, form, dev)
        for half, a, b in (("hi", out[0], two[0]), ("lo", out[1], two[1])):
            same = _bits(a[r0:r0 + 2 * N]) == _bits(b)
            if not bool(same.all()):
                r, c = (int(x) for x in (~same).nonzero()[0])
                raise AssertionError(f"b ring {form} N={N}: {name} two images differ from a B = 2 launch in {half} at "
                                     f"(b, h, q) = ({r0 // N + r // N}, {c // 64}, {r % N}), d = {c % 64}; {int((~same).sum())} elements differ")
    case = ar.reference(qp, B, N, H, 0.125, form)
    _check(case, _pair_value(out), f"b ring {form} N={N} nkt={nkt} pairs={B * H}")
    del case, out
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ c. strides and guards
class _IlvView:
    """An interleaved pair whose array is a column slice of a wider buffer (ops.IlvPair allocates a dense one)."""

    def __new__(cls, t, rows, cols):
        from mvp import ops

        self = ops.IlvPair.__new__(ops.IlvPair)
        self.rows, self.cols, self.t = rows, cols, t
        return self


@pytest.mark.parametrize("form", ar.FORMS)
@pytest.mark.parametrize("N", [70, 300])
def test_padded_strides_leave_guards_untouched(dev, form, N):
    """qkv and out as column slices of wider buffers with 64 extra rows behind B * N: the written region equals a dense launch bit for
    bit, and every guard column and row keeps its sentinel."""
    from mvp import ops

    B, H = 2, 2
    C, M, QOFF, PAD = H * 64, B * N, 64, 64
    qkv = _randn((M, 3 * C), 3000 + N, dev)
    qkv[:, :C] *= 2.0
    qp = _pack(qkv, C, form)
    dense = _launch(qp, B, N, H, 0.125, form, dev)
    ld_qkv = 3 * C + 128
    wide = [None if t is None else _sentinel(M + PAD, ld_qkv, dev, 11 + i) for i, t in enumerate(qp)]
    for w, t in zip(wide, qp):
        if w is not None:
            w[:M, QOFF:QOFF + 3 * C] = t
    wide_before = [None if w is None else w.clone() for w in wide]
    qs = tuple(None if w is None else w[:M, QOFF:QOFF + 3 * C] for w in wide)

    ld_out, OOFF = C + 32, 16
    buf = [_sentinel(M + PAD, ld_out, dev, 101), _sentinel(M + PAD, ld_out, dev, 202)]
    want = [b.clone() for b in buf]
    for w, d in zip(want, dense):
        w[:M, OOFF:OOFF + C] = d
    _attend(qs, (buf[0][:M, OOFF:OOFF + C], buf[1][:M, OOFF:OOFF + C]), B, N, H, 0.125, form, ld_qkv=ld_qkv, ld_out=ld_out)
    for half, g, w in zip(("hi", "lo"), buf, want):
        diff = _bits(g) != _bits(w)
        assert not bool(diff.any()), (f"c strides {form} N={N} separate {half}: {int(diff.sum())} elements differ from dense output + "
                                      f"sentinel, first at (row, col) = {tuple(int(x) for x in diff.nonzero()[0])} of [{M + PAD}, {ld_out}]")
    for w, w0 in zip(wide, wide_before):
        assert w is None or torch.equal(_bits(w), _bits(w0)), "the qkv buffer was written"

    if form != "bf16":  # the interleaved layout belongs to the bf16x3 forms
        ld_ilv, IOFF = 2 * C + 64, 32
        ibuf = _sentinel(M + PAD, ld_ilv, dev, 303)
        iwant = ibuf.clone()
        iwant[:M, IOFF:IOFF + 2 * C] = ops.interleave_pair(dense)
        _attend(qs, _IlvView(ibuf[:M, IOFF:IOFF + 2 * C], M, C), B, N, H, 0.125, form, ld_qkv=ld_qkv, ld_out=ld_ilv)
        diff = _bits(ibuf) != _bits(iwant)
        assert not bool(diff.any()), (f"c strides {form} N={N} interleaved: {int(diff.sum())} elements differ from dense output + sentinel, "
                                      f"first at (row, col) = {tuple(int(x) for x in diff.nonzero()[0])} of [{M + PAD}, {ld_ilv}]")
    case = ar.reference(qp, B, N, H, 0.125, form)
    _check(case, _pair_value((buf[0][:M, OOFF:OOFF + C], buf[1][:M, OOFF:OOFF + C])), f"c strides {form} N={N}")


# ------------------------------------------------------------------------------------------------ d. output forms
@pytest.mark.parametrize("form", [f for f in ar.FORMS if f != "bf16"])
@pytest.mark.parametrize("N", [70, 300])
def test_out_f16_separate_and_interleaved(dev, form, N):
    """out_f16 = 1: the compensated fp16 pair hi + (lo - hi / 8) / 8 meets the per-row bound + 2^-16, agrees with the bf16-pair output
    of the same inputs to 2^-15 per element (floor 2^-15 max |v|), and the interleaved array holds the separate pair's bits."""
    from mvp import ops

    B, H = 2, 2
    C, M = H * 64, B * N
    qkv = _randn((M, 3 * C), 4000 + N, dev)
    qkv[:, :C] *= 2.0
    qp = _pack(qkv, C, form)
    case = ar.reference(qp, B, N, H, 0.125, form)
    pair = _pair_value(_launch(qp, B, N, H, 0.125, form, dev))
    sep = _nan_pair(M, C, dev)
    _attend(qp, sep, B, N, H, 0.125, form, out_f16=True)
    got = ar.decode_out_f16(*sep)
    _check(case, got, f"d out_f16 {form} N={N}", extra=2.0 ** -16)
    tol = 2.0 ** -15 * torch.maximum(pair.abs(), case.v.abs().max())
    over = (got - pair).abs() > tol
    assert not bool(over.any()), f"d out_f16 {form} N={N}: {int(over.sum())} elements off the bf16-pair output, first (row, col) = {tuple(int(x) for x in over.nonzero()[0])}"
    ilv = ops.IlvPair(M, C, dev)
    ilv.t.fill_(float("nan"))
    _attend(qp, ilv, B, N, H, 0.125, form, out_f16=True)
    for half, a, b in zip(("hi", "lo"), ilv.separate(), sep):
        assert torch.equal(_bits(a), _bits(b)), f"d out_f16 {form} N={N}: interleaved {half} differs from separate"


def test_attention_argument_checks(dev):
    """The argument combinations mvp_attention_fwd refuses: MVP_EINVAL, and nothing is written."""
    from mvp import lib

    B, N, H = 1, 70, 2
    C = H * 64
    EINVAL = -1  # MVP_EINVAL, include/mvp_hip.h
    q = torch.zeros(B * N, 3 * C + 16, dtype=torch.bfloat16, device=dev)
    o, o_lo = _sentinel(B * N, 2 * C + 16, dev, 7), _sentinel(B * N, 2 * C + 16, dev, 8)
    o0, o_lo0 = o.clone(), o_lo.clone()
    fn = lib.load().mvp_attention_fwd

    def code(precision=lib.PREC_BF16X3, ld_qkv=3 * C, ld_out=C, layout=lib.PAIR_SEPARATE, v_format=0, out_f16=0):
        a = lib.AttentionArgs(lib.ptr(q), lib.ptr(q), lib.ptr(o), lib.ptr(o_lo), B, N, H, ld_qkv, ld_out, 0.125, precision, layout, v_format, out_f16)
        return fn(ctypes.byref(a), lib.stream_ptr())

    assert code(precision=lib.PREC_BF16, out_f16=1) == EINVAL
    assert code(precision=lib.PREC_BF16, layout=lib.PAIR_A_ILV32, ld_out=2 * C) == EINVAL
    assert code(v_format=3) == EINVAL
    assert code(precision=lib.PREC_BF16, v_format=1) == EINVAL
    assert code(ld_qkv=3 * C + 4) == EINVAL
    assert code(ld_out=C + 2) == EINVAL
    assert code(layout=lib.PAIR_A_ILV32, ld_out=2 * C - 4) == EINVAL
    assert code(layout=lib.PAIR_A_ILV32, ld_out=C) == EINVAL
    assert code(ld_qkv=3 * C - 8) == EINVAL and code(ld_out=C - 4) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(_bits(o), _bits(o0)) and torch.equal(_bits(o_lo), _bits(o_lo0))
    assert code() == 0  # and the accepted call of the same arguments goes through
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ e. softmax range
ROW_UNIFORM, ROW_KEY0, ROW_KEYLAST, ROW_ONEHOT, ROW_STAIR_UNDER, ROW_STAIR_OVER = 5, 21, 37, 53, 69, 101  # one per 16-row group of a wave


def _unit(i, dev):
    """Eight orthogonal unit directions of the head dimension: 8 dims each."""
    u = torch.zeros(64, device=dev)
    u[8 * i:8 * i + 8] = 8.0 ** -0.5
    return u


@pytest.mark.parametrize("form", ar.FORMS)
@pytest.mark.parametrize("scale", [0.03, 0.125, 1.0])
@pytest.mark.parametrize("N", [65, 257, 320])
def test_softmax_range_rows(dev, form, scale, N):
    """Rows built in exp2 units (score * scale * log2 e), each in a 16-row group of its own (the deferred rescale is decided per group):
      uniform    Q = 0: the output is the mean of V
      key 0      one key of the FIRST tile at 40 units, far above everything that follows
      key N - 1  the same for the last key — the only real key of the LAST tile at N = 65 and 257
      one-hot    a key 1200 units above the rest: every other probability underflows to zero
      staircases (N = 320) one key per tile parallel to the query, the tile maximum rising by 5.9 units per tile (below ATT_DEFER = 6:
                 the running maximum moves every second tile and probabilities reach 2^5.9) and by 6.1 (it moves in every tile);
                 all 16 rows of the group carry the staircase, so that no neighbour's maximum moves the group's first
    Every row is checked on its own against the bound with ITS largest exponent argument, and the whole case as everywhere."""
    B, H = 1, (2 if N < 320 else 1)
    C = H * 64
    qkv = _randn((B * N, 3 * C), 5000 + N, dev)
    qkv[:, :C] *= 0.125 / scale  # the random rows' logits as at scale = 1/8, whatever the scale
    q, k = _head_view(qkv[:, :C], B, N, H), _head_view(qkv[:, C:2 * C], B, N, H)
    unit = 1.0 / (scale * ar.LOG2E)  # a q . k of this size is one exp2 unit

    def dominant(row, key, d, units):
        amp = (units * unit) ** 0.5
        q[:, :, row] = amp * _unit(d, dev)
        k[:, :, key] = amp * _unit(d, dev)

    special = {"uniform": [ROW_UNIFORM], "key 0": [ROW_KEY0], "key N-1": [ROW_KEYLAST], "one-hot": [ROW_ONEHOT]}
    q[:, :, ROW_UNIFORM] = 0.0
    dominant(ROW_KEY0, 0, 0, 40.0)
    dominant(ROW_KEYLAST, N - 1, 1, 40.0)
    dominant(ROW_ONEHOT, N // 2, 2, 1200.0)
    if N == 320:
        for name, row, d, key0, step in (("stair 5.9", ROW_STAIR_UNDER, 3, 10, 5.9), ("stair 6.1", ROW_STAIR_OVER, 4, 20, 6.1)):
            special[name] = list(range(row - row % 16, row - row % 16 + 16))
            q[:, :, special[name]] = 0.5 * unit * _unit(d, dev)  # against a random key: 0.5 units rms
            for t in range(5):
                k[:, :, key0 + 64 * t] = 2.0 * step * (t + 1) * _unit(d, dev)
    qp = _pack(qkv, C, form)
    case = ar.reference(qp, B, N, H, scale, form)
    out = _launch(qp, B, N, H, scale, form, dev)
    got = _pair_value(out)
    label = f"e range {form} N={N} scale={scale}"
    err = _check(case, got, label)
    # the rows are what they were built to be (in the reference), and each meets the bound on its own
    x = (case.q @ case.k.transpose(-2, -1)) * (scale * ar.LOG2E)
    mean_v = case.v.mean(dim=2)
    assert float((case.ref[:, :, ROW_UNIFORM] - mean_v).abs().max()) <= 1e-12 * float(case.v.abs().max())
    assert float((x[:, :, ROW_KEY0, 0] - x[:, :, ROW_KEY0, 1:].max(-1).values).min()) > 6.0  # more than ATT_DEFER
    assert float((x[:, :, ROW_KEYLAST, N - 1] - x[:, :, ROW_KEYLAST, :N - 1].max(-1).values).min()) > 6.0
    others = torch.cat((x[:, :, ROW_ONEHOT, :N // 2], x[:, :, ROW_ONEHOT, N // 2 + 1:]), -1)
    assert float((x[:, :, ROW_ONEHOT, N // 2] - others.max(-1).values).min()) > 1000.0
    if N == 320 and form != "bf16":  # (bf16 operands move a score of 30 by 0.1; that form has no deferral)
        for row, lo, hi in ((ROW_STAIR_UNDER, 5.8, 6.0), (ROW_STAIR_OVER, 6.0, 6.2)):
            tmax = x[:, :, row].reshape(B, H, 5, 64).max(-1).values
            rise = torch.cat((tmax[..., :1], tmax[..., 1:] - tmax[..., :-1]), -1)
            assert lo < float(rise.min()) and float(rise.max()) < hi, (row, tmax)
    gh = ar.heads(got, B, N, H)
    for name, rows in special.items():
        row_bound = ar.bound(case.model_err, float(case.smax[:, :, rows].max()))
        e, (_, h, i) = ar.worst(err[:, :, rows])
        print(f"[attn-row] {label} row {name}: kernel {e:.3e} at (b, h, q) = (0, {h}, {rows[i]}), bound {row_bound:.3e}")
        assert e <= row_bound, f"{label}: the {name} row (b, h, q) = (0, {h}, {rows[i]}) has error {e:.3e} > {row_bound:.3e}"
    e = float(ar.row_err(gh[:, :, ROW_UNIFORM:ROW_UNIFORM + 1], mean_v.unsqueeze(2), case.v).max())
    assert e <= case.bound, f"{label}: the Q = 0 row is {e:.3e} off the fp64 mean of V (bound {case.bound:.3e})"


def test_torch_pair_split_is_the_library_split(dev):
    """attention_ref.split_bf16 (what the CPU test of the reference packs with) writes the bits of ops.split_bf16."""
    from mvp import ops

    x = _randn((70, 384), 6000, dev) * 3.0
    a, b = ops.split_bf16(x), ar.split_bf16(x)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
