"""mvp_attention_bias_fwd — softmax(Q K^T * scale + bias[h]) V — against fp64, one query row at a time (tests/attention_bias_ref.py: the
reference, the rounding model and the budget 4 x model row error + 2^-21 x the largest |logit * log2 e|, bias included):

  a  token counts at both kernels' edges, all four operand forms
  b  the persistent ring of the resident kernel: the bias row base follows the pair the ring is on
  c  a zero bias stays within the UNBIASED reference's bound
  d  the softmax's range under a bias: a +40 spike in the last tile, tile maxima that climb by just under / over the deferral threshold
     through the bias alone, a uniform -30
  e  ld_bias / bias_head_stride larger than minimal with NaN guards, out_f16, the interleaved output, padded ld_qkv / ld_out

Every output is prefilled with NaN bit patterns; the padding columns of every bias row, and everything around the array, hold NaN."""
import pytest
import torch

import attention_bias_ref as abr
import attention_ref as ar
from test_gpu_attention import _bits, _check, _head_view, _IlvView, _nan_pair, _pack, _pair_value, _prec, _randn, _sentinel, _unit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _attend(qp, out, B, N, H, scale, form, bias, **kw):
    from mvp import ops

    ops.attention(qp, out, B, N, H, scale, _prec(form), v_f16="_vf16" in form, qk_f16=form.endswith("_qk16"), bias=bias, **kw)
    torch.cuda.synchronize()


def _launch(qp, B, N, H, scale, form, bias, dev):
    out = _nan_pair(B * N, H * 64, dev)
    _attend(qp, out, B, N, H, scale, form, bias)
    return out


def _head_bias(H, N, seed, dev, std=2.0):
    """fp32 [H, N, N] ~ N(0, std), head h scaled by 1 + h / 2 and offset by 3 h: another head's bias is a gross row error."""
    b = _randn((H, N, N), seed, dev) * std
    for h in range(H):
        b[h] = b[h] * (1.0 + 0.5 * h) + 3.0 * h
    return b


def _qkv(B, N, H, seed, dev):
    C = H * 64
    qkv = _randn((B * N, 3 * C), seed, dev)
    qkv[:, :C] *= 2.0
    v = _head_view(qkv[:, 2 * C:], B, N, H)
    for b in range(B):
        for h in range(H):
            v[b, h] = v[b, h] * ((1 + b % 3) * (1 + h)) + (3 * (b % 5) + 5 * h)
    return qkv


# ------------------------------------------------------------------------------------------------ a. token-count edges
@pytest.mark.parametrize("form", ar.FORMS)
@pytest.mark.parametrize("N", [1, 17, 64, 65, 197, 256, 257, 384, 385])
def test_bias_token_count_edges_per_row_vs_fp64(dev, form, N):
    """One tile, one key past a tile, the production count, the last resident and first streaming count, a full and a one-key last
    streaming tile.  bias ~ N(0, 2) per head; NaN in every padding column."""
    B, H = 2, 2
    qp = _pack(_qkv(B, N, H, 11000 + N, dev), H * 64, form)
    dense = _head_bias(H, N, 12000 + N, dev)
    bias, _ = abr.bias_buffer(dense)
    case = abr.reference(qp, B, N, H, 0.125, form, dense)
    out = _launch(qp, B, N, H, 0.125, form, bias, dev)
    _check(case, _pair_value(out), f"bias a edges {form} N={N}")


# ------------------------------------------------------------------------------------------------ b. persistent ring
@pytest.mark.parametrize("form", ["bf16x3", "bf16x3_vf16_qk16"])
@pytest.mark.parametrize("N", [70, 150])
def test_bias_follows_the_ring(dev, form, N):
    """As many pairs as make every workgroup walk its ring past every slot offset and wrap (attention_ref.ring_pairs), H = 3: the head
    of a ring iteration is bh % H, not the workgroup's first.  Every pair against fp64."""
    from mvp import lib

    H, nkt = 3, ar.nkt_of(N)
    cus = int(lib.info().cu_count)
    assert cus > 0
    B = -(-ar.ring_pairs(nkt, form, cus) // H)
    qp = _pack(_qkv(B, N, H, 13000 + N, dev), H * 64, form)
    dense = _head_bias(H, N, 14000 + N, dev)
    bias, _ = abr.bias_buffer(dense)
    out = _launch(qp, B, N, H, 0.125, form, bias, dev)
    case = abr.reference(qp, B, N, H, 0.125, form, dense)
    _check(case, _pair_value(out), f"bias b ring {form} N={N} pairs={B * H}")
    del case, out
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ c. zero bias
@pytest.mark.parametrize("form", ar.FORMS)
@pytest.mark.parametrize("N", [197, 300])
def test_zero_bias_within_the_unbiased_bound(dev, form, N):
    """bias = 0 (NaN padding all the same): the output meets attention_ref's own bound of the unbiased case."""
    B, H = 2, 2
    qp = _pack(_qkv(B, N, H, 15000 + N, dev), H * 64, form)
    bias, _ = abr.bias_buffer(torch.zeros(H, N, N, device=dev))
    case = ar.reference(qp, B, N, H, 0.125, form)
    out = _launch(qp, B, N, H, 0.125, form, bias, dev)
    _check(case, _pair_value(out), f"bias c zero {form} N={N}")


# ------------------------------------------------------------------------------------------------ d. softmax range
ROW_SPIKE, ROW_UNDER, ROW_OVER = 21, 69, 101  # one per 16-row group of a wave


@pytest.mark.parametrize("form", ["bf16x3_vf16", "bf16x3_vf16_qk16"])
@pytest.mark.parametrize("N", [197, 300])
@pytest.mark.parametrize("kind", ["spike_stairs", "uniform_m30"])
def test_bias_softmax_range(dev, form, N, kind):
    """spike_stairs: a row whose Q.K favours key 0 (20 exp2 units above the rest) gets +40 on the LAST key — the best key moves into the
    last tile by far more than 2^6; two 16-row groups with Q = 0 whose tile maxima climb through the bias alone, by 5.9 / log2 e per
    tile (under ATT_DEFER: the running maximum may stay) and by 6.1 / log2 e (it must move in every tile).  uniform_m30: bias = -30
    everywhere, the softmax of the unbiased logits.  Each special row meets the bound with ITS largest exponent argument."""
    B, H = 1, 2
    C, scale = H * 64, 0.125
    nkt = ar.nkt_of(N)
    qkv = _qkv(B, N, H, 16000 + N, dev)
    dense = _head_bias(H, N, 17000 + N, dev, std=0.5)
    special = {}
    if kind == "uniform_m30":
        dense[:] = -30.0
    else:
        q, k = _head_view(qkv[:, :C], B, N, H), _head_view(qkv[:, C:2 * C], B, N, H)
        amp = (20.0 / (scale * ar.LOG2E)) ** 0.5
        q[:, :, ROW_SPIKE] = amp * _unit(0, dev)
        k[:, :, 0] = amp * _unit(0, dev)
        dense[:, ROW_SPIKE, N - 1] += 40.0
        special["spike"] = [ROW_SPIKE]
        for name, row, step in (("stair 5.9", ROW_UNDER, 5.9), ("stair 6.1", ROW_OVER, 6.1)):
            rows = list(range(row - row % 16, row - row % 16 + 16))
            q[:, :, rows] = 0.0
            dense[:, rows] *= 0.1
            for t in range(nkt):
                dense[:, rows, 64 * t + 2] = step / ar.LOG2E * (t + 1)
            special[name] = rows
    qp = _pack(qkv, C, form)
    bias, _ = abr.bias_buffer(dense)
    case = abr.reference(qp, B, N, H, scale, form, dense)
    out = _launch(qp, B, N, H, scale, form, bias, dev)
    label = f"bias d range {form} N={N} {kind}"
    err = _check(case, _pair_value(out), label)
    x = ((case.q @ case.k.transpose(-2, -1)) * scale + case.bias) * ar.LOG2E
    if kind == "spike_stairs":  # the rows are what they were built to be
        raw = x[:, :, ROW_SPIKE] - case.bias[:, ROW_SPIKE] * ar.LOG2E
        assert float((raw[..., 0] - raw[..., 1:].max(-1).values).min()) > 6.0
        assert float((x[:, :, ROW_SPIKE, N - 1] - x[:, :, ROW_SPIKE, :N - 1].max(-1).values).min()) > 6.0
        for row, lo, hi in ((ROW_UNDER, 5.8, 6.0), (ROW_OVER, 6.0, 6.2)):
            xr = torch.nn.functional.pad(x[:, :, row], (0, 64 * nkt - N), value=float("-inf"))
            tmax = xr.reshape(B, H, nkt, 64).max(-1).values
            rise = tmax[..., 1:] - tmax[..., :-1]
            assert lo < float(rise.min()) and float(rise.max()) < hi, (row, tmax)
    for name, rows in special.items():
        row_bound = abr.bound(case.model_err, float(case.smax[:, :, rows].max()))
        e, (_, h, i) = ar.worst(err[:, :, rows])
        print(f"[attn-row] {label} row {name}: kernel {e:.3e} at (b, h, q) = (0, {h}, {rows[i]}), bound {row_bound:.3e}")
        assert e <= row_bound, f"{label}: the {name} row (b, h, q) = (0, {h}, {rows[i]}) has error {e:.3e} > {row_bound:.3e}"


# ------------------------------------------------------------------------------------------------ e. strides and output forms
@pytest.mark.parametrize("form", ar.FORMS)
@pytest.mark.parametrize("N", [70, 300])
def test_bias_strides_and_output_forms(dev, form, N):
    """ld_bias and bias_head_stride larger than minimal (NaN in every gap, in front of and behind the array), qkv and out as column
    slices of wider sentinel buffers: the written region equals the dense launch bit for bit and every guard keeps its pattern; the
    interleaved output holds the separate pair's bits; out_f16 = 1 meets the per-row bound + 2^-16."""
    from mvp import ops

    B, H = 2, 2
    C, M, QOFF, PAD = H * 64, B * N, 64, 64
    qp = _pack(_qkv(B, N, H, 18000 + N, dev), C, form)
    dense_b = _head_bias(H, N, 19000 + N, dev)
    tight, _ = abr.bias_buffer(dense_b)
    case = abr.reference(qp, B, N, H, 0.125, form, dense_b)
    dense = _launch(qp, B, N, H, 0.125, form, tight, dev)
    _check(case, _pair_value(dense), f"bias e dense {form} N={N}")
    ld_bias = abr.padded(N) + 8
    loose, lbuf = abr.bias_buffer(dense_b, ld=ld_bias, head_stride=N * ld_bias + 100, lead=64)
    lbuf0 = lbuf.clone()

    ld_qkv = 3 * C + 128
    wide = [None if t is None else _sentinel(M + PAD, ld_qkv, dev, 11 + i) for i, t in enumerate(qp)]
    for w, t in zip(wide, qp):
        if w is not None:
            w[:M, QOFF:QOFF + 3 * C] = t
    qs = tuple(None if w is None else w[:M, QOFF:QOFF + 3 * C] for w in wide)
    ld_out, OOFF = C + 32, 16
    buf = [_sentinel(M + PAD, ld_out, dev, 101), _sentinel(M + PAD, ld_out, dev, 202)]
    want = [b.clone() for b in buf]
    for w, d in zip(want, dense):
        w[:M, OOFF:OOFF + C] = d
    _attend(qs, (buf[0][:M, OOFF:OOFF + C], buf[1][:M, OOFF:OOFF + C]), B, N, H, 0.125, form, loose, ld_qkv=ld_qkv, ld_out=ld_out)
    for half, g, w in zip(("hi", "lo"), buf, want):
        diff = _bits(g) != _bits(w)
        assert not bool(diff.any()), (f"bias e strides {form} N={N} {half}: {int(diff.sum())} elements differ from dense output + sentinel, "
                                      f"first at (row, col) = {tuple(int(x) for x in diff.nonzero()[0])} of [{M + PAD}, {ld_out}]")
    assert torch.equal(lbuf.view(torch.int32), lbuf0.view(torch.int32)), "the bias buffer was written"
    if form == "bf16":
        return
    ld_ilv, IOFF = 2 * C + 64, 32
    ibuf = _sentinel(M + PAD, ld_ilv, dev, 303)
    iwant = ibuf.clone()
    iwant[:M, IOFF:IOFF + 2 * C] = ops.interleave_pair(dense)
    _attend(qs, _IlvView(ibuf[:M, IOFF:IOFF + 2 * C], M, C), B, N, H, 0.125, form, loose, ld_qkv=ld_qkv, ld_out=ld_ilv)
    diff = _bits(ibuf) != _bits(iwant)
    assert not bool(diff.any()), f"bias e interleaved {form} N={N}: {int(diff.sum())} elements differ, first at {tuple(int(x) for x in diff.nonzero()[0])}"
    sep = _nan_pair(M, C, dev)
    _attend(qp, sep, B, N, H, 0.125, form, loose, out_f16=True)
    _check(case, ar.decode_out_f16(*sep), f"bias e out_f16 {form} N={N}", extra=2.0 ** -16)
    ilv = ops.IlvPair(M, C, dev)
    ilv.t.fill_(float("nan"))
    _attend(qp, ilv, B, N, H, 0.125, form, loose, out_f16=True)
    for half, a, b in zip(("hi", "lo"), ilv.separate(), sep):
        assert torch.equal(_bits(a), _bits(b)), f"bias e out_f16 {form} N={N}: interleaved {half} differs from separate"
