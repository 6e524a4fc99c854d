"""mvp_relpos_terms and mvp_attention_relpos_fwd — softmax(Q K^T * scale + rel[q][k / Kw] + rel[q][Kh + k % Kw]) V.

Terms: every element against fp64 within the fp32 dot-product bound gamma_64 * sum_d |q_d R_d| (gamma_64 = 64 u / (1 - 64 u), u = 2^-24),
computed per element; the pair buffer it writes equals the qkv GEMM's forms (the library's own split of the same values).
Attention: per query row against fp64 with tests/attention_bias_ref.py's rounding model and budget — the bias enters exactly like a dense
one; the fp64 reference is handed the kernel's OWN rel output (densified on the host in fp64), so the two checks stay separate.  Shapes:
N = 15 (3 x 5: one partial tile), 196 (14 x 14: the resident ring, a last tile of 4 keys, Kw % 4 != 0 so every second 4-key group straddles a
key row), 323 (17 x 19: streaming, Kw odd)."""
import pytest
import torch

import attention_bias_ref as abr
import attention_ref as ar
from test_gpu_attention import _bits, _check, _IlvView, _nan_pair, _pair_value, _prec, _randn
from test_gpu_attention_bias import _qkv

pytestmark = pytest.mark.gpu
GRIDS = {15: (3, 5), 196: (14, 14), 323: (17, 19)}
U = 2.0 ** -24
GAMMA64 = 64 * U / (1 - 64 * U)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _tables(Kh, Kw, seed, dev, std=0.15):
    return _randn((Kh, Kh, 64), seed, dev) * std, _randn((Kw, Kw, 64), seed + 1, dev) * std


def _terms(qkv, B, N, H, form, rh, rw, dev, ld=None):
    """mvp_relpos_terms on the fp32 projection -> (pair buffer, rel [B * H, N, ld] with NaN in the padding columns)."""
    from mvp import ops

    Kh, Kw = rh.shape[1], rw.shape[1]
    ld = ld or -(-(Kh + Kw) // 4) * 4
    rel = torch.full((B * H, N, ld), float("nan"), device=dev)
    out = _nan_pair(B * N, 3 * H * 64, dev)
    if form == "bf16":
        out = (out[0], None)
    ops.relpos_terms(qkv, out, rel, rh, rw, B * N, N, H, _prec(form), v_f16="_vf16" in form, qk_f16=form.endswith("_qk16"))
    torch.cuda.synchronize()
    return out, rel


def _epilogue_forms(qkv, C, form):
    """The pair the qkv GEMM's epilogue writes from these fp32 values (csrc/mvp_common.h, split2_form), each third converted FROM THE
    FP32 VALUE: bf16 pair | V as fp16 + bf16 (vf16) | Q the compensated activation pair, K the compensated weight-side pair (qk16).
    (ar.pack is not this: it re-forms the thirds from an already split bf16 pair, which is how the attention tests make operands.)"""
    from mvp import ops
    from test_gpu_kernels import _wcomp_pair

    hi, lo = ops.split_bf16(qkv, _prec(form))
    if "_vf16" in form:
        vh, vl = ops.split_f16_bf16(qkv[:, 2 * C:])
        hi[:, 2 * C:], lo[:, 2 * C:] = vh, vl
    if form.endswith("_qk16"):
        qh, ql = ops.split_f16_comp(qkv[:, :C])
        kh, kl = _wcomp_pair(qkv[:, C:2 * C])
        hi[:, :C], lo[:, :C] = qh, ql
        hi[:, C:2 * C], lo[:, C:2 * C] = kh, kl
    return hi, lo


def _dense(rel, B, H, Kh, Kw):
    """fp64 [B, H, N, N] of a rel buffer: bias[q][k] = rel[q][k // Kw] + rel[q][Kh + k % Kw]."""
    N = Kh * Kw
    r = rel.double().view(B, H, N, -1)
    return (r[..., :Kh, None] + r[..., None, Kh:Kh + Kw]).reshape(B, H, N, N)


def _attend(qp, out, B, N, H, form, rel, grid, **kw):
    from mvp import ops

    ops.attention(qp, out, B, N, H, 0.125, _prec(form), v_f16="_vf16" in form, qk_f16=form.endswith("_qk16"), rel=rel, rel_grid=grid, **kw)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the terms
@pytest.mark.parametrize("form", ar.FORMS)
@pytest.mark.parametrize("N", [15, 196, 323])
def test_relpos_terms_vs_fp64(dev, form, N):
    B, H = 2, 2
    Kh, Kw = GRIDS[N]
    C = H * 64
    qkv = _qkv(B, N, H, 21000 + N, dev)
    rh, rw = _tables(Kh, Kw, 22000 + N, dev)
    out, rel = _terms(qkv, B, N, H, form, rh, rw, dev)
    q = ar.heads(qkv[:, :C].double(), B, N, H).reshape(B, H, Kh, Kw, 64)
    want_h = torch.einsum("bnhwc,hkc->bnhwk", q, rh.double())
    want_w = torch.einsum("bnhwc,wkc->bnhwk", q, rw.double())
    mag_h = torch.einsum("bnhwc,hkc->bnhwk", q.abs(), rh.double().abs())
    mag_w = torch.einsum("bnhwc,wkc->bnhwk", q.abs(), rw.double().abs())
    got = rel.view(B, H, Kh, Kw, -1).double()
    eh, ew = (got[..., :Kh] - want_h).abs(), (got[..., Kh:Kh + Kw] - want_w).abs()
    print(f"\n[relpos terms {form} N={N}] worst error / bound: h {float((eh / (GAMMA64 * mag_h)).max()):.3f}, w {float((ew / (GAMMA64 * mag_w)).max()):.3f}")
    assert bool((eh <= GAMMA64 * mag_h).all()) and bool((ew <= GAMMA64 * mag_w).all())
    assert bool(torch.isnan(rel[..., Kh + Kw:]).all())  # padding columns are not written
    want = _epilogue_forms(qkv, C, form)
    assert torch.equal(_bits(out[0]), _bits(want[0]))
    if form != "bf16":
        assert torch.equal(_bits(out[1]), _bits(want[1]))


@pytest.mark.parametrize("form", ar.FORMS)
def test_relpos_terms_pair_equals_the_qkv_gemm_pair(dev, form):
    """The pair buffer against the qkv GEMM's OWN pair output (out_f16_col0 of the same form) from the same operands, bit for bit; the
    fp32 input is that GEMM's out_f32 — one definition of each 16-bit form, as for mvp_rope2d_qkv."""
    from mvp import lib, ops

    B, H, K, N = 2, 2, 128, 15
    Kh, Kw = GRIDS[N]
    M, C3 = B * N, 3 * H * 64
    prec = _prec(form)
    a, w, bias = _randn((M, K), 28000, dev), _randn((C3, K), 28001, dev) * K ** -0.5, _randn((C3,), 28002, dev)
    ap, wp = ops.split_bf16(a, prec), ops.split_bf16(w, prec)
    col0 = (-2 if form.endswith("_qk16") else 2) * H * 64 if "_vf16" in form else 0
    want = ops.empty_pair((M, C3), prec, dev)
    f32 = torch.empty(M, C3, device=dev)
    ops.gemm(ap, wp, M, C3, K, bias=bias, out=want, precision=prec, f16_col0=col0)
    ops.gemm(ap, wp, M, C3, K, bias=bias, out_f32=f32, precision=prec)
    got, _ = _terms(f32, B, N, H, form, *_tables(Kh, Kw, 28003, dev), dev)
    assert torch.equal(_bits(got[0]), _bits(want[0]))
    if form != "bf16":
        assert torch.equal(_bits(got[1]), _bits(want[1]))


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("form", ar.FORMS)
@pytest.mark.parametrize("N", [15, 196, 323])
@pytest.mark.parametrize("B,H", [(1, 3), (5, 1)])
def test_attention_relpos_per_row_vs_fp64(dev, form, N, B, H):
    """3 and 5 (batch, head) pairs; one key ROW of the grid gets a large bias (q . Rh large for ky = 1), so an off-by-one in k / Kw moves
    the arg-max; the output, out_f16 and the interleaved layout."""
    from mvp import ops

    Kh, Kw = GRIDS[N]
    C, M = H * 64, B * N
    qkv = _qkv(B, N, H, 23000 + N + B, dev)
    rh, rw = _tables(Kh, Kw, 24000 + N, dev)
    rh[:, 1] += 0.6 * torch.sign(qkv[:N, :64]).view(Kh, Kw, 64)[:, 0]  # head 0, image 0: query row yq favours key row 1 by ~ +60
    qp, rel = _terms(qkv, B, N, H, form, rh, rw, dev)
    dense = _dense(rel, B, H, Kh, Kw)
    case = abr.reference(qp, B, N, H, 0.125, form, dense)
    out = _nan_pair(M, C, dev)
    _attend(qp, out, B, N, H, form, rel, (Kh, Kw))
    _check(case, _pair_value(out), f"relpos {form} N={N} pairs={B * H}")
    if form == "bf16":
        return
    ibuf = torch.full((M, 2 * C), float("nan"), dtype=torch.bfloat16, device=dev)
    _attend(qp, _IlvView(ibuf, M, C), B, N, H, form, rel, (Kh, Kw), ld_out=2 * C)
    assert torch.equal(_bits(ibuf), _bits(ops.interleave_pair(out)))
    sep = _nan_pair(M, C, dev)
    _attend(qp, sep, B, N, H, form, rel, (Kh, Kw), out_f16=True)
    _check(case, ar.decode_out_f16(*sep), f"relpos out_f16 {form} N={N}", extra=2.0 ** -16)
    ilv = ops.IlvPair(M, C, dev)
    ilv.t.fill_(float("nan"))
    _attend(qp, ilv, B, N, H, form, rel, (Kh, Kw), out_f16=True)
    for a, b in zip(ilv.separate(), sep):
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("form", ar.FORMS)
@pytest.mark.parametrize("N", [15, 196, 323])
def test_zero_tables_equal_plain_attention_bit_for_bit(dev, form, N):
    """Zero tables (rel = 0 as the kernel computes it) at scale 2^-3: s * scale + 0 is exact, and a power-of-two scale commutes with every
    rounding of the exp2 argument, so the output equals mvp_attention_fwd's bit for bit."""
    from mvp import ops

    B, H = 2, 3
    Kh, Kw = GRIDS[N]
    qkv = _qkv(B, N, H, 25000 + N, dev)
    qp, rel = _terms(qkv, B, N, H, form, torch.zeros(Kh, Kh, 64, device=dev), torch.zeros(Kw, Kw, 64, device=dev), dev)
    assert not bool(rel[..., :Kh + Kw].any())
    out, plain = _nan_pair(B * N, H * 64, dev), _nan_pair(B * N, H * 64, dev)
    _attend(qp, out, B, N, H, form, rel, (Kh, Kw))
    ops.attention(qp, plain, B, N, H, 0.125, _prec(form), v_f16="_vf16" in form, qk_f16=form.endswith("_qk16"))
    torch.cuda.synchronize()
    assert torch.equal(_bits(out[0]), _bits(plain[0]))
    if form != "bf16":
        assert torch.equal(_bits(out[1]), _bits(plain[1]))


@pytest.mark.parametrize("N", [196, 323])
def test_against_the_dense_bias_kernel(dev, N):
    """B = 1: the same logits through mvp_attention_bias_fwd fed the densified bias (fp32) — both within the per-row budget of one case."""
    form, B, H = "bf16x3_vf16_qk16", 1, 2
    Kh, Kw = GRIDS[N]
    qkv = _qkv(B, N, H, 26000 + N, dev)
    rh, rw = _tables(Kh, Kw, 27000 + N, dev)
    qp, rel = _terms(qkv, B, N, H, form, rh, rw, dev, ld=-(-(Kh + Kw) // 4) * 4 + 8)  # (a longer row than minimal: NaN behind the terms)
    r = rel.view(H, N, -1)
    dense32 = (r[..., :Kh, None] + r[..., None, Kh:Kh + Kw]).reshape(H, N, N)  # fp32 sum of the two terms, as the kernel forms it
    case = abr.reference(qp, B, N, H, 0.125, form, dense32.double())
    out = _nan_pair(N, H * 64, dev)
    _attend(qp, out, B, N, H, form, rel, (Kh, Kw))
    _check(case, _pair_value(out), f"relpos vs dense (relpos) N={N}")
    from mvp import ops

    bias, _ = abr.bias_buffer(dense32)
    out_d = _nan_pair(N, H * 64, dev)
    ops.attention(qp, out_d, B, N, H, 0.125, _prec(form), v_f16=True, qk_f16=True, bias=bias)
    torch.cuda.synchronize()
    _check(case, _pair_value(out_d), f"relpos vs dense (dense) N={N}")
