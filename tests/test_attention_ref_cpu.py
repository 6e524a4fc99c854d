"""The attention reference of the GPU tests (tests/attention_ref.py) checked on its own, without a GPU: the rounding model with its
roundings switched off is the exact fp64 attention, ``decode`` inverts every operand packing to the accuracy that form documents, and
the model's error is non-zero and ordered bf16 pair < fp16 probabilities < plain bf16."""
import pytest
import torch

import attention_ref as ar

B, N, H, SCALE = 2, 70, 2, 0.125
C = H * 64


@pytest.fixture(scope="module")
def qkv():
    g = torch.Generator().manual_seed(70)
    x = torch.randn(B * N, 3 * C, generator=g)
    x[:, :C] *= 2.0
    x[3, 5] = 3e-4   # a value whose compensated lo half is an fp16 denormal
    x[4, C + 7] = 300.0
    return x


@pytest.mark.parametrize("form", ar.FORMS)
def test_model_without_roundings_is_the_exact_attention(qkv, form):
    qp = ar.pack(qkv, C, form)
    h = {k: ar.heads(t, B, N, H) for k, t in ar.halves(qp, C, form).items()}
    q, k, v = (ar.heads(t, B, N, H) for t in ar.decode(qp, C, form))
    ref = ar.exact(q, k, v, SCALE)
    ideal = ar.model(h, SCALE, form, ideal=True)
    assert ref.shape == (B, H, N, 64) and ref.dtype == torch.float64
    assert float((ideal - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    # and exact itself, spelled out for one row
    s = (q[1, 1, 7] @ k[1, 1].T) * SCALE
    w = torch.exp(s - s.max())
    assert torch.allclose(ref[1, 1, 7], (w / w.sum()) @ v[1, 1], rtol=0, atol=1e-13)
    # rows: the inverse of heads
    assert torch.equal(ar.heads(ar.rows(ref), B, N, H), ref)


def _max_rel(got, want, floor):
    """max (|got - want| - floor) / |want|: the relative error once an absolute ``floor`` is taken off."""
    d = (got - want).abs() - floor
    return float((d / want.abs().clamp_min(1e-300)).max())


def test_decode_inverts_each_packing_to_its_documented_accuracy(qkv):
    from mvp import ops
    from test_gpu_kernels import _v_third_as_f16_bf16, _wcomp_pair

    x = qkv.double()
    # bf16 pair: hi keeps 8 bits, lo 8 more of the remainder -> 2^-9 * 2^-9 relative; hi alone 2^-9
    q, k, v = ar.decode(ar.pack(qkv, C, "bf16x3"), C, "bf16x3")
    assert _max_rel(torch.cat((q, k, v), 1), x, 0.0) <= 2.0 ** -17
    q, k, v = ar.decode(ar.pack(qkv, C, "bf16"), C, "bf16")
    assert _max_rel(torch.cat((q, k, v), 1), x, 0.0) <= 2.0 ** -8
    assert torch.equal(torch.cat((q, k, v), 1), qkv.bfloat16().double())
    # V as fp16 + bf16: |v - hi - lo| <= 2^-20 |v| (include/mvp_hip.h, out_f16_col0); Q and K stay the bf16 pair
    pair = ar.pack(qkv, C, "bf16x3")
    vq = _v_third_as_f16_bf16(pair, C)
    q1, k1, v1 = ar.decode(vq, C, "bf16x3_vf16")
    vin = pair[0][:, 2 * C:].double() + pair[1][:, 2 * C:].double()
    q0 = pair[0][:, :C].double() + pair[1][:, :C].double()
    kin = pair[0][:, C:2 * C].double() + pair[1][:, C:2 * C].double()
    assert _max_rel(v1, vin, 0.0) <= 2.0 ** -20
    assert torch.equal(q1, q0) and torch.equal(k1, kin)
    # the compensated pairs: lo carries one fp16 rounding of a value of ~|x| / 8, read back through / 8 (activation: hi + (lo - hi/8)/8,
    # weight side: hi + lo/8) -> 2^-11 / 64 (1 + 2^-5) < 2^-16 relative, plus the fp16 denormal spacing 2^-24 / 8 of a tiny lo
    q2, k2, v2 = ar.decode(ar.pack(qkv, C, "bf16x3_vf16_qk16"), C, "bf16x3_vf16_qk16")
    assert _max_rel(q2, q0, 2.0 ** -27) <= 2.0 ** -16
    assert _max_rel(k2, kin, 2.0 ** -27) <= 2.0 ** -16
    assert torch.equal(v2, v1)
    # the two helpers on their own, on values the pair forms do not produce
    y = torch.tensor([[1.0, -0.3333333, 1e-3, 1234.5, 6.1e-5, -65504.0, 0.0, 2.0 ** -10]] * 8).repeat(1, 8)  # [8, 64]
    hi, lo = ops.split_f16_comp(y)
    assert _max_rel(ar.decode_out_f16(hi, lo), y.double(), 2.0 ** -27) <= 2.0 ** -16
    kh, kl = _wcomp_pair(y)
    got = kh.view(torch.float16).double() + kl.view(torch.float16).double() / 8.0
    assert _max_rel(got, y.double(), 2.0 ** -27) <= 2.0 ** -16


def test_model_error_is_nonzero_and_ordered_by_form(qkv):
    worst = {}
    for form in ar.FORMS:
        case = ar.reference(ar.pack(qkv, C, form), B, N, H, SCALE, form)
        worst[form] = float(case.model_err.max())
        assert case.model_err.shape == (B, H, N)
        assert 0.0 < worst[form] < ar.CAPS[form], (form, worst[form])
        assert case.bound > 4.0 * worst[form] and case.bound < 4.0 * worst[form] + 2.0 ** -22 * max(1.0, float(case.smax.max())) * 1.0001
        e, (b, h, q) = ar.worst(case.model_err)
        assert e == worst[form] and float(case.model_err[b, h, q]) == e
    print("model max row error:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert worst["bf16x3"] < worst["bf16x3_vf16"] < worst["bf16"]
    assert worst["bf16x3"] < worst["bf16x3_vf16_qk16"] < worst["bf16"]


def test_row_err_sees_one_wrong_row_where_rel_l2_does_not():
    """Gap 2 of the whole-tensor comparison: a 1 % error in one row of (1, 2501, 2)."""
    g = torch.Generator().manual_seed(1)
    v = torch.randn(1, 2, 2501, 64, generator=g, dtype=torch.float64)
    ref = torch.randn(1, 2, 2501, 64, generator=g, dtype=torch.float64)
    got = ref.clone()
    got[0, 1, 2500] *= 1.01
    assert ar.rel_l2(got, ref) < 3e-4
    err = ar.row_err(got, ref, v)
    e, where = ar.worst(err)
    assert where == (0, 1, 2500) and e > 3e-4 and int((err > 0).sum()) == 1


def test_ring_pair_count_visits_every_slot_and_wraps():
    for form in ar.FORMS:
        for nkt in (1, 2, 3, 4):
            pc = ar.per_cu(nkt, form)
            assert pc == max(1, (160 * 1024) // ((nkt + 1) * ar.STAGE_BYTES[form])) and (nkt + 1) * ar.STAGE_BYTES[form] * pc <= 160 * 1024
            grid, pairs = 256 * pc, ar.ring_pairs(nkt, form, 256)
            iters = [len(range(w, pairs, grid)) for w in (0, 2, 3, grid - 1)]
            assert iters == [nkt + 3, nkt + 3, nkt + 2, nkt + 2]
            assert {(nkt * i) % (nkt + 1) for i in range(nkt + 2)} == set(range(nkt + 1))
