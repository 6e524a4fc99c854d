"""GPU parity tests (run on the MI355X box with -m gpu): every HIP kernel of the backbone
path, called through the C ABI, against the CPU oracle / an fp64 torch restatement.

Tolerances: bf16x3 mode is held to the north-star bar (1e-3 rel on fp32 feature tensors;
kernels individually to ~1e-4); plain bf16 mode is checked against a bf16-rounded-operand
reference (so the MFMA arithmetic itself is verified tightly) and, end to end, against a
looser documented bound.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, max_rel, rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mvp import lib

    inf = lib.info()
    assert inf.gfx950 == 1, f"expected gfx950, got {inf.arch}"
    return torch.device("cuda:0")


def _bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("shape", [(3152, 2304, 768), (3152, 768, 3072), (197, 768, 768), (130, 192, 64), (33, 260, 128), (512, 1, 64)])
def test_gemm_epilogues(dev, precision, shape):
    from mvp import lib, ops
    from mvp.vit import parse_precision

    M, N, K = shape
    pr = parse_precision(precision)
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * 0.05
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    ad, wd = a.to(dev), w.to(dev)
    ap, wp = ops.split_bf16(ad, pr), ops.split_bf16(wd, pr)
    if pr == lib.PREC_BF16:
        a_ref, w_ref, tol = _bf16_round(a).double(), _bf16_round(w).double(), 2e-5
    else:
        a_ref, w_ref, tol = a.double(), w.double(), 5e-5
    base = a_ref @ w_ref.t()
    for act, use_res in ((lib.ACT_NONE, False), (lib.ACT_GELU, False), (lib.ACT_NONE, True), (lib.ACT_RELU, True)):
        ref = base + bias.double()
        if act == lib.ACT_GELU:
            ref = F.gelu(ref)
        elif act == lib.ACT_RELU:
            ref = ref.relu()
        if use_res:
            ref = ref + res.double()
        out = torch.full((M, N), float("nan"), device=dev)
        op = ops.empty_pair((M, N), lib.PREC_BF16X3, dev)
        ops.gemm(ap, wp, M, N, K, bias=bias.to(dev), residual=res.to(dev) if use_res else None, out_f32=out, out=op, act=act, precision=pr)
        torch.cuda.synchronize()
        assert rel_l2(out.cpu().numpy(), ref.numpy()) < tol, (shape, act, use_res)
        pair = op[0].float() + op[1].float()
        assert rel_l2(pair.cpu().numpy(), ref.numpy()) < tol + 2e-5


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_gemm_strided_operands_and_output_slices(dev, precision):
    """Operands that are column slices of wider buffers (lda / ldw > K, non-zero column offset: how the DPT head reads one tap of the
    packed features) and outputs written into column slices (ldo / ldob > N), ragged M and N: the buffer-form staging computes
    per-lane offsets from lda / ldw once per workgroup and must honour all of them."""
    from mvp import lib, ops
    from mvp.vit import parse_precision

    pr = parse_precision(precision)
    g = torch.Generator().manual_seed(77)
    for (M, N, K, LDA, LDW, LDO, aoff, woff, ooff) in ((1000, 200, 128, 512, 320, 264, 128, 64, 8), (77, 512, 256, 256, 1024, 512, 0, 256, 0), (3136, 128, 768, 3072, 768, 512, 1536, 0, 128)):
        abuf, wbuf = torch.randn(M, LDA, generator=g), torch.randn(N, LDW, generator=g) * 0.05
        bias = torch.randn(N, generator=g)
        ap_full, wp_full = ops.split_bf16(abuf.to(dev), pr), ops.split_bf16(wbuf.to(dev), pr)
        ap = (ap_full[0][:, aoff:], ap_full[1][:, aoff:] if ap_full[1] is not None else None)
        wp = (wp_full[0][:, woff:], wp_full[1][:, woff:] if wp_full[1] is not None else None)
        a, w = abuf[:, aoff:aoff + K], wbuf[:, woff:woff + K]
        if pr == lib.PREC_BF16:
            a, w = _bf16_round(a), _bf16_round(w)
        ref = (a.double() @ w.double().t() + bias.double()).relu()
        out = torch.full((M, LDO), float("nan"), device=dev)
        oph = torch.zeros(M, LDO, dtype=torch.bfloat16, device=dev)
        opl = torch.zeros(M, LDO, dtype=torch.bfloat16, device=dev)
        ops.gemm(ap, wp, M, N, K, bias=bias.to(dev), out_f32=out[:, ooff:], out=(oph[:, ooff:], opl[:, ooff:]), act=lib.ACT_RELU, precision=pr,
                 lda=LDA, ldw=LDW, ldo=LDO, ldob=LDO, splitk=1)
        torch.cuda.synchronize()
        got = out[:, ooff:ooff + N].cpu()
        assert rel_l2(got.numpy(), ref.numpy()) < (2e-5 if pr == lib.PREC_BF16 else 5e-5), (M, N, K)
        assert torch.isnan(out[:, :ooff]).all() and torch.isnan(out[:, ooff + N:]).all()  # nothing written outside the slice
        pair = (oph.float() + opl.float())[:, ooff:ooff + N].cpu()
        assert rel_l2(pair.numpy(), ref.numpy()) < 7e-5
        assert (oph[:, :ooff] == 0).all() and (oph[:, ooff + N:] == 0).all()


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_gemm_splitk(dev, precision):
    """Split-K (last-arriving workgroup reduces in a fixed order): parity with fp64 for several split factors and
    both tile widths, bit-reproducible across launches, and shapes alternating on ONE workspace (the tile
    counters must return to zero after every launch)."""
    from mvp import lib, ops
    from mvp.vit import parse_precision

    pr = parse_precision(precision)
    tol = 2e-5 if pr == lib.PREC_BF16 else 5e-5
    cases = []
    for (M, N, K) in ((3152, 768, 3072), (3136, 256, 3072), (777, 1280, 1024), (130, 72, 768)):
        g = torch.Generator().manual_seed(M + N + K)
        a, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.05
        bias, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
        ap, wp = ops.split_bf16(a.to(dev), pr), ops.split_bf16(w.to(dev), pr)
        if pr == lib.PREC_BF16:
            a, w = _bf16_round(a), _bf16_round(w)
        ref = F.gelu(a.double() @ w.double().t() + bias.double()) + res.double()
        cases.append((M, N, K, ap, wp, bias.to(dev), res.to(dev), ref.numpy()))
    for S in (2, 3, 5, 8):
        outs = []
        for rep in range(2):
            for (M, N, K, ap, wp, bias, res, ref) in cases:  # alternate shapes on the shared workspace
                out = torch.full((M, N), float("nan"), device=dev)
                op = ops.empty_pair((M, N), lib.PREC_BF16X3, dev)
                ops.gemm(ap, wp, M, N, K, bias=bias, residual=res, out_f32=out, out=op, act=lib.ACT_GELU, precision=pr, splitk=S)
                torch.cuda.synchronize()
                assert rel_l2(out.cpu().numpy(), ref) < tol, (M, N, K, S)
                assert rel_l2((op[0].float() + op[1].float()).cpu().numpy(), ref) < tol + 2e-5
                outs.append(out)
        n = len(cases)
        for i in range(n):
            assert torch.equal(outs[i], outs[n + i]), "split-K result must be bit-reproducible"
    # invalid: more parts than 64-wide K chunks
    with pytest.raises(lib.MvpError):
        M, N, K, ap, wp, bias, res, ref = cases[3]
        ops.gemm(ap, wp, M, N, K, out_f32=torch.empty(M, N, device=dev), precision=pr, splitk=16)


def test_gemm_row_remap(dev):
    """Patch-embed form: rows written behind a CLS slot, pos-embed residual indexed mod hw."""
    from mvp import lib, ops

    B, hw, C, K = 3, 10, 64, 128
    N = hw + 1
    g = torch.Generator().manual_seed(1)
    a, w = torch.randn(B * hw, K, generator=g), torch.randn(C, K, generator=g) * 0.1
    pos = torch.randn(N, C, generator=g)
    x = torch.zeros(B * N, C, device=dev)
    posd = pos.to(dev)
    ops.gemm(ops.split_bf16(a.to(dev)), ops.split_bf16(w.to(dev)), B * hw, C, K, residual=posd[1:], out_f32=x,
             row_group=hw, row_group_stride=N, row_group_off=1, res_row_mod=hw)
    torch.cuda.synchronize()
    ref = (a.double() @ w.double().t()).reshape(B, hw, C) + pos[1:].double()
    got = x.cpu().reshape(B, N, C)
    assert rel_l2(got[:, 1:].numpy(), ref.numpy()) < 5e-5
    assert got[:, 0].abs().max() == 0


@pytest.mark.parametrize("C", [768, 128, 64, 2048])
def test_layernorm(dev, C):
    from mvp import lib, ops

    M = 301
    g = torch.Generator().manual_seed(C)
    x = torch.randn(M, C, generator=g) * 3 + 1.5
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-6)
    out = ops.empty_pair((M, C), lib.PREC_BF16X3, dev)
    o32 = torch.empty(M, C, device=dev)
    ops.layernorm(x.to(dev), gamma.to(dev), beta.to(dev), out, M, C, 1e-6, out_f32=o32)
    torch.cuda.synchronize()
    assert rel_l2(o32.cpu().numpy(), ref.numpy()) < 2e-6
    assert rel_l2((out[0].float() + out[1].float()).cpu().numpy(), ref.numpy()) < 2e-5
    assert rel_l2(out[0].float().cpu().numpy(), ref.numpy()) < 4e-3  # hi alone is bf16-accurate


def _v_third_as_f16_bf16(qp, C):
    """The V third of a split qkv pair re-written as hi = fp16(v), lo = bf16(v - hi) — what the qkv GEMM's epilogue writes under
    mvp_gemm_args.out_f16_col0 (same arrays: the fp16 bits sit in the bf16-typed hi array)."""
    hi, lo = qp[0].clone(), qp[1].clone()
    v = (qp[0][:, 2 * C:].float() + qp[1][:, 2 * C:].float())
    vh = v.half()
    hi[:, 2 * C:] = vh.view(torch.bfloat16)
    lo[:, 2 * C:] = (v - vh.float()).bfloat16()
    return hi, lo


def _wcomp_pair(y):
    """The compensated WEIGHT-side pair as the qkv GEMM's epilogue computes it (csrc/mvp_common.h, split2_f16_wcomp; fp32 arithmetic):
    hi = fp16(fp32((1 - 2^-6) y)), d = fma(y, 1 - 2^-6, -hi), lo = fp16(fma(d, 8, y / 8)) — each fma stated in fp64 (exact there) and rounded once."""
    y = y.float()
    hi = (y * 0.984375).clamp(-65504.0, 65504.0).half()
    d = (y.double() * 0.984375 - hi.double()).float()                  # fma(y, 1 - 2^-6, -hi): exact in fp64, one rounding to fp32
    lo = (d.double() * 8.0 + y.double() * 0.125).float().clamp(-65504.0, 65504.0).half()  # fma(d, 8, y / 8)
    return hi.view(torch.bfloat16), lo.view(torch.bfloat16)


def _qk_thirds_as_f16_comp(qp, C):
    """Q third -> compensated activation pair, K third -> compensated weight-side pair (mvp_gemm_args.out_f16_col0 = -2C), V as given."""
    from mvp import ops

    hi, lo = qp[0].clone(), qp[1].clone()
    q = qp[0][:, :C].float() + qp[1][:, :C].float()
    k = qp[0][:, C:2 * C].float() + qp[1][:, C:2 * C].float()
    qh, ql = ops.split_f16_comp(q)
    kh, kl = _wcomp_pair(k)
    hi[:, :C], lo[:, :C] = qh, ql
    hi[:, C:2 * C], lo[:, C:2 * C] = kh, kl
    return hi, lo


@pytest.mark.parametrize("precision", ["bf16x3", "bf16x3_vf16", "bf16x3_vf16_qk16", "bf16"])
@pytest.mark.parametrize("BNH", [(2, 197, 12), (1, 1201, 3), (3, 25, 2), (2, 64, 1), (1, 129, 2), (1, 2501, 2)])
def test_attention(dev, precision, BNH):
    """softmax(Q K^T / 8) V against fp64 (ibot_transformers.py:129-145).  bf16x3_vf16 = the form the ViT engine runs since round 4:
    V as hi fp16 + lo bf16, the probabilities held as ONE fp16 value (2^-12 relative each, averaged over the keys) — the measured error
    is printed; the bound is 3e-4 (the bf16-pair probabilities of rounds 1-3: 6e-5)."""
    from mvp import lib, ops
    from mvp.vit import parse_precision

    B, N, H = BNH
    qk16 = precision.endswith("_qk16")  # Q.K^T as two f16 products over compensated fp16 pairs (MVP_ATT_V_F16_QK_F16): same bound as vf16
    vf16 = "_vf16" in precision
    pr = parse_precision(precision.replace("_qk16", "").replace("_vf16", ""))
    C = H * 64
    g = torch.Generator().manual_seed(N)
    qkv = torch.randn(B * N, 3 * C, generator=g)
    qkv[:, :C] *= 2.0  # sharpen the softmax a little
    qd = qkv.to(dev)
    qp = ops.split_bf16(qd, pr)
    if vf16:
        qp = _v_third_as_f16_bf16(qp, C)
    if qk16:
        qp = _qk_thirds_as_f16_comp(qp, C)
    src = (_bf16_round(qkv) if pr == lib.PREC_BF16 else qkv).double()
    t = src.reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    att = ((t[0] @ t[1].transpose(-2, -1)) * 0.125).softmax(-1)
    ref = (att @ t[2]).transpose(1, 2).reshape(B * N, C)
    out = ops.empty_pair((B * N, C), lib.PREC_BF16X3, dev)
    out[0].fill_(float("nan")); out[1].fill_(float("nan"))
    ops.attention(qp, out, B, N, H, 0.125, pr, v_f16=vf16, qk_f16=qk16)
    torch.cuda.synchronize()
    got = (out[0].float() + out[1].float()).cpu()
    assert torch.isfinite(got).all()
    # bf16 mode: P is rounded to bf16 inside the kernel (the reference is not) -> ~2^-9 error
    tol = (3e-4 if vf16 else 6e-5) if pr == lib.PREC_BF16X3 else 4e-3
    err = rel_l2(got.numpy(), ref.numpy())
    print(f"attention {precision} B,N,H={BNH}: rel-L2 vs fp64 {err:.2e} (bound {tol:.0e})")
    assert err < tol, (BNH, precision, err)


@pytest.mark.parametrize("vf16", [False, True])
def test_attention_online_softmax_rescale(dev, vf16):
    """Force the running-max rescale branch: one late key dominates one query row.  (vf16: the running maximum moves only when a row's
    maximum rises by more than 2^6 — here by 128 log2(e) in the fifth tile, for ONE row of the wave; a second spike of +3 exp2 units
    in the third tile stays below the threshold and must be absorbed by probabilities above 1.)"""
    from mvp import lib, ops

    B, N, H = 1, 300, 1
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(B * N, 192, generator=g)
    qkv[5, :64] = 4.0
    qkv[290, 64:128] = 4.0  # key 290 (5th key tile) matches query 5 strongly: score 4*4*64*0.125 = 128
    qkv[9, :64] = 1.0
    qkv[150, 64:128] = 0.9  # key 150 (3rd tile) for query 9: score 0.9*64*0.125 = 7.2 = 10.4 exp2 units... above the other keys' ~+-3
    qp = ops.split_bf16(qkv.to(dev))
    if vf16:
        qp = _v_third_as_f16_bf16(qp, 64)
    t = qkv.double().reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    ref = (((t[0] @ t[1].transpose(-2, -1)) * 0.125).softmax(-1) @ t[2]).transpose(1, 2).reshape(N, 64)
    out = ops.empty_pair((N, 64), lib.PREC_BF16X3, dev)
    ops.attention(qp, out, B, N, H, 0.125, lib.PREC_BF16X3, v_f16=vf16)
    torch.cuda.synchronize()
    got = (out[0].float() + out[1].float()).cpu()
    tol = 3e-4 if vf16 else 6e-5
    assert rel_l2(got.numpy(), ref.numpy()) < tol
    assert rel_l2(got[5].numpy(), ref[5].numpy()) < tol and rel_l2(got[9].numpy(), ref[9].numpy()) < tol


@pytest.mark.parametrize("BNC", [(2, 197, 768), (3, 25, 128), (1, 1201, 768)])
def test_bn_tokens(dev, BNC):
    from mvp import lib, ops
    from oracle import vit as ovit

    B, N, C = BNC
    hw = N - 1
    g = torch.Generator().manual_seed(N)
    x = torch.randn(B, N, C, generator=g) * 2 + torch.randn(C, generator=g) * 30  # |mean| >> std on some channels
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    rm, rv = torch.zeros(C), torch.ones(C)
    ref = ovit.batchnorm_tokens_train(x.double(), gamma.double(), beta.double(), (rm, rv))
    ref_nchw = ref[:, 1:].transpose(1, 2).reshape(B, C, hw)
    M = B * N
    ws = torch.empty(ops.bn_tokens_workspace_bytes(M, C) // 4 + 4, device=dev)
    stats = torch.empty(2 * C, device=dev)
    nchw = torch.empty(B, C, hw, device=dev)
    Mp = (B * hw + 63) // 64 * 64
    tok = ops.zeros_pair((Mp, 2 * C), lib.PREC_BF16X3, dev)
    tokT = ops.zeros_pair((2 * C, Mp), lib.PREC_BF16X3, dev)
    rmd, rvd = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    ops.bn_tokens_to_nchw(x.to(dev), B, N, C, hw, workspace=ws, stats=stats, gamma=gamma.to(dev), beta=beta.to(dev),
                          running_mean=rmd, running_var=rvd, nchw=nchw, tok=tok, ld_tok=2 * C, col_off=C, tokT=tokT, ldT=Mp)
    torch.cuda.synchronize()
    assert rel_l2(nchw.cpu().numpy(), ref_nchw.numpy()) < 2e-5
    assert rel_l2(rmd.cpu().numpy(), rm.numpy()) < 1e-5 and rel_l2(rvd.cpu().numpy(), rv.numpy()) < 1e-5
    flat = ref[:, 1:].reshape(B * hw, C)
    t = (tok[0].float() + tok[1].float()).cpu()
    assert rel_l2(t[: B * hw, C:].numpy(), flat.numpy()) < 3e-5
    assert t[:, :C].abs().max() == 0 and t[B * hw:].abs().max() == 0
    tt = (tokT[0].float() + tokT[1].float()).cpu()
    assert rel_l2(tt[C:, : B * hw].numpy(), flat.t().numpy()) < 3e-5


def test_patch_gather_matches_conv(dev):
    from mvp import lib, ops

    g = torch.Generator().manual_seed(2)
    img = torch.randn(2, 3, 70, 100, generator=g)
    P = 16
    ph, pw = P - 70 % P, P - 100 % P
    gh, gw = (70 + ph) // P, (100 + pw) // P
    out = ops.empty_pair((2 * gh * gw, 3 * P * P), lib.PREC_BF16X3, dev)
    ops.patch_gather(img.to(dev), out, P, gh, gw, ph // 2, pw // 2)
    torch.cuda.synchronize()
    padded = F.pad(img, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2))
    ref = F.unfold(padded, P, stride=P).transpose(1, 2).reshape(2 * gh * gw, -1)
    got = (out[0].float() + out[1].float()).cpu()
    assert rel_l2(got.numpy(), ref.numpy()) < 1e-5


# --------------------------------------------------------------------------- whole backbone
@pytest.mark.parametrize("tag", ["a", "b", "c"])
@pytest.mark.parametrize("precision", ["bf16x3", "f16x2"])
def test_vit_tiny128_vs_reference_golden(dev, tag, precision):
    """Full-tensor parity of the HIP backbone against the REFERENCE's outputs (golden); f16x2 = the opt-in two-product GEMM mode."""
    from mvp.vit import ViTEngine
    from oracle import vit as ovit

    g = load_golden("vit_tiny128.npz")
    sd = ovit.make_vit_weights(embed_dim=128, depth=4, seed=11)
    eng = ViTEngine(sd, heads=2, precision=precision)
    images = torch.from_numpy(g[f"{tag}_images"]).to(dev)
    bn = [dict(weight=torch.ones(128, device=dev), bias=torch.zeros(128, device=dev),
               running_mean=torch.zeros(128, device=dev), running_var=torch.ones(128, device=dev)) for _ in range(4)]
    taps = eng.forward_taps(images, [0, 1, 2, 3], bn=bn)
    torch.cuda.synchronize()
    print(f"\n[vit_tiny128 {tag} {precision}] rel-L2 per tap:", [rel_l2(t.cpu().numpy(), g[f"{tag}_tap{i}"]) for i, t in enumerate(taps)])
    for i, t in enumerate(taps):
        assert t.shape == g[f"{tag}_tap{i}"].shape
        assert rel_l2(t.cpu().numpy(), g[f"{tag}_tap{i}"]) < 1e-3, (tag, i)
        assert rel_l2(bn[i]["running_mean"].cpu().numpy(), g[f"{tag}_rmean{i}"]) < 1e-3
        assert rel_l2(bn[i]["running_var"].cpu().numpy(), g[f"{tag}_rvar{i}"]) < 1e-3
    raw = eng.forward_taps(images, [3], bn_mode=2)
    assert rel_l2(raw[0].cpu().numpy(), g[f"{tag}_raw_last"]) < 1e-3


def _outlier_vit_weights():
    """A tiny ViT bent towards what trained checkpoints do and seeded random weights do not: a residual stream with a few channels in the
    hundreds to thousands ("massive activations": two output rows of block 0's fc2 scaled up, with a large bias), LayerNorm gains of 20 on some
    channels (LayerNorm outputs in the tens to hundreds), 3x larger q / k projections (sharp attention) and 3x larger fc1 weights (hidden
    activations in the tens)."""
    from oracle import vit as ovit

    sd = {k: v.clone() for k, v in ovit.make_vit_weights(embed_dim=128, depth=4, seed=23).items()}
    sd["blocks.0.mlp.fc2.weight"][[7, 70]] *= 300.0
    sd["blocks.0.mlp.fc2.bias"][[7, 70]] = torch.tensor([250.0, -400.0])
    for i in range(4):
        sd[f"blocks.{i}.norm1.weight"][::16] *= 20.0
        sd[f"blocks.{i}.norm2.weight"][5::16] *= 20.0
        sd[f"blocks.{i}.attn.qkv.weight"][:256] *= 3.0
        sd[f"blocks.{i}.mlp.fc1.weight"] *= 3.0
    return sd


def test_vit_with_activation_outliers_vs_oracle(dev):
    """Parity on a network with trained-checkpoint-like outliers (no checkpoint can be fetched here; the reference's goldens are all on seeded
    random weights): the HIP backbone in both arithmetic modes against the fp32 oracle — itself pinned by the reference's goldens — on raw
    (un-normalised) taps, where the outlier channels dominate the norm, and on tap-BN outputs, where every channel counts the same.  Prints the
    extremes the fp16 halves of f16x2 met (its range is +-65504) and both modes' errors; contract 1e-3."""
    from mvp.vit import ViTEngine
    from oracle import vit as ovit

    sd = _outlier_vit_weights()
    images = torch.randn(4, 3, 96, 128, generator=torch.Generator().manual_seed(12))
    with torch.no_grad():
        ref_raw = ovit.vit_dense_features(sd, images, [0, 1, 2, 3], heads=2, add_norm=False)
        ref_bn = ovit.vit_dense_features(sd, images, [0, 1, 2, 3], heads=2, add_norm=True)
    peak = max(float(t.abs().max()) for t in ref_raw)
    assert peak > 500.0, peak  # the outliers are there
    errs = {}
    for precision in ("bf16x3", "f16x2"):
        eng = ViTEngine(sd, heads=2, precision=precision)
        raw = eng.forward_taps(images.to(dev), [0, 1, 2, 3], bn_mode=2)
        bn = [dict(weight=torch.ones(128, device=dev), bias=torch.zeros(128, device=dev), running_mean=torch.zeros(128, device=dev),
                   running_var=torch.ones(128, device=dev)) for _ in range(4)]
        nrm = eng.forward_taps(images.to(dev), [0, 1, 2, 3], bn=bn)
        torch.cuda.synchronize()
        errs[precision] = ([rel_l2(t.cpu().numpy(), r.numpy()) for t, r in zip(raw, ref_raw)], [rel_l2(t.cpu().numpy(), r.numpy()) for t, r in zip(nrm, ref_bn)])
    print(f"\n[vit outliers] residual-stream peak {peak:.0f}; rel-L2 (raw taps | tap-BN outputs): "
          + "; ".join(f"{k}: {[f'{e:.1e}' for e in v[0]]} | {[f'{e:.1e}' for e in v[1]]}" for k, v in errs.items()))
    for k, (a, b) in errs.items():
        assert max(a) < 1e-3 and max(b) < 1e-3, (k, a, b)
    # the two-product mode stays in the three-product mode's error class where the outliers are
    assert max(errs["f16x2"][1]) < 4 * max(errs["bf16x3"][1]) + 1e-5, errs
    # beyond fp16's range the mode saturates silently; its diagnostic switch names the place
    from mvp import lib

    sd2 = {k: v.clone() for k, v in sd.items()}
    sd2["blocks.1.norm2.weight"][3] = 3.0e7  # LayerNorm 2 of block 1: |output| of channel 3 far beyond 65504 (the rows' std is ~170 here)
    eng = ViTEngine(sd2, heads=2, precision="f16x2")
    eng.check_f16_range = True
    with pytest.raises(lib.MvpError, match="block 1: LayerNorm 2 output"):
        eng.forward_taps(images.to(dev), [3], bn_mode=2)
    eng.check_f16_range = False
    out = eng.forward_taps(images.to(dev), [3], bn_mode=2)  # unchecked: finite (saturated), not NaN
    torch.cuda.synchronize()
    assert torch.isfinite(out[0]).all()


@pytest.mark.parametrize("precision,tol", [("bf16x3", 1e-3), ("f16x2", 1e-3), ("bf16", 3e-2)])
def test_vit_base_224_vs_reference_golden(dev, precision, tol):
    """ViT-B/16 @224^2, 4 taps with train-mode BN: sampled elements from the reference.  f16x2 = the opt-in two-product GEMM mode
    (MVP_PREC_F16X2): held to the same 1e-3 feature contract (BASELINE.json north_star); the measured rel-L2 is printed."""
    from mvp.vit import ViTEngine
    from oracle import vit as ovit

    g = load_golden("vit_base.npz")
    seed, B, H, W = [int(v) for v in g["b224_seed"]]
    sd = ovit.make_vit_weights(seed=0)
    eng = ViTEngine(sd, heads=12, precision=precision)
    images = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed)).to(dev)
    taps = eng.forward_taps(images, [2, 5, 8, 11])
    raw = eng.forward_taps(images, [2, 5, 8, 11], bn_mode=2)
    torch.cuda.synchronize()
    errs = []
    for i in range(4):
        idx = torch.from_numpy(g[f"b224_idx{i}"])
        e_t = rel_l2(taps[i].flatten().cpu()[idx].numpy(), g[f"b224_tap{i}_samples"])
        e_r = rel_l2(raw[i].flatten().cpu()[idx].numpy(), g[f"b224_raw{i}_samples"])
        errs.append((e_t, e_r))
        assert abs(taps[i].norm().item() - g[f"b224_tap{i}_moments"][3]) / g[f"b224_tap{i}_moments"][3] < tol
    print(f"\n[vit_base {precision}] rel-L2 (tap, raw) per layer:", errs)
    for e_t, e_r in errs:
        assert e_t < tol and e_r < tol


@pytest.mark.parametrize("qk", ["pair", "f16"])
def test_vit_goldens_with_either_form_of_q_and_k(dev, monkeypatch, qk):
    """MVP_ATT_QK: Q.K^T as three bf16 products over bf16 pairs ("pair") or as two f16 products over compensated fp16 pairs ("f16":
    Q / K written in that form by the qkv GEMM's epilogue, ibot_transformers.py:129-145) — whichever is the default, BOTH hold the reference's
    ViT-B/16 goldens (224^2 and 480x640, f16x2 and bf16x3 GEMMs) to the 1e-3 feature contract; the measured errors are printed."""
    monkeypatch.setenv("MVP_ATT_QK", qk)
    for precision in ("f16x2", "bf16x3"):
        test_vit_base_224_vs_reference_golden(dev, precision, 1e-3)
        test_vit_base_480x640_vs_reference_golden(dev, precision)


@pytest.mark.parametrize("precision", ["bf16x3", "f16x2"])
def test_vit_base_480x640_vs_reference_golden(dev, precision):
    """BASELINE config #2 shape (N = 1201 tokens, pos-embed bicubic interpolation)."""
    from mvp.vit import ViTEngine
    from oracle import vit as ovit

    g = load_golden("vit_base.npz")
    seed, B, H, W = [int(v) for v in g["b480x640_seed"]]
    eng = ViTEngine(ovit.make_vit_weights(seed=0), heads=12, precision=precision)
    images = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed)).to(dev)
    taps = eng.forward_taps(images, [2, 5, 8, 11])
    torch.cuda.synchronize()
    errs = []
    for i in range(4):
        idx = torch.from_numpy(g[f"b480x640_idx{i}"])
        errs.append(rel_l2(taps[i].flatten().cpu()[idx].numpy(), g[f"b480x640_tap{i}_samples"]))
    print(f"\n[vit_base 480x640 {precision}] rel-L2 per tap:", errs)
    assert max(errs) < 1e-3, errs


# ------------------------------------------------------------------------------------------------ round 3: what the bench times
def _gemm_case(dev, M, N, K, seed):
    from mvp import lib, ops

    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * 0.05
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    ap, wp = ops.split_bf16(a.to(dev), lib.PREC_BF16X3), ops.split_bf16(w.to(dev), lib.PREC_BF16X3)
    # fp64 reference on the device (the M = 19k cases are 1e11 flops: seconds on the GPU, minutes on the host)
    ref = (ap[0].double() + ap[1].double()) @ (wp[0].double() + wp[1].double()).t() + bias.to(dev).double()
    return ap, wp, bias.to(dev), res.to(dev), ref


@pytest.mark.parametrize("policy", ["alone", "shared", "pp"])
@pytest.mark.parametrize("shape", [(3152, 2304, 768), (3152, 768, 768), (3152, 3072, 768), (3152, 768, 3072), (19216, 768, 3072), (18912, 2304, 768)])
def test_gemm_tile_policies_at_the_timed_shapes_vs_fp64(dev, policy, shape):
    """Every kernel family the bench can launch for the backbone GEMMs (VERDICT r2 #2a), at the shapes it launches them with:
    MVP_TILES_ALONE (64x64 family), MVP_TILES_SHARED (128x128, 8 waves) — both with the large-M kernel switched off so that the tile
    kernels themselves are measured — and mvp_gemm_pp (256x256 ping-pong).  Against fp64 (<= 5e-5 rel-L2) with the fused epilogues the
    ViT uses (bias; bias + GELU -> pair; bias + residual -> fp32), and all three bit-identical to one another (same k order)."""
    import ctypes as C

    from mvp import lib, ops

    M, N, K = shape
    ap, wp, bias, res, ref = _gemm_case(dev, M, N, K, M + N + K)
    so = lib.load()
    for act, use_res in ((lib.ACT_NONE, False), (lib.ACT_GELU, False), (lib.ACT_NONE, True)):
        r = ref
        if act == lib.ACT_GELU:
            r = F.gelu(r)
        if use_res:
            r = r + res.double()
        outs = {}
        for pol in ("alone", policy):
            out = torch.full((M, N), float("nan"), device=dev)
            op = ops.empty_pair((M, N), lib.PREC_BF16X3, dev)
            a = lib.GemmArgs(lib.ptr(ap[0]), lib.ptr(ap[1]), lib.ptr(wp[0]), lib.ptr(wp[1]), lib.ptr(bias), lib.ptr(res) if use_res else None,
                             lib.ptr(out), lib.ptr(op[0]), lib.ptr(op[1]), M, N, K, K, K, N, N, N, act, lib.PREC_BF16X3, 0, 0, 0, 0)
            a.tile_policy = {"alone": lib.TILES_NO_PP, "shared": lib.TILES_SHARED | lib.TILES_NO_PP, "pp": 0}[pol]
            lib.check((so.mvp_gemm_pp if pol == "pp" else so.mvp_gemm_bias_act_res)(C.byref(a), lib.stream_ptr()), pol)
            torch.cuda.synchronize()
            d = out.double() - r
            assert (d.norm() / r.norm()).item() < 5e-5, (shape, pol, act, use_res)
            d = op[0].double() + op[1].double() - r
            assert (d.norm() / r.norm()).item() < 7e-5
            outs[pol] = (out, op)
        assert torch.equal(outs[policy][0], outs["alone"][0]) and torch.equal(outs[policy][1][0], outs["alone"][1][0]) and torch.equal(outs[policy][1][1], outs["alone"][1][1])


@pytest.mark.parametrize("shape", [(21670, 2304, 768), (43900, 768, 160), (17000, 1800, 96), (9000, 516, 224), (70000, 264, 64)])
def test_gemm_pp_tile_loop_and_wide_epilogues_equal_the_tile_kernels(dev, shape):
    """Round 4: the large-M kernel is persistent over tiles (grid = CUs; the next tile's first k-step is fetched ahead of the current
    tile's epilogue stores) and its wide epilogues are branch-free buffer stores.  With more tiles than CUs (765 / 516 / 536 / 1096),
    a ragged last row tile, N ragged against 256 (1800), N % 8 != 0 (516: the generic epilogue inside the tile loop) and odd k-step
    counts (K = 160, 96, 224: 5, 3, 7 steps), in the output forms the ViT blocks use — pair only (qkv, fc1 + GELU), fp32 + residual
    (proj, fc2), fp32 only — the results are the tile kernels' bit for bit (which the other tests hold to fp64), and a second launch
    reproduces the first."""
    import ctypes as C

    from mvp import lib, ops

    M, N, K = shape
    ap, wp, bias, res, ref = _gemm_case(dev, M, N, K, 11 + M + N)
    so = lib.load()
    forms = (("pair", lib.ACT_NONE, False), ("pair", lib.ACT_GELU, False), ("f32", lib.ACT_NONE, True), ("f32", lib.ACT_GELU, False), ("f32", lib.ACT_NONE, False))
    for form, act, use_res in forms:
        r = ref
        if act == lib.ACT_GELU:
            r = F.gelu(r)
        if use_res:
            r = r + res.double()
        outs = {}
        for pol in ("tile", "pp", "pp_again"):
            out = torch.full((M, N), float("nan"), device=dev) if form == "f32" else None
            op = ops.empty_pair((M, N), lib.PREC_BF16X3, dev) if form == "pair" else None
            if op is not None:
                op[0].fill_(float("nan")); op[1].fill_(float("nan"))
            a = lib.GemmArgs(lib.ptr(ap[0]), lib.ptr(ap[1]), lib.ptr(wp[0]), lib.ptr(wp[1]), lib.ptr(bias), lib.ptr(res) if use_res else None,
                             lib.ptr(out), lib.ptr(op[0]) if op else None, lib.ptr(op[1]) if op else None, M, N, K, K, K, N, N, N, act, lib.PREC_BF16X3, 0, 0, 0, 0)
            a.tile_policy = lib.TILES_NO_PP if pol == "tile" else 0
            lib.check((so.mvp_gemm_bias_act_res if pol == "tile" else so.mvp_gemm_pp)(C.byref(a), lib.stream_ptr()), pol)
            torch.cuda.synchronize()
            val = out.double() if out is not None else op[0].double() + op[1].double()
            assert ((val - r).norm() / r.norm()).item() < 7e-5, (shape, pol, form, act, use_res)
            outs[pol] = (out, op)
        for pol in ("pp", "pp_again"):
            if form == "f32":
                assert torch.equal(outs[pol][0], outs["tile"][0]), (shape, pol, form, act, use_res)
            else:
                assert torch.equal(outs[pol][1][0], outs["tile"][1][0]) and torch.equal(outs[pol][1][1], outs["tile"][1][1]), (shape, pol, form, act)


@pytest.mark.parametrize("shape", [(3152, 2304, 768), (3152, 768, 3072), (21670, 3072, 768), (21670, 768, 768), (700, 768, 128)])
def test_gemm_two_product_mode_vs_fp64_and_across_kernel_families(dev, shape):
    """MVP_PREC_F16X2 (opt-in): two f16 MFMAs per fragment pair over the compensated fp16 pairs of include/mvp_hip.h (activation
    hi = fp16(a), lo = fp16(8 (a - hi) + hi / 8); weight hi = fp16((1 - 2^-6) w), lo = fp16((w + 64 d) / 8)).  Against fp64 of the fp32
    operands: what is left is (a - hi) * 64 d and the roundings of the two lo halves — <= 2e-5 rel-L2 asserted (the three-product mode:
    ~5e-6 to 1e-5; one fp16 rounding of the weights would be 2e-4) — printed.  The tile kernels and the large-M kernel (separate and
    interleaved operands, interleaved output, compensated output columns) return the same bits, as in the three-product mode."""
    import ctypes as C

    from mvp import lib, ops

    M, N, K = shape
    g = torch.Generator().manual_seed(M + N)
    a = torch.randn(M, K, generator=g).to(dev)
    w = (torch.randn(N, K, generator=g) * 0.05).to(dev)
    bias, res = torch.randn(N, generator=g).to(dev), torch.randn(M, N, generator=g).to(dev)
    ap, wp = ops.split_f16_comp(a), ops.f16x2_weight(w)

    def decode(pair):  # hi + (lo - hi / 8) / 8
        h = pair[0].view(torch.float16).double()
        return h + (pair[1].view(torch.float16).double() - h / 8) / 8

    assert ((decode(ap) - a.double()).abs().max() / a.abs().max()).item() < 2 ** -16  # the activation pair carries ~17 bits of a
    ref = a.double() @ w.double().t() + bias.double()
    so = lib.load()
    for form, act, use_res in (("pair", lib.ACT_GELU, False), ("f32", lib.ACT_NONE, True)):
        r = F.gelu(ref) if act == lib.ACT_GELU else ref
        if use_res:
            r = r + res.double()
        outs = {}
        for pol in ("tile", "pp", "pp_ilv"):
            if pol == "pp_ilv" and K % 32:
                continue
            out = torch.full((M, N), float("nan"), device=dev) if form == "f32" else None
            op = ops.empty_pair((M, N), lib.PREC_BF16X3, dev) if form == "pair" else None
            ai = ops.interleave_pair(ap) if pol == "pp_ilv" else None
            wi = ops.interleave_pair(wp) if pol == "pp_ilv" else None
            args = lib.GemmArgs(lib.ptr(ai if ai is not None else ap[0]), None if ai is not None else lib.ptr(ap[1]),
                                lib.ptr(wi if wi is not None else wp[0]), None if wi is not None else lib.ptr(wp[1]), lib.ptr(bias),
                                lib.ptr(res) if use_res else None, lib.ptr(out), lib.ptr(op[0]) if op else None, lib.ptr(op[1]) if op else None,
                                M, N, K, 2 * K if ai is not None else K, 2 * K if wi is not None else K, N, N, N, act, lib.PREC_F16X2, 0, 0, 0, 0)
            args.pair_layout = 3 if pol == "pp_ilv" else 0
            args.tile_policy = lib.TILES_NO_PP if pol == "tile" else 0
            args.out_f16_col0 = -1 if form == "pair" else 0  # the pair leaves as the next GEMM's activation operand (fc1's output in this mode)
            lib.check((so.mvp_gemm_bias_act_res if pol == "tile" else so.mvp_gemm_pp)(C.byref(args), lib.stream_ptr()), pol)
            torch.cuda.synchronize()
            val = out.double() if out is not None else decode(op)
            err = ((val - r).norm() / r.norm()).item()
            if pol == "tile":
                print(f"\n[gemm f16x2 M,N,K={shape} {form}] rel-L2 vs fp64: {err:.2e}")
            assert err < 2e-5, (shape, pol, form, err)
            outs[pol] = (out, op)
        for pol in outs:
            if form == "f32":
                assert torch.equal(outs[pol][0], outs["tile"][0]), (shape, pol, form)
            else:
                assert torch.equal(outs[pol][1][0], outs["tile"][1][0]) and torch.equal(outs[pol][1][1], outs["tile"][1][1]), (shape, pol, form)


@pytest.mark.parametrize("shape", [(1000, 256, 64), (3001, 1024, 256), (65500, 256, 64), (140000, 512, 128), (70000, 64, 256), (200000, 128, 64)])
def test_universal_epilogue_bits_equal_the_row_guarded_one(dev, shape):
    """gemm_epilogue_uni (round 4: branch-free buffer loads / stores, next unit's loads ahead of this unit's stores) against gemm_epilogue
    (rows guarded by branches) on the forms the ResNet-50 trunk, the DPT probe and the ViT use: ReLU -> pair; pair residual + ReLU after it ->
    pair + fp32 (ResNet identities, dino_res50.py:83-101); stored-gate backward (mask_mode 2 and 1); ReLU with its byte mask out; fp32
    residual + GELU.  Same launches with MVP_TILES_NO_UNI switched on and off, on the 128-column tile kernels and on the large-M kernel:
    every output (fp32, pair halves, mask bytes) bit for bit, ragged last row tile included.  Shapes: 64x64 tiles (no 64-column wave
    tile: the guarded epilogue either way), 128x128 tiles (universal), the large-M kernel with one tile per workgroup (256 tiles) and with
    its tile loop (1094 tiles: the next tile's operands are fetched under the universal epilogue)."""
    import ctypes as C

    from mvp import lib, ops

    M, N, K = shape
    g = torch.Generator().manual_seed(M + 7 * N)
    a = torch.randn(M, K, generator=g).to(dev)
    w = (torch.randn(N, K, generator=g) * 0.1).to(dev)
    ap, wp = ops.split_bf16(a, 3), ops.split_bf16(w, 3)
    bias = torch.randn(N, generator=g).to(dev)
    res = torch.randn(M, N, generator=g).to(dev)
    rp = ops.split_bf16(torch.randn(M, N, generator=g).to(dev), 3)
    gate = (torch.rand(M, N, generator=g) > 0.4).to(torch.uint8).to(dev)
    so = lib.load()
    forms = {
        "relu_pair": dict(act=lib.ACT_RELU, pair=True),
        "respair_relu_after": dict(act=lib.ACT_RELU, pair=True, f32=True, respair=True, act_after=True),
        "respair_hi_only": dict(act=lib.ACT_RELU, pair=True, respair="hi", act_after=True),
        "gate2_f32": dict(f32=True, gate=2),
        "gate1_both": dict(f32=True, pair=True, gate=1, res=True),
        "relu_mask_out": dict(act=lib.ACT_RELU, pair=True, f32=True, omask=True),
        "relu_after_mask_out": dict(act=lib.ACT_RELU, pair=True, omask=True, res=True, act_after=True),
        "res_gelu_pair": dict(act=lib.ACT_GELU, pair=True, res=True),
    }
    for name, f in forms.items():
        outs = {}
        for pol_name, pol in (("tile_generic", lib.TILES_NO_PP | lib.TILES_NO_UNI), ("tile_uni", lib.TILES_NO_PP), ("pp_uni", 0)):
            o32 = torch.full((M, N), float("nan"), device=dev) if f.get("f32") else None
            op = ops.empty_pair((M, N), 3, dev) if f.get("pair") else None
            if op is not None:
                op[0].fill_(float("nan")); op[1].fill_(float("nan"))
            om = torch.full((M, N), 77, dtype=torch.uint8, device=dev) if f.get("omask") else None
            args = lib.GemmArgs(lib.ptr(ap[0]), lib.ptr(ap[1]), lib.ptr(wp[0]), lib.ptr(wp[1]), lib.ptr(bias), lib.ptr(res) if f.get("res") else None,
                                lib.ptr(o32), lib.ptr(op[0]) if op else None, lib.ptr(op[1]) if op else None, M, N, K, K, K, N, N, N,
                                f.get("act", lib.ACT_NONE), lib.PREC_BF16X3, 0, 0, 0, 0)
            if f.get("gate"):
                args.relu_mask, args.mask_mode, args.ldm = lib.ptr(gate), f["gate"], N
            if om is not None:
                args.out_mask, args.ldm = lib.ptr(om), N
            if f.get("respair"):
                args.residual_hi = lib.ptr(rp[0])
                args.residual_lo = None if f["respair"] == "hi" else lib.ptr(rp[1])
            args.act_after_res = int(bool(f.get("act_after")))
            args.tile_policy = pol
            # ("pp_uni": the large-M kernel called directly — the dispatcher keeps masked / pair-residual plain GEMMs on the tile kernels)
            lib.check((so.mvp_gemm_pp if pol_name == "pp_uni" else so.mvp_gemm_bias_act_res)(C.byref(args), lib.stream_ptr()), f"{name}/{pol_name}")
            torch.cuda.synchronize()
            outs[pol_name] = (o32, op, om)
        ref = outs["tile_generic"]
        if ref[0] is not None:
            assert torch.isfinite(ref[0]).all()
        for pol_name in ("tile_uni", "pp_uni"):
            got = outs[pol_name]
            if ref[0] is not None:
                assert torch.equal(got[0], ref[0]), (shape, name, pol_name, "f32")
            if ref[1] is not None:
                assert torch.equal(got[1][0], ref[1][0]) and torch.equal(got[1][1], ref[1][1]), (shape, name, pol_name, "pair")
            if ref[2] is not None:
                assert torch.equal(got[2], ref[2]), (shape, name, pol_name, "mask")


@pytest.mark.parametrize("shape", [(18912, 3072, 768), (5000, 768, 3072), (300, 512, 96)])
def test_gemm_pp_interleaved_layouts_match_separate(dev, shape):
    """mvp_gemm_args.pair_layout / out_pair_layout: the large-M kernel on hi|lo-interleaved A and / or W operands, and writing an
    interleaved output pair, returns exactly the bits it returns on separate arrays (ragged M and N included).  mvp_gemm_pp is called
    directly: at the two smaller shapes the dispatch rule picks the tile kernels for separate operands."""
    import ctypes as C

    from mvp import lib, ops

    M, N, K = shape
    ap, wp, bias, res, ref = _gemm_case(dev, M, N, K, 5 + M)
    ai = ops.IlvPair(M, K, dev)
    ai.t.copy_(ops.interleave_pair(ap))
    wi = ops.interleave_pair(wp)
    assert torch.equal(ai.separate()[0], ap[0]) and torch.equal(ai.separate()[1], ap[1])
    assert ops.gemm_tile(M, N, K).startswith("pp ") == (shape == (18912, 3072, 768))
    so = lib.load()

    def run(a_ilv, w_ilv, o_ilv):
        out = ops.IlvPair(M, N, dev) if o_ilv else None
        sep = None if o_ilv else ops.empty_pair((M, N), lib.PREC_BF16X3, dev)
        if o_ilv:
            out.t.fill_(float("nan"))
        args = lib.GemmArgs(lib.ptr(ai.t if a_ilv else ap[0]), None if a_ilv else lib.ptr(ap[1]), lib.ptr(wi if w_ilv else wp[0]),
                            None if w_ilv else lib.ptr(wp[1]), lib.ptr(bias), None, None, lib.ptr(out.t if o_ilv else sep[0]),
                            None if o_ilv else lib.ptr(sep[1]), M, N, K, 2 * K if a_ilv else K, 2 * K if w_ilv else K, N, N,
                            2 * N if o_ilv else N, lib.ACT_GELU, lib.PREC_BF16X3, 0, 0, 0, 0)
        args.pair_layout = (lib.PAIR_A_ILV32 if a_ilv else 0) | (lib.PAIR_W_ILV32 if w_ilv else 0)
        args.out_pair_layout = lib.PAIR_A_ILV32 if o_ilv else lib.PAIR_SEPARATE
        if a_ilv or w_ilv:  # an interleaved operand: the dispatcher itself would send this call to the large-M kernel
            r = lib.GemmRoute()
            assert so.mvp_gemm_route(C.byref(args), C.byref(r)) == 0 and r.family == lib.ROUTE_PP, (shape, a_ilv, w_ilv, o_ilv)
        lib.check(so.mvp_gemm_pp(C.byref(args), lib.stream_ptr()), "mvp_gemm_pp")
        torch.cuda.synchronize()
        return out.separate() if o_ilv else sep

    base = run(False, False, False)
    for a_ilv, w_ilv, o_ilv in ((True, False, False), (False, True, False), (True, True, False), (True, True, True), (False, False, True)):
        got = run(a_ilv, w_ilv, o_ilv)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), (shape, a_ilv, w_ilv, o_ilv)
    r = F.gelu(ref)
    assert ((base[0].double() + base[1].double() - r).norm() / r.norm()).item() < 7e-5


def test_f16_pairs_saturate_instead_of_overflowing(dev):
    """The fp16 forms of a pair hold FINITE halves for values beyond fp16's range.  The compensated activation pair (LayerNorm out_f16):
    hi = +-65504 and a finite lo — the value is wrong there (documented range of MVP_PREC_F16X2) but a GEMM over such a row stays finite;
    inside the range hi + (lo - hi / 8) / 8 returns the value to 2^-16.  The fp16-hi / bf16-lo form of the V third (a GEMM epilogue's
    out_f16_col0 > 0): hi = 65504 and the excess in lo (bf16: fp32's exponent range), so hi + lo still carries the value to bf16's 8 bits."""
    import ctypes as C

    from mvp import lib, ops

    M, Cd = 64, 256
    g = torch.Generator().manual_seed(3)
    x = torch.randn(M, Cd, generator=g)
    gam = torch.ones(Cd)
    gam[5] = 3.0e5  # LayerNorm output column 5 = (x - mean) * rstd * 3e5: far beyond 65504
    out = ops.empty_pair((M, Cd), lib.PREC_BF16X3, dev)
    o32 = torch.empty(M, Cd, device=dev)
    ops.layernorm(x.to(dev), gam.to(dev), torch.zeros(Cd).to(dev), out, M, Cd, 1e-6, out_f32=o32, out_f16=True)
    torch.cuda.synchronize()
    hi, lo = out[0].view(torch.float16).float(), out[1].view(torch.float16).float()
    assert torch.isfinite(hi).all() and torch.isfinite(lo).all() and hi.abs().max().item() == 65504.0
    big = o32.abs() > 65504
    assert big.any()
    val = hi + (lo - hi / 8) / 8
    assert ((val - o32).abs()[~big] / o32.abs()[~big].clamp_min(1e-3)).max().item() < 2 ** -16
    ref = ops.split_f16_comp(o32)  # (the torch statement of the same form)
    assert torch.equal(ref[0], out[0]) and torch.equal(ref[1], out[1])
    # the V form: identity GEMM of a matrix with outliers, columns >= 64 written fp16-hi / bf16-lo
    K = N = 128
    a = torch.randn(M, K, generator=g)
    a[:, 70] *= 1.0e5
    ap, wp = ops.split_bf16(a.to(dev), 3), ops.split_bf16(torch.eye(N).to(dev), 3)
    op = ops.empty_pair((M, N), lib.PREC_BF16X3, dev)
    args = lib.GemmArgs(lib.ptr(ap[0]), lib.ptr(ap[1]), lib.ptr(wp[0]), lib.ptr(wp[1]), None, None, None, lib.ptr(op[0]), lib.ptr(op[1]), M, N, K, K, K, N, N, N,
                        lib.ACT_NONE, lib.PREC_BF16X3, 0, 0, 0, 0)
    args.out_f16_col0 = 64
    lib.check(lib.load().mvp_gemm_bias_act_res(C.byref(args), lib.stream_ptr()), "gemm")
    torch.cuda.synchronize()
    hi, lo = op[0][:, 64:].view(torch.float16).float(), op[1][:, 64:].float()
    av = a[:, 64:].to(dev)
    big = av.abs() > 65504
    assert big.any() and torch.isfinite(hi).all() and torch.isfinite(lo).all() and hi.abs().max().item() == 65504.0
    assert ((hi + lo - av).abs()[big] / av.abs()[big]).max().item() < 2 ** -8
    assert ((hi + lo - av).abs()[~big] / av.abs()[~big].clamp_min(1e-3)).max().item() < 1e-5


@pytest.mark.parametrize("prec", ["bf16x3", "f16x2"])
def test_qkv_epilogue_writes_q_k_v_in_their_attention_forms(dev, prec):
    """mvp_gemm_args.out_f16_col0 = -2C (the fused qkv projection for MVP_ATT_V_F16_QK_F16): the Q third leaves as the compensated
    activation pair, the K third as the compensated weight-side pair, the V third as fp16 hi + bf16 lo — each bit for bit the torch statement
    of its form applied to the fp32 output of the same GEMM, from the large-M kernel (tile loop, ragged last row tile) and from the tile kernels
    alike (serial loop = pipelined loop), and hi + lo / 8 of the K third returns the value to 2^-16."""
    from mvp import lib, ops

    M, C, K = 17000, 256, 128  # 67 x 3 tiles of 256 x 256 > 256 CUs: the persistent tile loop runs; N = 3C = 768
    g = torch.Generator().manual_seed(77)
    a = torch.randn(M, K, generator=g).to(dev)
    w = (torch.randn(3 * C, K, generator=g) * 0.3).to(dev)
    bias = torch.randn(3 * C, generator=g).to(dev)
    if prec == "f16x2":
        ap, wp, pr = ops.split_f16_comp(a), tuple(t.to(dev) for t in ops.f16x2_weight(w)), lib.PREC_F16X2
    else:
        ap, wp, pr = ops.split_bf16(a), ops.split_bf16(w), lib.PREC_BF16X3
    import ctypes as CT

    so, outs = lib.load(), {}
    N = 3 * C
    for fam in ("pp", "tiles"):
        o32 = torch.empty(M, N, device=dev)
        op = ops.empty_pair((M, N), lib.PREC_BF16X3, dev)
        for f32 in (True, False):
            args = lib.GemmArgs(lib.ptr(ap[0]), lib.ptr(ap[1]), lib.ptr(wp[0]), lib.ptr(wp[1]), lib.ptr(bias), None, lib.ptr(o32) if f32 else None,
                                None if f32 else lib.ptr(op[0]), None if f32 else lib.ptr(op[1]), M, N, K, K, K, N, N, N, lib.ACT_NONE, pr, 0, 0, 0, 0)
            args.tile_policy = lib.TILES_NO_PP if fam == "tiles" else 0
            args.out_f16_col0 = 0 if f32 else -2 * C
            lib.check((so.mvp_gemm_bias_act_res if fam == "tiles" else so.mvp_gemm_pp)(CT.byref(args), lib.stream_ptr()), fam)
        torch.cuda.synchronize()
        outs[fam] = (o32, op)
    (y, (hi, lo)), (y2, (hi2, lo2)) = outs["pp"], outs["tiles"]
    assert torch.equal(y, y2) and torch.equal(hi, hi2) and torch.equal(lo, lo2)
    qh, ql = ops.split_f16_comp(y[:, :C])
    assert torch.equal(hi[:, :C], qh) and torch.equal(lo[:, :C], ql)
    kh, kl = _wcomp_pair(y[:, C:2 * C])
    assert torch.equal(hi[:, C:2 * C], kh) and torch.equal(lo[:, C:2 * C], kl)
    vh = y[:, 2 * C:].half()
    assert torch.equal(hi[:, 2 * C:], vh.view(torch.bfloat16)) and torch.equal(lo[:, 2 * C:], (y[:, 2 * C:] - vh.float()).bfloat16())
    kv = y[:, C:2 * C]
    rec = kh.view(torch.float16).float() + kl.view(torch.float16).float() / 8
    assert ((rec - kv).abs() / kv.abs().clamp_min(1e-2)).max().item() < 2 ** -16


def test_layernorm_and_attention_interleaved_outputs_match_separate(dev):
    """LayerNorm and attention writing their output pair hi|lo-interleaved (the A operand of the large-M GEMM) = the separate pair, bit for bit."""
    from mvp import lib, ops

    g = torch.Generator().manual_seed(9)
    M, Cd = 1000, 768
    x = torch.randn(M, Cd, generator=g).to(dev)
    gam, bet = torch.randn(Cd, generator=g).to(dev), torch.randn(Cd, generator=g).to(dev)
    sep = ops.empty_pair((M, Cd), lib.PREC_BF16X3, dev)
    ilv = ops.IlvPair(M, Cd, dev)
    ops.layernorm(x, gam, bet, sep, M, Cd, 1e-6)
    ops.layernorm(x, gam, bet, ilv, M, Cd, 1e-6)
    torch.cuda.synchronize()
    assert torch.equal(ilv.separate()[0], sep[0]) and torch.equal(ilv.separate()[1], sep[1])
    for B, N in ((3, 197), (2, 300)):  # the LDS-resident kernel and the streaming one
        H = 12
        qkv = ops.split_bf16(torch.randn(B * N, 3 * H * 64, generator=g).to(dev), lib.PREC_BF16X3)
        sep = ops.empty_pair((B * N, H * 64), lib.PREC_BF16X3, dev)
        ilv = ops.IlvPair(B * N, H * 64, dev)
        ops.attention(qkv, sep, B, N, H, 0.125, lib.PREC_BF16X3)
        ops.attention(qkv, ilv, B, N, H, 0.125, lib.PREC_BF16X3)
        torch.cuda.synchronize()
        assert torch.equal(ilv.separate()[0], sep[0]) and torch.equal(ilv.separate()[1], sep[1]), (B, N)


@pytest.mark.parametrize("case", ["fwd_relu_mask", "dgrad_gate", "dgrad_gate_f32_only", "residuals", "upsampled_input"])
def test_conv_on_the_large_m_kernel_equals_the_tile_kernels(dev, case):
    """3x3 convolutions big enough for the large-M ping-pong kernel (csrc/gemm_pp.hip CONV mode: >= 512 tiles of 256x256, K >= 1024 —
    the DPT probe's layers at 8x the token grid, probes.py:384-398) against the 128x128 tile kernels (``tile_policy`` TILES_NO_PP),
    which the DPT tests hold to the oracle: same k order, same epilogue, so bit-identical — with the fused epilogues the DPT forward /
    backward use (ReLU + gate mask out, gated by a stored mask, two residuals, a virtually 2x-upsampled input) — plus a spot check of
    output pixels against a direct fp64 evaluation."""
    from mvp import conv as cv, lib, ops

    g = torch.Generator().manual_seed(42)
    B, H, W, C, N = 2, 192, 192, 128, 512
    up = 1 if case == "upsampled_input" else 0
    Hs, Ws = H >> up, W >> up
    x = torch.randn(B * Hs * Ws, C, generator=g).to(dev)
    w = (torch.randn(N, C, 3, 3, generator=g) * 0.05).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    xP = ops.split_bf16(x, 3)
    geo = cv.geom(B, H, W, C, 3, 3, 1, 1, up=up)
    M = B * H * W
    wk = cv.pack_weight(w, 0, 3)
    kw = dict(bias=bias, precision=3)
    if case == "fwd_relu_mask":
        kw.update(act=lib.ACT_RELU)
    elif case in ("dgrad_gate", "dgrad_gate_f32_only"):  # (fp32 output only: the gated wide epilogue, gemm_epilogue_wide<..., GATE>)
        kw.update(relu_mask=(torch.rand(M, N, generator=g) > 0.4).to(torch.uint8).to(dev), mask_mode=2)
    elif case == "residuals":
        kw.update(act=lib.ACT_RELU, residual=torch.randn(M, N, generator=g).to(dev), residual2=torch.randn(M, N, generator=g).to(dev))

    def run(policy):
        o32 = torch.empty(M, N, dtype=torch.float32, device=dev)
        oP = ops.empty_pair((M, N), 3, dev) if case != "dgrad_gate_f32_only" else None
        om = torch.zeros(M, N, dtype=torch.uint8, device=dev) if case == "fwd_relu_mask" else None
        cv.conv_gemm(xP, geo, wk, N, out_f32=o32, out=oP, out_mask=om, tile_policy=policy, **kw)
        return o32, oP, om

    a = run(0)
    b = run(lib.TILES_NO_PP)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0])
    if a[1] is not None:
        assert torch.equal(a[1][0], b[1][0]) and torch.equal(a[1][1], b[1][1])
    if a[2] is not None:
        assert torch.equal(a[2], b[2])
    if case == "fwd_relu_mask":  # direct fp64 evaluation of a few pixels (borders included)
        x4 = x.double().view(B, Hs, Ws, C)
        for (bi, y, xx) in [(0, 0, 0), (1, H - 1, W - 1), (0, 17, 0), (1, 100, 57)]:
            acc = bias.double().clone()
            for ky in range(3):
                for kx in range(3):
                    yy, xc = y + ky - 1, xx + kx - 1
                    if 0 <= yy < H and 0 <= xc < W:
                        acc += w[:, :, ky, kx].double() @ x4[bi, yy >> up, xc >> up]
            ref = acc.clamp_min(0)
            got = a[0][(bi * H + y) * W + xx].double()
            assert float((got - ref).abs().max()) < 2e-4 * float(ref.abs().max() + 1)
