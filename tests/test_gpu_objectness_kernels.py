"""The three objectness kernels (csrc/objectness.hip) against the fp64 restatement (tests/objectness_ref.py) on the same fp32 inputs.

Bounds.  These are fp32 element-wise kernels whose reductions run in fp64 over at most 1e5 terms: an element carries a few ulp
(exp, a divide, three or four multiplies: ~5e-7 relative at worst), a reduced scalar the same after averaging.  The bound is rel-L2 <= 1e-5
for y, grad_x, dgamma, dbeta, the loss and grad_pred, rtol 1e-5 for the running statistics, exact equality for the counts and for a
second launch on the same inputs.  Every figure is printed before it is asserted (pytest -s shows them; profiles/objectness_step.txt
records the maxima of one run)."""
import numpy as np
import pytest
import torch

import objectness_ref as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu

TOL = 1e-5
ACTS = {"none": 0, "sigmoid": 1, "tanh": 2}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rows(x_nchw, ld, dev):
    """[B, C, H, W] fp32 -> the channels-last [P, ld] device map with NaN in the padding columns."""
    B, C, H, W = x_nchw.shape
    rows = torch.full((B * H * W, ld), float("nan"), dtype=torch.float32)
    rows[:, :C] = x_nchw.permute(0, 2, 3, 1).reshape(-1, C)
    return rows.to(dev)


def _bn_case(dev, B, HW, C, ld, act, training, n_factor, x, seed):
    """Forward + backward of one configuration, twice; returns the worst relative figure."""
    from mvp import ops

    g = torch.Generator().manual_seed(seed)
    P = B * HW
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    # (running statistics on the side of the batch mean, so that their update adds terms of one sign and rtol means something)
    rm0, rv0 = torch.sign(x.mean()) * (torch.rand(C, generator=g) * 0.2 + 0.1), torch.rand(C, generator=g) + 0.5
    # The upstream gradient has a mean and a part along the centred input, so that dbeta = sum g_z and dgamma = sum g_z xhat are sums of
    # mostly one sign: a relative bound on a sum that happens to cancel (64 random signed terms do, now and then) would measure the
    # cancellation, not the kernel.
    xc = x - x.mean(dim=(0, 2, 3), keepdim=True)
    gy = torch.randn(B, C, HW, 1, generator=g) + 0.5 + 0.5 * xc / xc.pow(2).mean(dim=(0, 2, 3), keepdim=True).sqrt().clamp_min(1e-12)
    xr = _rows(x, ld, dev)
    sig = act == "sigmoid"
    worst = 0.0
    outs = []
    for _ in range(2):
        rm, rv, nbt = rm0.clone().to(dev), rv0.clone().to(dev), torch.tensor([7], dtype=torch.int64, device=dev)
        y = torch.full((B, C, HW, 1), float("nan"), device=dev)
        stats = torch.zeros(3 * C, device=dev)
        ws = ops.bn_act_workspace(dev)
        kw = dict(gamma=gamma.to(dev), beta=beta.to(dev), stats=stats, workspace=ws) if sig else {}
        ops.bn_act_fwd(xr, y, B, HW, C, ld, ACTS[act], training, running_mean=rm if sig else None, running_var=rv if sig else None,
                       num_batches_tracked=nbt if sig else None, n=n_factor * P, **kw)
        gx = torch.full((P, ld), float("nan"), device=dev)
        dg, db = torch.full((C,), float("nan"), device=dev), torch.full((C,), float("nan"), device=dev)
        ops.bn_act_bwd(xr, gy.to(dev), gx, B, HW, C, ld, ACTS[act], training, grad_gamma=dg if sig else None, grad_beta=db if sig else None, **kw)
        torch.cuda.synchronize()
        outs.append([t.cpu() for t in (y, stats, rm, rv, nbt, gx, dg, db)])
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), "two launches differ"
    y, stats, rm, rv, nbt, gx, dg, db = outs[0]
    f = R.bn_act_fwd(x.numpy(), gamma.numpy(), beta.numpy(), rm0.numpy(), rv0.numpy(), act=act, training=training, n=n_factor * P)
    b = R.bn_act_bwd(x.numpy(), gy.numpy(), gamma.numpy(), beta.numpy(), rm0.numpy(), rv0.numpy(), act=act, training=training)
    figs = {"y": rel_l2(y.numpy(), f["y"])}
    gxv = gx.view(B, HW, 1, ld).permute(0, 3, 1, 2)  # [B, ld, HW, 1]
    figs["grad_x"] = rel_l2(gxv[:, :C].numpy(), b["grad_x"])
    assert torch.equal(gxv[:, C:], torch.zeros_like(gxv[:, C:])), "padding columns of grad_x must be zero"
    if sig:
        figs["dgamma"], figs["dbeta"] = rel_l2(dg.numpy(), b["grad_gamma"]), rel_l2(db.numpy(), b["grad_beta"])
        figs["mean"] = float(np.abs(stats[:C].numpy().astype(np.float64) + stats[2 * C:].numpy() - f["mean"]).max() * f["rstd"].max())  # in units of sigma
        figs["rstd"] = rel_l2(stats[C:2 * C].numpy(), f["rstd"])
        if training:
            figs["running_mean"] = float((np.abs(rm.numpy() - f["running_mean"]) / np.abs(f["running_mean"])).max())
            figs["running_var"] = float((np.abs(rv.numpy() - f["running_var"]) / np.abs(f["running_var"])).max())
            assert int(nbt) == 8
        else:
            assert torch.equal(rm, rm0) and torch.equal(rv, rv0) and int(nbt) == 7
    print(f"bn_act B={B} HW={HW} C={C} ld={ld} {act} train={int(training)} n={n_factor}P: " + " ".join(f"{k}={v:.2e}" for k, v in figs.items()))
    for k, v in figs.items():
        assert v <= TOL, (k, v)
        worst = max(worst, v)
    return worst


# P = B * HW: one lane, the wave edge (63, 64, 65), past one workgroup (257, 258), many partial rows (70 001, 70 002); B = 3 makes the
# transpose to NCHW a real one.  (torch refuses one value per channel in train mode, so P = 2 is the floor.)
@pytest.mark.parametrize("B,HW", [(1, 2), (2, 1), (3, 21), (1, 64), (1, 65), (1, 257), (3, 86), (1, 70001), (3, 23334)])
def test_bn_act_forward_backward(dev, B, HW):
    seed = 1000 * B + HW
    for C in (1, 2, 3):
        x = torch.randn(B, C, HW, 1, generator=torch.Generator().manual_seed(seed + C)) * 1.5 + 0.3
        if B * HW == 2:
            # Two values per channel normalise to +-s, s^2 = var / (var + eps), whatever they are, so the input gradient is the small
            # factor (1 - s^2) = eps / (var + eps) times a difference of terms of unit size: at var ~ 1 that is a 1e-5 cancellation, which
            # no fp32 BatchNorm resolves to 1e-5.  A spread of the size of sqrt(eps) keeps the case well-conditioned; the code path
            # (one lane, one partial row) is the same.
            x = (x - 0.3) * 2e-3 + 0.3
        for ld in sorted({C, 4, 8}):
            _bn_case(dev, B, HW, C, ld, "sigmoid", True, 1 if ld != 8 else 4, x, seed)
            _bn_case(dev, B, HW, C, ld, "sigmoid", False, 1, x, seed + 1)
        _bn_case(dev, B, HW, C, 4, "tanh", False, 1, x, seed + 2)
        _bn_case(dev, B, HW, C, C, "none", False, 1, x, seed + 3)


@pytest.mark.parametrize("C,ld", [(1, 4), (2, 2), (8, 8), (5, 8)])
def test_bn_act_offset_map_normalises_like_a_centred_one(dev, C, ld):
    """x = 1000 + N(0, 1): a variance formed as E[x^2] - E[x]^2 in fp32 has no correct digit here (x^2 ~ 1e6, ulp 0.06, against a
    variance of 1); the (count, mean, M2) merge must meet the bound of the centred case."""
    x = 1000.0 + torch.randn(1, C, 70001, 1, generator=torch.Generator().manual_seed(5 + C))
    _bn_case(dev, 1, 70001, C, ld, "sigmoid", True, 1, x, 77)
    _bn_case(dev, 1, 70001, C, ld, "sigmoid", False, 1, torch.randn(1, C, 70001, 1, generator=torch.Generator().manual_seed(6)), 78)


def _bce(dev, p, t):
    from mvp import lib, ops

    outs = []
    for _ in range(2):
        loss = torch.full((1,), float("nan"), device=dev)
        grad = torch.full(p.shape, float("nan"), device=dev)
        ws = torch.empty(lib.BCE_WORKSPACE_BYTES // 8, dtype=torch.float64, device=dev)
        ops.bce_loss(p, t, loss, grad, ws, p.numel())
        torch.cuda.synchronize()
        outs.append((loss.cpu(), grad.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "two launches differ"
    return outs[0]


@pytest.mark.parametrize("N", [1, 63, 65, 100003])
@pytest.mark.parametrize("aligned", [True, False])
def test_bce_loss_and_gradient(dev, N, aligned):
    g = torch.Generator().manual_seed(N)
    p = torch.rand(N, generator=g) * 0.98 + 0.01
    t = (torch.rand(N, generator=g) < 0.4).float()
    t[::7] = 0.3  # soft targets
    off = 0 if aligned else 1  # an odd element offset: no 16-byte alignment, the scalar path
    pd, td = torch.zeros(N + 1).to(dev), torch.zeros(N + 1).to(dev)
    pd[off:off + N], td[off:off + N] = p.to(dev), t.to(dev)
    loss, grad = _bce(dev, pd[off:off + N], td[off:off + N])
    ref_l, ref_g = R.bce(p.numpy(), t.numpy()), R.bce_grad(p.numpy(), t.numpy())
    e_l, e_g = abs(float(loss) - ref_l) / abs(ref_l), rel_l2(grad.numpy(), ref_g)
    print(f"bce N={N} aligned={aligned}: loss={e_l:.2e} grad={e_g:.2e}")
    assert e_l <= TOL and e_g <= TOL


@pytest.mark.parametrize("N", [4, 65])
def test_bce_saturated_predictions(dev, N):
    """p exactly 0 or 1: loss 100 / gradient -+1e12 / N against the other target, 0 / 0 against its own; everything finite."""
    p = torch.tensor([0.0, 0.0, 1.0, 1.0]).repeat((N + 3) // 4)[:N]
    t = torch.tensor([0.0, 1.0, 0.0, 1.0]).repeat((N + 3) // 4)[:N]
    loss, grad = _bce(dev, p.to(dev), t.to(dev))
    assert torch.isfinite(loss).all() and torch.isfinite(grad).all()
    wrong = p != t
    np.testing.assert_allclose(float(loss), 100.0 * float(wrong.float().mean()), rtol=1e-6)
    assert torch.equal(grad[~wrong], torch.zeros(int((~wrong).sum())))
    np.testing.assert_allclose(grad[wrong].numpy(), ((p - t)[wrong] * 1e12 / N).numpy(), rtol=1e-6)
    np.testing.assert_allclose(float(loss), R.bce(p.numpy(), t.numpy()), rtol=1e-6)


@pytest.mark.parametrize("G", [1, 5])
@pytest.mark.parametrize("n", [1, 63, 65, 4096, 100003])
def test_binary_counts_equal_numpy(dev, G, n):
    from mvp import ops

    g = torch.Generator().manual_seed(G * 1000 + n)
    pred = torch.rand(G, n, generator=g)
    pred[:, ::5] = 0.5  # exactly the threshold: negative
    gt = (torch.rand(G, n, generator=g) < 0.45).float()
    ref = R.counts(pred.numpy(), gt.numpy())
    for _ in range(2):
        out = torch.full((G, 4), -1, dtype=torch.int64, device=dev)
        ops.binary_counts(pred.to(dev), gt.to(dev), out, G, n, 0.5)
        assert np.array_equal(out.cpu().numpy(), ref), (out.cpu().numpy(), ref)
    assert ref.sum(axis=1).tolist() == [n] * G
    assert int(ref[:, 0].sum() + ref[:, 1].sum()) == int((pred > 0.5).sum())


def test_functional_forms_reach_the_kernels(dev):
    """MF.bn_act on the permuted view a head returns (no copy: ld = 4 read in place), its autograd against the restatement, and
    MF.bce_loss with the root-gradient shortcut of MF.backward."""
    from mvp import functional as MF

    g = torch.Generator().manual_seed(11)
    B, C, H, W = 3, 2, 5, 7
    lq = torch.randn(B, H, W, 4, generator=g).to(dev).requires_grad_(True)
    bn = torch.nn.BatchNorm2d(C).to(dev)
    with torch.no_grad():
        bn.weight.copy_(torch.tensor([1.2, 0.7]))
        bn.bias.copy_(torch.tensor([0.1, -0.3]))
    x = lq[..., :C].permute(0, 3, 1, 2)
    assert MF._rows_view(x)[0].data_ptr() == lq.data_ptr() and MF._rows_view(x)[1] == 4
    y = MF.bn_act(x, bn, "sigmoid", True, n_factor=4)
    t = (torch.rand(B, C, H, W, generator=g) < 0.5).float().to(dev)
    loss = MF.bce_loss(y, t)
    MF.backward(loss)
    xn = lq.detach().cpu()[..., :C].permute(0, 3, 1, 2).numpy()
    f = R.bn_act_fwd(xn, [1.2, 0.7], [0.1, -0.3], np.zeros(C), np.ones(C), n=4 * B * H * W)
    gy = R.bce_grad(f["y"], t.cpu().numpy())
    b = R.bn_act_bwd(xn, gy, [1.2, 0.7], [0.1, -0.3])
    assert abs(float(loss) - R.bce(f["y"], t.cpu().numpy())) <= TOL * float(loss)
    assert rel_l2(lq.grad.cpu()[..., :C].permute(0, 3, 1, 2).numpy(), b["grad_x"]) <= TOL
    assert torch.equal(lq.grad[..., C:], torch.zeros_like(lq.grad[..., C:]))
    assert rel_l2(bn.weight.grad.cpu().numpy(), b["grad_gamma"]) <= TOL and rel_l2(bn.bias.grad.cpu().numpy(), b["grad_beta"]) <= TOL
    np.testing.assert_allclose(bn.running_var.cpu().numpy(), f["running_var"], rtol=1e-5)
    assert int(bn.num_batches_tracked) == 1
