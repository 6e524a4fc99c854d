"""The three Taskonomy kernels (csrc/taskonomy.hip) against the host transforms (evals/datasets/transforms.py), the goldens recorded
from the reference (tests/golden/taskonomy.npz) and the restatements of tests/taskonomy_ref.py.

Bounds.  mvp_task_prepare is a chain of correctly rounded fp32 operations and an integer rule: bit equality.  The loss is one fp64 sum
of exact differences divided once and rounded once to fp32: 2^-23 relative to the fp64 value (the fp64 sum's own error, ~1e-16 x the term
count, is far below); its gradient is a select of +-fp32(1 / count): bit equality.  The metric counts are integers: equality; the AbsRel
sum adds the same fp32 terms in fp64 in another order: 1e-12 relative."""
import numpy as np
import pytest
import torch

import taskonomy_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

SIZES = [(4, 4), (7, 9), (8, 8), (13, 37), (64, 64)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g():
    return load_golden("taskonomy.npz")


def _offset(t, dev, by=1):
    """``t`` on the device at a base that is ``by`` elements past an allocation's start (contiguous, misaligned)."""
    buf = torch.empty(t.numel() + by, dtype=t.dtype, device=dev)
    v = buf[by:].view(t.shape)
    v.copy_(t)
    return v


def _prepare(dev, raw, mask, task, misalign=False):
    from mvp import taskonomy

    put = (lambda t: _offset(t, dev)) if misalign else (lambda t: t.to(dev))
    target, valid = taskonomy.prepare_batch(put(raw), put(mask), task)
    torch.cuda.synchronize()
    return target.cpu(), valid.cpu()


def _host(raw, mask, task):
    from evals.datasets.transforms import task_transform

    return (torch.stack([task_transform(r, task) for r in raw]), torch.stack([task_transform(m, "mask_valid") for m in mask]))


@pytest.mark.parametrize("hw", SIZES)
def test_task_prepare_masks_and_targets(dev, g, hw):
    H, W = hw
    masks, want = torch.from_numpy(g[f"mask_{H}x{W}__raw"]), g[f"mask_{H}x{W}__valid"]
    gen = torch.Generator().manual_seed(H * 100 + W)
    configs = [("reshading", 1), ("principal_curvature", 3), ("normal", 3), ("principal_curvature", 4), ("normal", 5)]
    for i in range(0, masks.shape[0], 2):  # B = 2: every mask case of the fixture, the 8-bit forms in turn
        task, cs = configs[(i // 2) % len(configs)]
        raw = torch.randint(0, 256, (2, H, W, cs), generator=gen, dtype=torch.uint8)
        raw[0, 0, 0] = 0
        raw[1, -1, -1] = 255
        m = masks[i:i + 2].contiguous()
        target, valid = _prepare(dev, raw, m, task, misalign=(i // 2) % 3 == 2)
        ht, hv = _host(raw, m, task)
        assert valid.dtype == torch.uint8 and tuple(valid.shape) == (2, 1, H, W)
        assert np.array_equal(valid.numpy().astype(bool), want[i:i + 2]), (hw, i)
        assert np.array_equal(valid.numpy().astype(bool), hv.numpy())
        assert set(valid.unique().tolist()) <= {0, 1}
        assert np.array_equal(target.numpy().view(np.uint32), ht.numpy().view(np.uint32)), (hw, task, cs)


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("task", ["keypoints2d", "depth_euclidean", "depth_zbuffer", "edge_texture"])
def test_task_prepare_16bit_and_clamp(dev, g, hw, task):
    H, W = hw
    u16 = g[f"u16_{H}x{W}__raw"]  # starts 0, 8000, 8001, 65535: zero, the depth clamp's bound, just above it, the top
    other = u16[::-1, ::-1].copy()
    other.flat[:3] = [16383, 16384, 16385]  # around edge_texture's 0.25
    raw = torch.from_numpy(np.stack([u16, other]).view(np.int16))
    masks = torch.from_numpy(g[f"mask_{H}x{W}__raw"][-2:].copy())
    for misalign in (False, True):
        target, valid = _prepare(dev, raw, masks, task, misalign)
        ht, hv = _host(raw, masks, task)
        assert np.array_equal(target.numpy().view(np.uint32), ht.numpy().view(np.uint32)), (hw, task, misalign)
        assert np.array_equal(valid.numpy().astype(bool), hv.numpy())
    if task == "keypoints2d":
        assert np.array_equal(target[0].numpy().view(np.uint32), g[f"u16_{H}x{W}__out"].view(np.uint32))  # the reference's own transform
    if task.startswith("depth"):
        t = target[0].flatten()
        assert t[0] == 0.0 and t[1] == 1.0 and t[2] == 1.0 and t[3] == 1.0 and float(target.max()) == 1.0
    if task == "edge_texture":
        t = target[1].flatten()
        assert t[0] < 1.0 and t[1] == 1.0 and t[2] == 1.0


def test_task_prepare_refuses_a_map_without_a_block(dev):
    from mvp import lib, ops

    raw = torch.zeros(2, 3, 8, 1, dtype=torch.uint8, device=dev)
    with pytest.raises(lib.MvpError, match="invalid argument"):
        ops.task_prepare(raw, torch.zeros(2, 3, 8, dtype=torch.uint8, device=dev), torch.empty(2, 1, 3, 8, device=dev),
                         torch.empty(2, 1, 3, 8, dtype=torch.uint8, device=dev), 8)


def _l1(dev, pred, tgt, valid, misalign, with_grad=True):
    from mvp import ops

    B, C, HW = pred.shape
    p = _offset(pred, dev) if misalign else pred.to(dev)
    t = _offset(tgt, dev) if misalign else tgt.to(dev)
    m = valid.to(torch.uint8).to(dev)
    loss = torch.full((1,), 7.0, device=dev)
    grad = (_offset(torch.full_like(pred, float("nan")), dev) if misalign else torch.full_like(p, float("nan"))) if with_grad else None
    ops.masked_l1(p, t, m, loss, grad, ops.task_workspace(dev), B, C, m.shape[1], HW)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), (grad.cpu().numpy() if with_grad else None)


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 2, 35), (2, 3, 1023), (3, 1, 1025), (16, 2, 4096)])
@pytest.mark.parametrize("per_channel", [False, True])
def test_masked_l1_loss_and_gradient(dev, shape, per_channel):
    _l1_case(dev, shape, per_channel)


# A row is split over several workgroups from HW > 4096 on (the training shape, 512 x 512, has 32 chunks per row), and the rows are
# strided over grid.y from B C > 1024 on: a row of three chunks with 16-byte loads, one of three chunks with an odd length (scalar
# path, a short last chunk), and 1025 rows.
@pytest.mark.parametrize("shape", [(2, 2, 4096 * 3 + 4), (2, 1, 4096 * 2 + 3), (1025, 1, 5)])
@pytest.mark.parametrize("per_channel", [False, True])
def test_masked_l1_rows_in_chunks_and_strided_rows(dev, shape, per_channel):
    _l1_case(dev, shape, per_channel)


def _l1_case(dev, shape, per_channel):
    B, C, HW = shape
    gen = torch.Generator().manual_seed(B * 10000 + C * 1000 + HW + int(per_channel))
    pred, tgt = torch.randn(B, C, HW, generator=gen), torch.rand(B, C, HW, generator=gen)
    pred.view(-1)[::5] = tgt.view(-1)[::5]  # exact zeros of the difference
    valid = torch.rand(B, C if per_channel else 1, HW, generator=gen) < 0.8
    valid.view(-1)[0] = True
    pred[valid.expand_as(pred).logical_not()] = float("nan")  # what lies under an invalid pixel is never read into a result
    want = float(R.masked_l1(torch.nan_to_num(pred).double(), tgt.double(), valid))
    gwant = R.masked_l1_grad(torch.nan_to_num(pred), tgt, valid)
    for misalign in (False, True):
        loss, grad = _l1(dev, pred, tgt, valid, misalign)
        loss2, grad2 = _l1(dev, pred, tgt, valid, misalign)
        err = abs(float(loss[0]) - want) / abs(want) if want else abs(float(loss[0]))
        print(f"masked_l1 {shape} Cm={'C' if per_channel else 1} misaligned={misalign}: loss {float(loss[0]):.8g} fp64 {want:.12g} rel {err:.2e}")
        assert err <= 2.0**-23
        assert np.array_equal(grad.view(np.uint32), gwant.view(np.uint32))
        assert np.all(grad.reshape(-1)[::5][valid.expand_as(pred).reshape(-1)[::5].numpy()] == 0)  # sign(0) = 0
        assert loss.tobytes() == loss2.tobytes() and grad.tobytes() == grad2.tobytes()
    only, none = _l1(dev, pred, tgt, valid, False, with_grad=False)
    assert none is None and only.tobytes() == loss.tobytes()


def test_masked_l1_without_a_valid_pixel(dev):
    pred, tgt = torch.randn(2, 2, 35), torch.rand(2, 2, 35)
    loss, grad = _l1(dev, pred, tgt, torch.zeros(2, 1, 35, dtype=torch.bool), False)
    assert np.isnan(loss[0]) and np.all(grad == 0) and not np.any(np.signbit(grad))


def test_masked_l1_goldens_through_the_module(dev, g):
    from evals.utils.losses import MaskedL1Loss

    for case in ("l1_a", "l1_b", "l1_c", "l1_none"):
        pred = torch.from_numpy(g[f"{case}__pred"]).to(dev).requires_grad_(True)
        tgt = torch.from_numpy(g[f"{case}__target"]).to(dev)
        mask = torch.from_numpy(g[f"{case}__mask"]).to(dev) if g[f"{case}__mask"].size else None
        loss = MaskedL1Loss()(pred, tgt, mask)
        loss.backward()
        want = float(g[f"{case}__loss64"])
        assert abs(float(loss.detach()) - want) <= 2.0**-23 * abs(want), (case, float(loss.detach()), want)
        m = mask.cpu() if mask is not None else torch.ones(pred.shape[0], 1, *pred.shape[2:], dtype=torch.bool)
        gw = R.masked_l1_grad(pred.detach().cpu(), tgt.cpu(), m)
        assert np.array_equal(pred.grad.cpu().numpy().view(np.uint32), gw.view(np.uint32)), case


def test_masked_l1_module_without_a_gradient_runs_the_loss_only_form(dev, g):
    """Under no_grad or on a detached prediction nothing is saved for a backward, and the loss is the same bits."""
    from mvp import functional as MF

    pred, tgt = torch.from_numpy(g["l1_a__pred"]).to(dev), torch.from_numpy(g["l1_a__target"]).to(dev)
    mask = torch.from_numpy(g["l1_a__mask"]).to(dev)
    with_grad = MF.masked_l1_loss(pred.clone().requires_grad_(True), tgt, mask)
    assert with_grad.requires_grad and len(with_grad.grad_fn.saved_tensors) == 1
    with torch.no_grad():
        a = MF.masked_l1_loss(pred.clone().requires_grad_(True), tgt, mask)
    b = MF.masked_l1_loss(pred, tgt, mask)
    assert not a.requires_grad and not b.requires_grad
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == with_grad.detach().cpu().numpy().tobytes()
    with pytest.raises(ValueError, match="1 or 2 channels"):
        MF.masked_l1_loss(pred, tgt, torch.ones(2, 3, 5, 7, dtype=torch.bool, device=dev))


def _metrics(dev, pred, tgt, valid, form, misalign=False):
    from evals.utils.metrics import task_metric_sums

    p = _offset(pred, dev) if misalign else pred.to(dev)
    return task_metric_sums(p, tgt.to(dev), valid.to(dev), form, R.CURV_T if form == "curvature" else R.RESH_T).cpu()


def _check_sums(got, want, what):
    assert np.array_equal(got[..., 1:].numpy(), want[..., 1:].numpy()), what  # valid pixels and the three counts: exact
    a, b = got[..., 0].numpy(), want[..., 0].numpy()
    assert np.array_equal(np.isnan(a), np.isnan(b)), what  # NaN exactly where the fp32 restatement has it
    assert np.array_equal(np.isinf(a), np.isinf(b)), what
    fin = np.isfinite(b)
    rel = np.abs(a[fin] - b[fin]) / np.maximum(np.abs(b[fin]), 1e-300)
    print(f"task_metrics {what}: worst relative distance of the AbsRel sums {rel.max() if rel.size else 0.0:.2e}")
    assert np.all(rel <= 1e-12), what


@pytest.mark.parametrize("case,form", [("curv_rand", "curvature"), ("curv_rand2", "curvature"), ("curv_ties", "curvature"),
                                       ("resh_rand", "reshading"), ("resh_rand2", "reshading"), ("resh_ties", "reshading")])
def test_task_metrics_golden_cases(dev, g, case, form):
    from evals.utils.metrics import evaluate_curvature_absrel, evaluate_reshading_absrel_and_delta

    pred, tgt, valid = (torch.from_numpy(g[f"{case}__{k}"]) for k in ("pred", "target", "valid"))
    ref_pred = pred[:, :2].contiguous() if form == "curvature" else pred
    want = R.metric_sums(ref_pred, tgt, valid, form)
    for misalign in (False, True):
        _check_sums(_metrics(dev, ref_pred, tgt, valid, form, misalign), want, f"{case} misaligned={misalign}")
    # the public functions against the reference's recorded values: the counts' quotients to fp32 rounding, AbsRel within 4 x the
    # reference's own distance from the fp64 sum of its terms
    if form == "curvature":
        m, keys = evaluate_curvature_absrel(pred.to(dev), tgt.to(dev), valid.to(dev)), R.CURV_KEYS
    else:
        m, keys = evaluate_reshading_absrel_and_delta(pred.to(dev), tgt.to(dev), valid.float().to(dev)), R.RESH_KEYS
    assert list(m) == keys
    table, dist = g[f"{case}__table"], g[f"{case}__absrel_dist"]
    for k in keys[1:]:
        assert np.allclose(m[k].double().numpy(), table[keys.index(k)], rtol=2e-7, atol=0), k
    a, b = m["AbsRel"].double().numpy(), table[0]
    assert np.array_equal(np.isnan(a), np.isnan(b))
    fin = np.isfinite(b) & (b != 0)
    assert np.all(np.abs(a[fin] - b[fin]) <= (4 * dist[fin] + 2.0**-23) * np.abs(b[fin]))  # (+ the fp32 rounding of the returned value)
    avg = evaluate_curvature_absrel(pred.to(dev), tgt.to(dev), valid.to(dev), image_average=True) if form == "curvature" else \
        evaluate_reshading_absrel_and_delta(pred.to(dev), tgt.to(dev), valid.float().to(dev), image_average=True)
    assert all(v.dim() == 0 for v in avg.values())


@pytest.mark.parametrize("form,shape", [("curvature", (2, 2, 33, 31)), ("reshading", (2, 2, 33, 31)), ("curvature", (4, 1, 64, 64)),
                                        ("reshading", (4, 1, 64, 64))])
@pytest.mark.parametrize("per_channel", [False, True])
def test_task_metrics_random_maps(dev, form, shape, per_channel):
    _metrics_case(dev, form, shape, per_channel)


# rows of more than 4096 elements are split over several workgroups, whose partials the fold launch adds per row: three chunks with
# 16-byte loads (HW = 12 292) and three chunks of an odd row (HW = 8 195: scalar path, a short last chunk)
@pytest.mark.parametrize("form", ["curvature", "reshading"])
@pytest.mark.parametrize("shape", [(2, 2, 4, 3073), (2, 1, 5, 1639)])
@pytest.mark.parametrize("per_channel", [False, True])
def test_task_metrics_rows_in_chunks(dev, form, shape, per_channel):
    _metrics_case(dev, form, shape, per_channel)


def _metrics_case(dev, form, shape, per_channel):
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(sum(shape) + int(per_channel) + len(form))
    pred = torch.randn(B, C, H, W, generator=gen) * 0.6 + 0.4
    tgt = (torch.rand(B, C, H, W, generator=gen) * 255).round() / 255  # exact zeros among them
    valid = torch.rand(B, C if per_channel else 1, H, W, generator=gen) < 0.9
    want = R.metric_sums(pred, tgt, valid, form)
    got = _metrics(dev, pred, tgt, valid, form)
    _check_sums(got, want, f"{form} {shape} Cm={'C' if per_channel else 1}")
    assert _metrics(dev, pred, tgt, valid, form).numpy().tobytes() == got.numpy().tobytes()  # two runs, the same bits
