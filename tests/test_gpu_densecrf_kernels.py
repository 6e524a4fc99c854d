"""GPU checks of the dense-CRF kernels (csrc/densecrf.hip) against the fp64 oracle of tests/densecrf_ref.py.

Tolerances.
Filter: relative 1e-4 of each (positive) sum.  That is the worst case of an fp32 chunk of up to 1024 positive terms, 1024 * 2^-24 =
6.1e-5 (the kernel's chunks have 16), plus the rounding of the exp2 argument, <= 24 * 2^-24 on every weight that matters, plus the
skip rule's N * 2^-40.
Q after 10 iterations: 16 x the worst |Q_fp32 - Q_fp64| of the oracle itself run in fp32 on the four fixtures, recomputed here (the
margin is for another summation order and the hardware exp2).  MAP: equal to the oracle's outside the pixels whose oracle
|Q_1 - 0.5| < 1e-3, which may be at most 0.5 % of a fixture (the oracle excludes none).
Hole filling, the IoU rule and the union are integer work: exact."""
import functools

import numpy as np
import pytest
import torch

import densecrf_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = {"spatial": (1.0 / 3.0 ** 2, 0.0), "bilateral": (1.0 / 50.0 ** 2, 1.0 / 5.0 ** 2)}
CANARY = -77.0


def _image(H, W, style, seed):
    rng = np.random.default_rng(seed)
    if style == "constant":
        return np.full((H, W, 3), 131, dtype=np.uint8)
    if style == "extremes":  # both ends of the byte range: the largest colour difference there is
        img = np.zeros((H, W, 3), dtype=np.uint8)
        img[:, W // 2:] = 255
        img[H // 2:, :, 1] = 255 - img[H // 2:, :, 1]
        return img
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([60 + 2 * (xx * 7 // max(W, 1)), 120 + 3 * (yy * 5 // max(H, 1)), 200 - 2 * ((xx + yy) * 4 // max(H + W, 1))], axis=-1)
    return (base + rng.integers(-5, 6, size=(H, W, 3))).clip(0, 255).astype(np.uint8)


@functools.lru_cache(None)
def _kernels(H, W, style, seed):
    return ref.kernel_matrices(_image(H, W, style, seed))


def _filter(rgb, fields, kind, active=None, out=None):
    """rgb [B, H, W, 3] uint8 array, fields [B, F, N] fp32 array or (B, F) for the ones field -> out [B, F, N] fp32 tensor."""
    from mvp import ops

    B, H, W = rgb.shape[:3]
    if isinstance(fields, tuple):
        F, inp = fields[1], None
    else:
        F, inp = fields.shape[1], torch.from_numpy(fields).to(DEV)
    if out is None:
        out = torch.full((B, F, H * W), CANARY, dtype=torch.float32, device=DEV)
    act = None if active is None else torch.tensor(active, dtype=torch.uint8, device=DEV)
    ops.crf_filter(torch.from_numpy(rgb).to(DEV), out, B, F, H, W, *KINDS[kind], inp=inp, active=act)
    return out


CASES = [(1, 1, 1, "noise"), (5, 7, 1, "noise"), (37, 53, 1, "noise"), (37, 53, 3, "noise"), (64, 64, 2, "noise"), (37, 53, 2, "constant"),
         (37, 53, 2, "extremes")]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("H,W,F,style", CASES)
def test_filter_against_fp64(H, W, F, style, kind):
    rng = np.random.default_rng(H * 100 + F)
    rgb = _image(H, W, style, 1)
    K = _kernels(H, W, style, 1)[0 if kind == "spatial" else 1]
    fields = rng.uniform(0.0, 1.0, size=(1, F, H * W)).astype(np.float32)
    got = _filter(rgb[None], fields, kind).cpu().numpy().astype(np.float64)
    want = fields[0].astype(np.float64) @ K.T
    rel = np.abs(got[0] - want) / want
    ones = _filter(rgb[None], (1, 1), kind).cpu().numpy().astype(np.float64)
    rel1 = np.abs(ones[0, 0] - K.sum(axis=1)) / K.sum(axis=1)
    print(f"filter {kind} {H}x{W} F={F} {style}: max rel err {rel.max():.2e}, ones field {rel1.max():.2e}")
    assert rel.max() <= 1e-4 and rel1.max() <= 1e-4
    assert ones.min() >= 1.0 - 1e-6  # the self term


@pytest.mark.parametrize("kind", list(KINDS))
def test_filter_two_images_one_inactive_and_extra_fields_untouched(kind):
    H, W, F = 96, 80, 2
    rng = np.random.default_rng(5)
    rgb = np.stack([_image(H, W, "noise", 2), _image(H, W, "noise", 3)])
    K = _kernels(H, W, "noise", 2)[0 if kind == "spatial" else 1]
    fields = rng.uniform(0.0, 1.0, size=(2, F + 1, H * W)).astype(np.float32)
    from mvp import ops

    out = torch.full((2, F + 1, H * W), CANARY, dtype=torch.float32, device=DEV)
    ops.crf_filter(torch.from_numpy(rgb).to(DEV), out, 2, F, H, W, *KINDS[kind], inp=torch.from_numpy(fields).to(DEV),
                   in_stride=(F + 1) * H * W, out_stride=(F + 1) * H * W, active=torch.tensor([1, 0], dtype=torch.uint8, device=DEV))
    got = out.cpu().numpy().astype(np.float64)
    want = fields[0, :F].astype(np.float64) @ K.T
    rel = np.abs(got[0, :F] - want) / want
    print(f"filter {kind} {H}x{W} B=2: max rel err {rel.max():.2e}")
    assert rel.max() <= 1e-4
    assert np.all(got[0, F] == CANARY) and np.all(got[1] == CANARY)  # the field beyond F and the inactive image


@pytest.mark.parametrize("kind", list(KINDS))
def test_filter_is_deterministic(kind):
    rng = np.random.default_rng(9)
    rgb = _image(64, 64, "noise", 4)[None]
    fields = rng.uniform(0.0, 1.0, size=(1, 3, 64 * 64)).astype(np.float32)
    a, b = _filter(rgb, fields, kind), _filter(rgb, fields, kind)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@functools.lru_cache(None)
def _q_tolerance():
    return 16.0 * max(float(np.abs(ref.fixture(k, S)[3] - ref.fixture(k, S)[4]).max()) for k, S in ref.FIXTURES)


@pytest.mark.parametrize("kind,S", ref.FIXTURES)
def test_mean_field_on_the_fixtures(kind, S):
    from mvp import densecrf

    rgb, m, true, Q64, Q32 = ref.fixture(kind, S)
    rgb_t = torch.from_numpy(rgb.copy()).permute(2, 0, 1)[None].contiguous().to(DEV)
    m_t = torch.from_numpy(m.copy())[None, None].to(DEV)
    q, mp = densecrf.densecrf_batch(rgb_t, m_t)
    q2, mp2 = densecrf.densecrf_batch(rgb_t, m_t)
    assert torch.equal(q.view(torch.int32), q2.view(torch.int32)) and torch.equal(mp, mp2)
    q, mp = q.cpu().numpy()[0, 0].astype(np.float64), mp.cpu().numpy()[0, 0].astype(bool)
    want = Q64[:, 1].reshape(S, S)
    err, tol = float(np.abs(q - want).max()), _q_tolerance()
    excluded = np.abs(want - 0.5) < 1e-3
    print(f"mean field {kind} {S}: max |Q - Q_fp64| {err:.2e} (tolerance {tol:.2e}; the fp32 oracle {np.abs(Q64 - Q32).max():.2e}), "
          f"excluded {int(excluded.sum())}, MAP IoU with the true mask {ref.iou(mp, true):.3f}")
    assert err <= tol
    assert excluded.mean() <= 0.005
    assert np.array_equal(mp[~excluded], (want > 0.5)[~excluded])
    q0, mp0 = densecrf.densecrf_batch(rgb_t, m_t, iters=0)
    assert np.array_equal(mp0.cpu().numpy()[0, 0], m)


# ------------------------------------------------------------------------------------------------ hole filling, IoU rule, union
def _finish(maps, refs=None, active=None):
    """maps [B, F, H, W] 0 / 1 arrays -> (refined [B, F, H, W], kept [B, F], union [B, H, W]) arrays."""
    from mvp import ops

    maps = np.ascontiguousarray(maps, dtype=np.uint8)
    B, F, H, W = maps.shape
    refs = maps if refs is None else np.ascontiguousarray(refs, dtype=np.uint8)
    refined = torch.full((B, F, H * W), 7, dtype=torch.uint8, device=DEV)
    kept = torch.full((B, F), 7, dtype=torch.uint8, device=DEV)
    union = torch.full((B, H * W), 7, dtype=torch.uint8, device=DEV)
    act = None if active is None else torch.tensor(active, dtype=torch.uint8, device=DEV)
    ops.mask_finish(torch.from_numpy(maps).to(DEV), torch.from_numpy(refs).to(DEV), refined, B, F, H, W, kept=kept, union_mask=union, active=act)
    return refined.cpu().numpy().reshape(B, F, H, W), kept.cpu().numpy(), union.cpu().numpy().reshape(B, H, W)


def _ring(H, W, y0, y1, x0, x1):
    m = np.zeros((H, W), dtype=np.uint8)
    m[y0:y1, x0:x1] = 1
    m[y0 + 1:y1 - 1, x0 + 1:x1 - 1] = 0
    return m


def _spiral(S=480):
    """Nested one-pixel rings four pixels apart, each open at the corner opposite to the next one's opening: the background of every
    corridor reaches the border, but only through all the corridors outside it.  A closed box in the middle is the one hole."""
    m = np.zeros((S, S), dtype=np.uint8)
    for k, a in enumerate(range(1, S // 2 - 8, 4)):
        b = S - 1 - a
        m[a, a:b + 1] = m[b, a:b + 1] = 1
        m[a:b + 1, a] = m[a:b + 1, b] = 1
        if k % 2 == 0:
            m[a, a + 1:a + 3] = 0
        else:
            m[b, b - 2:b] = 0
    c = S // 2
    m[c - 3:c + 3, c - 3:c + 3] = _ring(6, 6, 0, 6, 0, 6)
    return m


def _hole_cases():
    rng = np.random.RandomState(3)
    cases = {}
    for H, W in ((1, 1), (1, 40), (33, 31), (9, 32), (9, 33), (9, 63), (9, 64), (9, 65)):
        for p in (0.45, 0.6):
            cases[f"random {H}x{W} p={p}"] = (rng.rand(H, W) < p).astype(np.uint8)
    cases["ring"] = _ring(12, 70, 2, 10, 3, 67)
    gap = _ring(12, 70, 2, 10, 3, 67)
    gap[2, 3] = 0  # the corner pixel: the inside now touches the outside diagonally only, which 4-connectivity does not cross
    cases["ring open by a diagonal gap"] = gap
    cav = _ring(12, 70, 0, 8, 20, 50)
    cav[0, 21:49] = 0  # the cavity's top wall is the image border: not a hole
    cases["cavity at the border"] = cav
    cases["ones"] = np.ones((10, 37), dtype=np.uint8)
    cases["zeros"] = np.zeros((10, 37), dtype=np.uint8)
    cases["spiral 480"] = _spiral()
    return cases


HOLES = _hole_cases()


@pytest.mark.parametrize("name", list(HOLES))
def test_hole_filling_against_scipy(name):
    m = HOLES[name]
    want = ref.fill_holes(m)
    if name == "ring open by a diagonal gap":
        assert want.sum() > m.sum()  # still a hole
    if name in ("cavity at the border",):
        assert want.sum() == m.sum()
    if name == "spiral 480":
        assert want.sum() == m.sum() + 16  # the box's inside and nothing else
    refined, kept, union = _finish(m[None, None], want[None, None])  # (the filled mask as the IoU rule's other side: nothing is dropped)
    assert np.array_equal(refined[0, 0].astype(bool), want) and kept[0, 0] == 1
    assert np.array_equal(union[0].astype(bool), want)


def test_iou_rule_at_the_boundary():
    H, W = 4, 40
    a = np.zeros((H, W), dtype=np.uint8)
    a[0, :8] = 1
    b_keep = np.zeros((H, W), dtype=np.uint8)
    b_keep[0, :16] = 1   # inter 8, union 16: 2 * inter == union
    b_drop = np.zeros((H, W), dtype=np.uint8)
    b_drop[0, 1:17] = 1  # inter 7, union 17
    empty = np.zeros((H, W), dtype=np.uint8)
    maps = np.stack([a, a, empty])[None]
    refs = np.stack([b_keep, b_drop, empty])[None]
    assert [ref.keeps(x, y) for x, y in zip(maps[0], refs[0])] == [True, False, True]
    refined, kept, union = _finish(maps, refs)
    assert kept[0].tolist() == [1, 0, 1]
    assert np.array_equal(refined[0, 0], a) and not refined[0, 1].any() and not refined[0, 2].any()
    assert np.array_equal(union[0], a)


def test_union_over_active_passes():
    rng = np.random.RandomState(11)
    B, F, H, W = 2, 3, 21, 45
    maps = (rng.rand(B, F, H, W) < 0.35).astype(np.uint8)
    refs = maps.copy()
    refs[0, 1] = 0
    refs[0, 1, :2] = 1  # pass 1 of image 0 disagrees with its input: dropped
    active = [[1, 1, 1], [1, 0, 1]]
    refined, kept, union = _finish(maps, refs, active)
    for b in range(B):
        want = np.zeros((H, W), dtype=bool)
        for f in range(F):
            if not active[b][f]:
                assert np.all(refined[b, f] == 7) and kept[b, f] == 7  # untouched
                continue
            filled = ref.fill_holes(maps[b, f])
            k = ref.keeps(filled, refs[b, f])
            assert kept[b, f] == int(k) and np.array_equal(refined[b, f].astype(bool), filled & k)
            want |= filled & k
        assert np.array_equal(union[b].astype(bool), ref.fill_holes(want))
    assert kept[0, 1] == 0
