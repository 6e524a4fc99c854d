"""mvp_augment_stats / mvp_augment_apply (csrc/augment.hip) against the stage-by-stage fp64 reference of tests/augment_ref.py.

Geometry is exact: every output value of every plane is one input value, so flips, crops and the full-box / zero-angle identities are
compared bit for bit (the image against the fp32 formula (x / 255 - mean) / std, which has no fused form).  Under a rotation the kernel's
fp32 source coordinate (error <= 7e-5 px at 480 x 640) may round the other way only where the fp64 coordinate lies within 1e-3 px of a
rounding tie: those pixels are excluded, and their share is asserted to stay <= 1 %.

Jitter tolerance: TOL = 4 x E, where E is the largest absolute error of the SAME formulas evaluated by torch in fp32 (augment_ref with
dtype=float32) against fp64 over the jitter inputs of this file (_jitter_sets, both input forms).  The kernel differs from that restatement by fp32
rounding in another operation order (fused multiply-adds) and by one shared reciprocal in RGB -> HSV.  Both figures are printed.

Contrast mean: relative 1e-6 against the fp64 mean (fp64 partial sums over at most 3e5 fp32 grey values)."""
import functools
import itertools
import math

import pytest
import torch

import augment_ref
from mvp import augment

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [((5, 7), (5, 7)), ((16, 16), (16, 16)), ((33, 47), (33, 47)), ((64, 48), (32, 40))]
CASES = [(hw, out, B) for hw, out in SHAPES for B in (1, 3)] + [((480, 640), (480, 640), 2)]
IDS = [f"{hw[0]}x{hw[1]}-B{B}" for hw, _, B in CASES]
FORMS = ["u8", "f32"]
ANGLES = [10.0, -10.0, 7.3, 0.37]
MEAN = "imagenet"


@functools.lru_cache(maxsize=None)
def inputs(B, H, W, form, seed=0):
    """(image, depth, snorm) on the host.  depth is the pixel's linear index (exact in fp32): the gathered depth IS the source index."""
    g = torch.Generator().manual_seed(97 * seed + 13 * B + 7 * H + W)
    if form == "u8":
        image = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    else:
        image = torch.rand(B, 3, H, W, generator=g)
    depth = torch.arange(H * W, dtype=torch.float32).view(1, 1, H, W).repeat(B, 1, 1, 1)
    snorm = torch.randn(B, 3, H, W, generator=g)
    return image, depth, snorm


def normalised(image, mean_name=MEAN):
    """The fp32 formula on the whole input: [B, 3, H, W]."""
    mean, std = augment.mean_std(mean_name)
    x = image.permute(0, 3, 1, 2).float() / 255 if image.dtype == torch.uint8 else image
    return (x - torch.tensor(mean).view(1, 3, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1)


def run(image, depth, snorm, params, out_hw, mean_name=MEAN, jitter=True):
    o = augment.augment_batch(image.to(DEV), depth.to(DEV), None if snorm is None else snorm.to(DEV), params.to(DEV), out_hw, mean_name,
                              jitter=jitter)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu() for t in o)


def gather(planes, idx):
    """planes [B, C, H, W], idx [B, Ho, Wo] linear source index -> [B, C, Ho, Wo]."""
    B, C = planes.shape[:2]
    flat = planes.reshape(B, C, -1)
    return torch.stack([flat[b][:, idx[b].reshape(-1)].reshape(C, *idx.shape[1:]) for b in range(B)])


def entry(H, W, **kw):
    return dict(augment.identity_entry(H, W), **kw)


def rot(deg):
    t = math.radians(deg)
    return {"rotate": True, "cos": math.cos(t), "sin": math.sin(t)}


def check_geometry(hw, out_hw, B, form, entries, max_tie_share=0.0):
    """Run len(entries) / B launches; every plane must equal the gather of the sequential reference outside the tie margin."""
    H, W = hw
    image, depth, snorm = inputs(B, H, W, form)
    norm = normalised(image)
    for k in range(0, len(entries), B):
        chunk = (entries[k:k + B] * B)[:B]
        params = augment.pack_params(chunk)
        idx, tie = augment_ref.source_index(params, H, W, out_hw)
        share = tie.float().mean().item()
        assert share <= max_tie_share, share
        o_img, o_dep, o_sn = run(image, depth, snorm, params, out_hw, jitter=False)
        assert o_img.shape == (B, 3, *out_hw) and o_dep.shape == (B, 1, *out_hw) and o_sn.shape == (B, 3, *out_hw)
        ok = ~tie
        assert torch.equal(o_dep[:, 0][ok].long(), idx[ok]), f"source index, entries {k}.."
        keep = ok.unsqueeze(1).expand(B, 3, *out_hw)
        assert torch.equal(o_img[keep], gather(norm, idx)[keep])
        assert torch.equal(o_sn[keep], gather(snorm, idx)[keep])
        if all(e == entry(H, W, flip=True) for e in chunk) and tuple(out_hw) == (H, W):
            assert torch.equal(o_img, norm.flip(-1)) and torch.equal(o_sn, snorm.flip(-1))  # bit for bit torch.flip of the normalised input
        yy, xx = augment.index_map(params, H, W, out_hw)
        assert torch.equal((yy * W + xx)[ok], idx[ok])  # the host restatement says the same


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("hw,out_hw,B", CASES, ids=IDS)
def test_exact_cases(hw, out_hw, B, form):
    H, W = hw
    s = min(H, W)
    entries = [entry(H, W),                                   # identity (a plain nearest resize at 64x48 -> 32x40)
               entry(H, W, flip=True),                        # flip only
               entry(H, W, box=(0, 0, W, H), jitter=False),   # the full box
               entry(H, W, box=(W - s, H - s, s, s)),         # a box touching the right and bottom borders
               entry(H, W, **rot(0.0)),                       # theta = 0 through the rotation path
               entry(H, W, flip=True, box=(W - s + 1, H - s + 1, s - 1, s - 1))]
    check_geometry(hw, out_hw, B, form, entries)
    if B > 1:
        check_geometry(hw, out_hw, B, form, [entry(H, W, flip=True)] * B)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("deg", ANGLES)
@pytest.mark.parametrize("hw,out_hw,B", CASES, ids=IDS)
def test_rotation_indices(hw, out_hw, B, deg, form):
    H, W = hw
    s = min(H, W)
    entries = [entry(H, W, **rot(deg)), entry(H, W, flip=True, **rot(deg)), entry(H, W, flip=True, box=(W - s, H - s, s, s), **rot(deg))]
    check_geometry(hw, out_hw, B, form, entries[:B] if B > 1 else entries[:2], max_tie_share=0.01)


def test_reflect101_at_all_four_corners():
    """16 x 16 at +-10 degrees: about 6 % of the source coordinates fall outside the image, at every corner; the kernel's pixels there
    are the reflected ones of the reference (no edge repeated, nothing out of bounds)."""
    H = W = 16
    image, depth, snorm = inputs(1, H, W, "f32")
    for deg in (10.0, -10.0):
        c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
        y, x = torch.meshgrid(torch.arange(16.0, dtype=torch.float64), torch.arange(16.0, dtype=torch.float64), indexing="ij")
        fx = torch.floor(7.5 + c * (x - 7.5) - s * (y - 7.5) + 0.5)
        fy = torch.floor(7.5 + s * (x - 7.5) + c * (y - 7.5) + 0.5)
        outside = (fx < 0) | (fx > 15) | (fy < 0) | (fy > 15)
        assert 0.03 < outside.float().mean().item() < 0.10
        assert all(outside[ys, xs].any() for ys in (slice(0, 4), slice(12, 16)) for xs in (slice(0, 4), slice(12, 16)))
        params = augment.pack_params([entry(H, W, **rot(deg))])
        idx, tie = augment_ref.source_index(params, H, W, (H, W))
        _, o_dep, _ = run(image, depth, snorm, params, (H, W), jitter=False)
        sel = outside & ~tie[0]
        assert sel.sum() >= 8 and torch.equal(o_dep[0, 0][sel].long(), idx[0][sel])


# ---------------------------------------------------------------------------------------------------------------- jitter

JH, JW = 33, 47
ORDERS = list(itertools.permutations(range(4)))


def _jitter_sets():
    """name -> (image kind, entries): every launch is one batch of len(entries) images."""
    J = lambda **kw: entry(JH, JW, jitter=True, **kw)  # noqa: E731
    sets = {
        "each operation alone": ("colour", [J(brightness=1.17), J(brightness=0.83), J(contrast=1.19), J(contrast=0.81), J(saturation=1.2),
                                            J(saturation=0.8), J(hue=0.13), J(hue=-0.17)]),
        "all 24 orders": ("colour", [J(order=o, brightness=1.15, contrast=0.85, saturation=1.18, hue=0.11) for o in ORDERS]),
        "hue wraps": ("colour", [J(hue=0.2), J(hue=-0.2), J(hue=0.49), J(hue=-0.49), J(order=(3, 0, 1, 2), hue=0.2, brightness=1.2)]),
        "grey image": ("grey", [J(order=o, brightness=1.1, contrast=1.2, saturation=0.8, hue=0.2) for o in ORDERS[::5]]),
        "black image": ("black", [J(order=o, brightness=1.2, contrast=0.8, saturation=1.2, hue=-0.2) for o in ORDERS[::7]]),
        "range ends": ("colour", [J(order=ORDERS[(3 * i) % 24], brightness=b, contrast=c, saturation=s, hue=h)
                                  for i, (b, c, s, h) in enumerate(itertools.product((0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.2, 0.2)))]),
    }
    return sets


def _jitter_image(kind, B, form):
    g = torch.Generator().manual_seed(11)
    if kind == "colour":
        img = torch.randint(0, 256, (1, JH, JW, 3), generator=g, dtype=torch.uint8)
        img[0, :4, :4] = torch.tensor([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0]], dtype=torch.uint8).view(1, 4, 3)  # pure hues
        img[0, 4, :3] = torch.tensor([[0, 0, 0], [255, 255, 255], [128, 128, 128]], dtype=torch.uint8)
    elif kind == "grey":
        img = torch.randint(0, 256, (1, JH, JW, 1), generator=g, dtype=torch.uint8).expand(1, JH, JW, 3).contiguous()
    else:
        img = torch.zeros(1, JH, JW, 3, dtype=torch.uint8)
    img = img.repeat(B, 1, 1, 1)
    return img if form == "u8" else (img.permute(0, 3, 1, 2).float() / 255).contiguous()


@functools.lru_cache(maxsize=None)
def jitter_case(name, form):
    """-> (image, depth, params, fp64 result, max abs error of the fp32 restatement)."""
    kind, entries = _jitter_sets()[name]
    B = len(entries)
    image = _jitter_image(kind, B, form)
    depth = torch.zeros(B, 1, JH, JW)
    params = augment.pack_params(entries)
    ref64 = augment_ref.apply(image, depth, None, params, (JH, JW), MEAN, dtype=torch.float64)[0]
    ref32 = augment_ref.apply(image, depth, None, params, (JH, JW), MEAN, dtype=torch.float32)[0]
    return image, depth, params, ref64, float((ref32.double() - ref64).abs().max())


@functools.lru_cache(maxsize=None)
def jitter_tolerance():
    """4 x the largest error of the fp32 torch restatement over every jitter input of this file."""
    e = max(jitter_case(name, form)[4] for name in _jitter_sets() for form in FORMS)
    assert 1e-8 < e < 1e-5, e  # fp32 rounding of values of magnitude <= 2.7 through four operations
    return 4.0 * e


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(_jitter_sets()))
def test_jitter_against_fp64(name, form):
    image, depth, params, ref64, e32 = jitter_case(name, form)
    tol = jitter_tolerance()
    out = run(image, depth, None, params, (JH, JW))[0]
    err = float((out.double() - ref64).abs().max())
    print(f"[augment jitter] {name} / {form}: kernel max abs err {err:.3e}, fp32 restatement {e32:.3e}, tolerance {tol:.3e}")
    assert err <= tol, (name, form, err, tol)
    if name == "black image":
        mean, std = augment.mean_std(MEAN)
        want = (torch.zeros(3) - torch.tensor(mean)) / torch.tensor(std)
        assert torch.equal(out, want.view(1, 3, 1, 1).expand_as(out))  # black stays exactly black


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("hw,B", [((33, 47), 3), ((16, 16), 1), ((480, 640), 2)])
def test_contrast_mean(hw, B, form):
    """The partials of mvp_augment_stats, added in index order and divided by H * W, against the fp64 mean of the grey value of the image
    as it stands when contrast is reached (relative 1e-6); images whose jitter is off write zeros."""
    from mvp import ops

    H, W = hw
    image, _, _ = inputs(B, H, W, form, seed=3)
    orders = [(1, 0, 2, 3), (0, 1, 2, 3), (3, 2, 0, 1)]
    entries = [entry(H, W, jitter=True, order=orders[b % 3], brightness=1.2, contrast=0.8, saturation=0.8, hue=0.2) for b in range(B)]
    if B > 1:
        entries[1]["jitter"] = False
    params = augment.pack_params(entries)
    partials = ops.augment_partials(B, DEV)
    partials.fill_(float("nan"))  # no initialisation needed: every slot is written
    ops.augment_stats(image.to(DEV), params.to(DEV), partials)
    torch.cuda.synchronize()
    p = partials.cpu()
    assert p.shape == (B, 32) and torch.isfinite(p).all()
    if H * W > 1024:
        assert (p[0] != 0).sum() > 1  # more than one workgroup contributes
    for b, e in enumerate(augment.unpack_params(params)):
        if not e["jitter"]:
            assert torch.equal(p[b], torch.zeros(32, dtype=torch.float64))
            continue
        got = float(p[b].sum()) / (H * W)
        want = augment_ref.contrast_mean(augment_ref.to_unit(image[b], torch.float64), e)
        print(f"[augment stats] {H}x{W} {form} image {b}: mean {got:.9f} fp64 {want:.9f} rel {abs(got - want) / want:.2e}")
        assert abs(got - want) <= 1e-6 * abs(want)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("hw,out_hw,B", CASES, ids=IDS)
def test_full_chain(hw, out_hw, B, form):
    """Two random tables per shape (flip, rotation, crop and jitter all drawn): geometry exact outside the tie margin, the image within the
    jitter tolerance there."""
    H, W = hw
    image, depth, snorm = inputs(B, H, W, form, seed=5)
    tol = jitter_tolerance()
    for seed in (1, 2):
        g = torch.Generator().manual_seed(1000 * seed + H)
        params = augment.sample_params(B, H, W, out_hw, g, rotateflip=True, crop_p=1.0 if tuple(out_hw) != (H, W) else 0.5, jitter_p=0.8)
        ref_img, ref_dep, ref_sn, tie = augment_ref.apply(image, depth, snorm, params, out_hw, MEAN)
        o_img, o_dep, o_sn = run(image, depth, snorm, params, out_hw)
        ok = ~tie  # (no share asserted here: on a 5 x 7 image one pixel is 3 %)
        assert torch.equal(o_dep[:, 0][ok], ref_dep[:, 0][ok])
        keep = ok.unsqueeze(1).expand_as(o_sn)
        assert torch.equal(o_sn[keep], ref_sn[keep])
        err = float((o_img.double() - ref_img)[keep].abs().max())
        print(f"[augment chain] {H}x{W} B{B} {form} seed {seed}: max abs err {err:.3e} (tolerance {tol:.3e})")
        assert err <= tol


@pytest.mark.parametrize("hw", [(33, 47), (480, 640)])
def test_same_inputs_same_bits(hw):
    H, W = hw
    image, depth, snorm = inputs(2, H, W, "u8", seed=7)
    params = augment.sample_params(2, H, W, hw, torch.Generator().manual_seed(3), rotateflip=True, jitter_p=1.0)
    a = run(image, depth, snorm, params, hw)
    b = run(image, depth, snorm, params, hw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_wrapper_rejects_what_the_kernel_cannot_take():
    from mvp import lib, ops

    image, depth, snorm = inputs(1, 16, 16, "f32")
    params = augment.pack_params([entry(16, 16)]).to(DEV)
    with pytest.raises(lib.MvpError):
        augment.augment_batch(image.to(DEV).half(), depth.to(DEV), None, params, (16, 16), MEAN)
    with pytest.raises(lib.MvpError):
        augment.augment_batch(image.to(DEV), depth.to(DEV)[:, :, :8], None, params, (16, 16), MEAN)
    with pytest.raises(lib.MvpError):
        ops.augment_apply(image.to(DEV), depth.to(DEV), None, params, None, torch.empty(1, 3, 16, 16, device=DEV),
                          torch.empty(1, 1, 16, 16, device=DEV), None, (0.0, 0.0, 0.0), (1.0, 0.0, 1.0))
