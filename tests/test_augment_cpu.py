"""Host side of the device augmentation (mvp/augment.py), no GPU: the parameter sampler, and the composed integer index map against the
stage-by-stage reference of tests/augment_ref.py (which materialises the flipped, the rotated and the cropped image one after the other)."""
import math

import pytest
import torch

import augment_ref
from mvp import augment


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _entries(B, H, W, seed=0, **kw):
    return augment.unpack_params(augment.sample_params(B, H, W, kw.pop("out_hw", (H, W)), _gen(seed), **kw))


def test_sampler_factor_ranges_and_order():
    es = _entries(4000, 48, 64, rotateflip=True)
    f32 = 1e-6
    for key, lo, hi in (("brightness", 0.8, 1.2), ("contrast", 0.8, 1.2), ("saturation", 0.8, 1.2), ("hue", -0.2, 0.2)):
        v = torch.tensor([e[key] for e in es])
        assert lo - f32 <= v.min() and v.max() <= hi + f32 and v.max() - v.min() > 0.95 * (hi - lo), key
    assert all(sorted(e["order"]) == [0, 1, 2, 3] for e in es)
    assert len({e["order"] for e in es}) == 24  # every permutation turns up
    assert abs(sum(e["jitter"] for e in es) / 4000 - 0.8) < 0.03
    assert abs(sum(e["flip"] for e in es) / 4000 - 0.5) < 0.04 and abs(sum(e["rotate"] for e in es) / 4000 - 0.5) < 0.04
    assert abs(sum(e["box"] != (0, 0, 64, 48) for e in es) / 4000 - 0.5) < 0.04
    for e in es:
        if e["rotate"]:
            assert abs(e["cos"] ** 2 + e["sin"] ** 2 - 1.0) < 1e-6 and abs(math.degrees(math.asin(e["sin"]))) <= 10.0 + 1e-4
        else:
            assert (e["cos"], e["sin"]) == (1.0, 0.0)


def test_sampler_is_a_pure_function_of_the_generator():
    a = augment.sample_params(8, 33, 47, (33, 47), _gen(5), rotateflip=True)
    b = augment.sample_params(8, 33, 47, (33, 47), _gen(5), rotateflip=True)
    c = augment.sample_params(8, 33, 47, (33, 47), _gen(6), rotateflip=True)
    assert a.dtype == torch.int32 and a.shape == (8, augment.WORDS) and torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(augment.pack_params(augment.unpack_params(a)), a)  # the table round-trips
    # image b's draws do not depend on how many images precede it in the call
    g = _gen(5)
    first = augment.sample_params(3, 33, 47, (33, 47), g, rotateflip=True)
    assert torch.equal(first, a[:3])


def test_seeding_by_seed_rank_epoch_and_batch():
    class Stub(augment.DeviceAugment):
        def __init__(self, seed, rank):  # the seeding needs no device
            self.seed, self.rank, self.augment, self.rotateflip, self.out_hw = seed, rank, True, False, None

    base = Stub(3, 0).params_for(0, 0, 4, 32, 32)
    assert torch.equal(base, Stub(3, 0).params_for(0, 0, 4, 32, 32))
    for other in (Stub(4, 0).params_for(0, 0, 4, 32, 32), Stub(3, 1).params_for(0, 0, 4, 32, 32), Stub(3, 0).params_for(1, 0, 4, 32, 32),
                  Stub(3, 0).params_for(0, 1, 4, 32, 32)):
        assert not torch.equal(base, other)
    ident = Stub(3, 0)
    ident.augment = False
    assert torch.equal(ident.params_for(0, 0, 2, 32, 48), augment.pack_params([augment.identity_entry(32, 48)] * 2))


def test_boxes_lie_inside_the_image_and_are_square():
    for H, W in ((48, 64), (64, 48), (33, 47), (480, 640)):
        es = _entries(500, H, W, seed=H, crop_p=1.0, out_hw=(H, W))
        for e in es:
            x0, y0, cw, ch = e["box"]
            assert cw == ch and 0 < cw <= min(H, W) and 0 <= x0 and x0 + cw <= W and 0 <= y0 and y0 + ch <= H
            assert cw * ch <= H * W and cw * ch >= 0.5 * H * W * 0.98 or cw == min(H, W)  # scale (0.5, 1) unless the fallback clamps it


def test_fallback_is_the_centred_square():
    # 480 x 640 at ratio 1: any area above 480^2 / (480 * 640) = 0.75 fails all ten attempts -> the centred 480^2
    es = _entries(200, 480, 640, crop_p=1.0, scale=(0.8, 1.0))
    assert all(e["box"] == (80, 0, 480, 480) for e in es)
    es = _entries(200, 640, 480, crop_p=1.0, scale=(0.8, 1.0))
    assert all(e["box"] == (0, 80, 480, 480) for e in es)
    assert augment._crop_box([0.99, 0.5, 0.5, 0.5] * 10, 480, 640, (0.5, 1.0), (1.0, 1.0)) == (80, 0, 480, 480)


def test_rotateflip_off_never_flips_or_rotates():
    es = _entries(1000, 32, 40)
    assert not any(e["flip"] or e["rotate"] for e in es) and all((e["cos"], e["sin"]) == (1.0, 0.0) for e in es)


def test_out_hw_needs_a_crop_that_always_applies():
    with pytest.raises(ValueError):
        augment.sample_params(2, 64, 48, (32, 40), _gen(0))
    augment.sample_params(2, 64, 48, (32, 40), _gen(0), crop_p=1.0)
    with pytest.raises(ValueError):
        augment.sample_params(2, 3, 48, (3, 48), _gen(0))


def _entry(H, W, **kw):
    return dict(augment.identity_entry(H, W), **kw)


def _rot(deg):
    t = math.radians(deg)
    return {"rotate": True, "cos": math.cos(t), "sin": math.sin(t)}


SHAPES = [((5, 7), (5, 7)), ((16, 16), (16, 16)), ((33, 47), (33, 47)), ((64, 48), (32, 40))]


@pytest.mark.parametrize("hw,out_hw", SHAPES)
def test_index_map_equals_the_sequential_gather_without_rotation(hw, out_hw):
    H, W = hw
    s = min(H, W)
    entries = [_entry(H, W), _entry(H, W, flip=True), _entry(H, W, box=(W - s, H - s, s, s)), _entry(H, W, flip=True, box=(W - s, H - s, s, s)),
               _entry(H, W, box=(1, 2, s - 2, s - 2)), _entry(H, W, flip=True, box=(0, 1, s - 1, s - 1)), _entry(H, W, box=(0, 0, 3, 2))]
    params = augment.pack_params(entries)
    yy, xx = augment.index_map(params, H, W, out_hw)
    ref, tie = augment_ref.source_index(params, H, W, out_hw)
    assert not tie.any() and torch.equal(yy * W + xx, ref)
    assert int(yy.min()) >= 0 and int(yy.max()) < H and int(xx.min()) >= 0 and int(xx.max()) < W


@pytest.mark.parametrize("deg", [10.0, -10.0, 7.3, 0.37])
@pytest.mark.parametrize("hw,out_hw", SHAPES + [((480, 640), (480, 640))])
def test_index_map_equals_the_sequential_gather_with_rotation(hw, out_hw, deg):
    H, W = hw
    s = min(H, W)
    entries = [_entry(H, W, **_rot(deg)), _entry(H, W, flip=True, **_rot(deg)), _entry(H, W, flip=True, box=(W - s, H - s, s, s), **_rot(deg))]
    params = augment.pack_params(entries)
    yy, xx = augment.index_map(params, H, W, out_hw)
    ref, tie = augment_ref.source_index(params, H, W, out_hw)
    assert tie.float().mean().item() <= 0.01  # what the margin excludes stays a small share
    assert torch.equal((yy * W + xx)[~tie], ref[~tie])
    assert int(yy.min()) >= 0 and int(yy.max()) < H and int(xx.min()) >= 0 and int(xx.max()) < W


def test_rotation_reaches_past_every_corner():
    """16 x 16 at +-10 degrees sends pixels out of range at all four corners: reflect-101 is what brings them back."""
    for deg in (10.0, -10.0):
        c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
        y, x = torch.meshgrid(torch.arange(16.0), torch.arange(16.0), indexing="ij")
        fx = 7.5 + c * (x - 7.5) - s * (y - 7.5)
        fy = 7.5 + s * (x - 7.5) + c * (y - 7.5)
        out = (torch.floor(fx + 0.5) < 0) | (torch.floor(fx + 0.5) > 15) | (torch.floor(fy + 0.5) < 0) | (torch.floor(fy + 0.5) > 15)
        assert 0.03 < out.float().mean().item() < 0.10
        assert all(out[ys, xs].any() for ys in (slice(0, 4), slice(12, 16)) for xs in (slice(0, 4), slice(12, 16)))


def test_identity_parameters_only_normalise():
    g = _gen(1)
    img = torch.randint(0, 256, (2, 9, 11, 3), generator=g, dtype=torch.uint8)
    depth, snorm = torch.rand(2, 1, 9, 11, generator=g), torch.randn(2, 3, 9, 11, generator=g)
    params = augment.pack_params([augment.identity_entry(9, 11)] * 2)
    for name in ("imagenet", "clip", None):
        mean, std = augment.mean_std(name)
        o, d, n, tie = augment_ref.apply(img, depth, snorm, params, (9, 11), name, dtype=torch.float32)
        want = (img.permute(0, 3, 1, 2).float() / 255 - torch.tensor(mean).view(1, 3, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1)
        assert torch.equal(o, want) and torch.equal(d, depth) and torch.equal(n, snorm) and not tie.any()
    fimg = torch.rand(2, 3, 9, 11, generator=g)
    o, _, _, _ = augment_ref.apply(fimg, depth, None, params, (9, 11), None, dtype=torch.float32)
    assert torch.equal(o, fimg)


def test_double_flip_is_the_identity():
    H, W = 12, 10
    flip = augment.pack_params([_entry(H, W, flip=True)])
    img = torch.randint(0, 256, (1, H, W, 3), generator=_gen(2), dtype=torch.uint8)
    depth = torch.rand(1, 1, H, W, generator=_gen(3))
    o1, d1, _, _ = augment_ref.apply(img, depth, None, flip, (H, W), None, dtype=torch.float32)
    o2, d2, _, _ = augment_ref.apply(o1, d1, None, flip, (H, W), None, dtype=torch.float32)
    assert torch.equal(d2, depth) and torch.equal(o2, img.permute(0, 3, 1, 2).float() / 255)
    yy, xx = augment.index_map(flip, H, W, (H, W))
    assert torch.equal(xx[0].flip(-1), torch.arange(W).expand(H, W)) and torch.equal(yy[0], torch.arange(H).view(H, 1).expand(H, W))


def test_jitter_reference_properties():
    """The fp64 jitter keeps [0, 1], leaves a black image black and a grey image grey, and with unit factors changes nothing."""
    g = _gen(4)
    img = torch.rand(3, 8, 8, generator=g, dtype=torch.float64)
    e = _entry(8, 8, jitter=True, order=(3, 1, 0, 2))
    assert torch.allclose(augment_ref.jitter(img, e), img, atol=1e-12)
    e = _entry(8, 8, jitter=True, order=(2, 3, 1, 0), brightness=1.2, contrast=0.8, saturation=1.2, hue=-0.2)
    out = augment_ref.jitter(img, e)
    assert out.min() >= 0 and out.max() <= 1 and not torch.allclose(out, img, atol=1e-3)
    assert torch.equal(augment_ref.jitter(torch.zeros(3, 8, 8, dtype=torch.float64), e), torch.zeros(3, 8, 8, dtype=torch.float64))
    grey = torch.rand(1, 8, 8, generator=g, dtype=torch.float64).expand(3, 8, 8)
    out = augment_ref.jitter(grey, e)
    assert torch.allclose(out[0], out[1], atol=1e-12) and torch.allclose(out[1], out[2], atol=1e-12)
    # a hue shift of a full turn is the identity; shifts that wrap past 1 and below 0 agree with their wrapped equivalents
    red = torch.tensor([0.9, 0.2, 0.1], dtype=torch.float64).view(3, 1, 1)
    for a, b in ((0.2, -0.8), (-0.2, 0.8)):
        o1 = augment_ref.jitter(red, _entry(1, 1, jitter=True, order=(3, 0, 1, 2), hue=a))
        o2 = augment_ref.jitter(red, _entry(1, 1, jitter=True, order=(3, 0, 1, 2), hue=b))
        assert torch.allclose(o1, o2, atol=1e-12)


def test_raw_dataset_contract():
    from evals.datasets import SyntheticNYURaw, build_loader

    ds = SyntheticNYURaw("train", num_samples=4, image_size=(32, 48))
    s = ds[0]
    assert s["image"].dtype == torch.uint8 and s["image"].shape == (32, 48, 3) and s["depth"].shape == (1, 32, 48)
    assert s["snorm"].shape == (3, 32, 48) and s["segmentation"].shape == (32, 48) and torch.equal(ds[0]["image"], s["image"])
    assert not torch.equal(ds[1]["image"], s["image"])
    im = s["image"].float()
    assert im.std() > 10 and (im[..., 0] - im[..., 1]).abs().mean() > 2  # structure and colour, not flat grey
    ld = build_loader({"name": "synthetic", "image_size": [16, 24], "num_batches": 2, "batch_size": 2, "raw": True}, "train", 2)
    b = next(iter(ld))
    assert b["image"].dtype == torch.uint8 and b["image"].shape == (2, 16, 24, 3)
    ld = build_loader({"name": "synthetic", "image_size": [16, 24], "num_batches": 2, "batch_size": 2}, "train", 2)
    assert next(iter(ld))["image"].dtype == torch.float32


def test_choice_file_and_abi_validation():
    import ctypes

    from mvp import config, lib

    cfg = config.compose("depth_training", ["dataset=synthetic_aug"])
    assert cfg["dataset"]["raw"] is True and cfg["dataset"]["augment_train"] is True and cfg["dataset"]["image_mean"] == "imagenet"
    so = lib.load()
    assert so.mvp_augment_partials_bytes(3) == 3 * 32 * 8
    a = lib.AugmentStatsArgs()
    assert so.mvp_augment_stats(ctypes.byref(a), None) == -1
    a = lib.AugmentStatsArgs(image=16, params=16, partials=16, partials_bytes=256, B=1, H=3, W=8, image_u8=1)
    assert so.mvp_augment_stats(ctypes.byref(a), None) == -1  # H < 4
    b = lib.AugmentApplyArgs(image=16, depth=16, params=16, out_image=16, out_depth=16, B=1, H=8, W=8, Ho=8, Wo=8, image_u8=1,
                             std_r=1.0, std_g=0.0, std_b=1.0)
    assert so.mvp_augment_apply(ctypes.byref(b), None) == -1  # a zero std
    b = lib.AugmentApplyArgs(image=16, depth=16, snorm=16, params=16, out_image=16, out_depth=16, B=1, H=8, W=8, Ho=8, Wo=8, image_u8=1,
                             std_r=1.0, std_g=1.0, std_b=1.0)
    assert so.mvp_augment_apply(ctypes.byref(b), None) == -1  # snorm without out_snorm
