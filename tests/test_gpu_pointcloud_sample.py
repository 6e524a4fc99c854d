"""mvp_pointcloud_sample (csrc/pointcloud.hip) against the fp64 definition of tests/corr_depth_ref.py.  The bound of a case is
delta_s = 4 * max|S32 - S64|, S32 being torch's fp32 CPU evaluation of the same formulas (projection included); sampled values are
continuous in the point, so the depth grids 3 x and 4 x finer than the map (whose border rows normalise to duplicates) are
checked like any other."""
import math

import pytest
import torch

import corr_depth_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K68 = torch.tensor([[11.5, 0.0, 8.6], [0.0, 12.25, 5.4], [0.0, 0.0, 1.0]])  # for a 12 x 16 image; fx != fy, off-centre principal point


def _run(feat, K, pc, image_shape, ld_out=None, sentinel=None, want_valid=True):
    """One ABI call -> (out [C, ld_out] on the host, valid [N] uint8 or None)."""
    from mvp import ops

    C, fh, fw = feat.shape
    N = pc.shape[0]
    ld = N if ld_out is None else ld_out
    out = torch.full((C, ld), math.nan if sentinel is None else sentinel, dtype=torch.float32, device=DEV)
    valid = torch.full((N,), 7, dtype=torch.uint8, device=DEV) if want_valid else None
    ops.pointcloud_sample(feat.to(DEV).contiguous(), pc.to(DEV).contiguous(), K.to(DEV).contiguous(), out, valid, C, fh, fw, N,
                          image_shape[0], image_shape[1], ld)
    return out.cpu(), None if valid is None else valid.cpu()


def _check(feat, K, pc, image_shape, **kw):
    S64 = ref.sample_pointcloud_features(feat, K, pc, image_shape)
    S32 = ref.sample_pointcloud_features(feat, K, pc, image_shape, torch.float32)
    delta = 4 * float((S32.double() - S64).abs().max())
    out, valid = _run(feat, K, pc, image_shape, **kw)
    got = out[:, :pc.shape[0]].t().double()
    err = float((got - S64).abs().max())
    print(f"C={feat.shape[0]} map {tuple(feat.shape[1:])} N={pc.shape[0]} image {tuple(image_shape)}: delta_s {delta:.2e}, max error {err:.2e}")
    assert 1e-8 < delta < 1e-4
    assert torch.isfinite(got).all() and err <= delta
    _, _, ok = ref.sample_positions(K, pc, feat.shape[1:], image_shape)
    assert (got[~ok] == 0).all()  # exactly 0, every channel
    assert torch.equal(valid, (pc[:, 2] > 0).to(torch.uint8))
    return out, ok


def _arbitrary_points(g, N, K, H, W):
    """Points built from chosen pixel positions: inside the image, on the half-texel band around it, far outside; then rows with
    z = 0, z < 0 and a NaN coordinate."""
    uv = torch.rand(N, 2, generator=g) * torch.tensor([W + 6.0, H + 6.0]) - 3.0
    z = torch.rand(N, generator=g) * 2 + 0.3
    pc = (torch.cat((uv, torch.ones(N, 1)), dim=1) * z[:, None]) @ K.inverse().t()
    pc[-12:-8, 2] = 0.0
    pc[-8:-4, 2] = -0.8
    pc[-4, 0], pc[-3, 1], pc[-2, 2], pc[-1, :] = math.nan, math.nan, math.nan, math.nan
    return pc


def test_arbitrary_points_inside_border_outside_and_degenerate():
    g = torch.Generator().manual_seed(5)
    K = torch.tensor([[7.1, 0.0, 4.9], [0.0, 6.4, 3.1], [0.0, 0.0, 1.0]])
    feat = torch.randn(5, 3, 4, generator=g)
    pc = _arbitrary_points(g, 130, K, 7, 9)
    x, y, ok = ref.sample_positions(K, pc, (3, 4), (7, 9))
    band = ok & ((x < 0) | (x > 3) | (y < 0) | (y > 2))
    inner = ok & ~band
    assert int(inner.sum()) >= 10 and int(band.sum()) >= 20 and int((~ok).sum()) >= 30 and not ok[-12:].any(), (int(inner.sum()), int(band.sum()))
    out, _ = _check(feat, K, pc, (7, 9))
    assert (out[:, band].abs().max(dim=0).values > 0).all()  # the band is sampled (scaled by the padding), not dropped


@pytest.mark.parametrize("k", [2, 3, 4])
def test_grid_pointclouds_at_2x_3x_4x(k):
    """The clouds the evaluation samples: a 6 x 8 map under depth grids of 12 x 16, 18 x 24, 24 x 32 with holes.  3 x puts row 1 on
    y = 0 (an integer) and row 0 at y = -1/3; 4 x puts rows 0 and 1 below 0."""
    g = torch.Generator().manual_seed(100 + k)
    H, W = 6 * k, 8 * k
    K = K68.clone()
    K[:2] *= k / 2
    feat = torch.randn(64, 6, 8, generator=g)
    depth = torch.rand(1, H, W, generator=g) * 2 + 0.5
    depth[0][torch.rand(H, W, generator=g) < 0.3] = 0.0
    pc = ref.grid_to_pointcloud(K.inverse(), depth, torch.float32)
    x, y, ok = ref.sample_positions(K, pc, (6, 8), (H, W))
    hole = depth.reshape(-1) == 0
    # every real point projects back into its own pixel; a hole is the point 0, which the clamp sends to u = v = 0 (x = y = -0.5: the
    # corner texel at a quarter weight, as grid_sample would give; the evaluation masks it by ``valid``)
    assert ok.all() and (pc[hole] == 0).all() and (x[hole] == -0.5).all() and (y[hole] == -0.5).all()
    assert bool((y[ok] < 0).any()) and (k != 3 or bool(((y - y.round()).abs()[ok] < 1e-6).any()))
    _check(feat, K, pc, (H, W))


@pytest.mark.parametrize("case", ["map_1x1", "one_point", "one_channel"])
def test_smallest_sizes(case):
    g = torch.Generator().manual_seed({"map_1x1": 11, "one_point": 12, "one_channel": 13}[case])
    if case == "map_1x1":   # everything is border: x, y in (-1, 1) see the single texel scaled by the padding
        feat, pc = torch.randn(9, 1, 1, generator=g), _arbitrary_points(g, 70, K68, 12, 16)
    elif case == "one_point":
        feat, pc = torch.randn(64, 6, 8, generator=g), torch.tensor([[0.13, -0.08, 1.7]])
    else:
        feat, pc = torch.randn(1, 6, 8, generator=g), _arbitrary_points(g, 130, K68, 12, 16)
    _, ok = _check(feat, K68, pc, (12, 16))
    assert ok.any()


def test_padding_columns_survive_and_valid_is_optional():
    g = torch.Generator().manual_seed(21)
    feat, pc = torch.randn(20, 6, 8, generator=g), _arbitrary_points(g, 133, K68, 12, 16)
    out, _ = _check(feat, K68, pc, (12, 16), ld_out=140, sentinel=-123.5)
    assert out.shape == (20, 140) and (out[:, 133:] == -123.5).all()
    plain, none = _run(feat, K68, pc, (12, 16), want_valid=False)
    assert none is None and torch.equal(plain, out[:, :133])


def test_two_calls_give_the_same_bits():
    g = torch.Generator().manual_seed(22)
    feat, pc = torch.randn(40, 6, 8, generator=g), _arbitrary_points(g, 600, K68, 12, 16)
    a, va = _run(feat, K68, pc, (12, 16))
    b, vb = _run(feat, K68, pc, (12, 16))
    assert torch.equal(a, b) and torch.equal(va, vb) and not torch.isnan(a).any()
