"""mvp_knn_ratio (csrc/knn.hip) against the fp64 definition of tests/corr3d_ref.py, at the smallest shapes where it can go wrong.

The kernel's tiles are 128 queries x 128 targets, C is padded to 32, and the target range is cut into slices of whole tiles (one
tile per slice until the grid has 512 workgroups).  Bound of every comparison: delta = 4 * max|D32 - D64|, D32 being torch's own
fp32 CPU evaluation of the same formula on the same inputs (the reference arithmetic's error; the factor 4 covers another
summation order in fp32, not fp16-level error)."""
import math

import numpy as np
import pytest
import torch

import corr3d_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def run(q, t, vq=None, vt=None):
    """q [N0, C], t [N1, C] CPU fp32 -> the kernel's outputs on the CPU."""
    from mvp import corr3d

    d = lambda x: None if x is None else x.to(DEV)  # noqa: E731
    out = corr3d.knn_ratio(d(q.t().contiguous()), d(t.t().contiguous()), d(vq), d(vt))
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


def check(out, q, t, vq=None, vt=None, tie_share=0.01):
    """The acceptance of every row.  ``tie_share``: largest share of valid rows whose fp64 gap between best and second best may lie
    within 2 delta (index equality is not required there); None for inputs with ties built in."""
    nn, dist, weight, n_valid = out
    N0, N1 = q.shape[0], t.shape[0]
    vq = torch.ones(N0, dtype=torch.bool) if vq is None else vq.bool()
    vt = torch.ones(N1, dtype=torch.bool) if vt is None else vt.bool()
    assert n_valid.tolist() == [int(vq.sum()), int(vt.sum())]
    D64 = ref.distance_matrix(q, t)
    delta = 4 * float((ref.distance_matrix(q, t, torch.float32).double() - D64).abs().max())
    print(f"N0={N0} N1={N1} C={q.shape[1]} delta={delta:.3e}")
    assert 1e-8 < delta < 2e-5
    if int(vt.sum()) < 2:
        assert (nn == -1).all() and (weight == -math.inf).all()
        return delta
    dead = ~vq
    assert (nn[dead] == -1).all() and (weight[dead] == -math.inf).all()
    idx64, d64 = ref.two_nearest(D64, vt)
    idx64, d64, nn_v, dist_v, w_v = idx64[vq], d64[vq], nn[vq].long(), dist[vq].double(), weight[vq].double()
    assert (nn_v >= 0).all() and (nn_v < N1).all() and vt[nn_v].all()
    picked = D64[vq].gather(1, nn_v[:, None])[:, 0]
    print(f"  worst excess of the picked distance {float((picked - d64[:, 0]).max()):.3e}, of dist {float((dist_v - d64).abs().max()):.3e}")
    assert (picked <= d64[:, 0] + delta).all()
    assert ((dist_v - d64).abs() <= delta).all() and (dist_v[:, 0] <= dist_v[:, 1]).all()
    w64 = ref.ratio_weight(d64)
    bound = 4 * delta / d64[:, 1].clamp(min=1e-9)
    print(f"  worst weight error / bound {float(((w_v - w64).abs() / bound).max()):.3f}")
    assert ((w_v - w64).abs() <= bound).all()
    clear = (d64[:, 1] - d64[:, 0]) > 2 * delta
    assert (nn_v[clear] == idx64[clear, 0]).all()
    if tie_share is not None:
        assert (~clear).double().mean() <= tie_share, float((~clear).double().mean())
    return delta


def gaussian(N0, N1, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N0, C, generator=g), torch.randn(N1, C, generator=g)


# one row; N1 = 2 and 3; one short of and one past the 128-row query tile and the 128-column target tile; the tile itself; three
# target tiles in three slices with ragged edges on both sides
SHAPES = [(1, 333), (37, 2), (37, 3), (127, 129), (129, 127), (128, 128), (300, 333)]


@pytest.mark.parametrize("C", [40, 64, 200])  # not a multiple of the k step, exact, a multiple of 8 only
@pytest.mark.parametrize("N0,N1", SHAPES)
def test_knn_gaussian_features(N0, N1, C):
    q, t = gaussian(N0, N1, C, seed=1000 * C + N0 + N1)
    out = run(q, t)
    check(out, q, t)
    again = run(q, t)
    assert all(torch.equal(a, b) for a, b in zip(out, again))  # the merges are deterministic


def test_knn_two_tiles_per_slice():
    """129 query tiles leave 4 slices for 5 target tiles: two tiles per slice (the k loop runs across a tile boundary inside one
    workgroup), a ragged last tile, a last slice of one tile."""
    q, t = gaussian(128 * 128 + 1, 600, 40, seed=7)
    g = torch.Generator().manual_seed(8)
    vq, vt = torch.rand(q.shape[0], generator=g) > 0.1, torch.rand(600, generator=g) > 0.3
    check(run(q, t, vq, vt), q, t, vq, vt)


def test_knn_bicubic_upsampled_maps_with_masks():
    """The workload's kind of input: 6 x 6 maps of C = 64 upsampled bicubically to 24 x 24 (close neighbours everywhere), holes in both masks."""
    g = torch.Generator().manual_seed(5)
    up = lambda f: torch.nn.functional.interpolate(f[None], size=(24, 24), mode="bicubic")[0].reshape(64, -1).t().contiguous()  # noqa: E731
    q, t = up(torch.randn(64, 6, 6, generator=g)), up(torch.randn(64, 6, 6, generator=g))
    vq, vt = torch.rand(576, generator=g) > 0.2, torch.rand(576, generator=g) > 0.2
    check(run(q, t, vq, vt), q, t, vq, vt)
    check(run(q, t), q, t)


@pytest.fixture(scope="module")
def base():
    """40 queries against 400 targets (4 tiles = 4 slices), C = 64."""
    return gaussian(40, 400, 64, seed=99)


def test_duplicate_targets_resolve_to_the_lowest_index(base):
    q, t = base[0].clone(), base[1].clone()
    # five exact copies of one vector close to query 3, in four different tiles / slices (and two in one tile)
    spots = [131, 17, 399, 260, 140]
    t[spots] = q[3] + 0.05 * t[17]
    # and copies of query 5 itself
    t[[390, 129]] = q[5]
    out = run(q, t)
    check(out, q, t, tie_share=None)
    assert out[0][3] == 17 and out[0][5] == 129
    assert out[2][3] == 0.0 and out[1][3, 0] == out[1][3, 1]  # equal distances: ratio 1


def test_best_and_second_best_in_different_tiles_and_in_the_last_column(base):
    q, t = base[0].clone(), base[1].clone()
    t[399] = q[0] + 0.01 * t[399]   # best in the last column (last tile, ragged), second best in the first tile
    t[5] = q[0] + 0.05 * t[5]
    t[127] = q[1] + 0.01 * t[127]   # either side of a tile boundary
    t[128] = q[1] + 0.02 * t[128]
    t[300] = q[2] + 0.02 * t[300]   # second best in a later slice than the best
    t[200] = q[2] + 0.01 * t[200]
    out = run(q, t)
    check(out, q, t)
    assert out[0][:3].tolist() == [399, 127, 200]
    # the last VALID column with invalid ones after it
    vt = torch.ones(400, dtype=torch.bool)
    vt[380:] = False
    t[379] = q[4] + 0.01 * t[379]
    out = run(q, t, None, vt)
    check(out, q, t, None, vt)
    assert out[0][4] == 379 and out[0][0] == 5


def test_target_masks(base):
    q, t = base
    D = ref.distance_matrix(q, t)
    vt = torch.ones(400, dtype=torch.bool)
    vt[120:136] = False                      # straddling the first tile boundary
    vt[D.argmin(dim=1)] = False              # every query's true best is invalid
    out = run(q, t, None, vt)
    check(out, q, t, None, vt)
    assert vt[out[0].long()].all()
    two = torch.zeros(400, dtype=torch.bool)
    two[[130, 398]] = True                   # all but two invalid: both are the answer, in distance order
    out = run(q, t, None, two)
    check(out, q, t, None, two)
    assert set(out[0].tolist()) <= {130, 398}
    one = torch.zeros(400, dtype=torch.bool)
    one[250] = True                          # a single valid target: nothing to take a ratio with
    out = run(q, t, None, one)
    check(out, q, t, None, one)
    assert (out[0] == -1).all() and (out[2] == -math.inf).all() and out[3].tolist() == [40, 1]


def test_invalid_queries_leave_the_rest_unchanged(base):
    q, t = base
    full = run(q, t)
    vq = torch.ones(40, dtype=torch.bool)
    vq[[0, 7, 39]] = False
    out = run(q, t, vq, None)
    check(out, q, t, vq, None)
    assert (out[0][~vq] == -1).all() and (out[2][~vq] == -math.inf).all() and out[3].tolist() == [37, 400]
    for a, b in zip(out[:3], full[:3]):
        assert torch.equal(a[vq], b[vq])


def test_query_equal_to_targets(base):
    q, t = base[0].clone(), base[1].clone()
    t[333] = q[9]                            # identical to one target
    t[[12, 290]] = q[10]                     # duplicated twice among the targets
    out = run(q, t)
    delta = check(out, q, t, tie_share=None)
    assert out[0][9] == 333 and out[1][9, 0] <= delta
    assert out[0][10] == 12 and math.isfinite(out[2][10]) and 0.0 <= out[2][10] <= 1.0


def test_row_scale_does_not_change_the_indices(base):
    q, t = base
    g = torch.Generator().manual_seed(3)
    sq = torch.where(torch.rand(40, 1, generator=g) < 0.5, 1e-3, 1e3)
    st = torch.where(torch.rand(400, 1, generator=g) < 0.5, 1e-3, 1e3)
    a, b = run(q, t), run(q * sq, t * st)
    assert torch.equal(a[0], b[0])
    check(b, q * sq, t * st)
    np.testing.assert_allclose(b[2].numpy(), a[2].numpy(), rtol=0, atol=1e-5)
