"""CPU checks of the dense-CRF refinement: the fp64 oracle (tests/densecrf_ref.py) on its own fixtures, the Python layer's keyword and
refusals, the config override, the ABI registry and the host-side argument checks of the three exports (they run before any launch)."""
import ctypes

import numpy as np
import pytest

import densecrf_ref as ref


def test_zero_iterations_return_the_mask():
    rgb, m, _, _, _ = ref.fixture("noisy", 48)
    Q = ref.mean_field(ref.kernel_matrices(rgb), m.astype(np.float64), iters=0)
    assert np.array_equal(ref.map_of(Q, m.shape), m != 0)
    e = np.e
    assert np.allclose(Q[m.reshape(-1) != 0, 1], e / (1 + e), rtol=1e-15) and np.allclose(Q[m.reshape(-1) == 0, 1], 1 / (1 + e), rtol=1e-15)


@pytest.mark.parametrize("S", [48, 64])
def test_flat_fixtures_recover_the_true_mask(S):
    rgb, m, true, Q64, Q32 = ref.fixture("flat", S)
    assert ref.iou(m, true) < 0.5  # the input is a poor mask (0.36 at 48, 0.43 at 64) ...
    assert np.array_equal(ref.map_of(Q64, (S, S)), true)  # ... and the CRF returns the object exactly
    assert np.abs(Q64[:, 1] - 0.5).min() > 0.49


def test_fixture_inputs_are_the_ones_described():
    assert abs(ref.iou(ref.input_mask(48), ref.true_mask(48)) - 0.36) < 0.005
    assert abs(ref.iou(ref.input_mask(64), ref.true_mask(64)) - 0.43) < 0.005
    rgb = ref.image("flat", 48)
    t = ref.true_mask(48)
    assert np.abs(rgb[t].astype(int) - [200, 120, 60]).max() <= 4 and np.abs(rgb[~t].astype(int) - [40, 90, 160]).max() <= 4


def test_normaliser_properties():
    rgb, _, _, _, _ = ref.fixture("noisy", 48)
    K_g, K_b = ref.kernel_matrices(rgb)
    for K in (K_g, K_b):
        assert np.array_equal(K, K.T) and np.all(np.diag(K) == 1.0)
        s = K.sum(axis=1)
        assert s.min() >= 1.0  # the self term
        n = ref.normaliser(K)
        assert np.allclose(n * n * s, 1.0, rtol=1e-14)
        Kn = n[:, None] * K * n[None, :]  # the symmetric normalisation has the eigenvalue 1 with the eigenvector n^-1
        assert np.allclose(Kn @ (1.0 / n), 1.0 / n, rtol=1e-12)
    assert np.all(K_b <= K_g ** ((3.0 / 50.0) ** 2) + 1e-15)  # the colour term only lowers the wide spatial kernel
    const = np.full((5, 7, 3), 9, dtype=np.uint8)
    Kc_g, Kc_b = ref.kernel_matrices(const)
    assert np.allclose(Kc_b, Kc_g ** ((3.0 / 50.0) ** 2), rtol=1e-13)


def test_post_processing_rules():
    ring = np.zeros((9, 9), dtype=bool)
    ring[2:7, 2:7] = True
    ring[3:6, 3:6] = False
    assert ref.fill_holes(ring).sum() == 25
    a = np.zeros((4, 5), dtype=bool)
    a[0, :4] = True
    b = np.zeros((4, 5), dtype=bool)
    b[0, 2:] = True          # inter 2, union 5
    assert not ref.keeps(a, b)
    b[0, 1] = True           # inter 3, union 5
    assert ref.keeps(a, b)
    a[0, 3] = False
    b[0, 4] = False          # a = 0..2, b = 1..3: inter 2, union 4: 2 * inter == union is kept
    assert ref.keeps(a, b)
    assert ref.keeps(np.zeros((3, 3)), np.zeros((3, 3)))  # the empty union (NaN < 0.5 is false in the reference)


def test_refine_keyword_and_crf_flag():
    from evals.models.maskcut_processor import MaskCutProcessor
    from mvp import maskcut

    assert MaskCutProcessor(backbone=None).refine == "none"
    p = MaskCutProcessor(backbone=None, refine="dense_crf")
    assert p.refine == "dense_crf" and p.crf is False
    for bad in ("crf", "", None, "DENSE_CRF"):
        with pytest.raises(ValueError, match="refine"):
            MaskCutProcessor(backbone=None, refine=bad)
    with pytest.raises(NotImplementedError, match="crf") as e:
        MaskCutProcessor(backbone=None, crf=True, refine="dense_crf")
    assert 'refine="dense_crf"' in str(e.value)
    assert maskcut.REFINE_MODES == ("none", "dense_crf")


def test_config_override_selects_the_refinement():
    from mvp import config

    base = ["backbone=dino_b16", "backbone.return_kqv=true", "dataset=synthetic_voc"]
    assert "refine" not in config.compose("objectness_eval", base)
    assert config.compose("objectness_eval", base + ["+refine=dense_crf"])["refine"] == "dense_crf"


def test_structs_and_symbols_are_registered():
    from mvp import lib

    for cname, sym in (("mvp_crf_filter_args", "mvp_crf_filter"), ("mvp_crf_update_args", "mvp_crf_update"),
                       ("mvp_mask_finish_args", "mvp_mask_finish")):
        assert lib.SYMBOLS[sym] is lib.STRUCTS[cname]
        assert lib.load().mvp_sizeof(cname.encode()) == ctypes.sizeof(lib.STRUCTS[cname])


def test_densecrf_entry_refuses_cpu_tensors():
    import torch

    from evals.models import crf
    from mvp import densecrf, lib

    assert (crf.MAX_ITER, crf.POS_W, crf.POS_XY_STD, crf.Bi_W, crf.Bi_XY_STD, crf.Bi_RGB_STD) == (10, 7, 3, 10, 50, 5)
    with pytest.raises(lib.MvpError, match="no CPU fallback"):
        crf.densecrf(torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(4, 4))
    with pytest.raises(lib.MvpError, match="no CPU fallback"):
        densecrf.densecrf_batch(torch.zeros(1, 3, 4, 4, dtype=torch.uint8), torch.zeros(1, 1, 4, 4, dtype=torch.uint8))
    with pytest.raises(lib.MvpError, match="no CPU fallback"):
        densecrf.refine_and_union(torch.zeros(1, 3, 4, 4, dtype=torch.uint8), torch.zeros(1, 1, 4, 4, dtype=torch.uint8))


def test_pair_count_follows_the_skip_rule():
    from mvp import ops

    assert ops.crf_filter_pairs(1, 16, 16, 1 / 9) == 256.0 * 256.0
    # sigma = 3: tiles more than two tiles apart are skipped (a gap of 17 pixels gives 2^-23, of 33 pixels 2^-87)
    assert ops.crf_filter_pairs(2, 64, 16, 1 / 9) == 2 * (4 + 2 * 3 + 2 * 2) * 65536.0
    # sigma = 50 at 480^2: only tiles at least 372 pixels apart go; counted here tile pair by tile pair
    t = np.arange(30)
    gap = np.maximum(0, np.abs(t[:, None] - t[None, :]) * 16 - 15) ** 2
    d2 = gap[:, None, :, None] + gap[None, :, None, :]  # [ty, tx, sy, sx]
    kept = int((0.5 * np.log2(np.e) / 2500 * d2 < 40.0).sum())
    assert 0.8 * 900 * 900 < kept < 900 * 900 and ops.crf_filter_pairs(1, 480, 480, 1 / 2500) == kept * 65536.0


# ----------------------------------------------------------------------------- MVP_EINVAL, every condition the header names, once each
P4, P1 = 4096, 4097  # fake pointers (nothing is launched on a rejected call)


def _einval(fn, args):
    from mvp import lib

    return getattr(lib.load(), fn)(ctypes.byref(args), None) == -1


def _filter(**kw):
    from mvp import lib

    base = dict(rgb=P4, out=P4, active=0, in_stride=2 * 48 * 40, out_stride=2 * 48 * 40, B=2, F=2, H=48, W=40, inv_var_xy=1 / 9, inv_var_rgb=1 / 25)
    base["in"] = P4
    base.update(kw)
    return lib.CrfFilterArgs(**base)


@pytest.mark.parametrize("bad", [dict(rgb=0), dict(out=0), dict(B=0), dict(B=65536), dict(F=0), dict(F=9), dict(H=0), dict(W=0), dict(H=4097),
                                 dict(H=4096, W=2048, in_stride=1 << 30, out_stride=1 << 30), dict(in_stride=2 * 48 * 40 - 1),
                                 dict(out_stride=2 * 48 * 40 - 1), dict(inv_var_xy=0.0), dict(inv_var_rgb=-1.0), dict(inv_var_xy=float("inf")),
                                 dict(inv_var_rgb=float("nan")), {"in": P1}, dict(out=P1)])
def test_filter_einval(bad):
    assert _einval("mvp_crf_filter", _filter(**bad))


def _update(**kw):
    from mvp import lib

    base = dict(mask=P4, active=0, norm_g=P4, norm_b=P4, ones_g=P4, ones_b=P4, filt_g=P4, filt_b=P4, q=P4, x_g=P4, x_b=P4, map=P4,
                stride=3 * 100, N=100, B=2, F=3, mode=2, w_g=7.0, w_b=10.0)
    base.update(kw)
    return lib.CrfUpdateArgs(**base)


@pytest.mark.parametrize("bad", [dict(norm_g=0), dict(norm_b=0, mode=0), dict(mask=0), dict(q=0, mode=1), dict(x_g=0), dict(x_b=0), dict(ones_g=0),
                                 dict(ones_b=0), dict(filt_g=0), dict(filt_b=0), dict(B=0), dict(B=65536), dict(F=0), dict(F=9), dict(N=0),
                                 dict(N=(1 << 22) + 1, stride=1 << 30), dict(stride=299), dict(mode=3), dict(mode=-1), dict(norm_g=P1, mode=0),
                                 dict(mask=P1), dict(q=P1), dict(filt_b=P1)])
def test_update_einval(bad):
    assert _einval("mvp_crf_update", _update(**bad))


def _finish(**kw):
    from mvp import lib

    base = dict(map=P4, ref=P4, active=0, refined=P4, kept=0, union_mask=P4, stride=3 * 480 * 480, B=2, F=3, H=480, W=480)
    base.update(kw)
    return lib.MaskFinishArgs(**base)


@pytest.mark.parametrize("bad", [dict(map=0), dict(ref=0), dict(refined=0), dict(B=0), dict(B=65536), dict(F=0), dict(F=65), dict(H=0), dict(W=0),
                                 dict(H=1025, W=1024, stride=1 << 30), dict(H=32769, W=1, stride=1 << 30), dict(stride=3 * 480 * 480 - 1)])
def test_finish_einval(bad):
    assert _einval("mvp_mask_finish", _finish(**bad))
