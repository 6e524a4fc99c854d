"""BEiT v2 on the HIP path (evals.models.beit_v2.BEiTV2; attention with a per-head relative-position bias, the replay pass after
``fc_norm``): tiny, mid and full-size goldens built from the reference's own VisionTransformer, the fp64 restatement, ``add_norm`` and
``return_cls``, grouped and span forwards, and an engine without tables."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden, rel_l2

sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

import beit_ref  # noqa: E402
import make_goldens_beit as mg  # noqa: E402
from make_goldens_dinov2 import sample_index  # noqa: E402

pytestmark = pytest.mark.gpu
PRECISIONS = ["f16x2", "bf16x3"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _beit(cfg, dev, precision, **kw):
    from evals.models.beit_v2 import BEiTV2

    return BEiTV2(weights=mg.state_dict(cfg), img_size=cfg["img_size"], precision=precision, **kw).to(dev).eval()


def _errs(outs, refs):
    return [rel_l2(o.detach().cpu().numpy(), np.asarray(r)) for o, r in zip(outs, refs)]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_tiny_vs_goldens_and_restatement(dev, precision):
    """4 x 6 grid (N = 25), images resized from 80 x 112: every tap without and with add_norm (train-mode BatchNorm1d over all tokens, class
    token included), and return_cls, against the reference's goldens; the dense taps against tests/beit_ref.py in fp64 too."""
    g = load_golden("beit_tiny.npz")
    images = torch.from_numpy(g["images"]).to(dev)
    m = _beit(mg.TINY, dev, precision, return_multilayer=True)
    assert m.engine().rel_pos_grid == (4, 6) and m.engine().pos_embed is None
    with torch.no_grad():
        outs = m(images)
    errs = _errs(outs, [g[f"dense_tap{j}"] for j in range(4)])
    ref = beit_ref.features(mg.state_dict(mg.TINY), torch.from_numpy(g["images"]).double(), [0, 1, 2, 3], img_size=mg.TINY["img_size"])
    errs_ref = _errs(outs, [r.numpy() for r in ref])
    mn = _beit(mg.TINY, dev, precision, return_multilayer=True, add_norm=True).train()
    with torch.no_grad():
        outs_n = mn(images)
    errs_n = _errs(outs_n, [g[f"norm_tap{j}"] for j in range(4)])
    mc = _beit(mg.TINY, dev, precision, return_cls=True, add_norm=True).train()
    with torch.no_grad():
        cls = mc(images)
    err_c = rel_l2(cls.cpu().numpy(), g["cls"])
    print(f"\n[beit tiny {precision}] rel-L2 per tap vs goldens: " + " ".join(f"{e:.2e}" for e in errs) + " | vs fp64 restatement: " +
          " ".join(f"{e:.2e}" for e in errs_ref) + " | add_norm: " + " ".join(f"{e:.2e}" for e in errs_n) + f" | return_cls: {err_c:.2e}")
    assert all(o.shape == (2, 128, 4, 6) for o in outs) and cls.shape == (2, 128)
    assert max(errs) < 1e-3 and max(errs_ref) < 1e-3 and max(errs_n) < 1e-3 and err_c < 1e-3, (errs, errs_ref, errs_n, err_c)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["mid", "full"])
def test_sampled_goldens(dev, precision, name):
    """mid: 14 x 14 grid (N = 197, the production token count, the resident kernel) at C = 128; full: ViT-B/16 at 224^2, B = 2."""
    cfg = mg.MID if name == "mid" else mg.FULL
    g = load_golden("beit_mid.npz" if name == "mid" else "beit_full_sampled.npz")
    np.testing.assert_allclose(mg.checksums(mg.state_dict(cfg)), g["checksums"], rtol=1e-9)
    images = mg.images(cfg).to(dev)
    for tag, norm in (("dense", False), ("norm", True)):
        m = _beit(cfg, dev, precision, return_multilayer=True, add_norm=norm)
        m.train(norm)
        with torch.no_grad():
            outs = m(images)
        errs = []
        for j, o in enumerate(outs):
            o = o.cpu().numpy()
            assert tuple(g[f"{tag}_tap{j}_shape"]) == o.shape
            errs.append(rel_l2(o.reshape(-1)[sample_index(o.size)], g[f"{tag}_tap{j}"]))
        print(f"\n[beit {name} {precision} {tag}] rel-L2 per tap vs sampled goldens: " + " ".join(f"{e:.2e}" for e in errs))
        assert max(errs) < 1e-3, errs
    with torch.no_grad():
        cls = _beit(cfg, dev, precision, return_cls=True)(images)
    err_c = rel_l2(cls.cpu().numpy(), g["cls"])
    print(f"[beit {name} {precision}] return_cls rel-L2 {err_c:.2e}")
    assert err_c < 1e-3


def test_replay_flag_is_not_a_no_op_and_wrong_grid_is_refused(dev):
    from mvp import lib

    m = _beit(mg.TINY, dev, "bf16x3", return_multilayer=True)
    eng = m.engine()
    images = mg.images(mg.TINY)[:, :, :64, :96].contiguous().to(dev)
    with torch.no_grad():
        once = eng.forward_taps(images, m.multilayers, bn=None, bn_mode=2, pack=False)
        twice = eng.forward_taps(images, m.multilayers, bn=None, bn_mode=2, pack=False, replay_after_norm=True)
    ref = beit_ref.features(mg.state_dict(mg.TINY), images.double().cpu(), [0, 1, 2, 3], img_size=mg.TINY["img_size"], replay=False)
    assert max(_errs(once, [r.numpy() for r in ref])) < 1e-3
    assert min(_errs(once, [t.cpu().numpy() for t in twice])) > 1e-2
    with pytest.raises(lib.MvpError, match=r"4 x 4 token grid.*4 x 6"):
        eng.forward_taps(images[:, :, :, :64].contiguous(), m.multilayers, bn=None, bn_mode=2, pack=False)
    from mvp.vit import ViTEngine
    from oracle import vit as ovit

    with pytest.raises(lib.MvpError, match="fc_norm"):
        ViTEngine(ovit.make_vit_weights(embed_dim=128, depth=4, seed=1), heads=2, device=dev).forward_taps(
            images[:, :, :, :64].contiguous(), [3], bn=None, bn_mode=2, pack=False, replay_after_norm=True)


@pytest.mark.parametrize("name", ["tiny", "mid"])
def test_grouped_forward_equals_single_batches(dev, name):
    """Two batches stacked into one forward give each batch exactly the bits of its own forward: the bias is per head, not per image."""
    cfg = mg.TINY if name == "tiny" else mg.MID
    m = _beit(cfg, dev, "f16x2", return_multilayer=True)
    eng = m.engine()
    imgs = torch.randn(8, 3, *cfg["img_size"], generator=torch.Generator().manual_seed(9)).to(dev)
    with torch.no_grad():
        grouped = eng.forward_taps(imgs, m.multilayers, bn=None, bn_mode=2, pack=False, want_cls=True, groups=2, replay_after_norm=True)
        for gidx in range(2):
            single = eng.forward_taps(imgs[4 * gidx:4 * (gidx + 1)].contiguous(), m.multilayers, bn=None, bn_mode=2, pack=False, want_cls=True,
                                      replay_after_norm=True)
            for a, b in zip(grouped[gidx], single):
                assert torch.equal(a, b), gidx
            for a, b in zip(grouped[gidx].cls, single.cls):
                assert torch.equal(a, b), gidx


def _build(cfg, dev):
    from evals.models.probes import DepthHead
    from evals.utils.optim import cosine_decay_linear_warmup
    from mvp.optim import FlatAdamW

    model = _beit(cfg, dev, "f16x2", return_multilayer=True, add_norm=True).train()
    torch.manual_seed(11)
    probe = DepthHead(feat_dim=model.feat_dim, head_type="linear", kernel_size=1, prediction_type="bindepth", min_depth=0.001, max_depth=10).to(dev)
    opt = FlatAdamW([{"params": probe.parameters(), "lr": 1e-3}])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda e: cosine_decay_linear_warmup(e, 100, 10))
    return model, probe, opt, sched


@pytest.mark.parametrize("name", ["tiny", "mid"])
def test_span_pipeline_with_graphs_is_bit_identical_to_serial(dev, name):
    """B = 4, forwards over spans of 6 images (every other forward starts with the 2 images of a batch the previous span cut), graph replay
    (the captured graphs hold the dense bias arrays' addresses: ViTEngine.slot_state), grouped tap BN — losses, probe weights, AdamW state and
    tap-BN running statistics equal the one-batch-at-a-time loop's bit for bit."""
    from evals.utils.losses import DepthLoss
    from mvp.pipeline import FeaturePipeline, pipelined_features
    from mvp.train import train_depth_step

    cfg = mg.TINY if name == "tiny" else mg.MID
    n, B, span = 6, 4, 6
    H, W = cfg["img_size"]
    bs = []
    for s in range(n):
        g = torch.Generator().manual_seed(800 + s)
        bs.append({"image": torch.randn(B, 3, H, W, generator=g).to(dev), "depth": (torch.rand(B, 1, H, W, generator=g) * 9.0 + 0.05).to(dev)})
    loss_fn = DepthLoss()

    def state(model, opt, losses):
        torch.cuda.synchronize()
        bn = [torch.cat([b.running_mean, b.running_var]).cpu().numpy() for b in model.batchnorms]
        return (torch.stack(losses).cpu().numpy(), opt.flat_param.cpu().numpy().copy(), opt.exp_avg_sq.cpu().numpy().copy(), bn,
                [int(b.num_batches_tracked) for b in model.batchnorms])

    model, probe, opt, sched = _build(cfg, dev)
    losses = [train_depth_step(model, probe, opt, sched, loss_fn, b["image"], b["depth"].clone()) for b in bs]
    ref = state(model, opt, losses)
    model, probe, opt, sched = _build(cfg, dev)
    pipe = FeaturePipeline(model, 2, graphs=True, group=2, span=span)
    losses = []
    for b, f in pipelined_features(model, bs, pipe=pipe):
        losses.append(train_depth_step(model, probe, opt, sched, loss_fn, None, b["depth"].clone(), feats=f))
    assert pipe.span == span and all(e["graph"] is not None for e in pipe._graphs.values())
    got = state(model, opt, losses)
    for i in range(3):
        np.testing.assert_array_equal(got[i], ref[i])
    for a, b in zip(got[3], ref[3]):
        np.testing.assert_array_equal(a, b)
    assert got[4] == ref[4] == [n] * 4


def test_engine_without_tables_is_unchanged(dev, golden):
    """A seeded DINO ViT (tiny dims) launches what it launched before: no block carries a bias, two runs give the same bits, and the
    token stream meets the existing oracle golden."""
    from mvp.vit import ViTEngine
    from oracle import vit as ovit

    g = golden("vit_tiny128.npz")
    sd = ovit.make_vit_weights(embed_dim=128, depth=4, seed=11)
    eng = ViTEngine(sd, heads=2, device=dev)
    assert eng.rel_pos_grid is None and eng.fc_norm is None and all("att_bias" not in b for b in eng.blocks) and eng._zero_c is None
    images = torch.from_numpy(g["a_images"]).to(dev)
    a, b = eng.forward_tokens(images), eng.forward_tokens(images)
    assert torch.equal(a, b)
    assert rel_l2(eng.forward_tokens(images, 0).cpu().numpy(), g["a_tokens0"]) < 1e-3
    bn = [dict(weight=torch.ones(128, device=dev), bias=torch.zeros(128, device=dev),
               running_mean=torch.zeros(128, device=dev), running_var=torch.ones(128, device=dev)) for _ in range(4)]
    taps = eng.forward_taps(images, [0, 1, 2, 3], bn=bn)
    for i, t in enumerate(taps):
        assert rel_l2(t.cpu().numpy(), g[f"a_tap{i}"]) < 1e-3, i
