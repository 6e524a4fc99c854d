"""SAM image encoders on the HIP path (evals.models.sam.SAM: windowed attention through row gathers, decomposed relative-position terms,
attention with the decomposed bias): tiny, mid and full-size goldens built from transformers' SamVisionEncoder in the three precisions,
single tap and gap, a second size after the first, graph capture, a grouped forward, the choice file through train_depth's builder, a
span-pipelined training loop against the serial one, and the interleaved operand form against the separate one."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden, rel_l2

sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

import make_goldens_sam as mg  # noqa: E402
import sam_ref  # noqa: E402
from make_goldens_dinov2 import sample_index  # noqa: E402

pytestmark = pytest.mark.gpu
BOUNDS = {"f16x2": 1e-3, "bf16x3": 1e-3, "bf16": 3e-2}  # the feature contract; one bf16 product gets what its sibling tests give it


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _sam(cfg, dev, precision, **kw):
    from evals.models.sam import SAM

    return SAM("vit_b", weights=mg.state_dict(cfg), precision=precision, **kw).to(dev).eval()


@pytest.mark.parametrize("precision", list(BOUNDS))
def test_tiny_vs_goldens(dev, precision):
    """5 x 7 grid, window 3 (both dimensions padded, pad rows are keys), resampled position table, global tables interpolated 15 -> 9 / 13."""
    g = load_golden("sam_tiny.npz")
    m = _sam(mg.TINY, dev, precision, return_multilayer=True)
    with torch.no_grad():
        outs = m(torch.from_numpy(g["images"]).to(dev))
    errs = [rel_l2(o.cpu().numpy(), g[f"tap{j}"]) for j, o in enumerate(outs)]
    print(f"\n[sam tiny {precision}] rel-L2 per tap vs goldens: " + " ".join(f"{e:.2e}" for e in errs))
    assert all(o.shape == (2, 128, 5, 7) for o in outs) and m.engine().n_prefix == 0
    assert [b["window"] for b in m.engine().blocks] == [3, 0, 3, 0]
    assert max(errs) < BOUNDS[precision], errs


@pytest.mark.parametrize("precision", list(BOUNDS))
@pytest.mark.parametrize("name", ["mid", "full"])
def test_sampled_goldens(dev, precision, name):
    """mid: 16 x 16 grid, window 14 (four windows of 196, the resident kernel), B = 2; full: ViT-B geometry at 224^2 (one window, global
    tables 127 -> 27) and 512^2 (nine windows; global N = 1024 on the streaming kernel)."""
    cfg = mg.MID if name == "mid" else mg.FULL
    g = load_golden("sam_mid.npz" if name == "mid" else "sam_full_sampled.npz")
    np.testing.assert_allclose(mg.checksums(mg.state_dict(cfg)), g["checksums"], rtol=1e-9)
    m = _sam(cfg, dev, precision, return_multilayer=True)
    for size in cfg["sizes"]:
        tag = "" if len(cfg["sizes"]) == 1 else f"s{size[0]}_"
        with torch.no_grad():
            outs = m(mg.images(cfg, size).to(dev))
        errs = []
        for j, o in enumerate(outs):
            o = o.cpu().numpy()
            assert tuple(g[f"{tag}tap{j}_shape"]) == o.shape
            errs.append(rel_l2(o.reshape(-1)[sample_index(o.size)], g[f"{tag}tap{j}"]))
        print(f"\n[sam {name} {precision} {size}] rel-L2 per tap vs sampled goldens: " + " ".join(f"{e:.2e}" for e in errs))
        assert max(errs) < BOUNDS[precision], errs


def test_single_tap_gap_and_second_size(dev):
    """``layer=``, ``gap``; a second forward at another size after the first matches the oracle evaluated from the CHECKPOINT's table
    (never the resampled one), and the first size again gives the first result's bits."""
    g = load_golden("sam_tiny.npz")
    images = torch.from_numpy(g["images"]).to(dev)
    with torch.no_grad():
        one = _sam(mg.TINY, dev, "f16x2", layer=1)(images)
        gap = _sam(mg.TINY, dev, "f16x2", layer=1, output="gap")(images)
    assert one.shape == (2, 128, 5, 7) and rel_l2(one.cpu().numpy(), g["tap1"]) < 1e-3
    assert gap.shape == (2, 128) and torch.equal(gap, one.mean(dim=(2, 3)))
    m = _sam(mg.TINY, dev, "f16x2", return_multilayer=True)
    other = torch.randn(2, 3, 96, 64, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        a = [t.clone() for t in m(images)]
        b = m(other.to(dev))
        c = m(images)
    ref, _ = sam_ref.forward(mg.state_dict(mg.TINY), other, [0, 1, 2, 3])
    errs = [rel_l2(o.cpu().numpy(), r.numpy()) for o, r in zip(b, ref)]
    print(f"\n[sam tiny second size 6 x 4] rel-L2 per tap vs the oracle: " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < 1e-3, errs
    assert all(torch.equal(x, y) for x, y in zip(a, c))


def test_graph_capture_and_grouped_forward(dev):
    """A forward under graph capture replays to the eager bits (index tables, relative-position tables and workspaces are in
    slot_state); two batches stacked into one forward give each batch exactly the bits of its own forward (windows are per image)."""
    m = _sam(mg.TINY, dev, "f16x2", return_multilayer=True)
    eng = m.engine()
    imgs = torch.randn(4, 3, 80, 112, generator=torch.Generator().manual_seed(9)).to(dev)
    with torch.no_grad():
        eager = [t.clone() for t in eng.forward_taps(imgs, m.multilayers, bn=None, bn_mode=2, pack=False)]
        grouped = eng.forward_taps(imgs, m.multilayers, bn=None, bn_mode=2, pack=False, groups=2)
        for gi in range(2):
            single = eng.forward_taps(imgs[2 * gi:2 * gi + 2].contiguous(), m.multilayers, bn=None, bn_mode=2, pack=False)
            for a, b in zip(grouped[gi], single):
                assert torch.equal(a, b), gi
        torch.cuda.synchronize()
        static = imgs.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            eng.forward_taps(static, m.multilayers, bn=None, bn_mode=2, pack=False)  # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = eng.forward_taps(static, m.multilayers, bn=None, bn_mode=2, pack=False)
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
    assert m.supports_grouping()
    state = eng.slot_state(0)
    assert all(any(t is s for s in state) for pu in eng._sam_win.values() for t in pu[:2]) and len(eng._sam_rel) >= 2
    for a, b in zip(outs, eager):
        assert torch.equal(a, b)


def test_choice_file_through_the_backbone_builder(dev):
    """configs/backbone/sam_base.yaml as train_depth instantiates it (random weights: no checkpoint here), at 224^2."""
    import warnings

    import yaml

    from mvp import config

    node = yaml.safe_load(open(os.path.join(config.CONFIG_DIR, "backbone", "sam_base.yaml")))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = config.instantiate(node, return_multilayer=True).to(dev).eval()
    with torch.no_grad():
        outs = model(torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(1)).to(dev))
    assert len(outs) == 4 and all(o.shape == (1, 768, 14, 14) and bool(torch.isfinite(o).all()) for o in outs)
    assert [b["window"] for b in model.engine().blocks] == [14, 14, 0] * 4


def test_span_pipeline_with_graphs_is_bit_identical_to_serial(dev):
    """The mid model (256 rows per image, four windows of 196 padded rows each, global blocks 1 and 3), B = 4 at 256^2: forwards over
    spans of 6 images (a span ends inside a batch; windows are per image, so it still holds whole windows) with graph replay and groups of
    two — losses, probe weights and AdamW state equal the one-batch-at-a-time loop's bit for bit."""
    from evals.models.probes import DepthHead
    from evals.utils.losses import DepthLoss
    from evals.utils.optim import cosine_decay_linear_warmup
    from mvp.optim import FlatAdamW
    from mvp.pipeline import FeaturePipeline, pipelined_features
    from mvp.train import train_depth_step

    n, B, span = 5, 4, 6
    bs = []
    for s in range(n):
        g = torch.Generator().manual_seed(900 + s)
        bs.append({"image": torch.randn(B, 3, 256, 256, generator=g).to(dev), "depth": (torch.rand(B, 1, 256, 256, generator=g) * 9.0 + 0.05).to(dev)})
    loss_fn = DepthLoss()

    def build():
        model = _sam(mg.MID, dev, "f16x2", return_multilayer=True)
        torch.manual_seed(11)
        probe = DepthHead(feat_dim=model.feat_dim, head_type="linear", kernel_size=1, prediction_type="bindepth", min_depth=0.001, max_depth=10).to(dev)
        opt = FlatAdamW([{"params": probe.parameters(), "lr": 1e-3}])
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda e: cosine_decay_linear_warmup(e, 100, 10))
        return model, probe, opt, sched

    def state(opt, losses):
        torch.cuda.synchronize()
        return torch.stack(losses).cpu().numpy(), opt.flat_param.cpu().numpy().copy(), opt.exp_avg_sq.cpu().numpy().copy()

    model, probe, opt, sched = build()
    ref = state(opt, [train_depth_step(model, probe, opt, sched, loss_fn, b["image"], b["depth"].clone()) for b in bs])
    model, probe, opt, sched = build()
    pipe = FeaturePipeline(model, 2, graphs=True, group=2, span=span)
    losses = []
    for b, f in pipelined_features(model, bs, pipe=pipe):
        losses.append(train_depth_step(model, probe, opt, sched, loss_fn, None, b["depth"].clone(), feats=f))
    assert pipe.span == span and all(e["graph"] is not None for e in pipe._graphs.values())
    assert [b["window"] for b in model.engine().blocks] == [14, 0, 14, 0]
    got = state(opt, losses)
    assert np.isfinite(got[0]).all()
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(a, b)


def test_interleaved_operands_equal_the_separate_form_bit_for_bit(dev, monkeypatch):
    """ViT-B width, two windowed blocks (w = 7 on a 13 x 13 grid: padded to 14 x 14) and a global one, B = 120: M = 20 280 and the padded
    Mp = 23 520 rows send all five GEMM shapes of a block to the large-M kernel, so LayerNorm's output, the window-ordered copies, the
    attention output and fc1's output are hi|lo-interleaved arrays and both gathers copy interleaved rows.  The taps equal those of the
    same engine with MVP_ILV=0 (separate arrays) bit for bit."""
    from evals.models.sam import SAM
    from mvp import backbone as bb
    from mvp import ops

    sd = bb.random_sam_state_dict(768, 3, 16, 7, (2,), seed=31)
    x = torch.randn(120, 3, 208, 208, generator=torch.Generator().manual_seed(32)).to(dev)

    def run():
        m = SAM("vit_b", weights=sd, precision="f16x2", return_multilayer=True, layer=-1).to(dev).eval()
        eng = m.engine()
        with torch.no_grad():
            outs = [t.clone() for t in eng.forward_taps(x, [0, 1, 2], bn=None, bn_mode=2, pack=False)]
        return outs, eng._workspace(120, 13, 13)

    outs, ws = run()
    assert all(isinstance(ws[k], ops.IlvPair) for k in ("xn", "xw", "aow", "ao", "hmid"))
    monkeypatch.setenv("MVP_ILV", "0")
    sep, ws0 = run()
    assert not any(isinstance(ws0[k], ops.IlvPair) for k in ("xn", "xw", "aow", "ao", "hmid"))
    assert all(bool(torch.isfinite(a).all()) and torch.equal(a, b) for a, b in zip(outs, sep))
