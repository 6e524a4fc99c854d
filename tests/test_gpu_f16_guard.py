"""The f16x2 range guard on the device: ViTEngine's audited forward (RangeAudit: which sites, what they count, that the taps do not
change), the five site kinds tripped by name and compared with the MVP_CHECK_F16_RANGE diagnostic, the other engine forms (SwiGLU, RoPE,
BEiT's replay pass), the wrapper policy (fallback / raise / warn / default, a checkpoint file under MVP_CKPT_DIR) and FeaturePipeline
with graphs on.  Engines are C = 128, depth 4, 2 heads; images 2 x 3 x 64 x 96 (4 x 6 patches + CLS = 25 tokens)."""
import re
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

C, DEPTH, HEADS = 128, 4, 2
KINDS = ["LayerNorm 1 output", "Q / K", "attention output", "LayerNorm 2 output", "GELU(fc1) output"]
GUARD_WARNING = "f16x2 range guard"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def images(dev):
    return torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(11)).to(dev)


def _sd(seed=5):
    from mvp import backbone as bb

    return bb.random_vit_state_dict(embed_dim=C, depth=DEPTH, patch=16, img=64, seed=seed)


def _plant(kind):
    """The clean weights with ONE value that drives one operand of block 1 beyond fp16's range."""
    sd = _sd()
    if kind == "LayerNorm 1 output":
        sd["blocks.1.norm1.weight"][5] = 3.0e7  # gain of one channel
    elif kind == "Q / K":
        sd["blocks.1.attn.qkv.bias"][C + 9] = 1.0e6  # a K column
    elif kind == "attention output":
        sd["blocks.1.attn.qkv.bias"][2 * C + 9] = 1.0e6  # a V column: V itself is an fp16 + bf16 pair and holds it; P.V = 1e6 does not fit
    elif kind == "LayerNorm 2 output":
        sd["blocks.1.norm2.weight"][3] = 3.0e7
    elif kind == "GELU(fc1) output":
        sd["blocks.1.mlp.fc1.bias"][7] = 1.0e6
    else:
        raise KeyError(kind)
    return sd


def _audited(eng, images, layers=(DEPTH - 1,), **kw):
    from mvp.vit import RangeAudit

    audit = RangeAudit(eng)
    taps = eng.forward_taps(images, list(layers), bn_mode=2, audit=audit, **kw)
    return taps, audit.read()


def _count_scans(monkeypatch):
    from mvp import ops

    calls = []
    real = ops.f16_range_scan
    monkeypatch.setattr(ops, "f16_range_scan", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def test_audit_changes_nothing_and_counts_every_site(dev, images):
    from mvp.vit import RangeAudit, ViTEngine, tripped_sites

    eng = ViTEngine(_sd(), heads=HEADS, precision="f16x2", device=dev)
    assert eng.f16x2 and eng.att_qk_f16
    plain = [t.clone() for t in eng.forward_taps(images, [0, 1, 2, 3], bn_mode=2)]
    taps, report = _audited(eng, images, layers=(0, 1, 2, 3))
    torch.cuda.synchronize()
    assert len(plain) == len(taps) == 4 and all(torch.equal(a, b) for a, b in zip(plain, taps))
    M = 2 * 25
    assert [r["site"] for r in report] == [f"block {i}: {k}" for i in range(DEPTH) for k in KINDS] == RangeAudit(eng).sites
    assert [r["block"] for r in report] == [i for i in range(DEPTH) for _ in KINDS]
    for r in report:
        kind = r["site"].split(": ")[1]
        assert r["n_scanned"] == M * {"Q / K": 2 * C, "GELU(fc1) output": 4 * C}.get(kind, C), r
        assert r["n_sat"] == 0 and r["n_nonfinite"] == 0 and 0.0 < r["max_abs"] < 65504.0, r
    assert tripped_sites(report) == []
    # a forward that stops early leaves the later blocks' sites untouched
    _, short = _audited(eng, images, layers=(1,))
    assert [r["n_scanned"] > 0 for r in short] == [True] * 10 + [False] * 10
    # last_block_qkv: blocks 0 .. depth-2 whole, of the last block LayerNorm 1's output alone
    audit = RangeAudit(eng)
    eng.last_block_qkv(images, audit=audit)
    assert [r["n_scanned"] > 0 for r in audit.read()] == [True] * 16 + [False] * 4


def test_engine_without_fp16_operands_has_no_sites(dev, images):
    from mvp.vit import RangeAudit, ViTEngine

    eng = ViTEngine(_sd(), heads=HEADS, precision="bf16x3", device=dev)
    audit = RangeAudit(eng)
    if eng.att_qk_f16:  # (MVP_ATT_QK=f16 in the environment: Q / K is then an fp16-form operand of a bf16x3 engine too)
        assert audit.sites == [f"block {i}: Q / K" for i in range(DEPTH)]
        return
    assert audit.sites == [] and audit.record.shape == (0, 4)
    a = eng.forward_taps(images, [3], bn_mode=2)[0].clone()
    b = eng.forward_taps(images, [3], bn_mode=2, audit=audit)[0]
    assert torch.equal(a, b) and audit.read() == []


@pytest.mark.parametrize("kind", KINDS)
def test_each_site_kind_is_tripped_by_name(dev, images, kind):
    """No environment variable: the audit's first tripped site is the one the MVP_CHECK_F16_RANGE diagnostic names, and block 0 is clean."""
    from mvp import lib
    from mvp.vit import ViTEngine, tripped_sites

    eng = ViTEngine(_plant(kind), heads=HEADS, precision="f16x2", device=dev)
    assert not eng.check_f16_range
    _, report = _audited(eng, images)
    bad = tripped_sites(report)
    assert bad and bad[0]["site"] == f"block 1: {kind}", [b["site"] for b in bad]
    assert all(r["n_sat"] + r["n_nonfinite"] == 0 for r in report if r["block"] < 1)
    eng.check_f16_range = True
    with pytest.raises(lib.MvpError) as e:
        eng.forward_taps(images, [DEPTH - 1], bn_mode=2)
    eng.check_f16_range = False
    named = re.match(r"f16x2: (.*) holds values beyond", str(e.value)).group(1)
    assert named == bad[0]["site"]


def test_swiglu_engine(dev, images):
    from mvp import backbone as bb
    from mvp.vit import ViTEngine, tripped_sites

    sd = bb.dinov2_hub_to_engine(bb.random_dinov2_state_dict(C, DEPTH, 0, seed=8, ffn="swiglu"))
    H = bb.swiglu_hidden(C)
    eng = ViTEngine(sd, heads=HEADS, patch=14, precision="f16x2", device=dev)
    plain = eng.forward_taps(images, [3], bn_mode=2)[0].clone()
    taps, report = _audited(eng, images)
    assert torch.equal(plain, taps[0]) and tripped_sites(report) == []
    M = 2 * (1 + 5 * 7)  # 64 x 96 centre-padded to 70 x 98
    site = "SwiGLU gate output silu(x1) * x2"
    assert [r["site"] for r in report if r["block"] == 2][-1] == f"block 2: {site}"
    assert all(r["n_scanned"] == M * eng.hidden for r in report if r["site"].endswith(site)) and eng.hidden == 384 and H == 344
    sd["blocks.2.mlp.w12.bias"][5], sd["blocks.2.mlp.w12.bias"][H + 5] = 1.0e3, 1.0e3  # silu(1e3) * 1e3 = 1e6
    bad = tripped_sites(_audited(ViTEngine(sd, heads=HEADS, patch=14, precision="f16x2", device=dev), images)[1])
    assert bad[0]["site"] == f"block 2: {site}"


def test_rope_engine_q_k(dev, images):
    """CroCo v2's form: Q / K are written by mvp_rope2d_qkv, not by the GEMM's epilogue."""
    from mvp import backbone as bb
    from mvp.vit import ViTEngine, tripped_sites

    sd = bb.croco_to_engine(bb.random_croco_state_dict(C, DEPTH, 16, (64, 96), pos_embed="RoPE100", seed=2))
    eng = ViTEngine(sd, heads=HEADS, precision="f16x2", device=dev, rope_freq=100.0)
    plain = eng.forward_taps(images, [3], bn_mode=2)[0].clone()
    taps, report = _audited(eng, images)
    assert torch.equal(plain, taps[0]) and tripped_sites(report) == []
    assert all(r["n_scanned"] == 2 * 24 * 2 * C for r in report if r["site"].endswith("Q / K"))
    sd["blocks.1.attn.qkv.bias"][C + 9] = 1.0e6
    bad = tripped_sites(_audited(ViTEngine(sd, heads=HEADS, precision="f16x2", device=dev, rope_freq=100.0), images)[1])
    assert bad[0]["site"] == "block 1: Q / K"


def test_sam_engine_windowed_and_global_blocks(dev, images):
    """SAM's form: LayerNorm 1's output is read in window order (zero pad rows included) by the qkv GEMM of a windowed block, and Q / K
    are written by mvp_relpos_terms.  4 x 6 grid, window 3: 2 x 2 windows of 9 rows per image; blocks 1 and 3 attend globally."""
    from mvp import backbone as bb
    from mvp.vit import ViTEngine, tripped_sites

    sd = bb.random_sam_state_dict(C, DEPTH, native_grid=8, window=3, global_idx=(1, 3), seed=6)

    def engine(sd):
        return ViTEngine(sd, heads=HEADS, precision="f16x2", device=dev, pos_embed_mode="sam")

    eng = engine(sd)
    plain = eng.forward_taps(images, [3], bn_mode=2)[0].clone()
    taps, report = _audited(eng, images)
    assert torch.equal(plain, taps[0]) and tripped_sites(report) == []
    M, Mp = 2 * 24, 2 * 4 * 9
    for r in report:
        kind = r["site"].split(": ")[1]
        rows = Mp if (r["block"] in (0, 2) and kind in ("LayerNorm 1 output", "Q / K")) else M
        assert r["n_scanned"] == rows * {"Q / K": 2 * C, "GELU(fc1) output": 4 * C}.get(kind, C), r
    sd["blocks.2.attn.qkv.bias"][C + 9] = 1.0e6
    bad = tripped_sites(_audited(engine(sd), images)[1])
    assert bad[0]["site"] == "block 2: Q / K"


def test_replay_after_norm_doubles_the_count(dev, images):
    from mvp import backbone as bb
    from mvp.vit import ViTEngine, tripped_sites

    sd = bb.random_beit_state_dict(C, DEPTH, 16, (64, 96), seed=3)
    eng = ViTEngine(sd, heads=HEADS, precision="f16x2", device=dev, rel_pos_grid=(4, 6))
    _, once = _audited(eng, images)
    plain = eng.forward_taps(images, [3], bn_mode=2, replay_after_norm=True)[0].clone()
    taps, twice = _audited(eng, images, replay_after_norm=True)
    assert torch.equal(plain, taps[0]) and tripped_sites(twice) == []
    assert [r["n_scanned"] for r in twice] == [2 * r["n_scanned"] for r in once] and all(r["n_scanned"] > 0 for r in once)


# ---------------------------------------------------------------- the wrapper's policy
def _dino(dev, sd, **kw):
    from evals.models.dino import DINO

    return DINO(return_multilayer=True, weights=sd, **kw).to(dev).eval()


def _guard_warnings(rec):
    return [w for w in rec if GUARD_WARNING in str(w.message)]


def test_wrapper_fallback(dev, images, monkeypatch):
    from mvp import lib
    from mvp.vit import tripped_sites

    monkeypatch.delenv("MVP_F16_GUARD", raising=False)
    sd = _plant("GELU(fc1) output")
    ref = [t.clone() for t in _dino(dev, sd, precision="bf16x3")(images)]
    m = _dino(dev, sd, precision="f16x2", range_guard="fallback")
    assert m._precision == lib.PREC_F16X2 and m.f16_range_report() is None
    calls = _count_scans(monkeypatch)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = m(images)
    ws = _guard_warnings(rec)
    assert len(ws) == 1 and "block 1: GELU(fc1) output" in str(ws[0].message) and "falling back to precision='bf16x3'" in str(ws[0].message)
    assert m._precision == lib.PREC_BF16X3 and not m.engine().f16x2
    assert len(out) == len(ref) == 4 and all(torch.equal(a, b) for a, b in zip(out, ref))
    n_audit = len(calls)
    assert n_audit == 5 * DEPTH
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        again = m(images)
    assert len(calls) == n_audit and not _guard_warnings(rec)  # resolved: no second audit, no second warning
    assert all(torch.equal(a, b) for a, b in zip(again, ref))
    report = m.f16_range_report()
    assert len(report) == 5 * DEPTH and tripped_sites(report)[0]["site"] == "block 1: GELU(fc1) output"


def test_wrapper_raise_and_warn(dev, images, monkeypatch):
    from mvp import lib

    monkeypatch.delenv("MVP_F16_GUARD", raising=False)
    sd = _plant("LayerNorm 2 output")
    with pytest.raises(lib.MvpError, match=r"block 1: LayerNorm 2 output.*precision='bf16x3'"):
        _dino(dev, sd, precision="f16x2", range_guard="raise")(images)
    unguarded = [t.clone() for t in _dino(dev, sd, precision="f16x2", range_guard="off")(images)]
    m = _dino(dev, sd, precision="f16x2", range_guard="warn")
    with pytest.warns(UserWarning, match="block 1: LayerNorm 2 output"):
        out = m(images)
    assert m._precision == lib.PREC_F16X2 and all(torch.equal(a, b) for a, b in zip(out, unguarded))
    # the environment variable arms a model built without the keyword
    monkeypatch.setenv("MVP_F16_GUARD", "raise")
    with pytest.raises(lib.MvpError, match=GUARD_WARNING):
        _dino(dev, sd, precision="f16x2")(images)


def test_wrapper_default_with_weights_runs_no_audit(dev, images, monkeypatch):
    monkeypatch.delenv("MVP_F16_GUARD", raising=False)
    sd = _plant("GELU(fc1) output")
    off = [t.clone() for t in _dino(dev, sd, precision="f16x2", range_guard="off")(images)]
    calls = _count_scans(monkeypatch)
    m = _dino(dev, sd, precision="f16x2")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = m(images)
    assert not calls and not _guard_warnings(rec) and m.f16_range_report() is None and m.range_guard_action() == "off"
    assert all(torch.equal(a, b) for a, b in zip(out, off))


def test_checkpoint_file_arms_auto(dev, images, monkeypatch, tmp_path):
    """The DINO wrapper's loader takes the C = 128, depth 4 file as it takes the published one: the default ('auto') falls back."""
    from evals.models.dino import DINO
    from mvp import lib

    monkeypatch.delenv("MVP_F16_GUARD", raising=False)
    monkeypatch.delenv("MVP_PRECISION", raising=False)
    sd = _plant("attention output")
    torch.save(sd, tmp_path / "dino_vitb16.pth")
    monkeypatch.setenv("MVP_CKPT_DIR", str(tmp_path))
    m = DINO(return_multilayer=True).to(dev).eval()
    assert m.weights_from_file and m._precision == lib.PREC_F16X2 and m.range_guard_action() == "fallback"
    with pytest.warns(UserWarning, match="block 1: attention output"):
        out = m(images)
    assert m._precision == lib.PREC_BF16X3
    ref = _dino(dev, sd, precision="bf16x3")(images)
    assert all(torch.equal(a, b) for a, b in zip(out, ref))
    # clean weights from a file: audited once, nothing tripped, f16x2 kept
    torch.save(_sd(), tmp_path / "dino_vitb16.pth")
    clean = DINO(return_multilayer=True).to(dev).eval()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        clean(images)
    assert not _guard_warnings(rec) and clean._precision == lib.PREC_F16X2 and len(clean.f16_range_report()) == 5 * DEPTH


# ---------------------------------------------------------------- the pipeline, graphs on
def _batches(dev, n=4):
    return [{"image": torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(300 + s)).to(dev)} for s in range(n)]


def _pipelined(model, bs):
    from mvp.pipeline import FeaturePipeline, pipelined_features

    pipe = FeaturePipeline(model, 2, graphs=True, group=1)
    assert pipe.graphs
    got = [[t.clone() for t in f] for _, f in pipelined_features(model, bs, pipe=pipe)]
    torch.cuda.synchronize()
    return got


def test_pipeline_fallback_equals_serial_bf16x3(dev, monkeypatch):
    from mvp import lib
    from mvp.train import extract_features

    monkeypatch.delenv("MVP_F16_GUARD", raising=False)
    sd, bs = _plant("Q / K"), _batches(dev)
    serial = _dino(dev, sd, precision="bf16x3", add_norm=True)
    ref = [[t.clone() for t in extract_features(serial, b["image"])] for b in bs]
    m = _dino(dev, sd, precision="f16x2", add_norm=True, range_guard="fallback")
    with pytest.warns(UserWarning, match="block 1: Q / K"):
        got = _pipelined(m, bs)
    assert m._precision == lib.PREC_BF16X3 and len(got) == len(ref)
    assert all(torch.equal(a, b) for g, r in zip(got, ref) for a, b in zip(g, r))


def test_pipeline_clean_weights_guard_on_equals_guard_off(dev, monkeypatch):
    from mvp import lib

    monkeypatch.delenv("MVP_F16_GUARD", raising=False)
    sd, bs = _sd(), _batches(dev)
    off = _pipelined(_dino(dev, sd, precision="f16x2", add_norm=True, range_guard="off"), bs)
    m = _dino(dev, sd, precision="f16x2", add_norm=True, range_guard="warn")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        on = _pipelined(m, bs)
    assert not _guard_warnings(rec) and m._precision == lib.PREC_F16X2 and len(m.f16_range_report()) == 5 * DEPTH
    assert all(torch.equal(a, b) for g, r in zip(on, off) for a, b in zip(g, r))


def test_pending_guard_under_capture_raises(dev, images, monkeypatch):
    """A pending guard would have to synchronise: met inside a real capture on a side stream (torch.cuda.graph, as the pipeline
    captures) it raises before it launches anything — the capture ends empty — and an eager forward beforehand settles it."""
    from mvp import lib

    monkeypatch.delenv("MVP_F16_GUARD", raising=False)
    m = _dino(dev, _sd(), precision="f16x2", range_guard="warn")
    m.engine()  # (built outside the capture, as the pipeline's first eager forward would have)
    calls = _count_scans(monkeypatch)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with pytest.raises(lib.MvpError, match="pending and the stream is capturing"):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side, capture_error_mode="thread_local"):
            assert torch.cuda.is_current_stream_capturing()
            m(images)
    torch.cuda.synchronize()
    assert not torch.cuda.is_current_stream_capturing()
    assert not calls and m.f16_range_report() is None
    m(images)  # eager: resolved
    assert len(calls) == 5 * DEPTH
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side, capture_error_mode="thread_local"):
        m.resolve_range_guard(images)  # resolved: nothing to do, nothing raised, nothing launched
    torch.cuda.synchronize()
    assert len(calls) == 5 * DEPTH


# ---------------------------------------------------------------- wrappers whose forward prepares the batch for the engine
def _raw_batches(dev, n=3, hw=(64, 96)):
    return [{"image": torch.randn(2, 3, *hw, generator=torch.Generator().manual_seed(500 + s)).to(dev)} for s in range(n)]


def _vit224(plant=None):
    """C = 128, depth 4 with the 14 x 14 + 1 position table of a 224 x 224 model (MoCo-v3 and MAE keep it 'fixed')."""
    from mvp import backbone as bb

    sd = bb.random_vit_state_dict(embed_dim=C, depth=DEPTH, patch=16, img=224, seed=5)
    if plant:
        sd["blocks.1.mlp.fc1.bias"][7] = 1.0e6
    return sd


def test_pipeline_resizing_wrapper_audits_what_the_engine_is_fed(dev, monkeypatch):
    """MoCo-v3 resizes every batch to 224 x 224 inside forward.  The pipeline hands the guard the loader's raw 64 x 96 batch: the audit
    must run on the resized one (197 tokens per image, the rows of the model's fixed position table — at the raw size the table would
    be read past its end), and a fallback must leave the pipelined loop equal to the serial bf16x3 loop bit for bit."""
    from evals.models.mocov3 import MoCoV3
    from mvp import lib
    from mvp.train import extract_features

    monkeypatch.delenv("MVP_F16_GUARD", raising=False)
    bs = _raw_batches(dev)

    def build(sd, **kw):
        return MoCoV3(return_multilayer=True, add_norm=True, weights=sd, **kw).to(dev).eval()

    clean = build(_vit224(), precision="f16x2", range_guard="warn")
    off = _pipelined(build(_vit224(), precision="f16x2", range_guard="off"), bs)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        on = _pipelined(clean, bs)
    assert not _guard_warnings(rec) and all(torch.equal(a, b) for g, r in zip(on, off) for a, b in zip(g, r))
    report = clean.f16_range_report()
    assert len(report) == 5 * DEPTH and report[0]["n_scanned"] == 2 * 197 * C and report[1]["n_scanned"] == 2 * 197 * 2 * C
    serial = build(_vit224(plant=True), precision="bf16x3")
    ref = [[t.clone() for t in extract_features(serial, b["image"])] for b in bs]
    m = build(_vit224(plant=True), precision="f16x2", range_guard="fallback")
    with pytest.warns(UserWarning, match=r"block 1: GELU\(fc1\) output"):
        got = _pipelined(m, bs)
    assert m._precision == lib.PREC_BF16X3 and all(torch.equal(a, b) for g, r in zip(got, ref) for a, b in zip(g, r))


def test_pipeline_beit_guard_runs_at_the_models_grid(dev, monkeypatch):
    """BEiT v2's relative-position bias belongs to ONE grid and its forward resizes to it: raw 80 x 112 batches through a guarded
    pipeline neither raise out of the engine nor change the features, and the replay pass is audited (counts doubled)."""
    from evals.models.beit_v2 import BEiTV2
    from mvp import backbone as bb

    monkeypatch.delenv("MVP_F16_GUARD", raising=False)
    sd, bs = bb.random_beit_state_dict(C, DEPTH, 16, (64, 96), seed=3), _raw_batches(dev, hw=(80, 112))

    def build(guard):
        return BEiTV2(return_multilayer=True, weights=sd, img_size=(64, 96), precision="f16x2", range_guard=guard).to(dev).eval()

    off = _pipelined(build("off"), bs)
    m = build("raise")
    on = _pipelined(m, bs)
    assert all(torch.equal(a, b) for g, r in zip(on, off) for a, b in zip(g, r))
    report = m.f16_range_report()
    assert len(report) == 5 * DEPTH and all(r["n_sat"] + r["n_nonfinite"] == 0 for r in report)
    assert report[0]["n_scanned"] == 2 * (2 * 25 * C)


def test_mae_guard_rebuilds_the_table_before_the_audit(dev, monkeypatch):
    """MAE keeps a fixed sincos table for ONE image size and rebuilds it in forward: the guard given a raw 64 x 96 batch audits the
    engine of the 4 x 6 grid (25 tokens per image), not the 14 x 14 one the wrapper was built with."""
    from evals.models.mae import MAE

    monkeypatch.delenv("MVP_F16_GUARD", raising=False)
    x = _raw_batches(dev, n=1)[0]["image"]
    m = MAE(return_multilayer=True, weights=_vit224(), precision="f16x2", range_guard="warn").to(dev).eval()
    off = MAE(return_multilayer=True, weights=_vit224(), precision="f16x2", range_guard="off").to(dev).eval()
    m.resolve_range_guard(x)
    assert tuple(m.image_size) == (64, 96) and m.vit.pos_embed.shape[1] == 25
    report = m.f16_range_report()
    assert report[0]["n_scanned"] == 2 * 25 * C and not [r for r in report if r["n_sat"] + r["n_nonfinite"]]
    calls = _count_scans(monkeypatch)
    assert all(torch.equal(a, b) for a, b in zip(m(x), off(x))) and not calls  # resolved for this size: no second audit


def test_class_token_shortcuts_are_guarded(dev, images, monkeypatch):
    """The single-tap return_cls paths of iBOT, MoCo-v3 and MAE run forward_tokens, not _extract: the guard stands in front of them too."""
    from evals.models.ibot import iBOT
    from evals.models.mae import MAE
    from evals.models.mocov3 import MoCoV3
    from mvp import lib

    monkeypatch.delenv("MVP_F16_GUARD", raising=False)
    for build in (lambda **kw: iBOT(return_cls=True, weights=_plant("GELU(fc1) output"), **kw),
                  lambda **kw: MoCoV3(return_cls=True, weights=_vit224(plant=True), **kw),
                  lambda **kw: MAE(return_cls=True, weights=_vit224(plant=True), **kw)):
        with pytest.raises(lib.MvpError, match=r"block 1: GELU\(fc1\) output"):
            build(precision="f16x2", range_guard="raise").to(dev)(images)
        m = build(precision="f16x2", range_guard="fallback").to(dev)
        with pytest.warns(UserWarning, match=GUARD_WARNING):
            out = m(images)
        ref = build(precision="bf16x3").to(dev)(images)
        assert m._precision == lib.PREC_BF16X3 and torch.equal(out, ref)
