"""GPU checks of the MaskCut evaluation with the dense-CRF refinement (mvp/maskcut.py, refine="dense_crf"; mvp/densecrf.py;
evals/models/crf.py) against the fp64 oracle of tests/densecrf_ref.py.

The oracle chain is fed the device's own per-pass CRF inputs (the pass loop itself is what tests/test_gpu_maskcut.py holds to its
oracle), so what is compared is the refinement: CRF, hole filling, IoU rule, union.  A pixel may differ only where the oracle's
|Q_1 - 0.5| < 1e-3 in one of the image's passes; such pixels may be at most 0.5 % of an image, and the counts against the ground
truth may differ by at most their number."""
import csv
import sys

import numpy as np
import pytest
import torch

import densecrf_ref as ref
from conftest import PKG
from test_gpu_maskcut import _vit

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _batch():
    from evals.datasets.synthetic import SyntheticVOC

    ds = SyntheticVOC("test", num_samples=8, fixed_size=64, seed=2)
    items = [ds[i] for i in range(8)]
    images = torch.stack([it["original_image"] for it in items]).to(DEV)
    rgb = torch.stack([it["original_image_rgb"] for it in items]).to(DEV)
    gt = torch.stack([it["gt_binary_mask"] for it in items]).to(DEV)
    return ds, items, images, rgb, gt, [int(it["num_objects"]) for it in items]


def test_processor_with_refinement_against_the_oracle_chain():
    from evals.models.maskcut_processor import MaskCutProcessor
    from mvp import maskcut
    from mvp.maskcut import metrics_from_counts

    ds, items, images, rgb, gt, nobj = _batch()
    proc = MaskCutProcessor(backbone=_vit(64), patch_size=16, tau=0.15, fixed_size=64, refine="dense_crf")
    union, inputs, active, n_fallback = proc.refined_union(images, nobj, rgb)
    union, inputs, active = union.cpu().numpy().astype(bool), inputs.cpu().numpy(), active.cpu().numpy()
    rgb_u8 = maskcut.quantise_rgb(images, rgb).permute(0, 2, 3, 1).cpu().numpy()
    assert np.array_equal(rgb_u8, np.round(255.0 * rgb.permute(0, 2, 3, 1).cpu().numpy().astype(np.float64)).astype(np.uint8))
    assert np.array_equal(maskcut.quantise_rgb(images, None).permute(0, 2, 3, 1).cpu().numpy(), rgb_u8)  # the normalisation undone
    rows, nf = proc.process_batch(images, gt, nobj, rgb)
    assert nf == n_fallback
    for b in range(8):
        assert active[b].tolist() == [1 if p < nobj[b] else 0 for p in range(active.shape[1])]
        ins = [inputs[b, p] for p in range(nobj[b])]
        for p in range(1, nobj[b]):  # the inputs are disjoint: each pass minus the earlier ones
            assert not (ins[p] & np.maximum.reduce(ins[:p])).any()
        want, passes = ref.refine_chain(rgb_u8[b], ins)
        excluded = np.zeros((64, 64), dtype=bool)
        for q1, _, _ in passes:
            excluded |= np.abs(q1 - 0.5) < 1e-3
        n_ex = int(excluded.sum())
        assert n_ex <= 0.005 * 64 * 64, (b, n_ex)
        g = items[b]["gt_binary_mask"][0].numpy()
        m_want = ref_counts(want, g)
        got_counts = ref_counts(union[b], g)
        assert np.array_equal(union[b][~excluded], want[~excluded]), b
        assert max(abs(x - y) for x, y in zip(got_counts, m_want)) <= n_ex, (b, got_counts, m_want)
        m = metrics_from_counts(*got_counts)  # the metrics come from the counts
        for k in maskcut.METRICS:
            assert abs(rows[b][k] - m[k]) <= 1e-12, (b, k)
        print(f"image {b}: objects {nobj[b]}, kept {[bool(k) for _, _, k in passes]}, excluded {n_ex}, union {int(want.sum())} px, "
              f"grid input {int(np.maximum.reduce(ins).sum())} px, IoU with gt {rows[b]['IoU']:.3f}")
    print(f"n_fallback {n_fallback}")
    avg, nf2, n = maskcut.predict(proc, ds, batch_size=5, device=torch.device(DEV))
    assert n == 8 and nf2 == n_fallback
    for k in avg:
        assert abs(avg[k] - np.mean([r[k] for r in rows])) <= 1e-9


def ref_counts(pred, gt):
    p, g = np.asarray(pred) != 0, np.asarray(gt) != 0
    return int((p & g).sum()), int((p & ~g).sum()), int((~p & g).sum()), int((~p & ~g).sum())


def test_refine_none_is_unchanged_bit_for_bit():
    from evals.models.maskcut_processor import MaskCutProcessor

    _, _, images, rgb, gt, nobj = _batch()
    model = _vit(64)
    plain = MaskCutProcessor(backbone=model, patch_size=16, tau=0.15, fixed_size=64)
    keyword = MaskCutProcessor(backbone=model, patch_size=16, tau=0.15, fixed_size=64, refine="none")
    rows_a, nf_a = plain.process_batch(images, gt, nobj)
    rows_b, nf_b = keyword.process_batch(images, gt, nobj, rgb)
    assert rows_a == rows_b and nf_a == nf_b
    for k in ("union", "painted", "mask", "v", "lam"):
        a, b = getattr(plain._buf, k), getattr(keyword._buf, k)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), k


def test_refinement_refuses_a_gt_of_another_size():
    from evals.models.maskcut_processor import MaskCutProcessor

    _, _, images, rgb, gt, nobj = _batch()
    proc = MaskCutProcessor(backbone=_vit(64), patch_size=16, tau=0.15, fixed_size=64, refine="dense_crf")
    with pytest.raises(ValueError, match="image's size"):
        proc.process_batch(images, gt[..., :32, :32].contiguous(), nobj, rgb)


def test_densecrf_entry_with_the_bilinear_logit_resize():
    from evals.models import crf

    H, W = 40, 56
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:H, 0:W]
    inside = ((yy - 18) / 11.0) ** 2 + ((xx - 30) / 16.0) ** 2 <= 1.0
    image = np.round(255.0 * (rng.uniform(0.0, 0.5, size=(H, W, 3)) + 0.5 * inside[..., None])).astype(np.uint8)
    mask = (inside.reshape(5, 8, 7, 8).mean(axis=(1, 3)) > 0.3).astype(np.float64)  # 5 x 7 cells
    got = crf.densecrf(image, mask)
    assert got.shape == (H, W) and got.dtype == np.float32 and set(np.unique(got)) <= {0.0, 1.0}
    want, q1 = ref.densecrf(image, mask)
    excluded = np.abs(q1 - 0.5) < 1e-3
    print(f"densecrf 40x56 from 5x7: excluded {int(excluded.sum())}, MAP pixels {int(want.sum())}, changed by the CRF "
          f"{float((want != (ref.resize_plane(mask, H, W) > 0.5)).mean()):.3f}")
    assert excluded.mean() <= 0.005
    assert np.array_equal(got[~excluded] > 0.5, want[~excluded])
    same = crf.densecrf(image, inside.astype(np.float64))  # equal sizes: no resize
    want_same, q_same = ref.densecrf(image, inside.astype(np.float64))
    ex = np.abs(q_same - 0.5) < 1e-3
    assert ex.mean() <= 0.005 and np.array_equal(same[~ex] > 0.5, want_same[~ex])


def test_entry_script_with_refinement_writes_the_csv_row(tmp_path, monkeypatch, capsys):
    from oracle import vit as ovit

    torch.save(ovit.make_vit_weights(embed_dim=128, depth=4, seed=1), tmp_path / "dino_vitb16.pth")
    monkeypatch.setenv("MVP_CKPT_DIR", str(tmp_path))
    monkeypatch.syspath_prepend(PKG)
    sys.modules.pop("evaluate_generic_objectness", None)
    import evaluate_generic_objectness as script

    args = ["backbone=dino_b16", "backbone.return_kqv=true", "backbone.fixed_size=64", "dataset=synthetic_voc", "dataset.num_samples=4",
            "dataset.fixed_size=64", "batch_size=4", "experiment_model=dino_b16", f"output_dir={tmp_path}/out"]
    plain_train, plain_test, _ = script.main(args)
    train_avg, test_avg, n_fallback = script.main(args + ["+refine=dense_crf"])
    text = capsys.readouterr().out
    assert text.count("Final test average metrics") == 2
    rows = list(csv.reader(open(tmp_path / "out" / "final_results_summary.csv")))
    assert len(rows) == 3 and len(rows[2]) == 10 and rows[0][9] == "n_fallback"  # the columns are unchanged
    keys = ("F-measure", "IoU", "Accuracy", "CorLoc")
    assert [float(x) for x in rows[2][1:9]] == [train_avg[k] for k in keys] + [test_avg[k] for k in keys]
    assert int(rows[2][9]) == n_fallback
    assert [train_avg[k] for k in keys] != [plain_train[k] for k in keys]  # pixel-level masks are not the 16-pixel blocks
