"""The MaskCut evaluation end to end on the GPU (mvp/maskcut.py, evals/models/maskcut_processor.py, evaluate_generic_objectness.py)
against the fp64 oracle of tests/maskcut_ref.py fed the same features.

The pass loop on the fixtures of tests/test_gpu_maskcut_kernels.py: every pass mask, the painting and the union are the oracle's,
exactly; no fixture but 8x8 may need the host solve (``n_fallback == 0``: this is what fails if the device solver is replaced by the
fallback), and on 8x8 (lambda_2 ~ lambda_3) the masks are the oracle's whether the device converged or not, with n_fallback = the
number of clear ``converged`` bytes.

The processor on SyntheticVOC(8, fixed_size=64) with a seeded tiny ViT (return_kqv=True): masks against the oracle run on the very
keys ``model(images)`` returned.  An image is excused when the oracle itself has an affinity entry within 2 AFF_TOL of tau or a
cell within 4 (R_TOL / gap) max |v| of the mean in one of its passes (at most one of the eight); the four averaged metrics then
agree to 1e-6.  The evaluation loop is a plain loop over batches (mvp/maskcut.py says why), so there is no two-rank run."""
import csv
import sys

import numpy as np
import pytest
import torch

import maskcut_ref as ref
from conftest import PKG
from test_gpu_maskcut_kernels import AFF_TOL, NAMES, oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("name", NAMES)
def test_pass_loop_on_the_fixtures(name):
    """Batch of two: the fixture with all its passes, and the same features with one pass only (idle in the later passes)."""
    from mvp import maskcut

    f, h, w, P, out = oracle(name)
    feats = torch.from_numpy(np.stack([f, f])).to(DEV)
    nobj = [P, 1]
    buf, conv, active, kept = maskcut.maskcut_batch(feats, h, w, nobj, keep_passes=True)
    conv_host = conv.cpu()
    clear = int(sum(1 for p in range(P) for b in range(2) if p < nobj[b] and not int(conv_host[p, b])))
    iters = [[int(k["iters"][b]) for b in range(2) if p < nobj[b]] for p, k in enumerate(kept)]
    n_fallback = maskcut.finish_fallbacks(feats, h, w, nobj, buf, conv_host)
    print(f"{name}: rounds per pass {iters}  clear converged bytes {clear}  n_fallback {n_fallback}")
    if name != "8x8":
        assert clear == 0 and n_fallback == 0
        for p, ps in enumerate(out["passes"]):
            assert np.array_equal(kept[p]["mask"][0].cpu().numpy().reshape(h, w).astype(bool), ps["mask"]), p
            assert np.array_equal(kept[p]["painted"][0].cpu().numpy().reshape(h, w).astype(bool), ps["painted"]), p
            if ref.seed_margin(ps["v"], ps["reverse"]) > 8 * maskcut.R_TOL / ps["gap"]:  # twice the bipartition's margin rule
                assert int(kept[p]["seed"][0]) == ps["seed"]
    else:
        assert n_fallback == clear  # one host solve per clear byte
    union = buf.union.cpu().numpy().reshape(2, h, w).astype(bool)
    assert np.array_equal(union[0], out["union"])
    assert np.array_equal(union[1], out["passes"][0]["union"])
    assert np.array_equal(buf.painted.cpu().numpy().reshape(2, h, w)[1].astype(bool), out["passes"][0]["painted"])


def test_host_eigenvector_is_the_oracles():
    from mvp import maskcut

    f, h, w, P, out = oracle("8x8")
    ps = out["passes"][0]
    bits = torch.from_numpy(ref.pack_bits(ps["B"]).view(np.int32)).to(DEV)
    v = maskcut.host_eigenvector(bits, torch.from_numpy(ps["d"]).to(DEV), h * w).numpy()
    assert np.abs(v - ps["v"]).max() <= 1e-6 * np.abs(ps["v"]).max()


def _vit(fixed_size):
    """The tiny seeded ViT of the other tests, with init scale 0.1 instead of 0.02: at 0.02 the keys of a random-init ViT on these
    images fall into two tight clusters, the thresholded graph is disconnected (lambda_2 ~ 1e-5) and the oracle's own painted cells
    then sit within the margin of the mean on every image with two or more passes (5 to 8 of 8 images excused over 30 dataset seeds,
    run on the CPU oracle).  Seeds 4 (weights) and 2 (dataset) were found the same way: one image of eight is excused."""
    from evals.models.dino import DINO
    from oracle import vit as ovit

    sd = ovit.make_vit_weights(embed_dim=128, depth=4, seed=4, std=0.1)
    return DINO(weights=sd, return_kqv=True, fixed_size=fixed_size).to(DEV).eval()


def _excused(passes):
    from mvp import maskcut

    for ps in passes:
        if (np.abs(ps["A"] - ps["tau"]) <= 2 * AFF_TOL).any():
            return True
        v = ps["v"]
        if (np.abs(v - v.mean()) <= 4 * (maskcut.R_TOL / max(ps["gap"], 1e-300)) * np.abs(v).max()).any():
            return True
    return False


def test_processor_on_synthetic_voc_against_the_oracle():
    from evals.datasets.synthetic import SyntheticVOC
    from evals.models.maskcut_processor import MaskCutProcessor
    from mvp import maskcut

    ds = SyntheticVOC("test", num_samples=8, fixed_size=64, seed=2)
    model = _vit(64)
    proc = MaskCutProcessor(backbone=model, patch_size=16, tau=0.15, fixed_size=64)
    items = [ds[i] for i in range(8)]
    images = torch.stack([it["original_image"] for it in items]).to(DEV)
    gt = torch.stack([it["gt_binary_mask"] for it in items]).to(DEV)
    nobj = [int(it["num_objects"]) for it in items]
    with torch.no_grad():
        feats = model(images).float().cpu().numpy()
    h = w = 4
    assert feats.shape[0] == 8 and feats.shape[2] == h * w
    rows, n_fallback = proc.process_batch(images, gt, nobj)
    union = proc._buf.union.cpu().numpy().reshape(8, h, w).astype(bool)
    want, skipped = [], []
    for b in range(8):
        out = ref.maskcut(feats[b], h, w, nobj[b])
        g = items[b]["gt_binary_mask"][0].numpy()
        m = ref.metrics_from_counts(*ref.counts(ref.upsample_nearest(out["union"], *g.shape), g))
        if _excused(out["passes"]):
            skipped.append((b, bool(np.array_equal(union[b], out["union"]))))  # (whether it agreed all the same is printed, not asserted)
            continue
        assert np.array_equal(union[b], out["union"]), b
        for k in m:
            assert abs(rows[b][k] - m[k]) <= 1e-6, (b, k)
        want.append((rows[b], m))
    print(f"skipped {skipped}  n_fallback {n_fallback}  objects {nobj}")
    assert len(skipped) <= 1
    for k in ("F-measure", "IoU", "Accuracy", "CorLoc"):
        assert abs(np.mean([r[k] for r, _ in want]) - np.mean([m[k] for _, m in want])) <= 1e-6
    # predict(): the running average over the same eight images, in two batches
    avg, nf, n = maskcut.predict(proc, ds, batch_size=5, device=torch.device(DEV))
    assert n == 8 and nf == n_fallback
    for k in avg:
        assert abs(avg[k] - np.mean([r[k] for r in rows])) <= 1e-9


def test_entry_script_writes_the_csv_row(tmp_path, monkeypatch, capsys):
    """evaluate_generic_objectness.py in-process on the synthetic config, the tiny weights found as a local checkpoint."""
    from oracle import vit as ovit

    torch.save(ovit.make_vit_weights(embed_dim=128, depth=4, seed=1), tmp_path / "dino_vitb16.pth")
    monkeypatch.setenv("MVP_CKPT_DIR", str(tmp_path))
    monkeypatch.syspath_prepend(PKG)
    sys.modules.pop("evaluate_generic_objectness", None)
    import evaluate_generic_objectness as script

    args = ["backbone=dino_b16", "backbone.return_kqv=true", "backbone.fixed_size=64", "dataset=synthetic_voc", "dataset.num_samples=4",
            "dataset.fixed_size=64", "batch_size=4", "experiment_model=dino_b16", f"output_dir={tmp_path}/out"]
    train_avg, test_avg, n_fallback = script.main(args)
    text = capsys.readouterr().out
    assert "Final training average metrics" in text and "Final test average metrics" in text
    rows = list(csv.reader(open(tmp_path / "out" / "final_results_summary.csv")))
    assert rows[0] == ["Model Name", "Train Avg F-measure", "Train Avg IoU", "Train Avg Accuracy", "Train Avg CorLoc", "Test Avg F-measure",
                       "Test Avg IoU", "Test Avg Accuracy", "Test Avg CorLoc", "n_fallback"]
    assert len(rows) == 2 and len(rows[1]) == 10 and rows[1][0] == "dino_vitb16"
    keys = ("F-measure", "IoU", "Accuracy", "CorLoc")
    assert [float(x) for x in rows[1][1:9]] == [train_avg[k] for k in keys] + [test_avg[k] for k in keys]
    assert int(rows[1][9]) == n_fallback
    script.main(args)
    assert len(list(csv.reader(open(tmp_path / "out" / "final_results_summary.csv")))) == 3  # appended, header once
