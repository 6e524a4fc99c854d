"""Validation of the trained objectness probe (reference: train_generic_objectness.py:417-492 ``validation`` and its metric helpers
:56-183): F-measure (beta^2 = 0.09), IoU, pixel accuracy and CorLoc of the prediction thresholded at 0.5.

The reference copies every thresholded prediction to the host and counts with numpy; here one kernel (``mvp_binary_counts``) leaves
TP / FP / FN / TN on the device and four integers per batch cross to the host.  Its quirks are kept: the metrics are taken over the
whole batch tensor at once (CorLoc therefore casts one vote per batch), batches weigh equally whatever their size, and the probe stays
in whatever mode the caller left it in — the reference never calls ``probe.eval()``, so its validation normalises with batch
statistics and keeps moving the running ones."""
from __future__ import annotations

from typing import Dict

import torch

from . import functional as MF
from . import ops

METRICS = ("F-measure", "IoU", "Accuracy", "CorLoc")
CSV_TITLES = ["Model Name", "Test Avg F-measure", "Test Avg IoU", "Test Avg Accuracy", "Test Avg CorLoc"]


def metrics_from_counts(tp: int, fp: int, fn: int, tn: int, beta: float = 0.3, threshold: float = 0.5) -> Dict[str, float]:
    """The reference's formulas on the four counts (compute_precision_recall / _f_measure / _iou / _accuracy / _corloc)."""
    tp, fp, fn, tn = int(tp), int(fp), int(fn), int(tn)
    precision = tp / (tp + fp + 1e-6)
    recall = tp / (tp + fn + 1e-6)
    beta_sq = beta**2
    f_measure = (1 + beta_sq) * (precision * recall) / (beta_sq * precision + recall + 1e-6)
    iou = tp / (tp + fp + fn + 1e-6)
    accuracy = (tp + tn) / (tp + fp + fn + tn)
    return {"Precision": precision, "Recall": recall, "F-measure": f_measure, "IoU": iou, "Accuracy": accuracy,
            "CorLoc": 1 if iou >= threshold else 0}


def binary_counts(pred: torch.Tensor, gt: torch.Tensor, per_image: bool = False, threshold: float = 0.5) -> torch.Tensor:
    """int64 [G, 4] = TP, FP, FN, TN of ``pred > threshold`` against the 0 / 1 mask ``gt`` (same shape), on the device.
    G = 1: the whole tensor at once (the reference's form); ``per_image``: one row per batch entry."""
    if tuple(pred.shape) != tuple(gt.shape):
        raise ValueError(f"binary_counts: prediction {tuple(pred.shape)} and mask {tuple(gt.shape)} differ")
    MF._need_cuda(pred, "binary_counts")
    p, g = pred.detach().contiguous().float(), gt.detach().contiguous().float()
    G = p.shape[0] if per_image else 1
    out = torch.empty(G, 4, dtype=torch.int64, device=p.device)
    ops.binary_counts(p, g, out, G, p.numel() // G, threshold)
    return out


def predict(probe, feats, size) -> torch.Tensor:
    """train_generic_objectness.py:440-443: probe, then bilinear resize to the mask."""
    with torch.no_grad():
        return MF.interpolate(probe(feats), size=tuple(size), mode="bilinear")


def validation(model, probe, loader) -> Dict[str, float]:
    """-> {"F-measure", "IoU", "Accuracy", "CorLoc"}: the running average over the loader's batches, each batch with weight one."""
    from .pipeline import pipelined_features
    from .train import _device_batches

    dev = torch.device("cuda", torch.cuda.current_device())
    avg = {k: 0.0 for k in METRICS}
    n = 0
    batches = _device_batches(loader, dev, keys=("original_image", "gt_binary_mask"))
    for batch, feats in pipelined_features(model, batches, image_key="original_image", probe=probe):
        gt = batch["gt_binary_mask"].to(dev, non_blocking=True).float()
        pred = predict(probe, feats, gt.shape[-2:])
        tp, fp, fn, tn = binary_counts(pred, gt)[0].tolist()  # the one device-to-host copy of this batch
        m = metrics_from_counts(tp, fp, fn, tn)
        n += 1
        for k in avg:
            avg[k] = (avg[k] * (n - 1) + m[k]) / n
    if n == 0:
        raise ValueError("validation(): empty loader")
    return avg


def append_summary_csv(output_dir: str, model_name: str, avg: Dict[str, float], dataset_name: str = "voc") -> str:
    """train_generic_objectness.py:608-640: <output_dir>/trained_objectness/final_results_summary_voc[12].csv, header once."""
    import csv
    import os

    path = os.path.join(output_dir, "trained_objectness", "final_results_summary_voc.csv" if dataset_name == "voc" else "final_results_summary_voc12.csv")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    if not os.path.exists(path):
        with open(path, mode="w", newline="") as f:
            csv.writer(f).writerow(CSV_TITLES)
    with open(path, mode="a", newline="") as f:
        csv.writer(f).writerow([model_name] + [avg[k] for k in METRICS])
    return path
