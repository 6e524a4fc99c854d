"""Restatements for the Taskonomy tests: the masked L1 loss, the per-pixel terms of the two metric forms in torch fp32 (one tensor
operation per rounding, as evals/utils/metrics.py:580-739 of the reference compute them) with fp64 sums, and the probe step in torch
autograd.  tests/golden/make_goldens_taskonomy.py uses ``metric_sums`` for the "fp64-summed value of the fp32 terms" it records."""
import numpy as np
import torch
import torch.nn.functional as F

CURV_T = (1.25, 1.25 * 2, 1.25 * 3)
RESH_T = (1.1, 1.1**2, 1.1**3)
CURV_KEYS = ["AbsRel", "δ1.25_k1", "δ2.5_k1", "δ3.75_k1", "δ1.25_k2", "δ2.5_k2", "δ3.75_k2", "δ1.25_avg", "δ2.5_avg", "δ3.75_avg"]
RESH_KEYS = ["AbsRel"] + [f"δ_{t}" for t in RESH_T]


def masked_l1(pred, target, valid=None):
    """sum valid |pred - target| / (count of valid elements, a one-channel mask counted once per channel), in the inputs' dtype."""
    if valid is None:
        valid = torch.ones_like(pred, dtype=torch.bool)
    valid = valid.bool().expand_as(pred) if valid.shape[1] == 1 else valid.bool()
    d = (pred - target).abs()
    return torch.where(valid, d, torch.zeros_like(d)).sum() / valid.sum()


def masked_l1_grad(pred, target, valid):
    """sign(pred - target) * float32(1 / count) where valid, 0 elsewhere (numpy fp32)."""
    valid = valid.bool().expand_as(pred) if valid.shape[1] == 1 else valid.bool()
    inv = np.float32(1.0 / float(valid.sum())) if int(valid.sum()) else np.float32(np.inf)
    s = torch.sign(pred - target).numpy().astype(np.float32)
    return np.where(valid.numpy(), s * inv, np.float32(0.0)).astype(np.float32)


def metric_terms(pred, target, valid, form):
    """(absrel * v, ratio, v) as fp32 tensors [B, C, ...]: every operation one fp32 tensor operation of the reference."""
    pred, target = pred.float(), target.float()
    v = valid.bool()
    v = (v.expand_as(pred) if v.shape[1] == 1 else v).float()
    if form == "curvature":
        p = torch.clamp(pred, min=-1, max=1)
        absrel = torch.abs(p - target) / torch.abs(target + 1e-6)
        ratio = torch.max(p / target, target / p)
    else:
        p, t = pred * v, target * v
        absrel = torch.abs(p - t) / (t + 1e-6)
        ratio = torch.max(p / (t + 1e-6), t / (p + 1e-6))
    return absrel * v, ratio, v


def metric_sums(pred, target, valid, form, thresholds=None):
    """fp64 [B, C, 5] = (sum absrel v, sum v, n < t1, n < t2, n < t3): the fp32 terms summed in fp64; thresholds compared in fp32."""
    thresholds = thresholds or (CURV_T if form == "curvature" else RESH_T)
    term, ratio, v = metric_terms(pred, target, valid, form)
    B, C = term.shape[:2]
    out = torch.zeros(B, C, 5, dtype=torch.float64)
    out[..., 0] = term.double().reshape(B, C, -1).sum(-1)
    out[..., 1] = v.double().reshape(B, C, -1).sum(-1)
    for j, t in enumerate(thresholds):
        hit = (ratio < t) & (v > 0)  # an fp32 tensor against a Python float: compared in fp32
        out[..., 2 + j] = hit.double().reshape(B, C, -1).sum(-1)
    return out


def curvature_metrics(sums):
    """[B, 2, 5] fp64 sums -> the reference's dict of [B] fp64 tensors."""
    n = sums[..., 1].clamp(min=1)
    absrel, acc = sums[..., 0] / n, sums[..., 2:5] / n.unsqueeze(-1)
    out = {"AbsRel": (absrel[:, 0] + absrel[:, 1]) / 2}
    for c, k in ((0, "k1"), (1, "k2")):
        for j, t in enumerate(("1.25", "2.5", "3.75")):
            out[f"δ{t}_{k}"] = acc[:, c, j]
    for j, t in enumerate(("1.25", "2.5", "3.75")):
        out[f"δ{t}_avg"] = (acc[:, 0, j] + acc[:, 1, j]) / 2
    return out


def reshading_metrics(sums, thresholds=RESH_T):
    """[B, C, 5] fp64 sums -> {"AbsRel", "δ_<t>"...} of [B] fp64 tensors, the mean over the channels."""
    n = sums[..., 1].clamp(min=1)
    out = {"AbsRel": (sums[..., 0] / n).mean(dim=1)}
    for j, t in enumerate(thresholds):
        out[f"δ_{t}"] = (sums[..., 2 + j] / n).mean(dim=1)
    return out


def margin(pred, target, valid):
    """min over valid elements of |pred - target|, over rms(pred): how far the L1 kink is from every valid pixel."""
    valid = valid.bool().expand_as(pred) if valid.shape[1] == 1 else valid.bool()
    d = (pred.double() - target.double()).abs()[valid]
    return float(d.min() / pred.double().pow(2).mean().sqrt())


def step_loss(pred_lowres, target, valid):
    """The training step's loss on a probe output: first C_t channels, bilinear resize, masked L1 (torch autograd)."""
    ct = target.shape[1]
    pred = F.interpolate(pred_lowres[:, :ct], size=target.shape[-2:], mode="bilinear", align_corners=False)
    return masked_l1(pred, target, valid), pred
