"""The fp64 definition of the 2AFC triplet scoring (include/mvp_hip.h: mvp_twoafc_score; reference: evaluate_model_percepture.py
:104-120) in torch on the CPU: global average pool, cosine similarity with F.cosine_similarity's two clamps, prediction, counts."""
import torch


def pool(x: torch.Tensor) -> torch.Tensor:
    """[B, C] (class tokens) or [B, C, ...] -> [B, C] fp64: the mean over everything behind the channel axis."""
    x = x.double()
    return x if x.dim() == 2 else x.flatten(2).mean(dim=2)


def cosine(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """<a, b> / (max(|a|, 1e-8) * max(|b|, 1e-8)) over the last axis, fp64."""
    a, b = a.double(), b.double()
    return (a * b).sum(-1) / (a.norm(dim=-1).clamp_min(1e-8) * b.norm(dim=-1).clamp_min(1e-8))


def counts(label: torch.Tensor, pred: torch.Tensor):
    """[TP, FP, FN, TN] with positive = 1."""
    label, pred = label.reshape(-1).double(), pred.reshape(-1).double()
    return [int(((pred == 1) & (label == 1)).sum()), int(((pred == 1) & (label == 0)).sum()),
            int(((pred == 0) & (label == 1)).sum()), int(((pred == 0) & (label == 0)).sum())]


def score(ref: torch.Tensor, left: torch.Tensor, right: torch.Tensor):
    """-> (sim [B, 2] fp64, pred [B] int64): pred = 0 where sim(left) > sim(right), else 1 (NaN compares false)."""
    f = pool(ref)
    sim = torch.stack((cosine(f, pool(left)), cosine(f, pool(right))), dim=1)
    pred = torch.where(sim[:, 0] > sim[:, 1], 0, 1)
    return sim, pred


def metrics(c):
    """accuracy / F1 / precision / recall of [TP, FP, FN, TN], 0.0 where a denominator is 0."""
    tp, fp, fn, tn = c

    def r(n, d):
        return n / d if d else 0.0

    return {"accuracy": r(tp + tn, tp + fp + fn + tn), "f1_score": r(2 * tp, 2 * tp + fp + fn), "precision": r(tp, tp + fp), "recall": r(tp, tp + fn)}
