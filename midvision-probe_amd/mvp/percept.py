"""The 2AFC perceptual-similarity evaluation (reference: evaluate_model_percepture.py): a backbone embeds the three images of a
triplet, the one of left / right whose embedding has the larger cosine similarity to the reference image's is the prediction, and
the predictions are scored against the human votes with accuracy / F1 / precision / recall.

``predict_batch`` stacks the three images of a batch into one forward, scores it with mvp_twoafc_score in stream order behind the
forward (class tokens as they are, CNN maps with the global average pool fused in) and keeps the predictions and the running
confusion counts on the device: one device-to-host transfer per shard, after the loop."""
from __future__ import annotations

import functools
from typing import Dict, Sequence, Tuple

import torch

from . import lib, ops
from .evalloop import PinnedRing, gather_parts
from .evalloop import shard as shard_batches  # the same function: rank r takes loader batches r, r + W, ...

METRIC_NAMES = ("accuracy", "f1_score", "precision", "recall")
CSV_HEADER = ["Model Name", "Test Accuracy", "Test F1-Score", "Test Precision", "Test Recall"]
_CONFIG_HINT = ("configure the backbone for this evaluation with return_cls=True (backbone.return_cls=True) and a single layer "
                "(return_multilayer=False): a ViT then returns its class token [B, C], a ResNet-50 its last map [B, C, h, w]")


# ----------------------------------------------------------------------------- scoring
def score_triplets(ref: torch.Tensor, left: torch.Tensor, right: torch.Tensor, label=None, counts=None, accumulate=False,
                   pred=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (sim [B, 2] fp32, pred [B] int32) of B triplets.  ref / left / right: fp32 device tensors [B, C] or [B, C, h, w], each
    contiguous per image with the same stride between images (slices of one stacked forward output are taken as they are).
    label [B] fp32 (0 / 1) with counts [4] int64: TP, FP, FN, TN, overwritten or (accumulate) added to.  pred: where to write the
    predictions (a [B] int32 device tensor; predict_batch passes a slice of its shard's log)."""
    for t in (ref, left, right):
        if not t.is_cuda:
            raise lib.MvpError("score_triplets needs device tensors (no CPU fallback)")
        if t.dtype != torch.float32 or t.shape != ref.shape or t.dim() not in (2, 4) or t.stride() != ref.stride():
            raise ValueError(f"score_triplets: three fp32 tensors of one shape [B, C] or [B, C, h, w], got {tuple(t.shape)} {t.dtype}")
    B, Cdim = ref.shape[:2]
    HW = 1 if ref.dim() == 2 else ref.shape[2] * ref.shape[3]
    if not ref[0].is_contiguous():  # (equal strides: this holds for left and right too)
        raise ValueError("score_triplets: every image must be contiguous")
    ld = ref.stride(0) if B > 1 else Cdim * HW
    dev = ref.device
    sim = torch.empty(B, 2, dtype=torch.float32, device=dev)
    pred = torch.empty(B, dtype=torch.int32, device=dev) if pred is None else pred
    ws = torch.empty(max(1, ops.twoafc_workspace_bytes(B, Cdim, HW) // 8), dtype=torch.float64, device=dev)
    ops.twoafc_score(ref, left, right, sim, pred, ws, B, Cdim, HW, ld, label=label, counts=counts, accumulate=accumulate)
    return sim, pred


def score_pixel_triplets(ref: torch.Tensor, left: torch.Tensor, right: torch.Tensor, metric: str, label=None, counts=None,
                          accumulate=False, pred=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """score_triplets for the pixel-level baselines: -> (sim [B, 2] fp32, pred [B] int32) of B triplets of IMAGES under ``metric``
    ("psnr": 10 log10(1 / mse), peak 1; "ssim": the reference's 11 x 11 Gaussian SSIM, per image).  ref / left / right: fp32 device
    tensors [B, C, H, W], each contiguous per image with the same stride between images (slices of one stacked batch are taken as they
    are); values are used as they are, nothing is clamped.  label / counts / accumulate / pred as in score_triplets."""
    if metric not in ops.PIXEL_METRICS:
        raise ValueError(f"score_pixel_triplets: metric {metric!r}; one of {sorted(ops.PIXEL_METRICS)}")
    for t in (ref, left, right):
        if not t.is_cuda:
            raise lib.MvpError("score_pixel_triplets needs device tensors (no CPU fallback)")
        if t.dtype != torch.float32 or t.shape != ref.shape or t.dim() != 4 or t.stride() != ref.stride():
            raise ValueError(f"score_pixel_triplets: three fp32 tensors of one shape [B, C, H, W], got {tuple(t.shape)} {t.dtype}")
    B, Cdim, H, W = ref.shape
    if not ref[0].is_contiguous():  # (equal strides: this holds for left and right too)
        raise ValueError("score_pixel_triplets: every image must be contiguous")
    ld = ref.stride(0) if B > 1 else Cdim * H * W
    dev = ref.device
    sim = torch.empty(B, 2, dtype=torch.float32, device=dev)
    pred = torch.empty(B, dtype=torch.int32, device=dev) if pred is None else pred
    ws = torch.empty(max(1, ops.pixel_score_workspace_bytes(B, Cdim, H, W, metric) // 8), dtype=torch.float64, device=dev)
    ops.pixel_score(ref, left, right, sim, pred, ws, B, Cdim, H, W, ld, metric, label=label, counts=counts, accumulate=accumulate)
    return sim, pred


def cosine_similarity_batch(tensor1: torch.Tensor, tensor2: torch.Tensor) -> torch.Tensor:
    """evaluate_model_percepture.py:46-48: F.cosine_similarity(tensor1, tensor2, dim=-1) of device tensors [B, C] -> [B] fp32, through
    the score kernel (fp64 accumulation, one rounding)."""
    if tensor1.shape != tensor2.shape or tensor1.dim() != 2:
        raise ValueError(f"cosine_similarity_batch: two [B, C] tensors, got {tuple(tensor1.shape)} and {tuple(tensor2.shape)}")
    a, b = tensor1.detach().float().contiguous(), tensor2.detach().float().contiguous()
    sim, _ = score_triplets(a, b, b)
    return sim[:, 0]


# ----------------------------------------------------------------------------- metrics
def metrics_from_counts(tp: int, fp: int, fn: int, tn: int) -> Dict[str, float]:
    """sklearn's accuracy_score / f1_score / precision_score / recall_score for binary labels with positive label 1, from the confusion
    counts; a ratio whose denominator is 0 is 0.0 (sklearn's zero_division default, which also warns)."""
    tp, fp, fn, tn = int(tp), int(fp), int(fn), int(tn)

    def ratio(n, d):
        return n / d if d else 0.0

    return {"accuracy": ratio(tp + tn, tp + fp + fn + tn), "f1_score": ratio(2 * tp, 2 * tp + fp + fn),
            "precision": ratio(tp, tp + fp), "recall": ratio(tp, tp + fn)}


def _check_labels(values, what: str) -> None:
    bad = [v for v in values if v != 0 and v != 1]
    if bad:
        raise ValueError(f"{what}: binary labels 0 / 1 expected, found {bad[0]!r}")


def counts_from_labels(gt_labels: Sequence, pred_labels: Sequence) -> Tuple[int, int, int, int]:
    """(TP, FP, FN, TN) with positive = 1 of two host sequences of 0 / 1."""
    gt, pr = [float(v) for v in gt_labels], [float(v) for v in pred_labels]
    if len(gt) != len(pr):
        raise ValueError(f"{len(gt)} labels against {len(pr)} predictions")
    _check_labels(gt, "gt_labels")
    _check_labels(pr, "pred_labels")
    tp = sum(1 for g, p in zip(gt, pr) if g == 1 and p == 1)
    fp = sum(1 for g, p in zip(gt, pr) if g == 0 and p == 1)
    fn = sum(1 for g, p in zip(gt, pr) if g == 1 and p == 0)
    return tp, fp, fn, len(gt) - tp - fp - fn


def compute_metrics(gt_labels, pred_labels) -> Dict[str, float]:
    """evaluate_model_percepture.py:51-64, without sklearn."""
    return metrics_from_counts(*counts_from_labels(gt_labels, pred_labels))


# ----------------------------------------------------------------------------- sharding
def merge_shards(parts):
    """parts: per rank (rows, counts, errors), rows = [(batch index, [result dicts])].  -> (results in loader order, summed counts,
    errors)."""
    rows = sorted((r for part in parts for r in part[0]), key=lambda r: r[0])
    results = [d for _, ds in rows for d in ds]
    counts = [sum(int(part[1][k]) for part in parts) for k in range(4)]
    errors = [e for part in parts for e in part[2]]
    return results, counts, errors


def _to_host(t: torch.Tensor) -> torch.Tensor:
    """The one device-to-host transfer of a shard."""
    return t.cpu()


_LOG_CAPACITY = 1024  # predictions a shard's log starts with when the loader does not say how many triplets it holds


class _DeviceLog:
    """The running counts [4] int64 and the int32 predictions of a shard in ONE device buffer, so that one transfer brings both."""

    def __init__(self, capacity: int, dev):
        self.dev, self.n = dev, 0
        self.buf = torch.zeros(4 + (max(1, capacity) + 1) // 2, dtype=torch.int64, device=dev)

    def reserve(self, B: int):
        """-> (the next B predictions, the counts), both views of the buffer as it is AFTER any growth.  They are handed out together
        because growing replaces the buffer: a counts view taken before it would be added to and then left behind."""
        cap = (self.buf.numel() - 4) * 2
        if self.n + B > cap:  # a loader without a length, or one that yields more than it announced: grow on the device
            grown = torch.zeros(4 + max(cap, self.n + B), dtype=torch.int64, device=self.dev)
            grown[:self.buf.numel()].copy_(self.buf)
            self.buf = grown
        pred = self.buf[4:].view(torch.int32)[self.n:self.n + B]
        self.n += B
        return pred, self.buf[:4]

    def fetch(self):
        host = _to_host(self.buf)
        return [int(v) for v in host[:4]], host[4:].view(torch.int32)[:self.n].tolist()


def _triplet_features(model, feats):
    """The forward's output as the kernel's operand: [3B, C] for a ViT, [3B, C, h, w] otherwise."""
    if isinstance(feats, (list, tuple)):
        raise ValueError(f"the backbone returned {len(feats)} feature maps (return_multilayer=True); {_CONFIG_HINT}")
    want = 2 if getattr(model, "arch", None) == "vit" else 4
    if not torch.is_tensor(feats) or feats.dim() != want:
        got = tuple(feats.shape) if torch.is_tensor(feats) else type(feats).__name__
        raise ValueError(f"arch {getattr(model, 'arch', None)!r} must return a rank-{want} tensor for this evaluation, got {got}; {_CONFIG_HINT}")
    if feats.shape[0] % 3:
        raise ValueError(f"{feats.shape[0]} feature rows for a stacked batch of triplets")
    return feats.detach().float().contiguous()  # (both no-ops on the wrappers' outputs)


def predict_batch(model, dataloader, output_dir, wandb_use=False, rank: int = 0, world: int = 1):
    """Reference: evaluate_model_percepture.py:67-167 -> (results, metrics, errors); results = [{"id", "gt", "prediction"}] in loader
    order.  ``output_dir`` and ``wandb_use`` are accepted and unused (the reference's csv dump is commented out; no wandb here).
    With world > 1 every rank returns the merged result of all ranks."""
    if not torch.cuda.is_available():
        raise lib.MvpError("predict_batch needs a GPU: the evaluation runs on the device (no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    model = model.to(dev)
    model.eval()
    ring = PinnedRing(4)
    try:  # a shard's share of the triplets, rounded up by one batch
        capacity = -(-len(dataloader.dataset) // world) + (getattr(dataloader, "batch_size", None) or 1)
    except (TypeError, AttributeError):  # a plain iterable of batches: the log grows as needed
        capacity = _LOG_CAPACITY
    log = _DeviceLog(capacity, dev)
    rows, errors = [], []
    try:
        n_batches = len(dataloader)
    except TypeError:  # a generator of batches, a loader over an iterable dataset: the shard is cut from the number of batches
        dataloader = list(dataloader)
        n_batches = len(dataloader)
    mine = set(shard_batches(n_batches, rank, world))
    for bi, batch in enumerate(dataloader):  # every rank walks the whole loader
        if bi not in mine:
            continue
        try:  # the reference's blanket try / except, kept for what can go wrong BEFORE anything is launched
            img_ref, img_left, img_right, p, ids = batch
            B = int(img_ref.shape[0])
            gts = [float(v) for v in torch.as_tensor(p).reshape(-1).tolist()]
            id_list = [int(v) for v in torch.as_tensor(ids).reshape(-1).tolist()]
            if not (len(gts) == len(id_list) == B and img_left.shape == img_ref.shape and img_right.shape == img_ref.shape):
                raise RuntimeError(f"batch {bi}: {B} reference images, {tuple(img_left.shape)} / {tuple(img_right.shape)} left / right, "
                                   f"{len(gts)} labels, {len(id_list)} ids")
        except Exception as e:  # noqa: BLE001
            errors.append(f"Error processing batch: {e}")
            print(errors[-1])
            continue
        _check_labels(gts, f"batch {bi}")  # sklearn rejects them too; here they would silently fall out of the counts
        images = ring.to_device((img_ref, img_left, img_right), dev).flatten(0, 1)  # [3B, 3, H, W]: ref | left | right
        label = ring.to_device((torch.as_tensor(p).reshape(-1),), dev)[0]
        if getattr(model, "arch", None) == "metric":  # PSNR / SSIM (evals/models/pixel_metrics.py): no forward, the images are scored
            feats, score = images, functools.partial(score_pixel_triplets, metric=model.metric)
        else:
            with torch.no_grad():
                feats, score = _triplet_features(model, model(images)), score_triplets
        pred, counts = log.reserve(B)
        score(feats[:B], feats[B:2 * B], feats[2 * B:], label=label, counts=counts, accumulate=True, pred=pred)
        rows.append((bi, id_list, gts))
    counts, preds = log.fetch()
    out_rows, k = [], 0
    for bi, id_list, gts in rows:
        out_rows.append((bi, [{"id": i, "gt": g, "prediction": int(pr)} for i, g, pr in zip(id_list, gts, preds[k:k + len(gts)])]))
        k += len(gts)
    results, counts, errors = merge_shards(gather_parts((out_rows, counts, errors), world))
    return results, metrics_from_counts(*counts), errors


# ----------------------------------------------------------------------------- data
class SyntheticTwoAFC(torch.utils.data.Dataset):
    """2AFC-shaped triplets with the item contract of evals/datasets/twoafcdataset.py:46-58: (img_ref, img_left, img_right, p, id),
    images [3, H, W] fp32, p float32 0 / 1, id an int.  One of left / right is the reference image plus small noise, the other an
    independent image; p = 1 when the LEFT one is the independent (far) image, i.e. p is the label of the closer side as the
    evaluation predicts it (0 = left closer, 1 = right closer).  Item i depends on (seed, i) alone.

    ``preprocess``: "DEFAULT" gives unnormalised Gaussian images, what a backbone's normalised input looks like.  "SSIM" / "PSNR" (the
    model types of the reference's get_preprocess whose transform is ToTensor() alone) give what a decoded 8-bit image looks like:
    values k / 255 in [0, 1].  The reference image is a smooth field (a bilinearly enlarged 4 x 4 grid in [0.25, 0.75]) plus noise of
    0.08, the near image the reference plus ``noise`` x Gaussian noise, clamped and quantised again, the far image an independent
    image of the same kind."""

    name = "synthetic_twoafc"

    def __init__(self, num_triplets=64, image_size=224, seed=0, noise=0.05, split="test", preprocess="DEFAULT"):
        if preprocess not in ("DEFAULT", "SSIM", "PSNR"):
            raise ValueError(f"SyntheticTwoAFC: preprocess {preprocess!r}; one of DEFAULT, SSIM, PSNR")
        self.n, self.seed, self.noise, self.split, self.preprocess = int(num_triplets), int(seed), float(noise), split, preprocess
        self.size = (int(image_size), int(image_size)) if isinstance(image_size, int) else tuple(int(v) for v in image_size)

    def __len__(self):
        return self.n

    @staticmethod
    def _natural(g, H, W):
        coarse = torch.rand(1, 3, 4, 4, generator=g)
        field = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)[0]
        return 0.25 + 0.5 * field + 0.08 * torch.randn(3, H, W, generator=g)

    @staticmethod
    def _eight_bit(x):
        return (x.clamp(0.0, 1.0) * 255.0).round() / 255.0

    def __getitem__(self, i):
        import numpy as np

        if not 0 <= i < self.n:
            raise IndexError(i)
        g = torch.Generator().manual_seed(self.seed * 7919 + int(i))
        H, W = self.size
        if self.preprocess == "DEFAULT":
            ref = torch.randn(3, H, W, generator=g)
            near = ref + self.noise * torch.randn(3, H, W, generator=g)
            far = torch.randn(3, H, W, generator=g)
        else:
            ref = self._eight_bit(self._natural(g, H, W))
            near = self._eight_bit(ref + self.noise * torch.randn(3, H, W, generator=g))
            far = self._eight_bit(self._natural(g, H, W))
        p = int(torch.randint(0, 2, (1,), generator=g))
        left, right = (far, near) if p == 1 else (near, far)
        return ref, left, right, np.float32(p), int(i)
