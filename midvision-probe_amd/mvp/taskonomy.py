"""Taskonomy pixel-to-pixel probing on the HIP path: the task table, the device-side sample transform, validation and the result CSV.

The reference wires this family through configs/taskonomy_training.yaml, evals.datasets.taskonomy, evals.models.probes.TaskonomyHead,
evals.utils.losses.MaskedL1Loss and two metric functions, but ships no trainer; INTEGRATION.md lists the conventions fixed here
(prediction sliced to the target's channels before the bilinear resize, probe in eval mode for validation, no augmentation).

A raw batch, as a decoder leaves it — "rgb" uint8 [B, H, W, 3], the task's target uint8 [B, H, W, Cs] or 16-bit [B, H, W], "mask_valid"
uint8 [B, H, W] — crosses the host link as bytes; ``DeviceTaskTransform`` turns it into the training tensors with two launches
(mvp_augment_apply in its normalise-only form, mvp_task_prepare)."""
from __future__ import annotations

import csv
import os
from typing import Dict, Iterable, Iterator, Tuple

import torch

# bits of the stored sample, channels of the target, upper clamp (the reference's clamp_to = (0, clamp); rescaled to [0, 1])
TASKS = {
    "principal_curvature": {"bits": 8, "channels": 2, "clamp": None},
    "reshading": {"bits": 8, "channels": 1, "clamp": None},
    "normal": {"bits": 8, "channels": 3, "clamp": None},
    "depth_euclidean": {"bits": 16, "channels": 1, "clamp": 8000.0 / 65535.0},
    "depth_zbuffer": {"bits": 16, "channels": 1, "clamp": 8000.0 / 65535.0},
    "edge_texture": {"bits": 16, "channels": 1, "clamp": 0.25},
    "keypoints2d": {"bits": 16, "channels": 1, "clamp": None},
    "keypoints3d": {"bits": 16, "channels": 1, "clamp": None},
}
ALIASES = {"curvature": "principal_curvature"}
_OUT_OF_SCOPE = {
    "edge_occlusion": "it blurs the target with torchvision's GaussianBlur, and torchvision is not a dependency of this path",
    **{t: "segmentation targets are class maps, not regression targets"
       for t in ("segment_semantic", "segment_instance", "segment_panoptic", "fragments", "segment_unsup2d", "segment_unsup25d")},
    **{t: "classification targets are not pixel-to-pixel" for t in ("class_object", "class_scene")},
}
RESHADING_THRESHOLDS = [1.1, 1.1**2, 1.1**3]  # the reference's defaults; their str() is part of the metric keys


def resolve_task(task: str) -> Tuple[str, Dict[str, object]]:
    """(canonical name, TASKS entry); NotImplementedError with the reason for the reference's tasks that are out of scope."""
    name = ALIASES.get(task, task)
    if name in TASKS:
        return name, TASKS[name]
    if name in _OUT_OF_SCOPE:
        raise NotImplementedError(f"Taskonomy task {task!r} is out of scope: {_OUT_OF_SCOPE[name]}")
    raise ValueError(f"unknown Taskonomy task {task!r} (in scope: {sorted(TASKS) + sorted(ALIASES)})")


def kernel_task(task: str) -> str:
    """The dataset's ``task == "depth"`` reads the key "depth" with depth_euclidean's transform; ``resolve_task("depth")`` itself raises."""
    return "depth_euclidean" if task == "depth" else task


def target_channels(task: str) -> int:
    return int(resolve_task(task)[1]["channels"])


def prepare_batch(target_raw: torch.Tensor, mask_raw: torch.Tensor, task: str):
    """Raw device target / mask -> (target fp32 [B, Ct, H, W], valid uint8 [B, 1, H, W]) with one launch."""
    from . import ops

    _, spec = resolve_task(task)
    B, H, W = mask_raw.shape
    bits = int(spec["bits"])
    if bits == 8 and target_raw.dim() == 3:
        target_raw = target_raw.unsqueeze(-1)
    if bits == 16 and target_raw.dim() == 4:
        target_raw = target_raw.reshape(B, H, W)
    target = torch.empty(B, int(spec["channels"]), H, W, dtype=torch.float32, device=mask_raw.device)
    valid = torch.empty(B, 1, H, W, dtype=torch.uint8, device=mask_raw.device)
    clamp = float(torch.tensor(spec["clamp"], dtype=torch.float32)) if spec["clamp"] is not None else 0.0
    ops.task_prepare(target_raw.contiguous(), mask_raw.contiguous(), target, valid, bits, clamp)
    return target, valid


class DeviceTaskTransform:
    """An iterable over raw device batches (normally a DevicePrefetcher over a loader of SyntheticTaskonomy(raw=True)-style samples) that
    yields {"rgb": float32 [B, 3, H, W] normalised, <task>: float32 [B, Ct, H, W], "mask_valid": uint8 [B, 1, H, W] of 0 / 1}.  Outputs
    are new tensors per batch and the raw inputs have been consumed (their kernels enqueued) when a batch is yielded, so a look-ahead
    consumer may hold batches as long as it likes.  No augmentation: the reference's Taskonomy() accepts augment_train / center_crop
    and ignores them."""

    def __init__(self, prefetcher: Iterable[Dict[str, object]], task: str, image_mean="imagenet"):
        from .augment import mean_std

        if not torch.cuda.is_available():
            raise RuntimeError("DeviceTaskTransform needs a HIP device (no CPU fallback on the product path)")
        mean_std(image_mean)
        resolve_task(kernel_task(task))
        self.batches, self.task, self.image_mean = prefetcher, task, image_mean
        self._scratch = {}

    def __len__(self):
        return len(self.batches)

    @property
    def sampler(self):
        return getattr(self.batches, "sampler", None)

    def _normalise(self, rgb: torch.Tensor) -> torch.Tensor:
        from . import ops
        from .augment import identity_entry, mean_std, pack_params

        B, H, W = rgb.shape[:3]
        key = (B, H, W, rgb.device)
        held = self._scratch.get(key)
        if held is None:
            # the normalise-only form of mvp_augment_apply carries a depth plane along: a zero plane in, a scratch plane out
            held = self._scratch[key] = (pack_params([identity_entry(H, W)] * B).to(rgb.device),
                                         torch.zeros(B, 1, H, W, dtype=torch.float32, device=rgb.device),
                                         torch.empty(B, 1, H, W, dtype=torch.float32, device=rgb.device))
        table, depth_in, depth_out = held
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=rgb.device)
        mean, std = mean_std(self.image_mean)
        ops.augment_apply(rgb, depth_in, None, table, None, out, depth_out, None, mean, std)
        return out

    def __iter__(self) -> Iterator[Dict[str, object]]:
        side = getattr(self.batches, "stream", None)
        if side is not None:
            # one prefetcher serves every pass: its first copies of this pass reuse the buffers the last launches of the previous pass read
            side.wait_stream(torch.cuda.current_stream())
        name = kernel_task(self.task)
        for batch in self.batches:
            rgb = batch["rgb"]
            if not rgb.is_cuda:
                raise RuntimeError("DeviceTaskTransform takes device batches: wrap the loader in mvp.prefetch.DevicePrefetcher")
            target, valid = prepare_batch(batch[self.task], batch["mask_valid"], name)
            yield {"rgb": self._normalise(rgb.contiguous()), self.task: target, "mask_valid": valid}


def predict(probe, feats, task: str, size) -> torch.Tensor:
    """probe -> the target's channels -> bilinear resize to the target (the slice comes first: the unused channels are not resized)."""
    from . import functional as MF

    ct = target_channels(kernel_task(task))
    pred = probe(feats)
    if pred.shape[1] < ct:
        raise ValueError(f"the probe has {pred.shape[1]} output channels, task {task!r} needs {ct} (probe.output_dim)")
    return MF.interpolate(pred[:, :ct], size=tuple(size), mode="bilinear", align_corners=False)


def metric_keys(task: str):
    name, _ = resolve_task(kernel_task(task))
    if name == "principal_curvature":
        return ["AbsRel"] + [f"δ{t}_{k}" for k in ("k1", "k2") for t in ("1.25", "2.5", "3.75")] + [f"δ{t}_avg" for t in ("1.25", "2.5", "3.75")]
    return ["AbsRel"] + [f"δ_{t}" for t in RESHADING_THRESHOLDS]


def batch_metrics(pred: torch.Tensor, target: torch.Tensor, valid: torch.Tensor, task: str) -> Dict[str, torch.Tensor]:
    """Per-image metrics ([B] host tensors) of one batch: ``evaluate_curvature_absrel`` for principal curvature; every other task one
    channel at a time through ``evaluate_reshading_absrel_and_delta`` (one launch chain for all channels), the mean over the channels."""
    from evals.utils.metrics import _per_image, evaluate_curvature_absrel, task_metric_sums

    name, _ = resolve_task(kernel_task(task))
    if name == "principal_curvature":
        return evaluate_curvature_absrel(pred, target, valid)
    absrel, acc = _per_image(task_metric_sums(pred, target, valid, "reshading", RESHADING_THRESHOLDS).cpu())
    out = {"AbsRel": absrel.mean(dim=1).float()}
    for j, t in enumerate(RESHADING_THRESHOLDS):
        out[f"δ_{t}"] = acc[:, :, j].mean(dim=1).float()
    return out


def validation(model, probe, loader, task: str) -> Dict[str, float]:
    """The mean of the per-image metrics over the whole loader (every image weighs the same whatever its batch).  ``loader`` yields
    device batches {"rgb", task, "mask_valid"} (a DeviceTaskTransform) or a host DataLoader of already transformed samples.  The probe
    is put in eval mode and returned to its mode afterwards."""
    from .pipeline import pipelined_features
    from .train import _device_batches

    dev = torch.device("cuda", torch.cuda.current_device())
    was_training = probe.training
    probe.eval()
    sums, n = {}, 0
    try:
        with torch.no_grad():
            batches = _device_batches(loader, dev, keys=("rgb", task, "mask_valid"))
            for batch, feats in pipelined_features(model, batches, image_key="rgb", probe=probe):
                target = batch[task].to(dev, non_blocking=True).float()
                valid = batch["mask_valid"].to(dev, non_blocking=True)
                pred = predict(probe, feats, task, target.shape[-2:])
                for k, v in batch_metrics(pred, target, valid, task).items():  # 5 B C numbers cross to the host here
                    sums[k] = sums.get(k, 0.0) + float(v.double().sum())
                n += target.shape[0]
    finally:
        probe.train(was_training)
    if n == 0:
        raise ValueError("validation(): empty loader")
    return {k: v / n for k, v in sums.items()}


def append_result_csv(output_dir: str, task: str, model_name: str, avg: Dict[str, float]) -> str:
    """<output_dir>/result/taskonomy-<task>/results.csv: one row per run, the header written once."""
    path = os.path.join(output_dir, "result", f"taskonomy-{task}", "results.csv")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    keys = metric_keys(task)
    if not os.path.exists(path):
        with open(path, mode="w", newline="") as f:
            csv.writer(f).writerow(["Model Name"] + keys)
    with open(path, mode="a", newline="") as f:
        csv.writer(f).writerow([model_name] + [avg[k] for k in keys])
    return path
