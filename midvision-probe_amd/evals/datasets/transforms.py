"""evals.datasets.transforms — the per-sample Taskonomy transforms of the reference (evals/datasets/transforms.py:58-181
``transform_16bit_single_channel``, ``make_valid_mask``, ``task_transform``) on the host, torch only (no torchvision).

Two uses: loaders that hand out decoded arrays or float tensors per sample (evals.datasets.taskonomy.TaskonomyDataset), and the host
side of the tests of the device path (mvp.taskonomy.DeviceTaskTransform runs the same conventions in csrc/taskonomy.hip):
  8-bit targets    uint8 [H, W] or [H, W, Cs] -> float32 [Ct, H, W] = k / 255 (ToTensor), the first Ct channels
  16-bit targets   uint16 [H, W] (numpy) or int16 holding those bit patterns (torch) -> float32 [1, H, W] = k / 65535
  clamp_to         min(max(x, 0), maxx) / maxx with maxx rounded to fp32 (torch.clamp with a Python scalar, then Normalize([0], [maxx]))
  rgb              k / 255, then (x - mean) / std
  mask_valid       k / 255, then ``make_valid_mask``
Every division is a true fp32 division."""
from __future__ import annotations

import numpy as np
import torch

from mvp.taskonomy import resolve_task


def make_valid_mask(mask_float: torch.Tensor, max_pool_size: int = 4) -> torch.Tensor:
    """Reference: transforms.py:74-93 — invalid areas grown to whole ``max_pool_size`` blocks.  ``mask_float`` [c, h, w] or [b, c, h, w]
    with 1 = valid; returns bool of the same shape.  The integer form of max_pool2d(k) + nearest interpolate + ``== 0``: pixel (y, x)
    reads block ((y hp) // h, (x wp) // w) of the hp x wp = (h // k) x (w // k) pooled map, and a block is valid iff all its k x k
    values equal 1; rows and columns from k hp / k wp on are in no block."""
    k = int(max_pool_size)
    h, w = mask_float.shape[-2:]
    hp, wp = h // k, w // k
    if hp < 1 or wp < 1:
        raise ValueError(f"make_valid_mask: a {h} x {w} mask has no {k} x {k} block")
    lead = mask_float.shape[:-2]
    ok = (mask_float[..., : hp * k, : wp * k] == 1).reshape(*lead, hp, k, wp, k).all(dim=-1).all(dim=-2)
    iy = (torch.arange(h) * hp) // h
    ix = (torch.arange(w) * wp) // w
    return ok[..., iy, :][..., ix]


def _to_chw_u(array) -> torch.Tensor:
    """A decoded sample (numpy or torch, [H, W] or [H, W, C], 8- or 16-bit) -> int32 [C, H, W] of the unsigned values."""
    if isinstance(array, np.ndarray):
        if array.dtype == np.uint16:
            array = array.astype(np.int32)
        t = torch.from_numpy(np.ascontiguousarray(array))
    else:
        t = torch.as_tensor(np.asarray(array)) if not torch.is_tensor(array) else array
    if t.dtype == torch.int16:  # the uint16 bit patterns (torch batches carry them as int16)
        t = t.to(torch.int32) & 0xFFFF
    t = t.to(torch.int32)
    if t.dim() == 2:
        t = t.unsqueeze(-1)
    return t.permute(2, 0, 1).contiguous()


def _decode(array, den: float) -> torch.Tensor:
    if torch.is_tensor(array) and array.is_floating_point():  # a loader that already produced [C, H, W] in [0, 1]
        return array.float()
    return _to_chw_u(array).to(torch.float32) / torch.tensor(den, dtype=torch.float32)


def task_transform(array, task: str, image_mean="imagenet"):
    """Reference: transforms.py:96-181 for "rgb", "mask_valid" and the tasks of mvp.taskonomy.TASKS."""
    if task == "rgb":
        from mvp.augment import mean_std

        mean, std = mean_std(image_mean)
        x = _decode(array, 255.0)
        return (x - torch.tensor(mean, dtype=torch.float32).view(3, 1, 1)) / torch.tensor(std, dtype=torch.float32).view(3, 1, 1)
    if task == "mask_valid":
        return make_valid_mask(_decode(array, 255.0))
    name, spec = resolve_task(task)
    x = _decode(array, 255.0 if spec["bits"] == 8 else 65535.0)
    if x.shape[0] < spec["channels"]:
        raise ValueError(f"task {name}: the sample has {x.shape[0]} channels, the target {spec['channels']}")
    x = x[: spec["channels"]]
    if spec["clamp"] is not None:
        maxx = torch.tensor(spec["clamp"], dtype=torch.float32)
        x = torch.clamp(x, min=0.0).minimum(maxx) / maxx
    return x.contiguous()
