"""NYU-shaped synthetic dataset honouring the reference's per-sample dict contract (evals/datasets/nyu.py:245-251):
{"image": float32 [3,H,W] (ImageNet-normalised statistics), "depth": float32 [1,H,W] metres with 0 = invalid,
 "snorm": float32 [3,H,W] unit vectors, "segmentation": int64 [H,W] OneFormer ADE20K ids in 16x16 blobs}.  Samples are a pure function of (seed, split, index), so every rank and every
epoch sees the same sample for the same index — what DistributedSampler sharding assumes."""
from __future__ import annotations

import torch
from torch.utils.data import Dataset


class SyntheticNYU(Dataset):
    def __init__(self, split: str = "train", num_samples: int = 128, image_size=(480, 640), max_depth: float = 10.0,
                 invalid_fraction: float = 0.1, seed: int = 0, with_snorm: bool = True, name: str = "synthetic"):
        self.split, self.n, self.hw = split, int(num_samples), tuple(int(v) for v in image_size)
        self.max_depth, self.invalid_fraction, self.seed, self.with_snorm, self.name = float(max_depth), float(invalid_fraction), int(seed), with_snorm, name
        self._salt = {"train": 0, "valid": 1, "val": 1, "test": 2}.get(split, 3)

    def __len__(self) -> int:
        return self.n

    def __getitem__(self, i: int):
        if not 0 <= i < self.n:
            raise IndexError(i)
        g = torch.Generator().manual_seed((self.seed * 4 + self._salt) * 1_000_003 + i)
        H, W = self.hw
        image = torch.randn(3, H, W, generator=g)
        depth = torch.rand(1, H, W, generator=g) * (self.max_depth - 0.1) + 0.05
        depth[torch.rand(1, H, W, generator=g) < self.invalid_fraction] = 0.0
        out = {"image": image, "depth": depth}
        if self.with_snorm:
            n = torch.randn(3, H, W, generator=g)
            out["snorm"] = n / n.norm(dim=0, keepdim=True).clamp_min(1e-6)
        blobs = torch.randint(0, 150, ((H + 15) // 16, (W + 15) // 16), generator=g)
        out["segmentation"] = blobs.repeat_interleave(16, 0).repeat_interleave(16, 1)[:H, :W].contiguous()
        return out


class SyntheticVOC(Dataset):
    """VOC-shaped synthetic objectness samples honouring the reference's per-sample dict contract (evals/datasets/voc.py):
    {"original_image": float32 [3,S,S] ImageNet-normalised, "original_image_rgb": float32 [3,S,S] in [0,1], "gt_binary_mask": float32
    [1,S,S] of exact 0 / 1, "num_objects": int}.  The mask is the union of one to three seeded rectangles or ellipses (never empty,
    never the whole image) and the image is brighter inside it, so a probe has something to learn.  Samples are a pure function of
    (seed, split, index); splits: "trainval" and "test"."""

    MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

    def __init__(self, split: str = "trainval", num_samples: int = 64, fixed_size: int = 480, seed: int = 0, name: str = "voc"):
        if split not in ("trainval", "test"):
            raise ValueError(f"SyntheticVOC: split {split!r} (expected 'trainval' or 'test')")
        self.split, self.n, self.size, self.seed, self.name = split, int(num_samples), int(fixed_size), int(seed), name
        self._salt = {"trainval": 0, "test": 1}[split]

    def __len__(self) -> int:
        return self.n

    def __getitem__(self, i: int):
        if not 0 <= i < self.n:
            raise IndexError(i)
        g = torch.Generator().manual_seed((self.seed * 2 + self._salt) * 1_000_003 + i + 77_000_000)
        S = self.size
        num_objects = int(torch.randint(1, 4, (1,), generator=g))
        ys = torch.arange(S, dtype=torch.float32).view(S, 1)
        xs = torch.arange(S, dtype=torch.float32).view(1, S)
        mask = torch.zeros(S, S, dtype=torch.bool)
        for _ in range(num_objects):
            u = torch.rand(5, generator=g)
            # half-extents between an eighth and a quarter of the side, centre kept inside the image: the union of three shapes covers at most
            # 3/4 of it, a single one at least one pixel
            ry, rx = float(S * (0.125 + 0.125 * u[0])), float(S * (0.125 + 0.125 * u[1]))
            cy, cx = float(u[2] * (S - 1)), float(u[3] * (S - 1))
            if u[4] < 0.5:
                shape = ((ys - cy).abs() <= ry) & ((xs - cx).abs() <= rx)
            else:
                shape = ((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2 <= 1.0
            mask |= shape
        rgb = torch.rand(3, S, S, generator=g) * 0.5
        rgb = torch.where(mask, rgb + 0.5, rgb).clamp_(0.0, 1.0)
        mean = torch.tensor(self.MEAN).view(3, 1, 1)
        std = torch.tensor(self.STD).view(3, 1, 1)
        return {"original_image": (rgb - mean) / std, "original_image_rgb": rgb, "gt_binary_mask": mask.float().unsqueeze(0),
                "num_objects": num_objects}


class SyntheticNYURaw(SyntheticNYU):
    """SyntheticNYU as a file reader would hand its samples to the device-side augmentation (mvp.augment.DeviceAugment): "image" is
    uint8 [H, W, 3], raw pixels that are neither jittered nor normalised; "depth", "snorm" and "segmentation" follow SyntheticNYU's
    contract.  The image has structure — a smooth ramp per channel plus a few soft coloured blobs, on top of a little noise — so that
    hue and saturation have colour to act on and two crops of one image can be told apart."""

    def __getitem__(self, i: int):
        out = super().__getitem__(i)
        g = torch.Generator().manual_seed((self.seed * 4 + self._salt) * 1_000_003 + i + 55_000_000)
        H, W = self.hw
        ys = torch.linspace(0.0, 1.0, H).view(H, 1)
        xs = torch.linspace(0.0, 1.0, W).view(1, W)
        u = torch.rand(3, 4, generator=g)
        # one ramp per channel: direction, offset and gain drawn per sample
        rgb = torch.stack([(u[c, 0] * xs + u[c, 1] * ys) * 0.5 + 0.25 * u[c, 2] for c in range(3)])
        for _ in range(4):
            v = torch.rand(6, generator=g)
            bump = torch.exp(-(((ys - v[0]) / (0.08 + 0.2 * v[2])) ** 2 + ((xs - v[1]) / (0.08 + 0.2 * v[2])) ** 2))
            rgb = rgb + bump.unsqueeze(0) * (v[3:6].view(3, 1, 1) - 0.4)
        rgb = rgb + 0.02 * torch.randn(3, H, W, generator=g)
        out["image"] = (rgb.clamp(0.0, 1.0) * 255.0).round().to(torch.uint8).permute(1, 2, 0).contiguous()
        return out


class SyntheticTaskonomy(Dataset):
    """Taskonomy-shaped synthetic samples for one task of mvp.taskonomy.TASKS.  ``raw=True``: what a PNG decoder hands over — "rgb" uint8
    [H, W, 3]; the task's target uint8 [H, W, Cs] (8-bit tasks: Cs = 3 stored channels for principal_curvature and normal, 1 for
    reshading) or int16 [H, W] holding the uint16 bit patterns (16-bit tasks; torch batches carry no uint16); "mask_valid" uint8 [H, W]
    with 255 = valid.  ``raw=False``: the same sample through evals.datasets.transforms.task_transform — the reference's item contract
    {"rgb": float32 [3, H, W] normalised, task: float32 [Ct, H, W], "mask_valid": bool [1, H, W]}.

    About a tenth of each mask is invalid, in five ellipses whose borders cross the 4 x 4 blocks make_valid_mask grows them to; the
    targets are a smooth field plus noise with exact zeros sprinkled in (AbsRel's denominator then is the 1e-6 alone).  Samples are a pure
    function of (seed, split, task, index)."""

    def __init__(self, split: str = "train", task: str = "principal_curvature", num_samples: int = 64, image_size=(512, 512), raw: bool = True,
                 seed: int = 0, name: str = "taskonomy", image_mean="imagenet"):
        from mvp.taskonomy import resolve_task

        if split not in ("train", "valid", "val", "test"):
            raise ValueError(f"SyntheticTaskonomy: split {split!r}")
        self.kernel_task, self.spec = resolve_task("depth_euclidean" if task == "depth" else task)
        self.split, self.task, self.n = split, task, int(num_samples)
        self.hw = (int(image_size), int(image_size)) if isinstance(image_size, int) else tuple(int(v) for v in image_size)
        self.raw, self.seed, self.name, self.image_mean = bool(raw), int(seed), name, image_mean
        self._salt = {"train": 0, "valid": 1, "val": 1, "test": 2}[split]

    def __len__(self) -> int:
        return self.n

    def __getitem__(self, i: int):
        if not 0 <= i < self.n:
            raise IndexError(i)
        g = torch.Generator().manual_seed((self.seed * 4 + self._salt) * 1_000_003 + i + 33_000_000)
        H, W = self.hw
        ys = torch.linspace(0.0, 1.0, H).view(H, 1)
        xs = torch.linspace(0.0, 1.0, W).view(1, W)
        u = torch.rand(3, 3, generator=g)
        rgb = torch.stack([(u[c, 0] * xs + u[c, 1] * ys) * 0.5 + 0.25 * u[c, 2] for c in range(3)]) + 0.05 * torch.randn(3, H, W, generator=g)
        rgb = (rgb.clamp(0.0, 1.0) * 255.0).round().to(torch.uint8).permute(1, 2, 0).contiguous()
        # the target follows the image (something to learn) with its own noise
        bits, ct = int(self.spec["bits"]), int(self.spec["channels"])
        cs = 1 if bits == 16 or ct == 1 else 3
        base = rgb.permute(2, 0, 1).float()[:cs] / 255.0
        field = (0.6 * base + 0.25 + 0.1 * torch.randn(cs, H, W, generator=g)).clamp(0.0, 1.0)
        if self.spec["clamp"] is not None:
            field = field * (2.0 * float(self.spec["clamp"]))  # half of the values above the clamp
        top = 255.0 if bits == 8 else 65535.0
        k = (field * top).round().to(torch.int32)
        k[torch.rand(cs, H, W, generator=g) < 0.02] = 0
        if bits == 8:
            target = k.to(torch.uint8).permute(1, 2, 0).contiguous()
        else:
            target = torch.where(k[0] >= 32768, k[0] - 65536, k[0]).to(torch.int16).contiguous()
        mask = torch.full((H, W), 255, dtype=torch.uint8)
        yy = torch.arange(H, dtype=torch.float32).view(H, 1)
        xx = torch.arange(W, dtype=torch.float32).view(1, W)
        for _ in range(5):
            v = torch.rand(3, generator=g)
            f = 0.7 + 0.7 * float(v[2])
            ry, rx = max(H * 0.0798 * f, 0.75), max(W * 0.0798 / f, 0.75)  # pi ry rx = 2 % of the image
            cy, cx = float(v[0]) * (H - 1), float(v[1]) * (W - 1)
            mask[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = 0
        sample = {"rgb": rgb, self.task: target, "mask_valid": mask}
        if self.raw:
            return sample
        from .transforms import task_transform

        return {"rgb": task_transform(rgb, "rgb", self.image_mean), self.task: task_transform(target, self.kernel_task),
                "mask_valid": task_transform(mask, "mask_valid")}
