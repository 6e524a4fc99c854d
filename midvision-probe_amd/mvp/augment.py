"""Device-side training augmentation (reference: get_nyu_transforms, evals/datasets/utils.py:160-218, applied per sample on the host by
nyu.py:227-239): ColorJitter(0.2, 0.2, 0.2, 0.2) with probability 0.8 on the image, then one geometric transform shared by image, depth and
normals — HorizontalFlip, Rotate(limit=10), RandomResizedCrop(scale=(0.5, 1), ratio=(1, 1), p=0.5), all nearest-neighbour — then Normalize.

The random draws are made here, on the host, one small table per batch (``sample_params``); the pixels never leave the device: two launches
of csrc/augment.hip per batch (``DeviceAugment``).  ``index_map`` restates the composed integer source index of every output pixel; it is
what the kernel computes and what tests/augment_ref.py's stage-by-stage pipeline arrives at.  include/mvp_hip.h documents the table."""
from __future__ import annotations

import math
from typing import Dict, Iterable, Iterator, List, Optional, Sequence, Tuple

import torch

from . import ops

WORDS = 16  # MVP_AUGMENT_WORDS: 32-bit words per image in the parameter table
FLAG_JITTER, FLAG_FLIP, FLAG_ROTATE = 1, 2, 4
OPS = ("brightness", "contrast", "saturation", "hue")  # operation ids 0..3 of the order word
MEAN_STD = {
    "imagenet": ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),
    "clip": ((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)),
    "None": ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
}
_DRAWS = 14 + 40  # uniforms per image: a fixed count whatever the branches taken, so image b's draws do not depend on image a's


def mean_std(image_mean) -> Tuple[Tuple[float, float, float], Tuple[float, float, float]]:
    key = "None" if image_mean is None else str(image_mean)
    if key not in MEAN_STD:
        raise ValueError(f"image_mean {image_mean!r} (expected 'imagenet', 'clip' or None)")
    return MEAN_STD[key]


def identity_entry(H: int, W: int) -> Dict[str, object]:
    """The entry that changes nothing: no jitter, no flip, no rotation, the full-image box."""
    return {"jitter": False, "order": (0, 1, 2, 3), "brightness": 1.0, "contrast": 1.0, "saturation": 1.0, "hue": 0.0,
            "flip": False, "rotate": False, "cos": 1.0, "sin": 0.0, "box": (0, 0, int(W), int(H))}


def pack_params(entries: Sequence[Dict[str, object]]) -> torch.Tensor:
    """Entries (dicts like ``identity_entry``'s) -> the int32 [B, WORDS] table the kernels read."""
    f = torch.zeros(len(entries), WORDS, dtype=torch.float32)
    i = torch.zeros(len(entries), WORDS, dtype=torch.int32)
    for b, e in enumerate(entries):
        order = tuple(int(o) for o in e["order"])
        if sorted(order) != [0, 1, 2, 3]:
            raise ValueError(f"order {order} is not a permutation of the four operations")
        i[b, 0] = (FLAG_JITTER if e["jitter"] else 0) | (FLAG_FLIP if e["flip"] else 0) | (FLAG_ROTATE if e["rotate"] else 0)
        i[b, 1] = sum(o << (2 * k) for k, o in enumerate(order))
        f[b, 2], f[b, 3], f[b, 4], f[b, 5] = float(e["brightness"]), float(e["contrast"]), float(e["saturation"]), float(e["hue"])
        f[b, 6], f[b, 7] = float(e["cos"]), float(e["sin"])
        i[b, 8], i[b, 9], i[b, 10], i[b, 11] = (int(v) for v in e["box"])
    bits = f.view(torch.int32)
    i[:, 2:8] = bits[:, 2:8]
    return i


def unpack_params(params: torch.Tensor) -> List[Dict[str, object]]:
    """The inverse of ``pack_params`` (factors come back as the fp32 values the kernel sees)."""
    p = params.detach().cpu().to(torch.int32).contiguous()
    f = p.view(torch.float32)
    out = []
    for b in range(p.shape[0]):
        flags, order = int(p[b, 0]), int(p[b, 1])
        out.append({"jitter": bool(flags & FLAG_JITTER), "flip": bool(flags & FLAG_FLIP), "rotate": bool(flags & FLAG_ROTATE),
                    "order": tuple((order >> (2 * k)) & 3 for k in range(4)),
                    "brightness": float(f[b, 2]), "contrast": float(f[b, 3]), "saturation": float(f[b, 4]), "hue": float(f[b, 5]),
                    "cos": float(f[b, 6]), "sin": float(f[b, 7]), "box": tuple(int(v) for v in p[b, 8:12])})
    return out


def _crop_box(u: Sequence[float], H: int, W: int, scale, ratio) -> Tuple[int, int, int, int]:
    """torchvision RandomResizedCrop.get_params (albumentations mirrors it) on 40 uniforms: ten attempts of (area, log-ratio, x, y)."""
    area = H * W
    log_lo, log_hi = math.log(ratio[0]), math.log(ratio[1])
    for k in range(10):
        ua, ur, ux, uy = u[4 * k: 4 * k + 4]
        target = area * (scale[0] + (scale[1] - scale[0]) * ua)
        r = math.exp(log_lo + (log_hi - log_lo) * ur)
        w, h = int(round(math.sqrt(target * r))), int(round(math.sqrt(target / r)))
        if 0 < w <= W and 0 < h <= H:
            return min(int(ux * (W - w + 1)), W - w), min(int(uy * (H - h + 1)), H - h), w, h
    in_ratio = W / H  # the fallback: the centred crop clamped to the ratio range
    if in_ratio < ratio[0]:
        w, h = W, int(round(W / ratio[0]))
    elif in_ratio > ratio[1]:
        h, w = H, int(round(H * ratio[1]))
    else:
        w, h = W, H
    return (W - w) // 2, (H - h) // 2, w, h


def sample_params(B: int, H: int, W: int, out_hw, generator: torch.Generator, *, jitter_p: float = 0.8, crop_p: float = 0.5,
                  scale=(0.5, 1.0), ratio=(1.0, 1.0), rotateflip: bool = False) -> torch.Tensor:
    """The int32 [B, WORDS] parameter table of one batch: a pure function of ``generator``'s state, which it advances by B * 54 fp64
    uniforms.  Jitter factors as torchvision draws them (brightness, contrast, saturation from U[0.8, 1.2], hue from U[-0.2, 0.2], the
    four operations in a random order); flip and rotation (theta from U[-10, 10] degrees) each with probability 0.5 when ``rotateflip``;
    the resized crop with probability ``crop_p``, its box by ``_crop_box``.  Not applied means the full-image box, which only gives an
    ``out_hw`` result when ``out_hw`` is the image size."""
    Ho, Wo = (int(v) for v in out_hw)
    if H < 4 or W < 4:
        raise ValueError(f"augmentation needs H, W >= 4, got {H} x {W}")
    if crop_p < 1.0 and (Ho, Wo) != (H, W):
        raise ValueError(f"out_hw {Ho} x {Wo} differs from the image size {H} x {W}: an image whose crop is not applied keeps its size (crop_p < 1)")
    u = torch.rand(B, _DRAWS, generator=generator, dtype=torch.float64)
    entries = []
    for b in range(B):
        ub = u[b].tolist()
        e = identity_entry(H, W)
        e["jitter"] = ub[0] < jitter_p
        e["order"] = tuple(sorted(range(4), key=lambda k: ub[1 + k]))
        e["brightness"], e["contrast"], e["saturation"] = (0.8 + 0.4 * ub[5 + k] for k in range(3))
        e["hue"] = -0.2 + 0.4 * ub[8]
        if rotateflip:
            e["flip"] = ub[9] < 0.5
            if ub[10] < 0.5:
                theta = math.radians(-10.0 + 20.0 * ub[11])
                e["rotate"], e["cos"], e["sin"] = True, math.cos(theta), math.sin(theta)
        if ub[12] < crop_p:
            e["box"] = _crop_box(ub[14:], H, W, scale, ratio)
        entries.append(e)
    return pack_params(entries)


def _reflect101(i: torch.Tensor, n: int) -> torch.Tensor:
    period = 2 * (n - 1)
    m = torch.remainder(i, period)
    return torch.where(m > n - 1, period - m, m)


def index_map(params: torch.Tensor, H: int, W: int, out_hw) -> Tuple[torch.Tensor, torch.Tensor]:
    """(yy, xx) int64 [B, Ho, Wo]: output pixel (dy, dx) of image b is source pixel (yy, xx) of every input plane.  Crop, then rotation,
    then flip, each read backwards, i.e. flip, rotate, crop applied forwards.  The rotation is evaluated in fp32 like the kernel's (which
    fuses its multiply-adds: the two may differ where the source coordinate is within rounding of a half-integer)."""
    Ho, Wo = (int(v) for v in out_hw)
    dy = torch.arange(Ho, dtype=torch.int64).view(Ho, 1).expand(Ho, Wo)
    dx = torch.arange(Wo, dtype=torch.int64).view(1, Wo).expand(Ho, Wo)
    ys, xs = [], []
    for e in unpack_params(params):
        x0, y0, cw, ch = e["box"]
        cw, ch = min(max(cw, 1), W), min(max(ch, 1), H)
        x0, y0 = min(max(x0, 0), W - cw), min(max(y0, 0), H - ch)
        xx = x0 + (dx * cw) // Wo
        yy = y0 + (dy * ch) // Ho
        if e["rotate"]:
            c, s = torch.tensor(e["cos"], dtype=torch.float32), torch.tensor(e["sin"], dtype=torch.float32)
            cx, cy = torch.tensor(0.5 * (W - 1), dtype=torch.float32), torch.tensor(0.5 * (H - 1), dtype=torch.float32)
            uu, vv = xx.to(torch.float32) - cx, yy.to(torch.float32) - cy
            fx = c * uu + (cx - s * vv)
            fy = c * vv + (s * uu + cy)
            xx = _reflect101(torch.floor(fx + 0.5).to(torch.int64), W)
            yy = _reflect101(torch.floor(fy + 0.5).to(torch.int64), H)
        if e["flip"]:
            xx = W - 1 - xx
        ys.append(yy)
        xs.append(xx)
    return torch.stack(ys), torch.stack(xs)


def augment_batch(image: torch.Tensor, depth: torch.Tensor, snorm: Optional[torch.Tensor], params: torch.Tensor, out_hw, image_mean,
                  jitter: bool = True):
    """One batch through the two launches on the current stream: (image [B, 3, Ho, Wo] normalised, depth [B, 1, Ho, Wo], snorm
    [B, 3, Ho, Wo] or None), freshly allocated.  ``params``: the int32 table on the device.  ``jitter`` False skips the statistics
    launch and every image's jitter (whatever the table says)."""
    B = image.shape[0]
    Ho, Wo = (int(v) for v in out_hw)
    mean, std = mean_std(image_mean)
    dev = image.device
    out_image = torch.empty(B, 3, Ho, Wo, dtype=torch.float32, device=dev)
    out_depth = torch.empty(B, 1, Ho, Wo, dtype=torch.float32, device=dev)
    out_snorm = torch.empty(B, 3, Ho, Wo, dtype=torch.float32, device=dev) if snorm is not None else None
    partials = None
    if jitter:
        partials = ops.augment_partials(B, dev)
        ops.augment_stats(image, params, partials)
    ops.augment_apply(image, depth, snorm, params, partials, out_image, out_depth, out_snorm, mean, std)
    return out_image, out_depth, out_snorm


class _SamplerProxy:
    """``loader.sampler.set_epoch(ep)`` as mvp.train.train() calls it: the epoch reaches the augmentation's draws and the wrapped sampler."""

    def __init__(self, owner: "DeviceAugment"):
        self._owner = owner

    def set_epoch(self, epoch: int) -> None:
        self._owner.set_epoch(epoch)

    def __getattr__(self, name):
        return getattr(self._owner._inner_sampler(), name)


class DeviceAugment:
    """An iterable over device batch dicts (normally a DevicePrefetcher over a loader of raw samples: "image" uint8 [B, H, W, 3] or
    float32 [B, 3, H, W] in [0, 1], "depth" [B, 1, H, W], optionally "snorm" [B, 3, H, W]) that yields the reference's dict contract:
    "image" float32 [B, 3, Ho, Wo] normalised, "depth", "snorm" transformed with it, every other key passed on (device tensors copied).

    The draws of batch i of a pass are seeded by (seed, rank, epoch, i).  The epoch is ``set_epoch``'s, also reachable as
    ``.sampler.set_epoch`` like a loader's; without a call it advances by one per pass, so single-process training does not repeat the
    first epoch's draws.  The table goes up through a ring of pinned host buffers guarded by events: the host never waits for the compute
    stream, only (when the ring wraps) for an upload issued ``ring`` batches ago.  The launches go on the stream that is current when
    the batch is pulled.  Outputs are new tensors per batch and the inputs have been consumed (their kernels enqueued) by the time a
    batch is yielded, so there is no ``consumer_lag`` here: a look-ahead consumer may hold the batches as long as it likes, and the
    prefetcher underneath keeps its plain recycling rule.  ``augment=False``: normalisation only (identity maps, one launch), the
    validation path of loaders that hand out raw pixels."""

    def __init__(self, batches: Iterable[Dict[str, object]], *, image_mean="imagenet", out_hw=None, seed: int = 0, rank: int = 0,
                 augment: bool = True, rotateflip: bool = False, ring: int = 4):
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceAugment needs a HIP device (no CPU fallback on the product path)")
        mean_std(image_mean)
        self.batches, self.image_mean, self.out_hw = batches, image_mean, None if out_hw is None else tuple(int(v) for v in out_hw)
        self.seed, self.rank, self.augment, self.rotateflip = int(seed), int(rank), bool(augment), bool(rotateflip)
        self._epoch = 0
        self._ring = [None] * max(2, int(ring))  # (pinned table, event of its last upload)

    def __len__(self):
        return len(self.batches)

    def _inner_sampler(self):
        return getattr(self.batches, "sampler", None)

    @property
    def sampler(self):
        return _SamplerProxy(self)

    def set_epoch(self, epoch: int) -> None:
        self._epoch = int(epoch)
        inner = self._inner_sampler()
        if hasattr(inner, "set_epoch"):
            inner.set_epoch(int(epoch))

    def batch_generator(self, epoch: int, index: int) -> torch.Generator:
        """The generator whose state ``sample_params`` consumes for batch ``index`` of pass ``epoch``."""
        s = self.seed
        for v in (self.rank, int(epoch), int(index)):
            s = (s * 1_000_003 + v + 1) % (1 << 62)
        return torch.Generator().manual_seed(s)

    def params_for(self, epoch: int, index: int, B: int, H: int, W: int) -> torch.Tensor:
        if not self.augment:
            return pack_params([identity_entry(H, W)] * B)
        return sample_params(B, H, W, self.out_hw or (H, W), self.batch_generator(epoch, index), rotateflip=self.rotateflip)

    def _upload(self, index: int, table: torch.Tensor, device) -> torch.Tensor:
        slot = index % len(self._ring)
        held = self._ring[slot]
        if held is not None:
            held[1].synchronize()  # the upload issued len(ring) batches ago (long finished): never the compute of this batch
        if held is not None and held[0].shape[0] >= table.shape[0]:
            pinned = held[0]
        else:
            pinned = torch.empty(table.shape, dtype=torch.int32).pin_memory()
        pinned[: table.shape[0]].copy_(table)
        dev = torch.empty(table.shape, dtype=torch.int32, device=device)
        dev.copy_(pinned[: table.shape[0]], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._ring[slot] = (pinned, ev)
        return dev

    def __iter__(self) -> Iterator[Dict[str, object]]:
        epoch = self._epoch
        self._epoch = epoch + 1
        side = getattr(self.batches, "stream", None)
        if side is not None:
            # one prefetcher serves every pass: its first copies of this pass reuse the buffers the last launches of the previous pass read
            side.wait_stream(torch.cuda.current_stream())
        for index, batch in enumerate(self.batches):
            image, depth, snorm = batch["image"], batch["depth"], batch.get("snorm")
            if not image.is_cuda:
                raise RuntimeError("DeviceAugment takes device batches: wrap the loader in mvp.prefetch.DevicePrefetcher")
            B = image.shape[0]
            H, W = (image.shape[1], image.shape[2]) if image.dtype == torch.uint8 else (image.shape[2], image.shape[3])
            table = self._upload(index, self.params_for(epoch, index, B, H, W), image.device)
            o_image, o_depth, o_snorm = augment_batch(image, depth, snorm, table, self.out_hw or (H, W), self.image_mean, jitter=self.augment)
            out = {}
            for k, v in batch.items():
                if k in ("image", "depth", "snorm"):
                    continue
                # whatever else rides along (validation's segmentation) is copied: the prefetcher underneath recycles its buffers
                out[k] = v.clone() if torch.is_tensor(v) and v.is_cuda else v
            out["image"], out["depth"] = o_image, o_depth
            if o_snorm is not None:
                out["snorm"] = o_snorm
            yield out
