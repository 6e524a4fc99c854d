#!/usr/bin/env python3
"""Device-side timing of the training augmentation (csrc/augment.hip: mvp_augment_stats + mvp_augment_apply).

    python tools/augment_bench.py [--reps 20] [--inner 10] [--warmup 3] [--out profiles/augment_bench.txt]

At B = 16, 224^2 and 480 x 640, uint8 NHWC and fp32 NCHW inputs, image + depth + normals, a table drawn by sample_params (jitter on
80 % of the images, crops on half, rotateflip on so that every path runs).  Four things are timed ALTERNATING with device events, each
window holding ``inner`` back-to-back calls: the statistics launch, the apply launch, a device copy_ that reads and writes as many bytes
as the two launches read and write together, and the same stage written with torch ops on the device (uint8 -> float, the four jitter
operations batched with per-image factors in ONE fixed order, a gather by a precomputed index, Normalize) — which does less (no per-image
order, the index map comes ready-made) and still launches some sixty kernels.  Reported per call: median (min - max) over the windows.
The apply launch is timed three more times on tables with the jitter, the geometry or both switched off, to say where its time goes.
Residency is stated per shape: the operands are written once before the loop and are re-read by every call, so whatever fits the
256 MB last-level cache is served from it (as a batch that the H2D copy has just written is); rates are whole-call rates and are put
beside the copy_, not against the HBM peak.  Needs a GPU; there is no CPU fallback."""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "midvision-probe_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed_alternating(fns, reps, inner, warmup):
    """[(median, min, max) ms per call] per function; window i of every function is taken before window i + 1 of any."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / inner)
    return [(sorted(m)[len(m) // 2], min(m), max(m)) for m in ms]


def torch_stage(image, depth, snorm, fac, on, idx, mean, std):
    """The stage with torch ops: fac [B, 4, 1, 1, 1] (brightness, contrast, saturation, hue), on [B, 1, 1, 1] bool, idx [B, 1, Ho * Wo]."""
    x = image.permute(0, 3, 1, 2).float() / 255 if image.dtype == torch.uint8 else image
    grey = lambda t: (0.2989 * t[:, 0] + 0.587 * t[:, 1] + 0.114 * t[:, 2]).unsqueeze(1)  # noqa: E731
    y = (fac[:, 0] * x).clamp(0, 1)
    y = (fac[:, 1] * y + (1 - fac[:, 1]) * grey(y).mean(dim=(1, 2, 3), keepdim=True)).clamp(0, 1)
    y = (fac[:, 2] * y + (1 - fac[:, 2]) * grey(y)).clamp(0, 1)
    r, g, b = y.unbind(1)
    maxc, minc = y.max(1).values, y.min(1).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    div = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    h = (maxc == r) * (bc - gc) + ((maxc == g) & (maxc != r)) * (2.0 + rc - bc) + ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod(h / 6.0 + 1.0, 1.0)
    h = torch.remainder(h + fac[:, 3, 0], 1.0)
    i = torch.floor(h * 6.0)
    f = h * 6.0 - i
    i = i.to(torch.int32) % 6
    p_, q_, t_ = (maxc * (1 - s)).clamp(0, 1), (maxc * (1 - s * f)).clamp(0, 1), (maxc * (1 - s * (1 - f))).clamp(0, 1)
    sel = lambda *c: torch.stack(c, 1).gather(1, i.long().unsqueeze(1)).squeeze(1)  # noqa: E731
    y = torch.stack((sel(maxc, q_, p_, p_, t_, maxc), sel(t_, maxc, maxc, q_, p_, p_), sel(p_, p_, t_, maxc, maxc, q_)), 1)
    x = torch.where(on, y, x)
    B, Ho, Wo = image.shape[0], depth.shape[-2], depth.shape[-1]
    take = lambda t: t.flatten(2).gather(2, idx.expand(-1, t.shape[1], -1)).view(B, t.shape[1], Ho, Wo)  # noqa: E731
    return (take(x) - mean) / std, take(depth), take(snorm)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs a GPU")
    from mvp import augment, ops

    dev = torch.device("cuda:0")
    B = 16
    fmt = lambda t: f"{t[0] * 1e3:8.1f} ({t[1] * 1e3:8.1f} - {t[2] * 1e3:8.1f}) us"  # noqa: E731
    lines = [f"augmentation stage at B = {B}: {a.reps} windows of {a.inner} calls each after {a.warmup} warm-up windows, alternating; device "
             "events, per call: median (min - max)"]
    mean, std = augment.mean_std("imagenet")
    mean_t, std_t = torch.tensor(mean, device=dev).view(1, 3, 1, 1), torch.tensor(std, device=dev).view(1, 3, 1, 1)
    for H, W in ((224, 224), (480, 640)):
        for form in ("uint8 NHWC", "fp32 NCHW"):
            g = torch.Generator().manual_seed(H)
            u8 = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
            image = (u8 if form.startswith("uint8") else (u8.permute(0, 3, 1, 2).float() / 255).contiguous()).to(dev)
            depth = torch.rand(B, 1, H, W, generator=g).to(dev)
            snorm = torch.randn(B, 3, H, W, generator=g).to(dev)
            table = augment.sample_params(B, H, W, (H, W), torch.Generator().manual_seed(1), rotateflip=True)
            params = table.to(dev)
            es = augment.unpack_params(table)
            partials = ops.augment_partials(B, dev)
            out_image = torch.empty(B, 3, H, W, device=dev)
            out_depth = torch.empty(B, 1, H, W, device=dev)
            out_snorm = torch.empty(B, 3, H, W, device=dev)
            n_on = sum(e["jitter"] for e in es)
            src = image.numel() * image.element_size()
            moved = n_on * src // B + src + (depth.numel() + snorm.numel()) * 4 + (out_image.numel() + out_depth.numel() + out_snorm.numel()) * 4
            half = torch.empty(moved // 8, dtype=torch.float32, device=dev)  # copy_ reads moved / 2 and writes moved / 2
            half_dst = torch.empty_like(half)
            fac = torch.tensor([[e["brightness"], e["contrast"], e["saturation"], e["hue"]] for e in es], device=dev).view(B, 4, 1, 1, 1)
            on = torch.tensor([e["jitter"] for e in es], device=dev).view(B, 1, 1, 1)
            yy, xx = augment.index_map(table, H, W, (H, W))
            idx = (yy * W + xx).view(B, 1, H * W).to(dev)

            def stats():
                ops.augment_stats(image, params, partials)

            def apply():
                ops.augment_apply(image, depth, snorm, params, partials, out_image, out_depth, out_snorm, mean, std)

            def copy():
                half_dst.copy_(half)

            def plain():
                return torch_stage(image, depth, snorm, fac, on, idx, mean_t, std_t)

            ts, ta, tc, tt = timed_alternating([stats, apply, copy, plain], a.reps, a.inner, a.warmup)
            # what the apply launch spends where: the same launch on tables with parts of the work switched off
            ident = augment.identity_entry(H, W)
            geo_keys = ("flip", "rotate", "cos", "sin", "box")
            variants = {"identity table (normalise only)": [ident] * B,
                        "jitter only": [dict(e, **{k: ident[k] for k in geo_keys}) for e in es],
                        "geometry only": [dict(e, jitter=False) for e in es]}
            vtabs = {k: augment.pack_params(v).to(dev) for k, v in variants.items()}

            def apply_with(tab):
                return lambda: ops.augment_apply(image, depth, snorm, tab, partials, out_image, out_depth, out_snorm, mean, std)

            tv = timed_alternating([apply_with(t) for t in vtabs.values()], a.reps, a.inner, a.warmup)
            resident = (moved + idx.numel() * 8) / 2 ** 20
            lines.append(f"{H} x {W}, {form}: {n_on} of {B} images jittered, {sum(e['rotate'] for e in es)} rotated, {sum(e['flip'] for e in es)} flipped, "
                         f"{sum(e['box'] != (0, 0, W, H) for e in es)} cropped; {moved / 1e6:.1f} MB read + written by the two launches; working set "
                         f"{resident:.0f} MiB ({'inside' if resident < 256 else 'LARGER than'} the 256 MiB last-level cache)")
            lines.append(f"    mvp_augment_stats {fmt(ts)}   {n_on * src / B / (ts[0] * 1e-3) / 1e9:8.1f} GB/s read")
            lines.append(f"    mvp_augment_apply {fmt(ta)}   {(moved - n_on * src // B) / (ta[0] * 1e-3) / 1e9:8.1f} GB/s read + written")
            for name, t in zip(vtabs, tv):
                lines.append(f"      apply, {name:32s} {fmt(t)}")
            lines.append(f"    copy_, same bytes {fmt(tc)}   {moved / (tc[0] * 1e-3) / 1e9:8.1f} GB/s read + written")
            lines.append(f"    torch ops         {fmt(tt)}   (stats + apply) / torch = {(ts[0] + ta[0]) / tt[0]:.3f};  (stats + apply) / copy_ = "
                         f"{(ts[0] + ta[0]) / tc[0]:.2f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
