#!/usr/bin/env python3
"""Device-side timing of mvp_pixel_score (csrc/pixelsim.hip) and the throughput of the 2AFC evaluation loop with the pixel baselines.

    python tools/pixelsim_bench.py [--reps 20] [--inner 10] [--warmup 3] [--triplets 64] [--skip-loop] [--out profiles/pixelsim_bench.txt]

Part 1, per metric and shape (B, C, H, W) — 16 triplets of 3 x 224^2 and of 3 x 512^2 — three things are timed ALTERNATING with device
events, each window holding ``inner`` back-to-back calls: the ABI call (two launches), a device copy_ of the same 3 B C H W 4 bytes
(which reads AND writes them: twice the traffic), and the same scores written with torch ops on the device (SSIM: the reference's
_ssim, five depthwise 11 x 11 conv2d per pair in fp32; PSNR: two mean-squared differences and log10).  Reported per call: median
(min - max) over the windows, and the op's bytes read over its median — a whole-call rate, launches included.  The operand (29 MB /
151 MB) is written once before the loop and stays in the 256 MB last-level cache between calls: the rates are cache rates and are not
put against the HBM peak; the copy_ beside it is the yardstick.  The SSIM kernel is bound by its fp64 arithmetic and LDS reads, not by
the bytes.

Part 2: triplets/s of mvp.percept.predict_batch(SSIM() | PSNR()) on SyntheticTwoAFC(preprocess="SSIM") at 224^2 against the same loop
written with the torch ops above and per-item .item() (the shape of the reference's loop), each timed by a host clock around a run
that ends in a device synchronise, after one warm-up run of each.  Needs a GPU; there is no CPU fallback."""
import argparse
import os
import sys
import time

import torch
import torch.nn.functional as F

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


def torch_scores(r, x, metric, window):
    """The score of each pair [B] with torch ops in fp32, as the reference evaluates it."""
    if metric == "psnr":
        return 10.0 * torch.log10(1.0 / ((r - x) ** 2).flatten(1).mean(dim=1))
    ch = r.shape[1]

    def filt(t):
        return F.conv2d(t, window, padding=5, groups=ch)

    mu1, mu2 = filt(r), filt(x)
    s1, s2, s12 = filt(r * r) - mu1 * mu1, filt(x * x) - mu2 * mu2, filt(r * x) - mu1 * mu2
    m = ((2 * mu1 * mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1 * mu1 + mu2 * mu2 + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    return m.mean(1).mean(1).mean(1)


def kernel_part(a, dev, lines):
    from evals.utils.losses import create_window
    from mvp import ops, percept

    fmt = lambda t: f"{t[0] * 1e3:8.1f} ({t[1] * 1e3:8.1f} - {t[2] * 1e3:8.1f}) us"  # noqa: E731
    window = create_window(11, 3).to(dev)
    for H in (224, 512):
        B, C, W = 16, 3, H
        ds = percept.SyntheticTwoAFC(B, image_size=H, seed=0, preprocess="SSIM")
        stacked = torch.cat([torch.stack([ds[i][k] for i in range(B)]) for k in range(3)]).to(dev)  # [3B, 3, H, W]: ref | left | right
        r, le, ri = stacked[:B], stacked[B:2 * B], stacked[2 * B:]
        label = torch.tensor([float(ds[i][3]) for i in range(B)]).to(dev)
        sim = torch.empty(B, 2, dtype=torch.float32, device=dev)
        pred = torch.empty(B, dtype=torch.int32, device=dev)
        counts = torch.zeros(4, dtype=torch.int64, device=dev)
        dst = torch.empty_like(stacked)
        nbytes = stacked.numel() * 4
        lines.append(f"(B, C, H, W) = ({B}, {C}, {H}, {W}): {nbytes / 1e6:.2f} MB read")
        for metric in ("ssim", "psnr"):
            ws = torch.empty(max(1, ops.pixel_score_workspace_bytes(B, C, H, W, metric) // 8), dtype=torch.float64, device=dev)

            def hip():
                ops.pixel_score(r, le, ri, sim, pred, ws, B, C, H, W, C * H * W, metric, label=label, counts=counts, accumulate=True)

            def copy():
                dst.copy_(stacked)

            def plain():
                sl, sr = torch_scores(r, le, metric, window), torch_scores(r, ri, metric, window)
                return sl, sr, torch.where(sl > sr, 0, 1)

            th, tc, tt = timed_alternating([hip, copy, plain], a.reps, a.inner, a.warmup)
            sl, sr, pp = plain()
            diff = float(torch.maximum((sim[:, 0] - sl).abs().max(), (sim[:, 1] - sr).abs().max()))
            lines.append(f"  {metric}")
            lines.append(f"    mvp_pixel_score   {fmt(th)}   {nbytes / (th[0] * 1e-3) / 1e9:8.1f} GB/s read (whole call, two launches)")
            lines.append(f"    copy_, same bytes {fmt(tc)}   {2 * nbytes / (tc[0] * 1e-3) / 1e9:8.1f} GB/s read + written")
            lines.append(f"    torch ops         {fmt(tt)}   op / torch = {th[0] / tt[0]:.3f};  max |sim - torch's| = {diff:.2e}, "
                         f"predictions equal: {bool((pred == pp).all())}")


def reference_loop(metric, batches, dev, window):
    """The shape of evaluate_model_percepture.py:91-133 with the metric in place of the embedding: torch ops, per-item .item()."""
    results = []
    for img_ref, img_left, img_right, p, ids in batches:
        img_ref, img_left, img_right, p = img_ref.to(dev), img_left.to(dev), img_right.to(dev), p.to(dev)
        sl, sr = torch_scores(img_ref, img_left, metric, window), torch_scores(img_ref, img_right, metric, window)
        predictions = torch.where(sl > sr, 0, 1)
        for i in range(len(ids)):
            results.append({"id": ids[i].item(), "gt": p[i].item(), "prediction": predictions[i].item()})
    return results


def loop_part(a, dev, lines):
    from evals.utils.losses import create_window
    from mvp import config, percept

    window = create_window(11, 3).to(dev)
    for metric in ("ssim", "psnr"):
        cfg = config.compose("model_percepture", [f"backbone={metric}", f"dataset.preprocess={metric.upper()}"])
        model = config.instantiate(cfg["backbone"]).to(dev).eval()
        ds = percept.SyntheticTwoAFC(a.triplets, image_size=224, seed=0, preprocess=metric.upper())
        batches = list(torch.utils.data.DataLoader(ds, int(cfg["batch_size"]), shuffle=False))
        times = {}
        for name, fn in (("predict_batch", lambda: percept.predict_batch(model, batches, None)[0]),
                         ("torch loop", lambda: reference_loop(metric, batches, dev, window))):
            fn()  # warm-up: code objects, pinned buffers, conv algorithms
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.loop_reps):
                out = fn()
            torch.cuda.synchronize()
            times[name] = (time.perf_counter() - t0) / a.loop_reps
            times[name + " preds"] = [r["prediction"] for r in out]
        same = times["predict_batch preds"] == times["torch loop preds"]
        lines.append(f"{metric}: {a.triplets} triplets at 224^2, batches of {cfg['batch_size']}, {a.loop_reps} runs each: predict_batch "
                     f"{a.triplets / times['predict_batch']:8.1f} triplets/s, torch-op loop {a.triplets / times['torch loop']:8.1f} triplets/s "
                     f"(x {times['torch loop'] / times['predict_batch']:.2f}); predictions equal: {same}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--triplets", type=int, default=64)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pixelsim_bench needs a GPU")
    dev = torch.device("cuda:0")
    lines = [f"mvp_pixel_score: {a.reps} windows of {a.inner} calls each after {a.warmup} warm-up windows, alternating; device events, per call: "
             "median (min - max); operands resident in the last-level cache"]
    kernel_part(a, dev, lines)
    if not a.skip_loop:
        loop_part(a, dev, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
