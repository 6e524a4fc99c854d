#!/usr/bin/env python3
"""Device-side timing of mvp_twoafc_score (csrc/twoafc.hip) and the throughput of the 2AFC evaluation loop around it.

    python tools/twoafc_bench.py [--reps 20] [--inner 20] [--warmup 3] [--triplets 64] [--skip-loop] [--out profiles/twoafc_bench.txt]

Part 1, per shape (B, C, HW) — (16, 2048, 225): a ResNet-50 tail at 480^2; (16, 768, 1): ViT-B class tokens — three things are timed
ALTERNATING with device events, each window holding ``inner`` back-to-back calls (a single call is too short for an event pair):
the ABI call (two launches), a device copy_ of the same 3 B C HW 4 bytes (which reads AND writes them: twice the traffic), and the
reference's torch composition (three adaptive_avg_pool2d for HW > 1, two F.cosine_similarity, torch.where).  Reported per call: median
(min - max) over the windows, and the score call's bytes read over its median — a whole-call rate, launches included.  The operand
is written once before the loop and, at 88 MB, stays in the 256 MB last-level cache between calls (as a forward's output does when the
score op follows it): the rates are cache rates and are not put against the HBM peak; the copy_ beside it is the yardstick.

Part 2: triplets/s of mvp.percept.predict_batch against the same loop written with the reference's torch ops (three forwards, pool,
F.cosine_similarity, per-item .item()), on the same wrapper and the same in-memory batches, each loop timed by a host clock around a
run that ends in a device synchronise, after one warm-up run of each.  Needs a GPU; there is no CPU fallback."""
import argparse
import os
import sys
import time
import warnings

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


def kernel_part(a, dev, lines):
    from mvp import ops

    fmt = lambda t: f"{t[0] * 1e3:8.1f} ({t[1] * 1e3:8.1f} - {t[2] * 1e3:8.1f}) us"  # noqa: E731
    for B, C, HW in [(16, 2048, 225), (16, 768, 1)]:
        g = torch.Generator().manual_seed(C)
        stacked = torch.randn(3 * B, C, HW, generator=g).to(dev)
        r, le, ri = stacked[:B], stacked[B:2 * B], stacked[2 * B:]
        label = torch.randint(0, 2, (B,), generator=g).float().to(dev)
        sim = torch.empty(B, 2, dtype=torch.float32, device=dev)
        pred = torch.empty(B, dtype=torch.int32, device=dev)
        counts = torch.zeros(4, dtype=torch.int64, device=dev)
        ws = torch.empty(max(1, ops.twoafc_workspace_bytes(B, C, HW) // 8), dtype=torch.float64, device=dev)
        dst = torch.empty_like(stacked)

        def hip():
            ops.twoafc_score(r, le, ri, sim, pred, ws, B, C, HW, C * HW, label=label, counts=counts, accumulate=True)

        def copy():
            dst.copy_(stacked)

        def plain():
            f = [t.mean(dim=2) if HW > 1 else t[:, :, 0] for t in (r, le, ri)]
            sl, sr = F.cosine_similarity(f[0], f[1], dim=-1), F.cosine_similarity(f[0], f[2], dim=-1)
            return sl, sr, torch.where(sl > sr, 0, 1)

        th, tc, tt = timed_alternating([hip, copy, plain], a.reps, a.inner, a.warmup)
        sl, sr, pp = plain()
        diff = float(torch.maximum((sim[:, 0] - sl).abs().max(), (sim[:, 1] - sr).abs().max()))
        nbytes = stacked.numel() * 4
        lines.append(f"(B, C, HW) = ({B}, {C}, {HW}): {nbytes / 1e6:.2f} MB read")
        lines.append(f"    mvp_twoafc_score {fmt(th)}   {nbytes / (th[0] * 1e-3) / 1e9:8.1f} GB/s read (whole call, two launches)")
        lines.append(f"    copy_, same bytes {fmt(tc)}   {2 * nbytes / (tc[0] * 1e-3) / 1e9:8.1f} GB/s read + written")
        lines.append(f"    torch ops         {fmt(tt)}   score / torch = {th[0] / tt[0]:.2f};  max |sim - torch's| = {diff:.2e}, "
                     f"predictions equal: {bool((pred == pp).all())}")


def reference_loop(model, batches, dev):
    """evaluate_model_percepture.py:91-133 with the reference's torch ops on this wrapper."""
    results = []
    for img_ref, img_left, img_right, p, ids in batches:
        img_ref, img_left, img_right, p = img_ref.to(dev), img_left.to(dev), img_right.to(dev), p.to(dev)
        with torch.no_grad():
            if model.arch == "vit":
                fr, fl, fq = model(img_ref), model(img_left), model(img_right)
            else:
                fr, fl, fq = (F.adaptive_avg_pool2d(model(x), 1).flatten(1) for x in (img_ref, img_left, img_right))
        sl, sr = F.cosine_similarity(fr, fl, dim=-1), F.cosine_similarity(fr, fq, dim=-1)
        predictions = torch.where(sl > sr, 0, 1)
        for i in range(len(ids)):
            results.append({"id": ids[i].item(), "gt": p[i].item(), "prediction": predictions[i].item()})
    return results


def loop_part(a, dev, lines):
    from mvp import config, percept

    for backbone in ("dinov2_b14", "dino_resnet50"):
        cfg = config.compose("model_percepture", [f"backbone={backbone}", "backbone.return_cls=True"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model = config.instantiate(cfg["backbone"]).to(dev).eval()
        ds = percept.SyntheticTwoAFC(a.triplets, image_size=224, seed=0)
        batches = list(torch.utils.data.DataLoader(ds, int(cfg["batch_size"]), shuffle=False))
        times = {}
        for name, fn in (("predict_batch", lambda: percept.predict_batch(model, batches, None)[0]),
                         ("reference loop", lambda: reference_loop(model, batches, dev))):
            fn()  # warm-up: engine tables, code objects, pinned buffers
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.loop_reps):
                out = fn()
            torch.cuda.synchronize()
            times[name] = (time.perf_counter() - t0) / a.loop_reps
            times[name + " preds"] = [r["prediction"] for r in out]
        same = times["predict_batch preds"] == times["reference loop preds"]
        lines.append(f"{backbone}: {a.triplets} triplets at 224^2, batches of {cfg['batch_size']}, {a.loop_reps} runs each: predict_batch "
                     f"{a.triplets / times['predict_batch']:8.1f} triplets/s, reference-style loop {a.triplets / times['reference loop']:8.1f} triplets/s "
                     f"(x {times['reference loop'] / times['predict_batch']:.2f}); predictions equal: {same}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--triplets", type=int, default=64)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("twoafc_bench needs a GPU")
    dev = torch.device("cuda:0")
    lines = [f"mvp_twoafc_score: {a.reps} windows of {a.inner} calls each after {a.warmup} warm-up windows, alternating; device events, per call: "
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
