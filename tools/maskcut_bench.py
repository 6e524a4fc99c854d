#!/usr/bin/env python3
"""Device-side timing of the four MaskCut launches (csrc/maskcut.hip) and of the whole pass loop, against a reference-style loop.

    python tools/maskcut_bench.py [--reps 10] [--warmup 2] [--images 16] [--budget-seconds 240] [--out profiles/maskcut_bench.txt]

Workload: the evaluation's own size, N = 900 cells (480^2 at patch 16), C = 768, a batch of 16 images with two objects each (seeded
prototype + noise features, so that the solver has real work: about 30 rounds per solve).  Part 1 times each launch of the first pass
ALTERNATING with device events: median (min - max) over the windows, one call per window (a call is 0.1 - 10 ms).  Part 2 times the
whole loop (both passes: mvp.maskcut.maskcut_batch, the transfer of the converged bytes, the host solves of images that did not
converge; ending in a device synchronise) by a host clock against a loop in the reference's
style on the same features: per image and pass a torch affinity on the device, the copy of A to the host, Lloyd's iteration in numpy
(the same rule; the reference runs sklearn's KMeans there), torch.linalg.eigh on S in fp64 on the host, and this library's
partition launch.  The two loops' unions are compared.  Every part stops taking windows once the budget is used up (at least one window
each).  Needs a GPU; there is no CPU fallback."""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "midvision-probe_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def make_feats(B, C, h, w, seed=0, noise=1.0):
    """[B, C, h*w] fp32: background + two rectangles, prototype[label] + noise / sqrt(C) per channel."""
    g = torch.Generator().manual_seed(seed)
    lab = torch.zeros(B, h, w, dtype=torch.long)
    for b in range(B):
        y0, x0 = 4 + b % 5, 3 + b % 4
        lab[b, y0:y0 + 12, x0:x0 + 8] = 1
        lab[b, y0 + 3:y0 + 14, x0 + 13:x0 + 21] = 2
    proto = F.normalize(torch.randn(3, C, generator=g), dim=1)
    f = proto[lab.reshape(B, -1)].transpose(1, 2) + noise * torch.randn(B, C, h * w, generator=g) / C ** 0.5
    return f.contiguous()


class Budget:
    def __init__(self, seconds):
        self.t0, self.seconds = time.perf_counter(), seconds

    def left(self):
        return time.perf_counter() - self.t0 < self.seconds


def timed_alternating(fns, reps, warmup, budget):
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for r in range(reps):
        if r and not budget.left():
            break
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return [(sorted(m)[len(m) // 2], min(m), max(m), len(m)) for m in ms]


def lloyd(a, max_rounds=64):
    a = a.reshape(-1).astype(np.float64)
    mean = a.mean()
    sd = np.sqrt(max((a * a).mean() - mean * mean, 0.0))
    c0, c1, prev = mean - sd, mean + sd, -1
    for _ in range(max_rounds):
        up = a > 0.5 * (c0 + c1)
        cnt = int(up.sum())
        if cnt == 0 or cnt == a.size:
            break
        c1, c0 = a[up].sum() / cnt, a[~up].sum() / (a.size - cnt)
        if cnt == prev:
            break
        prev = cnt
    return 0.5 * (c0 + c1)


def reference_loop(feats, h, w, passes, buf):
    """The reference's per-image, per-object loop (maskcut_processor.py:215-296) with host-side threshold and eigen-solve."""
    from mvp import maskcut

    B, C, N = feats.shape
    buf.painted.zero_()
    buf.mask.zero_()
    one = torch.zeros(B, dtype=torch.uint8, device=feats.device)
    for b in range(B):
        one.zero_()
        one[b] = 1
        for p in range(passes):
            f = F.normalize(feats[b] * (1 - buf.painted[b].float()), p=2, dim=0)
            A = (f.transpose(0, 1) @ f).cpu().numpy()  # the reference's device-to-host copy
            tau = lloyd(A)
            Bm = torch.from_numpy((A > tau).astype(np.float64))
            W = Bm + maskcut.EPS * (1 - Bm)
            s = W.sum(dim=1).rsqrt()
            _, U = torch.linalg.eigh(W * s[:, None] * s[None, :])
            v = U[:, -2] * s
            k = int(torch.argmax(v.abs()))
            buf.v[b].copy_((-v if v[k] < 0 else v).float())
            maskcut.partition(buf, h, w, use_prev=p >= 1, active=one)
    torch.cuda.synchronize()
    return buf.union.clone()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--budget-seconds", type=float, default=240.0)
    ap.add_argument("--noise", type=float, nargs="+", default=[2.5, 1.0],
                    help="feature noise levels: 2.5 gives connected graphs (lambda_2 ~ 0.05, ~30 solver rounds), 1.0 cleanly separated "
                         "components (lambda_2 ~ lambda_3: the solver runs to its cap and the host solves the image)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("maskcut_bench needs a GPU")
    dev = torch.device("cuda:0")
    lines = []
    for noise in a.noise:
        bench_one(a, dev, noise, Budget(a.budget_seconds / len(a.noise)), lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


def whole_loop(feats, h, w, nobj, buf):
    """maskcut_batch, the one transfer of the converged bytes, and the host solves of the images that did not converge."""
    from mvp import maskcut

    buf, conv, _ = maskcut.maskcut_batch(feats, h, w, nobj, buf=buf)
    n_fallback = maskcut.finish_fallbacks(feats, h, w, nobj, buf, conv.cpu())
    return buf.union.clone(), n_fallback


def bench_one(a, dev, noise, budget, lines):
    from mvp import maskcut

    B, C, h, w = a.images, 768, 30, 30
    N = h * w
    feats = make_feats(B, C, h, w, noise=noise).to(dev)
    buf = maskcut._Buffers(B, N, dev)
    conv = torch.ones(B, dtype=torch.uint8, device=dev)
    fns = [lambda: maskcut.affinity(feats, buf), lambda: maskcut.threshold(buf), lambda: maskcut.fiedler(buf, conv),
           lambda: maskcut.partition(buf, h, w, use_prev=False)]
    names = ["mvp_ncut_affinity", "mvp_ncut_threshold", "mvp_ncut_fiedler", "mvp_ncut_partition"]
    t = timed_alternating(fns, a.reps, a.warmup, budget)
    lines.append(f"feature noise {noise}: MaskCut launches at N = {N}, C = {C}, Bimg = {B} (first pass; device events, one call per window, "
                 "alternating): median (min - max) ms, windows")
    for n, (med, lo, hi, cnt) in zip(names, t):
        lines.append(f"    {n:20s} {med:9.3f} ({lo:9.3f} - {hi:9.3f}) ms  {cnt} windows")
    lines.append(f"    solver rounds per image: {buf.iters.cpu().tolist()}  converged: {conv.cpu().tolist()}  "
                 f"Lloyd rounds: {buf.rounds.cpu().tolist()}")
    lines.append(f"    affinity: {2.0 * B * N * N * C / (t[0][0] * 1e-3) / 1e12:.2f} TFLOP/s (fp32-input MFMA, whole call: norms, Gram, sums)")
    nobj = [2] * B
    times = {}
    unions = {}
    fallbacks = []

    def ours():
        union, nf = whole_loop(feats, h, w, nobj, buf)
        fallbacks.append(nf)
        return union

    for name, fn in (("maskcut_batch", ours), ("reference-style loop", lambda: reference_loop(feats, h, w, 2, buf))):
        fn()  # warm-up
        torch.cuda.synchronize()
        runs = []
        for r in range(a.loop_reps):
            if r and not budget.left():
                break
            t0 = time.perf_counter()
            unions[name] = fn()
            torch.cuda.synchronize()
            runs.append(time.perf_counter() - t0)
        times[name] = (sorted(runs)[len(runs) // 2], min(runs), max(runs), len(runs))
    same = int((unions["maskcut_batch"] == unions["reference-style loop"]).all(dim=1).sum())
    for name in times:
        med, lo, hi, cnt = times[name]
        lines.append(f"{name}: {B} images, two passes each: {med * 1e3:9.1f} ({lo * 1e3:9.1f} - {hi * 1e3:9.1f}) ms per batch over {cnt} runs, "
                     f"{B / med:8.1f} images/s (host clock, ends in a device synchronise)")
    lines.append(f"ratio reference-style / maskcut_batch = {times['reference-style loop'][0] / times['maskcut_batch'][0]:.1f}; "
                 f"images with equal unions: {same} of {B}; host solves per batch (n_fallback): {fallbacks[-1]} of {2 * B}")


if __name__ == "__main__":
    main()
