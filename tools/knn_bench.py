#!/usr/bin/env python3
"""Device-side timing of mvp_knn_ratio (csrc/knn.hip) at the NAVI workload's shapes — N0 = N1 = 16 384 (a 128 x 128 grid), C = 768
and C = 3 072 (multilayer) — beside the plain torch alternative in the same process: fp32 normalize -> q @ t.T -> topk(2).

    python tools/knn_bench.py [--n 16384] [--c 768 3072] [--reps 20] [--warmup 3] [--out profiles/knn_bench.txt]

Per shape: median / min / max over ``--reps`` calls timed with device events (the whole ABI call: count + 2 packs + candidates +
refine), the matrix-pipe work the algorithm issues (2 fp16 MFMA products of 2 N0 N1 Cpad FLOP each) over the median as a share of
the 2.5 PFLOP/s fp16 peak — a whole-call rate, not a kernel's —, and how far the results agree with the torch path (same index; the
torch path's distances are its own fp32 matmul).  Needs a GPU; there is no CPU fallback."""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "midvision-probe_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_F16 = 2.5e15  # dense fp16 / bf16 MFMA, FLOP/s (spec)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--c", type=int, nargs="+", default=[768, 3072])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench needs a GPU")
    from mvp import corr3d

    dev = torch.device("cuda:0")
    lines = [f"mvp_knn_ratio vs torch (normalize, matmul, topk 2); N0 = N1 = {a.n}; {a.reps} timed calls after {a.warmup}; device events, ms"]
    for C in a.c:
        g = torch.Generator(device="cpu").manual_seed(C)
        # a smooth map plus noise, like an upsampled feature map: low-resolution random field, bicubic x4
        side = int(round(a.n ** 0.5))
        low0, low1 = torch.randn(C, side // 4, side // 4, generator=g), torch.randn(C, side // 4, side // 4, generator=g)
        up = lambda x: torch.nn.functional.interpolate(x[None].to(dev), size=(side, side), mode="bicubic")[0].reshape(C, -1)[:, :a.n].contiguous()  # noqa: E731
        f0, f1 = up(low0), up(low1)
        N = f0.shape[1]

        def hip():
            return corr3d.knn_ratio(f0, f1)

        def plain():
            q = torch.nn.functional.normalize(f0.t(), dim=-1)
            t = torch.nn.functional.normalize(f1.t(), dim=-1)
            s, i = torch.topk(q @ t.t(), 2, dim=1, largest=True)
            d = 1 - s
            return i[:, 0], d, 1 - d[:, 0].clamp(min=1e-9) / d[:, 1].clamp(min=1e-9)

        th = timed(hip, a.reps, a.warmup)
        tt = timed(plain, a.reps, a.warmup)
        nn, dist, w, _ = hip()
        ti, td, tw = plain()
        same = float((nn.long() == ti).double().mean())
        Cpad = -(-C // 32) * 32
        flop = 2 * 2.0 * N * N * Cpad
        lines.append(f"C={C:5d}  hip   median {th[0]:8.3f}  min {th[1]:8.3f}  max {th[2]:8.3f}   matrix-pipe work {flop / 1e12:.2f} TFLOP -> "
                     f"{flop / (th[0] * 1e-3) / 1e12:7.1f} TFLOP/s = {100 * flop / (th[0] * 1e-3) / PEAK_F16:4.1f} % of the fp16 peak (whole call)")
        lines.append(f"C={C:5d}  torch median {tt[0]:8.3f}  min {tt[1]:8.3f}  max {tt[2]:8.3f}   hip / torch = {th[0] / tt[0]:.2f}")
        lines.append(f"C={C:5d}  same nearest index as the torch path on {100 * same:.3f} % of rows; max |dist - torch dist| {float((dist - td).abs().max()):.2e}; "
                     f"max |weight - torch weight| {float((w - tw).abs().max()):.2e}")
        # evidence for the candidate count: on 1024 rows, fp64 distances to every target — does the kernel pick the fp64 argmin, and
        # how many targets lie within 1e-6 / 1e-5 of the best (the compensated fp16 pair's score error is ~4e-6 relative to |score| <= 1;
        # more than KNN_KEEP - 1 = 3 rivals inside that band is what 4 candidates could lose)
        rows = torch.randperm(N, generator=g)[:1024].to(dev)
        q64 = torch.nn.functional.normalize(f0.t()[rows].double(), dim=-1)
        D64 = 1 - q64 @ torch.nn.functional.normalize(f1.t().double(), dim=-1).t()
        best, arg = D64.min(dim=1)
        lines.append(f"C={C:5d}  fp64 on 1024 rows: kernel index == fp64 argmin on {100 * float((nn[rows].long() == arg).double().mean()):.2f} %, "
                     f"worst excess of the picked distance {float((D64.gather(1, nn[rows].long()[:, None])[:, 0] - best).max()):.2e}; "
                     f"rivals within 1e-6 of the best: max {int(((D64 <= best[:, None] + 1e-6).sum(1) - 1).max())}, within 1e-5: max {int(((D64 <= best[:, None] + 1e-5).sum(1) - 1).max())}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
