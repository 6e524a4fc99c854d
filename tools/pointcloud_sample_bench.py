#!/usr/bin/env python3
"""Device-side timing of mvp_pointcloud_sample (csrc/pointcloud.hip) at the ScanNet workload's shape — feature map 30 x 40, depth
grid 120 x 160 = 19 200 points, C = 768 and C = 3 072 (multilayer) — beside the plain torch composition that produces the same
channel-major [C, N] map in the same process: project, grid_sample(bilinear, zeros, align_corners=False), transpose, contiguous()
(grid_sample's output is channel-major already, so transposing the reference's [N, C] view back costs torch no copy).

    python tools/pointcloud_sample_bench.py [--c 768 3072] [--reps 30] [--warmup 5] [--out profiles/pointcloud_sample_bench.txt]

The two are timed ALTERNATING, call by call, with device events (the whole ABI call / the whole torch chain); per shape: median
(min - max) of each, their ratio, the largest difference between the two results, and the kernel's bytes written (C N 4) over its
median as a share of the 8 TB/s HBM peak — a whole-call rate (launch included), not a kernel's.  Needs a GPU; there is no CPU
fallback."""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "midvision-probe_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_HBM = 8.0e12  # bytes/s (spec)


def timed_alternating(fns, reps, warmup):
    """[(median, min, max) ms] per function; call i of every function is made before call i + 1 of any."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return [(sorted(m)[len(m) // 2], min(m), max(m)) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c", type=int, nargs="+", default=[768, 3072])
    ap.add_argument("--feat", type=int, nargs=2, default=[30, 40])
    ap.add_argument("--grid", type=int, nargs=2, default=[120, 160])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pointcloud_sample_bench needs a GPU")
    from mvp import corr3d, ops

    dev = torch.device("cuda:0")
    (fh, fw), (H, W) = a.feat, a.grid
    N = H * W
    lines = [f"mvp_pointcloud_sample vs torch (project, grid_sample, transpose, contiguous); map {fh} x {fw}, {N} points ({H} x {W}); "
             f"{a.reps} timed calls each after {a.warmup}, alternating; device events, ms: median (min - max)"]
    for C in a.c:
        g = torch.Generator(device="cpu").manual_seed(C)
        feat = torch.randn(C, fh, fw, generator=g).to(dev)
        depth = torch.rand(1, H, W, generator=g) * 3 + 0.5
        depth[0][torch.rand(H, W, generator=g) < 0.2] = 0.0  # sensor holes
        K = torch.tensor([[0.9 * W, 0.0, 0.53 * W], [0.0, 0.93 * W, 0.47 * H], [0.0, 0.0, 1.0]])
        pc = corr3d.grid_to_pointcloud(K.inverse().to(dev), depth.to(dev)).contiguous()
        Kd = K.to(dev)
        out = torch.empty(C, N, dtype=torch.float32, device=dev)
        valid = torch.empty(N, dtype=torch.uint8, device=dev)

        def hip():
            ops.pointcloud_sample(feat, pc, Kd, out, valid, C, fh, fw, N, H, W, N)
            return out

        def plain():
            uvd = pc @ Kd.t()
            uv = uvd[:, :2] / uvd[:, 2:3].clamp(min=1e-9)
            uv = torch.stack((2 * uv[:, 0] / W - 1, 2 * uv[:, 1] / H - 1), dim=1)
            s = torch.nn.functional.grid_sample(feat[None], uv[None, None], mode="bilinear", padding_mode="zeros", align_corners=False)
            return s[0, :, 0].transpose(0, 1).t().contiguous()  # the reference's [N, C] view, transposed back: grid_sample's own layout, no copy

        th, tt = timed_alternating([hip, plain], a.reps, a.warmup)
        diff = float((hip() - plain()).abs().max())
        nbytes = C * N * 4
        fmt = lambda t: f"{t[0]:7.3f} ({t[1]:7.3f} - {t[2]:7.3f})"  # noqa: E731
        lines.append(f"C={C:5d}  hip   {fmt(th)}   writes {nbytes / 1e6:6.1f} MB -> {nbytes / (th[0] * 1e-3) / 1e9:7.1f} GB/s = "
                     f"{100 * nbytes / (th[0] * 1e-3) / PEAK_HBM:4.1f} % of the HBM peak (whole call)")
        lines.append(f"C={C:5d}  torch {fmt(tt)}   hip / torch = {th[0] / tt[0]:.2f}")
        lines.append(f"C={C:5d}  max |hip - torch| = {diff:.2e} on values of unit variance")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
