"""ConvNeXt on the GPU, measured (profiles/convnext_backbone.txt is one run of this):

1. mvp_dwconv7_ln_fwd at the four stage shapes of ConvNeXt-B at 224^2 (56^2 x 128, 28^2 x 256, 14^2 x 512, 7^2 x 1024), batch B, each beside
   (a) a device copy of the same bytes (the fp32 map read once + 4 bytes per element written: ``dst.copy_(src)`` on an fp32 tensor of the
       map's size) and
   (b) torch's own F.conv2d(groups=C) + F.layer_norm on the same data (channels-last memory format, fp32).
2. The whole forward (ConvNeXt-B and V2-B, four taps, dense) beside a plain-torch fp32 restatement on the same weights, with the
   relative L2 difference of the outputs.

Device events around ITERS launches per round, ROUNDS rounds, the candidates alternating inside every round; median and range.

    python tools/convnext_bench.py [--batch 16] [--rounds 7] [--iters 50]"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "midvision-probe_amd")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

STAGES = ((56, 128), (28, 256), (14, 512), (7, 1024))


def timed(fn, iters):
    """Device time per call, microseconds."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def fmt(xs):
    return f"{statistics.median(xs):8.1f} us ({min(xs):.1f} .. {max(xs):.1f})"


def torch_trunk(sd, images):
    """The trunk in plain torch fp32 (timm's ConvNeXt arithmetic) on an engine-layout state dict -> the four stage outputs, NCHW."""
    v2 = any(".mlp.grn." in k for k in sd)
    x = F.conv2d(images, sd["stem.0.weight"], sd["stem.0.bias"], stride=4).permute(0, 2, 3, 1)
    x = F.layer_norm(x, x.shape[-1:], sd["stem.1.weight"], sd["stem.1.bias"], 1e-6)
    outs = []
    for i in range(4):
        if i > 0:
            p = f"stages.{i}.downsample."
            x = F.layer_norm(x, x.shape[-1:], sd[p + "0.weight"], sd[p + "0.bias"], 1e-6)
            x = F.conv2d(x.permute(0, 3, 1, 2), sd[p + "1.weight"], sd[p + "1.bias"], stride=2).permute(0, 2, 3, 1)
        j = 0
        while f"stages.{i}.blocks.{j}.conv_dw.weight" in sd:
            p = f"stages.{i}.blocks.{j}."
            C = x.shape[-1]
            y = F.conv2d(x.permute(0, 3, 1, 2), sd[p + "conv_dw.weight"], sd[p + "conv_dw.bias"], padding=3, groups=C).permute(0, 2, 3, 1)
            y = F.layer_norm(y, (C,), sd[p + "norm.weight"], sd[p + "norm.bias"], 1e-6)
            y = F.gelu(F.linear(y, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"]))
            if v2:
                G = y.pow(2).sum(dim=(1, 2), keepdim=True).sqrt()
                y = sd[p + "mlp.grn.weight"] * (y * (G / (G.mean(dim=-1, keepdim=True) + 1e-6))) + sd[p + "mlp.grn.bias"] + y
            y = F.linear(y, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
            x = x + (y if v2 else y * sd[p + "gamma"])
            j += 1
        outs.append(x.permute(0, 3, 1, 2))
    return outs


def main():
    from evals.models.convnext import ConvNext
    from mvp import convnext as cnx
    from mvp import ops

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/convnext_bench.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    B = a.batch
    print(f"# tools/convnext_bench.py  B={B}, {a.rounds} rounds x {a.iters} launches, device events; {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d')}")
    print("# 1. mvp_dwconv7_ln_fwd (fp32 map -> bf16 pair) | device copy of the same bytes | torch F.conv2d(groups=C) + F.layer_norm (fp32, channels-last)")
    g = torch.Generator().manual_seed(0)
    for S, C in STAGES:
        M = B * S * S
        x = torch.randn(B, S, S, C, generator=g).to(dev)
        w, b = (torch.randn(C, 1, 7, 7, generator=g) / 7).to(dev), torch.randn(C, generator=g).to(dev)
        gamma, beta = (0.5 + torch.rand(C, generator=g)).to(dev), torch.randn(C, generator=g).to(dev)
        out = ops.empty_pair((M, C), 3, dev)
        src, dst = torch.randn(M * C, device=dev), torch.empty(M * C, device=dev)
        x_nchw = x.permute(0, 3, 1, 2)  # a channels-last view of the same memory

        def ours():
            ops.dwconv7_ln(x, w, b, gamma, beta, out, B, S, S, C, 1e-6)

        def copy():
            dst.copy_(src)

        def torch_pair():
            return F.layer_norm(F.conv2d(x_nchw, w, b, padding=3, groups=C).permute(0, 2, 3, 1), (C,), gamma, beta, 1e-6)

        ref = torch_pair().reshape(M, C)
        ours()
        err = float(((out[0].float() + out[1].float()) - ref).norm() / ref.norm())
        for fn in (ours, copy, torch_pair):
            timed(fn, 10)
        t = {"ours": [], "copy": [], "torch": []}
        for _ in range(a.rounds):
            t["ours"].append(timed(ours, a.iters))
            t["copy"].append(timed(copy, a.iters))
            t["torch"].append(timed(torch_pair, a.iters))
        mb = M * C * 8 / 1e6
        print(f"{S:3d}^2 x {C:4d} ({mb:6.1f} MB moved): fused {fmt(t['ours'])} = {mb / statistics.median(t['ours']):5.2f} TB/s | copy {fmt(t['copy'])} | "
              f"torch pair {fmt(t['torch'])} | fused / torch {statistics.median(t['ours']) / statistics.median(t['torch']):.2f}x  (rel L2 vs torch {err:.1e})")
    print("# 2. whole forward, four taps, dense, 224^2: HIP engine (bf16x3) | plain torch fp32 on the same weights")
    img = torch.randn(B, 3, 224, 224, generator=g).to(dev)
    for v2 in (False, True):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sd = cnx.random_state_dict(v2=v2, seed=1)
            m = ConvNext("convnext_base", "fcmae_ft_in22k_in1k_384" if v2 else "in22k", weights=sd, return_multilayer=True, precision="bf16x3").to(dev)
        sdd = {k: v.to(dev) for k, v in sd.items()}

        def ours():
            return m(img)

        def plain():
            with torch.no_grad():
                return [F.interpolate(t, (14, 14), mode="bilinear") for t in torch_trunk(sdd, img)]

        errs = [float((o - r).norm() / r.norm()) for o, r in zip(ours(), plain())]
        for fn in (ours, plain):
            timed(fn, 3)
        t = {"ours": [], "plain": []}
        for _ in range(a.rounds):
            t["ours"].append(timed(ours, 5) / 1e3)
            t["plain"].append(timed(plain, 5) / 1e3)
        mo, mp = statistics.median(t["ours"]), statistics.median(t["plain"])
        print(f"ConvNeXt{' V2' if v2 else ''}-B: engine {mo:7.2f} ms ({min(t['ours']):.2f} .. {max(t['ours']):.2f}) = {B / mo * 1e3:6.0f} img/s | "
              f"torch fp32 {mp:7.2f} ms ({min(t['plain']):.2f} .. {max(t['plain']):.2f}) = {B / mp * 1e3:6.0f} img/s | engine / torch {mo / mp:.2f}x  "
              f"(rel L2 per tap vs torch fp32 {', '.join('%.1e' % e for e in errs)})")


if __name__ == "__main__":
    main()
