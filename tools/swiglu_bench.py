"""DINOv2's SwiGLU MLP on the GPU, measured (profiles/swiglu_bench.txt is one run of this):

1. mvp_swiglu_fwd at H = 4096 (ViT-g/14) for M = 4112 (B = 16 at 224^2: 16 x 257 rows) and M = 25 776 (B = 16 at 480 x 640: 16 x 1611
   rows), fp32 gate | value -> bf16 pair, each beside
   (a) torch's own ops on the same buffers (``F.silu(a) * b``, then the pair split hi = bf16(y), lo = bf16(y - hi)) and
   (b) a device copy that moves the same bytes (the kernel reads 8 and writes 4 bytes per element: 12 M H in all; ``dst.copy_(src)`` on
       an fp32 tensor of 6 M H bytes reads and writes that much).
   The ratio kernel / copy is the figure to watch: a pointwise kernel cannot beat the copy by much, and should not lose to it by much.
2. The whole forward, four taps, dense-cls, B images at 224^2: ViT-g/14 (40 blocks, C = 1536, SwiGLU) and ViT-L/14 (24 blocks, C = 1024,
   GELU) in 'bf16x3' and 'f16x2', in one run.  Seeded random weights (no checkpoint is needed).

Device events around ITERS launches per round, ROUNDS rounds, the candidates alternating inside every round; median and range.

    python tools/swiglu_bench.py [--batch 16] [--rounds 7] [--iters 50] [--out profiles/swiglu_bench.txt] [--skip-models]"""
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

H = 4096
ROWS = (4112, 25776)


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


def main():
    from evals.models.dino import DINO
    from mvp import backbone as bb
    from mvp import lib, ops

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "swiglu_bench.txt"))
    ap.add_argument("--skip-models", action="store_true", help="section 1 only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/swiglu_bench.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    B = a.batch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/swiglu_bench.py  B={B}, {a.rounds} rounds x {a.iters} launches, device events; {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d')}")
    say("# 1. mvp_swiglu_fwd (fp32 gate | value -> bf16 pair, H = 4096) | torch F.silu(a) * b + pair split on the same buffers | device copy of the same bytes")
    g = torch.Generator().manual_seed(0)
    for M in ROWS:
        h12 = (torch.randn(M, 2 * H, generator=g) * 3.0).to(dev)
        out = ops.empty_pair((M, H), lib.PREC_BF16X3, dev)
        out16 = ops.empty_pair((M, H), lib.PREC_BF16X3, dev)
        src, dst = torch.randn(M * H * 3 // 2, device=dev), torch.empty(M * H * 3 // 2, device=dev)  # 6 M H bytes each way
        t_hi, t_lo = torch.empty(M, H, dtype=torch.bfloat16, device=dev), torch.empty(M, H, dtype=torch.bfloat16, device=dev)
        ga, va = h12[:, :H], h12[:, H:]

        def ours():
            ops.swiglu(h12, out, M, H)

        def ours16():
            ops.swiglu(h12, out16, M, H, precision=lib.PREC_F16X2)

        def copy():
            dst.copy_(src)

        def torch_ops():
            y = F.silu(ga) * va  # then the split: two conversions and a subtraction
            t_hi.copy_(y)
            t_lo.copy_(y - t_hi.float())

        ours()
        torch_ops()
        ref = F.silu(ga.double()) * va.double()
        err = float(((out[0].double() + out[1].double()) - ref).norm() / ref.norm())
        err_t = float(((t_hi.double() + t_lo.double()) - ref).norm() / ref.norm())
        del ref
        for fn in (ours, ours16, copy, torch_ops):
            timed(fn, 10)
        t = {"ours": [], "ours16": [], "copy": [], "torch": []}
        for _ in range(a.rounds):
            t["ours"].append(timed(ours, a.iters))
            t["ours16"].append(timed(ours16, a.iters))
            t["copy"].append(timed(copy, a.iters))
            t["torch"].append(timed(torch_ops, a.iters))
        mb = M * H * 12 / 1e6
        mo, mc, mt, m16 = (statistics.median(t[k]) for k in ("ours", "copy", "torch", "ours16"))
        say(f"M={M:6d} ({mb:7.1f} MB moved): kernel {fmt(t['ours'])} = {mb / mo:5.2f} TB/s | fp16 pair form {fmt(t['ours16'])} | copy {fmt(t['copy'])} = {mb / mc:5.2f} TB/s | "
            f"torch ops {fmt(t['torch'])} | kernel / copy {mo / mc:.2f}x, kernel / torch {mo / mt:.2f}x  (rel L2 of the pair vs fp64: kernel {err:.1e}, torch {err_t:.1e})")
        del h12, out, out16, src, dst, t_hi, t_lo
    if not a.skip_models:
        say(f"# 2. whole forward, four taps, dense-cls, B={B} at 224^2, seeded random weights: ViT-g/14 (SwiGLU, 40 blocks) | ViT-L/14 (GELU, 24 blocks)")
        img = torch.randn(B, 3, 224, 224, generator=g).to(dev)
        for name in ("vitg14", "vitl14"):
            C, depth, R = bb.DINOV2_ARCH[name]
            sd = bb.random_dinov2_state_dict(C, depth, R, seed=1, ffn=bb.DINOV2_FFN.get(name, "mlp"))
            for precision in ("bf16x3", "f16x2"):
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    m = DINO(dino_name="dinov2", model_name=name, output="dense-cls", return_multilayer=True, add_norm=True, weights=sd,
                             precision=precision).to(dev).eval()

                def fwd():
                    with torch.no_grad():
                        return m(img)

                timed(fwd, 3)
                ts = [timed(fwd, 5) / 1e3 for _ in range(a.rounds)]
                mo = statistics.median(ts)
                say(f"{name} {precision}: {mo:7.2f} ms ({min(ts):.2f} .. {max(ts):.2f}) = {B / mo * 1e3:6.0f} img/s  (taps {m.multilayers}, hidden {m.engine().hidden})")
                del m
                torch.cuda.empty_cache()
            del sd
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
