"""Attention kernel time at the token counts of ViT-B/16 (N = 197, the resident kernel) and DINOv2 B/14 / B/14-reg (N = 257 / 261 at
224^2, just past the resident kernel's N <= 256: the streaming kernel), B = 16 and 110 images, 12 heads, all four forms (bf16 pair,
VF16, VF16 + f16 Q.K^T, bf16).  HIP events around REPS launches, the shapes interleaved round by round in one process; prints the median
time per launch and the time per query-key pair per head (what a resident path for 256 < N <= 320 could at best bring back to the N = 197
figure).

    python tools/attn_n_bench.py [--rounds 5] [--reps 20]"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "midvision-probe_amd")]

import torch  # noqa: E402

FORMS = {"bf16x3 pair": (3, False, False), "vf16": (3, True, False), "vf16+qk16": (3, True, True), "bf16": (1, False, False)}


def main():
    from mvp import lib, ops

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    H, C = 12, 768
    cases = {}
    for B in (16, 110):
        for N in (197, 257, 261):
            g = torch.Generator().manual_seed(N + B)
            qkv = torch.randn(B * N, 3 * C, generator=g).to(dev)
            for name, (pr, vf16, qk16) in FORMS.items():
                qp = ops.split_bf16(qkv, pr)  # (the bit patterns of the fp16 forms do not change the work: timing only)
                out = ops.empty_pair((B * N, C), lib.PREC_BF16X3, dev)
                cases[(B, N, name)] = (qp, out, pr, vf16, qk16)
    times = {k: [] for k in cases}
    for _ in range(2):  # warm-up
        for k, (qp, out, pr, vf16, qk16) in cases.items():
            ops.attention(qp, out, k[0], k[1], H, 0.125, pr, v_f16=vf16, qk_f16=qk16)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, (qp, out, pr, vf16, qk16) in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                ops.attention(qp, out, k[0], k[1], H, 0.125, pr, v_f16=vf16, qk_f16=qk16)
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / a.reps)
    print(f"# attention, H = 12, median of {a.rounds} rounds x {a.reps} launches (HIP events); ps/pair = time / (B * H * N^2)")
    for (B, N, name), t in times.items():
        us = statistics.median(t)
        print(f"B={B:4d} N={N:4d} {name:12s} {us:9.1f} us  {us * 1e6 / (B * H * N * N):7.2f} ps/pair  "
              f"({'resident' if N <= 256 else 'streaming'} kernel; rounds {', '.join(f'{x:.1f}' for x in t)})")


if __name__ == "__main__":
    main()
