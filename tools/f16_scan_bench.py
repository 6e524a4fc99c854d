"""The f16x2 range guard on the GPU, measured (profiles/f16_scan_bench.txt is one run of this):

1. mvp_f16_range_scan at (M, cols) = (3152, 768), (3152, 3072), (21670, 3072) — B = 16 at 224^2 with C and 4C columns, B = 16 x 5 at 518^2
   rows with 4C — in both layouts, each beside
   (a) a device copy of the bytes the kernel reads, 2 M cols (``dst.copy_(src)``: that many bytes read AND written).  In the
       interleaved layout the kernel reads the hi half — 64 of every 128 bytes — of an array of 4 M cols bytes; the copy beside it still
       moves 2 M cols contiguous bytes, and a second copy moves the whole stored array (4 M cols), since the memory system may fetch whole lines;
   (b) the torch expression of the MVP_CHECK_F16_RANGE diagnostic on the same operand (``(t.view(fp16).abs() < 65504).all()`` on hi and
       lo, each with its host sync).
   "warm": the same operand every launch (it stays in the last-level cache, as an operand its producer has just written may);
   "cold": launches rotate over enough operands (>= 512 MiB in all) that every one comes from HBM.
2. The guard's one-off cost: the FIRST forward of a fresh DINO ViT-B/16 wrapper (seeded random weights, B = 16 at 224^2; host clock
   around forward + synchronise, engine construction included) with ``range_guard="warn"`` and with ``"off"``, alternating; then the
   second forward of each.

Device events around ITERS launches per round, ROUNDS rounds, the candidates alternating inside every round; median and range.

    python tools/f16_scan_bench.py [--rounds 7] [--iters 50] [--out profiles/f16_scan_bench.txt] [--skip-model]"""
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

SHAPES = ((3152, 768), (3152, 3072), (21670, 3072))
COLD_BYTES = 512 << 20


def timed(fn, iters):
    """Device time per call, microseconds."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def fmt(xs):
    return f"{statistics.median(xs):7.1f} us ({min(xs):.1f} .. {max(xs):.1f})"


def main():
    from evals.models.dino import DINO
    from mvp import backbone as bb
    from mvp import ops

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "f16_scan_bench.txt"))
    ap.add_argument("--skip-model", action="store_true", help="section 1 only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/f16_scan_bench.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/f16_scan_bench.py  {a.rounds} rounds x {a.iters} launches, device events; {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d')}")
    say("# 1. mvp_f16_range_scan | device copy of the bytes it reads (2 M cols read + as many written) | interleaved only: copy of the whole stored array "
        "(4 M cols) | torch expression of the MVP_CHECK_F16_RANGE diagnostic (hi and lo, host sync each)")
    g = torch.Generator().manual_seed(0)
    for M, cols in SHAPES:
        for layout in ("separate", "interleaved"):
            ilv = layout == "interleaved"
            read_b, stored_b = 2 * M * cols, (4 if ilv else 2) * M * cols
            n_ops = -(-COLD_BYTES // stored_b)
            vals = (torch.randn(M, cols, generator=g) * 30.0).to(dev)
            hi, lo = ops.split_f16_comp(vals)
            one = ops.interleave_pair((hi, lo)) if ilv else hi  # [M, 2 cols] or [M, cols] 16-bit words
            pool = one.unsqueeze(0).repeat(n_ops, 1, 1).contiguous()
            lo_pool = None if ilv else lo.unsqueeze(0).repeat(n_ops, 1, 1).contiguous()
            src = torch.empty(n_ops, read_b // 2, dtype=torch.bfloat16, device=dev).copy_(pool.view(n_ops, -1)[:, :read_b // 2])
            dst, dst_all = torch.empty(read_b // 2, dtype=torch.bfloat16, device=dev), torch.empty_like(one)
            rec = torch.zeros(4, dtype=torch.int32, device=dev).view(torch.uint32)

            def operand(k):
                t = pool[k]
                if not ilv:
                    return (t, None)
                p = ops.IlvPair.__new__(ops.IlvPair)
                p.rows, p.cols, p.t = M, cols, t
                return p

            operands = [operand(k) for k in range(n_ops)]

            def scan(i, cold):
                ops.f16_range_scan(operands[i % n_ops if cold else 0], M, cols, rec)

            def copy(i, cold):
                dst.copy_(src[i % n_ops if cold else 0])

            def copy_all(i, cold):
                dst_all.copy_(pool[i % n_ops if cold else 0])

            def torch_check(i, cold):
                k = i % n_ops if cold else 0
                for t in ([pool[k]] if ilv else [pool[k], lo_pool[k]]):
                    bool((t.view(torch.float16).abs() < 65504.0).all())

            scan(0, False)
            torch.cuda.synchronize()
            words = (rec.view(torch.int32).cpu().to(torch.int64) & 0xFFFFFFFF).tolist()
            assert words[1:] == [0, 0, M * cols], words
            cands = [("scan", scan), ("copy", copy)] + ([("copy_all", copy_all)] if ilv else []) + [("torch", torch_check)]
            for cold in (False, True):
                for _, fn in cands:
                    timed(lambda i: fn(i, cold), 10)
                t = {k: [] for k, _ in cands}
                for _ in range(a.rounds):
                    for k, fn in cands:
                        t[k].append(timed(lambda i: fn(i, cold), a.iters))
                ms, mc = statistics.median(t["scan"]), statistics.median(t["copy"])
                line = (f"M={M:6d} cols={cols:5d} {layout:<11} {'cold' if cold else 'warm'} ({read_b / 1e6:6.1f} MB read of {stored_b / 1e6:6.1f} MB stored, "
                        f"{n_ops if cold else 1:3d} operand(s)): scan {fmt(t['scan'])} = {read_b / 1e6 / ms:5.2f} TB/s read | copy {fmt(t['copy'])} = "
                        f"{read_b / 1e6 / mc:5.2f} TB/s read (+ as much written)")
                if ilv:
                    ma = statistics.median(t["copy_all"])
                    line += f" | copy of the stored array {fmt(t['copy_all'])} = {stored_b / 1e6 / ma:5.2f} TB/s read"
                line += f" | torch check {fmt(t['torch'])} | scan / copy {ms / mc:.2f}x, scan / torch {ms / statistics.median(t['torch']):.3f}x"
                say(line)
            del pool, lo_pool, src, dst, dst_all, operands, vals, hi, lo, one
            torch.cuda.empty_cache()
    if not a.skip_model:
        B = 16
        say(f"# 2. first forward of a fresh DINO ViT-B/16 wrapper (f16x2, four taps, B={B} at 224^2, seeded random weights; host clock, engine build "
            "included) with the guard forced on (range_guard='warn': one extra audited forward, one sync, one 960-byte copy) and off; then the second forward")
        sd = bb.random_vit_state_dict(seed=1)
        img = torch.randn(B, 3, 224, 224, generator=g).to(dev)
        first, second = {"warn": [], "off": []}, {"warn": [], "off": []}

        def once(guard):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                m = DINO(return_multilayer=True, add_norm=True, weights=sd, precision="f16x2", range_guard=guard).to(dev).eval()
            out = []
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with torch.no_grad():
                    m(img)
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t0) * 1e3)
            assert (m.f16_range_report() is not None) == (guard == "warn")
            return out

        once("off")  # (the process's first forward loads code objects: not part of either series)
        for _ in range(5):
            for guard in ("warn", "off"):
                f, s = once(guard)
                first[guard].append(f)
                second[guard].append(s)
        for guard in ("warn", "off"):
            say(f"range_guard={guard:<4}: first forward {statistics.median(first[guard]):7.2f} ms ({min(first[guard]):.2f} .. {max(first[guard]):.2f}) | "
                f"second forward {statistics.median(second[guard]):6.2f} ms ({min(second[guard]):.2f} .. {max(second[guard]):.2f})")
        say(f"guard's one-off cost: {statistics.median(first['warn']) - statistics.median(first['off']):.2f} ms on the first forward (medians of 5)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
