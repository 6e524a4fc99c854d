#!/usr/bin/env python3
"""Device-side timing of the dense-CRF refinement (csrc/densecrf.hip, mvp/densecrf.py) at the evaluation's own size.

    python tools/densecrf_bench.py [--reps 5] [--warmup 1] [--images 16] [--size 480] [--budget-seconds 300] [--out profiles/densecrf_bench.txt]

Workload: 480 x 480 SyntheticVOC images, a batch of 16 with two objects each (the 16-pixel block masks of two rectangles).
Part 1 times one filter pass of each kernel ALTERNATING with device events: the spatial and the bilateral kernel on the two objects'
fields and on the ones field; pair evaluations per second from the library's own skip rule (mvp.ops.crf_filter_pairs).
Part 2 times a refined batch (mvp.densecrf.refine_and_union: 4 + 20 filter passes, 12 pointwise launches, the finish step) by a host
clock around a device synchronise.
Part 3 times a plain-torch restatement of one filter pass on the same device, row blocks of the N x N weight matrix, for ONE image
(a whole batch of it would take minutes) and compares its result with the kernel's.
Part 4 runs the whole evaluation (mvp.maskcut.predict on the same 16 images, a seeded ViT-B/16) with the refinement off and on.
Every part stops taking windows once the budget is used up (at least one window each).  Needs a GPU; there is no CPU fallback.

The instruction-count bound: the bilateral inner loop compiles to 3 subtractions, 4 fused multiply-adds and one v_exp_f32 per pair
plus one fused multiply-add per field (9 VALU + 1 exp at two fields; the spatial one to 1 add + 1 exp + 1 per field).  With several
waves resident a SIMD issues an fp32 VALU instruction of a wave in 2 clocks (32 lanes per clock) and a transcendental in twice
that, so a pair costs 9 + 2 = 11 issue slots per lane at two fields, and the chip issues 256 CUs x 4 SIMDs x 32 lanes per clock.  The
bound leaves out the staging of the source tiles, the LDS reads and the fp64 folding of the row sums."""
import argparse
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "midvision-probe_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

LANES_PER_CLOCK = 256 * 4 * 32
SLOTS = {"spatial": lambda F: 1 + 2 + F, "bilateral": lambda F: 7 + 2 + F}  # VALU + the exp at two slots, per pair


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


def host_timed(fn, reps, warmup, budget):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for r in range(reps):
        if r and not budget.left():
            break
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return sorted(ms)[len(ms) // 2], min(ms), max(ms), len(ms)


def make_batch(B, S, dev):
    """(rgb_u8 [B, 3, S, S], masks [B, 2, S, S] uint8, dataset): SyntheticVOC images, two block masks each."""
    from evals.datasets.synthetic import SyntheticVOC
    from mvp import maskcut

    ds = SyntheticVOC("test", num_samples=B, fixed_size=S, seed=1)
    rgb = torch.stack([ds[i]["original_image_rgb"] for i in range(B)]).to(dev)
    masks = torch.zeros(B, 2, S // 16, S // 16, dtype=torch.uint8)
    c = S // 16
    for b in range(B):
        y0, x0 = 2 + b % 5, 1 + b % 4
        masks[b, 0, y0:y0 + c // 3, x0:x0 + c // 4] = 1
        masks[b, 1, y0 + c // 4:y0 + c // 2, x0 + c // 2:x0 + c * 3 // 4] = 1
    masks = masks.repeat_interleave(16, dim=2).repeat_interleave(16, dim=3).contiguous().to(dev)
    return maskcut.quantise_rgb(rgb, rgb), masks, ds


def torch_filter(rgb_hwc, field, inv_var_xy, inv_var_rgb, rows=2048):
    """One filter pass of ONE image in plain torch: row blocks of the N x N weights.  rgb_hwc [H, W, 3] uint8, field [F, N] fp32."""
    H, W = rgb_hwc.shape[:2]
    dev = rgb_hwc.device
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    y, x, c = yy.reshape(-1), xx.reshape(-1), rgb_hwc.reshape(-1, 3).float()
    out = torch.empty_like(field)
    for i0 in range(0, H * W, rows):
        s = slice(i0, min(i0 + rows, H * W))
        e = ((y[s, None] - y[None, :]) ** 2 + (x[s, None] - x[None, :]) ** 2) * (-0.5 * inv_var_xy)
        if inv_var_rgb > 0:
            for k in range(3):
                e -= (c[s, None, k] - c[None, :, k]) ** 2 * (0.5 * inv_var_rgb)
        out[:, s] = field @ torch.exp(e).t()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--budget-seconds", type=float, default=300.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("densecrf_bench needs a GPU")
    from mvp import densecrf, maskcut, ops

    dev = torch.device("cuda:0")
    B, S = a.images, a.size
    N = S * S
    rgb_u8, masks, ds = make_batch(B, S, dev)
    hwc = rgb_u8.permute(0, 2, 3, 1).contiguous()
    clock_hz = 2.4e9  # the peak engine clock the bound is stated at
    lines = [f"densecrf_bench: {B} images of {S} x {S}, two objects each; {torch.cuda.get_device_name(0)}; bound clock {clock_hz / 1e9:.2f} GHz"]
    kinds = {"spatial": (1.0 / densecrf.POS_XY_STD ** 2, 0.0), "bilateral": (1.0 / densecrf.BI_XY_STD ** 2, 1.0 / densecrf.BI_RGB_STD ** 2)}

    # ---- part 1: one filter pass per kernel and field count, alternating
    x2 = torch.rand(B, 2, N, device=dev)
    o2, o1 = torch.empty(B, 2, N, device=dev), torch.empty(B, 1, N, device=dev)
    legs, fns = [], []
    for kind, (vxy, vrgb) in kinds.items():
        legs.append((kind, 2))
        fns.append(lambda vxy=vxy, vrgb=vrgb: ops.crf_filter(hwc, o2, B, 2, S, S, vxy, vrgb, inp=x2))
        legs.append((kind, 1))
        fns.append(lambda vxy=vxy, vrgb=vrgb: ops.crf_filter(hwc, o1, B, 1, S, S, vxy, vrgb))
    budget = Budget(a.budget_seconds * 0.3)
    for (kind, F), (med, lo, hi, n) in zip(legs, timed_alternating(fns, a.reps, a.warmup, budget)):
        pairs = ops.crf_filter_pairs(B, S, S, kinds[kind][0])
        bound_ms = 1e3 * pairs * SLOTS[kind](F) / (LANES_PER_CLOCK * clock_hz)
        lines.append(f"filter {kind:9s} F={F}: {med:9.2f} ms ({lo:.2f} - {hi:.2f}, {n} windows)  {pairs / B:.3e} pairs/image  "
                     f"{pairs / med / 1e6:.1f} G pairs/s  issue bound {bound_ms:.2f} ms ({bound_ms / med:.0%} of the bound's rate)")

    # ---- part 2: a refined batch
    budget = Budget(a.budget_seconds * 0.3)
    med, lo, hi, n = host_timed(lambda: densecrf.refine_and_union(rgb_u8, masks), max(1, a.reps // 2), a.warmup, budget)
    union = densecrf.refine_and_union(rgb_u8, masks)[0]
    lines.append(f"refined batch ({B} x 2 objects, {densecrf.MAX_ITER} iterations): {med:.1f} ms ({lo:.1f} - {hi:.1f}, {n} windows); "
                 f"union {float(union.float().mean()):.4f} of the pixels, input masks {float(masks.amax(dim=1).float().mean()):.4f}")

    # ---- part 3: the plain-torch restatement, one image
    budget = Budget(a.budget_seconds * 0.2)
    for kind, (vxy, vrgb) in kinds.items():
        t_med, t_lo, t_hi, t_n = host_timed(lambda: torch_filter(hwc[0], x2[0], vxy, vrgb), 2, 1, budget)
        want = torch_filter(hwc[0], x2[0], vxy, vrgb)
        ops.crf_filter(hwc, o2, B, 2, S, S, vxy, vrgb, inp=x2)
        k_med = timed_alternating([lambda: ops.crf_filter(hwc[:1], o2[:1], 1, 2, S, S, vxy, vrgb, inp=x2[:1])], 3, 1, budget)[0][0]
        rel = float(((o2[0] - want).abs() / want).max())
        lines.append(f"torch restatement {kind:9s} F=2, ONE image: {t_med:.1f} ms ({t_n} windows) against {k_med:.2f} ms for the kernel "
                     f"({t_med / k_med:.1f}x); max relative difference {rel:.1e} (torch sums in fp32)")

    # ---- part 4: the whole evaluation, refinement off and on
    from evals.models.dino import DINO
    from oracle import vit as ovit

    model = DINO(weights=ovit.make_vit_weights(embed_dim=768, depth=12, seed=1), return_kqv=True, fixed_size=S).to(dev).eval()
    budget = Budget(a.budget_seconds * 0.2)
    for refine in ("none", "dense_crf"):
        proc = maskcut.MaskCutProcessor(backbone=model, patch_size=16, fixed_size=S, refine=refine)
        res = {}

        def run():
            res["avg"], res["fb"], res["n"] = maskcut.predict(proc, ds, B, dev)

        med, lo, hi, n = host_timed(run, 2, 1, budget)
        lines.append(f"evaluation of {res['n']} images, refine={refine}: {med:.1f} ms ({lo:.1f} - {hi:.1f}, {n} windows)  "
                     f"IoU {res['avg']['IoU']:.4f} F-measure {res['avg']['F-measure']:.4f}  fallback solves {res['fb']}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
