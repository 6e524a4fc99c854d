#!/usr/bin/env python3
"""Device-side timing of the Taskonomy kernels (csrc/taskonomy.hip) at the workload's own shapes, the same stages written in torch
ops, a device copy of the same bytes, and the step they belong to beside the objectness step.

    python tools/taskonomy_bench.py [--batch 16] [--size 512] [--launches 100] [--steps 20] [--out profiles/taskonomy_bench.txt]

(a) Per kernel at B x size^2 with C_t = 2 (principal curvature: 8-bit target of 3 stored channels): ``--launches`` back-to-back calls
    between two device events after a warm-up; per call the time, the bytes the algorithm must move, that rate — and beside it
    (i) a device-to-device copy of as many bytes (half read, half written) timed the same way, (ii) the same stage written in torch
    ops on the same device.  The 16-bit clamp form (depth_euclidean) of mvp_task_prepare is timed too.
(b) The step: train_taskonomy_step (TaskonomyHead dpt k3, 3 channels, 2-channel target) and train_objectness_step (BinaryHead dpt k3),
    same backbone, batch and process, in alternating blocks; median step time by device events around whole steps.
Needs a GPU; there is no CPU fallback."""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "midvision-probe_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK = 8.0e12  # B/s (spec)


def per_call_ms(fn, launches, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / launches


def copy_ms(nbytes, dev, launches):
    """A device copy that moves ``nbytes`` in all (half read, half written)."""
    n = max(int(nbytes) // 2 // 16 * 16, 16)
    src, dst = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    return per_call_ms(lambda: dst.copy_(src), launches)


def kernels(a, dev, lines):
    from mvp import ops

    B, S = a.batch, a.size
    HW, N = S * S, B * S * S
    g = torch.Generator().manual_seed(0)
    raw8 = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
    raw16 = torch.randint(-32768, 32768, (B, S, S), generator=g, dtype=torch.int16).to(dev)
    mask = torch.where(torch.rand(B, S, S, generator=g) < 0.01, 0, 255).to(torch.uint8).to(dev)
    tgt2, tgt1 = torch.empty(B, 2, S, S, device=dev), torch.empty(B, 1, S, S, device=dev)
    valid = torch.empty(B, 1, S, S, dtype=torch.uint8, device=dev)
    clamp = float(torch.tensor(8000.0 / 65535.0, dtype=torch.float32))
    ops.task_prepare(raw8, mask, tgt2, valid, 8)
    pred = torch.randn(B, 2, S, S, generator=g).to(dev)
    loss, grad, ws = torch.empty(1, device=dev), torch.empty_like(pred), ops.task_workspace(dev)
    sums = torch.empty(B, 2, 5, dtype=torch.float64, device=dev)
    vb = valid.bool()

    def t_prepare8():
        x = raw8[..., :2].permute(0, 3, 1, 2).float() / 255.0
        m = (mask == 255).view(B, 1, S // 4, 4, S // 4, 4).all(dim=5).all(dim=3)
        return x.contiguous(), m.repeat_interleave(4, 2).repeat_interleave(4, 3)

    def t_prepare16():
        x = (raw16.to(torch.int32) & 0xFFFF).float().unsqueeze(1) / 65535.0
        x = x.clamp(0.0, clamp) / clamp
        m = (mask == 255).view(B, 1, S // 4, 4, S // 4, 4).all(dim=5).all(dim=3)
        return x, m.repeat_interleave(4, 2).repeat_interleave(4, 3)

    def t_l1():
        p = pred.detach().requires_grad_(True)
        d = (p - tgt2).abs()
        m = vb.expand_as(d)
        l = torch.where(m, d, torch.zeros_like(d)).sum() / m.sum()
        l.backward()
        return l

    def t_metrics(form):
        v = vb.expand_as(pred).float()
        if form == "curvature":
            q = pred.clamp(-1, 1)
            absrel = (q - tgt2).abs() / (tgt2 + 1e-6).abs()
            ratio = torch.max(q / tgt2, tgt2 / q)
        else:
            q, t = pred * v, tgt2 * v
            absrel = (q - t).abs() / (t + 1e-6)
            ratio = torch.max(q / (t + 1e-6), t / (q + 1e-6))
        out = [(absrel * v).double().sum(dim=(2, 3)), v.sum(dim=(2, 3))]
        return out + [((ratio < t_).float() * v).sum(dim=(2, 3)) for t_ in (1.25, 2.5, 3.75)]

    rows = [
        # name, HIP call, torch restatement, bytes the algorithm must move, note
        ("task_prepare 8-bit Cs=3 Ct=2", lambda: ops.task_prepare(raw8, mask, tgt2, valid, 8), t_prepare8, N * (3 + 1 + 8 + 1),
         "3 raw bytes + 1 mask byte read, 2 fp32 + 1 mask byte written per pixel"),
        ("task_prepare 16-bit clamp", lambda: ops.task_prepare(raw16, mask, tgt1, valid, 16, clamp), t_prepare16, N * (2 + 1 + 4 + 1),
         "2 raw bytes + 1 mask byte read, 1 fp32 + 1 mask byte written per pixel"),
        ("masked_l1_fwd_bwd", lambda: ops.masked_l1(pred, tgt2, valid, loss, grad, ws, B, 2, 1, HW), t_l1, 2 * N * (2 * 8 + 1) + 2 * N * 4,
         "pred, target and the mask read twice (the count comes first), grad_pred written"),
        ("masked_l1 loss only", lambda: ops.masked_l1(pred, tgt2, valid, loss, None, ws, B, 2, 1, HW), None, N * (2 * 8 + 1), "pred, target, mask read once"),
        ("task_metrics curvature", lambda: ops.task_metrics(pred, tgt2, valid, sums, ws, B, 2, 1, HW, "curvature", (1.25, 2.5, 3.75)),
         lambda: t_metrics("curvature"), N * (2 * 8 + 1), "pred, target, mask read once"),
        ("task_metrics reshading", lambda: ops.task_metrics(pred, tgt2, valid, sums, ws, B, 2, 1, HW, "reshading", (1.25, 2.5, 3.75)),
         lambda: t_metrics("reshading"), N * (2 * 8 + 1), "pred, target, mask read once"),
    ]
    lines.append(f"(a) kernels at B = {B}, {S}^2, C_t = 2; {a.launches} back-to-back calls between two device events after a warm-up")
    for name, fn, tfn, nbytes, note in rows:
        ms = per_call_ms(fn, a.launches)
        cp = copy_ms(nbytes, dev, a.launches)
        rate = nbytes / (ms * 1e-3)
        tms = per_call_ms(tfn, max(a.launches // 5, 5)) if tfn is not None else None
        lines.append(f"  {name:30s} {ms * 1e3:8.1f} us   {nbytes / 1e6:7.1f} MB must move -> {rate / 1e12:5.2f} TB/s = {100 * rate / HBM_PEAK:4.1f} % of "
                     f"the 8.0 TB/s HBM peak;  a device copy of the same bytes {cp * 1e3:8.1f} us ({nbytes / (cp * 1e-3) / 1e12:5.2f} TB/s);  "
                     + (f"torch ops {tms * 1e3:8.1f} us ({tms / ms:5.1f} x)" if tms is not None else "torch ops: see the row above") + f"   [{note}]")


def steps(a, dev, lines):
    from evals.models.probes import BinaryHead, TaskonomyHead
    from mvp import config
    from mvp.optim import FlatAdamW
    from mvp.train import train_objectness_step, train_taskonomy_step

    B, S = a.batch, a.step_size
    model = config.instantiate(config.compose("taskonomy_training", [f"backbone={a.backbone}"])["backbone"], return_multilayer=True).to(dev).eval()
    g = torch.Generator().manual_seed(1)
    images = torch.randn(B, 3, S, S, generator=g).to(dev)
    mask = (torch.rand(B, 1, S, S, generator=g) < 0.4).float().to(dev)
    target = ((torch.rand(B, 2, S, S, generator=g) * 255).round() / 255).to(dev)
    valid = (torch.rand(B, 1, S, S, generator=g) < 0.9).to(torch.uint8).to(dev)
    tk_probe = TaskonomyHead(feat_dim=model.feat_dim, head_type="dpt", kernel_size=3, output_dim=3, pred_type="vanilla", uncertainty_aware=True).to(dev)
    ob_probe = BinaryHead(feat_dim=model.feat_dim, head_type="dpt", kernel_size=3, output_dim=1).to(dev)
    tk_opt, ob_opt = FlatAdamW([{"params": tk_probe.parameters(), "lr": 5e-4}]), FlatAdamW([{"params": ob_probe.parameters(), "lr": 5e-4}])

    def tk_step():
        return train_taskonomy_step(model, tk_probe, tk_opt, None, images, target, valid)

    def ob_step():
        return train_objectness_step(model, ob_probe, ob_opt, None, images, mask)

    ms = {"taskonomy": [], "objectness": []}
    for _ in range(3):
        tk_step(); ob_step()
    torch.cuda.synchronize()
    block = max(1, a.steps // 4)
    for _ in range(4):  # alternating blocks
        for name, fn in (("taskonomy", tk_step), ("objectness", ob_step)):
            for _ in range(block):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                last = fn()
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
    assert bool(torch.isfinite(last))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    lines.append(f"(b) whole steps (frozen {a.backbone} forward + DPT k3 probe forward / backward + loss + FlatAdamW), B = {B}, {S}^2, one process, "
                 f"4 alternating blocks of {block} steps each, device events around each step, no pipelining")
    for k in ("taskonomy", "objectness"):
        v = ms[k]
        lines.append(f"  {k:10s} step  median {med[k]:8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f}   = {B / (med[k] * 1e-3):7.1f} img/s at the median")
    lines.append(f"  taskonomy - objectness = {med['taskonomy'] - med['objectness']:+.3f} ms per step (3 output channels against 1, no BatchNorm tail, "
                 f"masked L1 against BCE)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--step-size", type=int, default=512, help="image side of the step comparison")
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--backbone", default="dinov2_b14")
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("taskonomy_bench needs a GPU")
    dev = torch.device("cuda:0")
    lines = [f"Taskonomy kernels and step; {torch.cuda.get_device_name(0)}"]
    kernels(a, dev, lines)
    if not a.skip_steps:
        steps(a, dev, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
