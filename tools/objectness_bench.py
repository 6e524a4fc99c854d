#!/usr/bin/env python3
"""Device-side timing of the objectness probe's tail (csrc/objectness.hip) at the workload's own shapes, and the step it belongs to
beside the existing sigmoid-depth DPT step.

    python tools/objectness_bench.py [--batch 16] [--size 480] [--launches 200] [--steps 20] [--out profiles/objectness_step.txt]

(a) The kernels: the 1-channel 280 x 280 logit map of dinov2_b14 + DPT at 480^2 (the map BinaryHead normalises before DPT's nearest
    x2; channels-last rows of ld = 4 floats, as the trunk writes it) for mvp_bn_act_fwd / _bwd, B x 480 x 480 for mvp_bce_loss_fwd_bwd
    and mvp_binary_counts.  ``--launches`` back-to-back calls between two device events after a warm-up; per call: the time, the bytes
    the algorithm must move over that time, and that rate as a share of the bandwidth bound (HBM peak 8.0 TB/s; a float4 copy
    measures 6.29 TB/s on this part).  The depth tail the step comparison needs (depth_sigmoid fwd / bwd, DepthLoss) and the two
    resizes both steps share are timed the same way.
(b) The step: train_objectness_step (BinaryHead dpt k3, 1 channel) and train_depth_step (DepthHead sigdepth dpt k3), same backbone,
    batch and process, in alternating blocks; median step time by device events around whole steps.  The two differ in the tail
    only, so the difference of the medians is to be read against the difference of the summed tail kernels of (a).
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


def per_call_ms(fn, launches, warmup=10):
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


def kernels(a, dev, lines):
    from mvp import lib, ops

    B, S = a.batch, a.size
    side = S // 14 * 8  # dinov2_b14: S / 14 tokens a side, DPT's fusion blocks bring them to x8 before the last nearest x2
    HW, P, N = side * side, B * side * side, B * S * S
    g = torch.Generator().manual_seed(0)
    x = torch.randn(P, 4, generator=g).to(dev)
    y, gy, gx = torch.empty(B, 1, HW, device=dev), torch.randn(B, 1, HW, generator=g).to(dev), torch.empty(P, 4, device=dev)
    gamma, beta = torch.ones(1, device=dev), torch.zeros(1, device=dev)
    rm, rv, nbt = torch.zeros(1, device=dev), torch.ones(1, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    stats, ws = torch.empty(3, device=dev), ops.bn_act_workspace(dev)
    dg, db = torch.empty(1, device=dev), torch.empty(1, device=dev)
    kw = dict(gamma=gamma, beta=beta, stats=stats, workspace=ws)
    pred = (torch.rand(N, generator=g) * 0.98 + 0.01).to(dev)
    tgt = (torch.rand(N, generator=g) < 0.4).float().to(dev)
    loss, grad = torch.empty(1, device=dev), torch.empty(N, device=dev)
    bws = torch.empty(lib.BCE_WORKSPACE_BYTES // 8, dtype=torch.float64, device=dev)
    cnt = torch.empty(1, 4, dtype=torch.int64, device=dev)
    lg, depth, gl = torch.randn(P, generator=g).to(dev), torch.empty(P, device=dev), torch.empty(P, device=dev)
    dtgt = (torch.rand(B, S * S, generator=g) * 9 + 0.5).to(dev)
    dpred = (torch.rand(B, S * S, generator=g) * 9 + 0.5).to(dev)
    dl, dgrad = torch.empty(4, device=dev), torch.empty(B, S * S, device=dev)
    dws = torch.empty(ops.depth_loss_workspace_bytes(B, S * S) // 4 + 4, device=dev)
    up, full = torch.randn(B, 1, 2 * side, 2 * side, generator=g).to(dev), torch.empty(B, 1, S, S, device=dev)
    gup = torch.empty_like(up)
    BIL = lib.RESIZE_BILINEAR
    rows = [
        # name, call, bytes the algorithm must move, note
        ("bn_act_fwd  train sigmoid", lambda: ops.bn_act_fwd(x, y, B, HW, 1, 4, lib.BN_ACT_SIGMOID, True, running_mean=rm, running_var=rv, num_batches_tracked=nbt, n=4 * P, **kw),
         12 * P, f"x twice + y once, 4 B each, {P} pixels (the ld = 4 rows make the two reads 16 B each in lines fetched: {36 * P / 1e6:.1f} MB)"),
        ("bn_act_fwd  eval sigmoid", lambda: ops.bn_act_fwd(x, y, B, HW, 1, 4, lib.BN_ACT_SIGMOID, False, running_mean=rm, running_var=rv, **kw), 8 * P, "x + y"),
        ("bn_act_bwd  train sigmoid", lambda: ops.bn_act_bwd(x, gy, gx, B, HW, 1, 4, lib.BN_ACT_SIGMOID, True, grad_gamma=dg, grad_beta=db, **kw),
         32 * P, "x and grad_y twice, grad_x rows of 16 B once"),
        ("bce_loss_fwd_bwd", lambda: ops.bce_loss(pred, tgt, loss, grad, bws, N), 12 * N, f"pred + target + grad_pred, {N} pixels"),
        ("binary_counts", lambda: ops.binary_counts(pred, tgt, cnt, 1, N, 0.5), 8 * N, "pred + gt"),
        ("depth_sigmoid fwd", lambda: ops.depth_predict_fwd(lg, depth, None, P, 1, 0.001, 10.0, 1), 8 * P, "the depth step's tail"),
        ("depth_sigmoid bwd", lambda: ops.depth_predict_bwd(lg, depth, None, gy, gl, P, 1, 0.001, 10.0, 1), 12 * P, "the depth step's tail"),
        ("depth_loss_fwd_bwd", lambda: ops.depth_loss(dpred, dtgt, dl, dgrad, dws, B, S * S), 12 * N, "the depth step's tail"),
        ("bilinear resize fwd", lambda: ops.resize(up, full, B, 2 * side, 2 * side, S, S, BIL), 4 * (4 * P + N), "shared by both steps"),
        ("bilinear resize bwd", lambda: ops.resize(full, gup, B, 2 * side, 2 * side, S, S, BIL, backward=True), 4 * (4 * P + N), "shared by both steps"),
    ]
    lines.append(f"(a) kernels at B = {B}, {S}^2: logit map {side} x {side} ([{P}, 4] rows), masks {S} x {S}; {a.launches} back-to-back calls between two device events")
    t = {}
    for name, fn, nbytes, note in rows:
        ms = per_call_ms(fn, a.launches)
        t[name] = ms
        rate = nbytes / (ms * 1e-3)
        lines.append(f"  {name:27s} {ms * 1e3:8.1f} us   {nbytes / 1e6:7.1f} MB must move -> {rate / 1e12:5.2f} TB/s = {100 * rate / HBM_PEAK:4.1f} % of the "
                     f"bandwidth bound (8.0 TB/s HBM peak)   [{note}]")
    obj = t["bn_act_fwd  train sigmoid"] + t["bn_act_bwd  train sigmoid"] + t["bce_loss_fwd_bwd"]
    dep = t["depth_sigmoid fwd"] + t["depth_sigmoid bwd"] + t["depth_loss_fwd_bwd"]
    lines.append(f"  tails: objectness (bn_act fwd + bwd + bce) {obj * 1e3:.1f} us; depth (sigmoid fwd + bwd + DepthLoss) {dep * 1e3:.1f} us; "
                 f"difference {1e3 * (obj - dep):+.1f} us; the two resizes both steps run {1e3 * (t['bilinear resize fwd'] + t['bilinear resize bwd']):.1f} us")
    return obj - dep


def steps(a, dev, lines, tail_diff_ms):
    from evals.models.probes import BinaryHead, DepthHead
    from evals.utils.losses import DepthLoss
    from mvp import config
    from mvp.optim import FlatAdamW
    from mvp.train import train_depth_step, train_objectness_step

    B, S = a.batch, a.size
    model = config.instantiate(config.compose("objectness_train", [f"backbone={a.backbone}"])["backbone"], return_multilayer=True).to(dev).eval()
    g = torch.Generator().manual_seed(1)
    images = torch.randn(B, 3, S, S, generator=g).to(dev)
    mask = (torch.rand(B, 1, S, S, generator=g) < 0.4).float().to(dev)
    depth = (torch.rand(B, 1, S, S, generator=g) * 9 + 0.5).to(dev)
    bin_probe = BinaryHead(feat_dim=model.feat_dim, head_type="dpt", kernel_size=3, output_dim=1).to(dev)
    dep_probe = DepthHead(feat_dim=model.feat_dim, head_type="dpt", kernel_size=3, prediction_type="sigdepth").to(dev)
    bin_opt, dep_opt = FlatAdamW([{"params": bin_probe.parameters(), "lr": 5e-4}]), FlatAdamW([{"params": dep_probe.parameters(), "lr": 5e-4}])
    loss_fn = DepthLoss()

    def obj_step():
        return train_objectness_step(model, bin_probe, bin_opt, None, images, mask)

    def dep_step():
        return train_depth_step(model, dep_probe, dep_opt, None, loss_fn, images, depth.clone())

    ms = {"objectness": [], "depth": []}
    for _ in range(3):
        obj_step(); dep_step()
    torch.cuda.synchronize()
    block = max(1, a.steps // 4)
    for _ in range(4):  # alternating blocks
        for name, fn in (("objectness", obj_step), ("depth", dep_step)):
            for _ in range(block):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                last = fn()
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
    assert bool(torch.isfinite(last))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    lines.append(f"(b) whole steps (frozen {a.backbone} forward + DPT probe forward / backward + loss + FlatAdamW), B = {B}, {S}^2, one process, "
                 f"4 alternating blocks of {block} steps each, device events around each step, no pipelining")
    for k in ("objectness", "depth"):
        v = ms[k]
        lines.append(f"  {k:10s} step  median {med[k]:8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f}   = {B / (med[k] * 1e-3):7.1f} img/s at the median")
    lines.append(f"  objectness - depth = {med['objectness'] - med['depth']:+.3f} ms per step; the tails of (a) differ by {tail_diff_ms:+.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--backbone", default="dinov2_b14")
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("objectness_bench needs a GPU")
    dev = torch.device("cuda:0")
    lines = [f"objectness probe tail: kernels and step; {torch.cuda.get_device_name(0)}"]
    diff = kernels(a, dev, lines)
    if not a.skip_steps:
        steps(a, dev, lines, diff)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
