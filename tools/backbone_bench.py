"""The driver's training step for several ViT backbones side by side: B images at 224^2 (synthetic NYU-shaped batches resident in HBM), the
backbone with return_multilayer (4 taps, train-mode tap BN) -> DepthHead(linear, k = 1, bindepth) -> bilinear -> DepthLoss -> backward ->
FlatAdamW, PIPELINED as train_depth.py runs it (mvp.pipeline: the trainers' default in-flight depth, grouped / span forwards, hipGraph
replay), backbone precision f16x2.  Models: dino_b16 (bench.py's headline), dinov2_b14, dinov2_b14_reg, dinov2_l14 (seeded weights), in
one process, alternating round by round so that clock and thermal drift hit all of them alike.  Each round = STEPS steps between two
barriers (the pipeline starts and ends empty), after WARMUP untimed steps per model (graph capture).

    python tools/backbone_bench.py [--batch 16] [--rounds 5] [--steps 30] [--warmup 8] [--models dino_b16,dinov2_b14,...]

One line per model: median img/s over the rounds, the ratio to dino_b16, the pipeline's shape."""
from __future__ import annotations

import argparse
import os
import statistics
import subprocess
import sys
import time
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "midvision-probe_amd")]

import torch  # noqa: E402

MODELS = {"dino_b16": ("dino", "vitb16", "dense"), "dinov2_b14": ("dinov2", "vitb14", "dense-cls"),
          "dinov2_b14_reg": ("dinov2", "vitb14_reg", "dense-cls"), "dinov2_l14": ("dinov2", "vitl14", "dense-cls"),
          # the same GEMMs; crocov2 adds mvp_rope2d_qkv and the fp32 qkv output per block
          "croco_b16": ("croco", "vitb16", "dense"), "crocov2_b16": ("crocov2", "vitb16", "dense"),
          # 24 block passes per forward (all blocks + fc_norm, then the tapped pass) with a logit bias in attention
          "beit-v2_vitb16": ("beit_v2", "vitb16", "dense"),
          # windowed blocks: two row gathers, fp32 qkv + mvp_relpos_terms, attention with the decomposed bias (SAM); no tap norm
          # (the wrapper refuses add_norm); --size 512 / 1024 for the sizes the encoder is meant for
          "sam_base": ("sam", "vit_b", "dense"), "sam_large": ("sam", "vit_l", "dense"),
          # ConvNeXt-B / ConvNeXt V2-B: four taps of widths 128 ... 1024 resized to one 14 x 14 grid; bf16x3 whatever --precision says, no tap
          # norm (the wrapper refuses add_norm), serial forwards (the engine is not pipelined) (ConvNeXt)
          "convnext_in22k": ("convnext", "in22k", "dense"), "convnext_fcmae": ("convnext", "fcmae_ft_in22k_in1k_384", "dense")}


def build(name, precision, dev):
    from evals.models.dino import DINO
    from evals.models.probes import DepthHead
    from evals.utils.optim import cosine_decay_linear_warmup
    from mvp.optim import FlatAdamW

    dn, mn, out = MODELS[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # seeded random init
        if dn in ("croco", "crocov2"):
            from evals.models.croco import CROCO
            from evals.models.crocov2 import CROCOV2

            model = (CROCO if dn == "croco" else CROCOV2)(model_name=mn, output=out, return_multilayer=True, add_norm=True, precision=precision).to(dev)
        elif dn == "sam":
            from evals.models.sam import SAM

            model = SAM(mn, output=out, return_multilayer=True, precision=precision).to(dev)
        elif dn == "convnext":
            from evals.models.convnext import ConvNext

            model = ConvNext("convnext_base", mn, output=out, return_multilayer=True, precision=precision).to(dev)
        elif dn == "beit_v2":
            from evals.models.beit_v2 import BEiTV2

            model = BEiTV2(model_name=mn, output=out, return_multilayer=True, add_norm=True, precision=precision).to(dev)
        else:
            model = DINO(dino_name=dn, model_name=mn, output=out, return_multilayer=True, add_norm=True, precision=precision).to(dev)
    torch.manual_seed(0)
    probe = DepthHead(feat_dim=model.feat_dim, head_type="linear", kernel_size=1, prediction_type="bindepth", min_depth=0.001, max_depth=10).to(dev)
    opt = FlatAdamW([{"params": probe.parameters(), "lr": 5e-4}])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda e: cosine_decay_linear_warmup(e, 100000, 100))
    return model, probe, opt, sched


def main():
    from evals.utils.losses import DepthLoss
    from mvp.pipeline import pipelined_features
    from mvp.train import train_depth_step

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--precision", default="f16x2")
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--size", type=int, default=224, help="image side (a multiple of every patch size used: 224, 448, ...; SAM: 512, 1024)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, H, W = a.batch, a.size, a.size
    names = a.models.split(",")
    batches = []
    for s in range(4):
        g = torch.Generator().manual_seed(1000 + s)
        depth = torch.rand(B, 1, H, W, generator=g) * 9.9 + 0.05
        depth[torch.rand(B, 1, H, W, generator=g) < 0.1] = 0.0
        batches.append({"image": torch.randn(B, 3, H, W, generator=g).to(dev), "depth": depth.to(dev)})
    runs = {n: build(n, a.precision, dev) for n in names}
    loss_fn = DepthLoss()

    def steps(name, n):
        model, probe, opt, sched = runs[name]
        seq = [batches[i % len(batches)] for i in range(n)]
        for b, f in pipelined_features(model, seq, probe=probe):
            train_depth_step(model, probe, opt, sched, loss_fn, None, b["depth"], feats=f)
        opt.finish_pending()
        torch.cuda.synchronize()

    for n in names:
        steps(n, a.warmup)
    rates = {n: [] for n in names}
    for _ in range(a.rounds):
        for n in names:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(n, a.steps)
            rates[n].append(B * a.steps / (time.perf_counter() - t0))
    try:
        rev = subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "n/a"
    except OSError:
        rev = "n/a"
    print(f"# tools/backbone_bench.py  B={B} {H}x{W} {a.precision} linear k=1 bindepth probe, pipelined; {a.rounds} rounds x {a.steps} steps "
          f"(+{a.warmup} warm-up); tree {rev}; {time.strftime('%Y-%m-%d')}")
    base = statistics.median(rates[names[0]])
    from mvp.pipeline import cached_pipelines

    for n in names:
        r = statistics.median(rates[n])
        pipes = [p for p in cached_pipelines(runs[n][0]).values()]
        shape = f"depth={pipes[0].depth} group={pipes[0].group} span={pipes[0].span}" if pipes else ""
        print(f"{n:16s} {r:8.0f} img/s  ({r / base:.2f}x {names[0]}; {shape}; rounds {', '.join(f'{x:.0f}' for x in rates[n])})")


if __name__ == "__main__":
    main()
