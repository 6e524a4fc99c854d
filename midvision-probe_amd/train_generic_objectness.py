#!/usr/bin/env python3
"""Entry point mirroring the reference's train_generic_objectness.py (:350-398 train loop: bilinear resize to the mask, nn.BCELoss,
BinaryHead; :417-492 validation; :608-640 the summary CSV) on synthetic VOC-shaped batches.

    python train_generic_objectness.py backbone=dinov2_b14 probe=binaryhead batch_size=16

Deviations: the run ends by saving ``ckpt.pth`` like train_depth.py / train_snorm.py (the reference saves nothing),
and ``is_eval=True ckpt_path=...`` loads that file and only validates (the reference ignores both keys).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from mvp import checkpoint, config, objectness  # noqa: E402
from mvp.optim import FlatAdamW  # noqa: E402
from mvp.pipeline import freeze_gc, pipelined_features  # noqa: E402
from mvp.train import train_objectness_step  # noqa: E402


def main(argv):
    from evals.datasets import build_loader
    from evals.utils.optim import cosine_decay_linear_warmup
    from mvp.prefetch import DevicePrefetcher

    cfg = config.compose("objectness_train", argv)
    if int(cfg["system"]["num_gpus"]) > 1:
        # train_generic_objectness.py:645-647 spawns ranks that never initialise a process group before wrapping in DDP (:553-555)
        raise NotImplementedError("system.num_gpus > 1: the reference's multi-process objectness path creates no process group and cannot "
                                  "have run; this trainer is single-GPU")
    if float(cfg["optimizer"].get("model_lr", 0.0)) != 0.0:
        raise NotImplementedError("optimizer.model_lr != 0 (backbone fine-tuning) is outside the frozen-backbone hot path")
    torch.manual_seed(int(cfg["system"]["random_seed"]))
    dev = torch.device("cuda", torch.cuda.current_device())
    ds, B = cfg["dataset"], cfg["batch_size"]
    workers = int(cfg.get("num_workers", 1))
    # train_generic_objectness.py:517-529: shuffled trainval loader, ordered test loader (build_loader shuffles only the split "train")
    train_set = config.instantiate(ds, split="trainval")
    loader = torch.utils.data.DataLoader(train_set, B, shuffle=True, num_workers=workers, pin_memory=True, persistent_workers=workers > 0)
    test_loader = build_loader(ds, "test", B, num_workers=workers)
    nb = len(loader)
    bcfg = dict(cfg["backbone"])
    if cfg["probe"].get("head_type", "dpt") != "linear":
        bcfg.setdefault("return_multilayer", True)  # the dpt / multiscale trunks take four maps (the reference needs the override spelt out)
    model = config.instantiate(bcfg)
    model.eval()                                                    # :532 — the backbone; the probe is never put in eval mode
    probe = config.instantiate(cfg["probe"], feat_dim=model.feat_dim)
    model, probe = model.to(dev), probe.to(dev)
    if "sam" in model.checkpoint_name or "vit-mae" in model.checkpoint_name:  # :547-550
        model.resize_pos_embed(image_size=tuple(train_set[0]["original_image"].shape[-2:]))
    opt = FlatAdamW([{"params": probe.parameters(), "lr": cfg["optimizer"]["probe_lr"]}])
    n_ep = cfg["optimizer"]["n_epochs"]
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda e: cosine_decay_linear_warmup(e, n_ep * nb, cfg["optimizer"]["warmup_epochs"] * nb))
    freeze_gc()  # no full-heap collector pause inside the loop
    is_eval = bool(cfg.get("is_eval", False))
    if is_eval:
        ck = str(cfg.get("ckpt_path", "") or "").replace("\\$", "$")
        if not ck:
            raise SystemExit("is_eval=True needs ckpt_path=<.../ckpt.pth> (refusing to validate a randomly initialised probe)")
        checkpoint.load_checkpoint(ck, model, probe, load_model=True)
    out = os.path.join(cfg["output_dir"], "objectness_exps", f"{model.checkpoint_name}_{probe.name}".replace("$", ""))
    for ep in range(0 if is_eval else n_ep):
        tot = 0.0
        batches = DevicePrefetcher(loader, dev, keys=("original_image", "gt_binary_mask"))
        for batch, feats in pipelined_features(model, batches, image_key="original_image", probe=probe):  # the next forward is already in flight
            tot += train_objectness_step(model, probe, opt, sched, None, batch["gt_binary_mask"].float(), feats=feats).item()
        print(f"epoch {ep} train loss {tot / nb:.4f}")
    opt.finish_pending()
    if not is_eval:
        # saved BEFORE validation: the probe stays in train mode there (as in the reference), so validating moves its running statistics
        print("saved", checkpoint.save_checkpoint(os.path.join(out, "ckpt.pth"), cfg, model, probe))
    avg = objectness.validation(model, probe, test_loader)
    print("test " + " ".join(f"{k} {float(avg[k]):.6f}" for k in objectness.METRICS))
    print("results ->", objectness.append_summary_csv(cfg["output_dir"], cfg["model_name"], avg, ds.get("name", "voc")))


if __name__ == "__main__":
    main(sys.argv[1:])
