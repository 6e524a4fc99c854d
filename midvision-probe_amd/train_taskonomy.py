#!/usr/bin/env python3
"""Entry point for Taskonomy pixel-to-pixel probing.  The reference ships the parts (configs/taskonomy_training.yaml,
evals.datasets.taskonomy, evals.models.probes.TaskonomyHead, evals.utils.losses.MaskedL1Loss, the curvature and reshading metrics) but
no trainer; this one follows train_snorm.py's shape with the conventions INTEGRATION.md lists (first C_t channels of the probe, bilinear
resize, MaskedL1Loss under the valid mask, no augmentation, probe in eval mode for validation).

    python train_taskonomy.py backbone=dinov2_b14 probe=taskonomy_dpt dataset.task=reshading batch_size=16
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from mvp import checkpoint, config, taskonomy  # noqa: E402
from mvp import dist as mdist  # noqa: E402
from mvp.optim import FlatAdamW  # noqa: E402
from mvp.pipeline import freeze_gc, pipelined_features  # noqa: E402
from mvp.train import train_taskonomy_step  # noqa: E402


def main(argv):
    from evals.datasets import build_loader
    from evals.utils.optim import cosine_decay_linear_warmup
    from mvp.prefetch import DevicePrefetcher

    cfg = config.compose("taskonomy_training", argv)
    if float(cfg["optimizer"].get("model_lr", 0.0)) != 0.0:
        raise NotImplementedError("optimizer.model_lr != 0 (backbone fine-tuning) is outside the frozen-backbone hot path")
    rank, local, world = mdist.env_setup("nccl")
    torch.manual_seed(int(cfg["system"]["random_seed"]))
    dev = torch.device("cuda", torch.cuda.current_device())
    ds, B = cfg["dataset"], cfg["batch_size"]
    task = ds["task"]
    ct = taskonomy.target_channels("depth_euclidean" if task == "depth" else task)
    if int(cfg["probe"].get("output_dim", 1)) < ct:
        raise ValueError(f"probe.output_dim={cfg['probe'].get('output_dim', 1)} is less than the {ct} channels of task {task!r}")
    workers = int(cfg.get("num_workers", 2))
    loader = build_loader(ds, "train", B, num_gpus=world, num_workers=workers)
    test_loader = build_loader(ds, "test", B, num_workers=workers)
    nb = len(loader)
    keys = ("rgb", task, "mask_valid")

    def device_batches(ld):
        # raw loaders hand out undecoded bytes: normalised and decoded on the device, after the H2D copy
        pre = DevicePrefetcher(ld, dev, keys=keys)
        return taskonomy.DeviceTaskTransform(pre, task, image_mean=ds.get("image_mean", "imagenet")) if ds.get("raw") else pre

    bcfg = dict(cfg["backbone"])
    if cfg["probe"].get("head_type", "dpt") != "linear":
        bcfg.setdefault("return_multilayer", True)  # the dpt / multiscale trunks take four maps
    model = config.instantiate(bcfg)
    model.eval()
    probe = config.instantiate(cfg["probe"], feat_dim=model.feat_dim)
    model, probe = model.to(dev), probe.to(dev)
    if "sam" in model.checkpoint_name or "vit-mae" in model.checkpoint_name:
        model.resize_pos_embed(image_size=tuple(loader.dataset[0]["rgb"].shape[:2] if ds.get("raw") else loader.dataset[0]["rgb"].shape[-2:]))
    opt = FlatAdamW([{"params": probe.parameters(), "lr": cfg["optimizer"]["probe_lr"]}], overlap_comm=world > 1)
    n_ep = cfg["optimizer"]["n_epochs"]
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda e: cosine_decay_linear_warmup(e, n_ep * nb, cfg["optimizer"]["warmup_epochs"] * nb))
    freeze_gc()  # no full-heap collector pause inside the loop
    is_eval = bool(cfg.get("is_eval", False))
    if is_eval:
        ck = str(cfg.get("ckpt_path", "") or "").replace("\\$", "$")
        if not ck:
            raise SystemExit("is_eval=True needs ckpt_path=<.../ckpt.pth> (refusing to validate a randomly initialised probe)")
        checkpoint.load_checkpoint(ck, model, probe, load_model=True)
    batches = device_batches(loader)
    for ep in range(0 if is_eval else n_ep):
        tot = 0.0
        if world > 1:
            loader.sampler.set_epoch(ep)
        probe.train()
        for batch, feats in pipelined_features(model, batches, image_key="rgb", probe=probe):  # the next forward is already in flight
            tot += train_taskonomy_step(model, probe, opt, sched, None, batch[task], batch["mask_valid"], feats=feats).item()
        if rank == 0:
            print(f"epoch {ep} train loss {tot / nb:.4f}")
    opt.finish_pending()
    if rank == 0:
        out = os.path.join(cfg["output_dir"], "taskonomy_exps", f"{model.checkpoint_name}_{probe.name}_{task}".replace("$", ""))
        if not is_eval:
            print("saved", checkpoint.save_checkpoint(os.path.join(out, "ckpt.pth"), cfg, model, probe))
        avg = taskonomy.validation(model, probe, device_batches(test_loader), task)
        print("test " + " ".join(f"{k} {float(v):.6f}" for k, v in avg.items()))
        print("results ->", taskonomy.append_result_csv(cfg["output_dir"], task, cfg["experiment_model"], avg))
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1:])
