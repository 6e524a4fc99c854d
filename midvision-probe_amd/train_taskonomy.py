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

from mvp import checkpoint, taskonomy, trainer  # noqa: E402
from mvp import dist as mdist  # noqa: E402
from mvp.train import train_taskonomy_step  # noqa: E402


def main(argv):
    from evals.datasets import build_loader
    from mvp.prefetch import DevicePrefetcher

    cfg = trainer.compose_and_check("taskonomy_training", argv)
    ck = trainer.checkpoint_for_eval(cfg)
    rank, local, world = mdist.env_setup("nccl")
    torch.manual_seed(int(cfg["system"]["random_seed"]))
    dev = torch.device("cuda", torch.cuda.current_device())
    ds, B = cfg["dataset"], cfg["batch_size"]
    task = ds["task"]
    ct = taskonomy.target_channels(taskonomy.kernel_task(task))
    if int(cfg["probe"].get("output_dim", 1)) < ct:
        raise ValueError(f"probe.output_dim={cfg['probe'].get('output_dim', 1)} is less than the {ct} channels of task {task!r}")
    workers = int(cfg.get("num_workers", 2))
    loader = build_loader(ds, "train", B, num_gpus=world, num_workers=workers)
    test_loader = build_loader(ds, "test", B, num_workers=workers)

    def device_batches(ld):
        # raw loaders hand out undecoded bytes: normalised and decoded on the device, after the H2D copy
        pre = DevicePrefetcher(ld, dev, keys=("rgb", task, "mask_valid"))
        return taskonomy.DeviceTaskTransform(pre, task, image_mean=ds.get("image_mean", "imagenet")) if ds.get("raw") else pre

    model, probe = trainer.build_model_and_probe(cfg, dev, multilayer_default=True, eval_backbone=True)
    trainer.resize_pos_embed_for(model, lambda: loader.dataset[0]["rgb"].shape[:2] if ds.get("raw") else loader.dataset[0]["rgb"].shape[-2:])
    opt, sched = trainer.build_optimizer(cfg, probe, len(loader), world)
    trainer.load_for_eval(ck, model, probe, load_model=True)
    batches = device_batches(loader)  # one prefetcher (and transform) serves every epoch
    trainer.run_epochs(model, probe, 0 if ck else cfg["optimizer"]["n_epochs"], lambda ep: batches,
                       lambda batch, feats: train_taskonomy_step(model, probe, opt, sched, None, batch[task], batch["mask_valid"], feats=feats),
                       loader=loader, image_key="rgb", world=world, rank=rank, on_epoch=lambda ep: probe.train())
    opt.finish_pending()
    if rank == 0:
        if not ck:
            # saved, then validated in eval mode (taskonomy.validation): the running statistics in the file are those of training
            print("saved", checkpoint.save_checkpoint(os.path.join(trainer.experiment_dir(cfg, "taskonomy", model, probe, task), "ckpt.pth"), cfg, model, probe))
        avg = taskonomy.validation(model, probe, device_batches(test_loader), task)
        print("test " + " ".join(f"{k} {float(v):.6f}" for k, v in avg.items()))
        print("results ->", taskonomy.append_result_csv(cfg["output_dir"], task, cfg["experiment_model"], avg))
    trainer.finish(world)


if __name__ == "__main__":
    main(sys.argv[1:])
