#!/usr/bin/env python3
"""Entry point mirroring the reference's train_snorm.py (train_snorm.py:86-120 loop; bicubic upsample,
uncertainty-aware angular loss, SurfaceNormalHead) on synthetic NYU-shaped batches.

    python train_snorm.py backbone=dino_b16 +backbone.return_multilayer=True probe=snorm_dpt batch_size=8
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from mvp import checkpoint, trainer  # noqa: E402
from mvp import dist as mdist  # noqa: E402
from mvp.train import train_snorm_step  # noqa: E402


def main(argv):
    from evals.datasets import build_loader
    from evals.utils.metrics import evaluate_surface_norm
    from mvp import functional as MF
    from mvp.prefetch import DevicePrefetcher

    cfg = trainer.compose_and_check("snorm_training", argv)
    ck = trainer.checkpoint_for_eval(cfg)
    rank, local, world = mdist.env_setup("nccl")
    torch.manual_seed(int(cfg["system"]["random_seed"]))
    dev = torch.device("cuda", torch.cuda.current_device())
    ds = cfg["dataset"]
    hw, B = tuple(ds["image_size"]), cfg["batch_size"]
    loader = build_loader(dict(ds, batch_size=B), "train", B, num_gpus=world, num_workers=cfg.get("num_workers", 2))
    augmented, wrap_valid = trainer.nyu_device_batches(cfg, loader, dev, rank, valid_keys=("image", "depth", "snorm"))
    model, probe = trainer.build_model_and_probe(cfg, dev, multilayer_default=False, eval_backbone=False)
    # no trainer.resize_pos_embed_for here: this script has never resized the SAM / MAE position tables (train_snorm.py:622 does)
    opt, sched = trainer.build_optimizer(cfg, probe, len(loader), world)
    trainer.load_for_eval(ck, model, probe, load_model=True)

    def step(batch, feats):
        mask = batch["depth"] > 0                                   # train_snorm.py:95
        return train_snorm_step(model, probe, opt, sched, None, batch["snorm"], mask, feats=feats)

    trainer.run_epochs(model, probe, 0 if ck else cfg["optimizer"]["n_epochs"],
                       lambda ep: augmented if augmented is not None else DevicePrefetcher(loader, dev), step, loader=loader, world=world, rank=rank,
                       on_epoch=None if augmented is None else augmented.set_epoch)  # the epoch enters the draws' seed (and reaches the sampler again)
    opt.finish_pending()
    if rank == 0:
        model.eval(); probe.eval()
        b = next(iter(wrap_valid(build_loader(dict(ds, num_batches=1, batch_size=B), "valid", B))))
        with torch.no_grad():
            pred = MF.interpolate(probe(model(b["image"].to(dev))).contiguous(), size=hw, mode="bicubic")
        gm, _, _ = evaluate_surface_norm(pred, b["snorm"].to(dev), None, image_average=True, is_navi=True)
        print("valid " + " ".join(f"{k} {float(v):.4f}" for k, v in gm.items()))
        if not ck:
            print("saved", checkpoint.save_checkpoint(os.path.join(trainer.experiment_dir(cfg, "snorm", model, probe), "ckpt.pth"), cfg, model, probe))
    trainer.finish(world)


if __name__ == "__main__":
    main(sys.argv[1:])
