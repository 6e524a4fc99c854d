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

from mvp import checkpoint, config, objectness, trainer  # noqa: E402
from mvp.train import train_objectness_step  # noqa: E402


def main(argv):
    from evals.datasets import build_loader
    from mvp.prefetch import DevicePrefetcher

    cfg = trainer.compose_and_check("objectness_train", argv, single_gpu_only=True)
    ck = trainer.checkpoint_for_eval(cfg)
    torch.manual_seed(int(cfg["system"]["random_seed"]))
    dev = torch.device("cuda", torch.cuda.current_device())
    ds, B = cfg["dataset"], cfg["batch_size"]
    workers = int(cfg.get("num_workers", 1))
    # train_generic_objectness.py:517-529: shuffled trainval loader, ordered test loader (build_loader shuffles only the split "train")
    train_set = config.instantiate(ds, split="trainval")
    loader = torch.utils.data.DataLoader(train_set, B, shuffle=True, num_workers=workers, pin_memory=True, persistent_workers=workers > 0)
    test_loader = build_loader(ds, "test", B, num_workers=workers)
    model, probe = trainer.build_model_and_probe(cfg, dev, multilayer_default=True, eval_backbone=True)
    trainer.resize_pos_embed_for(model, lambda: train_set[0]["original_image"].shape[-2:])
    opt, sched = trainer.build_optimizer(cfg, probe, len(loader), world=1)
    trainer.load_for_eval(ck, model, probe, load_model=True)
    trainer.run_epochs(model, probe, 0 if ck else cfg["optimizer"]["n_epochs"],
                       lambda ep: DevicePrefetcher(loader, dev, keys=("original_image", "gt_binary_mask")),  # a fresh prefetcher per epoch
                       lambda batch, feats: train_objectness_step(model, probe, opt, sched, None, batch["gt_binary_mask"].float(), feats=feats),
                       loader=loader, image_key="original_image")
    opt.finish_pending()
    if not ck:
        # saved BEFORE validation: the probe stays in train mode there (as in the reference), so validating moves its running statistics
        print("saved", checkpoint.save_checkpoint(os.path.join(trainer.experiment_dir(cfg, "objectness", model, probe), "ckpt.pth"), cfg, model, probe))
    avg = objectness.validation(model, probe, test_loader)
    print("test " + " ".join(f"{k} {float(avg[k]):.6f}" for k in objectness.METRICS))
    print("results ->", objectness.append_summary_csv(cfg["output_dir"], cfg["model_name"], avg, ds.get("name", "voc")))


if __name__ == "__main__":
    main(sys.argv[1:])
