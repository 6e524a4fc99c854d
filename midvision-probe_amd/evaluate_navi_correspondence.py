#!/usr/bin/env python3
"""Entry point mirroring the reference's evaluate_navi_correspondence.py main (lines 121-277) on MI355X: instantiate the backbone
(output="dense"), extract both views' features, match every pair with the fused top-2 kNN + ratio test, report the 3-D / 2-D recalls
and the recall per relative-angle bin, append the reference's CSV row.  Data: NAVI-shaped synthetic pairs (mvp.corr3d.SyntheticNAVI;
the NAVI reader, wandb and the matplotlib visualisation are out of scope).

    python evaluate_navi_correspondence.py backbone=dinov2_b14 image_size=512 num_instances=16
"""
import os
import sys
from datetime import datetime

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from mvp import config, corr3d, results  # noqa: E402
from mvp import dist as mdist  # noqa: E402


def main(argv):
    cfg = config.compose("navi_correspondence", argv)
    rank, local, world = mdist.env_setup("nccl")
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(int(cfg["random_seed"]))
    model = config.instantiate(cfg["backbone"], output="dense", return_multilayer=cfg["multilayer"]).to(dev)
    ds = config.instantiate(cfg["dataset"], num_pairs=int(cfg["num_instances"]), image_size=int(cfg["image_size"]), seed=int(cfg["random_seed"]))
    numbers = corr3d.evaluate_dataset(model, ds, int(cfg["num_corr"]), float(cfg["scale_factor"]), bool(cfg["multilayer"]), rank=rank, world=world)
    if rank == 0:
        for name, v in zip(corr3d.RESULT_NAMES, numbers):
            print(f"{name:>20s}:  {v:.2f}")
        row = [datetime.now().strftime("%d%m%Y-%H%M"), model.checkpoint_name, model.patch_size, str(model.layer), model.output,
               cfg["num_corr"], cfg["scale_factor"], ds.name] + [f"{v:5.02f}" for v in numbers]
        path = results.append_result_csv(os.path.join(str(cfg["output_dir"]), "navi_correspondence_final.csv"), corr3d.CSV_HEADER, row)
        print(f"results -> {path}")
    if world > 1:
        torch.distributed.destroy_process_group()
    return numbers


if __name__ == "__main__":
    main(sys.argv[1:])
