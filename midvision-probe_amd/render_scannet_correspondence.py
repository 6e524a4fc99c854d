#!/usr/bin/env python3
"""Entry point mirroring the reference's render_scannet_correspondence.py main (lines 158-328) on MI355X: instantiate the backbone
(output="dense"), one forward per pair on the stacked two views, back-project both depth maps, sample the features at the points
(mvp_pointcloud_sample), match with the fused top-2 kNN + ratio test, report the 2-D / 3-D recalls and the 2 cm recall per
relative-angle bin, append the reference's CSV row.  Data: ScanNet-pairs-shaped synthetic rooms (mvp.corr3d.SyntheticScanNetPairs;
the ScanNet file reader, wandb, the matplotlib figures and the per-instance JSON are out of scope).  Unlike the reference, every
pair is evaluated and the four bin columns hold the bin recalls (INTEGRATION.md lists the deviations).

    python render_scannet_correspondence.py backbone=dinov2_b14 image_height=480 image_width=640 num_instances=16
"""
import os
import sys
from datetime import datetime

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from mvp import config, corr3d, results  # noqa: E402
from mvp import dist as mdist  # noqa: E402


def main(argv):
    cfg = config.compose("scannet_correspondence", argv)
    rank, local, world = mdist.env_setup("nccl")
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(int(cfg["random_seed"]))
    model = config.instantiate(cfg["backbone"], output="dense", return_multilayer=cfg["multilayer"]).to(dev)
    ds = config.instantiate(cfg["dataset"], num_pairs=int(cfg["num_instances"]), image_height=int(cfg["image_height"]),
                            image_width=int(cfg["image_width"]), seed=int(cfg["random_seed"]))
    numbers = corr3d.evaluate_scannet(model, ds, int(cfg["num_corr"]), float(cfg["scale_factor"]), bool(cfg["multilayer"]), rank=rank, world=world)
    if rank == 0:
        for name, v in zip(corr3d.SCANNET_RESULT_NAMES, numbers):
            print(f"{name:>20s}:  {v:.2f}")
        row = [datetime.now().strftime("%d%m%Y-%H%M"), model.checkpoint_name, model.patch_size, str(model.layer), model.output, ds.name,
               str(cfg["num_corr"]), str(cfg["scale_factor"])] + [f"{v:5.02f}" for v in numbers]
        path = results.append_result_csv(os.path.join(str(cfg["output_dir"]), "scannet_correspondence_final.csv"), corr3d.SCANNET_CSV_HEADER, row)
        print(f"results -> {path}")
    if world > 1:
        torch.distributed.destroy_process_group()
    return numbers


if __name__ == "__main__":
    main(sys.argv[1:])
