#!/usr/bin/env python3
"""Entry point mirroring the reference's evaluate_model_percepture.py main (lines 170-240) on MI355X: compose the config, build the
test loader and the backbone, score every triplet (mvp.percept.predict_batch: one stacked forward per batch, the fused pooled-cosine
kernel behind it, predictions and counts on the device until the end), print the metrics and append the reference's row to
<output_dir>/final_results_summary.csv.  Data: 2AFC-shaped synthetic triplets (the NIGHTS reader and wandb are out of scope).

    python evaluate_model_percepture.py backbone=dino_b16 backbone.return_cls=True experiment_model=dino_b16
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from evals.datasets.builder import build_loader  # noqa: E402
from mvp import config, percept, results  # noqa: E402
from mvp import dist as mdist  # noqa: E402


def main(argv):
    cfg = config.compose("model_percepture", argv)
    rank, local, world = mdist.env_setup("nccl")
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(int(cfg["system"]["random_seed"]))
    # every rank walks the whole loader and keeps batches rank, rank + world, ... (percept.shard_batches): no DistributedSampler
    test_loader = build_loader(cfg["dataset"], "test", int(cfg["batch_size"]), num_workers=0)
    model = config.instantiate(cfg["backbone"]).to(dev)
    model.eval()
    test_results, test_metrics, test_errors = percept.predict_batch(model=model, dataloader=test_loader, output_dir=cfg["output_dir"],
                                                                    wandb_use=False, rank=rank, world=world)
    if rank == 0:
        print(f"Test metrics: {test_metrics}  ({len(test_results)} triplets, {len(test_errors)} batch errors)")
        row = [cfg["experiment_model"]] + [test_metrics[k] for k in percept.METRIC_NAMES]
        path = results.append_result_csv(os.path.join(str(cfg["output_dir"]), "final_results_summary.csv"), percept.CSV_HEADER, row)
        print(f"Final results saved to {path}")
    if world > 1:
        torch.distributed.destroy_process_group()
    return test_results, test_metrics, test_errors


if __name__ == "__main__":
    main(sys.argv[1:])
