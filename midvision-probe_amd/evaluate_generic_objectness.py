#!/usr/bin/env python3
"""Entry point mirroring the reference's evaluate_generic_objectness.py main (lines 337-422) on MI355X: compose the config, build the
trainval and test sets and the backbone, run MaskCut on every image (mvp.maskcut: four launches per pass, batched, the eigen-solve out
of LDS; with +refine=dense_crf also the reference's dense-CRF post-processing of every pass, mvp.densecrf), print the train and test averages of F-measure / IoU / accuracy / CorLoc and append the reference's row, plus the number of
host-side fallback solves, to <output_dir>/final_results_summary.csv.  Data: VOC-shaped synthetic samples (the VOC file reader, wandb
and the plots are out of scope).

    python evaluate_generic_objectness.py backbone=dino_b16 backbone.return_kqv=true dataset=synthetic_voc
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from evals.models.maskcut_processor import MaskCutProcessor  # noqa: E402
from mvp import config, maskcut, results  # noqa: E402


def main(argv):
    cfg = config.compose("objectness_eval", argv)
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(int(cfg["system"]["random_seed"]))
    trainval_dataset = config.instantiate(cfg["dataset"], split="trainval")
    test_dataset = config.instantiate(cfg["dataset"], split="test")
    model = config.instantiate(cfg["backbone"]).to(dev)
    model.eval()
    fixed_size = int(cfg["dataset"].get("fixed_size", 480))
    processor = MaskCutProcessor(backbone=model, patch_size=int(model.patch_size), tau=0.15, fixed_size=fixed_size,
                                 refine=str(cfg.get("refine", "none")))
    batch_size = int(cfg["batch_size"])
    train_avg, train_fb, n_train = maskcut.predict(processor, trainval_dataset, batch_size, dev)
    print(f"Final training average metrics: {train_avg}  ({n_train} images, {train_fb} fallback solves)")
    test_avg, test_fb, n_test = maskcut.predict(processor, test_dataset, batch_size, dev)
    print(f"Final test average metrics: {test_avg}  ({n_test} images, {test_fb} fallback solves)")
    model_name = getattr(model, "checkpoint_name", cfg["experiment_model"])
    row = [model_name] + [train_avg[k] for k in maskcut.METRICS] + [test_avg[k] for k in maskcut.METRICS] + [train_fb + test_fb]
    path = results.append_result_csv(os.path.join(str(cfg["output_dir"]), "final_results_summary.csv"), maskcut.CSV_HEADER, row)
    print(f"Final results saved to {path}")
    return train_avg, test_avg, train_fb + test_fb


if __name__ == "__main__":
    main(sys.argv[1:])
