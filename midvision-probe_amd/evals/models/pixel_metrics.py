"""The pixel-level baselines of the 2AFC perceptual-similarity evaluation: PSNR and SSIM as "backbones" (the model types "psnr" and
"ssim" of the reference's evals/datasets/utils.py:get_preprocess, whose preprocessing is ToTensor() alone: values in [0, 1], native
size, no normalisation).  They embed nothing: ``arch == "metric"`` tells mvp.percept.predict_batch to score the images of a triplet
directly (mvp_pixel_score, csrc/pixelsim.hip) in place of a forward and a cosine.

    python evaluate_model_percepture.py backbone=ssim dataset.preprocess=SSIM experiment_model=ssim
"""
from __future__ import annotations

import torch
import torch.nn as nn


class PixelMetric(nn.Module):
    """No parameters.  ``return_cls``, ``return_multilayer``, ``output`` and ``layer`` are what every backbone config and the
    evaluation's command line pass; they are accepted and mean nothing here."""

    arch = "metric"
    metric = ""

    def __init__(self, return_cls=False, return_multilayer=False, output="dense", layer=-1):
        super().__init__()
        self.checkpoint_name = f"${self.metric}$"
        self.preprocess = self.metric.upper()

    def forward(self, ref: torch.Tensor, other: torch.Tensor) -> torch.Tensor:
        """[B, C, H, W] x 2 (fp32 on the device) -> the score of each pair [B], through the kernel of the evaluation."""
        from mvp import percept

        a, b = ref.detach().float().contiguous(), other.detach().float().contiguous()
        sim, _ = percept.score_pixel_triplets(a, b, b, self.metric)
        return sim[:, 0]


class PSNR(PixelMetric):
    """10 log10(1 / mse): the peak is 1 (conventions)."""

    metric = "psnr"


class SSIM(PixelMetric):
    """The reference's evals/utils/losses.py ssim(size_average=False): 11 x 11 Gaussian window, sigma 1.5, zero padding, per channel."""

    metric = "ssim"
