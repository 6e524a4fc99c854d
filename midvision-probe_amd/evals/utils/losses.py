"""evals.utils.losses — drop-in for the losses the trainers use
(evals/utils/losses.py:54-74,77-94,97-182), forward + analytic backward in HIP kernels, and for its SSIM (losses.py:203-288),
forward only."""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from mvp import functional as MF


class DepthLoss(nn.Module):
    """Reference: losses.py:97-111.  10*sig_loss + 0.5*gradient_loss, quirks Q1/Q2 included
    (target is modified in place)."""

    def __init__(self, weight_sig=10.0, weight_grad=0.5, max_depth=10):
        super().__init__()
        self.sig_w, self.grad_w, self.max_depth = weight_sig, weight_grad, max_depth

    def forward(self, pred, target):
        return MF.depth_loss(pred, target, self.sig_w, self.grad_w, self.max_depth)


class MaskedL1Loss(nn.Module):
    """Reference: losses.py:77-94.  ``mask_valid`` None: every element counts; a one-channel mask is repeated over the channels."""

    def __init__(self):
        super().__init__()

    def forward(self, preds, target, mask_valid=None):
        return MF.masked_l1_loss(preds, target, mask_valid)


def sig_loss(depth_pr, depth_gt, sigma=0.85, eps=0.001, only_mean=False):
    """Reference: losses.py:54-74 (as DepthLoss with the gradient term weighted 0).  ``only_mean`` is accepted and unused,
    exactly as in the reference (losses.py:54: the flag never reaches the arithmetic)."""
    if sigma != 0.85 or eps != 0.001:
        raise NotImplementedError("sig_loss: only the reference defaults are compiled in")
    return MF.depth_loss(depth_pr, depth_gt, 1.0, 0.0, float("inf"))


def angular_loss(snorm_pr, snorm_gt, mask, uncertainty_aware=False, eps=1e-4):
    """Reference: losses.py:157-182."""
    return MF.angular_loss(snorm_pr, snorm_gt, mask, uncertainty_aware, eps)


def gaussian(window_size, sigma):
    """Reference: losses.py:203-210.  exp(-(k - window_size // 2)^2 / (2 sigma^2)), rounded to fp32 and divided by their fp32 sum."""
    g = torch.tensor([math.exp(-((k - window_size // 2) ** 2) / float(2 * sigma**2)) for k in range(window_size)], dtype=torch.float32)
    return g / g.sum()


def create_window(window_size, channel):
    """Reference: losses.py:213-219 -> [channel, 1, window_size, window_size] fp32: the outer product of gaussian(window_size, 1.5) with
    itself, the same for every channel.  (mvp_pixel_score holds gaussian(11, 1.5) itself and filters separably.)"""
    g = gaussian(window_size, 1.5).unsqueeze(1)
    return g.mm(g.t()).float().unsqueeze(0).unsqueeze(0).expand(channel, 1, window_size, window_size).contiguous()


def ssim(img1, img2, window_size=11, size_average=True):
    """Reference: losses.py:280-288 on device tensors [B, C, H, W], forward only (mvp_pixel_score; the result has no grad_fn).
    ``size_average=False``: the score of each image pair [B]; True: their mean, which is the reference's mean over the whole map
    because all images have one size."""
    if window_size != 11:
        raise NotImplementedError("ssim: only the reference's default window (11 x 11, sigma 1.5) is compiled in")
    if img1.requires_grad or img2.requires_grad:
        raise NotImplementedError("ssim is forward only in this build (no SSIM backward): detach the inputs")
    from mvp import percept

    a, b = img1.float().contiguous(), img2.float().contiguous()
    per_image = percept.score_pixel_triplets(a, b, b, "ssim")[0][:, 0]
    return per_image.mean() if size_average else per_image


class SSIM(nn.Module):
    """Reference: losses.py:254-277."""

    def __init__(self, window_size=11, size_average=True):
        super().__init__()
        if window_size != 11:
            raise NotImplementedError("SSIM: only the reference's default window (11 x 11, sigma 1.5) is compiled in")
        self.window_size, self.size_average = window_size, size_average

    def forward(self, img1, img2):
        return ssim(img1, img2, self.window_size, self.size_average)
