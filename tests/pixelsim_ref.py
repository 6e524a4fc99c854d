"""The fp64 definition of the pixel-level 2AFC baselines (include/mvp_hip.h: mvp_pixel_score) in torch on the CPU: SSIM with the
reference's window (evals/utils/losses.py:203-251: 11 x 11 Gaussian, sigma 1.5, the fp32 outer product of the fp32 1-D window, zero
padding, per channel), PSNR with peak 1, triplet scores, predictions and counts; and the same SSIM written in fp32 conv2d form, which
is used only to measure what torch's own fp32 arithmetic loses on given inputs (the yardstick of the SSIM bound)."""
import math

import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2


def window1d() -> torch.Tensor:
    """[11] fp32: exp(-(k - 5)^2 / (2 * 1.5^2)) rounded to fp32, divided by their fp32 sum."""
    g = torch.tensor([math.exp(-((k - 5) ** 2) / (2 * 1.5 ** 2)) for k in range(11)], dtype=torch.float32)
    return g / g.sum()


def window2d() -> torch.Tensor:
    """[11, 11] fp32: the outer product, rounded to fp32 (what create_window(11, 1)[0, 0] holds)."""
    g = window1d().unsqueeze(1)
    return g.mm(g.t())


def _map(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The SSIM map of a pair [B, C, H, W], in the dtype of ``a``."""
    ch = a.shape[1]
    w = window2d().to(a.dtype).expand(ch, 1, 11, 11).contiguous()

    def filt(x):
        return F.conv2d(x, w, padding=5, groups=ch)

    mu1, mu2 = filt(a), filt(b)
    s1, s2, s12 = filt(a * a) - mu1 * mu1, filt(b * b) - mu2 * mu2, filt(a * b) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def ssim(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """[B, C, H, W] x 2 -> the mean of the map per image pair [B], fp64."""
    return _map(a.double(), b.double()).flatten(1).mean(dim=1)


def ssim_fp32(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The same in fp32 throughout, as the reference's ssim(size_average=False) evaluates: its error against ssim() is torch's own."""
    return _map(a.float(), b.float()).mean(1).mean(1).mean(1)


def psnr(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """[B, C, H, W] x 2 -> 10 log10(1 / mse) per image pair [B], fp64; mse = 0 gives +inf."""
    mse = ((a.double() - b.double()) ** 2).flatten(1).mean(dim=1)
    return 10.0 * torch.log10(1.0 / mse)


METRICS = {"ssim": ssim, "psnr": psnr}


def score(ref: torch.Tensor, left: torch.Tensor, right: torch.Tensor, metric: str):
    """-> (sim [B, 2] fp64, pred [B] int64): pred = 0 where sim(left) > sim(right), else 1 (NaN compares false)."""
    f = METRICS[metric]
    sim = torch.stack((f(ref, left), f(ref, right)), dim=1)
    return sim, torch.where(sim[:, 0] > sim[:, 1], 0, 1)


def counts(label: torch.Tensor, pred: torch.Tensor):
    """[TP, FP, FN, TN] with positive = 1."""
    label, pred = label.reshape(-1).double(), pred.reshape(-1).double()
    return [int(((pred == 1) & (label == 1)).sum()), int(((pred == 1) & (label == 0)).sum()),
            int(((pred == 0) & (label == 1)).sum()), int(((pred == 0) & (label == 0)).sum())]
