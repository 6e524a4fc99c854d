"""fp64 restatement of the ConvNeXt / ConvNeXt V2 trunk and of the reference wrapper around it (evals/models/convnext.py:81-108),
on an engine-layout state dict (mvp/convnext.py: timm's key layout).  Plain torch in float64 on the CPU: the oracle of the GPU tests and,
through tests/test_convnext_cpu.py, itself held to goldens made with transformers' ConvNextModel / ConvNextV2Model."""
from __future__ import annotations

import torch
import torch.nn.functional as F

EPS = 1e-6


def dwconv7_ln(x, w, b, gamma, beta, eps=EPS):
    """x [B, H, W, C] channels-last -> LayerNorm_C(depthwise 7x7, padding 3) [B, H, W, C], float64."""
    x, w, b, gamma, beta = (t.double() for t in (x, w, b, gamma, beta))
    C = x.shape[-1]
    y = F.conv2d(x.permute(0, 3, 1, 2), w.reshape(C, 1, 7, 7), b, padding=3, groups=C).permute(0, 2, 3, 1)
    return F.layer_norm(y, (C,), gamma, beta, eps)


def dwconv7(x, w, b):
    """The convolution alone (channels-last in and out), float64."""
    C = x.shape[-1]
    return F.conv2d(x.double().permute(0, 3, 1, 2), w.double().reshape(C, 1, 7, 7), b.double(), padding=3, groups=C).permute(0, 2, 3, 1)


def grn_stats(h):
    """h [B, HW, C4] -> (G [B, C4], N [B, C4]): G = ||h||_2 over HW, N = G / (mean_c G + 1e-6)."""
    G = h.double().pow(2).sum(dim=1).sqrt()
    return G, G / (G.mean(dim=-1, keepdim=True) + 1e-6)


def grn_apply(h, N, gamma, beta):
    h = h.double()
    return gamma.double() * (h * N.double()[:, None, :]) + beta.double() + h


def block(sd, p, x, v2):
    """One block on a channels-last map x [B, H, W, C]."""
    B, H, W, C = x.shape
    y = dwconv7_ln(x, sd[p + "conv_dw.weight"], sd[p + "conv_dw.bias"], sd[p + "norm.weight"], sd[p + "norm.bias"])
    h = F.gelu(F.linear(y, sd[p + "mlp.fc1.weight"].double(), sd[p + "mlp.fc1.bias"].double()))
    if v2:
        hh = h.reshape(B, H * W, 4 * C)
        h = grn_apply(hh, grn_stats(hh)[1], sd[p + "mlp.grn.weight"].reshape(-1), sd[p + "mlp.grn.bias"].reshape(-1)).reshape(B, H, W, 4 * C)
    y = F.linear(h, sd[p + "mlp.fc2.weight"].double(), sd[p + "mlp.fc2.bias"].double())
    if not v2:
        y = y * sd[p + "gamma"].double()
    return x + y


def trunk(sd, images, block_change=None):
    """stem + stages on images [B, 3, H, W] (sides multiples of 4) -> the four stage outputs, NCHW float64.  ``block_change``: a list
    that receives every block's relative L2 change of its input."""
    v2 = any(".mlp.grn." in k for k in sd)
    n_stage = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("stages."))
    x = F.conv2d(images.double(), sd["stem.0.weight"].double(), sd["stem.0.bias"].double(), stride=4).permute(0, 2, 3, 1)
    x = F.layer_norm(x, x.shape[-1:], sd["stem.1.weight"].double(), sd["stem.1.bias"].double(), EPS)
    outs = []
    for i in range(n_stage):
        if i > 0:
            p = f"stages.{i}.downsample."
            x = F.layer_norm(x, x.shape[-1:], sd[p + "0.weight"].double(), sd[p + "0.bias"].double(), EPS)
            x = F.conv2d(x.permute(0, 3, 1, 2), sd[p + "1.weight"].double(), sd[p + "1.bias"].double(), stride=2).permute(0, 2, 3, 1)
        j = 0
        while f"stages.{i}.blocks.{j}.conv_dw.weight" in sd:
            y = block(sd, f"stages.{i}.blocks.{j}.", x, v2)
            if block_change is not None:
                block_change.append(float((y - x).norm() / x.norm()))
            x = y
            j += 1
        outs.append(x.permute(0, 3, 1, 2).contiguous())
    return outs


def center_padding(images, patch_size=16):
    """evals/models/utils.py:55-72."""
    _, _, h, w = images.shape
    dh, dw = h % patch_size, w % patch_size
    if dh == 0 and dw == 0:
        return images
    ph, pw = patch_size - dh, patch_size - dw
    return F.pad(images, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2))


def finish(stage_maps, multilayers, output, out_hw):
    """convnext.py:89-108 on the stage outputs: the tapped maps, bilinear to (H / 16, W / 16) ('dense') or their spatial mean ('gap')."""
    outs = []
    for i in multilayers:
        x = stage_maps[i]
        outs.append(F.interpolate(x, out_hw, mode="bilinear") if output == "dense" else x.mean(dim=(2, 3)))
    return outs


def wrapper_forward(sd, images, multilayers=(3,), output="dense"):
    """The reference wrapper's forward (convnext.py:81-108) without add_norm -> a list of float64 outputs, one per tap."""
    images = center_padding(images.double(), 16)
    out_hw = (images.shape[-2] // 16, images.shape[-1] // 16)
    return finish(trunk(sd, images), list(multilayers), output, out_hw)


# ------------------------------------------------------------------------------------------------ kernel-test fixtures
DW_CHANNELS = (32, 64, 192, 1024, 1536)  # 192: no power of two; 1024 / 1536: rows reduced across several waves
DW_SIZES = ((1, 1), (1, 2), (3, 5), (7, 7), (9, 13), (12, 20))  # from maps smaller than the window to several strips per row
SIGMA_FLOOR = 1e-3  # rows whose sigma is below this share of their RMS are kept out: LayerNorm amplifies any error by 1 / sigma


def dwconv_fixture(C, H, W, B=2, seed=0, ldx=None):
    """Seeded fp32 inputs of mvp_dwconv7_ln_fwd: x [B, H, W, ldx] (columns >= C are filler the kernel must not read into its result),
    weight [C, 7, 7], bias, gamma, beta.  O(1) independent values, so a row's sigma is of the order of its RMS (tests/test_convnext_cpu.py holds every fixture to SIGMA_FLOOR)."""
    g = torch.Generator().manual_seed(1000 * C + 10 * H + W + 7919 * seed)
    ldx = C if ldx is None else ldx
    x = torch.randn(B, H, W, ldx, generator=g)
    w = torch.randn(C, 7, 7, generator=g) / 7.0
    b = torch.randn(C, generator=g)
    gamma = 0.5 + torch.rand(C, generator=g)
    beta = torch.randn(C, generator=g) * 0.5
    return x, w, b, gamma, beta


def row_sigma_ratio(x, w, b):
    """min over the pixels of sigma_C(conv output) / RMS_C(conv output), float64."""
    y = dwconv7(x[..., : w.shape[0]], w, b)
    return float((y.std(dim=-1, unbiased=False) / y.pow(2).mean(dim=-1).sqrt()).min())


def dwconv_yardstick(x, w, b, gamma, beta, eps=EPS):
    """(fp64 reference, max |torch fp32 CPU - fp64|): torch's own F.conv2d(groups=C) + F.layer_norm in fp32 against the fp64 evaluation
    of the same fixture — the measured error of an fp32 evaluation, from which the kernel's tolerance is derived."""
    C = w.shape[0]
    xc = x[..., :C].contiguous()
    ref = dwconv7_ln(xc, w, b, gamma, beta, eps)
    y32 = F.conv2d(xc.permute(0, 3, 1, 2), w.reshape(C, 1, 7, 7), b, padding=3, groups=C).permute(0, 2, 3, 1)
    y32 = F.layer_norm(y32, (C,), gamma, beta, eps)
    return ref, float((y32.double() - ref).abs().max())
