"""Records tests/golden/ssim.npz from the reference's own SSIM (evals/utils/losses.py: gaussian, create_window, ssim) on seeded inputs:

    MVP_REFERENCE=<path to a checkout of the reference> python tests/golden/make_goldens_ssim.py

The reference's evals/utils/losses.py imports torch and numpy only and is loaded by file path.  It is read only while this script
runs; nothing of it is stored but numbers:

    window                  create_window(11, 1)                                            [1, 1, 11, 11] fp32
    <case>__a, <case>__b    an input pair [B, C, H, W] fp32 on the 8-bit grid (k / 255)
    <case>__per32, __all32  ssim(a, b, size_average=False) and ssim(a, b) in fp32, the dtype the reference runs in
    <case>__per64, __all64  the same on a.double(), b.double(): ``window.type_as(img1)`` makes the whole computation fp64

Cases (B, C, H, W): 1 x 1 x 7 x 9 (every window hangs over a border), 2 x 3 x 5 x 5, 1 x 2 x 13 x 12 and 2 x 3 x 24 x 20; the first and
third are uniform noise against a noisy copy, the others a smooth field plus noise against a noisier copy."""
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("MVP_REFERENCE")
CASES = [("noise_1x1x7x9", (1, 1, 7, 9), False), ("smooth_2x3x5x5", (2, 3, 5, 5), True), ("noise_1x2x13x12", (1, 2, 13, 12), False),
         ("smooth_2x3x24x20", (2, 3, 24, 20), True)]


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def q8(x):
    return (x.clamp(0.0, 1.0) * 255.0).round() / 255.0


def make_pair(shape, smooth, g):
    B, C, H, W = shape
    if smooth:
        yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
        ph = torch.rand(B, C, 1, 1, generator=g) * 6.28
        a = 0.5 + 0.3 * torch.sin(3.0 * xx + 2.0 * yy + ph) + 0.02 * torch.randn(B, C, H, W, generator=g)
    else:
        a = torch.rand(B, C, H, W, generator=g)
    a = q8(a)
    return a, q8(a + 0.1 * torch.randn(B, C, H, W, generator=g))


def main():
    if not REF:
        raise SystemExit("set MVP_REFERENCE to a checkout of the reference")
    L = _load(os.path.join(REF, "evals", "utils", "losses.py"), "ref_losses")
    g = torch.Generator().manual_seed(20261021)
    out = {"window": L.create_window(11, 1).numpy()}
    assert out["window"].dtype == np.float32 and out["window"].shape == (1, 1, 11, 11)
    for name, shape, smooth in CASES:
        a, b = make_pair(shape, smooth, g)
        out[f"{name}__a"], out[f"{name}__b"] = a.numpy(), b.numpy()
        for tag, cast in (("32", torch.Tensor.float), ("64", torch.Tensor.double)):
            per, mean = L.ssim(cast(a), cast(b), size_average=False), L.ssim(cast(a), cast(b))
            assert per.dtype == mean.dtype == (torch.float32 if tag == "32" else torch.float64) and per.shape == (shape[0],)
            out[f"{name}__per{tag}"], out[f"{name}__all{tag}"] = per.numpy(), mean.numpy()
        print(name, out[f"{name}__per64"], float(out[f"{name}__all64"]),
              "fp32 - fp64:", np.abs(out[f"{name}__per32"].astype(np.float64) - out[f"{name}__per64"]).max())
    path = os.path.join(HERE, "ssim.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
