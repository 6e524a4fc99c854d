"""Shared pieces of tests/test_gpu_corr_depth.py, and — run as a script — one rank of its two-rank test (fresh interpreter per rank,
torchrun-style environment; two ranks share cuda:0 over gloo on the one-GPU pool): mvp.corr3d.evaluate_scannet on this rank's shard
of the pairs of a SyntheticScanNetPairs dataset, one all_gather_object of the per-pair error vectors, the 19 numbers dumped."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "midvision-probe_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from _navi_rank import build_vit  # noqa: E402,F401  (the seeded tiny ViT, patch 16)

PAIRS, HEIGHT, WIDTH, NUM_CORR, SCALE = 5, 128, 160, 60, 0.25  # 5 pairs over 2 ranks: uneven shards
GT_SEED = 11  # the dataset seed of the ground-truth-feature test (chosen so that no error sits on a threshold: see the test)


def dataset(pairs=PAIRS, seed=21):
    from mvp import corr3d

    return corr3d.SyntheticScanNetPairs(num_pairs=pairs, image_height=HEIGHT, image_width=WIDTH, seed=seed)


class GroundTruthFeatures(torch.nn.Module):
    """A stub backbone whose dense "features" are random Fourier features (sin and cos of C / 2 fixed random projections, a few
    radians per metre) of each pixel's ground-truth 3-D point in view-1 coordinates (the scene without depth holes), average-pooled
    to a patch grid of 8 pixels.  Unlike a plain linear projection, whose L2-normalised value keeps only the point's direction,
    these separate neighbouring cells by cosine distances of 1e-3 and more, far above fp32 resolution.  It recognises an image by a
    few of its pixel values (a host lookup: the stub has no ``supports_pipelining``, so its forwards run inline)."""

    patch_size, checkpoint_name, layer, output = 8, "ground_truth_stub", "-1", "dense"

    def __init__(self, ds, C=32):
        super().__init__()
        self.W = 4.0 * torch.randn(3, C // 2, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
        self.table = {}
        for i in range(len(ds)):
            it, geo = ds[i], ds.geometry(i)
            self.table[self.key(it["rgb_0"])] = geo["xyz_0"] @ geo["R"].t() + geo["t"]
            self.table[self.key(it["rgb_1"])] = geo["xyz_1"]

    @staticmethod
    def key(img):
        H, W = img.shape[-2:]
        return tuple(img[:, H // 2, W // 2 - 2:W // 2 + 2].flatten().tolist())

    def features(self, img):
        """[C, H / 8, W / 8] float32 (CPU) for one image."""
        ph = self.table[self.key(img)] @ self.W
        f = torch.cat((ph.sin(), ph.cos()), dim=-1).permute(2, 0, 1)
        return torch.nn.functional.avg_pool2d(f[None], self.patch_size)[0].float()

    def forward(self, images):
        return torch.stack([self.features(im) for im in images.cpu()]).to(images.device)


def main():
    out_dir = sys.argv[1]
    from mvp import corr3d
    from mvp import dist as mdist

    rank, local, world = mdist.env_setup("nccl")
    dev = torch.device("cuda", torch.cuda.current_device())
    numbers = corr3d.evaluate_scannet(build_vit(dev), dataset(), NUM_CORR, SCALE, False, rank=rank, world=world)
    np.savez(os.path.join(out_dir, f"scannet{rank}.npz"), numbers=np.array(numbers, dtype=np.float64), world=world,
             backend=np.array(torch.distributed.get_backend()))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
