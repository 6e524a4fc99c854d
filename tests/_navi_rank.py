"""Shared pieces of tests/test_gpu_corr3d.py, and — run as a script — one rank of its two-rank test (fresh interpreter per rank,
torchrun-style environment; two ranks share cuda:0 over gloo on the one-GPU pool): mvp.corr3d.evaluate_dataset on this rank's shard
of the loader batches of a SyntheticNAVI dataset, one all_gather_object of the per-pair error vectors, the ten numbers dumped."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "midvision-probe_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

D, DEPTH, PAIRS, SIZE, NUM_CORR, SCALE, BATCH = 128, 4, 5, 128, 60, 0.25, 2  # 5 pairs in batches of 2: uneven shards, a ragged last batch


def build_vit(dev):
    from evals.models.dino import DINO
    from oracle import vit as ovit  # seeded tiny-ViT weights only (test infrastructure)

    return DINO(output="dense", add_norm=True, weights=ovit.make_vit_weights(embed_dim=D, depth=DEPTH, seed=77)).to(dev)


def dataset(pairs=PAIRS):
    from mvp import corr3d

    return corr3d.SyntheticNAVI(num_pairs=pairs, image_size=SIZE, seed=21)


class GroundTruthFeatures(torch.nn.Module):
    """A stub backbone whose dense "features" are a fixed random projection (3 -> C) of each pixel's ground-truth 3-D point in
    view-1 coordinates (0 outside the object), average-pooled to the patch grid.  It recognises an image by a few of its pixel values
    (a host lookup: the stub has no ``supports_pipelining``, so its forwards run inline)."""

    patch_size, checkpoint_name, layer, output = 16, "ground_truth_stub", "-1", "dense"

    def __init__(self, ds, C=32):
        super().__init__()
        from corr3d_ref import transform

        self.W = torch.randn(3, C, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
        self.table = {}
        for i in range(len(ds)):
            it = ds[i]
            for view in (0, 1):
                xyz = it[f"xyz_grid_{view}"].permute(1, 2, 0).double()
                m = xyz[..., 2] > 0
                p = transform(xyz.reshape(-1, 3), it["Rt_01"]).reshape(xyz.shape) if view == 0 else xyz
                self.table[self.key(it[f"image_{view}"])] = torch.where(m[..., None], p, torch.zeros_like(p))

    @staticmethod
    def key(img):
        S = img.shape[-1]
        return tuple(img[:, S // 2, S // 2 - 2:S // 2 + 2].flatten().tolist())

    def features(self, img):
        """[C, S / 16, S / 16] float32 (CPU) for one image."""
        f = (self.table[self.key(img)] @ self.W).permute(2, 0, 1)
        return torch.nn.functional.avg_pool2d(f[None], self.patch_size)[0].float()

    def forward(self, images):
        return torch.stack([self.features(im) for im in images.cpu()]).to(images.device)


def main():
    out_dir = sys.argv[1]
    from mvp import corr3d
    from mvp import dist as mdist

    rank, local, world = mdist.env_setup("nccl")
    dev = torch.device("cuda", torch.cuda.current_device())
    numbers = corr3d.evaluate_dataset(build_vit(dev), dataset(), NUM_CORR, SCALE, False, batch_size=BATCH, rank=rank, world=world)
    np.savez(os.path.join(out_dir, f"navi{rank}.npz"), numbers=np.array(numbers, dtype=np.float64), world=world,
             backend=np.array(torch.distributed.get_backend()))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
