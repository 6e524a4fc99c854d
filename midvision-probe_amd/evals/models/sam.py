"""evals.models.sam.SAM — drop-in for the reference wrapper (evals/models/sam.py:11-113): segment_anything's image encoder (ViT-B / ViT-L;
no class token, a [1, S, S, C] position table, 14 x 14 windowed attention in most blocks and global attention in four, decomposed
relative-position terms on the unscaled q, erf-GELU MLP, no final norm) as a dense (multi-layer) feature extractor on the HIP kernels."""
from __future__ import annotations

import warnings

import torch.nn as nn

from mvp import backbone as bb
from mvp.vit import check_head_dim


class SAM(bb.ViTBackbone):
    """The reference's constructor signature plus ``weights`` (the published ``sam_vit_*.pth`` layout, transformers' SamVisionEncoder
    layout, or the engine's), ``precision`` and ``init_seed``.  Weights: ``weights``, else the local file ``sam_vit_b_01ec64.pth`` /
    ``sam_vit_l_0b3195.pth`` under MVP_CKPT_DIR, else seeded random init with a warning — nothing is ever fetched (the reference's
    ``urlretrieve`` is not ported).  Global / windowed blocks are inferred from the lengths of the relative-position tables.  The neck is
    not loaded (the reference's forward never runs it).  ``vit_h`` (head dim 80) is refused by the engine's head-dim check.
    Forward (sam.py:85-113): input sides must be multiples of the patch size; at a size other than the table's the position table is
    resampled bicubically (align_corners=False, no antialias) — always from the CHECKPOINT's table, where the reference overwrites its
    parameter and resamples the already resampled table at the next size change; blocks in order, NHWC -> NCHW maps per
    tap, ``output='gap'`` their spatial mean.  ``add_norm=True`` raises: the reference indexes ``self.batchnorms`` (one entry per TAP) by
    BLOCK index and applies BatchNorm2d(C) to an NHWC tensor sliced along H, which raises for every published configuration."""

    params_attr = "vit"
    ln_eps = 1e-6
    pos_embed_mode = "sam"

    def __init__(self, arch, output="dense", layer=-1, return_multilayer=False, add_norm=False, weights=None, precision=None, range_guard=None, init_seed=0):
        super().__init__()
        assert output in ["gap", "dense"], "Options: [gap, dense]"
        if add_norm:
            raise NotImplementedError(
                "add_norm: the reference's forward (sam.py:101-102) indexes self.batchnorms — one module per tap — by block index and applies "
                "BatchNorm2d(C) to the NHWC tensor x[:, 1:]; it raises for every published configuration, so there is nothing to reproduce")
        self.output = output
        self.checkpoint_name = f"sam_{arch}"
        ckpt_file = bb.SAM_CKPT_FILES[arch]
        sd = weights
        if sd is None:
            path = bb.find_checkpoint(ckpt_file)
            if path is not None:
                self.weights_from_file = True  # arms the f16x2 range guard under 'auto' (mvp/backbone.py)
                sd = bb.load_checkpoint_file(path)
            else:
                warnings.warn(f"no local checkpoint {ckpt_file}: using seeded random init (seed={init_seed})")
                C, depth, _, gidx = bb.SAM_ARCH[arch]
                sd = bb.random_sam_state_dict(C, depth, 64, 14, gidx, seed=init_seed)
        eng = bb.sam_to_engine(sd)
        feat_dim = int(eng["pos_embed"].shape[-1])
        emb_h, emb_w = eng["pos_embed"].shape[1:3]
        self.patch_size = int(eng["patch_embed.proj.weight"].shape[-1])
        self.image_size = (emb_h * self.patch_size, emb_w * self.patch_size)
        assert self.patch_size == 16
        # the arch's published head count at its published width (vit_h: 1280 / 16 = 80, refused); other widths (test models): C / 64
        self.heads = bb.SAM_ARCH[arch][2] if feat_dim == bb.SAM_ARCH[arch][0] else feat_dim // 64
        check_head_dim(feat_dim, self.heads)  # (the engine's own check, here so that construction on the CPU refuses already)
        self.vit = bb.ViTParams(eng).eval()
        self.block_windows = bb.sam_block_windows(eng)
        self.n_prefix = 0
        self._setup_taps(feat_dim, layer, return_multilayer, add_norm, self.vit.depth)
        self.batchnorms = nn.ModuleList([nn.BatchNorm2d(feat_dim) for _ in self.multilayers])
        self.set_precision(precision or bb.default_precision())
        self.set_range_guard(range_guard)

    def forward(self, x):
        _, _, h, w = x.shape
        assert h % self.patch_size == 0 and w % self.patch_size == 0, f"{h}, {w}"
        return self._finish(self._extract(x))
