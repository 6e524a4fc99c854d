"""evals.models.clip.CLIP — drop-in for the reference wrapper (evals/models/clip.py:11-101): the image tower of CLIP
(ViT-B/16, ViT-L/14, ViT-L/14 at 336) as a dense (multi-layer) feature extractor on the HIP kernels."""
from __future__ import annotations

import warnings

import torch.nn as nn

from mvp import backbone as bb


class CLIP(bb.ViTBackbone):
    """``arch``: an open_clip architecture name (mvp.backbone.CLIP_ARCH); ``checkpoint``: open_clip's pretrained tag.  The activation
    after fc1 follows open_clip's rule for these architectures: QuickGELU for the "openai" weights, erf GELU for every other tag.
    Weights: ``weights`` (a state dict in open_clip's ``visual.*`` layout, transformers' CLIPVisionModel layout or the engine's own), else
    a local file ``<checkpoint_name>`` under MVP_CKPT_DIR, else seeded random init — nothing is ever fetched.
    ``add_norm=True``: train-mode per-channel BatchNorm1d over all tokens of the batch at each tap, as the DINO wrapper does (the
    reference's own line, clip.py:97, hands [B, hw, C] to BatchNorm1d(C) and raises unless hw == C)."""

    pos_embed_mode = "resize_aa"
    ln_eps = 1e-5

    def __init__(self, arch="ViT-B-16", checkpoint="openai", output="dense", layer=-1, return_multilayer=False, add_norm=False,
                 weights=None, precision=None, range_guard=None, init_seed=0):
        super().__init__()
        assert output in ["dense-cls", "cls", "gap", "dense"]
        if arch not in bb.CLIP_ARCH:
            raise NotImplementedError(f"CLIP arch {arch!r}: the HIP path covers {sorted(bb.CLIP_ARCH)}")
        self.output = output
        self.arch_name = arch
        self.checkpoint_name = "clip_" + arch.replace("-", "").lower() + checkpoint
        self.act = "quick_gelu" if checkpoint == "openai" else "gelu"
        sd = weights
        if sd is None:
            path = bb.find_checkpoint(self.checkpoint_name)
            if path is not None:
                self.weights_from_file = True  # arms the f16x2 range guard under 'auto' (mvp/backbone.py)
                sd = bb.load_checkpoint_file(path)
            else:
                warnings.warn(f"no local checkpoint for {self.checkpoint_name}: using seeded random init (seed={init_seed})")
                C, depth, patch, img = bb.CLIP_ARCH[arch]
                sd = bb.random_clip_state_dict(C, depth, patch, img, seed=init_seed)
        self.vit = bb.ViTParams(bb.clip_to_engine(sd)).eval()
        self.patch_size = self.vit.patch_embed.proj.weight.shape[-1]
        self.heads = self.vit.embed_dim // 64
        self.n_prefix = 1
        feat_dim = self.vit.embed_dim
        feat_dim = feat_dim * 2 if output == "dense-cls" else feat_dim
        # clip.py:51-59: feat_dim is the four-entry list either way
        self._setup_taps(feat_dim, layer, return_multilayer, add_norm, self.vit.depth)
        self.feat_dim = [feat_dim] * 4
        self.batchnorms = nn.ModuleList([nn.BatchNorm1d(self.vit.embed_dim) for _ in self.multilayers])
        self.set_precision(precision or bb.default_precision())
        self.set_range_guard(range_guard)

    def forward(self, images):
        return self._finish(self._extract(images))
