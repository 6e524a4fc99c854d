"""evals.models.siglip.SigLIP — drop-in for the reference wrapper (evals/models/siglip.py:10-93): the image tower of SigLIP
(ViT-B/16, ViT-L/16; no class token) as a dense (multi-layer) feature extractor on the HIP kernels."""
from __future__ import annotations

import warnings

import torch.nn as nn

from mvp import backbone as bb


class SigLIP(bb.ViTBackbone):
    """``checkpoint``: a timm model name (mvp.backbone.SIGLIP_ARCH).  ``pretrained`` is accepted for the reference's signature; weights
    come from ``weights`` (timm's or transformers' SiglipVisionModel layout), else a local file ``<checkpoint>`` under MVP_CKPT_DIR, else
    seeded random init — nothing is ever fetched.
    ``act``: the activation after fc1, "gelu_tanh" by default — the SigLIP checkpoints were trained with the tanh form and transformers'
    SiglipVisionConfig defaults to it; which form a given timm release builds for these model names could not be checked where this was
    written (timm was not installed), so ``act="gelu"`` (erf) is there for users who want to match a release that builds the other.
    ``resize_pos_embeds=False`` keeps the position table as it is (the image grid must then match it).
    ``add_norm=True``: train-mode per-channel BatchNorm1d over all tokens of the batch at each tap, as the DINO wrapper does (the
    reference's own lines, siglip.py:83, index ``batchnorms`` by block number and feed tokens to BatchNorm2d)."""

    ln_eps = 1e-6

    def __init__(self, checkpoint="vit_large_patch16_siglip_384", output="dense", layer=-1, resize_pos_embeds=True, pretrained=True,
                 return_multilayer=False, add_norm=False, act="gelu_tanh", weights=None, precision=None, range_guard=None, init_seed=0):
        super().__init__()
        assert output in ["gap", "dense"], "Options: [gap, dense]"
        if checkpoint not in bb.SIGLIP_ARCH:
            raise NotImplementedError(f"SigLIP checkpoint {checkpoint!r}: the HIP path covers {sorted(bb.SIGLIP_ARCH)}")
        if act not in ("gelu_tanh", "gelu"):
            raise ValueError(f"act {act!r}: 'gelu_tanh' or 'gelu'")
        self.output = output
        self.checkpoint_name = checkpoint
        self.act = act
        self.resize_pos_embeds = resize_pos_embeds
        self.pos_embed_mode = "resize_aa" if resize_pos_embeds else "fixed"
        C, depth, patch, img = bb.SIGLIP_ARCH[checkpoint]
        sd = weights
        if sd is None:
            path = bb.find_checkpoint(checkpoint)
            if path is not None:
                self.weights_from_file = True  # arms the f16x2 range guard under 'auto' (mvp/backbone.py)
                sd = bb.load_checkpoint_file(path)
            else:
                warnings.warn(f"no local checkpoint for {checkpoint}: using seeded random init (seed={init_seed})")
                sd = bb.random_siglip_state_dict(C, depth, patch, img, seed=init_seed)
        self.vit = bb.ViTParams(bb.siglip_to_engine(sd)).eval()
        self.patch_size = self.vit.patch_embed.proj.weight.shape[-1]
        side = int(self.vit.pos_embed.shape[1] ** 0.5)
        self.embed_size = (side, side)
        self.heads = self.vit.embed_dim // 64
        self.n_prefix = 0
        self._setup_taps(self.vit.embed_dim, layer, return_multilayer, add_norm, self.vit.depth)
        self.batchnorms = nn.ModuleList([nn.BatchNorm1d(self.vit.embed_dim) for _ in self.multilayers])
        self.set_precision(precision or bb.default_precision())
        self.set_range_guard(range_guard)

    def forward(self, images):
        return self._finish(self._extract(images))
