"""evals.models.croco.CROCO — drop-in for the reference wrapper (evals/models/croco.py:20-178): the encoder of CroCo (cross-view
completion; a plain ViT-B/16 without a class token, fixed sin-cos position table) as a dense (multi-layer) feature extractor on the
HIP kernels.  evals.models.crocov2.CROCOV2 shares everything but the checkpoint and the position form (RoPE100)."""
from __future__ import annotations

import argparse
import warnings

import torch
import torch.nn as nn

from mvp import backbone as bb
from mvp import functional as MF
from mvp import pipeline


def _load_published(path: str):
    """The whole checkpoint object (``load_checkpoint_file`` would unwrap ``model`` and lose ``croco_kwargs``)."""
    with torch.serialization.safe_globals([argparse.Namespace]):  # (the published files carry their training ``args`` as well)
        return torch.load(path, map_location="cpu", weights_only=True)


class CROCO(bb.ViTBackbone):
    """The reference's constructor signature plus ``weights`` (the published ``{"model": ..., "croco_kwargs": ...}`` layout, the bare model
    dict, or the engine's layout), ``precision`` and ``init_seed``.  Weights: ``weights``, else the local file ``CroCo.pth`` under
    MVP_CKPT_DIR, else seeded random init with a warning — nothing is ever fetched.
    The position form comes from the checkpoint's ``croco_kwargs["pos_embed"]`` ('cosine': the fixed table ``enc_pos_embed``; 'RoPE<freq>':
    no table, Q and K of every block rotated by the token's grid position); without it, the class's own (``default_pos_embed``).
    Images are resized bilinearly (align_corners=False) to the model's ``img_size`` (croco.py:138-140; 224 for the published models, a
    (height, width) pair is accepted); there is no centre padding.  ``layer`` is accepted and, as in the reference, not used: the taps are
    blocks n/4-1, n/2-1, 3n/4-1, n-1 with ``return_multilayer``, else the last block.  ``add_norm``: train-mode BatchNorm1d over all tokens
    of the batch at each tap.  ``return_cls=True`` with a single tap returns the FIRST PATCH token [B, C] (the reference's
    ``embeds[0][:, 0]``: there is no class token).  ``return_kqv=True`` raises: the reference's own branch hands a 5-D tensor to the patch
    convolution and cannot run."""

    params_attr = "model"
    ckpt_key = "croco"
    default_pos_embed = "cosine"
    ln_eps = 1e-6
    pos_embed_mode = "fixed"

    def __init__(self, model_name="vitb16", layer=-1, output="dense", return_multilayer=False, add_norm=False, return_kqv=False,
                 fixed_size=480, mode_selected="k", return_layers=None, return_cls=False, weights=None, precision=None, range_guard=None, init_seed=0):
        super().__init__()
        self.arch = "vit"
        self.return_cls = return_cls
        assert model_name == "vitb16", f"Invalid model: {model_name}"
        if return_kqv:
            raise NotImplementedError("return_kqv: the reference's branch (croco.py:133-136) feeds a 5-D tensor to the patch convolution and cannot run")
        sd = weights
        if sd is None:
            path = bb.find_checkpoint(bb.CROCO_CKPT_FILES[self.ckpt_key])
            if path is not None:
                self.weights_from_file = True  # arms the f16x2 range guard under 'auto' (mvp/backbone.py)
                sd = _load_published(path)
            else:
                warnings.warn(f"no local checkpoint {bb.CROCO_CKPT_FILES[self.ckpt_key]}: using seeded random init (seed={init_seed})")
                sd = bb.random_croco_state_dict(768, 12, 16, 224, pos_embed=self.default_pos_embed, seed=init_seed)
        kwargs = dict(sd.get("croco_kwargs") or {}) if isinstance(sd.get("model"), dict) else {}
        eng = bb.croco_to_engine(sd)
        self.pos_form = str(kwargs.get("pos_embed", self.default_pos_embed))
        self.patch_size = 16
        self.img_size = bb._pair(kwargs.get("img_size", 224))
        C = eng["patch_embed.proj.weight"].shape[0]
        if self.pos_form == "cosine":
            if "pos_embed" not in eng:  # (a registered buffer of the reference model: in every state dict it saves)
                grid = (self.img_size[0] // self.patch_size, self.img_size[1] // self.patch_size)
                eng["pos_embed"] = torch.from_numpy(bb.sincos_pos_embed_2d(C, grid, add_cls_token=False)).float().unsqueeze(0)
        elif self.pos_form.startswith("RoPE"):
            self.rope_freq = float(self.pos_form[len("RoPE"):])
            eng.pop("pos_embed", None)
        else:
            raise NotImplementedError("Unknown pos_embed " + self.pos_form)
        self.model = bb.ViTParams(eng).eval()
        self.output = output
        self.checkpoint_name = f"{self.ckpt_key}_{model_name}_{output}"
        self.heads = C // 64
        self.n_prefix = 0
        self._setup_taps(C, -1, return_multilayer, add_norm, self.model.depth)  # (768 for the published ViT-B/16)
        self.batchnorms = nn.ModuleList([nn.BatchNorm1d(C) for _ in self.multilayers])
        self.return_kqv, self.fixed_size, self.mode_selected = return_kqv, fixed_size, mode_selected
        self.set_precision(precision or bb.default_precision())
        self.set_range_guard(range_guard)

    def _engine_images(self, images):
        """The resize to the model's image size that ``forward`` starts with (also what the f16x2 range guard audits)."""
        if tuple(images.shape[-2:]) != self.img_size:  # (a same-size bilinear resize with align_corners=False returns its input's values)
            with torch.no_grad():
                images = MF.interpolate(images, size=self.img_size, mode="bilinear", align_corners=False)  # croco.py:138-140
        return images

    def forward(self, images):
        images = self._engine_images(images)
        taps = self._extract(images)
        if isinstance(taps, bb.TapGroups):  # several batches stacked into one forward (mvp/pipeline.py): one result per batch
            return pipeline.GroupedFeatures((t[0] if len(t) == 1 else t) for t in taps)
        if len(taps) == 1 and self.return_cls:
            return taps[0][:, :, 0, 0].contiguous()  # the first patch token, tap-normalised when add_norm (embeds[0][:, 0], croco.py:175-176)
        return taps[0] if len(taps) == 1 else taps
