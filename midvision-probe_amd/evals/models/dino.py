"""evals.models.dino.DINO — drop-in for the reference wrapper (evals/models/dino.py:9-210),
DINO ViT-B/16 and ViT-B/8 and DINOv2 (ViT-B/14, B/14 with registers, L/14, g/14) dense (multi-layer) feature extraction on the HIP kernels."""
from __future__ import annotations

import warnings

import torch
import torch.nn as nn

from mvp import backbone as bb


DINO_ARCH = {"vitb16": ("dino_vitbase16_pretrain", 16), "vitb8": ("dino_vitbase8_pretrain", 8)}  # model_name -> (torch.hub file, patch size); ViT-B both


class DINO(bb.ViTBackbone):
    def __init__(self, dino_name="dino", model_name="vitb16", output="dense", layer=-1, return_multilayer=False, add_norm=False,
                 return_kqv=False, fixed_size=480, mode_selected="k", return_layers=None, return_cls=False,
                 weights=None, precision=None, range_guard=None, init_seed=0):
        super().__init__()
        feat_dims = {"vitb8": 768, "vitb16": 768, "vitb14": 768, "vitb14_reg": 768, "vitl14": 1024, "vitg14": 1536}
        v2 = dino_name == "dinov2"
        if not ((dino_name == "dino" and model_name in DINO_ARCH) or (v2 and model_name in bb.DINOV2_ARCH)):
            raise NotImplementedError("the HIP path covers DINO ViT-B/16, B/8 and DINOv2 ViT-B/14, B/14-reg, L/14, g/14 "
                                      "(configs/backbone/dino_b16.yaml, dino_b8.yaml, dinov2_*.yaml)")
        if v2 and return_kqv:
            # the reference's extract_kqv calls self.vit.prepare_tokens (dino.py:104), which DINOv2's hub model does not have
            raise NotImplementedError("return_kqv with dinov2: the reference's extract_kqv has no DINOv2 path (prepare_tokens)")
        if return_kqv and mode_selected not in ("k", "q", "v", "kqv"):
            raise ValueError(f"mode_selected {mode_selected!r}: one of k, q, v, kqv (dino.py:126-139)")
        self.arch = "vit"
        self.return_cls = return_cls
        self.dino_name, self.model_name = dino_name, model_name
        self.checkpoint_name = f"{dino_name}_{model_name}"
        # reference: torch.hub.load("facebookresearch/dino", ...) (dino.py:40) — no network here:
        # local checkpoint (MVP_CKPT_DIR/<checkpoint_name>.pth) or an explicit state dict, else seeded random init.
        sd = weights
        if sd is None:
            hub = bb.DINOV2_HUB_NAMES[model_name] if v2 else DINO_ARCH[model_name][0]
            path = bb.find_checkpoint(self.checkpoint_name, hub)
            if path is not None:
                self.weights_from_file = True  # arms the f16x2 range guard under 'auto' (mvp/backbone.py)
                sd = bb.load_checkpoint_file(path)
            elif v2 and bb.DINOV2_FFN.get(model_name) == "swiglu":
                # 4.4 GB of random weights in place of a missing file is never what was meant
                raise NotImplementedError(f"dinov2 {model_name} (SwiGLU MLP, 1.1 B parameters): no local checkpoint and no weights=; "
                                          "the seeded random-init fallback is not offered at this size")
            else:
                warnings.warn(f"no local checkpoint for {self.checkpoint_name}: using seeded random init (seed={init_seed})")
                if v2:
                    C, depth, R = bb.DINOV2_ARCH[model_name]
                    sd = bb.random_dinov2_state_dict(C, depth, R, seed=init_seed)
                else:
                    sd = bb.random_vit_state_dict(patch=DINO_ARCH[model_name][1], seed=init_seed)
        if v2:
            sd = bb.dinov2_hub_to_engine(sd)
        self.vit = bb.ViTParams(sd).eval()
        self.has_registers = "_reg" in model_name
        self.n_prefix = 1 + (self.vit.register_tokens.shape[1] if hasattr(self.vit, "register_tokens") else 0)
        self.patch_size = self.vit.patch_embed.proj.weight.shape[-1]
        assert output in ["cls", "gap", "dense", "dense-cls"]
        self.output = output
        feat_dim = self.vit.embed_dim  # == feat_dims[model_name] for real checkpoints
        feat_dim = feat_dim * 2 if output == "dense-cls" else feat_dim
        self._setup_taps(feat_dim, layer, return_multilayer, add_norm, self.vit.depth)
        if output == "dense-cls":
            feat_dim = feat_dim // 2
        self.batchnorms = nn.ModuleList([nn.BatchNorm1d(feat_dim) for _ in self.multilayers])
        self.return_kqv, self.fixed_size, self.mode_selected = return_kqv, fixed_size, mode_selected
        # DINOv2's register models resample the pos-embed to the grid size with antialiasing (interpolate_offset 0); the others use the
        # +0.1 scale nudge, DINO's rule
        self.heads, self.ln_eps = self.vit.embed_dim // 64, 1e-6
        self.pos_embed_mode = "dinov2_reg" if (v2 and self.has_registers) else "dino"
        self.set_precision(precision or bb.default_precision())
        self.set_range_guard(range_guard)

    def forward(self, images):
        if self.return_kqv:  # dino.py:164-169
            return self.extract_kqv(self.preprocess_image(images)[0])
        if len(self.multilayers) == 1 and self.return_cls:
            # dino.py:206-207: embeds[0][:, 0] — the (tap-BN normalised when add_norm) CLS token of the single tap
            return self._extract(images, want_cls=True).cls[0]
        taps = self._extract(images)
        return self._finish(taps)
