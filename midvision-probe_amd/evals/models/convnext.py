"""evals.models.convnext.ConvNext — drop-in for the reference wrapper (evals/models/convnext.py:12-108): ConvNeXt-B (open_clip's
``convnext_base_w`` CLIP towers, timm's ``convnext_base_in22k``) and ConvNeXt V2-B (``convnextv2_base.fcmae_ft_in22k_in1k_384``) as a
dense (multi-layer) feature extractor on the HIP kernels (mvp/convnext.py)."""
from __future__ import annotations

import warnings

import torch
import torch.nn as nn

from mvp import backbone as bb
from mvp import convnext as cnx
from mvp import functional as MF
from mvp import lib
from mvp.vit import parse_precision

# arch -> (widths, depths); the reference's choice files name ConvNeXt-B only
ARCHS = {"convnext_base_w": (cnx.WIDTHS_B, cnx.DEPTHS_B), "convnext_base": (cnx.WIDTHS_B, cnx.DEPTHS_B)}
# local file names looked for under MVP_CKPT_DIR, per reference branch (nothing is ever fetched)
_TIMM_NAMES = {"in22k": ("convnext_base_in22k", "convnext_base_22k_224"),
               "fcmae_ft_in22k_in1k_384": ("convnextv2_base.fcmae_ft_in22k_in1k_384", "convnextv2_base_22k_384_ema")}


class ConvNextParams(nn.Module):
    """Parameter container with the engine's (timm's) key layout."""

    def __init__(self, sd):
        super().__init__()
        for k, v in sd.items():
            parts = k.split(".")
            mod = self
            for p in parts[:-1]:
                if not hasattr(mod, p):
                    setattr(mod, p, bb._Named())
                mod = getattr(mod, p)
            mod.register_parameter(parts[-1], nn.Parameter(v.clone().float(), requires_grad=False))


class ConvNext(nn.Module):
    """The reference's constructor signature plus ``weights`` (a state dict in transformers' ConvNextModel / ConvNextV2Model layout,
    timm's, open_clip's ``visual.trunk.`` form of it, or the engine's), ``precision`` and ``init_seed``.  Weights: ``weights``, else a
    local file under MVP_CKPT_DIR, else seeded random init with a warning.  ``add_norm=True`` raises: the reference feeds the
    batch-normalised map into the next stage (convnext.py:94-96) and no choice file enables it."""

    def __init__(self, arch="convnext_base_w", checkpoint="laion2b_s13b_b82k", output="dense", layer=-1, return_multilayer=False,
                 add_norm=False, weights=None, precision=None, init_seed=0):
        super().__init__()
        assert output in ["gap", "dense"]
        self.output = output
        self.patch_size = 16
        # convnext.py:27-50
        if "laion2b" in checkpoint:
            self.checkpoint_name = f"{arch}_{checkpoint}"
            names, v2 = (f"{arch}_{checkpoint}", f"{arch}-{checkpoint}"), False
        elif arch == "convnext_base" and checkpoint == "in22k":
            self.checkpoint_name = "convnext_base_in22k"
            names, v2 = _TIMM_NAMES[checkpoint], False
        elif arch == "convnext_base" and checkpoint == "fcmae_ft_in22k_in1k_384":
            self.checkpoint_name = "convnext_base_fcmae_ft_in22k_in1k_384"
            names, v2 = _TIMM_NAMES[checkpoint], True
        else:
            raise ValueError()
        self.checkpoint_name = self.checkpoint_name.replace("convnext", "cnxt").replace("base", "b")  # convnext.py:52-53
        if add_norm:
            raise NotImplementedError(
                "add_norm: the reference's forward (convnext.py:94-96) feeds the batch-normalised tap into the next stage; no choice "
                "file enables it and it is not reproduced")
        assert layer in [-1, 0, 1, 2, 3]
        sd = weights
        if sd is None:
            path = bb.find_checkpoint(*names)
            if path is not None:
                sd = bb.load_checkpoint_file(path)
            else:
                if arch not in ARCHS:
                    raise ValueError(f"no local checkpoint and no known geometry for arch {arch!r}")
                warnings.warn(f"no local checkpoint for {self.checkpoint_name}: using seeded random init (seed={init_seed})")
                sd = cnx.random_state_dict(*ARCHS[arch], v2=v2, seed=init_seed)
        eng = cnx.to_engine(sd)
        self.widths, self.depths, self.v2 = cnx.arch_of(eng)
        assert len(self.widths) == 4
        self.visual = ConvNextParams(eng).eval()
        feat_dims = list(self.widths)  # convnext.py:60-62
        multilayers = [0, 1, 2, 3]
        if return_multilayer:
            self.feat_dim = feat_dims
            self.multilayers = multilayers
        else:
            layer = multilayers[-1] if layer == -1 else layer
            self.feat_dim = feat_dims[layer]
            self.multilayers = [layer]
        self.layer = "-".join(str(_x) for _x in self.multilayers)
        self.batchnorms = nn.ModuleList([nn.BatchNorm2d(fd) for fd in feat_dims])
        self.add_norm = add_norm
        self.set_precision(precision or bb.default_precision())

    def set_precision(self, precision) -> None:
        self._precision = parse_precision(precision)

    def engine(self) -> cnx.ConvNeXtEngine:
        sig = tuple((p.data_ptr(), p._version) for p in self.visual.parameters()) + (self._precision,)
        if getattr(self, "_engine_sig", None) != sig:
            dev = next(self.visual.parameters()).device
            if dev.type != "cuda":
                raise lib.MvpError("backbone parameters are on the CPU: call model.to('cuda') — the HIP path has no CPU fallback")
            self._engine_obj = cnx.ConvNeXtEngine(self.visual.state_dict(), self.depths, self.widths, precision=self._precision, device=dev)
            self._engine_sig = sig
        return self._engine_obj

    def forward(self, images):
        if not images.is_cuda:
            raise lib.MvpError("images must be on the HIP device (no CPU fallback)")
        with torch.no_grad():
            # center_padding to a multiple of the patch size (convnext.py:82) happens inside the stem's gather
            taps = self.engine().forward_taps(images, self.multilayers, pad_to=self.patch_size)
            img_h, img_w = images.shape[-2:]
            dh, dw = img_h % self.patch_size, img_w % self.patch_size
            if dh or dw:  # utils.py:55-72: both sides grow, a non-ragged one by a whole patch
                img_h, img_w = img_h + self.patch_size - dh, img_w + self.patch_size - dw
            out_hw = (img_h // self.patch_size, img_w // self.patch_size)  # convnext.py:83-84, of the padded image
            outputs = []
            for x_i in taps:
                if self.output == "dense":  # F.interpolate(x_i, out_hw, mode="bilinear"), convnext.py:103
                    x_i = x_i if tuple(x_i.shape[-2:]) == out_hw else MF.interpolate(x_i, size=out_hw, mode="bilinear", align_corners=False)
                else:
                    x_i = x_i.mean(dim=(2, 3))
                outputs.append(x_i)
        return outputs[0] if len(outputs) == 1 else outputs
