"""evals.models.beit_v2.BEiTV2 — drop-in for the reference wrapper (evals/models/beit_v2.py:17-86, 248-287): BEiT v2's ViT-B/16 (class
token, no absolute position table, a learned relative-position bias per block added to the attention logits, LayerScale, q / v bias with
a zero k bias, ``fc_norm``) as a dense (multi-layer) feature extractor on the HIP kernels."""
from __future__ import annotations

import warnings

import torch
import torch.nn as nn

from mvp import backbone as bb
from mvp import functional as MF
from mvp import pipeline


class BEiTV2(bb.ViTBackbone):
    """The reference's constructor signature plus ``weights`` (the published ``{"model": ...}`` layout, the bare dict, or the engine's
    layout), ``img_size`` (the model's image size when ``weights`` belong to a non-square grid, which a table's length does not reveal),
    ``precision`` and ``init_seed``.  Weights: ``weights``, else the local file ``beit_v2_vitb16.pth`` under MVP_CKPT_DIR, else seeded
    random init with a warning — nothing is ever fetched.  A relative-position table of another grid than the model's is refused (the
    reference re-interpolates it with scipy; not built).
    The forward is the reference's, quirk included (beit_v2.py:255-277): images are resized bilinearly (align_corners=False) to the
    model's image size (the literal 224 of the published model; grid x patch of the checkpoint here), ``forward_features(...,
    return_all_tokens=True)`` runs ALL blocks and then ``fc_norm`` over all tokens, and the blocks then run AGAIN on that result — the
    taps (blocks n/4-1, n/2-1, 3n/4-1, n-1 with ``return_multilayer``, else the last) are taken in this second pass.  ``add_norm``:
    train-mode BatchNorm1d over all tokens of the batch, class token included, on the tap only.  ``return_cls`` with a single tap returns
    ``x[:, 0]`` un-normalised.  ``output`` is stored and, as in the reference, ignored: the result is always dense.  ``layer`` is ignored.
    ``return_kqv=True`` raises: see INTEGRATION.md."""

    params_attr = "model"
    ln_eps = 1e-6
    pos_embed_mode = "fixed"
    replay_after_norm = True

    def __init__(self, model_name="beit_vitb16", layer=-1, arch="beit_vitb16", output="dense", return_multilayer=False, add_norm=False,
                 return_kqv=False, fixed_size=224, mode_selected="k", return_cls=False, weights=None, img_size=None, precision=None, range_guard=None, init_seed=0):
        super().__init__()
        self.arch = "vit"
        self.return_cls = return_cls
        assert arch == "beit_vitb16", f"Invalid arch: {arch}"
        if return_kqv:
            raise NotImplementedError(
                "return_kqv: in the reference this path never sees the hooked projection (Attention.forward calls F.linear, not self.qkv, "
                "beit_model.py:162), and its fallback (beit_v2.py:171-177) applies qkv to the un-normalised residual without bias and swaps "
                "heads and head-dim in the reshape; it is not reproduced")
        sd = weights
        if sd is None:
            path = bb.find_checkpoint(bb.BEIT_CKPT_FILE)
            if path is not None:
                self.weights_from_file = True  # arms the f16x2 range guard under 'auto' (mvp/backbone.py)
                sd = bb.load_checkpoint_file(path)
            else:
                warnings.warn(f"no local checkpoint {bb.BEIT_CKPT_FILE}: using seeded random init (seed={init_seed})")
                sd = bb.random_beit_state_dict(768, 12, 16, 224, seed=init_seed)
        eng = bb.beit_to_engine(sd)
        eng.pop("pos_embed", None)  # use_abs_pos_emb=False (beit_v2.py:78)
        self.patch_size = int(eng["patch_embed.proj.weight"].shape[-1])
        C = eng["patch_embed.proj.weight"].shape[0]
        grid = None if img_size is None else tuple(s // self.patch_size for s in bb._pair(img_size))
        self.rel_pos_grid = bb.beit_grid(eng["blocks.0.attn.rel_pos_bias_table"].shape[0], grid)
        self.img_size = (self.rel_pos_grid[0] * self.patch_size, self.rel_pos_grid[1] * self.patch_size)
        self.model = bb.ViTParams(eng).eval()
        for i in range(self.model.depth):
            bb.beit_grid(eng[f"blocks.{i}.attn.rel_pos_bias_table"].shape[0], self.rel_pos_grid)
        self.output = output
        self.heads = C // 64
        self.n_prefix = 1
        self._setup_taps(C, -1, return_multilayer, add_norm, self.model.depth)  # (768 for the published ViT-B/16; ``layer`` is not used)
        self.checkpoint_name = f"$beit_v2$_{model_name}_{output}_{self.layer}"
        self.batchnorms = nn.ModuleList([nn.BatchNorm1d(C) for _ in self.multilayers])
        self.return_kqv, self.fixed_size, self.mode_selected = return_kqv, fixed_size, mode_selected
        self.set_precision(precision or bb.default_precision())
        self.set_range_guard(range_guard)

    def supports_grouping(self) -> bool:
        return not (len(self.multilayers) == 1 and self.return_cls)

    def _tap_bn(self):
        if len(self.multilayers) == 1 and self.return_cls:  # x[:, 0] leaves before any norm (beit_v2.py:267-268)
            return None, 2
        return super()._tap_bn()

    def _engine_images(self, images):
        """The resize to the model's image size that ``forward`` starts with (also what the f16x2 range guard audits)."""
        if tuple(images.shape[-2:]) != self.img_size:  # (a same-size bilinear resize with align_corners=False returns its input's values)
            with torch.no_grad():
                images = MF.interpolate(images, size=self.img_size, mode="bilinear", align_corners=False)  # beit_v2.py:255-257
        return images

    def forward(self, images):
        images = self._engine_images(images)
        single_cls = len(self.multilayers) == 1 and self.return_cls
        taps = self._extract(images, want_cls=single_cls)
        if isinstance(taps, bb.TapGroups):  # several batches stacked into one forward (mvp/pipeline.py): one result per batch
            return pipeline.GroupedFeatures((t[0] if len(t) == 1 else t) for t in taps)
        if single_cls:
            return taps.cls[0]
        return taps[0] if len(taps) == 1 else taps
