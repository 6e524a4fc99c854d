"""evals.models.crocov2.CROCOV2 — drop-in for the reference wrapper (evals/models/crocov2.py:20-178): the encoder of CroCo v2, a plain
ViT-B/16 without a class token and without a position table — Q and K of every block are rotated by the token's (y, x) grid position
(RoPE100; mvp_rope2d_qkv on the HIP path)."""
from __future__ import annotations

from .croco import CROCO


class CROCOV2(CROCO):
    """``CROCO`` with the local checkpoint file ``CroCo_V2_ViTBase_BaseDecoder.pth``, ``checkpoint_name`` ``crocov2_<model>_<output>`` and
    RoPE100 where the checkpoint's ``croco_kwargs`` name no position form."""

    ckpt_key = "crocov2"
    default_pos_embed = "RoPE100"
