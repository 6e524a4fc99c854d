"""Frozen ConvNeXt / ConvNeXt V2 trunk on the HIP path (evals/models/convnext.py:27-47,87-98: the reference runs timm's
``stem`` and ``stages`` and taps the four stage outputs; no final norm, no head).

Activations are channels-last: a stage's map is a [B*H*W, C] row matrix, the ViT engines' token matrix.  The fp32 residual stream is
kept (the depthwise convolution reads it); MFMA operands are bf16 pairs.  Per block:
  mvp_dwconv7_ln_fwd (depthwise 7x7 + LayerNorm -> fc1's A operand), fc1 GEMM + erf GELU, V2: mvp_grn_stats / mvp_grn_apply,
  fc2 GEMM + (V1: LayerScale) + the fp32 block input as residual.
Between stages: mvp_layernorm_fwd + the 2x2 / 2 implicit-GEMM convolution (odd sides floor, as nn.Conv2d).  Stem: 4x4 / 4 patch gather
(K = 48 padded to 64) + GEMM + LayerNorm.  Every LayerNorm eps is 1e-6.

Engine key layout = timm's ConvNeXt: stem.0 (conv) / stem.1 (LayerNorm), stages.i.downsample.0 (LayerNorm) / .1 (conv) for i > 0,
stages.i.blocks.j.{conv_dw, norm, mlp.fc1, mlp.fc2, gamma (V1), mlp.grn (V2)}.  ``to_engine`` also takes transformers'
ConvNextModel / ConvNextV2Model layout and open_clip's ``visual.trunk.`` prefix.
"""
from __future__ import annotations

import math
from typing import Dict, List, Sequence

import torch

from . import conv as cv
from . import lib, ops, pipeline
from .vit import TapOutputs, parse_precision

WIDTHS_B = (128, 256, 512, 1024)
DEPTHS_B = (3, 3, 27, 3)
LN_EPS = 1e-6
STEM_K = 64  # 3 * 4 * 4 = 48 patch values padded to the GEMM's K multiple

_HF_BLOCK = (("dwconv", "conv_dw"), ("layernorm", "norm"), ("pwconv1", "mlp.fc1"), ("pwconv2", "mlp.fc2"), ("grn", "mlp.grn"))


def to_engine(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """A checkpoint in transformers' (``embeddings.*``, ``encoder.stages.*``; optional ``convnext.`` / ``convnextv2.`` prefix) or timm's
    (``stem.*``, ``stages.*``; optional open_clip ``visual.trunk.`` / ``trunk.`` prefix) layout -> the engine's (timm's, trunk only:
    ``norm_pre`` and ``head`` are never run by the reference's forward).  GRN parameters come out as [4C] vectors."""
    sd = {k: v for k, v in sd.items() if torch.is_tensor(v)}
    for pre in ("convnextv2.", "convnext.", "visual.trunk.", "trunk."):
        if any(k.startswith(pre) for k in sd):
            sd = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
    out: Dict[str, torch.Tensor] = {}
    if any(k.startswith("embeddings.") for k in sd):
        for k, v in sd.items():
            if k.startswith("embeddings.patch_embeddings."):
                out["stem.0." + k.rsplit(".", 1)[1]] = v
            elif k.startswith("embeddings.layernorm."):
                out["stem.1." + k.rsplit(".", 1)[1]] = v
            elif k.startswith("encoder.stages."):
                parts = k.split(".")
                i = parts[2]
                if parts[3] == "downsampling_layer":
                    out[f"stages.{i}.downsample.{parts[4]}.{parts[5]}"] = v
                elif parts[3] == "layers":
                    j, rest = parts[4], ".".join(parts[5:])
                    if rest == "layer_scale_parameter":
                        out[f"stages.{i}.blocks.{j}.gamma"] = v
                        continue
                    for src, dst in _HF_BLOCK:
                        if rest.startswith(src + "."):
                            out[f"stages.{i}.blocks.{j}.{dst}.{rest[len(src) + 1:]}"] = v
    else:
        for k, v in sd.items():
            if k.startswith("stem.") or (k.startswith("stages.") and (".blocks." in k or ".downsample." in k)):
                out[k] = v
    if "stem.0.weight" not in out:
        raise ValueError("not a ConvNeXt checkpoint: neither embeddings.patch_embeddings.weight nor stem.0.weight")
    return {k: (v.reshape(-1) if ".mlp.grn." in k else v).detach().float().contiguous() for k, v in out.items()}


def engine_to_hf(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The inverse of ``to_engine`` for transformers' ConvNextModel / ConvNextV2Model (without their final ``layernorm``)."""
    out = {}
    for k, v in sd.items():
        parts = k.split(".")
        if parts[0] == "stem":
            out[("embeddings.patch_embeddings." if parts[1] == "0" else "embeddings.layernorm.") + parts[2]] = v
        elif parts[2] == "downsample":
            out[f"encoder.stages.{parts[1]}.downsampling_layer.{parts[3]}.{parts[4]}"] = v
        else:
            i, j, rest = parts[1], parts[3], ".".join(parts[4:])
            if rest == "gamma":
                out[f"encoder.stages.{i}.layers.{j}.layer_scale_parameter"] = v
                continue
            for dst, src in _HF_BLOCK:
                if rest.startswith(src + "."):
                    leaf = rest[len(src) + 1:]
                    out[f"encoder.stages.{i}.layers.{j}.{dst}.{leaf}"] = v.reshape(1, 1, 1, -1) if dst == "grn" else v
    return out


def engine_to_timm(sd: Dict[str, torch.Tensor], prefix: str = "") -> Dict[str, torch.Tensor]:
    """The engine's layout is timm's; ``prefix`` = 'visual.trunk.' gives the open_clip file's keys."""
    return {prefix + k: v for k, v in sd.items()}


def random_state_dict(widths: Sequence[int] = WIDTHS_B, depths: Sequence[int] = DEPTHS_B, v2: bool = False, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Seeded weights in the engine's layout with O(1) statistics everywhere.  (The published initialisation — LayerScale 1e-6, GRN
    gamma = beta = 0, zero biases — makes every block the identity to seven digits and GRN a no-op: a forward on such weights tests
    nothing.)  LayerScale: uniform in +-[0.5, 1.5]; GRN gamma / beta: N(0, 1); LayerNorm weight: uniform [0.5, 1.5], bias N(0, 0.5);
    conv / linear biases N(0, 0.5); weights scaled to keep activations O(1)."""
    g = torch.Generator().manual_seed(seed)

    def rn(*shape, std=1.0):
        return torch.randn(*shape, generator=g) * std

    def ln(name, c):
        sd[name + ".weight"] = 0.5 + torch.rand(c, generator=g)
        sd[name + ".bias"] = rn(c, std=0.5)

    sd: Dict[str, torch.Tensor] = {}
    sd["stem.0.weight"], sd["stem.0.bias"] = rn(widths[0], 3, 4, 4, std=1.0 / math.sqrt(48.0)), rn(widths[0], std=0.5)
    ln("stem.1", widths[0])
    for i, (c, n) in enumerate(zip(widths, depths)):
        if i > 0:
            ln(f"stages.{i}.downsample.0", widths[i - 1])
            sd[f"stages.{i}.downsample.1.weight"] = rn(c, widths[i - 1], 2, 2, std=1.0 / math.sqrt(4.0 * widths[i - 1]))
            sd[f"stages.{i}.downsample.1.bias"] = rn(c, std=0.5)
        for j in range(n):
            p = f"stages.{i}.blocks.{j}."
            sd[p + "conv_dw.weight"], sd[p + "conv_dw.bias"] = rn(c, 1, 7, 7, std=1.0 / 7.0), rn(c, std=0.5)
            ln(p + "norm", c)
            sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = rn(4 * c, c, std=1.0 / math.sqrt(c)), rn(4 * c, std=0.5)
            sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = rn(c, 4 * c, std=1.0 / math.sqrt(4.0 * c)), rn(c, std=0.5)
            if v2:
                sd[p + "mlp.grn.weight"], sd[p + "mlp.grn.bias"] = rn(4 * c), rn(4 * c)
            else:
                sign = (torch.rand(c, generator=g) < 0.5).float() * 2.0 - 1.0
                sd[p + "gamma"] = sign * (0.5 + torch.rand(c, generator=g))
    return sd


def arch_of(sd: Dict[str, torch.Tensor]):
    """(widths, depths, v2) of an engine-layout state dict."""
    n_stage = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("stages."))
    depths = [1 + max(int(k.split(".")[3]) for k in sd if k.startswith(f"stages.{i}.blocks.")) for i in range(n_stage)]
    widths = [int(sd[f"stages.{i}.blocks.0.conv_dw.weight"].shape[0]) for i in range(n_stage)]
    return widths, depths, any(".mlp.grn." in k for k in sd)


class ConvNeXtEngine:
    def __init__(self, state_dict: Dict[str, torch.Tensor], depths: Sequence[int], widths: Sequence[int], *, precision="bf16x3", device="cuda"):
        self.device = torch.device(device)
        self.pr = parse_precision(precision)
        if self.pr == lib.PREC_F16X2:  # a mode of the ViT blocks' GEMMs: the convolution trunk has no two-product kernels
            self.pr = lib.PREC_BF16X3
        pr = self.pr
        sd = {k: v.detach().to(self.device, torch.float32).contiguous() for k, v in state_dict.items() if v.dtype.is_floating_point}
        self.depths, self.widths = list(depths), list(widths)
        for c in self.widths:
            if c % 64 or not 64 <= c <= 2048:
                raise lib.MvpError(f"ConvNeXt on the HIP path needs stage widths that are multiples of 64 in 64..2048 (got {c})")
        c0 = self.widths[0]
        wk = sd["stem.0.weight"].reshape(c0, -1)  # k = c*16 + ky*4 + kx: the patch gather's column order
        wpad = wk.new_zeros(c0, STEM_K)
        wpad[:, : wk.shape[1]] = wk
        self.stem_w, self.stem_b = ops.split_bf16(wpad.contiguous(), pr), sd["stem.0.bias"]
        self.stem_ln = (sd["stem.1.weight"], sd["stem.1.bias"])
        self.v2 = any(".mlp.grn." in k for k in sd)
        self.down: List[dict] = [None]
        self.blocks: List[List[dict]] = []
        for i, (c, n) in enumerate(zip(self.widths, self.depths)):
            if i > 0:
                p = f"stages.{i}.downsample."
                self.down.append(dict(ln=(sd[p + "0.weight"], sd[p + "0.bias"]), w=cv.pack_weight(sd[p + "1.weight"], 0, pr), b=sd[p + "1.bias"]))
            stage = []
            for j in range(n):
                p = f"stages.{i}.blocks.{j}."
                blk = dict(dw_w=sd[p + "conv_dw.weight"].reshape(c, 49).contiguous(), dw_b=sd[p + "conv_dw.bias"],
                           ln=(sd[p + "norm.weight"], sd[p + "norm.bias"]),
                           w1=ops.split_bf16(sd[p + "mlp.fc1.weight"], pr), b1=sd[p + "mlp.fc1.bias"],
                           w2=ops.split_bf16(sd[p + "mlp.fc2.weight"], pr), b2=sd[p + "mlp.fc2.bias"])
                if self.v2:
                    blk["grn"] = (sd[p + "mlp.grn.weight"].reshape(-1).contiguous(), sd[p + "mlp.grn.bias"].reshape(-1).contiguous())
                else:
                    blk["gamma"] = sd[p + "gamma"]
                stage.append(blk)
            self.blocks.append(stage)
        pipeline.publish()  # the split weights are read by forwards on any stream

    # ------------------------------------------------------------------ pieces (x = fp32 [B*H*W, C])
    def _stem(self, images: torch.Tensor, pad_top: int, pad_left: int, gh: int, gw: int) -> torch.Tensor:
        B = images.shape[0]
        pr, dev, c0 = self.pr, self.device, self.widths[0]
        M = B * gh * gw
        col = ops.empty_pair((M, STEM_K), pr, dev)
        ops.patch_gather_ld(images, col, 4, gh, gw, pad_top, pad_left, STEM_K)
        x = torch.empty(M, c0, dtype=torch.float32, device=dev)
        ops.gemm(col, self.stem_w, M, c0, STEM_K, bias=self.stem_b, out_f32=x, precision=pr, splitk=1)
        ops.layernorm(x, self.stem_ln[0], self.stem_ln[1], None, M, c0, LN_EPS, out_f32=x)
        return x

    def _block(self, blk: dict, x: torch.Tensor, B: int, H: int, W: int, C: int) -> torch.Tensor:
        pr, dev = self.pr, self.device
        M, C4 = B * H * W, 4 * C
        a = ops.empty_pair((M, C), pr, dev)
        ops.dwconv7_ln(x, blk["dw_w"], blk["dw_b"], blk["ln"][0], blk["ln"][1], a, B, H, W, C, LN_EPS)
        hP = ops.empty_pair((M, C4), pr, dev)
        y = torch.empty(M, C, dtype=torch.float32, device=dev)
        if self.v2:
            h = torch.empty(M, C4, dtype=torch.float32, device=dev)
            ops.gemm(a, blk["w1"], M, C4, C, bias=blk["b1"], out_f32=h, act=lib.ACT_GELU, precision=pr, splitk=1)
            G = torch.empty(B, C4, dtype=torch.float32, device=dev)
            N = torch.empty(B, C4, dtype=torch.float32, device=dev)
            ws = torch.empty(ops.grn_workspace_bytes(B, H * W, C4) // 8, dtype=torch.float64, device=dev)
            ops.grn_stats(h, G, N, ws, B, H * W, C4)
            ops.grn_apply(h, N, blk["grn"][0], blk["grn"][1], hP, B, H * W, C4)
            ops.gemm(hP, blk["w2"], M, C, C4, bias=blk["b2"], residual=x, out_f32=y, precision=pr, splitk=1)
        else:
            ops.gemm(a, blk["w1"], M, C4, C, bias=blk["b1"], out=hP, act=lib.ACT_GELU, precision=pr, splitk=1)
            ops.gemm(hP, blk["w2"], M, C, C4, bias=blk["b2"], residual=x, out_f32=y, precision=pr, col_scale=blk["gamma"])
        return y

    def _downsample(self, d: dict, x: torch.Tensor, B: int, H: int, W: int, C: int, Cout: int):
        pr, dev = self.pr, self.device
        a = ops.empty_pair((B * H * W, C), pr, dev)
        ops.layernorm(x, d["ln"][0], d["ln"][1], a, B * H * W, C, LN_EPS)
        g = cv.geom(B, H, W, C, 2, 2, 2, 0)
        y = torch.empty(B * g["Ho"] * g["Wo"], Cout, dtype=torch.float32, device=dev)
        cv.conv_gemm(a, g, d["w"], Cout, bias=d["b"], out_f32=y, precision=pr)
        return y, g["Ho"], g["Wo"]

    # ------------------------------------------------------------------ forward
    def forward_taps(self, images: torch.Tensor, multilayers: Sequence[int], *, pad_to: int = 4) -> TapOutputs:
        """images: [B, 3, H, W] fp32 device.  Sides are zero-padded to a multiple of ``pad_to`` inside the stem's gather exactly as
        evals/models/utils.py:55-72 (center_padding) pads them; ``pad_to`` must be a multiple of 4.  Returns NCHW fp32 maps of the
        stage indices in ``multilayers`` (0 ... 3) at the stages' own resolutions, in stage order."""
        images = images.to(self.device, torch.float32).contiguous()
        B, _, H, W = images.shape
        if pad_to % 4 or not multilayers or min(multilayers) < 0 or max(multilayers) >= len(self.widths):
            raise lib.MvpError(f"ConvNeXtEngine.forward_taps: bad pad_to / multilayers ({pad_to}, {list(multilayers)})")
        dh, dw = H % pad_to, W % pad_to
        ph, pw = (pad_to - dh, pad_to - dw) if (dh or dw) else (0, 0)  # (a non-ragged side gets a full patch when the other is ragged)
        Hp, Wp = H + ph, W + pw
        if Hp < 32 or Wp < 32:
            raise lib.MvpError(f"ConvNeXt needs a padded input of at least 32 x 32 (got {Hp} x {Wp}): three 2x2 / 2 downsamples follow the 4x4 / 4 stem")
        h, w = Hp // 4, Wp // 4
        x = self._stem(images, ph // 2, pw // 2, h, w)
        outs = TapOutputs()
        outs.dims = []
        last = max(multilayers)
        for i, C in enumerate(self.widths):
            if i > 0:
                x, h, w = self._downsample(self.down[i], x, B, h, w, self.widths[i - 1], C)
            for blk in self.blocks[i]:
                x = self._block(blk, x, B, h, w, C)
            if i in multilayers:
                hw = h * w
                nchw = torch.empty(B, C, h, w, dtype=torch.float32, device=self.device)
                ws = torch.empty(ops.bn_tokens_workspace_bytes(B * hw, C) // 4 + 16, dtype=torch.float32, device=self.device)
                ops.bn_tokens_to_nchw(x, B, hw, C, hw, workspace=ws, nchw=nchw, mode=2)  # mode 2: no normalisation, the transpose alone
                outs.append(nchw)
                outs.dims.append((C, h, w))
            if i == last:
                break
        return outs
