"""How much of fp16's range does a backbone use?  Builds a ViT wrapper from its config with ``range_guard="warn"``, runs ONE batch and
prints the table of the guard's audited forward (mvp/backbone.py ``resolve_range_guard``, mvp/vit.py ``RangeAudit``): per fp16-form
operand of every block the largest |v|, its share of fp16's range (65504), and the counts of saturated and non-finite elements.

    python tools/f16_range.py backbone=<choice> [image=224] [batch=4] [images=<file.pt>] [precision=f16x2]

``backbone``: a file under midvision-probe_amd/configs/backbone (dino_b16, dinov2_g14, clip_b16, ...).  The weights are what the
wrapper finds: a checkpoint under MVP_CKPT_DIR, else seeded random init (which says nothing about a published model: this tool is for
whoever has the file).  ``images``: a tensor file [B, 3, H, W] of normalised images; synthetic N(0, 1) images otherwise; either way
the wrapper's own preprocessing (a resize, a rebuilt position table) is applied before the audit, as in its forward.  Exit status 1
when a site tripped."""
from __future__ import annotations

import importlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "midvision-probe_amd")]

import torch  # noqa: E402

F16_MAX = 65504.0


def table(report) -> str:
    rows = [f"{'site':<52} {'max |v|':>12} {'of range':>9} {'saturated':>10} {'non-finite':>10} {'scanned':>12}"]
    for r in report:
        share = r["max_abs"] / F16_MAX if r["max_abs"] == r["max_abs"] else float("nan")
        flag = "  <-- beyond fp16's range" if r["n_sat"] + r["n_nonfinite"] else ""
        rows.append(f"{r['site']:<52} {r['max_abs']:>12.6g} {share:>8.2%} {r['n_sat']:>10d} {r['n_nonfinite']:>10d} {r['n_scanned']:>12d}{flag}")
    return "\n".join(rows)


def main(argv) -> int:
    from mvp import backbone as bb
    from mvp import config

    kv = dict(a.split("=", 1) for a in argv)
    unknown = set(kv) - {"backbone", "image", "batch", "images", "precision"}
    if "backbone" not in kv or unknown:
        raise SystemExit(__doc__)
    if not torch.cuda.is_available():
        raise SystemExit("tools/f16_range.py runs the backbone on the GPU: no device found")
    dev = torch.device("cuda:0")
    node = config._load(os.path.join(config.CONFIG_DIR, "backbone", kv["backbone"] + ".yaml"))
    mod, _, name = node["_target_"].rpartition(".")
    if not issubclass(getattr(importlib.import_module(mod), name), bb.ViTBackbone):  # (before the keyword only those wrappers take)
        raise SystemExit(f"backbone={kv['backbone']}: not a ViT wrapper (the ResNet and ConvNeXt engines never run f16x2)")
    model = config.instantiate(node, range_guard="warn", precision=kv.get("precision", "f16x2")).to(dev).eval()
    if "images" in kv:
        images = torch.load(kv["images"], map_location="cpu", weights_only=True).float()
    else:
        s, b = int(kv.get("image", 224)), int(kv.get("batch", 4))
        images = torch.randn(b, 3, s, s, generator=torch.Generator().manual_seed(0))
    source = "a checkpoint file" if model.weights_from_file else "seeded random init (NOT the published weights)"
    print(f"# {kv['backbone']}: weights from {source}; images {tuple(images.shape)}; precision {kv.get('precision', 'f16x2')}")
    model.resolve_range_guard(images.to(dev))
    report = model.f16_range_report()
    if not report:
        print("no fp16-form operands on this engine: nothing to audit")
        return 0
    print(table(report))
    bad = [r for r in report if r["n_sat"] + r["n_nonfinite"]]
    top = max(r["max_abs"] if r["max_abs"] == r["max_abs"] else float("inf") for r in report)
    print(f"# {len(bad)} of {len(report)} sites beyond fp16's range; largest |v| {top:.6g} = {top / F16_MAX:.2%} of the range"
          + ("" if not bad else f"; first: {bad[0]['site']}: run this model with precision='bf16x3'"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
