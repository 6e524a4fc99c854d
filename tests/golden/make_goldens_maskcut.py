"""Records tests/golden/maskcut.npz from the reference's own MaskCut code on the seeded fixtures of tests/maskcut_ref.py:

    python tests/golden/make_goldens_maskcut.py <path to a checkout of the reference>

evals/models/maskcut_processor.py is loaded by file path behind empty stubs of the modules it imports and this machine lacks or that
would pull the rest of the reference in (torchvision, pydensecrf through evals.models.crf, pycocotools, wandb, seaborn, matplotlib,
evals.utils.metric).  Recorded per fixture and pass: the outputs of its get_affinity_matrix(is_wandb=False) with a seeded KMeans
(n_init=10, random_state=0; the reference's is unseeded) and the tau that KMeans gave, second_smallest_eigenvector,
get_salient_areas, check_num_fg_corners, detect_box and, on the square grids its view(dim, ps, ps) can take,
get_masked_affinity_matrix.  maskcut_forward itself calls .cuda() and cannot be recorded: the seed, the reversal and the chaining of
the passes between the recorded calls are the oracle's (tests/maskcut_ref.py), which the goldens then hold step by step.  The
reference is read only while this script runs; nothing of it is stored but numbers."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import maskcut_ref as ref  # noqa: E402


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def load_processor(root):
    ident = lambda *a, **k: None  # noqa: E731
    tv = _stub("torchvision")
    tv.transforms = _stub("torchvision.transforms", Compose=ident, ToTensor=ident, Normalize=ident)
    for name in ("pycocotools", "wandb", "seaborn", "evals", "evals.utils", "evals.models"):
        _stub(name)
    sys.modules["pycocotools"].mask = _stub("pycocotools.mask")
    sys.modules["evals.utils"].metric = _stub("evals.utils.metric")
    _stub("evals.models.crf", densecrf=ident)
    try:
        import matplotlib.pyplot  # noqa: F401
    except Exception:
        _stub("matplotlib").pyplot = _stub("matplotlib.pyplot")
    spec = importlib.util.spec_from_file_location("ref_maskcut_processor", os.path.join(root, "evals", "models", "maskcut_processor.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from sklearn.cluster import KMeans

    taus = []

    class SeededKMeans(KMeans):
        def __init__(self, n_clusters=2):
            super().__init__(n_clusters=n_clusters, n_init=10, random_state=0)

        def fit(self, X, *a, **k):
            out = super().fit(X, *a, **k)
            taus.append(float(np.mean(self.cluster_centers_)))
            return out

    mod.KMeans = SeededKMeans
    return mod.MaskCutProcessor(backbone=None), taus


def main(root):
    proc, taus = load_processor(root)
    out = {}
    for name in ref.FIXTURES:
        f, lab, h, w, P = ref.fixture(name)
        feats = torch.from_numpy(f)
        painting = torch.zeros(h, w)
        orc = ref.maskcut(f, h, w, P)
        for k in range(P):
            if k >= 1:
                if h != w:
                    break  # get_masked_affinity_matrix views the features as (dim, ps, ps)
                prev = torch.from_numpy(orc["passes"][k - 1]["mask"].astype(np.float32))
                feats, painting = proc.get_masked_affinity_matrix(painting, feats, prev, h)
                out[f"{name}/{k}/painting"] = painting.numpy().astype(np.uint8)
                out[f"{name}/{k}/zero_cols"] = (feats.abs().sum(dim=0) == 0).numpy()
            A, D = proc.get_affinity_matrix(feats, 0.15, is_wandb=False)
            eigenvec, second = proc.second_smallest_eigenvector(A, D)
            bip = proc.get_salient_areas(second)
            nc = proc.check_num_fg_corners(bip, [h, w])
            # the seed and the reversal between the recorded calls: the oracle's, on the reference's own eigenvector
            o = ref.partition(ref.fix_sign(second), h, w, painting.numpy(), None, False)
            _, _, objects, cc = proc.detect_box(o["bip"].astype(float), o["seed"], [h, w], scales=[16, 16], initial_im_size=[h * 16, w * 16])
            comp = np.zeros((h, w), dtype=np.uint8)
            comp[cc[0], cc[1]] = 1
            out[f"{name}/{k}/tau"] = np.float64(taus[-1])
            out[f"{name}/{k}/W_on"] = np.packbits(A > 0.5)
            out[f"{name}/{k}/d"] = np.diag(D).astype(np.float64)
            out[f"{name}/{k}/eigvec"] = np.asarray(second, dtype=np.float64)
            out[f"{name}/{k}/bipartition"] = np.asarray(bip).astype(np.uint8)
            out[f"{name}/{k}/nc"] = np.int64(nc)
            out[f"{name}/{k}/seed"] = np.int64(o["seed"])
            out[f"{name}/{k}/component"] = comp
            print(name, k, "tau", taus[-1], "oracle tau", orc["passes"][k]["tau"], "nc", nc, "component", int(comp.sum()))
    path = os.path.join(HERE, "maskcut.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    # configs/objectness_eval.yaml as parsed: its digest, and the four values this package's file changes
    import hashlib
    import json

    import yaml

    cfg = yaml.safe_load(open(os.path.join(root, "configs", "objectness_eval.yaml")))
    dataset = next(d["dataset"] for d in cfg["defaults"] if isinstance(d, dict) and "dataset" in d)
    rec = {"objectness_eval": hashlib.sha256(json.dumps(cfg, sort_keys=True).encode()).hexdigest(),
           "reference_values": {"num_gpus": cfg["system"]["num_gpus"], "wandb_use": cfg["wandb"]["use"], "dataset": dataset,
                                "output_dir": cfg["output_dir"]}}
    with open(os.path.join(HERE, "reference_config_digest_objectness_eval.json"), "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
