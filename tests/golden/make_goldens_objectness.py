"""Records tests/golden/objectness.npz and reference_config_digests_objectness.json from the reference's own code on seeded inputs:

    python tests/golden/make_goldens_objectness.py <path to a checkout of the reference>

evals/models/probes.py and evals/utils/optim.py are loaded by file path (they import torch and numpy only).
train_generic_objectness.py imports wandb and hydra at module level, so its five ``compute_*`` metric helpers are taken out of the
file with ``ast`` and executed on their own.  The reference is read only while this script runs; nothing of it is stored but numbers.

Conditioning.  BatchNorm divides by the batch spread sigma of the trunk's output, so an error eps there becomes eps / sigma after it,
and a randomly initialised trunk can be nearly constant over the batch.  Every recorded case therefore has sigma >= 0.3 x the rms of
its pre-BatchNorm map (the seeded conv weights of the
trunk are doubled until it holds; the rms is taken with and without the last conv's bias), and rms / sigma is stored with it:
the factor by which BatchNorm amplifies a relative error of the trunk."""
import ast
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from oracle import probes as oprobes  # noqa: E402

C, HID, B, TOK, MASK = 8, 16, 2, 4, 24
FEAT_DIM = [C] * 4


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _metric_helpers(path):
    tree = ast.parse(open(path).read())
    want = ["compute_precision_recall", "compute_f_measure", "compute_iou", "compute_accuracy", "compute_corloc"]
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert sorted(n.name for n in body) == sorted(want)
    ns = {"np": np}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in want]


def _np(t):
    return t.detach().cpu().numpy()


def _weights(head_type, k, out_dim, seed):
    if head_type == "linear":
        return oprobes.make_linear_head_weights(FEAT_DIM, out_dim, k, seed=seed), "head.conv.weight"
    if head_type == "multiscale":
        return oprobes.make_multiscale_weights(FEAT_DIM, out_dim, hidden=HID, k=k, seed=seed), "head.conv_out.2.weight"
    return oprobes.make_dpt_weights(FEAT_DIM, out_dim, hidden=HID, k=k, seed=seed), "head.out_conv.2.weight"


def _amplification(probe, feats, last_bias):
    """rms / sigma of the pre-BatchNorm map, the worst channel — of the map as it is and of the map without the last conv's bias (a bias
    that happens to cancel the mean does not cancel the trunk's rounding errors), whichever is larger."""
    with torch.no_grad():
        x = probe.head([f.clone() for f in feats]).double()
    sigma = x.var(dim=(0, 2, 3), unbiased=False).sqrt()
    rms = x.pow(2).mean(dim=(0, 2, 3)).sqrt()
    rms0 = (x - last_bias.double()[None, :, None, None]).pow(2).mean(dim=(0, 2, 3)).sqrt()
    return float((torch.maximum(rms, rms0) / sigma).max())


def _build(pr, head_type, k, out_dim, pred_type, seed, feats_list):
    """BinaryHead with seeded weights, every conv weight of its trunk doubled until sigma >= 0.3 rms on every feature set of
    ``feats_list`` (torch's default init shrinks the spread from layer to layer while the biases stay: scaling the last conv alone
    would scale its nearly constant input's mean along with the spread)."""
    probe = pr.BinaryHead(feat_dim=FEAT_DIM, head_type=head_type, hidden_dim=HID, kernel_size=k, output_dim=out_dim, pred_type=pred_type)
    sd, last = _weights(head_type, k, out_dim, seed)
    for _ in range(6):
        full = dict(probe.state_dict())
        full.update(sd)
        probe.load_state_dict(full, strict=True)
        amp = max(_amplification(probe, f, sd[last.replace(".weight", ".bias")]) for f in feats_list)
        if amp <= 1.0 / 0.3:
            return probe, {k_: v.clone() for k_, v in probe.state_dict().items()}, amp
        sd = {k_: (v * 2.0 if k_.endswith(".weight") else v) for k_, v in sd.items()}
    raise AssertionError(f"{head_type} k{k}: sigma stayed below 0.3 rms")


def main():
    ref = os.path.abspath(sys.argv[1])
    pr = _load(os.path.join(ref, "evals", "models", "probes.py"), "ref_probes")
    op = _load(os.path.join(ref, "evals", "utils", "optim.py"), "ref_optim")
    g = torch.Generator().manual_seed(20241019)
    out = {}
    feats = [torch.randn(B, C, TOK, TOK, generator=g) for _ in range(4)]
    mask = (torch.rand(B, 1, MASK, MASK, generator=g) < 0.4).float()
    out["feats"], out["mask"] = np.stack([_np(f) for f in feats]), _np(mask)
    bce = torch.nn.BCELoss()

    for name, head_type, k, seed in (("lin_k1", "linear", 1, 41), ("lin_k3", "linear", 3, 42), ("ms_k1", "multiscale", 1, 43), ("dpt_k3", "dpt", 3, 44)):
        probe, sd, amp = _build(pr, head_type, k, 1, "sigmoid", seed, [feats])
        # a non-trivial affine and non-default running statistics, so that both are seen to be used
        with torch.no_grad():
            probe.batch_norm.weight.fill_(1.3)
            probe.batch_norm.bias.fill_(-0.2)
            probe.batch_norm.running_mean.fill_(0.05)
            probe.batch_norm.running_var.fill_(0.8)
        sd = {k_: v.clone() for k_, v in probe.state_dict().items()}
        for k_, v in sd.items():
            out[f"{name}__sd__{k_}"] = _np(v)
        y = probe([f.clone() for f in feats])
        loss = bce(F.interpolate(y, size=mask.shape[-2:], mode="bilinear"), mask)
        loss.backward()
        out[f"{name}__out"], out[f"{name}__loss"], out[f"{name}__amp"] = _np(y), _np(loss), np.float64(amp)
        out[f"{name}__name"] = np.array(probe.name)
        for n, p in probe.named_parameters():
            if head_type == "linear" or n.startswith("batch_norm."):
                out[f"{name}__grad__{n}"] = _np(p.grad)
        for b in ("running_mean", "running_var", "num_batches_tracked"):
            out[f"{name}__after__{b}"] = _np(getattr(probe.batch_norm, b))
        probe.eval()
        with torch.no_grad():
            out[f"{name}__eval_out"] = _np(probe([f.clone() for f in feats]))
        print(name, tuple(y.shape), probe.name, f"loss {float(loss.detach()):.6f} rms/sigma {amp:.3f}")

    probe, sd, amp = _build(pr, "linear", 1, 2, "sigmoid", 45, [feats])
    for k_, v in sd.items():
        out[f"od2__sd__{k_}"] = _np(v)
    out["od2__out"], out["od2__amp"] = _np(probe([f.clone() for f in feats])), np.float64(amp)
    for b in ("running_mean", "running_var", "num_batches_tracked"):
        out[f"od2__after__{b}"] = _np(getattr(probe.batch_norm, b))
    probe = pr.BinaryHead(feat_dim=FEAT_DIM, head_type="linear", kernel_size=1, output_dim=1, pred_type="tanh")
    probe.load_state_dict(_weights("linear", 1, 1, 46)[0], strict=True)
    for k_, v in probe.state_dict().items():
        out[f"tanh__sd__{k_}"] = _np(v)
    out["tanh__out"] = _np(probe([f.clone() for f in feats]))

    # 8 steps of the reference's loop body (train_generic_objectness.py:376-398) with its optimiser and schedule
    steps = 8
    tf = [[torch.randn(B, C, TOK, TOK, generator=g) for _ in range(4)] for _ in range(steps)]
    tm = [(torch.rand(B, 1, MASK, MASK, generator=g) < 0.4).float() for _ in range(steps)]
    probe, sd, amp = _build(pr, "linear", 1, 1, "sigmoid", 47, tf)
    for k_, v in sd.items():
        out[f"traj__sd__{k_}"] = _np(v)
    opt = torch.optim.AdamW([{"params": probe.parameters(), "lr": 5e-4}])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda e: op.cosine_decay_linear_warmup(e, 30, 2))
    losses = []
    for s in range(steps):
        amp = max(amp, _amplification(probe, tf[s], probe.head.conv.bias.detach()))
        opt.zero_grad()
        pred = F.interpolate(probe([f.clone() for f in tf[s]]), size=tm[s].shape[-2:], mode="bilinear")
        loss = bce(pred, tm[s])
        loss.backward()
        opt.step()
        sched.step()
        losses.append(float(loss.detach()))
    assert amp <= 1.0 / 0.3, amp
    out["traj__feats"] = np.stack([np.stack([_np(f) for f in fs]) for fs in tf])
    out["traj__masks"] = np.stack([_np(m) for m in tm])
    out["traj__losses"], out["traj__amp"] = np.array(losses, dtype=np.float64), np.float64(amp)
    for k_, v in probe.state_dict().items():
        out[f"traj__final__{k_}"] = _np(v)
    print("trajectory", losses, f"rms/sigma {amp:.3f}")

    # metrics table: validation()'s threshold (:446) and the five helpers on it
    prec_rec, f_measure, iou, accuracy, corloc = _metric_helpers(os.path.join(ref, "train_generic_objectness.py"))
    n = 2 * 6 * 6
    preds, gts = [], []
    for _ in range(4):
        preds.append(torch.rand(n, generator=g).numpy())
        gts.append((torch.rand(n, generator=g) < 0.5).float().numpy())
    preds.append(np.full(n, 0.1, np.float32)); gts.append(np.zeros(n, np.float32))       # all background, predicted all background
    preds.append(np.full(n, 0.9, np.float32)); gts.append(np.ones(n, np.float32))        # all foreground, predicted all foreground
    preds.append(np.full(n, 0.5, np.float32)); gts.append(gts[0].copy())                 # exactly 0.5 everywhere: negative
    p = preds[1].copy(); p[::3] = 0.5; preds.append(p); gts.append(gts[1].copy())        # 0.5 mixed in
    preds.append(np.full(n, 0.9, np.float32)); gts.append(np.zeros(n, np.float32))       # all false positives
    p = gts[2].copy() * 0.8 + 0.1; preds.append(p.astype(np.float32)); gts.append(gts[2].copy())  # a perfect prediction
    rows = []
    for p, t in zip(preds, gts):
        bp = (torch.from_numpy(p).view(2, 1, 6, 6) > 0.5).float().numpy()
        gt = t.reshape(2, 1, 6, 6)
        pr_, rc_ = prec_rec(bp, gt)
        rows.append([pr_, rc_, f_measure(pr_, rc_), iou(bp, gt), accuracy(bp, gt), corloc(bp, gt)])
    out["metrics__pred"], out["metrics__gt"] = np.stack(preds).astype(np.float32), np.stack(gts).astype(np.float32)
    out["metrics__table"] = np.array(rows, dtype=np.float64)  # precision, recall, F-measure, IoU, accuracy, CorLoc

    path = os.path.join(HERE, "objectness.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")

    def digest(node):
        return hashlib.sha256(json.dumps(node, sort_keys=True).encode()).hexdigest()

    root = yaml.safe_load(open(os.path.join(ref, "configs", "objectness_train.yaml")))
    # the root file with the two keys this package sets differently blanked (dataset choice, wandb.use): everything else must agree
    root["defaults"] = [({"dataset": None} if isinstance(d, dict) and "dataset" in d else d) for d in root["defaults"]]
    root["wandb"]["use"] = None
    dig = {"probe/binaryhead": digest(yaml.safe_load(open(os.path.join(ref, "configs", "probe", "binaryhead.yaml")))),
           "objectness_train(dataset, wandb.use blanked)": digest(root)}
    with open(os.path.join(HERE, "reference_config_digests_objectness.json"), "w") as f:
        json.dump(dig, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
