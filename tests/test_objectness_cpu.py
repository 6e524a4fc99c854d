"""CPU checks of the objectness probe: the fp64 restatement (tests/objectness_ref.py) against everything the reference recorded
(tests/golden/objectness.npz), the metric formulas, the synthetic dataset, the configs, the entry script's refusals and the new
exports' argument checks.  No GPU."""
import ctypes
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

import objectness_ref as R
from conftest import GOLDEN, PKG, load_golden, rel_l2

DIGESTS = json.load(open(os.path.join(GOLDEN, "reference_config_digests_objectness.json")))
CASES = [("lin_k1", "linear", 1), ("lin_k3", "linear", 3), ("ms_k1", "multiscale", 1), ("dpt_k3", "dpt", 3)]
# fp64 against values the reference computed in fp32: every stored number carries fp32 rounding (6e-8 relative per operation), a map
# or a gradient a few of them in a row.  1e-6 is the issue's bound.
RTOL = 1e-6


@pytest.fixture(scope="module")
def g():
    return load_golden("objectness.npz")


def _sd(g, case):
    pre = f"{case}__sd__"
    return {k[len(pre):]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith(pre)}


def _trunk(sd, feats, head_type, k):
    """The pre-BatchNorm logits in fp64 from the CPU oracle's functional heads (oracle/probes.py)."""
    from oracle import probes as oprobes

    sd = {n: v.double() for n, v in sd.items() if n.startswith("head.")}
    feats = [f.double() for f in feats]
    if head_type == "linear":
        return oprobes.linear_head(sd, feats, k)
    if head_type == "multiscale":
        return oprobes.multiscale_head(sd, feats)
    return oprobes.dpt_head(sd, feats, k)


def _resize(y, size):
    return F.interpolate(y, size=size, mode="bilinear")


@pytest.mark.parametrize("case,head_type,k", CASES)
def test_restatement_matches_reference_forward_loss_and_statistics(g, case, head_type, k):
    sd = _sd(g, case)
    feats = [torch.from_numpy(f) for f in g["feats"]]
    mask = g["mask"].astype(np.float64)
    x = _trunk(sd, feats, head_type, k).numpy()
    bn = {n: sd[f"batch_norm.{n}"].numpy() for n in ("weight", "bias", "running_mean", "running_var")}
    f = R.bn_act_fwd(x, bn["weight"], bn["bias"], bn["running_mean"], bn["running_var"])
    assert f["y"].shape == g[f"{case}__out"].shape
    assert rel_l2(f["y"], g[f"{case}__out"]) < RTOL
    pred = _resize(torch.from_numpy(f["y"]), mask.shape[-2:]).numpy()
    np.testing.assert_allclose(R.bce(pred, mask), float(g[f"{case}__loss"]), rtol=RTOL)
    np.testing.assert_allclose(f["running_mean"], g[f"{case}__after__running_mean"], rtol=RTOL)
    np.testing.assert_allclose(f["running_var"], g[f"{case}__after__running_var"], rtol=RTOL)
    assert int(g[f"{case}__after__num_batches_tracked"]) == int(sd["batch_norm.num_batches_tracked"]) + 1
    e = R.bn_act_fwd(x, bn["weight"], bn["bias"], f["running_mean"], f["running_var"], training=False)
    assert rel_l2(e["y"], g[f"{case}__eval_out"]) < RTOL
    assert 1.0 <= float(g[f"{case}__amp"]) <= 1.0 / 0.3
    assert str(g[f"{case}__name"]) == f"snorm_{head_type}_k{k}"


@pytest.mark.parametrize("case,head_type,k", CASES)
def test_restatement_matches_reference_gradients(g, case, head_type, k):
    sd = _sd(g, case)
    feats = [torch.from_numpy(f) for f in g["feats"]]
    mask = g["mask"].astype(np.float64)
    params = {n: v.double().requires_grad_(True) for n, v in sd.items() if n.startswith("head.")}
    x = _trunk(params, feats, head_type, k)
    bn = {n: sd[f"batch_norm.{n}"].numpy() for n in ("weight", "bias", "running_mean", "running_var")}
    y = torch.from_numpy(R.bn_act_fwd(x.detach().numpy(), bn["weight"], bn["bias"])["y"]).requires_grad_(True)
    pred = _resize(y, mask.shape[-2:])
    pred.backward(torch.from_numpy(R.bce_grad(pred.detach().numpy(), mask)))
    b = R.bn_act_bwd(x.detach().numpy(), y.grad.numpy(), bn["weight"], bn["bias"])
    np.testing.assert_allclose(b["grad_gamma"], g[f"{case}__grad__batch_norm.weight"], rtol=1e-5)  # a sum of 512..8192 fp32 terms of both signs
    np.testing.assert_allclose(b["grad_beta"], g[f"{case}__grad__batch_norm.bias"], rtol=1e-5)     # (likewise)
    if head_type != "linear":
        return
    x.backward(torch.from_numpy(b["grad_x"]))
    gw = g[f"{case}__grad__head.conv.weight"]
    # the conv's weight gradient is an fp32 reduction over 512 pixels x batch in the reference: a few 1e-7 per term
    assert rel_l2(params["head.conv.weight"].grad.numpy(), gw) < 5e-6
    # the gradient of a bias in front of a train-mode BatchNorm is exactly zero (the batch mean absorbs a constant): what the reference
    # stores is the rounding of its sum over pixels, so it is held absolutely, against the scale of the weight gradient (the same sum
    # over pixels, weighted by features of unit size)
    for db in (params["head.conv.bias"].grad.numpy(), g[f"{case}__grad__head.conv.bias"]):
        assert np.abs(db).max() < 5e-6 * np.linalg.norm(gw)


def test_restatement_matches_two_channel_and_tanh_forward(g):
    feats = [torch.from_numpy(f) for f in g["feats"]]
    sd = _sd(g, "od2")
    x = _trunk(sd, feats, "linear", 1).numpy()
    f = R.bn_act_fwd(x, sd["batch_norm.weight"].numpy(), sd["batch_norm.bias"].numpy(), sd["batch_norm.running_mean"].numpy(), sd["batch_norm.running_var"].numpy())
    assert g["od2__out"].shape == (2, 2, 16, 16) and rel_l2(f["y"], g["od2__out"]) < RTOL
    np.testing.assert_allclose(f["running_var"], g["od2__after__running_var"], rtol=RTOL)
    sd = _sd(g, "tanh")
    assert set(sd) == {"head.conv.weight", "head.conv.bias"}  # no BatchNorm in the tanh form
    x = _trunk(sd, feats, "linear", 1).numpy()
    assert rel_l2(R.bn_act_fwd(x, act="tanh")["y"], g["tanh__out"]) < RTOL


class _RefBnSigmoid(torch.autograd.Function):
    """The restatement as an autograd node (train mode), for the trajectory below."""

    @staticmethod
    def forward(ctx, x, gamma, beta):
        ctx.save_for_backward(x, gamma, beta)
        return torch.from_numpy(R.bn_act_fwd(x.numpy(), gamma.numpy(), beta.numpy())["y"])

    @staticmethod
    def backward(ctx, gy):
        x, gamma, beta = ctx.saved_tensors
        b = R.bn_act_bwd(x.numpy(), gy.numpy(), gamma.numpy(), beta.numpy())
        return torch.from_numpy(b["grad_x"]), torch.from_numpy(b["grad_gamma"]), torch.from_numpy(b["grad_beta"])


class _RefBce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, t):
        ctx.save_for_backward(p, t)
        return torch.tensor(R.bce(p.numpy(), t.numpy()), dtype=torch.float64)

    @staticmethod
    def backward(ctx, g):
        p, t = ctx.saved_tensors
        return torch.from_numpy(R.bce_grad(p.numpy(), t.numpy())) * g, None


def test_restatement_matches_reference_trajectory(g):
    """8 steps of the loop body with AdamW (lr 5e-4) under cosine_decay_linear_warmup(., 30, 2), all in fp64."""
    from evals.utils.optim import cosine_decay_linear_warmup
    from oracle import probes as oprobes

    sd = _sd(g, "traj")
    params = {n: v.double().requires_grad_(True) for n, v in sd.items() if v.is_floating_point() and "running" not in n}
    opt = torch.optim.AdamW([{"params": list(params.values()), "lr": 5e-4}])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda e: cosine_decay_linear_warmup(e, 30, 2))
    losses = []
    for s in range(8):
        feats = [torch.from_numpy(f).double() for f in g["traj__feats"][s]]
        mask = torch.from_numpy(g["traj__masks"][s]).double()
        opt.zero_grad()
        x = oprobes.linear_head({n: p for n, p in params.items() if n.startswith("head.")}, feats, 1)
        y = _RefBnSigmoid.apply(x, params["batch_norm.weight"], params["batch_norm.bias"])
        loss = _RefBce.apply(_resize(y, mask.shape[-2:]), mask)
        loss.backward()
        opt.step()
        sched.step()
        losses.append(float(loss.detach()))
    np.testing.assert_allclose(losses, g["traj__losses"], rtol=RTOL)
    for n, p in params.items():
        if n == "head.conv.bias":
            # A bias in front of a train-mode BatchNorm has gradient zero: what reaches AdamW is rounding noise (1e-9 in the fp32
            # reference, 1e-17 here), and Adam's m / sqrt(v) turns the SIGN of that noise into steps of the size of the learning rate.
            # Its trajectory is therefore not reproducible, only bounded: |step| <= lr_t / (1 - beta1) ... in practice about lr_t; the
            # loss does not depend on it.  Held to twice the summed learning rates.
            lr_sum = sum(5e-4 * cosine_decay_linear_warmup(e, 30, 2) for e in range(8))
            assert abs(p.detach().item() - g[f"traj__final__{n}"].item()) <= 2 * lr_sum
            continue
        # eight AdamW updates of 5e-4 x a sign-like step: the fp32 reference rounds each update to the weight's ulp
        assert rel_l2(p.detach().numpy(), g[f"traj__final__{n}"]) < 2e-6, n
    assert int(g["traj__final__batch_norm.num_batches_tracked"]) == 8


def test_bce_edges_of_the_restatement():
    """p in {0, 1}: 100 and -+1e12 / N against the other target, 0 and 0 against its own (torch's clamps)."""
    p, t = np.array([0.0, 0.0, 1.0, 1.0]), np.array([0.0, 1.0, 0.0, 1.0])
    assert R.bce(p, t) == 50.0
    np.testing.assert_array_equal(R.bce_grad(p, t), np.array([0.0, -1e12, 1e12, 0.0]) / 4)
    tp, tt = torch.tensor(p, requires_grad=True), torch.tensor(t)
    loss = torch.nn.BCELoss()(tp, tt)
    loss.backward()
    assert loss.item() == 50.0
    np.testing.assert_allclose(tp.grad.numpy(), R.bce_grad(p, t), rtol=1e-8)  # torch's 1e-12 is the fp32 constant 9.99999996e-13


def test_metrics_from_counts_equals_the_reference_table_exactly(g):
    from mvp.objectness import metrics_from_counts

    pred, gt, table = g["metrics__pred"], g["metrics__gt"], g["metrics__table"]
    cnt = R.counts(pred, gt)
    assert cnt.sum(axis=1).tolist() == [pred.shape[1]] * pred.shape[0]
    keys = ("Precision", "Recall", "F-measure", "IoU", "Accuracy", "CorLoc")
    for i in range(len(table)):
        m, r = metrics_from_counts(*cnt[i]), R.metrics(*cnt[i])
        assert [repr(float(m[k])) for k in keys] == [repr(float(v)) for v in table[i]], (i, m, table[i])
        assert m == r
    assert table[4][3] == 0.0 and cnt[4].tolist() == [0, 0, 0, pred.shape[1]]      # all background: IoU 0 / (0 + 1e-6)
    assert cnt[5].tolist() == [pred.shape[1], 0, 0, 0] and table[5][5] == 1.0        # all foreground
    assert cnt[6][0] == 0 and cnt[6][1] == 0                                         # exactly 0.5 is negative


def test_synthetic_voc_contract():
    from evals.datasets.synthetic import SyntheticVOC

    ds = SyntheticVOC("trainval", num_samples=6, fixed_size=40, seed=3)
    assert len(ds) == 6
    for i in range(6):
        s = ds[i]
        assert set(s) == {"original_image", "original_image_rgb", "gt_binary_mask", "num_objects"}
        assert s["original_image"].shape == (3, 40, 40) and s["original_image"].dtype == torch.float32
        rgb, m = s["original_image_rgb"], s["gt_binary_mask"]
        assert rgb.shape == (3, 40, 40) and float(rgb.min()) >= 0.0 and float(rgb.max()) <= 1.0
        assert m.shape == (1, 40, 40) and m.dtype == torch.float32
        assert set(m.unique().tolist()) == {0.0, 1.0}  # exact 0 / 1, never empty, never full
        assert isinstance(s["num_objects"], int) and 1 <= s["num_objects"] <= 3
        assert float(rgb[:, m[0] > 0].mean()) > float(rgb[:, m[0] == 0].mean()) + 0.3  # brighter inside the mask
        again = SyntheticVOC("trainval", num_samples=6, fixed_size=40, seed=3)[i]
        assert all(torch.equal(s[k], again[k]) for k in ("original_image", "original_image_rgb", "gt_binary_mask")) and s["num_objects"] == again["num_objects"]
        mean, std = torch.tensor(ds.MEAN).view(3, 1, 1), torch.tensor(ds.STD).view(3, 1, 1)
        torch.testing.assert_close(s["original_image"] * std + mean, rgb)
    assert not torch.equal(ds[0]["gt_binary_mask"], SyntheticVOC("test", 6, 40, 3)[0]["gt_binary_mask"])
    assert not torch.equal(ds[0]["gt_binary_mask"], SyntheticVOC("trainval", 6, 40, 4)[0]["gt_binary_mask"])
    with pytest.raises(ValueError):
        SyntheticVOC("valid")
    with pytest.raises(IndexError):
        ds[6]


def _digest(node):
    return hashlib.sha256(json.dumps(node, sort_keys=True).encode()).hexdigest()


def test_configs_match_the_reference_and_compose():
    from mvp import config

    node = yaml.safe_load(open(os.path.join(config.CONFIG_DIR, "probe", "binaryhead.yaml")))
    assert _digest(node) == DIGESTS["probe/binaryhead"], node
    probe = config.instantiate(node, feat_dim=[768] * 4)
    assert type(probe).__name__ == "BinaryHead" and probe.name == "snorm_dpt_k3"
    assert {k for k in probe.state_dict() if k.startswith("batch_norm.")} == {f"batch_norm.{n}" for n in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")}
    # the root file: the reference's keys and values, `dataset` and `wandb.use` aside
    root = yaml.safe_load(open(os.path.join(config.CONFIG_DIR, "objectness_train.yaml")))
    assert {"dataset": "synthetic_voc"} in root["defaults"] and root["wandb"]["use"] is False
    root["defaults"] = [({"dataset": None} if isinstance(d, dict) and "dataset" in d else d) for d in root["defaults"]]
    root["wandb"]["use"] = None
    assert _digest(root) == DIGESTS["objectness_train(dataset, wandb.use blanked)"], root
    cfg = config.compose("objectness_train", ["batch_size=4", "dataset.fixed_size=56"])
    assert cfg["probe"]["_target_"] == "evals.models.probes.BinaryHead" and cfg["probe"]["output_dim"] == 1
    assert cfg["backbone"]["model_name"] == "vitb14" and cfg["optimizer"]["n_epochs"] == 10 and cfg["batch_size"] == 4
    ds = config.instantiate(cfg["dataset"], split="test")
    assert type(ds).__name__ == "SyntheticVOC" and ds.size == 56 and ds.name == "voc"


def test_heads_signatures_and_state_dict_keys():
    import inspect

    from evals.models.probes import BinaryHead, TaskonomyHead

    want = dict(head_type="dpt", uncertainty_aware=False, hidden_dim=512, kernel_size=1, pred_type="sigmoid")
    for cls, od in ((BinaryHead, 2), (TaskonomyHead, 1)):
        sig = inspect.signature(cls.__init__).parameters
        assert list(sig)[:8] == ["self", "feat_dim", "head_type", "uncertainty_aware", "hidden_dim", "kernel_size", "output_dim", "pred_type"]
        assert {k: sig[k].default for k in want} == want and sig["output_dim"].default == od
        p = cls(feat_dim=[8] * 4, head_type="linear", uncertainty_aware=True)
        assert p.name == "snorm_linear_k1_UA" and p.head.conv.out_channels == od and p.batch_norm.num_features == od
    assert not hasattr(BinaryHead(feat_dim=[8] * 4, head_type="linear", pred_type="tanh"), "batch_norm")
    assert not hasattr(BinaryHead(feat_dim=[8] * 4, head_type="linear", pred_type="raw"), "batch_norm")


def test_reference_state_dict_loads_strict(g):
    from evals.models.probes import BinaryHead

    for case, head_type, k in CASES:
        probe = BinaryHead(feat_dim=[8] * 4, head_type=head_type, hidden_dim=16, kernel_size=k, output_dim=1)
        probe.load_state_dict(_sd(g, case), strict=True)


def _entry():
    spec = importlib.util.spec_from_file_location("train_generic_objectness", os.path.join(PKG, "train_generic_objectness.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("override,word", [("system.num_gpus=2", "num_gpus"), ("optimizer.model_lr=1e-5", "model_lr")])
def test_entry_script_refuses_what_it_does_not_do(override, word):
    with pytest.raises(NotImplementedError, match=word):
        _entry().main([override])


def test_new_exports_reject_bad_arguments():
    """The host-side checks run before any launch (no GPU needed): error code, nothing touched."""
    from mvp import lib

    so = lib.load()
    for cname, st in (("mvp_bn_act_args", lib.BnActArgs), ("mvp_bce_loss_args", lib.BceLossArgs), ("mvp_binary_counts_args", lib.BinaryCountsArgs)):
        assert so.mvp_sizeof(cname.encode()) == ctypes.sizeof(st) and lib.STRUCTS[cname] is st
    ok = dict(x=16, y=16, gamma=16, beta=16, running_mean=16, running_var=16, stats=16, workspace=16, workspace_bytes=lib.BN_ACT_WORKSPACE_BYTES,
              B=2, HW=8, C=2, ld=4, n=16, eps=1e-5, momentum=0.1, act=lib.BN_ACT_SIGMOID, training=1)
    for bad in (dict(x=None), dict(y=None), dict(C=0), dict(C=9), dict(ld=1), dict(B=0), dict(HW=0), dict(act=3), dict(gamma=None), dict(stats=None),
                dict(workspace=None), dict(workspace_bytes=1024), dict(B=1, HW=1), dict(n=1), dict(training=0, running_mean=None, running_var=None),
                dict(running_var=None)):
        assert so.mvp_bn_act_fwd(ctypes.byref(lib.BnActArgs(**dict(ok, **bad))), None) == -1, bad
    okb = dict(ok, grad_y=16, grad_x=16)
    for bad in (dict(grad_y=None), dict(grad_x=None), dict(C=9), dict(ld=1), dict(stats=None)):
        assert so.mvp_bn_act_bwd(ctypes.byref(lib.BnActArgs(**dict(okb, **bad))), None) == -1, bad
    okc = dict(pred=16, target=16, loss=16, workspace=16, workspace_bytes=lib.BCE_WORKSPACE_BYTES, N=4)
    for bad in (dict(pred=None), dict(target=None), dict(loss=None), dict(workspace=None), dict(workspace_bytes=64), dict(N=0), dict(workspace=12)):
        assert so.mvp_bce_loss_fwd_bwd(ctypes.byref(lib.BceLossArgs(**dict(okc, **bad))), None) == -1, bad
    okd = dict(pred=16, gt=16, counts=16, G=1, n=4, threshold=0.5)
    for bad in (dict(pred=None), dict(gt=None), dict(counts=None), dict(G=0), dict(G=70000), dict(n=0), dict(counts=12)):
        assert so.mvp_binary_counts(ctypes.byref(lib.BinaryCountsArgs(**dict(okd, **bad))), None) == -1, bad
