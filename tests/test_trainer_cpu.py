"""CPU checks of the run scaffold the four probe trainers share (mvp/trainer.py): the refusals every entry script makes before it
touches a device, the experiment directory, the optimiser's schedule and the order of an epoch.  No GPU.  FlatAdamW itself needs device
parameters, so the schedule is checked with torch's AdamW standing in for it."""
import importlib.util
import os
import types

import pytest
import torch

from conftest import PKG

SCRIPTS = ["train_depth", "train_snorm", "train_generic_objectness", "train_taskonomy"]


def _entry(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(PKG, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture
def no_device(monkeypatch):
    """A refusal that came after the first device call would surface as this error instead of its own."""
    def boom(*a, **k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(torch.cuda, "current_device", boom)
    monkeypatch.setattr(torch.cuda, "set_device", boom)


@pytest.mark.parametrize("script", SCRIPTS)
def test_entry_script_refuses_a_trainable_backbone_before_any_device_work(script, no_device):
    with pytest.raises(NotImplementedError, match="model_lr"):
        _entry(script).main(["optimizer.model_lr=1e-5"])


@pytest.mark.parametrize("script", SCRIPTS)
def test_entry_script_refuses_an_evaluation_without_a_checkpoint_before_any_device_work(script, no_device):
    with pytest.raises(SystemExit) as e:
        _entry(script).main(["is_eval=True"])
    assert "ckpt_path" in str(e.value.code)


def test_checkpoint_for_eval():
    from mvp import trainer

    assert trainer.checkpoint_for_eval({}) is None and trainer.checkpoint_for_eval({"is_eval": False, "ckpt_path": "x"}) is None
    assert trainer.checkpoint_for_eval({"is_eval": True, "ckpt_path": "a/\\$mae\\$b/ckpt.pth"}) == "a/$mae$b/ckpt.pth"
    for empty in ("", None):
        with pytest.raises(SystemExit, match="ckpt_path"):
            trainer.checkpoint_for_eval({"is_eval": True, "ckpt_path": empty})


def test_experiment_dir_strips_dollars_and_places_family_and_task():
    from mvp import trainer

    cfg = {"output_dir": "out"}
    model, probe = types.SimpleNamespace(checkpoint_name="$mae$vit-mae-base"), types.SimpleNamespace(name="snorm_dpt_k3")
    assert trainer.experiment_dir(cfg, "snorm", model, probe) == os.path.join("out", "snorm_exps", "maevit-mae-base_snorm_dpt_k3")
    assert trainer.experiment_dir(cfg, "objectness", model, probe) == os.path.join("out", "objectness_exps", "maevit-mae-base_snorm_dpt_k3")
    assert trainer.experiment_dir(cfg, "taskonomy", model, probe, "reshading") == os.path.join("out", "taskonomy_exps", "maevit-mae-base_snorm_dpt_k3_reshading")


@pytest.mark.filterwarnings("ignore:Detected call of `lr_scheduler.step")  # no optimiser step is taken: only the schedule is looked at
@pytest.mark.parametrize("world", [1, 2])
def test_build_optimizer_schedule_equals_the_inline_one(monkeypatch, world):
    from evals.utils.optim import cosine_decay_linear_warmup
    from mvp import trainer

    seen = {}

    def adamw(groups, overlap_comm):
        seen["overlap_comm"] = overlap_comm
        return torch.optim.AdamW(groups)

    monkeypatch.setattr(trainer, "FlatAdamW", adamw)
    cfg = {"optimizer": {"probe_lr": 5e-4, "n_epochs": 5, "warmup_epochs": 2}}
    nb, warm = 3, 2
    opt, sched = trainer.build_optimizer(cfg, torch.nn.Linear(2, 1), nb, world)
    assert seen["overlap_comm"] is (world > 1)
    ref_opt = torch.optim.AdamW([{"params": torch.nn.Linear(2, 1).parameters(), "lr": 5e-4}])
    ref = torch.optim.lr_scheduler.LambdaLR(ref_opt, lr_lambda=lambda e: cosine_decay_linear_warmup(e, 5 * nb, warm * nb))
    for s in range(warm * nb + 1):
        if s in (0, 1, warm * nb):
            assert repr(sched.get_last_lr()) == repr(ref.get_last_lr()), s
        sched.step()
        ref.step()
    assert sched.get_last_lr() != [5e-4]  # past the warm-up's peak: the cosine has begun


class _Sampler:
    def __init__(self, events):
        self.events = events

    def set_epoch(self, ep):
        self.events.append(("sampler", ep))


@pytest.mark.parametrize("world,rank", [(1, 0), (2, 0), (2, 1)])
def test_run_epochs_order_printing_and_divisor(monkeypatch, capsys, world, rank):
    from mvp import trainer

    events = []

    class Loader:
        sampler = _Sampler(events)

        def __len__(self):
            return 4  # the divisor is the loader's length, as in the scripts, not the number of steps taken

    def pipelined(model, batches, image_key="image", probe=None):
        events.append(("pipeline", model, image_key, probe))
        for b in batches:
            yield b, ("feats", b)

    def batches(ep):
        events.append(("batches", ep))
        return [1.0 + ep, 2.0 + ep]

    def step(batch, feats):
        assert feats == ("feats", batch)
        return torch.tensor(batch)

    monkeypatch.setattr(trainer, "pipelined_features", pipelined)
    monkeypatch.setattr(trainer, "freeze_gc", lambda: events.append(("freeze_gc",)))
    trainer.run_epochs("M", "P", 2, batches, step, loader=Loader(), image_key="rgb", world=world, rank=rank, on_epoch=lambda ep: events.append(("on_epoch", ep)))
    per_epoch = [[("sampler", ep)] * (world > 1) + [("on_epoch", ep), ("batches", ep), ("pipeline", "M", "rgb", "P")] for ep in range(2)]
    assert events == [("freeze_gc",)] + per_epoch[0] + per_epoch[1]
    out = capsys.readouterr().out
    assert out == ("epoch 0 train loss 0.7500\nepoch 1 train loss 1.2500\n" if rank == 0 else "")


def test_run_epochs_runs_nothing_for_an_evaluation(monkeypatch, capsys):
    from mvp import trainer

    monkeypatch.setattr(trainer, "freeze_gc", lambda: None)
    trainer.run_epochs(None, None, 0, lambda ep: pytest.fail("no epoch"), lambda b, f: pytest.fail("no step"), loader=[1, 2])
    assert capsys.readouterr().out == ""
