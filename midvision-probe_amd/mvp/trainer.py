"""What a run of train_depth.py, train_snorm.py, train_generic_objectness.py or train_taskonomy.py does around its step: plain functions,
each taking what differs between the four as an argument, so that a script reads as the list of its choices (INTEGRATION.md has
the table of them and which ones are the reference's)."""
import os

import torch

from . import checkpoint, config
from .optim import FlatAdamW
from .pipeline import freeze_gc, pipelined_features


def check_config(cfg, single_gpu_only=False):
    """The refusals that need no device, in the scripts' order."""
    if single_gpu_only and int(cfg["system"]["num_gpus"]) > 1:
        # train_generic_objectness.py:645-647 spawns ranks that never initialise a process group before wrapping in DDP (:553-555)
        raise NotImplementedError("system.num_gpus > 1: the reference's multi-process objectness path creates no process group and cannot "
                                  "have run; this trainer is single-GPU")
    if float(cfg["optimizer"].get("model_lr", 0.0)) != 0.0:
        raise NotImplementedError("optimizer.model_lr != 0 (backbone fine-tuning) is outside the frozen-backbone hot path")
    return cfg


def compose_and_check(config_name, argv, single_gpu_only=False):
    return check_config(config.compose(config_name, argv), single_gpu_only)


def checkpoint_for_eval(cfg):
    """cfg.ckpt_path of an ``is_eval=True`` run, None for a training run.  Called right after compose: an evaluation without a checkpoint
    would score a randomly initialised probe under the real experiment's CSV columns, and is refused before anything is built."""
    if not cfg.get("is_eval", False):
        return None
    path = str(cfg.get("ckpt_path", "") or "").replace("\\$", "$")
    if not path:
        raise SystemExit("is_eval=True needs ckpt_path=<.../ckpt.pth> (refusing to validate a randomly initialised probe)")
    return path


def load_for_eval(path, model, probe, load_model):
    """``load_model``: train_snorm.py:541-542 loads model AND probe; train_depth.py:526-535,570 the probe only (its model line is
    commented out)."""
    if path is not None:
        checkpoint.load_checkpoint(path, model, probe, load_model=load_model)


def build_model_and_probe(cfg, dev, *, multilayer_default, eval_backbone, **probe_kwargs):
    bcfg = dict(cfg["backbone"])
    if multilayer_default and cfg["probe"].get("head_type", "dpt") != "linear":
        bcfg.setdefault("return_multilayer", True)  # the dpt / multiscale trunks take four maps (the reference needs the override spelt out)
    model = config.instantiate(bcfg)
    if eval_backbone:
        model.eval()  # train_generic_objectness.py:532 — the backbone; the probe is never put in eval mode here
    probe = config.instantiate(cfg["probe"], feat_dim=model.feat_dim, **probe_kwargs)
    return model.to(dev), probe.to(dev)


def resize_pos_embed_for(model, image_size):
    """train_depth.py:613-617, train_generic_objectness.py:547-550.  ``image_size`` is a callable: a sample is decoded for these backbones only."""
    if "sam" in model.checkpoint_name or "vit-mae" in model.checkpoint_name:
        model.resize_pos_embed(image_size=tuple(image_size()))


def build_optimizer(cfg, probe, steps_per_epoch, world):
    from evals.utils.optim import cosine_decay_linear_warmup

    o, nb = cfg["optimizer"], steps_per_epoch
    opt = FlatAdamW([{"params": probe.parameters(), "lr": o["probe_lr"]}], overlap_comm=world > 1)
    return opt, torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda e: cosine_decay_linear_warmup(e, o["n_epochs"] * nb, o["warmup_epochs"] * nb))


def nyu_device_batches(cfg, loader, dev, rank, valid_keys):
    """(device-side training batches or None, wrapper for a validation loader)."""
    ds = cfg["dataset"]
    train_batches, wrap_valid = None, (lambda ld: ld)
    if ds.get("augment_train") or ds.get("raw"):
        # the reference's get_nyu_transforms(augment=True) on the device, between the H2D prefetcher and the frozen forward; raw loaders
        # (uint8 pixels) are normalised there too, on the validation side with nothing else
        from .augment import DeviceAugment
        from .prefetch import DevicePrefetcher

        aug = dict(image_mean=ds.get("image_mean", "imagenet"), seed=int(cfg["system"]["random_seed"]), rank=rank)
        train_batches = DeviceAugment(DevicePrefetcher(loader, dev, keys=("image", "depth", "snorm")), augment=bool(ds.get("augment_train")),
                                      rotateflip=bool(ds.get("rotateflip", False)), **aug)
        if ds.get("raw"):
            wrap_valid = lambda ld: DeviceAugment(DevicePrefetcher(ld, dev, keys=valid_keys), augment=False, **aug)  # noqa: E731
    return train_batches, wrap_valid


def run_epochs(model, probe, n_epochs, batches, step, *, loader, image_key="image", world=1, rank=0, on_epoch=None):
    """``batches(ep)``: the epoch's device batches (a script decides there what lives for one epoch and what for the run);
    ``step(batch, feats)``: the device loss of one training step; ``on_epoch(ep)`` runs after the sampler's ``set_epoch``."""
    freeze_gc()  # no full-heap collector pause inside the loop
    nb = len(loader)
    for ep in range(n_epochs):
        tot = 0.0
        if world > 1:
            loader.sampler.set_epoch(ep)
        if on_epoch is not None:
            on_epoch(ep)
        for batch, feats in pipelined_features(model, batches(ep), image_key=image_key, probe=probe):  # the next forward is already in flight
            tot += step(batch, feats).item()
        if rank == 0:
            print(f"epoch {ep} train loss {tot / nb:.4f}")


def experiment_dir(cfg, family, model, probe, suffix=None):
    name = f"{model.checkpoint_name}_{probe.name}" + (f"_{suffix}" if suffix else "")
    return os.path.join(cfg["output_dir"], f"{family}_exps", name.replace("$", ""))


def finish(world):
    if world > 1:
        torch.distributed.destroy_process_group()
