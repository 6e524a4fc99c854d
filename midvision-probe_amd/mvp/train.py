"""The hot loop bodies of train_depth.py:93-144, train_snorm.py:86-120 and train_generic_objectness.py:372-398, on the HIP path, and
the loop body of Taskonomy probing, for which the reference ships every part but the loop.

``train_depth_step`` / ``train_snorm_step`` / ``train_objectness_step`` / ``train_taskonomy_step`` are the per-batch bodies (bench.py
times the first);
``train`` mirrors the reference's ``train()`` signature for drop-in use.
"""
from __future__ import annotations

import torch

from . import functional as MF
from . import fused_step
from .pipeline import freeze_gc, pipelined_features


def extract_features(model, images, detach_model=True):
    """train_depth.py:103-112."""
    if detach_model:
        from .pipeline import GroupedFeatures

        def _detached(f):
            return [_f.detach() for _f in f] if isinstance(f, (tuple, list)) else f.detach()

        with torch.no_grad():
            feats = model(images)
            if isinstance(feats, GroupedFeatures):  # several batches stacked into one forward (mvp/pipeline.py): one result per batch
                feats = GroupedFeatures(_detached(f) for f in feats)
            else:
                feats = _detached(feats)
    else:
        # every head Function returns None for the feature gradient and the backbone engines run under no_grad: a
        # trainable backbone (optimizer.model_lr != 0, train_depth.py:566-575) would silently train nothing
        raise NotImplementedError("detach_model=False (backbone fine-tuning, optimizer.model_lr != 0) is outside the frozen-backbone hot path")
    return feats


def _finish_pending(optimizer):
    """FlatAdamW(overlap_comm=True): the previous step's gradient all-reduce has been running under this step's frozen
    forward; its AdamW update must land before the probe reads its weights."""
    fin = getattr(optimizer, "finish_pending", None)
    if fin is not None:
        fin()


def _begin_step(model, optimizer, images, detach_model, feats):
    """Steps 1-3 of every probe step: drop the old gradients, get the frozen features (``feats`` when the caller already has them in
    flight, mvp/pipeline.py; None runs the backbone here), land the previous step's overlapped update.  Returns the features."""
    optimizer.zero_grad()
    if feats is None:
        feats = extract_features(model, images, detach_model)
    _finish_pending(optimizer)
    return feats


def _end_step(probe, optimizer, scheduler, feats, loss_of):
    """Steps 4-8: ``loss_of`` (probe output -> loss), backward, optimiser, schedule; the loss as a DEVICE scalar (the reference's
    per-step ``loss.item()`` host sync is left to the caller)."""
    loss = loss_of(probe(feats))
    MF.backward(loss)
    optimizer.step()
    if scheduler is not None:
        scheduler.step()
    return loss.detach()


def _depth_loss_of(loss_fn, target, scale_invariant):
    """The tape path's ``loss_of``; built outside train_depth_step so that its tape-free branch pays for no closure cells."""
    def loss_of(pred):
        pred = MF.interpolate(pred, size=target.shape[-2:], mode="bilinear")
        if scale_invariant:  # train_depth.py:116-118: per-image scale/shift fit (detached) + clamp, one fused kernel each way
            from evals.utils.metrics import match_scale_and_shift

            pred = match_scale_and_shift(pred, target, clamp=(0.001, 1.0))
        return loss_fn(pred, target)

    return loss_of


def train_depth_step(model, probe, optimizer, scheduler, loss_fn, images, target, detach_model=True, scale_invariant=False, feats=None):
    """One iteration of train_depth.py:99-143."""
    feats = _begin_step(model, optimizer, images, detach_model, feats)
    plan = fused_step.plan_for(probe, optimizer, scheduler, loss_fn, feats, target, scale_invariant)
    if plan is not None:  # the benchmarked probe: the same launches without the autograd tape (mvp/fused_step.py)
        return plan.run(feats, target, scheduler)
    return _end_step(probe, optimizer, scheduler, feats, _depth_loss_of(loss_fn, target, scale_invariant))


def train_snorm_step(model, probe, optimizer, scheduler, images, target, mask, detach_model=True, feats=None):
    """One iteration of train_snorm.py:93-120 (bicubic upsample, angular loss, UA iff 4 channels)."""
    from evals.utils.losses import angular_loss

    def loss_of(pred):
        pred = MF.interpolate(pred.contiguous(), size=target.shape[-2:], mode="bicubic")
        return angular_loss(pred, target, mask, uncertainty_aware=pred.shape[1] > 3)

    return _end_step(probe, optimizer, scheduler, _begin_step(model, optimizer, images, detach_model, feats), loss_of)


def train_objectness_step(model, probe, optimizer, scheduler, images, target, detach_model=True, feats=None):
    """One iteration of train_generic_objectness.py:372-398 (bilinear resize to the mask, nn.BCELoss).  ``target``: the float 0 / 1
    mask [B, C, H, W] with the probe's channel count."""
    return _end_step(probe, optimizer, scheduler, _begin_step(model, optimizer, images, detach_model, feats),
                     lambda pred: MF.bce_loss(MF.interpolate(pred, size=target.shape[-2:], mode="bilinear"), target))


def train_taskonomy_step(model, probe, optimizer, scheduler, images, target, valid, detach_model=True, feats=None):
    """One iteration of Taskonomy probing (the reference ships the parts, not the loop: INTEGRATION.md lists the conventions): the
    probe's first C_t channels, C_t the target's, are resized bilinearly to the target and meet it in MaskedL1Loss under ``valid``
    [B, 1, H, W]; the probe's other channels get a zero gradient."""
    def loss_of(pred):
        ct = target.shape[1]
        if pred.shape[1] < ct:
            raise ValueError(f"the probe has {pred.shape[1]} output channels, the target {ct} (probe.output_dim)")
        pred = MF.interpolate(pred[:, :ct], size=target.shape[-2:], mode="bilinear", align_corners=False)
        return MF.masked_l1_loss(pred, target, valid)

    return _end_step(probe, optimizer, scheduler, _begin_step(model, optimizer, images, detach_model, feats), loss_of)


def _device_batches(loader, dev, keys=("image", "depth", "snorm")):
    """Wrap a host-side loader in the pinned double-buffered H2D prefetcher (mvp/prefetch.py); loaders that already
    yield device tensors (or custom iterables) pass through."""
    from torch.utils.data import DataLoader

    from .prefetch import DevicePrefetcher

    if isinstance(loader, DataLoader):
        return DevicePrefetcher(loader, dev, depth=2, keys=keys)
    return loader


def train(model, probe, train_loader, optimizer, scheduler, n_epochs, detach_model, loss_fn, rank=0, world_size=1,
          valid_loader=None, scale_invariant=False, wandb_use=False, is_final=False, is_navi=False, log_every=0):
    """Reference signature: train_depth.py:76-92.  Batches are dicts {"image", "depth"} (nyu.py:245-251)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    history = []
    freeze_gc()  # no full-heap collector pause inside the loop
    for ep in range(n_epochs):
        if world_size > 1 and hasattr(getattr(train_loader, "sampler", None), "set_epoch"):
            train_loader.sampler.set_epoch(ep)
        train_loss = 0.0
        if not detach_model:
            extract_features(model, None, detach_model)  # raises: backbone fine-tuning is outside the frozen hot path
        # the frozen forward of batch t+1 is already in flight (side stream) while the probe step of batch t runs
        for i, (batch, feats) in enumerate(pipelined_features(model, _device_batches(train_loader, dev), probe=probe)):
            target = batch["depth"].to(dev, non_blocking=True).contiguous()
            loss = train_depth_step(model, probe, optimizer, scheduler, loss_fn, None, target, detach_model, scale_invariant, feats=feats)
            train_loss += loss.item()  # the reference syncs every step too (train_depth.py:143)
        history.append(train_loss / max(len(train_loader), 1))
    # FlatAdamW(overlap_comm=True): the last step's all-reduce + AdamW are still pending — a caller that validates or saves
    # probe.state_dict() next must see the final weights (optimizer.state_dict() is not on that path)
    _finish_pending(optimizer)
    return history


def validate(model, probe, loader, loss_fn, verbose=True, scale_invariant=False, aggregate=True, render_images=False, wandb_use=False,
             is_navi=False, output_dir="result"):
    """Reference: validate(), train_depth.py:357-483 -> (mean loss, global_metrics, level_metrics).  Global metrics include the
    stuff/things groups when ``is_navi`` is False (batches then carry "segmentation", nyu.py:245-251); per-segment rows are
    collected in ``validate.last_segment_metrics`` (the reference only plots them).  PNG dumps / W&B are out of scope."""
    from evals.utils.metrics import evaluate_depth

    dev = torch.device("cuda", torch.cuda.current_device())
    total_loss, count = 0.0, 0
    global_metrics, level_metrics, segments = None, None, []
    with torch.no_grad():
        # eval-mode forwards mutate nothing: the next batches' forwards run on side streams under this batch's probe + metric kernels
        for batch, feats in pipelined_features(model, _device_batches(loader, dev, keys=("image", "depth", "snorm", "segmentation")), probe=probe):
            target = batch["depth"].to(dev).contiguous()
            seg = None if is_navi else batch["segmentation"].to(dev)
            pred = probe(feats)
            pred = MF.interpolate(pred, size=target.shape[-2:], mode="bilinear")
            loss = loss_fn(pred, target)
            total_loss += loss.item()
            gm, lm, sm = evaluate_depth(pred, target, seg, scale_invariant=scale_invariant, nyu_crop=not is_navi, is_navi=is_navi)
            segments.extend(sm)
            if global_metrics is None:
                global_metrics = {k: [v.reshape(-1)] for k, v in gm.items()}
                level_metrics = {L: {k: [v] for k, v in d.items()} for L, d in lm.items()}
            else:
                for k, v in gm.items():
                    global_metrics[k].append(v.reshape(-1))
                for L, d in lm.items():
                    for k, v in d.items():
                        level_metrics[L][k].append(v)
            count += 1
    if global_metrics is None:
        raise ValueError("validate(): empty loader")
    if aggregate:
        global_metrics = {k: torch.cat(v, dim=0).mean() for k, v in global_metrics.items()}
        level_metrics = {L: {k: torch.cat(v, dim=0).mean() for k, v in d.items()} for L, d in level_metrics.items()}
    validate.last_segment_metrics = segments
    return total_loss / max(count, 1), global_metrics, level_metrics
