#!/usr/bin/env python3
"""Entry point mirroring the reference's train_depth.py (hydra.main -> train_model, train_depth.py:542-855)
for the hot path on MI355X: compose config -> instantiate backbone & probe -> FlatAdamW + LambdaLR ->
train() -> validate() -> ckpt.pth.  Data: evals.datasets.build_loader (reference sampler semantics) over the
synthetic NYU-shaped dataset, fed through the pinned double-buffered H2D prefetcher (the reference's dataset
decoders, W&B, CSV bookkeeping are out of scope).

    python train_depth.py backbone=dino_b16 +backbone.return_multilayer=True probe=depth_linear batch_size=16
    torchrun --nproc-per-node N --master-addr 127.0.0.1 train_depth.py ...      # one rank per GPU
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from mvp import checkpoint, config, trainer  # noqa: E402
from mvp import dist as mdist  # noqa: E402
from mvp.train import train, validate  # noqa: E402


def self_launch(world: int, argv) -> int:
    """cfg.system.num_gpus > 1 without a torchrun environment: start one fresh rank per GPU BEFORE this process touches
    the GPU (the reference does mp.spawn(train_model, nprocs=world_size), train_depth.py:851-855)."""
    import socket
    import subprocess

    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    return subprocess.call(cmd, env=env)


def main(argv):
    from evals.datasets import build_loader
    from evals.utils.losses import DepthLoss
    from mvp import results

    cfg = config.compose("depth_training", argv)
    if int(cfg["system"]["num_gpus"]) > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(int(cfg["system"]["num_gpus"]), argv))
    trainer.check_config(cfg)
    loaded_ckpt = trainer.checkpoint_for_eval(cfg)  # train_depth.py:526-535,570: an evaluation run scores the probe of cfg.ckpt_path
    is_eval = loaded_ckpt is not None
    rank, local, world = mdist.env_setup("nccl")
    cfg["system"]["num_gpus"] = world
    torch.manual_seed(int(cfg["system"]["random_seed"]))  # probe initialisation; rank 0's copy is broadcast by FlatAdamW
    dev = torch.device("cuda", torch.cuda.current_device())
    ds = cfg["dataset"]
    loader = build_loader(dict(ds, batch_size=cfg["batch_size"]), "train", cfg["batch_size"], num_gpus=world, num_workers=cfg.get("num_workers", 2),
                          with_snorm=False)
    augmented, wrap_valid = trainer.nyu_device_batches(cfg, loader, dev, rank, valid_keys=("image", "depth", "snorm", "segmentation"))
    model, probe = trainer.build_model_and_probe(cfg, dev, multilayer_default=False, eval_backbone=False, max_depth=ds["max_depth"])
    trainer.resize_pos_embed_for(model, lambda: ds["image_size"] if ds.get("raw") else loader.dataset[0]["image"].shape[-2:])
    opt, sched = trainer.build_optimizer(cfg, probe, len(loader), world)
    trainer.load_for_eval(loaded_ckpt, model, probe, load_model=False)
    hist = [] if is_eval else train(model, probe, loader if augmented is None else augmented, opt, sched, cfg["optimizer"]["n_epochs"],
                                    detach_model=True, loss_fn=DepthLoss(), rank=rank, world_size=world)
    opt.finish_pending()
    if rank == 0:
        model.eval(); probe.eval()
        is_navi = ds["name"] in ("navi_reldepth", "navi")
        vcfg = dict(ds, num_batches=2, batch_size=cfg["batch_size"])
        timestamp, exp_name, exp_info = results.experiment_info(cfg, model, probe, ds["name"], ds["name"])
        out = os.path.join(cfg["output_dir"], "depth_exps", exp_name.replace("$", ""))
        ckpt = loaded_ckpt if is_eval else os.path.join(out, "ckpt.pth")  # the CSV's ckpt_path column names what was scored
        sa_loss, sa_g, sa_l = validate(model, probe, wrap_valid(build_loader(vcfg, "valid", cfg["batch_size"], with_snorm=False)), DepthLoss(), is_navi=is_navi)
        si_loss, si_g, si_l = validate(model, probe, wrap_valid(build_loader(vcfg, "valid", cfg["batch_size"], with_snorm=False)), DepthLoss(),
                                       scale_invariant=True, is_navi=is_navi)
        print(f"train loss/epoch {hist} | SA valid loss {sa_loss:.4f} d1 {sa_g['d1']:.4f} rmse {sa_g['rmse']:.4f} | SI loss {si_loss:.4f} rmse {si_g['rmse']:.4f}")
        titles, row = results.depth_result_row(timestamp, exp_info, sa_g, si_g, sa_l, si_l, ckpt, ds["name"])
        print("results ->", results.append_result_csv(results.result_csv_path(cfg["output_dir"], "depth", ds["name"], bool(cfg["backbone"].get("add_norm"))), titles, row))
        if not is_eval:
            print("saved", checkpoint.save_checkpoint(ckpt, cfg, model, probe))
    trainer.finish(world)


if __name__ == "__main__":
    main(sys.argv[1:])
