"""Training driver on DTU training folders: the loop of the reference's ``train`` (train_rcmvsnet.py:130-232) on one GPU --
``mvs_dataset.DTUTrainDataset`` through ``prefetch()`` over a shuffled epoch, ``train_step.train_step`` with the loader's
``imgs_aug`` and ``center_imgs``, the reference's ``WarmupMultiStepLR`` schedule (utils.py:216-260) and ``adjust_w_aug``
(train_rcmvsnet.py:379-394), and checkpoints under the reference's names and keys

    <logdir>/model_<epoch:06d>_cas.ckpt  = {"epoch", "model", "optimizer"}
    <logdir>/model_<epoch:06d>_nerf.ckpt = {"model"}

so either side resumes the other's.  Every ``--summary_freq`` steps one JSON line goes to stdout and ``<logdir>/train_log.jsonl``:
the loss parts, the learning rate, the step's wall time and the time the loop waited for the loader.

Not provided here: the validation loop, TensorBoard summaries, the multi-GPU launch.

    python -m rc_mvsnet_amd.train_driver --trainpath /data/dtu_training --trainlist lists/dtu/train.txt --logdir ckpt [--resume]
"""
import argparse
import json
import os
import sys
import time
from bisect import bisect_right

import torch

from . import mvs_dataset, train_step as ts


def adjust_w_aug(epoch_idx, w_aug):
    """train_rcmvsnet.py:379-394: doubled from epochs 2, 4, 6, 8 and 10 (1-based) on"""
    for first in (2, 4, 6, 8, 10):
        if epoch_idx >= first - 1:
            w_aug *= 2
    return w_aug


def parse_lrepochs(text, steps_per_epoch):
    """'10,12,14:2' -> (milestones in steps, gamma) (train_rcmvsnet.py:131-132)"""
    epochs, rate = text.split(":")
    return [steps_per_epoch * int(e) for e in epochs.split(",")], 1 / float(rate)


def warmup_multistep_lr(base_lr, step, milestones, gamma, warmup_factor=1.0 / 3, warmup_iters=500):
    """WarmupMultiStepLR.get_lr (linear warm-up) as a function of the number of scheduler steps taken"""
    factor = 1
    if step < warmup_iters:
        alpha = float(step) / warmup_iters
        factor = warmup_factor * (1 - alpha) + alpha
    return base_lr * factor * gamma ** bisect_right(milestones, step)


def epoch_order(n, epoch, seed):
    """the shuffled item order of an epoch: a function of (seed, epoch), so a resumed run continues the same sequence"""
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed * 1000003 + epoch)).tolist()


def checkpoint_paths(logdir, epoch):
    return ("{}/model_{:0>6}_cas.ckpt".format(logdir, epoch), "{}/model_{:0>6}_nerf.ckpt".format(logdir, epoch))


def save_checkpoint(logdir, epoch, model, model_nerf, opt):
    cas, nerf = checkpoint_paths(logdir, epoch)
    torch.save({"epoch": epoch, "model": model.state_dict(), "optimizer": opt.state_dict()}, cas)
    torch.save({"model": model_nerf.state_dict()}, nerf)
    return cas, nerf


def latest_checkpoint(logdir):
    """the newest (cas, nerf) pair of ``logdir`` (train_rcmvsnet.py:543-551), or None"""
    def newest(suffix):
        names = sorted((fn for fn in os.listdir(logdir) if fn.endswith(suffix)), key=lambda x: int(x.split("_")[1]))
        return os.path.join(logdir, names[-1]) if names else None
    cas, nerf = newest("cas.ckpt"), newest("nerf.ckpt")
    return (cas, nerf) if cas and nerf else None


def load_checkpoint(cas, nerf, model, model_nerf, opt=None):
    """-> the epoch to start at.  ``opt`` None: weights only (--loadckpt)."""
    sd = torch.load(cas, map_location="cpu")
    model.load_state_dict(sd["model"], strict=True)
    if nerf is not None:
        model_nerf.load_state_dict(torch.load(nerf, map_location="cpu")["model"], strict=True)
    if opt is None:
        return 0
    opt.load_state_dict(sd["optimizer"])
    return sd["epoch"] + 1


def step_inputs(dataset, item):
    """an item of DTUTrainDataset -> the arguments of train_step (batch dimension added, on the item's device)"""
    dev = item["imgs"].device
    proj = {k: torch.from_numpy(v)[None].to(dev) for k, v in item["proj_matrices"].items()}
    dv = torch.from_numpy(item["depth_values"])[None].to(dev)
    return dict(imgs=item["imgs"][None], proj=proj, depth_values=dv, batch=dataset.render_batch(item), imgs_aug=item["imgs_aug"][None],
                loss_imgs=item["center_imgs"][None])


def train(args, dataset, model, model_nerf, opt, start_epoch, step_fn=None, out=sys.stdout):
    """The epoch loop.  step_fn(model, model_nerf, opt, w_aug=..., **step_inputs) -> dict of floats (default train_step).
    Returns the log records."""
    step_fn = step_fn or ts.train_step
    n = len(dataset) if args.max_steps_per_epoch is None else min(len(dataset), args.max_steps_per_epoch)
    milestones, gamma = parse_lrepochs(args.lrepochs, n)
    records = []
    log = open(os.path.join(args.logdir, "train_log.jsonl"), "a")
    cuda = dataset.device.type == "cuda"
    for epoch in range(start_epoch, args.epochs):
        dataset.set_epoch(epoch)
        order = epoch_order(len(dataset), epoch, args.seed)[:n]
        w_aug = adjust_w_aug(epoch, args.w_aug)
        items = mvs_dataset.prefetch(dataset, indices=order, workers=args.workers, depth=2 * args.workers)
        t_prev = time.perf_counter()
        for batch_idx in range(n):
            global_step = n * epoch + batch_idx
            lr = warmup_multistep_lr(args.lr, global_step, milestones, gamma)
            for group in opt.param_groups:
                group["lr"] = lr
            item = next(items)
            t_got = time.perf_counter()
            losses = step_fn(model, model_nerf, opt, w_aug=w_aug, **step_inputs(dataset, item))
            if cuda:
                torch.cuda.synchronize(dataset.device)
            t_done = time.perf_counter()
            if global_step % args.summary_freq == 0:
                rec = dict(epoch=epoch, step=global_step, lr=lr, w_aug=w_aug, scan=item["scan"], step_ms=1e3 * (t_done - t_got),
                           loader_wait_ms=1e3 * (t_got - t_prev), **losses)
                records.append(rec)
                line = json.dumps(rec)
                print(line, file=out, flush=True)
                log.write(line + "\n")
                log.flush()
            t_prev = t_done
        if (epoch + 1) % args.save_freq == 0:
            save_checkpoint(args.logdir, epoch, model, model_nerf, opt)
    log.close()
    return records


def parser():
    p = argparse.ArgumentParser(description="RC-MVSNet training on a DTU training folder, one GPU")
    p.add_argument("--trainpath", required=True)
    p.add_argument("--trainlist", required=True)
    p.add_argument("--logdir", required=True)
    p.add_argument("--epochs", type=int, default=15)
    p.add_argument("--lr", type=float, default=0.0001)
    p.add_argument("--lrepochs", type=str, default="10,12,14:2")
    p.add_argument("--w_aug", type=float, default=0.01)
    p.add_argument("--num_view", type=int, default=4)
    p.add_argument("--ndepths", type=str, default="48,32,8")
    p.add_argument("--numdepth", type=int, default=192)
    p.add_argument("--interval_scale", type=float, default=1.06)
    p.add_argument("--loadckpt", default=None, help="a *_cas.ckpt to start from (the *_nerf.ckpt next to it is loaded too when present)")
    p.add_argument("--resume", action="store_true")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--workers", type=int, default=4, help="threads decoding items ahead of the GPU")
    p.add_argument("--summary_freq", type=int, default=10)
    p.add_argument("--save_freq", type=int, default=1)
    p.add_argument("--random_view", action="store_true")
    p.add_argument("--max_steps_per_epoch", type=int, default=None, help="cut every epoch short (trial runs)")
    p.add_argument("--device", default="cuda:0")
    return p


def main(argv=None):
    args = parser().parse_args(argv)
    os.makedirs(args.logdir, exist_ok=True)
    device = torch.device(args.device)
    torch.manual_seed(args.seed)
    dataset = mvs_dataset.DTUTrainDataset(args.trainpath, args.trainlist, "train", args.num_view, args.numdepth, args.interval_scale,
                                          random_view=args.random_view, device=device, seed=args.seed)
    model, model_nerf, opt = ts.build(device, ndepths=[int(x) for x in args.ndepths.split(",")], seed=args.seed)
    for group in opt.param_groups:
        group["lr"] = args.lr
    start_epoch = 0
    if args.resume and latest_checkpoint(args.logdir):
        start_epoch = load_checkpoint(*latest_checkpoint(args.logdir), model, model_nerf, opt)
    elif args.loadckpt:
        nerf = args.loadckpt.replace("_cas.ckpt", "_nerf.ckpt")
        load_checkpoint(args.loadckpt, nerf if nerf != args.loadckpt and os.path.exists(nerf) else None, model, model_nerf)
    return train(args, dataset, model, model_nerf, opt, start_epoch)


if __name__ == "__main__":
    main()
