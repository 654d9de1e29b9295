"""Training driver on DTU training folders: the loop of the reference's ``train`` (train_rcmvsnet.py:130-232) on one GPU --
``mvs_dataset.DTUTrainDataset`` through ``prefetch()`` over a shuffled epoch, ``train_step.train_step`` with the loader's
``imgs_aug`` and ``center_imgs``, the reference's ``WarmupMultiStepLR`` schedule (utils.py:216-260) and ``adjust_w_aug``
(train_rcmvsnet.py:379-394), and checkpoints under the reference's names and keys

    <logdir>/model_<epoch:06d>_cas.ckpt  = {"epoch", "model", "optimizer"}
    <logdir>/model_<epoch:06d>_nerf.ckpt = {"model"}

so either side resumes the other's.  Every ``--summary_freq`` steps one JSON line goes to stdout and ``<logdir>/train_log.jsonl``:
the loss parts, the learning rate, the step's wall time and the time the loop waited for the loader.

With ``--testlist`` the validation pass of the reference runs too (``validation.validate`` over ``mvs_dataset.DTUValDataset``,
train_rcmvsnet.py:229-258): after the checkpoint of every epoch with ``epoch % eval_freq == 0`` and of the last one.  It logs one
``{"phase": "test", ...}`` line per ``--summary_freq`` items and one ``{"phase": "fulltest", "epoch": ..., <the 12 means>}`` line.
``--mode test`` (the reference's ``test()``, :262-275) loads ``--loadckpt`` or the newest checkpoint of ``--logdir`` (``--resume``)
into the cascade alone -- no training folder, renderer or optimizer is built -- runs that pass once and exits.  Without ``--testlist`` nothing of this happens.

Not provided here: TensorBoard summaries, the multi-GPU launch (validation included: the set is not sharded).

    python -m rc_mvsnet_amd.train_driver --trainpath /data/dtu_training --trainlist lists/dtu/train.txt --logdir ckpt [--resume] \
        [--testlist lists/dtu/val.txt] [--eval_freq 1]
    python -m rc_mvsnet_amd.train_driver --mode test --testpath /data/dtu_training --testlist lists/dtu/test.txt \
        --logdir ckpt --loadckpt ckpt/model_000014_cas.ckpt
"""
import argparse
import json
import os
import sys
import time
from bisect import bisect_right

import torch

from . import mvs_dataset, train_step as ts, validation


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


def run_validation(args, val_dataset, model, epoch, log, out=sys.stdout, validate_fn=None):
    """One validation pass, logged: a {"phase": "test"} line per summary_freq items, then the {"phase": "fulltest"} line with the
    means over the items (DictAverageMeter.mean).  -> the fulltest record."""
    validate_fn = validate_fn or validation.validate
    n = len(val_dataset) if args.max_val_items is None else min(len(val_dataset), args.max_val_items)

    def emit(rec):
        line = json.dumps(rec)
        print(line, file=out, flush=True)
        log.write(line + "\n")
        log.flush()

    def on_summary(i, record):
        emit(dict(phase="test", epoch=epoch, item=i, **{k: record[k] for k in validation.SCALAR_KEYS}))

    t0 = time.perf_counter()
    _, mean = validate_fn(model, val_dataset, dlossw=[float(e) for e in args.dlossw.split(",") if e], indices=range(n), workers=args.workers,
                          summary_freq=args.summary_freq, on_summary=on_summary, image_dir=args.val_images)
    full = dict(phase="fulltest", epoch=epoch, items=n, seconds=time.perf_counter() - t0, **mean)
    emit(full)
    return full


def train(args, dataset, model, model_nerf, opt, start_epoch, step_fn=None, out=sys.stdout, val_dataset=None, validate_fn=None):
    """The epoch loop.  step_fn(model, model_nerf, opt, w_aug=..., **step_inputs) -> dict of floats (default train_step).
    val_dataset (a DTUValDataset; None = no validation): validated after the checkpoint when epoch % eval_freq == 0 or on the
    last epoch (train_rcmvsnet.py:230).  Returns the log records of the training steps."""
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
        if val_dataset is not None and (epoch % args.eval_freq == 0 or epoch == args.epochs - 1):
            run_validation(args, val_dataset, model, epoch, log, out=out, validate_fn=validate_fn)
    log.close()
    return records


def parser():
    p = argparse.ArgumentParser(description="RC-MVSNet training on a DTU training folder, one GPU")
    p.add_argument("--trainpath", default=None, help="the training folder (needed in --mode train)")
    p.add_argument("--trainlist", default=None, help="scan list to train on (needed in --mode train)")
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
    p.add_argument("--mode", default="train", choices=["train", "test"])
    p.add_argument("--testpath", default=None, help="the validation folder (default: --trainpath)")
    p.add_argument("--testlist", default=None, help="scan list to validate on; without it no validation runs")
    p.add_argument("--eval_freq", type=int, default=1)
    p.add_argument("--dlossw", type=str, default="0.5,1.0,2.0", help="stage weights of the validation loss")
    p.add_argument("--val_num_view", type=int, default=5, help="views of a validation item (train_rcmvsnet.py:518-519)")
    p.add_argument("--max_val_items", type=int, default=None, help="cut every validation pass short (trial runs)")
    p.add_argument("--val-images", dest="val_images", default=None, help="write depth_est / errormap of every summary_freq-th item there (PFM)")
    return p


def check_mode(args, have_checkpoint):
    """--mode train needs a folder and a list to train on; --mode test a folder, a list to validate on and weights to validate"""
    if args.mode != "test":
        if not (args.trainpath and args.trainlist):
            raise SystemExit("--mode train needs --trainpath and --trainlist")
        return
    if not args.testlist:
        raise SystemExit("--mode test needs --testlist")
    if not (args.testpath or args.trainpath):
        raise SystemExit("--mode test needs --testpath (or --trainpath)")
    if not (args.loadckpt or (args.resume and have_checkpoint)):
        raise SystemExit("--mode test needs --loadckpt, or --resume with a checkpoint in --logdir")


def validation_dataset(args, device):
    return mvs_dataset.DTUValDataset(args.testpath or args.trainpath, args.testlist, "test", args.val_num_view, args.numdepth,
                                     args.interval_scale, device=device)


def run_test_mode(args, device):
    """--mode test (the reference's test(), train_rcmvsnet.py:262-275): the cascade alone -- no training set, no renderer, no
    optimizer -- with the weights of --loadckpt or of the newest checkpoint of --logdir; one validation pass.
    -> [the fulltest record]"""
    from .casmvsnet import CascadeMVSNet
    model = CascadeMVSNet(ndepths=[int(x) for x in args.ndepths.split(",")], depth_interals_ratio=[4, 2, 1]).to(device)
    cas = latest_checkpoint(args.logdir)[0] if args.resume and latest_checkpoint(args.logdir) else args.loadckpt
    sd = torch.load(cas, map_location="cpu")
    model.load_state_dict(sd["model"], strict=True)
    with open(os.path.join(args.logdir, "train_log.jsonl"), "a") as log:
        return [run_validation(args, validation_dataset(args, device), model, int(sd.get("epoch", 0)), log)]


def main(argv=None):
    args = parser().parse_args(argv)
    os.makedirs(args.logdir, exist_ok=True)
    check_mode(args, bool(latest_checkpoint(args.logdir)))
    device = torch.device(args.device)
    torch.manual_seed(args.seed)
    if args.mode == "test":
        return run_test_mode(args, device)
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
    return train(args, dataset, model, model_nerf, opt, start_epoch, val_dataset=validation_dataset(args, device) if args.testlist else None)


if __name__ == "__main__":
    main()
