"""The validation pass (validation.validate over mvs_dataset.DTUValDataset) on a synthetic DTU-layout folder with seeded
weights.  One JSON line:

* ``validate``: items/s of the whole pass at ``--workers`` threads, and the time it waited for the loader per item.
* ``forward_ms``: the train-variant CascadeMVSNet forward alone (eval mode, no_grad, 5 views of 512x640, D = 48/32/8), per item.
* ``metrics_launch_us``: the depth_metrics kernel from its own start / stop timestamps (median, min, max over ``--reps`` launches),
  and the same launch timed from the host over a queued batch (launch overhead included).
* ``aten_metrics``: the same 12 scalars from stock ATen ops on the same GPU tensors, living in this file, with the reference's
  op pattern (utils.py:139-159, models/modules.py:527-546, train_rcmvsnet.py:468-487: boolean-mask indexing per metric, the
  scalars read back one by one) -- ms per item.
* ``--rocprof DIR``: one child process under ``rocprofv3 --kernel-trace --stats`` running ``--reps`` metric launches; the
  kernel's statistics are added and left in DIR.

    python tools/validation_bench.py [--reps 50] [--items 20] [--workers 4] [--rocprof DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from rc_mvsnet_amd import _lib, mvs_dataset, synthetic, train_step as ts, validation  # noqa: E402

STAGES = ("stage1", "stage2", "stage3")


def aten_scalars(outputs, depth_gt_ms, mask_ms, dlossw):
    """The comparator: the same twelve numbers from stock ATen ops, the way the reference's training script gets them -- every
    metric selects the valid pixels again by boolean-mask indexing (a nonzero + gather each), a band is a second boolean
    selection, and all twelve 0-d tensors are read to the host one by one at the end."""
    def valid_error(stage):                                  # |est - gt| over the valid pixels of a stage
        keep = mask_ms[stage][0] > 0.5
        return (outputs[stage]["depth"][0][keep] - depth_gt_ms[stage][0][keep]).abs()

    def rate_above(limit):
        return (valid_error("stage3") > limit).float().mean()

    def band_mean(lo, hi):
        err = valid_error("stage3")
        inside = err[(err >= lo) & (err <= hi)]
        return inside.mean() if inside.numel() else err.new_zeros(())          # an empty band is 0

    loss = torch.zeros((), dtype=torch.float32, device=mask_ms["stage1"].device)
    for weight, stage in zip(dlossw, STAGES):
        keep = mask_ms[stage] > 0.5
        stage_loss = F.smooth_l1_loss(outputs[stage]["depth"][keep], depth_gt_ms[stage][keep], reduction="mean")
        loss += weight * stage_loss
    out = {"loss": loss, "depth_loss": stage_loss, "abs_depth_error": valid_error("stage3").mean()}
    for limit, lo in ((2, 0.0), (4, 2.0), (8, 4.0)):
        out["thres%dmm_error" % limit] = rate_above(limit)
        out["thres%dmm_accu" % limit] = 1 - rate_above(limit)
        out["thres%dmm_abserror" % limit] = band_mean(lo, float(limit))
    return {k: float(v) for k, v in out.items()}


def kernel_stats(folder):
    import csv
    rows = []
    for root, _, files in os.walk(folder):
        for f in files:
            if f.endswith("kernel_stats.csv"):
                rows += list(csv.DictReader(open(os.path.join(root, f))))
    return [{"name": r["Name"].split("(")[0], "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
             "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)} for r in rows if "depth_metrics" in r["Name"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--items", type=int, default=20)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--folder", default=None, help="an existing folder of write_dtu_train_folder (default: a temporary one)")
    ap.add_argument("--rocprof", default=None)
    ap.add_argument("--metrics-only", action="store_true", help="(the profiled child) --reps metric launches on one item, no timing")
    args = ap.parse_args()
    _lib.load()
    dev = torch.device("cuda:0")
    tmp = None
    if args.folder is None:
        tmp = tempfile.TemporaryDirectory()
        args.folder = tmp.name
        synthetic.write_dtu_train_folder(args.folder, ["scan1"], 5, 0)
    lst = os.path.join(args.folder, "train_list.txt")
    ds = mvs_dataset.DTUValDataset(args.folder, lst, "test", 5, device=dev)
    model, _, _ = ts.build(dev, seed=0)
    model.eval()
    w = list(validation.DLOSSW)
    item = ds[0]
    inputs = validation.item_inputs(item)
    table = torch.zeros((args.reps, validation.RECORD), dtype=torch.float64, device=dev)
    with torch.no_grad():
        for _ in range(3):
            outputs, _ = model(*inputs)
        for i in range(args.reps if args.metrics_only else 3):
            validation.depth_metrics(outputs, item["depth_dev"], item["mask_dev"], dlossw=w, table=table, slot=i)
        torch.cuda.synchronize()
        if args.metrics_only:
            return
        t0 = time.perf_counter()
        for _ in range(args.reps):
            model(*inputs)
        torch.cuda.synchronize()
        forward_ms = 1e3 * (time.perf_counter() - t0) / args.reps
        # the kernel's own timestamps
        events = []
        for i in range(args.reps):
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
            ev[1].record()                                                      # a torch event owns its hipEvent_t after a first record
            validation.depth_metrics(outputs, item["depth_dev"], item["mask_dev"], dlossw=w, table=table, slot=i, events=ev)
            events.append(ev)
        torch.cuda.synchronize()
        own = sorted(1e3 * a.elapsed_time(b) for a, b in events)
        t0 = time.perf_counter()
        for i in range(args.reps):
            validation.depth_metrics(outputs, item["depth_dev"], item["mask_dev"], dlossw=w, table=table, slot=i)
        torch.cuda.synchronize()
        queued_us = 1e6 * (time.perf_counter() - t0) / args.reps
        record = validation.record_to_dict(table[0])
        aten = aten_scalars(outputs, item["depth_dev"], item["mask_dev"], w)     # first call: allocator, kernel loads
        t0 = time.perf_counter()
        for _ in range(args.reps):
            aten = aten_scalars(outputs, item["depth_dev"], item["mask_dev"], w)
        torch.cuda.synchronize()
        aten_ms = 1e3 * (time.perf_counter() - t0) / args.reps
    agree = max(abs(record[k] - aten[k]) / max(abs(aten[k]), 1e-3) for k in validation.SCALAR_KEYS)
    idx = [i % len(ds) for i in range(args.items)]
    validation.validate(model, ds, dlossw=w, indices=idx[:4], workers=args.workers)
    stats = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    validation.validate(model, ds, dlossw=w, indices=idx, workers=args.workers, summary_freq=10, stats=stats)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    line = {"what": "validation pass, 5 views of 512x640 per item, synthetic folder, seeded weights", "workers": args.workers, "reps": args.reps,
            "validate": {"items": len(idx), "items_per_s": round(len(idx) / seconds, 2), "ms_per_item": round(1e3 * seconds / len(idx), 2),
                         "loader_wait_ms_per_item": round(1e3 * stats["loader_wait_s"] / len(idx), 3)},
            "forward_ms": round(forward_ms, 3),
            "metrics_launch_us": {"kernel_median": round(own[len(own) // 2], 2), "kernel_min": round(own[0], 2), "kernel_max": round(own[-1], 2),
                                  "host_queued": round(queued_us, 2)},
            "aten_metrics": {"what": "the 12 scalars from stock ATen ops in the reference's op pattern on the same GPU tensors, read back one by one",
                             "ms_per_item": round(aten_ms, 3), "max_rel_difference_from_kernel": float("%.3g" % agree)}}
    if args.rocprof:
        os.makedirs(args.rocprof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.abspath(args.rocprof), "-o", "validation",
               "--", sys.executable, os.path.abspath(__file__), "--metrics-only", "--reps", str(args.reps), "--folder", args.folder]
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
        line["kernels"] = kernel_stats(args.rocprof) if p.returncode == 0 else f"rocprofv3 exit {p.returncode}"
    print(json.dumps(line), flush=True)
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
