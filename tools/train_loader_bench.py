"""Throughput of the training loader (mvs_dataset.DTUTrainDataset) on a synthetic DTU-layout folder, next to the training
iteration it has to keep ahead of.  One JSON line:

* ``loader``: items/s through ``prefetch()`` at ``--workers`` threads; the host half alone (one thread, ms per item: PNG and
  PFM decoding, camera parsing) and the device half alone (ms per item: uploads, tone tables, the two launches, synchronised).
* ``cpu_reference_style``: a single-thread Pillow + numpy + torch restatement, living in this file, of what the reference's
  loader does per item with its ``num_workers=1`` -- every PNG decoded three times, ColorJitter through Pillow, ToTensor /
  pow / clamp / Normalize, center_image in fp32, the depth and mask pyramids.
* ``train_step_ms``: ``train_step`` on a loader item in the same process (full size, D = 48/32/8), and the loader wait per
  step measured inside ``train_driver``'s loop.
* ``--rocprof DIR``: one child process under ``rocprofv3 --kernel-trace --stats`` preparing ``--reps`` items; the kernels'
  statistics are added and left in DIR.

    python tools/train_loader_bench.py [--reps 20] [--workers 4] [--rocprof DIR]
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

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from rc_mvsnet_amd import _lib, mvs_dataset, synthetic, train_driver, train_step as ts  # noqa: E402


def reference_style_item(ds, idx, rng):
    """the reference's per-item image and map work, one thread (datasets/dtu_train.py:238-330 restated with Pillow / numpy / torch)"""
    from PIL import Image, ImageEnhance
    from rc_mvsnet_amd.data_io import read_pfm
    scan, light, ref, srcs = ds.metas[idx]
    mean = torch.tensor(mvs_dataset.MEAN).view(3, 1, 1)
    std = torch.tensor(mvs_dataset.STD).view(3, 1, 1)
    out = []
    for i, vid in enumerate([ref] + srcs[:ds.nviews - 1]):
        name = os.path.join(ds.datapath, "Rectified/{}_train/rect_{:0>3}_{}_r5000.png".format(scan, vid + 1, light))
        img = Image.open(name)                                                  # read_img_aug
        for op in rng.permutation(4):
            if op == 0:
                img = ImageEnhance.Brightness(img).enhance(rng.uniform(0, 2))
            elif op == 1:
                img = ImageEnhance.Contrast(img).enhance(rng.uniform(0, 2))
            elif op == 2:
                img = ImageEnhance.Color(img).enhance(rng.uniform(0.5, 1.5))
            else:
                h, s, v = img.convert("HSV").split()
                nh = (np.array(h, dtype=np.uint8).astype(np.int32) + int(rng.uniform(-0.5, 0.5) * 255) % 256).astype(np.uint8)
                img = Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB")
        t = torch.from_numpy(np.array(img, dtype=np.uint8)).permute(2, 0, 1).contiguous().float().div(255)
        t = torch.pow(t, rng.uniform(0.5, 2.0)).clamp_(0.0, 1.0)
        aug = (t - mean) / std
        seg = (torch.from_numpy(np.array(Image.open(name), dtype=np.uint8)).permute(2, 0, 1).contiguous().float().div(255) - mean) / std
        x = np.array(Image.open(name).convert("RGB"), dtype=np.uint8).astype(np.float32)                # cv2.imread + center_image
        cen = (x - np.mean(x, axis=(0, 1), keepdims=True)) / (np.sqrt(np.var(x, axis=(0, 1), keepdims=True)) + 1e-8)
        depth = read_pfm(os.path.join(ds.datapath, "Depths_raw/{}/depth_map_{:0>4}.pfm".format(scan, vid)))[0]
        dh = np.ascontiguousarray(depth[::2, ::2][44:556, 80:720])
        if i == 0:
            m = (np.array(Image.open(os.path.join(ds.datapath, "Depths_raw/{}/depth_visual_{:0>4}.png".format(scan, vid))), dtype=np.float32) > 10)
            m = np.ascontiguousarray(m.astype(np.float32)[::2, ::2][44:556, 80:720])
            d2 = np.ascontiguousarray(read_pfm(os.path.join(ds.datapath, "Depths_raw/{}/depth_map_{:0>4}.pfm".format(scan, vid)))[0][::2, ::2][44:556, 80:720])
            out.append((m[::4, ::4].copy(), m[::2, ::2].copy(), d2[::4, ::4].copy(), d2[::2, ::2].copy()))
        out.append((aug, seg, cen, dh))
    return out


def kernel_stats(folder):
    import csv
    rows = []
    for root, _, files in os.walk(folder):
        for f in files:
            if f.endswith("kernel_stats.csv"):
                rows += list(csv.DictReader(open(os.path.join(root, f))))
    return [{"name": r["Name"].split("(")[0], "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
             "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)} for r in rows if "train_" in r["Name"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--folder", default=None, help="an existing folder of write_dtu_train_folder (default: a temporary one)")
    ap.add_argument("--rocprof", default=None)
    ap.add_argument("--prepare-only", action="store_true", help="(the profiled child) prepare --reps items, no timing")
    ap.add_argument("--no-train-step", action="store_true")
    args = ap.parse_args()
    _lib.load()
    dev = torch.device("cuda:0")
    tmp = None
    if args.folder is None:
        tmp = tempfile.TemporaryDirectory()
        args.folder = tmp.name
        synthetic.write_dtu_train_folder(args.folder, ["scan1"], 5, 0)
    lst = os.path.join(args.folder, "train_list.txt")
    ds = mvs_dataset.DTUTrainDataset(args.folder, lst, "train", 4, device=dev)
    idx = [i % len(ds) for i in range(args.reps)]
    if args.prepare_only:
        for i in idx:
            ds[i]
        torch.cuda.synchronize()
        return
    ds[0]
    torch.cuda.synchronize()                                                     # library load, first launches
    t0 = time.perf_counter()
    hosts = [ds.load_host(i) for i in idx]
    host_ms = 1e3 * (time.perf_counter() - t0) / len(idx)
    t0 = time.perf_counter()
    for h in hosts:
        ds.to_device(h)
    torch.cuda.synchronize()
    device_ms = 1e3 * (time.perf_counter() - t0) / len(idx)
    del hosts
    t0 = time.perf_counter()
    for _ in mvs_dataset.prefetch(ds, indices=idx, workers=args.workers, depth=2 * args.workers):
        pass
    torch.cuda.synchronize()
    items_per_s = len(idx) / (time.perf_counter() - t0)
    rng = np.random.default_rng(0)
    n_cpu = max(2, min(5, args.reps))
    t0 = time.perf_counter()
    for i in idx[:n_cpu]:
        reference_style_item(ds, i, rng)
    cpu_ms = 1e3 * (time.perf_counter() - t0) / n_cpu
    line = {"what": "DTU training loader, 4 views of 512x640 per item, synthetic folder", "workers": args.workers, "reps": args.reps,
            "loader": {"items_per_s_prefetch": round(items_per_s, 1), "host_half_ms_one_thread": round(host_ms, 2),
                       "device_half_ms": round(device_ms, 3)},
            "cpu_reference_style": {"what": "single-thread Pillow + numpy + torch restatement of the reference's per-item work",
                                    "ms_per_item": round(cpu_ms, 1), "items_per_s": round(1e3 / cpu_ms, 2)}}
    if not args.no_train_step:
        import warnings
        warnings.simplefilter("ignore")
        model, model_nerf, opt = ts.build(dev)
        inp = train_driver.step_inputs(ds, ds[0])
        for _ in range(3):
            ts.train_step(model, model_nerf, opt, **inp)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            ts.train_step(model, model_nerf, opt, **inp)
        torch.cuda.synchronize()
        line["train_step_ms"] = round(1e3 * (time.perf_counter() - t0) / 10, 2)
        logdir = tempfile.mkdtemp()
        a = train_driver.parser().parse_args(["--trainpath", args.folder, "--trainlist", lst, "--logdir", logdir, "--epochs", "1",
                                              "--max_steps_per_epoch", str(max(args.reps, 12)), "--summary_freq", "1", "--workers", str(args.workers),
                                              "--save_freq", "1000"])
        rec = train_driver.train(a, ds, model, model_nerf, opt, 0, out=open(os.devnull, "w"))[2:]
        line["driver"] = {"steps": len(rec), "step_ms_mean": round(float(np.mean([r["step_ms"] for r in rec])), 2),
                          "loader_wait_ms_mean": round(float(np.mean([r["loader_wait_ms"] for r in rec])), 3),
                          "loader_wait_ms_max": round(float(np.max([r["loader_wait_ms"] for r in rec])), 3)}
        line["loader_keeps_ahead"] = bool(1e3 / items_per_s < line["driver"]["step_ms_mean"])
    if args.rocprof:
        os.makedirs(args.rocprof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.abspath(args.rocprof), "-o", "train_loader",
               "--", sys.executable, os.path.abspath(__file__), "--prepare-only", "--reps", str(args.reps), "--folder", args.folder]
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
        line["kernels"] = kernel_stats(args.rocprof) if p.returncode == 0 else f"rocprofv3 exit {p.returncode}"
    print(json.dumps(line), flush=True)
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
