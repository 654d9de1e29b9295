#!/usr/bin/env python
"""The Tanks-and-Temples evaluation path on one GPU, one JSON line (committed as profiles/tanks_eval_bench.json):

* ``colormap``: ``depth_vis.depth_colormap`` at 1056 x 1920 on a smooth and on a noisy synthetic map -- microseconds per call from
  device events over ``--reps`` queued calls, against two yardsticks: the reference's own code path for the same map (numpy's
  percentile + matplotlib's to_rgba + truncation, one thread, timed on this host in this run; skipped when matplotlib is absent)
  and the floor of the map's traffic at 8 TB/s (three 8.1 MB reads for the selection, one read plus a 6.1 MB write to colour).
* ``writer``: host time per view of the PNG writer job with the device colour map (copy of the finished image + PNG encoding)
  and with the host colouring in front of the same encoder.
* ``driver``: views/s of ``eval_driver --dataset tanks`` (network + writers + fusion) over one synthetic scene of ``--views`` views
  at full size, with the maps handed to the fusion step on the device and with ``--resident-gb 0`` (PFM files read back).
* ``--rocprof DIR``: one child process under ``rocprofv3 --kernel-trace --stats`` running ``--reps`` colour-map calls; the
  kernels' statistics are added and left in DIR.

    python tools/tanks_eval_bench.py [--reps 50] [--views 8] [--rocprof DIR]
"""
import argparse
import io
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

from rc_mvsnet_amd import _lib, depth_vis, synthetic  # noqa: E402

H, W = 1056, 1920
HBM_BYTES_PER_S = 8e12


def maps():
    return {"smooth": synthetic.depth_vis_map(H, W, seed=1, outliers=0.0, noise=0.0), "noisy": synthetic.depth_vis_map(H, W, seed=2)}


def host_colour(depth):
    """the reference's three lines (eval_rcmvsnet_tanks.py:149-152)"""
    import matplotlib as mpl
    from matplotlib import cm
    vmax = np.percentile(depth, 95)
    mapper = cm.ScalarMappable(norm=mpl.colors.Normalize(vmin=depth.min(), vmax=vmax), cmap="magma_r")
    return (mapper.to_rgba(depth)[:, :, :3] * 255).astype(np.uint8)


def best(fn, reps=3):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return min(out)


def encode(rgb):
    from PIL import Image
    Image.fromarray(rgb).save(io.BytesIO(), format="PNG")


def kernel_stats(folder):
    import csv
    rows = []
    for root, _, files in os.walk(folder):
        for f in files:
            if f.endswith("kernel_stats.csv"):
                rows += list(csv.DictReader(open(os.path.join(root, f))))
    return [{"name": r["Name"].split("(")[0], "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
             "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
            for r in rows if "count_kernel" in r["Name"] or "colour_kernel" in r["Name"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--rocprof", default=None)
    ap.add_argument("--colormap-only", action="store_true", help="(the profiled child) --reps colour-map calls per map, no timing")
    ap.add_argument("--no-driver", action="store_true")
    args = ap.parse_args()
    _lib.load()
    dev = torch.device("cuda:0")
    host = maps()
    device = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    for d in device.values():                                                  # warm-up: library load, workspace, table
        for _ in range(5):
            depth_vis.depth_colormap(d)
    torch.cuda.synchronize()
    if args.colormap_only:
        for d in device.values():
            for _ in range(args.reps):
                depth_vis.depth_colormap(d)
        torch.cuda.synchronize()
        return
    try:
        import matplotlib  # noqa: F401
        have_mpl = True
    except ImportError:
        have_mpl = False
    floor_us = 1e6 * (4 * H * W * 4 + H * W * 3) / HBM_BYTES_PER_S
    line = {"bench": "tanks_eval", "gpu": torch.cuda.get_device_name(0), "map": [H, W], "reps": args.reps, "traffic_floor_us": round(floor_us, 2),
            "colormap": {}, "writer": {}}
    for name, d in device.items():
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.reps):
            rgb, _ = depth_vis.depth_colormap(d)
        stop.record()
        torch.cuda.synchronize()
        us = 1e3 * start.elapsed_time(stop) / args.reps
        entry = {"device_us_per_call": round(us, 2), "ratio_to_traffic_floor": round(us / floor_us, 2)}
        rec = {"device_copy_and_encode_ms": round(1e3 * best(lambda: encode(depth_vis.depth_colormap(d)[0].cpu().numpy())), 2),
               "encode_alone_ms": round(1e3 * best(lambda r=rgb.cpu().numpy(): encode(r)), 2)}
        if have_mpl:
            want = host_colour(host[name])
            entry["equal_to_host_path"] = bool(np.array_equal(want, rgb.cpu().numpy()))
            entry["host_percentile_ms"] = round(1e3 * best(lambda: np.percentile(host[name], 95)), 2)
            entry["host_colouring_ms"] = round(1e3 * best(lambda: host_colour(host[name])), 2)
            entry["host_over_device"] = round(1e3 * entry["host_colouring_ms"] / us, 1)
            rec["host_colour_and_encode_ms"] = round(1e3 * best(lambda: encode(host_colour(host[name]))), 2)
        line["colormap"][name], line["writer"][name] = entry, rec
    if not args.no_driver:
        from rc_mvsnet_amd import eval_driver
        with tempfile.TemporaryDirectory() as tmp:
            data = os.path.join(tmp, "tt")
            synthetic.write_tanks_tree(data, scenes=("Family",), V=args.views, hw=(H, W), orig_hw=(1080, 1920), n_src=6)
            common = ["--dataset", "tanks", "--testpath", data, "--scenes", "Family", "--ndepths", "64,32,8"]
            line["driver"] = {"views": args.views, "ndepths": "64,32,8"}
            for key, extra in (("warmup", []), ("resident", []), ("file_readback", ["--resident-gb", "0"]), ("resident_no_png", ["--no-depth-png"])):
                out = os.path.join(tmp, key)
                t0 = time.perf_counter()
                eval_driver.main(common + ["--outdir", out, "--plydir", os.path.join(out, "ply")] + extra)
                torch.cuda.synchronize()
                if key != "warmup":
                    line["driver"][key + "_views_per_s"] = round(args.views / (time.perf_counter() - t0), 2)
    if args.rocprof:
        os.makedirs(args.rocprof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.abspath(args.rocprof), "-o", "tanks_eval",
               "--", sys.executable, os.path.abspath(__file__), "--colormap-only", "--reps", str(args.reps)]
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
        line["kernels"] = kernel_stats(args.rocprof) if p.returncode == 0 else f"rocprofv3 exit {p.returncode}"
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
