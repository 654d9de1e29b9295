"""DTU scorer (rc_mvsnet_amd/dtu_eval.py) on a DTU-sized synthetic scan: ms per phase on the HIP path, one JSON line.

The sizes (3 M data points before the 0.2 mm reduction, 2.5 M stl points, a 600 mm box) are assumed, not measured from DTU
files.  Phases, each timed alone after a warm-up scan (synchronised wall time, median of --reps): grid build over the stl cloud,
the reduction (with its round count), data -> stl and stl -> reduced data (each including its target grid), the mask / plane /
threshold pass with the statistics, and the whole ``evaluate_scan``.  ``--rocprof DIR`` also runs one scan in a child process
under ``rocprofv3 --kernel-trace --stats`` and adds the kernels' totals.  The CPU baseline is the two nearest-neighbour passes
through ``scipy.spatial.cKDTree`` (16 workers) when scipy is importable, otherwise "not measured".

    python tools/dtu_eval_bench.py [--reps 3] [--rocprof DIR] [--no-cpu-baseline]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from rc_mvsnet_amd import _lib, dtu_eval, synthetic        # noqa: E402

N_STL, N_DATA, EXTENT, RES = 2_500_000, 3_000_000, 600.0, 4.0


def timed(fn, reps):
    out, ts = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return out, round(float(np.median(ts)), 2)


def kernel_stats(outdir):
    """rocprofv3's kernel stats CSV -> [{name, calls, total_ms}] (largest first)"""
    files = glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return None
    rows = []
    with open(files[0]) as f:
        for r in csv.DictReader(f):
            rows.append({"name": r["Name"][:80], "calls": int(r["Calls"]), "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3)})
    return sorted(rows, key=lambda r: -r["total_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rocprof", default=None, help="directory: one scan in a child process under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--one-scan", action="store_true", help="(the profiled child) one evaluate_scan, no timing")
    args = ap.parse_args()
    _lib.load()
    dev = "cuda:0"
    s = synthetic.dtu_eval_scan(n_stl=N_STL, n_data=N_DATA, extent=EXTENT, res=RES, seed=0)
    data, stl = torch.from_numpy(s["data"]).to(dev), torch.from_numpy(s["stl"]).to(dev)
    mask = torch.from_numpy(s["obs_mask"])

    def scan():
        return dtu_eval.evaluate_scan(data, stl, mask, s["bb"], s["res"], s["plane"], per_point=True)

    r = scan()                                                   # warm-up (and the profiled child's whole run)
    torch.cuda.synchronize()
    if args.one_scan:
        return
    line = {"workload": "dtu_eval", "n_data": N_DATA, "n_stl": N_STL, "n_reduced": len(r["Qdata"]), "extent_mm": EXTENT}
    grid, line["grid_build_ms"] = timed(lambda: dtu_eval.Grid(stl, h_min=1e-6 * 20.0), args.reps)
    line["grid_cell_mm"], line["grid_dims"] = round(grid.h, 4), grid.dims
    (_, qdata), line["reduce_ms"] = timed(lambda: dtu_eval.reduce_points(data, 0.2, seed=0), args.reps)
    line["reduce_rounds"] = dtu_eval.last_reduce_rounds
    lat = (s["bb"], dtu_eval.LATTICE)
    ddata, line["nn_data_to_stl_ms"] = timed(lambda: dtu_eval.nearest_distances(qdata, stl, cap=20.0, lattice=lat), args.reps)
    dstl, line["nn_stl_to_data_ms"] = timed(lambda: dtu_eval.nearest_distances(stl, qdata, cap=20.0, lattice=lat), args.reps)

    def stats():
        dtu_eval.select_stats(qdata, ddata, "mask", (s["bb"][0], s["res"]), 20.0, obs_mask=mask)
        return dtu_eval.select_stats(stl, dstl, "plane", s["plane"], 20.0)

    _, line["stats_ms"] = timed(stats, args.reps)
    r, line["scan_ms"] = timed(scan, args.reps)
    line.update({k: r[k] for k in dtu_eval.STAT_FIELDS})
    if args.rocprof:
        os.makedirs(args.rocprof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.abspath(args.rocprof), "-o", "dtu_eval",
               "--", sys.executable, os.path.abspath(__file__), "--one-scan"]
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=900)
        line["kernels"] = kernel_stats(args.rocprof) if p.returncode == 0 else f"rocprofv3 exit {p.returncode}"
    if args.no_cpu_baseline:
        line["cpu_baseline"] = "not measured"
    else:
        try:
            from scipy.spatial import cKDTree
        except ImportError:
            line["cpu_baseline"] = "not measured (no scipy)"
        else:
            q, t = qdata.cpu().numpy(), s["stl"]
            t0 = time.perf_counter()
            cKDTree(t).query(q, k=1, distance_upper_bound=20.0, workers=16)
            cKDTree(q).query(t, k=1, distance_upper_bound=20.0, workers=16)
            line["cpu_baseline"] = {"what": "scipy cKDTree, both nearest-neighbour passes incl. tree builds, 16 workers",
                                    "ms": round((time.perf_counter() - t0) * 1e3, 1)}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
