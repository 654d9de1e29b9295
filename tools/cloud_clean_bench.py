"""The point-cloud clean-up (rc_mvsnet_amd/cloud_clean.py, csrc/cloud_knn.hip) on the fused cloud of the synthetic whole scan of
tools/fusion_dynamic_bench.py (5 views of 1184 x 1600, the reference filter; some 3.2 M points): ms per phase, one JSON line, also
written to profiles/cloud_clean_bench.json.

The scan is synthetic and its size is ASSUMED (a DTU-like scan, not measured from one).  Reported per phase, each as the median of
--reps after a warm-up, from the start / stop timestamps of the launches themselves (the *_timed entry points; the grid build has no
such twin and is bracketed by two events on the stream), next to the time its bytes would take at 8 TB/s if every array it must touch
crossed HBM once (n points, k neighbours):
    grid        positions read twice (24 n), keys written and read (8 n), the sorted points and their indices written (20 n)
    knn_mean    the sorted points and their indices read (20 n), the means written (8 n); the candidates are in no floor: the ratio
                to the floor is what the search costs
    knn_full    the same plus idx and d2 written (12 n k)
    radius      the sorted points and indices read (20 n), counts and flags written (5 n)
    normals     idx read (4 n k), positions read once (12 n), normals written (12 n); the gather of k positions is in no floor
    compact     flags read twice (2 n), offsets written and read (8 n), the rows read and the survivors written (19 n + 23 m)
Also the cells read and the candidates tested per query, ``clean_cloud``'s wall time, and the baseline
``scipy.spatial.cKDTree.query(k + 1, workers=16)`` on the same host and cloud.  The tool has no pass threshold: it records.

    python tools/cloud_clean_bench.py [--reps 5] [--no-cpu-baseline] [--out profiles/cloud_clean_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from rc_mvsnet_amd import _lib, cloud_clean as CC, fusion, synthetic        # noqa: E402
from tools.fusion_dynamic_bench import DEPTH, DIST, NCONS, PROB, load        # noqa: E402
from tools.mesh_render_bench import timed        # noqa: E402

HBM_BYTES_PER_S = 8e12
KS = (8, 20, 32)
WHAT = "see the docstring of tools/cloud_clean_bench.py"


def fused_cloud(dev):
    """the reference filter over the whole synthetic scan -> xyz, rgb, view on the device and the camera centres"""
    s = synthetic.fusion_scan(V=5, H=1184, W=1600, seed=0, n_src=4)
    depth_all, jobs = load(s, dev)
    pts, cols, views = [], [], []
    for i, (ref, srcs, conf, img, mats) in enumerate(jobs):
        r = fusion.fuse_view(depth_all, ref, srcs, conf, img, mats, PROB, NCONS, DIST, DEPTH)
        xyz, rgb = fusion.compact_points(r["masks"][2], r["xyz"], r["rgb"])
        pts.append(xyz)
        cols.append(rgb)
        views.append(torch.full((len(xyz),), i, device=dev, dtype=torch.int32))
    centres = np.stack([fusion.camera_centre(s["E"][ref]) for ref, _ in s["pairs"]])
    return torch.cat(pts).contiguous(), torch.cat(cols).contiguous(), torch.cat(views).contiguous(), centres


def entry(ms, floor_bytes):
    floor_ms = floor_bytes / HBM_BYTES_PER_S * 1e3
    return {"ms_median": ms[0], "ms_min": ms[1], "bytes_floor": int(floor_bytes), "floor_ms": round(floor_ms, 5), "times_floor": round(ms[0] / floor_ms, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cloud_clean_bench.json"))
    args = ap.parse_args()
    _lib.load()
    dev = "cuda:0"
    xyz, rgb, view, centres = fused_cloud(dev)
    n = int(xyz.shape[0])
    builds = []
    for _ in range(args.reps + 1):
        grid = CC.Grid(xyz, _timed=True)
        builds.append(grid.build_ms)
    result = {"what": WHAT, "device": torch.cuda.get_device_name(0), "points": n, "size": "assumed (synthetic scan)", "reps": args.reps,
              "hbm_bytes_per_s": HBM_BYTES_PER_S, "grid": dict(grid.describe(), **entry((round(float(np.median(builds[1:])), 4), round(min(builds[1:]), 4)), 52 * n)),
              "knn": {}}
    for k in KS:
        counters = torch.zeros(2, device=dev, dtype=torch.int64)
        CC.knn_device(xyz, k, want=("mean",), counters=counters, grid=grid)
        cells_read, tested = counters.cpu().tolist()
        result["knn"][str(k)] = {
            "mean_only": entry(timed(lambda e0, e1: CC.knn_device(xyz, k, want=("mean",), grid=grid, _timed=("all", e0, e1)), args.reps), 28 * n),
            "idx_d2": entry(timed(lambda e0, e1: CC.knn_device(xyz, k, want=("idx", "d2"), grid=grid, _timed=("all", e0, e1)), args.reps), 20 * n + 12 * n * k),
            "cells_per_query": round(cells_read / n, 2), "candidates_per_query": round(tested / n, 1)}
    mean20 = CC.knn_device(xyz, 20, want=("mean",), grid=grid)["mean"]
    radius = float(torch.nanmean(mean20).item())                  # a radius of the cloud's own scale: the mean 20-neighbour distance
    result["radius"] = dict({"radius": radius, "min_points": 8},
                            **entry(timed(lambda e0, e1: CC._radius(xyz, radius, 8, grid=grid, _timed=("all", e0, e1)), args.reps), 25 * n))
    idx16 = CC.knn_device(xyz, 16, want=("idx",), grid=grid)["idx"]
    result["normals"] = dict({"k": 16}, **entry(timed(lambda e0, e1: CC.normals_from_neighbours(xyz, idx16, view, centres, _timed=("all", e0, e1)), args.reps),
                                                 4 * n * 16 + 24 * n))
    result["normals"]["counters"] = CC.counters_dict(CC.normals_from_neighbours(xyz, idx16, view, centres)[1])
    keep, _ = CC.statistical_from_means(mean20, 2.0)
    m = int(keep.sum().item())
    result["stat"] = dict({"k": 20, "ratio": 2.0, "kept": m}, **entry(timed(lambda e0, e1: CC.statistical_from_means(mean20, 2.0, _timed=("all", e0, e1)), args.reps), 36 * n))
    result["compact"] = entry(timed(lambda e0, e1: CC.compact(keep, xyz, rgb, view, _timed=("all", e0, e1)), args.reps), 29 * n + 23 * m)
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = CC.clean_cloud(xyz, rgb, view, centres, radius=(radius, 8), stat=(20, 2.0), normals=16)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    result["clean_cloud"] = {"wall_ms_median": round(float(np.median(walls)) * 1e3, 2), "options": {"radius": [radius, 8], "stat": [20, 2.0], "normals": 16},
                             "out": r["stats"]["out"], "stat": {k: r["stats"]["stat"][k] for k in ("valid", "mu", "sigma", "threshold")}}
    if not args.no_cpu_baseline:
        from scipy.spatial import cKDTree
        host = xyz.cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        tree = cKDTree(host)
        build_s = time.perf_counter() - t0
        base = {"build_ms": round(build_s * 1e3, 1)}
        for k in KS:
            t0 = time.perf_counter()
            tree.query(host, k + 1, workers=16)
            base[f"query_k{k}_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        result["ckdtree_workers16"] = base
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
