"""Tanks and Temples F-score (rc_mvsnet_amd/tanks_fscore.py) on a synthetic scene: ms per phase on the HIP path, one JSON line.

The sizes (2 M ground-truth points, 2 M estimated points, tau = 0.005 on a surface of radius 1) are ASSUMED, not measured from
Tanks and Temples files.  Phases, each timed alone after a warm-up scene (synchronised wall time, median of --reps): the crop,
each voxel down-sample, each ICP round of ``register`` with its iteration count, the two nearest-neighbour passes, the histogram
and the whole scene (register + evaluate).  One kernel comparison: ``rcmvs_pc_icp_step`` next to ``rcmvs_pc_nearest`` on the same
queries, target and grid.  ``--rocprof DIR`` also runs one scene in a child process under ``rocprofv3 --kernel-trace --stats``.
The CPU baseline is the same pipeline in numpy with ``scipy.spatial.cKDTree`` searches (16 workers) on this host.

    python tools/tanks_fscore_bench.py [--reps 3] [--rocprof DIR] [--no-cpu-baseline] [--out profiles/tanks_fscore_bench.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from rc_mvsnet_amd import _lib, dtu_eval, synthetic, tanks_fscore as F        # noqa: E402
from tools.dtu_eval_bench import kernel_stats, timed                           # noqa: E402

N_GT, N_EST, TAU = 2_000_000, 2_000_000, 0.005


def cpu_pipeline(s, vol):
    """register + evaluate in numpy, searches through cKDTree (16 workers) -> (ms, fscore)"""
    from scipy.spatial import cKDTree
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import tanks_fscore_oracle as O
    ovol = (vol["axis"], vol["axis_min"], vol["axis_max"], vol["polygon"])
    tau = s["tau"]

    def icp(src, tgt, thr, T):
        tree, n = cKDTree(tgt), len(src)
        t64 = tgt.astype(np.float64)

        def ev(T):
            q = O.transform(src, T)
            d, i = tree.query(q, k=1, distance_upper_bound=thr, workers=16)
            ok = np.isfinite(d)
            sm, tm = q[ok], t64[i[ok]]
            mom = np.concatenate([[ok.sum(), (d[ok] ** 2).sum()], sm.sum(0), tm.sum(0), (sm.T @ tm).ravel(), [(sm * sm).sum()]])
            return mom, mom[0] / n, (np.sqrt(mom[1] / mom[0]) if mom[0] else 0.0)

        mom, fit, rmse = ev(T)
        for _ in range(20):
            if mom[0] < 3:
                break
            T = O.umeyama_from_moments(mom) @ T
            mom, f2, r2 = ev(T)
            done = abs(f2 - fit) < 1e-6 and abs(r2 - rmse) < 1e-6
            fit, rmse = f2, r2
            if done:
                break
        return T

    t0 = time.perf_counter()
    T = s["init"]
    f, q = O.crop(s["gt"], *ovol)
    gt_c = q[f]
    for voxel, thr in ((tau, 80 * tau), (tau / 2, 20 * tau), (None, 2 * tau)):
        f, q = O.crop(s["est"], *ovol, T=T)
        est_c = q[f]
        a, b = (est_c, gt_c) if voxel is None else (O.voxel_down_sample(est_c, voxel), O.voxel_down_sample(gt_c, voxel))
        T = icp(O.transform(a, np.linalg.inv(T)).astype(np.float32), b, thr, T)
    f, q = O.crop(s["est"], *ovol, T=T)
    e, g = O.voxel_down_sample(q[f], tau / 2), O.voxel_down_sample(gt_c, tau / 2)
    de = cKDTree(g).query(e, k=1, distance_upper_bound=5 * tau, workers=16)[0]
    dg = cKDTree(e).query(g, k=1, distance_upper_bound=5 * tau, workers=16)[0]
    P, R = float((de < tau).mean()), float((dg < tau).mean())
    np.histogram(np.minimum(de, 5 * tau), bins=np.arange(500) * tau / 100)
    np.histogram(np.minimum(dg, 5 * tau), bins=np.arange(500) * tau / 100)
    return round((time.perf_counter() - t0) * 1e3, 1), 2 * P * R / (P + R) if P + R else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rocprof", default=None, help="directory: one scene in a child process under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--one-scene", action="store_true", help="(the profiled child) one register + evaluate, no timing")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    _lib.load()
    dev = "cuda:0"
    s = synthetic.tanks_fscore_scene(n_gt=N_GT, n_est=N_EST, tau=TAU, seed=0)
    v = s["volume"]
    vol = F.make_volume(v["axis"], v["axis_min"], v["axis_max"], v["polygon"])
    est, gt, tau = torch.from_numpy(s["est"]).to(dev), torch.from_numpy(s["gt"]).to(dev), s["tau"]

    def scene():
        T, rounds = F.register(est, gt, s["init"], vol, tau)
        return T, rounds, F.evaluate(est, gt, T, vol, tau)

    T, rounds, r = scene()                                       # warm-up (and the profiled child's whole run)
    torch.cuda.synchronize()
    if args.one_scene:
        return
    line = {"workload": "tanks_fscore", "sizes": "assumed, not taken from Tanks and Temples files", "n_gt": N_GT, "n_est": N_EST, "tau": tau,
            "n_est_scored": r["n_est"], "n_gt_scored": r["n_gt"], "precision": r["precision"], "recall": r["recall"], "fscore": r["fscore"],
            "max_abs_T_error": float(np.abs(T - s["T_true"]).max())}
    (_, est_c), line["crop_est_transformed_ms"] = timed(lambda: F.crop(est, vol, T), args.reps)
    (_, gt_c), line["crop_gt_ms"] = timed(lambda: F.crop(gt, vol), args.reps)
    for name, cloud, voxel in (("est_tau", est_c, tau), ("gt_tau", gt_c, tau), ("est_half_tau", est_c, tau / 2), ("gt_half_tau", gt_c, tau / 2)):
        out, line[f"voxel_{name}_ms"] = timed(lambda: F.voxel_down_sample(cloud, voxel), args.reps)
        line[f"voxel_{name}_points"] = [len(cloud), len(out)]
    Tr = s["init"]
    for i, (voxel, thr) in enumerate(((tau, 80 * tau), (tau / 2, 20 * tau), (None, 2 * tau))):
        _, a = F.crop(est, vol, Tr)
        a, b = (a, gt_c) if voxel is None else (F.voxel_down_sample(a, voxel), F.voxel_down_sample(gt_c, voxel))
        src = F.transform_points(a, np.linalg.inv(Tr))
        res, line[f"icp_round{i + 1}_ms"] = timed(lambda: F.icp(src, b, thr, Tr), args.reps)
        line[f"icp_round{i + 1}_iterations"], line[f"icp_round{i + 1}_points"] = res["iterations"], [len(src), len(b)]
        # the step next to the plain search: same queries (T applied beforehand for the fp32 search), target and grid
        tgt = F.IcpTarget(b, thr)
        q = F.transform_points(src, Tr)
        d = torch.empty(len(q), device=dev, dtype=torch.float64)
        g = tgt.grid

        def plain():
            _lib.call("rcmvs_pc_nearest", F._chk(q, "q"), len(q), ctypes.cast(g._g, ctypes.c_void_p), ctypes.cast(g._d, ctypes.c_void_p),
                      F._chk(g.cell_start, "cell_start", torch.int32), F._chk(g.sorted, "sorted"), tgt.n, float(thr), None,
                      F._chk(d, "d", torch.float64), F._stream())

        _, t_plain = timed(plain, max(args.reps, 5))
        _, t_step = timed(lambda: F.icp_step(src, tgt, Tr, thr), max(args.reps, 5))
        line[f"icp_round{i + 1}_step_vs_nearest"] = {"icp_step_ms": t_step, "pc_nearest_ms": t_plain, "ratio": round(t_step / t_plain, 3),
                                                      "what": "synchronised wall time of one call; the step also copies 18 doubles to the host"}
        Tr = res["transformation"]
    e, g2 = F.voxel_down_sample(est_c, tau / 2), F.voxel_down_sample(gt_c, tau / 2)
    de, line["nn_est_to_gt_ms"] = timed(lambda: dtu_eval.nearest_distances(e, g2, cap=5 * tau), args.reps)
    dg, line["nn_gt_to_est_ms"] = timed(lambda: dtu_eval.nearest_distances(g2, e, cap=5 * tau), args.reps)
    _, line["hist_both_ms"] = timed(lambda: (F.dist_hist(de, tau, 499, tau / 100), F.dist_hist(dg, tau, 499, tau / 100)), args.reps)
    _, line["register_ms"] = timed(lambda: F.register(est, gt, s["init"], vol, tau), args.reps)
    _, line["evaluate_ms"] = timed(lambda: F.evaluate(est, gt, T, vol, tau), args.reps)
    _, line["scene_ms"] = timed(scene, args.reps)
    line["icp_iterations"] = [rd["iterations"] for rd in rounds]
    if args.rocprof:
        os.makedirs(args.rocprof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.abspath(args.rocprof), "-o", "tanks_fscore",
               "--", sys.executable, os.path.abspath(__file__), "--one-scene"]
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=900)
        line["kernels"] = kernel_stats(args.rocprof) if p.returncode == 0 else f"rocprofv3 exit {p.returncode}"
    if args.no_cpu_baseline:
        line["cpu_baseline"] = "not measured"
    else:
        try:
            ms, f = cpu_pipeline(s, vol)
            line["cpu_baseline"] = {"what": "the same pipeline in numpy, searches through scipy cKDTree with 16 workers, same host", "ms": ms,
                                    "fscore": f}
        except ImportError:
            line["cpu_baseline"] = "not measured (no scipy)"
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
