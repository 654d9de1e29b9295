"""COLMAP import (rc_mvsnet_amd/colmap_import.py) on a synthetic sparse model: ms per phase on the HIP path, one JSON line.

The sizes (300 images, 1 M points, a mean track length of about 6) are ASSUMED, not measured from a COLMAP reconstruction.  The
three phases (pair scores, top views, depth ranks) are timed with device events around each call, median of --reps after a
warm-up.  The yardstick is the numpy oracle (tests/colmap_oracle.py) on the same model and the same host, timed once; the results
of both are compared.  ``--rocprof DIR`` also runs the three phases once in a child process under ``rocprofv3 --kernel-trace --stats``.

    python tools/colmap_import_bench.py [--reps 5] [--rocprof DIR] [--no-cpu-baseline] [--out profiles/colmap_import_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from rc_mvsnet_amd import _lib, colmap_import as CI, synthetic        # noqa: E402

N_IMAGES, N_POINTS, TRACK, NUM_SRC = 300, 1_000_000, 6.0, 10


def event_ms(fn, reps):
    """-> (result, median ms between two device events around fn)"""
    out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return out, round(float(np.median(times)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rocprof", default=None, help="directory: the three phases once in a child process under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--one-pass", action="store_true", help="(the profiled child) the three phases once, no timing")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    _lib.load()
    dev = "cuda:0"
    # every camera of the ring sees the whole box, so the frustum alone would give tracks of 300: observations are kept with the
    # probability that leaves about TRACK of them per point
    probe = synthetic.colmap_arrays(N_IMAGES, 20_000, hw=(1080, 1920), seed=0, arc_deg=300.0, keep=1.0)
    frac = len(probe["ids"]) / (N_IMAGES * 20_000)
    A = synthetic.colmap_arrays(N_IMAGES, N_POINTS, hw=(1080, 1920), seed=0, arc_deg=300.0, keep=TRACK / (N_IMAGES * frac))
    counts = np.diff(A["offsets"])
    ranks = np.array([CI.rank_pair(int(c)) for c in counts], dtype=np.int32)
    zrows = np.ascontiguousarray(A["extrinsics"][:, 2, :])
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         (("centres", A["centres"]), ("points", A["points"]), ("offsets", A["offsets"]), ("ids", A["ids"]), ("zrows", zrows), ("ranks", ranks))}

    def scores():
        return CI.pair_scores(t["centres"], t["points"], t["offsets"], t["ids"])

    def depth():
        return CI.depth_ranges(t["points"], t["zrows"], t["offsets"], t["ids"], t["ranks"])

    if args.one_pass:
        CI.top_views(scores(), NUM_SRC)
        depth()
        torch.cuda.synchronize()
        return
    line = {"workload": "colmap_import", "sizes": "assumed, not taken from a COLMAP reconstruction", "images": N_IMAGES, "points": N_POINTS,
            "observations": int(len(A["ids"])), "mean_track": round(len(A["ids"]) / N_POINTS, 3), "num_src": NUM_SRC,
            "timing": "device events around each call, median of %d" % args.reps}
    S, line["pair_scores_ms"] = event_ms(scores, args.reps)
    (ids, _, cnt), line["top_views_ms"] = event_ms(lambda: CI.top_views(S, NUM_SRC), args.reps)
    dr, line["depth_ranks_ms"] = event_ms(depth, args.reps)
    line["gpu_total_ms"] = round(line["pair_scores_ms"] + line["top_views_ms"] + line["depth_ranks_ms"], 4)
    line["two_runs_bit_identical"] = bool(torch.equal(S.view(torch.int64), scores().view(torch.int64)))
    if args.rocprof:
        os.makedirs(args.rocprof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.abspath(args.rocprof), "-o", "colmap_import",
               "--", sys.executable, os.path.abspath(__file__), "--one-pass"]
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=900)
        if p.returncode == 0:
            from tools.dtu_eval_bench import kernel_stats
            line["kernels"] = kernel_stats(args.rocprof)
        else:
            line["kernels"] = f"rocprofv3 exit {p.returncode}"
    if args.no_cpu_baseline:
        line["cpu_baseline"] = "not measured"
    else:
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import colmap_oracle as O
        t0 = time.perf_counter()
        want, common = O.pair_scores(A["centres"], A["points"], A["offsets"], A["ids"])
        t1 = time.perf_counter()
        lists, wcnt = O.top_views(want, NUM_SRC)
        t2 = time.perf_counter()
        wdr = O.depth_ranks(A["points"], zrows, A["offsets"], A["ids"], ranks)
        t3 = time.perf_counter()
        got = S.cpu().numpy()
        same_lists = [[j for j in row if j >= 0] for row in ids.cpu().numpy().tolist()] == lists
        line["cpu_baseline"] = {"what": "tests/colmap_oracle.py (numpy, one process) on the same model, same host",
                                "pair_scores_ms": round((t1 - t0) * 1e3, 1), "top_views_ms": round((t2 - t1) * 1e3, 1),
                                "depth_ranks_ms": round((t3 - t2) * 1e3, 1), "total_ms": round((t3 - t0) * 1e3, 1)}
        line["vs_oracle"] = {"max_score_error_over_bound": float((np.abs(got - want) / (1e-12 * (1 + common))).max()),
                             "top_lists_equal": bool(same_lists), "counts_equal": bool(np.array_equal(cnt.cpu().numpy(), wcnt)),
                             "depth_ranks_bit_identical": bool(np.array_equal(dr.cpu().numpy().view(np.int64), wdr.view(np.int64)))}
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
