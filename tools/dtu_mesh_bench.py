"""DTU mesh evaluation (rc_mvsnet_amd/dtu_eval.py: sample_mesh + evaluate_mesh) on a DTU-sized synthetic mesh: one JSON line.

No DTU Poisson mesh was available to size this, so the mesh is an assumption: a triangulated height field of --nx x --ny
vertices at --edge mm spacing (default 1000 x 800 at 0.4 mm: 1.6 M triangles over 400 x 320 mm) and 2.5 M stl points.  Timed
(synchronised wall time, median of --reps, after a warm-up): the super-sampling alone, the reduction of its cloud (with the
round count), and the whole ``evaluate_mesh``.  ``sample_bytes_written`` is the cloud the sampling writes (12 bytes a point);
``sample_hbm_bound_ms`` is that over 8 TB/s, the least time HBM allows for the write alone.  ``--rocprof DIR`` also runs one
evaluation in a child process under ``rocprofv3 --kernel-trace --stats`` and adds the kernels' totals.  The CPU baseline is the
vectorised numpy fp64 form of MeshSupSamp (tests/mesh_oracle.py), whose points the kernels must match bit for bit.

    python tools/dtu_mesh_bench.py [--reps 3] [--rocprof DIR] [--no-cpu-baseline]
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
sys.path.insert(0, os.path.join(REPO, "tools"))
from rc_mvsnet_amd import _lib, dtu_eval, synthetic        # noqa: E402
from dtu_eval_bench import kernel_stats, timed              # noqa: E402

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=1000)
    ap.add_argument("--ny", type=int, default=800)
    ap.add_argument("--edge", type=float, default=0.4)
    ap.add_argument("--n-stl", type=int, default=2_500_000)
    ap.add_argument("--dst", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rocprof", default=None, help="directory: one evaluation in a child process under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--one-scan", action="store_true", help="(the profiled child) one evaluate_mesh, no timing")
    args = ap.parse_args()
    _lib.load()
    dev = "cuda:0"
    s = synthetic.dtu_eval_mesh(nx=args.nx, ny=args.ny, edge=args.edge, n_stl=args.n_stl, res=4.0, seed=0)
    verts, faces = torch.from_numpy(s["verts"]).to(dev), torch.from_numpy(s["faces"]).to(dev)
    stl = torch.from_numpy(s["stl"]).to(dev)
    mask = torch.from_numpy(s["obs_mask"])

    def evaluate():
        return dtu_eval.evaluate_mesh(verts, faces, stl, mask, s["bb"], s["res"], s["plane"], dst=args.dst)

    evaluate()                                                   # warm-up (and the profiled child's whole run)
    torch.cuda.synchronize()
    if args.one_scan:
        return
    line = {"workload": "dtu_mesh", "assumed_sizes": "synthetic height-field mesh; no DTU mesh was available to size it",
            "n_verts": len(s["verts"]), "n_faces": len(s["faces"]), "edge_mm": args.edge, "n_stl": args.n_stl, "dst": args.dst}
    cloud, line["sample_ms"] = timed(lambda: dtu_eval.sample_mesh(verts, faces, args.dst), args.reps)
    line["n_points"] = len(cloud)
    line["n_samples"] = len(cloud) - len(s["verts"])
    line["sample_bytes_written"] = 12 * len(cloud)
    line["sample_hbm_bound_ms"] = round(12 * len(cloud) / HBM_BYTES_PER_S * 1e3, 4)
    (_, qdata), line["reduce_ms"] = timed(lambda: dtu_eval.reduce_points(cloud, args.dst, seed=0), args.reps)
    line["reduce_rounds"] = dtu_eval.last_reduce_rounds
    line["n_reduced"] = len(qdata)
    r, line["evaluate_mesh_ms"] = timed(evaluate, args.reps)
    line.update({k: r[k] for k in dtu_eval.STAT_FIELDS})
    if args.rocprof:
        os.makedirs(args.rocprof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.abspath(args.rocprof), "-o", "dtu_mesh",
               "--", sys.executable, os.path.abspath(__file__), "--one-scan", "--nx", str(args.nx), "--ny", str(args.ny),
               "--edge", str(args.edge), "--n-stl", str(args.n_stl), "--dst", str(args.dst)]
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=900)
        line["kernels"] = kernel_stats(args.rocprof) if p.returncode == 0 else f"rocprofv3 exit {p.returncode}"
    if args.no_cpu_baseline:
        line["cpu_baseline"] = "not measured"
    else:
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import mesh_oracle
        t0 = time.perf_counter()
        want = mesh_oracle.vectorised(s["verts"], s["faces"], args.dst)
        line["cpu_baseline"] = {"what": "numpy fp64 MeshSupSamp (tests/mesh_oracle.vectorised), one thread",
                                "ms": round((time.perf_counter() - t0) * 1e3, 1),
                                "bit_identical": bool(np.array_equal(want.astype(np.float32), cloud.cpu().numpy()))}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
