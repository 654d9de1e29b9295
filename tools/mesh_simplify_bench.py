"""Mesh simplification (rc_mvsnet_amd/mesh_simplify.py, csrc/mesh_simplify.hip) on the mesh of the dense TSDF bench's synthetic scene
(tools/tsdf_mesh_bench.py: 512 x 512 x 384 voxels, some 1.27 M vertices / 2.53 M faces) at --ratios (default 0.5 and 0.1): rounds,
collapses per round, ms per phase of a round from the kernels' own timestamps, the wall time of simplify(), one JSON line.

The scene is synthetic and its size is ASSUMED (a DTU-like scan, not measured from one).
    rounds      per ratio: the rounds simplify() needed, the collapses of every round and the edges the closed-ring rule selected in
                the first one as a fraction of the candidates -- the number that decides whether max_rounds reaches a ratio; the sum
                of the rounds' own durations (first launch's start to last launch's stop of every round) and the wall time of
                simplify() with its one host read a round, median of --reps
    first round each phase of the FIRST round (all faces live) on a fresh state, median of --reps, next to the time its bytes would
                take at 8 TB/s if every array it must touch crossed HBM once per kernel that needs it (e = 6 nf CSR entries, c = 3 nf
                corners, Q the radix passes of the corner sort):
        topology    mesh_clean's adjacency, the corner sort, the locked flags.  Floor: faces read three times (36 nf), nbr and mult
                    written, sorted and read (32 e), per pass the pairs read twice and written once (24 c Q) and the digit table
                    (12 c Q / 256 x 256), sorted keys and indices (8 c), rows, segments, cursor (24 nv), positions (12 nv)
        candidates  one lane per entry.  Floor: nbr, mult, edge, key (21 e), per candidate two quadrics (160 per edge, e / 2 edges,
                    cache hits assumed free: counted once per vertex, 80 nv), positions, locked, rows and segments (29 nv), faces
                    and their corners' indices (12 nf + 4 c)
        selection   best1, best2, flags, scan.  Floor: key read (8 e), nbr (4 e), best1 written and read, best2 written and read
                    (32 nv), edge read and flags written, read by the scan (3 e), ranks written (4 e)
        apply       collapses, remap, faces.  Floor: flags and ranks read, applied written (6 e), remap written and read (8 nv), faces
                    read and written (24 nf)
    The serial walks of rings and corners, the bisections and the fp64 arithmetic are in no floor: the ratio is what they cost.
``oracle`` is tests/mesh_simplify_oracle.py (Python, one process) on a crop of the first --crop faces on the same host: seconds for
one round, and whether the GPU's round equals it in every bit.

    python tools/mesh_simplify_bench.py [--reps 5] [--ratios 0.5 0.1] [--crop 20000] [--no-cpu-baseline] [--out profiles/mesh_simplify_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from rc_mvsnet_amd import _lib, mesh_simplify as MS        # noqa: E402
from tools.mesh_clean_bench import phase        # noqa: E402
from tools.tsdf_mesh_bench import DIMS, ORIGIN, TRUNC_VOXELS, VOXEL, scene, timed_events        # noqa: E402
from rc_mvsnet_amd import tsdf_mesh as TM        # noqa: E402

PHASES = ("all", "topology", "candidates", "selection", "apply")


def timed_round(state, target, which):
    ev = timed_events()
    r = MS.round(state, target, timed=(PHASES.index(which), ctypes.c_void_p(ev[0].cuda_event), ctypes.c_void_p(ev[1].cuda_event)))
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), r


def median(ts):
    return round(float(np.median(ts)), 4), round(min(ts), 4)


def first_round(verts, faces, rgb, reps):
    nv, nf = int(verts.shape[0]), int(faces.shape[0])
    e, c = 6 * nf, 3 * nf
    q = max(1, (nv.bit_length() + 7) // 8)
    floors = {"topology": (36 * nf + 32 * e + 24 * c * q + 12 * c * q + 8 * c + 36 * nv, "the docstring's topology floor, Q = %d" % q),
              "candidates": (21 * e + 80 * nv + 29 * nv + 12 * nf + 4 * c, "the docstring's candidates floor"),
              "selection": (8 * e + 4 * e + 32 * nv + 3 * e + 4 * e, "the docstring's selection floor"),
              "apply": (6 * e + 8 * nv + 24 * nf, "the docstring's apply floor")}
    out = {}
    for which in PHASES[1:] + ("all",):
        ts = []
        for _ in range(reps + 1):
            s = MS.begin(verts, faces, rgb)
            t, r = timed_round(s, 0, which)
            ts.append(t)
            del s
        out[which] = phase(median(ts[1:]), floors[which][0], floors[which][1]) if which in floors else {"ms": median(ts[1:])[0], "ms_min": median(ts[1:])[1]}
    out["candidates_edges"], out["selected_edges"] = r["candidates"], r["selected_edges"]
    out["selected_fraction_of_candidates"] = round(r["selected_edges"] / max(1, r["candidates"]), 5)
    return out


def run_ratio(verts, faces, rgb, ratio, reps):
    walls, sums, stats = [], [], None
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v, f, c, stats = MS.simplify(verts, faces, rgb, ratio=ratio)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    for _ in range(reps):                                         # the same loop with every round's own timestamps
        s = MS.begin(verts, faces, rgb)
        total, done = 0.0, 0
        while s["live"] > stats["target_faces"] and done < 256:
            t, r = timed_round(s, stats["target_faces"], "all")
            total, done = total + t, done + 1
            if r["selected_edges"] == 0:
                break
        sums.append(total)
        del s
    w, k = median(walls[1:]), median(sums)
    return {"target_faces": stats["target_faces"], "faces_out": stats["faces_out"], "vertices_out": stats["vertices_out"], "rounds": stats["rounds"],
            "stop": stats["stop"], "target_reached": stats["stop"] == "target", "collapses_per_round": stats["collapses"], "locked_vertices": stats["locked_vertices"],
            "rejected": {k2: stats["rejected_" + k2] for k2 in ("cost", "link", "flip")}, "placed": {n: stats["placed_" + n] for n in MS.PATH_NAMES},
            "max_cost": stats["max_cost"], "rounds_kernel_ms": k[0], "rounds_kernel_ms_min": k[1], "simplify_wall_ms": round(w[0], 2), "simplify_wall_ms_min": round(w[1], 2)}


def oracle_crop(verts, faces, rgb, crop):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import mesh_simplify_oracle as O
    f = faces[:crop].cpu().numpy()
    used = np.unique(f)
    number = np.full(int(verts.shape[0]), -1, np.int64)
    number[used] = np.arange(len(used))
    v, c, f = verts.cpu().numpy()[used], rgb.cpu().numpy()[used], number[f].astype(np.int32)
    t0 = time.perf_counter()
    S = O.begin(v, f, c)
    t1 = time.perf_counter()
    wr = O.round_(S, 0)
    t2 = time.perf_counter()
    dev = verts.device
    s = MS.begin(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(c).to(dev))
    t, gr = timed_round(s, 0, "all")
    used = int(wr["row_start"][-1])                               # the CSR entries in use

    def got(k):
        a = gr[k].cpu().numpy()
        a = a.view(np.uint64) if k in ("key", "best1", "best2") else a
        return a[:used] if k in ("nbr", "mult") else a

    same = all(np.array_equal(got(k), wr[k][:used] if k in ("nbr", "mult") else wr[k])
               for k in ("row_start", "row_len", "nbr", "mult", "locked", "edge", "key", "best1", "best2", "selected", "applied", "remap"))
    same = same and np.array_equal(s["faces"].cpu().numpy(), S["faces"]) and gr["applied_edges"] == wr["applied_edges"]
    assert same, "the GPU's round differs from the oracle's"
    return {"what": "tests/mesh_simplify_oracle.py (Python, one process) on the first %d faces, same host" % crop, "vertices": len(v), "faces": len(f),
            "begin_s": round(t1 - t0, 2), "round_s": round(t2 - t1, 2), "gpu_round_ms": round(t, 4), "applied_edges": wr["applied_edges"],
            "gpu_round_equal_in_every_bit": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ratios", type=float, nargs="+", default=[0.5, 0.1])
    ap.add_argument("--crop", type=int, default=20000, help="faces of the oracle's crop")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    _lib.load()
    dev = "cuda:0"
    depth, rgb_views, cams = scene(dev)
    vol = TM.TsdfVolume(ORIGIN, VOXEL, DIMS, dev)
    vol.integrate(depth, cams, rgb_views, trunc=TRUNC_VOXELS * VOXEL)
    verts, faces, rgb = vol.extract(1)
    del vol, depth, rgb_views
    line = {"workload": "mesh_simplify", "sizes": "assumed, synthetic scene (not measured from a scan)", "vertices": int(verts.shape[0]),
            "faces": int(faces.shape[0]), "voxel": VOXEL, "timing": "the kernels' own start / stop timestamps, median of %d" % args.reps, "max_rounds": 256,
            "first_round": first_round(verts, faces, rgb, args.reps)}
    for r in args.ratios:
        line["ratio_%g" % r] = run_ratio(verts, faces, rgb, r, args.reps)
    if not args.no_cpu_baseline:
        line["oracle"] = oracle_crop(verts, faces, rgb, args.crop)
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
