"""Hole filling (rc_mvsnet_amd/mesh_holes.py, csrc/mesh_holes.hip) on the mesh of the dense TSDF bench's synthetic scene
(tools/tsdf_mesh_bench.py: 512 x 512 x 384 voxels, some 1.27 M vertices / 2.53 M faces) with --holes seeded caps of faces removed
(every face within --rings rings of a seeded vertex; caps that meet leave complex vertices, which are counted): ms per phase from
the kernels' own timestamps, one JSON line.

The scene is synthetic and its size is ASSUMED (a DTU-like scan, not measured from one).  Reported per phase, each as the median of
--reps after a warm-up, from the start / stop timestamps of the launches themselves (the *_timed entry points, first kernel's start
to last kernel's stop), next to the time its bytes would take at 8 TB/s if every array it must touch crossed HBM once per kernel
that needs it (b = the boundary half-edges, a / t = the vertices / faces added, L = the edges of the filled loops):
    boundary    init + one thread per corner + classify.  Floor: the four per-vertex arrays written and counts and arrays read
                again by the classification (16 nv + 8 nv + nv), faces read (12 nf), row_start and row_len (8 nv), the segments
                of nbr and mult that the bisections touch counted as all of both (48 nf)
    leaders     the walks + the two scans.  Floor: succ and pred read (8 nv), loop_len, the two counts written (9 nv), the counts
                read twice by the scans (10 nv), the ranks written (8 nv); the walks' own loads (4 L) are in it once
    emit        the bit copies + one lane per leader.  Floor: verts, faces and colours read and written (2 (15 nv + 12 nf)),
                loop_len read (4 nv), per member its successor, position and colour (19 L), the new faces and vertices (12 t + 15 a)
The adjacency that fill_holes() builds first is mesh_clean's and is timed by tools/mesh_clean_bench.py; here it is reported as its
own row.  The dependent loads of a walk (L of them in a row for the longest loop) and the atomics are in no floor: the ratio to the
floor is what they cost.  ``oracle`` is tests/mesh_holes_oracle.py (numpy and a Python walk, one process) on the same mesh on the
same host, and whether the GPU's result equals it in every bit.

    python tools/mesh_holes_bench.py [--reps 5] [--holes 3000] [--rings 2] [--max-edges 64] [--no-cpu-baseline] [--out profiles/mesh_holes_bench.json]
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
from rc_mvsnet_amd import _lib, mesh_clean as MC, mesh_holes as MH        # noqa: E402
from tools.mesh_clean_bench import ev_args, i32, i64, phase, timed, u8        # noqa: E402
from tools.tsdf_mesh_bench import DIMS, ORIGIN, TRUNC_VOXELS, VOXEL, ptr, scene        # noqa: E402
from rc_mvsnet_amd import tsdf_mesh as TM        # noqa: E402

WHAT = "see the docstring of tools/mesh_holes_bench.py"


def punch(verts_n, faces, holes, rings, seed=0):
    """faces without those within ``rings`` rings of ``holes`` seeded vertices (bench set-up, torch on the device)"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    marked = torch.zeros(verts_n, dtype=torch.bool, device=faces.device)
    marked[torch.randperm(verts_n, generator=gen)[:holes].to(faces.device)] = True
    idx = faces.long()
    for ring in range(rings):
        gone = marked[idx].any(1)
        if ring + 1 < rings:
            marked[idx[gone].reshape(-1)] = True
    return faces[~gone].contiguous(), int(gone.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--holes", type=int, default=3000)
    ap.add_argument("--rings", type=int, default=2)
    ap.add_argument("--max-edges", type=int, default=64)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    _lib.load()
    dev = "cuda:0"
    depth, rgb_views, cams = scene(dev)
    vol = TM.TsdfVolume(ORIGIN, VOXEL, DIMS, dev)
    vol.integrate(depth, cams, rgb_views, trunc=TRUNC_VOXELS * VOXEL)
    verts, whole, rgb = vol.extract(1)
    del vol, depth, rgb_views
    nv = int(verts.shape[0])
    faces, removed = punch(nv, whole, args.holes, args.rings)
    nf = int(faces.shape[0])
    E = lambda n, dt: torch.empty(n, device=dev, dtype=dt)        # noqa: E731

    # the 1-ring (mesh_clean's), then the three phases with the arrays fill_holes() allocates
    adj = MC.adjacency(nv, faces)
    cursor, heavy, awork, astats = E(nv, torch.int32), E(6 * nf // (MC.SORT_LIMIT + 1) + 1, torch.int32), MC._scan_work(nv, dev), E(6, torch.int64)
    a_ms = timed([lambda ev: _lib.call("rcmvs_mc_adjacency_timed", i32(faces), nv, nf, i32(adj["row_start"]), i32(adj["row_len"]), i32(adj["nbr"]),
                                       i32(adj["mult"]), u8(adj["on_boundary"]), i32(cursor), i32(heavy), int(heavy.numel()), i32(awork), i64(astats),
                                       *ev_args(ev))], args.reps)
    bnd = MH.boundary(nv, faces, adj)
    oc, ic, succ, pred = (E(nv, torch.int32) for _ in range(4))
    flags, cnt = E(nv, torch.uint8), E(2, torch.int64)
    b_ms = timed([lambda ev: _lib.call("rcmvs_mh_boundary_timed", i32(faces), nv, nf, i32(adj["row_start"]), i32(adj["row_len"]), i32(adj["nbr"]),
                                       i32(adj["mult"]), 6 * nf, i32(oc), i32(ic), i32(succ), i32(pred), u8(flags), i64(cnt), *ev_args(ev))], args.reps)
    assert torch.equal(succ, bnd["succ"]) and torch.equal(pred, bnd["pred"]) and torch.equal(flags, bnd["flags"])
    led = MH.leaders(bnd, args.max_edges)
    ll, vc, fc, vr, fr, tot = E(nv, torch.int32), E(nv, torch.uint8), E(nv, torch.int32), E(nv + 1, torch.int32), E(nv + 1, torch.int32), E(5, torch.int64)
    lwork = MC._scan_work(nv, dev)
    l_ms = timed([lambda ev: _lib.call("rcmvs_mh_leaders_timed", i32(succ), i32(pred), nv, args.max_edges, i32(ll), u8(vc), i32(fc), i32(vr), i32(fr),
                                       i32(lwork), i64(tot), *ev_args(ev))], args.reps)
    assert torch.equal(ll, led["loop_len"]) and torch.equal(vr, led["vert_rank"]) and torch.equal(fr, led["face_rank"])
    gv, gf, gc, stats = MH.fill_holes(verts, faces, rgb, max_edges=args.max_edges)
    nvo, nfo = int(gv.shape[0]), int(gf.shape[0])
    ov, of, ocol = torch.empty_like(gv), torch.empty_like(gf), torch.empty_like(gc)
    e_ms = timed([lambda ev: _lib.call("rcmvs_mh_emit_timed", ptr(verts), u8(rgb), i32(faces), nv, nf, i32(succ), i32(ll), i32(vr), i32(fr), nvo, nfo, ptr(ov),
                                       u8(ocol), i32(of), *ev_args(ev))], args.reps)
    assert torch.equal(ov.view(torch.int32), gv.view(torch.int32)) and torch.equal(of, gf) and torch.equal(ocol, gc)
    walls = []
    for _ in range(args.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        MH.fill_holes(verts, faces, rgb, max_edges=args.max_edges)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    a, t = stats["vertices_added"], stats["faces_added"]
    L = stats["boundary_edges"] - stats["boundary_edges_left"]
    line = {"workload": "mesh_holes", "sizes": "assumed, synthetic scene (not measured from a scan)", "vertices": nv, "faces_whole": int(whole.shape[0]),
            "faces": nf, "faces_removed": removed, "seeded_caps": args.holes, "rings": args.rings, "max_edges": args.max_edges,
            "timing": "the kernels' own start / stop timestamps, median of %d launches" % args.reps,
            "adjacency": {"ms": a_ms[0], "ms_min": a_ms[1], "what": "mesh_clean's 1-ring of the punched mesh; its floor is tools/mesh_clean_bench.py's"},
            "boundary": phase(b_ms, 25 * nv + 12 * nf + 8 * nv + 48 * nf, WHAT),
            "leaders": phase(l_ms, 35 * nv + 4 * L, WHAT),
            "emit": phase(e_ms, 2 * (15 * nv + 12 * nf) + 4 * nv + 19 * L + 12 * t + 15 * a, WHAT),
            "fill_holes_wall_ms": {"median": round(float(np.median(walls[1:])), 2), "min": round(min(walls[1:]), 2),
                                   "what": "fill_holes() end to end with its allocations, the adjacency and its host reads, host clock"},
            "stats": stats}
    if args.no_cpu_baseline:
        line["oracle"] = "not measured"
    else:
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import mesh_holes_oracle as O
        hv, hf, hc = verts.cpu().numpy(), faces.cpu().numpy(), rgb.cpu().numpy()
        t0 = time.perf_counter()
        wb = O.boundary(nv, hf)
        t1 = time.perf_counter()
        O.loops(wb)
        t2 = time.perf_counter()
        wv, wf, wc, wstats, _ = O.fill_holes(hv, hf, hc, args.max_edges)
        t3 = time.perf_counter()
        same = (np.array_equal(succ.cpu().numpy(), wb["succ"]) and np.array_equal(flags.cpu().numpy(), wb["flags"]) and stats == wstats and
                np.array_equal(gv.cpu().numpy().view(np.uint32), wv.view(np.uint32)) and np.array_equal(gf.cpu().numpy(), wf) and
                np.array_equal(gc.cpu().numpy(), wc))
        assert same, "the GPU's result differs from the oracle's"
        line["oracle"] = {"what": "tests/mesh_holes_oracle.py (numpy and a Python walk, one process) on the same mesh, same host",
                          "boundary_ms": round((t1 - t0) * 1e3, 1), "loops_ms": round((t2 - t1) * 1e3, 1), "fill_holes_ms": round((t3 - t2) * 1e3, 1),
                          "gpu_result_equal_in_every_bit": bool(same)}
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
