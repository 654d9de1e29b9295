"""Mesh decimation (rc_mvsnet_amd/mesh_decimate.py, csrc/mesh_decimate.hip) on the mesh of the dense TSDF bench's synthetic scene
(tools/tsdf_mesh_bench.py: 512 x 512 x 384 voxels, some 1.27 M vertices / 2.53 M faces) with cells of --voxels voxels (default 2 and
4): ms per phase from the kernels' own timestamps, one JSON line.

The scene is synthetic and its size is ASSUMED (a DTU-like scan, not measured from one).  Reported per phase and cell size, each as
the median of --reps after a warm-up, from the start / stop timestamps of the launches themselves (the *_timed entry points, first
kernel's start to last kernel's stop; a phase of several entry points is their sum), next to the time its bytes would take at
8 TB/s if every array it must touch crossed HBM once per kernel that needs it (P = the radix passes of the vertex sort, Q those of
the corner sort, m the clusters, c = 3 nf the corners):
    cluster     bounds + keys + sort + heads + scan + emit.  Floor: verts read twice (24 nv), per pass the pairs read twice and
                written once (36 nv P) and the digit table written and scanned (12 nv P / 256 x 256), the sorted keys read twice
                (16 nv), heads and ranks (10 nv), cluster, order written (8 nv), starts and keys (12 m)
    classify    map + table + insert + resolve.  Floor: faces read (12 nf), cface written and read twice (36 nf), classes written
                and read (3 nf), the table initialised (4 x capacity), cluster gathered (12 nf)
    quadrics    corner keys + sort + segments + accumulation.  Floor: faces read (12 nf), per pass the pairs read twice and
                written once (24 c Q) and the digit table (12 c Q / 256 x 256), the sorted keys and indices (8 c), per
                contributing corner its face and three positions (48 per corner, cache hits assumed free: counted once per face,
                12 nf + 12 nv), quadrics written (72 m)
    place       one thread per cluster.  Floor: order and the members' positions and colours (19 nv), quadrics (72 m), starts
                and keys (12 m), outputs (16 m)
    compact     select + mesh_clean's gather.  Floor: cface read twice (24 nf), classes (nf), flags and ranks written and read
                (nf + m and 8 (nf + m)), cluster vertices read (15 m), outputs written (15 nv' + 12 nf')
The hash table's atomics, the LDS histograms and the serial walks of long segments are not in any floor: the ratio to the floor is
what they and the gathers cost.  ``oracle`` is tests/mesh_decimate_oracle.py (numpy, one process) on the same mesh on the same
host, per phase, and whether the GPU's result equals it in every bit.

    python tools/mesh_decimate_bench.py [--reps 5] [--voxels 2 4] [--no-cpu-baseline] [--out profiles/mesh_decimate_bench.json]
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
from rc_mvsnet_amd import _lib, mesh_decimate as MD        # noqa: E402
from tools.mesh_clean_bench import ev_args, i32, i64, phase, timed, u8        # noqa: E402
from tools.tsdf_mesh_bench import DIMS, ORIGIN, TRUNC_VOXELS, VOXEL, ptr, scene        # noqa: E402
from rc_mvsnet_amd import tsdf_mesh as TM        # noqa: E402

WHAT = "see the docstring of tools/mesh_decimate_bench.py"


def f64(t):
    return ptr(t, torch.float64)


def bench_cell(verts, faces, rgb, cell, reps, cpu_baseline):
    dev = verts.device
    nv, nf = int(verts.shape[0]), int(faces.shape[0])
    E = lambda n, dt: torch.empty(n, device=dev, dtype=dt)        # noqa: E731
    lo, hi, _ = MD.bounds(verts)
    lat = MD.lattice(lo, hi, cell)
    lat_host, dims_host, plat, pg = MD._host_lattice(lat)          # the two host arrays plat / pg point into: alive for the whole function
    cells = lat["dims"][0] * lat["dims"][1] * lat["dims"][2]
    P = max(1, (cells.bit_length() + 7) // 8)
    # bounds + cluster
    bnd = E(8, torch.int32)
    key, idx = [E(nv, torch.int64) for _ in range(2)], [E(nv, torch.int32) for _ in range(2)]
    hist, hist_start, work = MD._sort_buffers(nv, dev)
    head, head_rank = E(nv, torch.uint8), E(nv + 1, torch.int32)
    cl = MD.cluster(verts, lat)
    m = cl["m"]
    c2, o2, s2, k2, tot = E(nv, torch.int32), E(nv, torch.int32), E(nv + 1, torch.int32), E(nv, torch.int64), E(2, torch.int64)
    c_ms = timed([lambda ev: _lib.call("rcmvs_md_bounds_timed", ptr(verts), nv, i32(bnd), *ev_args(ev)),
                  lambda ev: _lib.call("rcmvs_md_cluster_timed", ptr(verts), nv, plat, pg, i64(key[0]), i32(idx[0]), i64(key[1]), i32(idx[1]), i32(hist),
                                       i32(hist_start), i32(work), u8(head), i32(head_rank), i32(c2), i32(o2), i32(s2), i64(k2), i64(tot), *ev_args(ev))], reps)
    assert torch.equal(c2, cl["cluster"]) and torch.equal(o2, cl["order"]) and torch.equal(s2[:m + 1], cl["cluster_start"])
    # classify
    fc = MD.classify_faces(nv, faces, cl)
    capacity = 1 << max(1, (2 * nf).bit_length())
    table, cface, fclass, cnt4 = E(capacity, torch.int32), E((nf, 3), torch.int32), E(nf, torch.uint8), E(4, torch.int64)
    f_ms = timed([lambda ev: _lib.call("rcmvs_md_classify_faces_timed", i32(faces), nv, nf, i32(cl["cluster"]), i32(cface), u8(fclass), i32(table), capacity,
                                       i64(cnt4), *ev_args(ev))], reps)
    assert torch.equal(cface, fc["cface"]) and torch.equal(fclass, fc["face_class"])
    # quadrics
    n = 3 * nf
    Q = max(1, (m.bit_length() + 7) // 8)
    ck, ci = [E(n, torch.int32) for _ in range(2)], [E(n, torch.int32) for _ in range(2)]
    chist, chist_start, cwork = MD._sort_buffers(n, dev)
    seg, quad = E(2 * m, torch.int32), E((m, 9), torch.float64)
    q_ms = timed([lambda ev: _lib.call("rcmvs_md_quadrics_timed", ptr(verts), i32(faces), nv, nf, i32(cl["cluster"]), i64(cl["cluster_key"]), m, plat, pg,
                                       i32(ck[0]), i32(ci[0]), i32(ck[1]), i32(ci[1]), i32(chist), i32(chist_start), i32(cwork), i32(seg), f64(quad),
                                       *ev_args(ev))], reps)
    del ck, ci, chist, chist_start
    # place
    ov, oc, via, cnt3 = E((m, 3), torch.float32), E((m, 3), torch.uint8), E(m, torch.uint8), E(3, torch.int64)
    p_ms = timed([lambda ev: _lib.call("rcmvs_md_place_timed", ptr(verts), u8(rgb), nv, i32(cl["order"]), i32(cl["cluster_start"]), i64(cl["cluster_key"]), m,
                                       plat, pg, f64(quad), MD.PLACEMENTS["quadric"], MD.DEFAULT_REG, ptr(ov), u8(oc), u8(via), i64(cnt3), *ev_args(ev))], reps)
    # compact
    face_keep, vert_keep = E(nf, torch.uint8), E(m, torch.uint8)
    face_rank, vert_rank, tot2 = E(nf + 1, torch.int32), E(m + 1, torch.int32), E(2, torch.int64)
    swork = MD._scan_work(max(m, nf), dev)
    gv, gf, gc, stats = MD.decimate(verts, faces, rgb, cell=cell)
    nvo, nfo = int(gv.shape[0]), int(gf.shape[0])
    gv2, gf2, gc2 = torch.empty_like(gv), torch.empty_like(gf), torch.empty_like(gc)
    k_ms = timed([lambda ev: _lib.call("rcmvs_md_select_timed", i32(cface), u8(fclass), m, nf, 1, u8(face_keep), u8(vert_keep), i32(face_rank), i32(vert_rank),
                                       i32(swork), i64(tot2), *ev_args(ev)),
                  lambda ev: _lib.call("rcmvs_mc_gather_timed", ptr(ov), u8(oc), i32(cface), u8(face_keep), i32(face_rank), u8(vert_keep), i32(vert_rank), m, nf,
                                       nvo, nfo, ptr(gv2), u8(gc2), i32(gf2), *ev_args(ev))], reps)
    assert torch.equal(gf2, gf) and torch.equal(gv2.view(torch.int32), gv.view(torch.int32)) and torch.equal(gc2, gc)
    t0 = time.perf_counter()
    MD.decimate(verts, faces, rgb, cell=cell)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    corners = 3 * (nf - stats["invalid_faces"] - stats["unclustered_faces"])
    out = {"cell": cell, "lattice": lat["dims"], "vertex_sort_passes": P, "corner_sort_passes": Q, "clusters": m, "contributing_corners": corners,
           "cluster": phase(c_ms, 24 * nv + 36 * nv * P + 12 * nv * P + 16 * nv + 10 * nv + 8 * nv + 12 * m, WHAT),
           "classify": phase(f_ms, 12 * nf + 36 * nf + 3 * nf + 4 * capacity + 12 * nf, WHAT),
           "quadrics": phase(q_ms, 12 * nf + 24 * n * Q + 12 * n * Q + 8 * n + 12 * nf + 12 * nv + 72 * m, WHAT),
           "place": phase(p_ms, 19 * nv + 72 * m + 12 * m + 16 * m, WHAT),
           "compact": phase(k_ms, 24 * nf + nf + (nf + m) + 8 * (nf + m) + 15 * m + 15 * nvo + 12 * nfo, WHAT),
           "decimate_wall_ms": round(wall, 2), "stats": stats}
    if not cpu_baseline:
        out["oracle"] = "not measured"
        return out
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import mesh_decimate_oracle as O
    hv, hf, hc = verts.cpu().numpy(), faces.cpu().numpy(), rgb.cpu().numpy()
    t0 = time.perf_counter()
    wlo, whi, _ = O.bounds(hv)
    wlat = O.lattice(wlo, whi, cell)
    wcl = O.cluster(hv, wlat)
    t1 = time.perf_counter()
    wcface, wcls, _ = O.classify_faces(nv, hf, wcl)
    t2 = time.perf_counter()
    wquad = O.quadrics(hv, hf, wcl, wlat)
    t3 = time.perf_counter()
    wv, wc, wvia, _ = O.place(hv, hc, wcl, wlat, wquad)
    t4 = time.perf_counter()
    ov_, of_, oc_, wstats, _ = O.decimate(hv, hf, hc, cell=cell)
    same = (wlat == lat and np.array_equal(cl["cluster"].cpu().numpy(), wcl["cluster"]) and np.array_equal(fclass.cpu().numpy(), wcls) and
            np.array_equal(quad.cpu().numpy().view(np.uint64), wquad.view(np.uint64)) and np.array_equal(ov.cpu().numpy().view(np.uint32), wv.view(np.uint32)) and
            np.array_equal(oc.cpu().numpy(), wc) and np.array_equal(via.cpu().numpy(), wvia) and np.array_equal(gf.cpu().numpy(), of_) and
            np.array_equal(gv.cpu().numpy().view(np.uint32), ov_.view(np.uint32)) and np.array_equal(gc.cpu().numpy(), oc_) and stats == wstats)
    assert same, "the GPU's result differs from the oracle's"
    out["oracle"] = {"what": "tests/mesh_decimate_oracle.py (numpy, one process) on the same mesh, same host", "cluster_ms": round((t1 - t0) * 1e3, 1),
                     "classify_ms": round((t2 - t1) * 1e3, 1), "quadrics_ms": round((t3 - t2) * 1e3, 1), "place_ms": round((t4 - t3) * 1e3, 1),
                     "gpu_result_equal_in_every_bit": bool(same)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--voxels", type=float, nargs="+", default=[2.0, 4.0], help="cell edges in voxels of the bench volume")
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
    line = {"workload": "mesh_decimate", "sizes": "assumed, synthetic scene (not measured from a scan)", "vertices": int(verts.shape[0]),
            "faces": int(faces.shape[0]), "voxel": VOXEL, "timing": "the kernels' own start / stop timestamps, median of %d launches" % args.reps,
            "placement": "quadric", "reg": MD.DEFAULT_REG}
    for k in args.voxels:
        line["voxels_%g" % k] = bench_cell(verts, faces, rgb, k * VOXEL, args.reps, not args.no_cpu_baseline)
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
