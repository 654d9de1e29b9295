"""The mesh clean-up pass (rc_mvsnet_amd/mesh_clean.py, csrc/mesh_clean.hip) on the mesh of the dense TSDF bench's synthetic scene
(tools/tsdf_mesh_bench.py: 512 x 512 x 384 voxels, some 1.27 M vertices / 2.53 M faces) plus --specks seeded floating tetrahedra: ms
per phase from the kernels' own timestamps, one JSON line.

The scene is synthetic and its size is ASSUMED (a DTU-like scan, not measured from one).  Reported per phase, each as the median of
--reps after a warm-up, from the start / stop timestamps of the launches themselves (the *_timed entry points, first kernel's start
to last kernel's stop; a phase of several entry points is their sum), next to the time its bytes would take at 8 TB/s if every
array it must touch crossed HBM once per kernel that needs it:
    components      validate + union-find + flatten + per-component face counts.  Floor: faces read by the hook and the count kernel
                    (2 x 12 nf), face_ok written and read (2 nf), label initialised, flattened (read + write) (12 nv), comp_faces
                    zeroed (4 nv)
    select_compact  component table + select + gather.  Floor: label and comp_faces read twice (16 nv), the two flag arrays written and
                    read by their scans and by the gather (3 x (nv + nf)) plus the table's flags (2 nv), three rank arrays written and
                    read (8 x (2 nv + nf)), faces read twice (24 nf), face_ok (nf), verts and rgb read (15 nv), the outputs written
                    (15 nv' + 12 nf')
    adjacency       degree, scan, fill, sort + collapse.  Floor: faces read twice (24 nf), the 6 nf neighbour entries written, read
                    and written again (72 nf), the multiplicities written (24 nf), cursor zeroed, counted, scanned and counted
                    down (16 nv), row_start written and read twice (12 nv), row_len and on_boundary written (5 nv)
    taubin_step     one lambda step.  Floor: positions read once and written once (24 nv), row_start, row_len, pins (9 nv), the
                    distinct neighbours' indices read (4 per entry); the gathered neighbour positions are assumed to hit in cache
The atomics of the union-find and of the degree count are not in any floor: the ratio to the floor is what they and the gathers cost.
``oracle`` is tests/mesh_clean_oracle.py (numpy, scipy.sparse.csgraph where it imports) on the same mesh on the same host, per
phase, and whether the GPU's result equals it in every bit.

    python tools/mesh_clean_bench.py [--reps 5] [--specks 3000] [--no-cpu-baseline] [--out profiles/mesh_clean_bench.json]
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
from rc_mvsnet_amd import _lib, fusion, mesh_clean as MC, tsdf_mesh as TM        # noqa: E402
from tools.tsdf_mesh_bench import DIMS, HBM_BYTES_PER_S, ORIGIN, TRUNC_VOXELS, VOXEL, ptr, scene, timed_events        # noqa: E402

TET = torch.tensor([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], dtype=torch.int32)


def bench_mesh(dev, specks, seed=0):
    """the dense bench's mesh with ``specks`` small tetrahedra floating above the surface appended"""
    depth, rgb, cams = scene(dev)
    vol = TM.TsdfVolume(ORIGIN, VOXEL, DIMS, dev)
    vol.integrate(depth, cams, rgb, trunc=TRUNC_VOXELS * VOXEL)
    verts, faces, colours = vol.extract(1)
    del vol, depth, rgb
    gen = torch.Generator(device="cpu").manual_seed(seed)
    centre = torch.rand((specks, 1, 3), generator=gen) * torch.tensor([500.0, 500.0, 60.0]) + torch.tensor([-250.0, -250.0, 290.0])
    corners = centre + 1.5 * torch.randn((specks, 4, 3), generator=gen)
    nv = int(verts.shape[0])
    speck_faces = (TET[None] + (nv + 4 * torch.arange(specks, dtype=torch.int32))[:, None, None]).reshape(-1, 3)
    speck_rgb = torch.randint(0, 256, (4 * specks, 3), generator=gen, dtype=torch.uint8)
    return (torch.cat([verts, corners.reshape(-1, 3).float().to(dev)]).contiguous(), torch.cat([faces, speck_faces.to(dev)]).contiguous(),
            torch.cat([colours, speck_rgb.to(dev)]).contiguous())


def ev_args(ev):
    return ctypes.c_void_p(ev[0].cuda_event), ctypes.c_void_p(ev[1].cuda_event), fusion._stream()


def timed(calls, reps):
    """calls: functions launch(ev) -> the median over reps of the sum of the launches' own durations (one warm-up first)"""
    runs = []
    for _ in range(reps + 1):
        events = [timed_events() for _ in calls]
        for launch, ev in zip(calls, events):
            launch(ev)
        runs.append(events)
    torch.cuda.synchronize()
    t = [sum(a.elapsed_time(b) for a, b in events) for events in runs[1:]]
    return round(float(np.median(t)), 4), round(min(t), 4)


def phase(ms, floor_bytes, what):
    floor = floor_bytes / HBM_BYTES_PER_S * 1e3
    return {"ms": ms[0], "ms_min": ms[1], "floor_ms": round(floor, 4), "ratio_to_floor": round(ms[0] / floor, 1), "floor_bytes": int(floor_bytes),
            "floor_what": what}


def i32(t):
    return ptr(t, torch.int32)


def u8(t):
    return ptr(t, torch.uint8)


def i64(t):
    return ptr(t, torch.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--specks", type=int, default=3000)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    _lib.load()
    dev = "cuda:0"
    verts, faces, rgb = bench_mesh(dev, args.specks)
    nv, nf = int(verts.shape[0]), int(faces.shape[0])
    min_faces = 100                                                          # drops the specks, keeps the surface

    # components
    comp = MC.components(verts, faces)
    c_ms = timed([lambda ev: _lib.call("rcmvs_mc_components_timed", i32(faces), nv, nf, i32(comp["label"]), u8(comp["face_ok"]), i32(comp["comp_faces"]),
                                       i64(comp["counts"]), *ev_args(ev))], args.reps)
    # component table + select + gather, with the arrays compact() allocates
    table, most = MC.component_table(comp, capacity=min(nv, nf))
    rows = int(table.shape[0])
    flags, rank = torch.empty(nv, device=dev, dtype=torch.uint8), torch.empty(nv + 1, device=dev, dtype=torch.int32)
    work = MC._scan_work(max(nv, nf), dev)
    tab = torch.empty((min(nv, nf), 2), device=dev, dtype=torch.int32)
    tot2, tot3 = torch.empty(2, device=dev, dtype=torch.int64), torch.empty(3, device=dev, dtype=torch.int64)
    face_keep, vert_keep = torch.empty(nf, device=dev, dtype=torch.uint8), torch.empty(nv, device=dev, dtype=torch.uint8)
    face_rank, vert_rank = torch.empty(nf + 1, device=dev, dtype=torch.int32), torch.empty(nv + 1, device=dev, dtype=torch.int32)
    ov, of, oc, info = MC.compact(verts, faces, rgb, comp, min_faces=min_faces)
    nvo, nfo = int(ov.shape[0]), int(of.shape[0])
    ov2, of2, oc2 = torch.empty_like(ov), torch.empty_like(of), torch.empty_like(oc)
    s_ms = timed([
        lambda ev: _lib.call("rcmvs_mc_component_table_timed", i32(comp["label"]), i32(comp["comp_faces"]), nv, u8(flags), i32(rank), i32(work), i32(tab),
                             int(tab.shape[0]), i64(tot2), *ev_args(ev)),
        lambda ev: _lib.call("rcmvs_mc_select_timed", i32(faces), u8(comp["face_ok"]), i32(comp["label"]), i32(comp["comp_faces"]), nv, nf, min_faces, 0.0, most,
                             0, 0, 0, 1, u8(face_keep), u8(vert_keep), i32(face_rank), i32(vert_rank), i32(work), i64(tot3), *ev_args(ev)),
        lambda ev: _lib.call("rcmvs_mc_gather_timed", ptr(verts), u8(rgb), i32(faces), u8(face_keep), i32(face_rank), u8(vert_keep), i32(vert_rank), nv, nf,
                             nvo, nfo, ptr(ov2), u8(oc2), i32(of2), *ev_args(ev))], args.reps)
    assert torch.equal(of2, of) and torch.equal(ov2.view(torch.int32), ov.view(torch.int32)) and torch.equal(oc2, oc)
    # adjacency of the compacted mesh
    adj = MC.adjacency(nvo, of)
    cursor = torch.empty(nvo, device=dev, dtype=torch.int32)
    heavy = torch.empty(6 * nfo // (MC.SORT_LIMIT + 1) + 1, device=dev, dtype=torch.int32)
    stats = torch.empty(6, device=dev, dtype=torch.int64)
    a_ms = timed([lambda ev: _lib.call("rcmvs_mc_adjacency_timed", i32(of), nvo, nfo, i32(adj["row_start"]), i32(adj["row_len"]), i32(adj["nbr"]), i32(adj["mult"]),
                                       u8(adj["on_boundary"]), i32(cursor), i32(heavy), int(heavy.numel()), i32(work), i64(stats), *ev_args(ev))], args.reps)
    entries = int(adj["row_len"].sum())
    seg = (adj["row_start"][1:] - adj["row_start"][:-1])
    # one Taubin step
    dst = torch.empty_like(ov)
    t_ms = timed([lambda ev: _lib.call("rcmvs_mc_taubin_step_timed", ptr(ov), ptr(dst), nvo, i32(adj["row_start"]), i32(adj["row_len"]), i32(adj["nbr"]),
                                       int(adj["nbr"].numel()), u8(adj["on_boundary"]), 0.5, *ev_args(ev))], args.reps)
    t0 = time.perf_counter()
    cv, cf, cc, cstats = MC.clean_mesh(verts, faces, rgb, min_faces=min_faces, smooth_iterations=10)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3

    line = {"workload": "mesh_clean", "sizes": "assumed, synthetic scene (not measured from a scan)", "vertices": nv, "faces": nf, "specks": args.specks,
            "min_faces": min_faces, "timing": "the kernels' own start / stop timestamps, median of %d launches" % args.reps,
            "components": phase(c_ms, 2 * 12 * nf + 2 * nf + 12 * nv + 4 * nv, "see the docstring of tools/mesh_clean_bench.py"),
            "select_compact": phase(s_ms, 16 * nv + 3 * (nv + nf) + 2 * nv + 8 * (2 * nv + nf) + 24 * nf + nf + 15 * nv + 15 * nvo + 12 * nfo,
                                    "see the docstring of tools/mesh_clean_bench.py"),
            "adjacency": phase(a_ms, 24 * nfo + 72 * nfo + 24 * nfo + 16 * nvo + 12 * nvo + 5 * nvo, "see the docstring of tools/mesh_clean_bench.py"),
            "taubin_step": phase(t_ms, 24 * nvo + 9 * nvo + 4 * entries, "see the docstring of tools/mesh_clean_bench.py"),
            "components_in": rows, "vertices_out": nvo, "faces_out": nfo, "neighbour_entries": entries, "longest_segment": int(seg.max()),
            "segments_on_the_long_path": adj["long_segments"], "sort_limit": MC.SORT_LIMIT,
            "clean_mesh_10_iterations_wall_ms": round(wall, 2), "stats": cstats}
    if args.no_cpu_baseline:
        line["oracle"] = "not measured"
    else:
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import mesh_clean_oracle as O
        hv, hf, hc = verts.cpu().numpy(), faces.cpu().numpy(), rgb.cpu().numpy()
        t0 = time.perf_counter()
        label, ok, comp_faces, _ = O.components(nv, hf)
        t1 = time.perf_counter()
        wv, wf, wc, _ = O.compact(hv, hf, hc, min_faces=min_faces)              # runs the components again: its time includes them
        t2 = time.perf_counter()
        wadj = O.adjacency(len(wv), wf)
        t3 = time.perf_counter()
        step = O.taubin_step(wv, wadj, 0.5, wadj["on_boundary"])
        t4 = time.perf_counter()
        n = wadj["defined"]
        same = (np.array_equal(comp["label"].cpu().numpy(), label) and np.array_equal(of.cpu().numpy(), wf) and
                np.array_equal(ov.cpu().numpy().view(np.uint32), wv.view(np.uint32)) and np.array_equal(oc.cpu().numpy(), wc) and
                np.array_equal(adj["nbr"].cpu().numpy()[:n], wadj["nbr"][:n]) and np.array_equal(adj["mult"].cpu().numpy()[:n], wadj["mult"][:n]) and
                np.array_equal(dst.cpu().numpy().view(np.uint32), step.view(np.uint32)))
        assert same, "the GPU's result differs from the oracle's"
        line["oracle"] = {"what": "tests/mesh_clean_oracle.py (numpy + scipy.sparse.csgraph, one process) on the same mesh, same host",
                          "components_ms": round((t1 - t0) * 1e3, 1), "select_compact_incl_components_ms": round((t2 - t1) * 1e3, 1),
                          "adjacency_ms": round((t3 - t2) * 1e3, 1), "taubin_step_ms": round((t4 - t3) * 1e3, 1), "gpu_result_equal_in_every_bit": bool(same)}
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
