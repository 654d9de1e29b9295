"""The block-sparse TSDF volume (rc_mvsnet_amd/tsdf_mesh.py SparseTsdfVolume, csrc/tsdf_sparse.hip) on the synthetic scene of
tools/tsdf_mesh_bench.py: ms per phase from the kernels' own timestamps, one JSON line.

The scene is synthetic and its size is ASSUMED (a DTU-like scan, not measured from one): 49 depth maps of 1184 x 1600 of a smooth
height field in the box the dense bench cuts into 512 x 512 x 384 voxels.  Two grids over that box:
    a   voxel 1: 64 x 64 x 48 blocks, the dense bench's grid (its figures, measured in the same session, come in through --dense)
    b   voxel 1/4: 256 x 256 x 192 blocks = 2048 x 2048 x 1536 virtual voxels, a grid the dense volume refuses
Reported per grid, each as the median of --reps after a warm-up, from the start / stop timestamps of the launches themselves (the
*_timed entry points): mark and integrate per launch of 16 views, build, count + scan (first kernel's start to last kernel's
stop), emit; the active fraction, the allocated bytes and the floor of the state bytes read and written once at 8 TB/s.
``oracle`` is tests/tsdf_sparse_oracle.py (numpy, one process) on a crop of 8 x 8 x 8 blocks (64^3 voxels) of grid b on the same
host, and whether the GPU's mesh of that crop equals it in every bit.  ``--rocprof DIR`` also runs one pass of grid a in a child
process under ``rocprofv3 --kernel-trace --stats`` (kernel trace only).

    python tools/tsdf_sparse_bench.py [--reps 5] [--dense profiles/tsdf_mesh_bench.json] [--rocprof DIR] [--no-cpu-baseline]
                                      [--out profiles/tsdf_sparse_bench.json]
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
from rc_mvsnet_amd import _lib, fusion, tsdf_mesh as TM        # noqa: E402
from tools.tsdf_mesh_bench import H, HBM_BYTES_PER_S, ORIGIN, TRUNC_VOXELS, VIEWS, W, ptr, scene, timed_events        # noqa: E402

GRIDS = {"a": (1.0, (64, 64, 48)), "b": (0.25, (256, 256, 192))}
CHUNK = 16


def ev_args(ev):
    return ctypes.c_void_p(ev[0].cuda_event), ctypes.c_void_p(ev[1].cuda_event), fusion._stream()


def median_ms(launch, reps):
    """launch(ev) reps + 1 times (the first is the warm-up) -> the launches' own durations"""
    events = []
    for _ in range(reps + 1):
        ev = timed_events()
        launch(ev)
        events.append(ev)
    torch.cuda.synchronize()
    t = [a.elapsed_time(b) for a, b in events[1:]]
    return {"ms": round(float(np.median(t)), 4), "ms_min": round(min(t), 4)}


def cam_ptr(cams):
    return np.ascontiguousarray(cams).ctypes.data_as(ctypes.c_void_p)


def run_grid(name, depth, rgb, cams, reps, dev):
    voxel, bdims = GRIDS[name]
    trunc = TRUNC_VOXELS * voxel
    vol = TM.SparseTsdfVolume(ORIGIN, voxel, bdims, dev)
    grid, bd = vol._host()
    c16 = cams[:CHUNK]
    mark = median_ms(lambda ev: _lib.call("rcmvs_tsdf_sp_mark_timed", ptr(depth[:CHUNK]), CHUNK, H, W, cam_ptr(c16), trunc, grid, bd,
                                          ptr(vol.flags, torch.uint8), ptr(vol._skipped, torch.int64), *ev_args(ev)), reps)
    vol.flags.zero_()
    vol._skipped.zero_()
    t0 = time.perf_counter()
    vol.mark(depth, cams, trunc)
    torch.cuda.synchronize()
    mark_all_ms = (time.perf_counter() - t0) * 1e3
    words = (vol.blocks + 31) // 32
    mask_words = torch.empty(words, device=dev, dtype=torch.int32)
    word_rank = torch.empty(words + 1, device=dev, dtype=torch.int32)
    active = torch.empty(min(vol.blocks, TM.SP_MAX_ACTIVE), device=dev, dtype=torch.int32)
    work = torch.empty((words + TM.SP_SCAN_TILE - 1) // TM.SP_SCAN_TILE, device=dev, dtype=torch.int32)
    build = median_ms(lambda ev: _lib.call("rcmvs_tsdf_sp_build_timed", ptr(vol.flags, torch.uint8), bd, ptr(mask_words, torch.int32),
                                           ptr(word_rank, torch.int32), ptr(active, torch.int32), int(active.numel()), ptr(work, torch.int32),
                                           *ev_args(ev)), reps)
    n_active = vol.build()
    voxels = vol.voxels
    table = vol._table()
    integ = median_ms(lambda ev: _lib.call("rcmvs_tsdf_sp_integrate_timed", ptr(depth[:CHUNK]), ptr(rgb[:CHUNK], torch.uint8), CHUNK, H, W, cam_ptr(c16),
                                           trunc, grid, bd, ptr(vol.active, torch.int32), n_active, ptr(vol.dsum), ptr(vol.wsum),
                                           *[ptr(c) for c in vol.csum], *ev_args(ev)), reps)
    for p in [vol.dsum, vol.wsum] + vol.csum:
        p.zero_()
    t0 = time.perf_counter()
    vol.integrate(depth, cams, rgb, trunc=trunc)
    torch.cuda.synchronize()
    all_views_ms = (time.perf_counter() - t0) * 1e3

    edge_mask = torch.empty(voxels, device=dev, dtype=torch.uint8)
    tri_count = torch.empty(voxels, device=dev, dtype=torch.uint8)
    cwork = torch.empty(1024 + 2 * n_active, device=dev, dtype=torch.int32)
    vert_start = torch.empty(voxels + 1, device=dev, dtype=torch.int32)
    tri_start = torch.empty(voxels + 1, device=dev, dtype=torch.int32)
    totals = torch.empty(2, device=dev, dtype=torch.int64)
    count = median_ms(lambda ev: _lib.call("rcmvs_tsdf_sp_mesh_count_timed", ptr(vol.dsum), ptr(vol.wsum), bd, *table, 1, ptr(edge_mask, torch.uint8),
                                           ptr(tri_count, torch.uint8), ptr(cwork, torch.int32), ptr(vert_start, torch.int32),
                                           ptr(tri_start, torch.int32), ptr(totals, torch.int64), *ev_args(ev)), reps)
    nv, nf = (int(t) for t in totals.cpu())
    verts = torch.empty((nv, 3), device=dev, dtype=torch.float32)
    vrgb = torch.empty((nv, 3), device=dev, dtype=torch.uint8)
    faces = torch.empty((nf, 3), device=dev, dtype=torch.int32)
    emit = median_ms(lambda ev: _lib.call("rcmvs_tsdf_sp_mesh_emit_timed", ptr(vol.dsum), ptr(vol.wsum), *[ptr(c) for c in vol.csum], grid, bd, *table, 1,
                                          ptr(edge_mask, torch.uint8), ptr(tri_count, torch.uint8), ptr(vert_start, torch.int32),
                                          ptr(tri_start, torch.int32), nv, nf, ptr(verts), ptr(vrgb, torch.uint8), ptr(faces, torch.int32),
                                          *ev_args(ev)), reps)
    state_floor = 2 * 5 * 4 * voxels / HBM_BYTES_PER_S * 1e3
    integ.update(views_per_launch=CHUNK, floor_ms=round(state_floor, 4), floor_what="five fp32 state planes read and written once, at 8 TB/s",
                 ns_per_allocated_voxel_view=round(integ["ms"] * 1e6 / (voxels * CHUNK), 5))
    mark.update(views_per_launch=CHUNK)
    virtual = 512 * vol.blocks
    return {"voxel": voxel, "bdims": list(bdims), "virtual_voxels": virtual, "active_blocks": n_active, "active_fraction": round(n_active / vol.blocks, 5),
            "allocated_voxels": voxels, "allocated_state_bytes": 5 * 4 * voxels, "flag_and_mask_bytes": vol.blocks + 8 * words,
            "skipped_pixels": vol.skipped, "mark": mark, "mark_all_views_wall_ms": round(mark_all_ms, 2), "build": build, "integrate_chunk": integ,
            "integrate_all_views_wall_ms": round(all_views_ms, 2), "count_scan": count, "emit": emit, "vertices": nv, "faces": nf,
            "observed_voxels": int((vol.wsum >= 1).sum())}


def crop_against_the_oracle(depth, rgb, cams, dev):
    """8 x 8 x 8 blocks of grid b round the surface in the middle of the box: the numpy oracle's time, and the GPU's mesh against it"""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import tsdf_sparse_oracle as S
    voxel, bdims = GRIDS["b"][0], (8, 8, 8)
    trunc = TRUNC_VOXELS * voxel
    g = [-8.0, -8.0, 184.0, voxel]                                 # 16 world units a side; the surface is at z = 192 there
    d_host, c_host = depth.cpu().numpy(), rgb.cpu().numpy()
    t0 = time.perf_counter()
    flags, skipped = S.mark(d_host, cams, trunc, g, bdims)
    t1 = time.perf_counter()
    active = S.build(flags)[2]
    _, kept = S.integrate(bdims, active, d_host, cams, c_host, trunc, g)
    t2 = time.perf_counter()
    r = S.extract(kept, g, bdims, active, 1)
    t3 = time.perf_counter()
    vol = TM.SparseTsdfVolume(g[:3], voxel, bdims, dev)
    vol.mark(depth, cams, trunc)
    n = vol.build()
    v, f, c = vol.integrate(depth, cams, rgb, trunc=trunc).extract(1)
    same = (n == len(active) and vol.skipped == skipped and np.array_equal(v.cpu().numpy().view(np.uint32), r["verts"].view(np.uint32))
            and np.array_equal(f.cpu().numpy(), r["faces"]) and np.array_equal(c.cpu().numpy(), r["rgb"]))
    assert same, "the GPU's mesh of the crop differs from the oracle's"
    return {"what": "tests/tsdf_sparse_oracle.py (numpy, one process) on 8 x 8 x 8 blocks (64^3 voxels) of grid b, all 49 views, same host",
            "mark_ms": round((t1 - t0) * 1e3, 1), "integrate_ms": round((t2 - t1) * 1e3, 1), "extract_ms": round((t3 - t2) * 1e3, 1),
            "active_blocks": int(len(active)), "faces": int(len(r["faces"])), "gpu_mesh_of_the_crop_equal_in_every_bit": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dense", default=None, help="the JSON tools/tsdf_mesh_bench.py wrote in the same session: the yardstick of grid a")
    ap.add_argument("--rocprof", default=None, help="directory: one pass of grid a in a child process under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--one-pass", action="store_true", help="(the profiled child) mark, build, integrate, count, emit once on grid a, no timing")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    _lib.load()
    dev = "cuda:0"
    depth, rgb, cams = scene(dev)
    if args.one_pass:
        voxel, bdims = GRIDS["a"]
        vol = TM.SparseTsdfVolume(ORIGIN, voxel, bdims, dev)
        vol.mark(depth, cams, TRUNC_VOXELS * voxel)
        vol.build()
        vol.integrate(depth, cams, rgb, trunc=TRUNC_VOXELS * voxel).extract(1)
        torch.cuda.synchronize()
        return
    line = {"workload": "tsdf_sparse", "sizes": "assumed, synthetic scene (not measured from a scan)", "views": VIEWS, "image": [H, W],
            "trunc_voxels": TRUNC_VOXELS, "timing": "the kernels' own start / stop timestamps, median of %d launches" % args.reps}
    for name in GRIDS:
        line["grid_" + name] = run_grid(name, depth, rgb, cams, args.reps, dev)
    if args.dense:
        with open(args.dense) as f:
            d = json.loads(f.read())
        a = line["grid_a"]
        per_voxel_view = d["integrate_chunk"]["ms"] * 1e6 / (d["voxels"] * d["integrate_chunk"]["views_per_launch"])
        line["dense_same_session"] = {"integrate_chunk_ms": d["integrate_chunk"]["ms"], "count_scan_ms": d["count_scan"]["ms"], "emit_ms": d["emit"]["ms"],
                                      "voxels": d["voxels"], "ns_per_voxel_view": round(per_voxel_view, 5), "vertices": d["vertices"], "faces": d["faces"]}
        line["grid_a_against_dense"] = {
            "integrate_per_voxel_view_ratio": round(a["integrate_chunk"]["ns_per_allocated_voxel_view"] / per_voxel_view, 3),
            "integrate_chunk_ratio": round(a["integrate_chunk"]["ms"] / d["integrate_chunk"]["ms"], 3),
            "count_scan_ratio": round(a["count_scan"]["ms"] / d["count_scan"]["ms"], 3), "emit_ratio": round(a["emit"]["ms"] / d["emit"]["ms"], 3),
            "same_mesh_size": a["vertices"] == d["vertices"] and a["faces"] == d["faces"]}
    if args.rocprof:
        os.makedirs(args.rocprof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.abspath(args.rocprof), "-o", "tsdf_sparse",
               "--", sys.executable, os.path.abspath(__file__), "--one-pass"]
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=900)
        if p.returncode == 0:
            from tools.dtu_eval_bench import kernel_stats
            line["kernels"] = kernel_stats(args.rocprof)
        else:
            line["kernels"] = f"rocprofv3 exit {p.returncode}"
    line["oracle"] = "not measured" if args.no_cpu_baseline else crop_against_the_oracle(depth, rgb, cams, dev)
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
