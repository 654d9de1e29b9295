"""TSDF fusion and marching tetrahedra (rc_mvsnet_amd/tsdf_mesh.py, csrc/tsdf_mesh.hip) on a synthetic scene: ms per phase from
the kernels' own timestamps, one JSON line.

The scene is synthetic and its size is ASSUMED (a DTU-like scan, not measured from one): 49 depth maps of 1184 x 1600 of a smooth
height field, seen from a 7 x 7 array of cameras above it, into 512 x 512 x 384 voxels, truncation 3 voxels.  Reported, each as
the median of --reps after a warm-up, from the start / stop timestamps of the launches themselves (the *_timed entry points):
    integrate_chunk_ms   one launch of 16 views
    count_scan_ms        the count kernel and the three-level scan (first kernel's start to last kernel's stop)
    emit_ms              the emit kernel
with the bytes-moved floor of each at 8 TB/s: for a chunk the five state planes read and written once; for count + scan the two
planes read, the two byte arrays written and read, the two start arrays written; for emit the two byte arrays read and the
outputs written.  ``oracle_ms`` is tests/tsdf_oracle.py (numpy, one process) on a 64^3 crop of the same grid on the same host.
``--rocprof DIR`` also runs one pass in a child process under ``rocprofv3 --kernel-trace --stats``.

    python tools/tsdf_mesh_bench.py [--reps 3] [--rocprof DIR] [--no-cpu-baseline] [--out profiles/tsdf_mesh_bench.json]
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

VIEWS, H, W, DIMS, VOXEL, TRUNC_VOXELS = 49, 1184, 1600, (512, 512, 384), 1.0, 3.0
ORIGIN = (-256.0, -256.0, 0.0)
FOCAL, HEIGHT, HBM_BYTES_PER_S = 2600.0, 1200.0, 8e12


def surface(x, y):
    return 192.0 + 40.0 * torch.sin(x / 80.0) * torch.cos(y / 60.0)


def scene(dev, views=VIEWS):
    """-> depth (views,H,W) fp32, rgb (views,H,W,3) uint8 on the device, cams (views,16) float64: cameras looking straight down"""
    R = np.diag([1.0, -1.0, -1.0])
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    rx, ry = (xs - 0.5 * W) / FOCAL, (ys - 0.5 * H) / FOCAL
    depth, cams = torch.empty((views, H, W), device=dev, dtype=torch.float32), []
    gen = torch.Generator(device=dev).manual_seed(0)
    for v in range(views):
        C = np.array([-150.0 + 50.0 * (v % 7), -150.0 + 50.0 * ((v // 7) % 7), HEIGHT])
        d = torch.full((H, W), HEIGHT - 192.0, device=dev, dtype=torch.float64)
        for _ in range(12):                                       # fixed-point ray / surface intersection
            d = HEIGHT - surface(C[0] + rx * d, C[1] - ry * d)
        depth[v] = (d + 0.25 * torch.randn((H, W), device=dev, dtype=torch.float64, generator=gen)).float()
        cams.append(np.concatenate([R.ravel(), -R @ C, [FOCAL, FOCAL, 0.5 * W, 0.5 * H]]))
    rgb = torch.randint(0, 256, (views, H, W, 3), device=dev, dtype=torch.uint8, generator=gen)
    return depth, rgb, np.stack(cams)


def timed_events():
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    ev[1].record()                                                # a torch event owns its hipEvent_t after a first record
    return ev


def ptr(t, dtype=torch.float32):
    return fusion._chk(t, "bench", dtype)


def integrate_timed(vol, depth, rgb, cams, trunc, ev):
    grid, dims = vol._host()
    n = depth.shape[0]
    _lib.call("rcmvs_tsdf_integrate_timed", ptr(depth), ptr(rgb, torch.uint8), n, H, W, np.ascontiguousarray(cams).ctypes.data_as(ctypes.c_void_p),
              trunc, grid, dims, ptr(vol.dsum), ptr(vol.wsum), *[ptr(c) for c in vol.csum], ctypes.c_void_p(ev[0].cuda_event),
              ctypes.c_void_p(ev[1].cuda_event), fusion._stream())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rocprof", default=None, help="directory: one pass in a child process under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--one-pass", action="store_true", help="(the profiled child) integrate, count, emit once, no timing")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    _lib.load()
    dev = "cuda:0"
    trunc = TRUNC_VOXELS * VOXEL
    depth, rgb, cams = scene(dev)
    vol = TM.TsdfVolume(ORIGIN, VOXEL, DIMS, dev)
    if args.one_pass:
        vol.integrate(depth, cams, rgb, trunc=trunc)
        vol.extract(1)
        torch.cuda.synchronize()
        return
    voxels = vol.voxels
    # integrate: the first chunk of 16 views over and over (the state keeps growing, the work per launch is the same)
    events = []
    for _ in range(args.reps + 1):                                # the first launch is the warm-up
        ev = timed_events()
        integrate_timed(vol, depth[:16], rgb[:16], cams[:16], trunc, ev)
        events.append(ev)
    torch.cuda.synchronize()
    chunk = [a.elapsed_time(b) for a, b in events[1:]]
    # the real state: all 49 views, once
    for p in [vol.dsum, vol.wsum] + vol.csum:
        p.zero_()
    t0 = time.perf_counter()
    vol.integrate(depth, cams, rgb, trunc=trunc)
    torch.cuda.synchronize()
    all_views_ms = (time.perf_counter() - t0) * 1e3

    edge_mask = torch.empty(voxels, device=dev, dtype=torch.uint8)
    tri_count = torch.empty(voxels, device=dev, dtype=torch.uint8)
    work = torch.empty(256 + 2 * ((voxels + TM.SCAN_TILE - 1) // TM.SCAN_TILE), device=dev, dtype=torch.int32)
    vert_start = torch.empty(voxels + 1, device=dev, dtype=torch.int32)
    tri_start = torch.empty(voxels + 1, device=dev, dtype=torch.int32)
    totals = torch.empty(2, device=dev, dtype=torch.int64)
    grid, dims = vol._host()
    events = []
    for _ in range(args.reps + 1):
        ev = timed_events()
        _lib.call("rcmvs_tsdf_mesh_count_timed", ptr(vol.dsum), ptr(vol.wsum), dims, 1, ptr(edge_mask, torch.uint8), ptr(tri_count, torch.uint8),
                  ptr(work, torch.int32), ptr(vert_start, torch.int32), ptr(tri_start, torch.int32), ptr(totals, torch.int64),
                  ctypes.c_void_p(ev[0].cuda_event), ctypes.c_void_p(ev[1].cuda_event), fusion._stream())
        events.append(ev)
    torch.cuda.synchronize()
    count = [a.elapsed_time(b) for a, b in events[1:]]
    nv, nf = (int(t) for t in totals.cpu())
    verts = torch.empty((nv, 3), device=dev, dtype=torch.float32)
    vrgb = torch.empty((nv, 3), device=dev, dtype=torch.uint8)
    faces = torch.empty((nf, 3), device=dev, dtype=torch.int32)
    events = []
    for _ in range(args.reps + 1):
        ev = timed_events()
        _lib.call("rcmvs_tsdf_mesh_emit_timed", ptr(vol.dsum), ptr(vol.wsum), *[ptr(c) for c in vol.csum], grid, dims, 1, ptr(edge_mask, torch.uint8),
                  ptr(tri_count, torch.uint8), ptr(vert_start, torch.int32), ptr(tri_start, torch.int32), nv, nf, ptr(verts), ptr(vrgb, torch.uint8),
                  ptr(faces, torch.int32), ctypes.c_void_p(ev[0].cuda_event), ctypes.c_void_p(ev[1].cuda_event), fusion._stream())
        events.append(ev)
    torch.cuda.synchronize()
    emit = [a.elapsed_time(b) for a, b in events[1:]]

    def row(times, floor_bytes, what):
        ms, floor = float(np.median(times)), floor_bytes / HBM_BYTES_PER_S * 1e3
        return {"ms": round(ms, 4), "ms_min": round(min(times), 4), "floor_ms": round(floor, 4), "floor_what": what,
                "fraction_of_floor_rate": round(floor / ms, 4)}

    line = {"workload": "tsdf_mesh", "sizes": "assumed, synthetic scene (not measured from a scan)", "views": VIEWS, "image": [H, W], "dims": list(DIMS),
            "voxels": voxels, "trunc_voxels": TRUNC_VOXELS, "timing": "the kernels' own start / stop timestamps, median of %d launches" % args.reps,
            "integrate_chunk": dict(row(chunk, 2 * 5 * 4 * voxels, "five fp32 state planes read and written once, at 8 TB/s"), views_per_launch=16),
            "integrate_all_views_wall_ms": round(all_views_ms, 2),
            "count_scan": row(count, 20 * voxels, "per voxel: dsum + wsum read (8 B), mask + count written and read (4 B), two starts written (8 B), at 8 TB/s"),
            "emit": row(emit, 2 * voxels + 15 * nv + 12 * nf, "mask + count read (2 B per voxel), vertices (15 B) and faces (12 B) written, at 8 TB/s"),
            "vertices": nv, "faces": nf, "observed_voxels": int((vol.wsum >= 1).sum())}
    referenced = int(torch.unique(faces).numel())
    line["unreferenced_vertices"] = nv - referenced
    if args.rocprof:
        os.makedirs(args.rocprof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.abspath(args.rocprof), "-o", "tsdf_mesh",
               "--", sys.executable, os.path.abspath(__file__), "--one-pass"]
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=900)
        if p.returncode == 0:
            from tools.dtu_eval_bench import kernel_stats
            line["kernels"] = kernel_stats(args.rocprof)
        else:
            line["kernels"] = f"rocprofv3 exit {p.returncode}"
    if args.no_cpu_baseline:
        line["oracle"] = "not measured"
    else:
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import tsdf_oracle as O
        crop, lo = (64, 64, 64), (224, 224, 160)                  # around the surface in the middle of the grid
        g = [ORIGIN[a] + lo[a] * VOXEL for a in range(3)] + [VOXEL]
        d_host, c_host = depth.cpu().numpy(), rgb.cpu().numpy()
        t0 = time.perf_counter()
        state = O.integrate(O.new_state(crop), d_host, cams, c_host, trunc, g, crop)
        t1 = time.perf_counter()
        r = O.extract(state["dsum"], state["wsum"], state["csum"], g, crop, 1)
        t2 = time.perf_counter()
        sub = TM.TsdfVolume(g[:3], VOXEL, crop, dev).integrate(depth, cams, rgb, trunc=trunc)
        v, f, c = sub.extract(1)
        same = (np.array_equal(v.cpu().numpy().view(np.uint32), r["verts"].view(np.uint32)) and np.array_equal(f.cpu().numpy(), r["faces"])
                and np.array_equal(c.cpu().numpy(), r["rgb"]))
        line["oracle"] = {"what": "tests/tsdf_oracle.py (numpy, one process) on a 64^3 crop of the grid, all 49 views, same host",
                          "integrate_ms": round((t1 - t0) * 1e3, 1), "extract_ms": round((t2 - t1) * 1e3, 1), "faces": int(len(r["faces"])),
                          "gpu_mesh_of_the_crop_equal_in_every_bit": bool(same)}
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
