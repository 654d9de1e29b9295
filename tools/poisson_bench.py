"""The Poisson reconstruction (rc_mvsnet_amd/poisson_mesh.py, csrc/poisson.hip) on the fused cloud of the synthetic whole scan of
tools/cloud_clean_bench.py (some 3.2 M points; its size is ASSUMED, a DTU-like scan, not measured from one) with the normals of
``estimate_normals(k=16)``, at resolutions 256 and 512: ms per phase, one JSON line, also written to profiles/poisson_bench.json.

Each phase is the median of --reps after a warm-up, from the start / stop timestamps of the launches themselves (the *_timed entry
points), next to the time its bytes would take at 8 TB/s if every array it must touch crossed HBM once (n points, v voxels):
    density     positions and normals read (24 n), eight 8-byte accumulators read and written per point (128 n); at most 8 n atomics
    normal      positions, normals and colours read (27 n), eight W (32 n), {s, W_p} written (16 n), 48 accumulators read and written
                (768 n); at most 48 n atomics
    splat       both, the zero fill of the 7 accumulator planes (56 v) and the seven fp32 planes from them (56 v + 32 v)
    rhs         three planes read, one written (16 v)
    sweep       x and b read, x' written (12 v): the +-y and +-z rows are expected from L2
    restrict    x and b read (8 v), the coarse b written (v / 2)
    prolong     x read and written (8 v), the coarse x read (v / 2)
    vcycle      per level with a coarser one: four sweeps, a restriction, a prolongation and (coarser levels) a zero fill; the coarsest:
                64 sweeps and a zero fill; the fine residual norm (8 v)
    iso         positions and {s, W_p} read (28 n), eight chi (32 n), the terms written and read (64 n)
    field       chi and W read (8 v), dsum and wsum written (8 v); the 27-voxel maximum is expected from L2
    count, emit tools/tsdf_mesh_bench.py's floors
Also ``reconstruct()``'s wall time, the device memory it holds at its peak, the dense TSDF bench's count and emit times from
profiles/tsdf_mesh_bench.json for comparison, and the numpy oracle (tests/poisson_oracle.py) on a 64^3 grid over every 16th point on
the same host, whose every plane the GPU's 64^3 result must equal in every bit.  The tool has no pass threshold: it records.

    python tools/poisson_bench.py [--reps 5] [--resolutions 256 512] [--no-oracle] [--out profiles/poisson_bench.json]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from rc_mvsnet_amd import _lib, cloud_clean as CC, fusion, poisson_mesh as PM        # noqa: E402
from rc_mvsnet_amd import tsdf_mesh as TM        # noqa: E402
from tools.cloud_clean_bench import fused_cloud        # noqa: E402
from tools.mesh_render_bench import timed        # noqa: E402

HBM_BYTES_PER_S = 8e12
WHAT = "see the docstring of tools/poisson_bench.py"


def entry(ms, floor_bytes, **more):
    floor_ms = floor_bytes / HBM_BYTES_PER_S * 1e3
    return dict({"ms_median": ms[0], "ms_min": ms[1], "bytes_floor": int(floor_bytes), "floor_ms": round(floor_ms, 5), "times_floor": round(ms[0] / floor_ms, 1)}, **more)


def vcycle_bytes(levels):
    """the floor of one V(2,2) cycle (the docstring's rule)"""
    vox = [math.prod(d) for d in levels]
    total = 8 * vox[0]
    for l, v in enumerate(vox):
        if l + 1 < len(vox):
            total += 4 * 12 * v + 8 * v + 4 * vox[l + 1] + 8 * v + 4 * vox[l + 1] + (4 * v if l else 0)
        else:
            total += PM._lib.CONSTANTS["RCMVS_PO_COARSEST_SWEEPS"] * 12 * v + (4 * v if l else 0)
    return total


def extraction(vol, reps):
    """the count and emit launches of the dense marching tetrahedra on the field, as tools/tsdf_mesh_bench.py times them"""
    dev, voxels = vol.device, vol.voxels
    ptr = lambda t, dtype=torch.float32: fusion._chk(t, "t", dtype)                                         # noqa: E731
    edge_mask, tri_count = (torch.empty(voxels, device=dev, dtype=torch.uint8) for _ in range(2))
    work = torch.empty(256 + 2 * ((voxels + TM.SCAN_TILE - 1) // TM.SCAN_TILE), device=dev, dtype=torch.int32)
    vert_start, tri_start = (torch.empty(voxels + 1, device=dev, dtype=torch.int32) for _ in range(2))
    totals = torch.empty(2, device=dev, dtype=torch.int64)
    grid, dims = vol._host()
    count = timed(lambda e0, e1: _lib.call("rcmvs_tsdf_mesh_count_timed", ptr(vol.dsum), ptr(vol.wsum), dims, 1, ptr(edge_mask, torch.uint8), ptr(tri_count, torch.uint8),
                                           ptr(work, torch.int32), ptr(vert_start, torch.int32), ptr(tri_start, torch.int32), ptr(totals, torch.int64), e0, e1,
                                           fusion._stream()), reps)
    nv, nf = (int(t) for t in totals.cpu())
    verts, faces = torch.empty((max(nv, 1), 3), device=dev, dtype=torch.float32), torch.empty((max(nf, 1), 3), device=dev, dtype=torch.int32)
    vrgb = torch.empty((max(nv, 1), 3), device=dev, dtype=torch.uint8) if vol.csum is not None else None
    emit = timed(lambda e0, e1: _lib.call("rcmvs_tsdf_mesh_emit_timed", ptr(vol.dsum), ptr(vol.wsum), *vol._colour_ptrs(), grid, dims, 1, ptr(edge_mask, torch.uint8),
                                          ptr(tri_count, torch.uint8), ptr(vert_start, torch.int32), ptr(tri_start, torch.int32), nv, nf, ptr(verts),
                                          TM._ptr(vrgb, "vert_rgb", torch.uint8), ptr(faces, torch.int32), e0, e1, fusion._stream()), reps)
    return {"count_scan": entry(count, 20 * voxels), "emit": entry(emit, 2 * voxels + 15 * nv + 12 * nf), "vertices": nv, "faces": nf}


def bench_resolution(xyz, nrm, rgb, resolution, reps):
    n = int(xyz.shape[0])
    lo, hi = PM._bounds(xyz, nrm)
    grid = PM.plan_grid(lo, hi, resolution)
    vol = PM.PoissonVolume(*grid, xyz.device)
    v = vol.voxels
    out = {"dims": vol.dims, "voxels": v, "voxel": vol.grid[3], "levels": vol.levels}
    out["density"] = entry(timed(lambda e0, e1: vol.splat(xyz, nrm, rgb, _timed=("density", e0, e1)), reps), 152 * n, atomics_at_most=8 * n)
    out["normal"] = entry(timed(lambda e0, e1: vol.splat(xyz, nrm, rgb, _timed=("normal", e0, e1)), reps), 843 * n, atomics_at_most=48 * n)
    out["splat"] = entry(timed(lambda e0, e1: vol.splat(xyz, nrm, rgb, _timed=("all", e0, e1)), reps), 995 * n + 144 * v)
    out["counters"] = {k: vol.stats[k] for k in PM.COUNTER_NAMES}
    rhs_args = [*[fusion._chk(p, "V") for p in vol.V], *vol._host(), fusion._chk(vol.b, "b")]
    out["rhs"] = entry(timed(lambda e0, e1: PM._call("rcmvs_po_rhs", rhs_args, ("all", e0, e1)), reps), 16 * v)
    vol.solve(0)
    out["sweep"] = entry(timed(lambda e0, e1: vol.solve(1, _timed=("sweep", e0, e1)), reps), 12 * v)
    if len(vol.levels) > 1:
        out["restrict"] = entry(timed(lambda e0, e1: vol.solve(1, _timed=("restrict", e0, e1)), reps), 8 * v + v // 2)
        out["prolong"] = entry(timed(lambda e0, e1: vol.solve(1, _timed=("prolong", e0, e1)), reps), 8 * v + v // 2)
    out["vcycle"] = entry(timed(lambda e0, e1: vol.solve(1, _timed=("all", e0, e1)), reps), vcycle_bytes(vol.levels))
    out["solve8"] = entry(timed(lambda e0, e1: vol.solve(8, _timed=("all", e0, e1)), reps), 8 * vcycle_bytes(vol.levels))
    out["residual_first_8_cycles"] = vol.stats["residual"][:8]      # from chi = 0: the timed single cycles above continue one solve
    out["iso"] = entry(timed(lambda e0, e1: vol.isovalue(_timed=("all", e0, e1)), reps), 124 * n)
    out["field"] = entry(timed(lambda e0, e1: vol.field(trim_relative=0.05, _timed=("all", e0, e1)), reps), 16 * v)
    out["iso_value"], out["wp_mean"], out["wp_min"], out["trimmed_voxels"] = vol.stats["iso"], vol.stats["wp_mean"], vol.stats["wp_min"], vol.stats["trimmed_voxels"]
    out.update(extraction(vol.field(trim_relative=0.05), reps))
    del vol
    walls = []
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = PM.reconstruct(xyz, nrm, rgb, resolution=resolution, trim_relative=0.05)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        del r
    out["reconstruct"] = {"wall_ms_median": round(float(np.median(walls)) * 1e3, 2), "wall_ms_all": [round(w * 1e3, 2) for w in walls],
                          "device_bytes_peak_above_the_cloud": int(torch.cuda.max_memory_allocated() - before)}
    return out


def oracle_comparison(xyz, nrm, rgb):
    """the numpy oracle on 64^3 over every 16th point, timed on this host, against the kernels on the same input: equal in every bit"""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import poisson_oracle as O
    sub = [t[::16].contiguous() for t in (xyz, nrm, rgb)]
    lo, hi = PM._bounds(sub[0], sub[1])
    origin, h, dims = PM.plan_grid(lo, hi, 64)
    grid = origin + [h]
    host = [t.cpu().numpy() for t in sub]
    t0 = time.perf_counter()
    ref = O.reconstruct(*host, grid, dims, 8, 0.0, 0.05)
    oracle_s = time.perf_counter() - t0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vol = PM.PoissonVolume(origin, h, dims, xyz.device)
    vol.splat(*sub).solve(8)
    tv = vol.field(trim_relative=0.05)
    torch.cuda.synchronize()
    gpu_s = time.perf_counter() - t0
    same = lambda a, b: bool(np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)))      # noqa: E731
    equal = {"acc": same(vol.acc.cpu().numpy().reshape(7, -1), ref["acc"]), "W": same(vol.W.cpu().numpy(), ref["W"]), "b": same(vol.b.cpu().numpy(), ref["b"]),
             "x": same(vol.x.cpu().numpy(), ref["x"]), "stats": same(vol.iso.cpu().numpy(), ref["stats"]), "dsum": same(tv.dsum.cpu().numpy(), ref["dsum"]),
             "wsum": same(tv.wsum.cpu().numpy(), ref["wsum"]), "residual": vol.stats["residual"] == [float(r) for r in ref["resid"]]}
    return {"points": int(sub[0].shape[0]), "dims": dims, "numpy_oracle_ms": round(oracle_s * 1e3, 1), "gpu_wall_ms": round(gpu_s * 1e3, 2), "equal_in_every_bit": equal,
            "all_equal": all(equal.values())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "poisson_bench.json"))
    args = ap.parse_args()
    _lib.load()
    dev = "cuda:0"
    xyz, rgb, view, centres = fused_cloud(dev)
    nrm, counters = CC.estimate_normals(xyz, 16, view, centres)
    result = {"what": WHAT, "device": torch.cuda.get_device_name(0), "points": int(xyz.shape[0]), "size": "assumed (synthetic scan)", "reps": args.reps,
              "hbm_bytes_per_s": HBM_BYTES_PER_S, "timing": "the kernels' own start / stop timestamps, median of %d" % args.reps,
              "normals": {k: counters[k] for k in ("with_normal", "degenerate", "oriented", "flipped")}, "resolutions": {}}
    for r in args.resolutions:
        result["resolutions"][str(r)] = bench_resolution(xyz, nrm, rgb, r, args.reps)
    dense = os.path.join(REPO, "profiles", "tsdf_mesh_bench.json")
    if os.path.exists(dense):
        with open(dense) as f:
            d = json.load(f)
        result["dense_tsdf_bench"] = {k: d[k] for k in ("dims", "voxels", "count_scan", "emit", "vertices", "faces") if k in d}
    if not args.no_oracle:
        result["oracle_64"] = oracle_comparison(xyz, nrm, rgb)
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
