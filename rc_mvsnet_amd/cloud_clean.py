"""Clean-up of a fused point cloud on the HIP path (csrc/cloud_knn.hip; the contract is csrc/cloud_knn.h, the per-element rules
csrc/cloud_knn_math.h, restated by tests/cloud_clean_oracle.py): k nearest neighbours, radius and statistical outlier removal,
normals from the neighbourhoods oriented towards the cameras, and the ordered compaction that keeps the input order.

``knn`` gives, for every point, its k nearest OTHER points ordered by (squared distance, input index), the squared distances in
fp64 from the fp32 coordinates.  A duplicate at another index is a neighbour at distance 0; slots that do not exist hold -1 / +inf.
The answer does not depend on the search grid: ``cell=`` forces a cell edge (tests use a tiny one, the default and one single cell).

``statistical_outliers`` is Open3D's ``remove_statistical_outlier`` with ``nb_neighbors = k + 1`` (Open3D counts the point itself;
its mean distance is ours times k / (k + 1), which scales mu, sigma and the bound alike), with two stated differences: a point is
kept when ``mean <= mu + ratio sigma`` where Open3D has ``<``, and there is no ``mean > 0`` test.  So a cloud whose means are all
equal keeps all its points, and duplicates are not dropped for being duplicates.  A point with fewer than k neighbours is not valid
and is dropped.  mu and sigma (N - 1) are reduced in fp64 in one fixed order: two runs give the same bits.

``estimate_normals`` takes the eigenvector of the smallest eigenvalue of the covariance of a point and its k neighbours (cyclic
Jacobi, fp64), makes its largest component positive, and, given the view that produced each point and the camera centres, flips it
towards that camera.  Neighbourhoods of fewer than 3 points, of duplicates only and of collinear points get a zero normal and are
counted.

The default cell edge comes from the box and the number of points (``dtu_eval.cell_edge``): the smallest edge whose grid has at most
n / OCCUPANCY cells, within RCMVS_PC_MAX_CELLS, so that a cell of a volume-filling cloud holds about OCCUPANCY points and the first
shell around a point (27 cells) about a hundred.  It is a performance choice only.

    python -m rc_mvsnet_amd.cloud_clean --in a.ply --out b.ply --radius 2.0 4 --stat 20 2.0 --normals 16 --viewpoint 0 0 0

Limits: n < 2^31, 1 <= k <= 32, n k <= 2^31 - 256; one lane walks the cells around one point, so a far outlier in a fine grid is slow
(it visits every shell up to its nearest neighbours); normals are not propagated along the surface, only flipped towards a camera.
No CPU fallback."""
import argparse
import ctypes
import json
import math

import numpy as np
import torch

from . import _lib, dtu_eval, fusion
from .mesh_clean import _ptr, _scan_work

MAX_K, MAX_NK, MAX_SWEEPS, COUNTERS = (_lib.CONSTANTS["RCMVS_CK_" + k] for k in ("MAX_K", "MAX_NK", "MAX_SWEEPS", "COUNTERS"))
PHASES = {"all": _lib.CONSTANTS["RCMVS_CK_PHASE_ALL"]}
MAX_CELLS = _lib.CONSTANTS["RCMVS_PC_MAX_CELLS"]
BBOX_BLOCKS, MOMENT_BLOCKS, PC_SCAN_TILE = (_lib.CONSTANTS["RCMVS_PC_" + k] for k in ("BBOX_BLOCKS", "MOMENT_BLOCKS", "SCAN_TILE"))
OCCUPANCY = 4                                                     # points per cell the default grid aims for
COUNTER_NAMES = ("with_normal", "too_few", "degenerate", "unconverged", "unoriented", "flipped", "oriented")
_NULL = ctypes.c_void_p(0)


def _call(name, args, _timed):
    if _timed is None:
        _lib.call(name, *args, fusion._stream())
    else:
        _lib.call(name + "_timed", *args, PHASES[_timed[0]], _timed[1], _timed[2], fusion._stream())


def _cloud(pts, what, name="pts"):
    if not torch.is_tensor(pts) or pts.dtype != torch.float32 or pts.dim() != 2 or pts.shape[1] != 3:
        raise _lib.RcmvsError(f"{what}: {name} must be an (n,3) float32 tensor, got "
                              f"{(tuple(pts.shape), pts.dtype) if torch.is_tensor(pts) else type(pts).__name__}")
    n = int(pts.shape[0])
    if n >= 1 << 31:
        raise _lib.RcmvsError(f"{what}: n = {n} points (below 2^31)")
    return n


def _k(k, n, what):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= MAX_K:
        raise _lib.RcmvsError(f"{what}: k = {k!r} (1 .. {MAX_K})")
    if n * int(k) > MAX_NK:
        raise _lib.RcmvsError(f"{what}: n k = {n * int(k)} (at most 2^31-256)")
    return int(k)


def finite_flags(pts, _timed=None):
    """-> (flags (n,) uint8 on the device: 1 where the point's three coordinates are finite, the number of such points)"""
    what = "cloud_clean.finite_flags"
    n = _cloud(pts, what)
    flags = torch.empty(n, device=pts.device, dtype=torch.uint8)
    count = torch.empty(1, device=pts.device, dtype=torch.int32)
    _call("rcmvs_ck_finite", [_ptr(pts, "pts", torch.float32), n, _ptr(flags, "flags", torch.uint8), fusion._chk(count, "count", torch.int32)], _timed)
    return flags, int(count.item())


def compact(keep, xyz, rgb=None, view=None, _timed=None):
    """The rows of xyz (n,3) fp32, rgb (n,3) uint8 and view (n,) int32 whose keep byte (0 / 1) is set, in input order -> dict of device
    tensors xyz, rgb, view (None where not given), index (the input index of every survivor, int32)."""
    what = "cloud_clean.compact"
    n = _cloud(xyz, what, "xyz")
    dev = xyz.device
    if not torch.is_tensor(keep) or keep.dtype != torch.uint8 or tuple(keep.shape) != (n,) or keep.device != dev:
        raise _lib.RcmvsError(f"{what}: keep must be an ({n},) uint8 tensor on the cloud's device")
    if rgb is not None and (not torch.is_tensor(rgb) or rgb.dtype != torch.uint8 or tuple(rgb.shape) != (n, 3) or rgb.device != dev):
        raise _lib.RcmvsError(f"{what}: rgb must be an ({n},3) uint8 tensor on the cloud's device or None")
    if view is not None and (not torch.is_tensor(view) or view.dtype != torch.int32 or tuple(view.shape) != (n,) or view.device != dev):
        raise _lib.RcmvsError(f"{what}: view must be an ({n},) int32 tensor on the cloud's device or None")
    out = {"xyz": torch.empty((n, 3), device=dev, dtype=torch.float32), "rgb": None if rgb is None else torch.empty((n, 3), device=dev, dtype=torch.uint8),
           "view": None if view is None else torch.empty(n, device=dev, dtype=torch.int32), "index": torch.empty(n, device=dev, dtype=torch.int32)}
    offsets = torch.empty(n + 1, device=dev, dtype=torch.int32)
    total = torch.empty(1, device=dev, dtype=torch.int64)
    work = _scan_work(n, dev)
    _call("rcmvs_ck_compact", [_ptr(keep, "keep", torch.uint8), _ptr(xyz, "xyz", torch.float32), _ptr(rgb, "rgb", torch.uint8), _ptr(view, "view", torch.int32), n,
                               fusion._chk(offsets, "offsets", torch.int32), fusion._chk(work, "scan_work", torch.int32),
                               _ptr(out["xyz"], "out_xyz", torch.float32), _ptr(out["rgb"], "out_rgb", torch.uint8), _ptr(out["view"], "out_view", torch.int32),
                               _ptr(out["index"], "out_index", torch.int32), fusion._chk(total, "total", torch.int64)], _timed)
    m = int(total.item())
    return {k: (None if v is None else v[:m]) for k, v in out.items()}


def finite_points(xyz, rgb=None, view=None):
    """compact() of the points whose coordinates are finite -> its dict plus "removed", the number of points dropped"""
    flags, count = finite_flags(xyz)
    out = compact(flags, xyz, rgb, view)
    out["removed"] = int(xyz.shape[0]) - count
    return out


class Grid:
    """The uniform grid of rcmvs_pc_bbox / rcmvs_pc_grid_build over a non-empty cloud of finite points: the scorer's grid (dtu_eval.Grid
    builds the same one through the same two entry points and dtu_eval.cell_edge), here with this module's rule for the edge.  cell
    None: the default edge (the module docstring); a number: the smallest edge, raised only as far as RCMVS_PC_MAX_CELLS demands."""

    def __init__(self, pts, cell=None, _timed=None):
        what = "cloud_clean.Grid"
        n = _cloud(pts, what)
        if n == 0:
            raise _lib.RcmvsError(f"{what}: empty cloud")
        dev = pts.device
        part = torch.empty(6 * BBOX_BLOCKS, device=dev, dtype=torch.float32)
        box = torch.empty(6, device=dev, dtype=torch.float32)
        _lib.call("rcmvs_pc_bbox", fusion._chk(pts, "pts"), n, fusion._chk(part, "part"), fusion._chk(box, "out"), fusion._stream())
        box = box.cpu().numpy().astype(np.float64)
        if not np.isfinite(box).all():
            raise _lib.RcmvsError(f"{what}: non-finite coordinates (finite_points removes them)")
        if cell is None:
            h_min, max_cells = 1e-30, min(MAX_CELLS, max(1, n // OCCUPANCY))
        else:
            h_min, max_cells = float(cell), MAX_CELLS
            if not (h_min > 0 and math.isfinite(h_min)):
                raise _lib.RcmvsError(f"{what}: cell = {cell!r} (finite and > 0)")
        self.h, self.dims = dtu_eval.cell_edge(box[:3], box[3:], h_min, max_cells)
        self.origin = [float(v) for v in box[:3]]
        self.n, self.cells = n, math.prod(self.dims)
        key = torch.empty(n, device=dev, dtype=torch.int32)
        count = torch.empty(self.cells, device=dev, dtype=torch.int32)
        work = torch.empty((self.cells + PC_SCAN_TILE - 1) // PC_SCAN_TILE + 1, device=dev, dtype=torch.int32)
        self.cell_start = torch.empty(self.cells + 1, device=dev, dtype=torch.int32)
        self.sorted = torch.empty((n, 4), device=dev, dtype=torch.float32)
        self.sorted_idx = torch.empty(n, device=dev, dtype=torch.int32)
        self._g = (ctypes.c_double * 4)(*(self.origin + [self.h]))
        self._d = (ctypes.c_int * 3)(*self.dims)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if _timed else None
        if ev:
            ev[0].record()
        _lib.call("rcmvs_pc_grid_build", fusion._chk(pts, "pts"), n, *self.host(), fusion._chk(key, "key", torch.int32), fusion._chk(count, "count", torch.int32),
                  fusion._chk(work, "scan_work", torch.int32), fusion._chk(self.cell_start, "cell_start", torch.int32), fusion._chk(self.sorted, "sorted"),
                  fusion._chk(self.sorted_idx, "sorted_idx", torch.int32), fusion._stream())
        if ev:
            ev[1].record()
            ev[1].synchronize()
            self.build_ms = ev[0].elapsed_time(ev[1])

    def host(self):
        return ctypes.cast(self._g, ctypes.c_void_p), ctypes.cast(self._d, ctypes.c_void_p)

    def args(self):
        return [*self.host(), fusion._chk(self.cell_start, "cell_start", torch.int32), fusion._chk(self.sorted, "sorted"),
                fusion._chk(self.sorted_idx, "sorted_idx", torch.int32)]

    def describe(self):
        return {"cell": self.h, "dims": list(self.dims), "cells": self.cells}


def _grid_args(pts, n, cell, grid):
    if n == 0:
        return None, [_NULL] * 5
    if grid is None:
        if finite_flags(pts)[1] != n:
            raise _lib.RcmvsError("cloud_clean: non-finite coordinates (finite_points removes them)")
        grid = Grid(pts, cell)
    if grid.n != n:
        raise _lib.RcmvsError(f"cloud_clean: the grid holds {grid.n} points, the cloud {n}")
    return grid, grid.args()


def knn_device(pts, k, cell=None, want=("idx", "d2"), counters=None, grid=None, _timed=None):
    """-> dict of the device tensors named in ``want`` (idx (n,k) int32, d2 (n,k) fp64, mean (n,) fp64) plus "grid".  pts must be
    finite (finite_points).  counters: a (2,) int64 device tensor that receives += cells read and candidates tested."""
    what = "cloud_clean.knn"
    n = _cloud(pts, what)
    k = _k(k, n, what)
    bad = [w for w in want if w not in ("idx", "d2", "mean")]
    if bad:
        raise _lib.RcmvsError(f"{what}: want = {want!r} (of idx, d2, mean)")
    dev = pts.device
    grid, gargs = _grid_args(pts, n, cell, grid)
    out = {"idx": torch.empty((n, k), device=dev, dtype=torch.int32) if "idx" in want else None,
           "d2": torch.empty((n, k), device=dev, dtype=torch.float64) if "d2" in want else None,
           "mean": torch.empty(n, device=dev, dtype=torch.float64) if "mean" in want else None}
    _call("rcmvs_ck_knn", [n, k, *gargs, _ptr(out["idx"], "idx", torch.int32), _ptr(out["d2"], "d2", torch.float64), _ptr(out["mean"], "mean", torch.float64),
                           _ptr(counters, "counters", torch.int64)], _timed)
    out["grid"] = grid.describe() if grid else None
    return out


def knn(pts, k, cell=None):
    """pts (n,3) fp32 on the device, finite -> (idx (n,k) int32, d2 (n,k) fp64): the k nearest other points of every point by
    (d2, index); -1 / +inf where n - 1 < k"""
    r = knn_device(pts, k, cell)
    return r["idx"], r["d2"]


def mean_distances(pts, k, cell=None):
    """-> (n,) fp64: the mean distance to the k nearest other points (the sum of the k square roots in rank order, one division), NaN
    where a point has fewer than k"""
    return knn_device(pts, k, cell, want=("mean",))["mean"]


def _ratio(ratio, what):
    try:
        ratio = float(ratio)
    except (TypeError, ValueError):
        raise _lib.RcmvsError(f"{what}: ratio = {ratio!r} (a number >= 0)") from None
    if not ratio >= 0:
        raise _lib.RcmvsError(f"{what}: ratio = {ratio} (>= 0; inf keeps every point with k neighbours)")
    return ratio


def statistical_from_means(mean, ratio, _timed=None):
    """the statistical rule on the mean distances (n,) fp64 -> (keep (n,) uint8, stats (8,) fp64: valid, mu, sigma, threshold, ...), on the device"""
    what = "cloud_clean.statistical_outliers"
    ratio = _ratio(ratio, what)
    n, dev = int(mean.shape[0]), mean.device
    flags, keep = (torch.empty(n, device=dev, dtype=torch.uint8) for _ in range(2))
    offsets = torch.empty(n + 1, device=dev, dtype=torch.int32)
    valid_mean = torch.empty(n, device=dev, dtype=torch.float64)
    part = torch.empty(MOMENT_BLOCKS, device=dev, dtype=torch.float64)
    stats = torch.empty(8, device=dev, dtype=torch.float64)
    work = _scan_work(n, dev)
    _call("rcmvs_ck_stat", [_ptr(mean, "mean", torch.float64), n, ratio, _ptr(flags, "flags", torch.uint8), fusion._chk(offsets, "offsets", torch.int32),
                            fusion._chk(work, "scan_work", torch.int32), _ptr(valid_mean, "valid_mean", torch.float64),
                            fusion._chk(part, "part", torch.float64), fusion._chk(stats, "stats", torch.float64), _ptr(keep, "keep", torch.uint8)], _timed)
    return keep, stats


def statistical_outliers(pts, k=20, ratio=2.0, cell=None):
    """-> (keep (n,) uint8 on the device: 1 = kept, info): the rule of the module docstring.  info: k, ratio, valid, mu, sigma, threshold
    (fp64, NaN when no point has k neighbours) and the grid."""
    what = "cloud_clean.statistical_outliers"
    _ratio(ratio, what)
    r = knn_device(pts, k, cell, want=("mean",))
    keep, stats = statistical_from_means(r["mean"], ratio)
    s = stats.cpu().tolist()
    return keep, {"k": int(k), "ratio": float(ratio), "valid": int(s[0]), "mu": s[1], "sigma": s[2], "threshold": s[3], "grid": r["grid"]}


def _radius(pts, radius, min_points, cell=None, grid=None, _timed=None):
    """radius_outliers plus the description of the grid it searched"""
    what = "cloud_clean.radius_outliers"
    n = _cloud(pts, what)
    try:
        radius = float(radius)
    except (TypeError, ValueError):
        raise _lib.RcmvsError(f"{what}: radius = {radius!r} (a number >= 0)") from None
    if not radius >= 0:
        raise _lib.RcmvsError(f"{what}: radius = {radius} (>= 0)")
    if isinstance(min_points, bool) or not isinstance(min_points, (int, np.integer)) or not 0 <= min_points < 1 << 31:
        raise _lib.RcmvsError(f"{what}: min_points = {min_points!r} (an integer, 0 .. 2^31-1)")
    dev = pts.device
    grid, gargs = _grid_args(pts, n, cell, grid)
    counts = torch.empty(n, device=dev, dtype=torch.int32)
    keep = torch.empty(n, device=dev, dtype=torch.uint8)
    _call("rcmvs_ck_radius", [n, radius * radius, int(min_points), *gargs, _ptr(counts, "count", torch.int32), _ptr(keep, "keep", torch.uint8)], _timed)
    return keep, counts, grid.describe() if grid else None


def radius_outliers(pts, radius, min_points, cell=None):
    """-> (keep (n,) uint8: 1 where at least min_points OTHER points lie within radius (d2 <= radius radius, formed once in fp64),
    counts (n,) int32: that number, saturating at min_points), both on the device.  radius = inf is allowed."""
    return _radius(pts, radius, min_points, cell)[:2]


def normals_from_neighbours(pts, idx, view=None, centres=None, _timed=None):
    """the normals of the neighbourhoods idx (n,k) int32 -> (normals (n,3) fp32, counters (COUNTERS,) int64), on the device"""
    what = "cloud_clean.estimate_normals"
    n = _cloud(pts, what)
    dev = pts.device
    if not torch.is_tensor(idx) or idx.dtype != torch.int32 or idx.dim() != 2 or idx.shape[0] != n or idx.device != dev:
        raise _lib.RcmvsError(f"{what}: idx must be an ({n},k) int32 tensor on the cloud's device")
    k = _k(int(idx.shape[1]), n, what)
    if (view is None) != (centres is None):
        raise _lib.RcmvsError(f"{what}: view and centres come together")
    nc, cen = 0, None
    if view is not None:
        if not torch.is_tensor(view) or view.dtype != torch.int32 or tuple(view.shape) != (n,) or view.device != dev:
            raise _lib.RcmvsError(f"{what}: view must be an ({n},) int32 tensor on the cloud's device")
        c = np.ascontiguousarray(np.asarray(centres.cpu() if torch.is_tensor(centres) else centres, dtype=np.float64))
        if c.ndim != 2 or c.shape[1] != 3 or not np.isfinite(c).all():
            raise _lib.RcmvsError(f"{what}: centres must be (nc,3) finite numbers")
        nc, cen = len(c), torch.from_numpy(c).to(dev)
    normals = torch.empty((n, 3), device=dev, dtype=torch.float32)
    counters = torch.empty(COUNTERS, device=dev, dtype=torch.int64)
    _call("rcmvs_ck_normals", [_ptr(pts, "pts", torch.float32), n, k, _ptr(idx, "idx", torch.int32), _ptr(view, "view", torch.int32), _ptr(cen, "centres", torch.float64), nc,
                               _ptr(normals, "normals", torch.float32), fusion._chk(counters, "counters", torch.int64)], _timed)
    return normals, counters


def counters_dict(counters):
    return dict(zip(COUNTER_NAMES, (int(x) for x in counters.cpu().tolist())))


def estimate_normals(pts, k=16, view=None, centres=None, cell=None):
    """pts (n,3) fp32 on the device, finite; view (n,) int32 and centres (nc,3) (host or device, taken as fp64), both or neither ->
    (normals (n,3) fp32 on the device, counters dict of COUNTER_NAMES).  A view number outside 0 .. nc-1 leaves the normal as it is."""
    r = knn_device(pts, k, cell, want=("idx",))
    normals, counters = normals_from_neighbours(pts, r["idx"], view, centres)
    return normals, dict(counters_dict(counters), k=int(k), grid=r["grid"])


def clean_options(radius=None, stat=None, normals=None):
    """The drivers' options (--cloud-radius R N, --cloud-stat K RATIO, --cloud-normals K) -> the dict ``clean_cloud`` and the ``clean``
    keyword of the fusion drivers take, or None when none is given"""
    out = {}
    if radius is not None:
        out["radius"] = (float(radius[0]), int(radius[1]))
    if stat is not None:
        out["stat"] = (int(stat[0]), float(stat[1]))
    if normals is not None:
        out["normals"] = int(normals)
    return out or None


def clean_cloud(xyz, rgb=None, view=None, centres=None, radius=None, stat=None, normals=None):
    """xyz (n,3) fp32, rgb (n,3) uint8, view (n,) int32 on the device; centres (nc,3).  The steps, each on the cloud the previous one
    left, each with its own grid, the input order kept throughout: the finite filter; radius = (R, N): keep points with at least N
    others within R; stat = (K, RATIO): the statistical rule; normals = K: normals of the K-neighbourhoods, oriented by view and
    centres when both are given.  -> dict: xyz, rgb, view, normals (None where absent), index (the input index of every point left,
    int32), all on the device, and stats: points in / out per step, mu, sigma, the threshold, the normal counters, the grids."""
    what = "cloud_clean.clean_cloud"
    n = _cloud(xyz, what, "xyz")
    if (view is None) != (centres is None):
        raise _lib.RcmvsError(f"{what}: view and centres come together")
    cur = finite_points(xyz, rgb, view)
    stats = {"in": n, "finite": {"in": n, "out": int(cur["xyz"].shape[0]), "removed": cur.pop("removed")}}
    index = cur["index"]

    def keep_only(keep):
        nonlocal cur, index
        cur = compact(keep, cur["xyz"], cur["rgb"], cur["view"])
        index = index[cur["index"].long()]                           # the survivors' indices into the caller's cloud

    if radius is not None:
        r, m = radius
        keep, _, grid = _radius(cur["xyz"], r, m)
        before = int(cur["xyz"].shape[0])
        keep_only(keep)
        stats["radius"] = {"radius": float(r), "min_points": int(m), "in": before, "out": int(cur["xyz"].shape[0]), "grid": grid}
    if stat is not None:
        k, ratio = stat
        keep, info = statistical_outliers(cur["xyz"], k, ratio)
        before = int(cur["xyz"].shape[0])
        keep_only(keep)
        stats["stat"] = dict(info, **{"in": before, "out": int(cur["xyz"].shape[0])})
    nrm = None
    if normals is not None:
        nrm, info = estimate_normals(cur["xyz"], normals, cur["view"], centres if cur["view"] is not None else None)
        stats["normals"] = info
    stats["out"] = int(cur["xyz"].shape[0])
    return {"xyz": cur["xyz"], "rgb": cur["rgb"], "view": cur["view"], "normals": nrm, "index": index, "stats": stats}


def main(argv=None):
    from . import dtu_io
    ap = argparse.ArgumentParser(description="clean a point-cloud PLY: outlier removal and oriented normals")
    ap.add_argument("--in", dest="src", required=True, help="the PLY to read (positions, vertex colours when it has them)")
    ap.add_argument("--out", required=True, help="the PLY to write: x y z [nx ny nz] red green blue")
    ap.add_argument("--radius", nargs=2, default=None, metavar=("R", "N"), help="keep points with at least N others within R")
    ap.add_argument("--stat", nargs=2, default=None, metavar=("K", "RATIO"), help="keep points whose mean distance to K neighbours is <= mu + RATIO sigma")
    ap.add_argument("--normals", type=int, default=None, metavar="K", help="add normals from the K nearest neighbours")
    ap.add_argument("--viewpoint", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="orient every normal towards this point")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    verts, _, rgb = dtu_io.read_ply_mesh_rgb(a.src)
    dev = torch.device(a.device)
    xyz = torch.from_numpy(np.ascontiguousarray(verts, np.float32)).to(dev)
    col = None if rgb is None else torch.from_numpy(np.ascontiguousarray(rgb, np.uint8)).to(dev)
    view = centres = None
    if a.viewpoint is not None:
        view, centres = torch.zeros(len(verts), device=dev, dtype=torch.int32), np.array([a.viewpoint], np.float64)
    opts = clean_options(None if a.radius is None else (float(a.radius[0]), int(a.radius[1])), None if a.stat is None else (int(a.stat[0]), float(a.stat[1])),
                         a.normals) or {}
    r = clean_cloud(xyz, col, view, centres, **opts)
    out_rgb = np.zeros((r["stats"]["out"], 3), np.uint8) if r["rgb"] is None else r["rgb"].cpu().numpy()
    with open(a.out, "wb") as f:
        f.write(fusion.ply_bytes(r["xyz"].cpu().numpy(), out_rgb, None if r["normals"] is None else r["normals"].cpu().numpy()))
    summary = {"in": a.src, "out": a.out, "cloud": r["stats"]}
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
