"""DTU accuracy / completeness of fused point clouds on the HIP path.

The reference computes the paper's DTU numbers only in MATLAB (matlab_eval/BaseEvalMain_web_pt.m -> PointCompareMain.m ->
reducePts_haa.m / MaxDistCP.m, then ComputeStat_web_pt.m and compute_mean.m).  This module restates that pipeline on the
GPU (csrc/pointcloud.hip):

1. ``reduce_points``: reducePts_haa's 0.2 mm density reduction -- points visited in a permutation order, a point kept unless an
   earlier-visited KEPT point lies within ``dst``.  MATLAB's order comes from ``randperm`` and cannot be reproduced; here it is
   an explicit ``order`` or ``torch.randperm(n, generator=torch.Generator().manual_seed(seed))``.
2. ``nearest_distances``: MaxDistCP -- min(nearest-neighbour distance, cap), fp64; a from-point outside the 60 mm block lattice
   gets ``cap``.  MATLAB can report values above 60 for points far from everything; we report ``cap`` (the one intended
   difference; the statistics only use d < 20).  ``evaluate_scan`` asks for cap = ``outlier`` (20): the statistics are
   identical and far outliers stop their search sooner.
3. DataInMask / StlAbovePlane, the outlier threshold and ComputeStat_web_pt's statistics (fp64 sums, variance N - 1, the
   median of an even count = the mean of the two middle values, NaN for an empty set).

Meshes (BaseEvalMain_web.m with representation 'Surfaces'): ``sample_mesh`` is MeshSupSamp's super-sampling (csrc/pointcloud.hip,
samples computed in fp64 and rounded to fp32 once), ``evaluate_mesh`` scores that cloud as above, and ``error_colours`` /
``write_error_clouds`` give BaseEval2Obj_web.m's coloured clouds as binary PLY (MATLAB writes text OBJ).

CUDA tensors only; no CPU fallback.  ``python -m rc_mvsnet_amd.dtu_eval --plydir OUT --gtpath MVS_Data`` scores the clouds
``eval_driver --filter`` wrote; ``--surfaces --pattern ...`` scores meshes.
"""
import argparse
import ctypes
import json
import math
import os
import sys
import tempfile

import numpy as np
import torch

from . import _lib
from .ops import _chk, _stream

BLOCK, SCAN_TILE = 256, 2048                        # csrc/pointcloud.hip
MAX_CELLS = _lib.CONSTANTS["RCMVS_PC_MAX_CELLS"]
BBOX_BLOCKS, MOMENT_BLOCKS = 1024, 256
LATTICE = 60.0                                      # MaxDistCP's block edge (PointCompareMain: MaxDist = 60)
USED_SETS = (1, 4, 9, 10, 11, 12, 13, 15, 23, 24, 29, 32, 33, 34, 48, 49, 62, 75, 77, 110, 114, 118)     # GetUsedSets.m
STAT_FIELDS = ("nStl", "nData", "MeanStl", "MeanData", "VarStl", "VarData", "MedStl", "MedData")

# rounds of the last reduce_points call (the round count is data-dependent; tools/dtu_eval_bench.py records it)
last_reduce_rounds = 0


def _cdiv(a, b):
    return (a + b - 1) // b


def _points(pts, name):
    """(n,3) fp32 contiguous on the device, finite, n below 2^31 -> n"""
    _chk(pts, name)
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise _lib.RcmvsError(f"{name}: expected an (n,3) tensor, got {tuple(pts.shape)}")
    n = pts.shape[0]
    if n >= 1 << 31:
        raise _lib.RcmvsError(f"{name}: {n} points (below 2^31)")
    if n and not bool(torch.isfinite(pts).all()):
        raise _lib.RcmvsError(f"{name}: non-finite coordinates")
    return n


def _dbl(vals):
    vals = [float(v) for v in vals]
    return (ctypes.c_double * len(vals))(*vals)


def _host_ptr(arr):
    return ctypes.cast(arr, ctypes.c_void_p)


def bbox(pts):
    """(min xyz, max xyz) of a non-empty cloud as two fp32 numpy triples (one host synchronisation)."""
    n = _points(pts, "pts")
    if n == 0:
        raise _lib.RcmvsError("bbox: empty cloud")
    part = torch.empty(6 * BBOX_BLOCKS, device=pts.device, dtype=torch.float32)
    out = torch.empty(6, device=pts.device, dtype=torch.float32)
    _lib.call("rcmvs_pc_bbox", _chk(pts, "pts"), n, _chk(part, "part"), _chk(out, "out"), _stream())
    o = out.cpu().numpy()
    return o[:3], o[3:]


def cell_edge(lo, hi, h_min, max_cells):
    """The grid over [lo, hi]: the smallest edge >= h_min (about) whose grid has at most max_cells cells -> (h, dims)."""
    ext = [max(float(b) - float(a), 0.0) for a, b in zip(lo, hi)]
    vol = ext[0] * ext[1] * ext[2]
    h = max(h_min, max(ext) / max_cells, (vol / max_cells) ** (1.0 / 3.0) if vol > 0 else 0.0, 1e-30)

    def dims(h):
        return [int(math.floor(e / h)) + 1 for e in ext]

    while math.prod(dims(h)) > max_cells:
        h *= 1.01
    return h, dims(h)


class Grid:
    """A uniform grid over a cloud (rcmvs_pc_grid_build): the points in cell order, the first slot of every cell."""

    def __init__(self, pts, h_min, max_cells=None):
        n = _points(pts, "pts")
        if n == 0:
            raise _lib.RcmvsError("Grid: empty cloud")
        max_cells = min(MAX_CELLS, max(64, 8 * n)) if max_cells is None else min(int(max_cells), MAX_CELLS)
        lo, hi = bbox(pts)
        self.h, self.dims = cell_edge(lo, hi, h_min, max_cells)
        self.origin = [float(v) for v in lo]
        self.n = n
        ncell = math.prod(self.dims)
        dev = pts.device
        key = torch.empty(n, device=dev, dtype=torch.int32)
        count = torch.empty(ncell, device=dev, dtype=torch.int32)
        scan_work = torch.empty(_cdiv(ncell, SCAN_TILE) + 1, device=dev, dtype=torch.int32)
        self.cell_start = torch.empty(ncell + 1, device=dev, dtype=torch.int32)
        self.sorted = torch.empty((n, 4), device=dev, dtype=torch.float32)
        self.sorted_idx = torch.empty(n, device=dev, dtype=torch.int32)
        self._g = _dbl(self.origin + [self.h])
        self._d = (ctypes.c_int * 3)(*self.dims)
        _lib.call("rcmvs_pc_grid_build",
            _chk(pts, "pts"), n, _host_ptr(self._g), _host_ptr(self._d), _chk(key, "key", torch.int32), _chk(count, "count", torch.int32),
            _chk(scan_work, "scan_work", torch.int32), _chk(self.cell_start, "cell_start", torch.int32), _chk(self.sorted, "sorted"),
            _chk(self.sorted_idx, "sorted_idx", torch.int32), _stream())


def lattice_bounds(bb, edge=LATTICE):
    """MaxDistCP's block lattice over BB (2,3): [BB(1,:), BB(1,:) + (floor((BB(2,:) - BB(1,:)) / edge) + 1) edge), the upper
    bound computed as the last block's High (Low + edge)."""
    bb = np.asarray(bb, dtype=np.float64).reshape(2, 3)
    rng = np.floor((bb[1] - bb[0]) / edge)
    hi = (bb[0] + rng * edge) + edge
    return list(bb[0]), list(hi)


def nearest_distances(q_from, q_to, cap=60.0, lattice=None):
    """min(distance from every q_from point to its nearest q_to point, cap) as fp64 (n_from,); lattice = (BB, edge) or None:
    a from-point outside MaxDistCP's block lattice gets cap.  An empty q_to gives cap everywhere."""
    n_from = _points(q_from, "q_from")
    n_to = _points(q_to, "q_to")
    if not cap > 0 or not math.isfinite(cap):
        raise _lib.RcmvsError(f"nearest_distances: cap {cap}")
    out = torch.empty(n_from, device=q_from.device, dtype=torch.float64)
    if n_from == 0:
        return out
    lat = None
    if lattice is not None:
        lo, hi = lattice_bounds(*lattice) if isinstance(lattice, tuple) else lattice_bounds(lattice)
        lat = _dbl(lo + hi)
    if n_to:
        grid = Grid(q_to, h_min=1e-6 * cap)
        args = (_host_ptr(grid._g), _host_ptr(grid._d), _chk(grid.cell_start, "cell_start", torch.int32), _chk(grid.sorted, "sorted"))
    else:
        grid, args = None, (None, None, None, None)
    _lib.call("rcmvs_pc_nearest", _chk(q_from, "q_from"), n_from, *args, n_to, float(cap),
              None if lat is None else _host_ptr(lat), _chk(out, "out", torch.float64), _stream())
    return out


def permutation(n, seed=0):
    """The default visiting order of reduce_points: a CPU torch.randperm with a seeded generator."""
    return torch.randperm(n, generator=torch.Generator().manual_seed(int(seed)))


def reduce_points(pts, dst=0.2, order=None, seed=0):
    """reducePts_haa: -> (kept (n,) bool, pts[kept]).  order: the visiting order (a permutation of 0..n-1, any device);
    default ``permutation(n, seed)``.  The kept set is the sequential greedy's for that order, bit for bit."""
    global last_reduce_rounds
    n = _points(pts, "pts")
    if not dst > 0:
        raise _lib.RcmvsError(f"reduce_points: dst {dst}")
    dev = pts.device
    if n == 0:
        last_reduce_rounds = 0
        return torch.zeros(0, device=dev, dtype=torch.bool), pts
    order = permutation(n, seed) if order is None else torch.as_tensor(order)
    order = order.to(device=dev, dtype=torch.int64).contiguous()
    if order.shape != (n,) or not torch.equal(torch.sort(order).values, torch.arange(n, device=dev)):
        raise _lib.RcmvsError("reduce_points: order must be a permutation of 0 .. n-1")
    grid = Grid(pts, h_min=dst * 1.01)            # every neighbour within dst lies in the 27 cells around a point
    rank = torch.empty(n, device=dev, dtype=torch.int32)
    sorted_rank = torch.empty(n, device=dev, dtype=torch.int32)
    state = [torch.empty(n, device=dev, dtype=torch.uint8) for _ in range(2)]
    undecided = torch.empty(1, device=dev, dtype=torch.int32)
    _lib.call("rcmvs_pc_reduce_init", _chk(order, "order", torch.int64), _chk(grid.sorted_idx, "sorted_idx", torch.int32), n,
              _chk(rank, "rank", torch.int32), _chk(sorted_rank, "sorted_rank", torch.int32),
              _chk(state[0], "state", torch.uint8), _stream())
    rounds = 0
    while True:
        _lib.call("rcmvs_pc_reduce_round", _host_ptr(grid._g), _host_ptr(grid._d), _chk(grid.cell_start, "cell_start", torch.int32),
                  _chk(grid.sorted, "sorted"), _chk(sorted_rank, "sorted_rank", torch.int32),
                  _chk(state[0], "s_in", torch.uint8), _chk(state[1], "s_out", torch.uint8), n, float(dst),
                  _chk(undecided, "undecided", torch.int32), _stream())
        rounds += 1
        state.reverse()
        left = int(undecided.item())
        if left == 0:
            break
        if rounds > n:                             # every round decides at least the earliest undecided point
            raise _lib.RcmvsError(f"reduce_points: {left} points still undecided after {rounds} rounds")
    last_reduce_rounds = rounds
    kept = torch.empty(n, device=dev, dtype=torch.uint8)
    _lib.call("rcmvs_pc_reduce_finish", _chk(state[0], "state", torch.uint8), _chk(grid.sorted_idx, "sorted_idx", torch.int32), n,
              _chk(kept, "kept", torch.uint8), _stream())
    from .fusion import compact_points
    reduced, _ = compact_points(kept, pts)
    return kept.bool(), reduced


def _median(x):
    """MATLAB median of a 1-D fp64 device tensor: the mean of the two middle values for an even count, NaN when empty."""
    k = x.numel()
    if k == 0:
        return float("nan")
    s = torch.sort(x).values
    if k % 2:
        return float(s[k // 2])
    a, b = float(s[k // 2 - 1]), float(s[k // 2])
    return (a + b) / 2.0


def select_stats(pts, d, mode, params, thresh, obs_mask=None):
    """The points of pts whose flag holds (mode "mask": DataInMask with params = (BB(1,:), Res) and obs_mask (s1,s2,s3) bool
    indexed [x,y,z]; mode "plane": StlAbovePlane with params = P) and d < thresh -> (flags (n,) bool, their distances in point
    order, {n, mean, var, median})."""
    n = _points(pts, "pts")
    dev = pts.device
    if d.shape != (n,):
        raise _lib.RcmvsError(f"select_stats: {tuple(d.shape)} distances for {n} points")
    flags = torch.zeros(n, device=dev, dtype=torch.uint8)
    if n == 0:
        nan = float("nan")
        return flags.bool(), torch.zeros(0, device=dev, dtype=torch.float64), {"n": 0, "mean": nan, "var": nan, "median": nan}
    if mode == "mask":
        m = obs_mask.to(device=dev, dtype=torch.uint8)
        if m.dim() != 3:
            raise _lib.RcmvsError(f"select_stats: ObsMask must be 3-D, got {tuple(m.shape)}")
        s1, s2, s3 = m.shape
        mask = m.permute(2, 1, 0).contiguous()                   # column-major, as MATLAB stores it
        prm, code = [float(v) for v in params[0]] + [float(params[1])], 0
    elif mode == "plane":
        mask, (s1, s2, s3), code = None, (0, 0, 0), 1
        prm = [float(v) for v in np.asarray(params, dtype=np.float64).ravel()]
        if len(prm) != 4:
            raise _lib.RcmvsError("select_stats: the plane has 4 coefficients")
    else:
        raise _lib.RcmvsError(f"select_stats: mode {mode!r}")
    nblk = _cdiv(n, BLOCK)
    work = torch.empty(2 * nblk + 1 + _cdiv(nblk, SCAN_TILE) + 1, device=dev, dtype=torch.int32)
    sel = torch.empty(n, device=dev, dtype=torch.float64)
    p = _dbl(prm)
    _lib.call("rcmvs_pc_select", _chk(pts, "pts"), _chk(d, "d", torch.float64), n, code, _host_ptr(p),
              None if mask is None else _chk(mask, "obs_mask", torch.uint8), s1, s2, s3, float(thresh),
              _chk(flags, "flags", torch.uint8), _chk(sel, "out", torch.float64), _chk(work, "work", torch.int32),
              _stream())
    count = work[2 * nblk:2 * nblk + 1]
    part = torch.empty(MOMENT_BLOCKS, device=dev, dtype=torch.float64)
    stats = torch.empty(3, device=dev, dtype=torch.float64)
    _lib.call("rcmvs_pc_moments", _chk(sel, "x", torch.float64), _chk(count, "count", torch.int32), _chk(part, "part", torch.float64),
              _chk(stats, "stats", torch.float64), _stream())
    st = stats.cpu().tolist()
    k = int(st[0])
    sel = sel[:k]
    return flags.bool(), sel, {"n": k, "mean": st[1], "var": st[2], "median": _median(sel)}


def evaluate_scan(data, stl, obs_mask, bb, res, plane, dst=0.2, outlier=20.0, seed=0, order=None, per_point=False):
    """PointCompareMain + ComputeStat_web_pt for one scan.  data / stl: (n,3) fp32 device clouds; obs_mask (s1,s2,s3) bool
    indexed [x,y,z]; bb (2,3); res; plane (4,).  -> dict of BaseStat's fields (nStl, nData, MeanStl, MeanData, VarStl, VarData,
    MedStl, MedData); with per_point=True also Qdata (the reduced data), Ddata, Dstl, DataInMask, StlAbovePlane, whose
    distances are min(d, outlier) (the statistics only read d < outlier)."""
    _points(data, "data")
    _points(stl, "stl")
    bb = np.asarray(bb, dtype=np.float64).reshape(2, 3)
    _, qdata = reduce_points(data, dst=dst, order=order, seed=seed)
    ddata = nearest_distances(qdata, stl, cap=outlier, lattice=(bb, LATTICE))
    dstl = nearest_distances(stl, qdata, cap=outlier, lattice=(bb, LATTICE))
    in_mask, _, sd = select_stats(qdata, ddata, "mask", (bb[0], float(res)), outlier, obs_mask=torch.as_tensor(obs_mask))
    above, _, ss = select_stats(stl, dstl, "plane", plane, outlier)
    out = {"nStl": ss["n"], "nData": sd["n"], "MeanStl": ss["mean"], "MeanData": sd["mean"], "VarStl": ss["var"],
           "VarData": sd["var"], "MedStl": ss["median"], "MedData": sd["median"]}
    if per_point:
        out.update({"Qdata": qdata, "Ddata": ddata, "Dstl": dstl, "DataInMask": in_mask, "StlAbovePlane": above})
    return out


def sample_mesh(verts, faces, dst=0.2):
    """MeshSupSamp (BaseEvalMain_web.m's 'Surfaces' input): verts (n,3) fp32 and faces (m,3) int (0-based) on the device ->
    (n + samples, 3) fp32: the vertices, then the samples of face 0, 1, ... in MeshSupSamp's order.  Every sample is computed in
    fp64 as MeshSupSamp.cpp's SubTri does and rounded to fp32 once (MATLAB keeps the double: at most half an fp32 ulp apart).
    Raises RcmvsError for an index outside 0 .. n-1 and, before allocating the cloud, for 2^31 points or more."""
    nv = _points(verts, "verts")
    _chk(faces.contiguous(), "faces", faces.dtype)
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise _lib.RcmvsError(f"faces: expected an (m,3) tensor, got {tuple(faces.shape)}")
    if faces.dtype not in (torch.int32, torch.int64):
        raise _lib.RcmvsError(f"faces: integer indices expected, got {faces.dtype}")
    if not (dst > 0 and math.isfinite(dst)):
        raise _lib.RcmvsError(f"sample_mesh: dst {dst}")
    m = faces.shape[0]
    if m >= 1 << 31:
        raise _lib.RcmvsError(f"sample_mesh: {m} faces (below 2^31)")
    if m == 0:
        return verts.clone()
    if nv == 0:
        raise _lib.RcmvsError("sample_mesh: faces without vertices")
    if faces.dtype != torch.int32:
        if int(faces.min()) < 0 or int(faces.max()) >= nv:
            raise _lib.RcmvsError(f"sample_mesh: face indices outside 0 .. {nv - 1}")
        faces = faces.to(torch.int32)
    faces = faces.contiguous()
    dev, dst = verts.device, float(dst)
    args = (_chk(verts, "verts"), nv, _chk(faces, "faces", torch.int32), m, dst)
    tri_rows = torch.empty(m, device=dev, dtype=torch.int32)
    totals = torch.empty(3, device=dev, dtype=torch.int64)
    _lib.call("rcmvs_pc_mesh_rows", *args, _chk(tri_rows, "tri_rows", torch.int32), _chk(totals, "totals", torch.int64), _stream())
    rows, bad = totals[:2].tolist()
    if bad:
        raise _lib.RcmvsError(f"sample_mesh: {bad} faces index outside 0 .. {nv - 1}")
    if nv + rows >= 1 << 31:
        raise _lib.RcmvsError(f"sample_mesh: {nv} vertices + at least {rows} samples (dst {dst}): the scorer takes below 2^31 points")
    if rows == 0:
        return verts.clone()
    scan_work = torch.empty(_cdiv(max(m, rows), SCAN_TILE) + 1, device=dev, dtype=torch.int32)
    tri_row_start = torch.empty(m + 1, device=dev, dtype=torch.int32)
    row_len = torch.empty(rows, device=dev, dtype=torch.int32)
    _lib.call("rcmvs_pc_mesh_count", *args, _chk(tri_rows, "tri_rows", torch.int32), rows, _chk(scan_work, "scan_work", torch.int32),
              _chk(tri_row_start, "tri_row_start", torch.int32), _chk(row_len, "row_len", torch.int32),
              _chk(totals, "totals", torch.int64), _stream())
    samples = int(totals[2])
    if nv + samples >= 1 << 31:
        raise _lib.RcmvsError(f"sample_mesh: {nv} vertices + {samples} samples (dst {dst}): the scorer takes below 2^31 points")
    row_start = torch.empty(rows + 1, device=dev, dtype=torch.int32)
    out = torch.empty((nv + samples, 3), device=dev, dtype=torch.float32)
    _lib.call("rcmvs_pc_mesh_emit", *args, _chk(tri_row_start, "tri_row_start", torch.int32), _chk(row_len, "row_len", torch.int32),
              rows, samples, _chk(scan_work, "scan_work", torch.int32), _chk(row_start, "row_start", torch.int32),
              _chk(out, "out"), _stream())
    return out


def evaluate_mesh(verts, faces, stl, obs_mask, bb, res, plane, dst=0.2, outlier=20.0, seed=0, order=None, per_point=False):
    """BaseEvalMain_web.m with representation 'Surfaces': sample_mesh(verts, faces, dst), then evaluate_scan on that cloud
    (order, if given, is a permutation of its points)."""
    data = sample_mesh(verts, faces, dst)
    return evaluate_scan(data, stl, obs_mask, bb, res, plane, dst=dst, outlier=outlier, seed=seed, order=order, per_point=per_point)


ERROR_CAP = 10.0                                    # BaseEval2Obj_web.m's dist_tresshold (mm)


def error_colours(d, flag):
    """BaseEval2Obj_web.m's colours as (n,3) uint8 on d's device: alpha = min(d, 10) / 10; flag set: [1 0 0] alpha + [1 1 1]
    (1 - alpha) (white to red), clear: [0 1 0] alpha + [0 0 1] (1 - alpha) (blue to green); stored as floor(255 C + 0.5)."""
    a = torch.clamp(d.to(torch.float64), max=ERROR_CAP) / ERROR_CAP
    b = 1.0 - a
    f = flag.to(device=d.device, dtype=torch.bool)
    zero = torch.zeros_like(a)
    c = torch.where(f[:, None], torch.stack([a + b, b, b], 1), torch.stack([zero, a, b], 1))
    return torch.floor(255.0 * c + 0.5).to(torch.uint8)


def write_error_clouds(result, stl, out_dir, method, scan):
    """BaseEval2Obj_web.m as two binary PLY files (MATLAB writes text OBJ): <method>2Stl_<scan>.ply (the reduced data coloured by
    Ddata / DataInMask) and Stl2<method>_<scan>.ply (the stl points by Dstl / StlAbovePlane).  result: evaluate_scan(...,
    per_point=True).  -> the two paths."""
    from .fusion import ply_bytes
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for name, pts, d, flag in ((f"{method}2Stl_{scan}.ply", result["Qdata"], result["Ddata"], result["DataInMask"]),
                               (f"Stl2{method}_{scan}.ply", stl, result["Dstl"], result["StlAbovePlane"])):
        path = os.path.join(out_dir, name)
        with open(path, "wb") as f:
            f.write(ply_bytes(pts.cpu().numpy(), error_colours(d, flag).cpu().numpy()))
        paths.append(path)
    return paths


def summarize(per_scan):
    """compute_mean.m over a list of evaluate_scan results: acc = mean(MeanData), comp = mean(MeanStl), overall = their mean."""
    acc = float(np.mean([s["MeanData"] for s in per_scan]))
    comp = float(np.mean([s["MeanStl"] for s in per_scan]))
    return {"acc": acc, "comp": comp, "overall": (acc + comp) / 2.0}


# ---- files and command line -------------------------------------------------------------------------------------------
def scan_paths(plydir, gtpath, scan, pattern="scan{scan}.ply"):
    """The four files of one scan: <plydir>/<pattern formatted with scan=N> (default eval_driver's scan{N}.ply) and the DTU ground
    truth of MVS_Data."""
    return {"data": os.path.join(plydir, pattern.format(scan=scan)),
            "stl": os.path.join(gtpath, "Points", "stl", f"stl{scan:03d}_total.ply"),
            "mask": os.path.join(gtpath, "ObsMask", f"ObsMask{scan}_10.mat"),
            "plane": os.path.join(gtpath, "ObsMask", f"Plane{scan}.mat")}


def evaluate_files(plydir, gtpath, scan, device="cuda:0", dst=0.2, outlier=20.0, seed=0, pattern="scan{scan}.ply", surfaces=False,
                   error_clouds=None, method="rcmvsnet"):
    """evaluate_scan on one scan's files -> the BaseStat dict (plus "scan").  surfaces: the input is a triangle mesh, super-sampled
    at dst first (evaluate_mesh).  error_clouds: a folder for BaseEval2Obj_web's two coloured clouds (write_error_clouds)."""
    from .dtu_io import read_mat, read_ply_mesh, read_ply_xyz
    p = scan_paths(plydir, gtpath, scan, pattern)
    dev = torch.device(device)
    if surfaces:
        verts, faces = read_ply_mesh(p["data"])
        data = sample_mesh(torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev), dst)
    else:
        data = torch.from_numpy(read_ply_xyz(p["data"])).to(dev)
    stl = torch.from_numpy(read_ply_xyz(p["stl"])).to(dev)
    m = read_mat(p["mask"])
    for k in ("ObsMask", "BB", "Res"):
        if k not in m:
            raise _lib.RcmvsError(f"{p['mask']}: no variable {k}")
    pl = read_mat(p["plane"])
    if "P" not in pl:
        raise _lib.RcmvsError(f"{p['plane']}: no variable P")
    r = evaluate_scan(data, stl, torch.from_numpy(np.ascontiguousarray(m["ObsMask"]).astype(bool)), m["BB"],
                      float(np.asarray(m["Res"]).ravel()[0]), np.asarray(pl["P"], dtype=np.float64).ravel(), dst=dst, outlier=outlier, seed=seed,
                      per_point=error_clouds is not None)
    if error_clouds is not None:
        write_error_clouds(r, stl, error_clouds, method, scan)
        r = {k: r[k] for k in STAT_FIELDS}
    return dict(scan=scan, **r)


def main(argv=None):
    ap = argparse.ArgumentParser(description="DTU accuracy / completeness (mm) of fused point clouds or meshes, on the GPU")
    ap.add_argument("--plydir", required=True, help="folder of the inputs, named by --pattern (eval_driver --filter writes scan{N}.ply)")
    ap.add_argument("--gtpath", required=True, help="the DTU MVS_Data folder (Points/stl, ObsMask)")
    ap.add_argument("--scans", default=",".join(str(s) for s in USED_SETS), help="comma-separated scan numbers (default: GetUsedSets' 22)")
    ap.add_argument("--dst", type=float, default=0.2, help="reduction distance (mm)")
    ap.add_argument("--outlier", type=float, default=20.0, help="outlier threshold (mm)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the reduction's visiting order")
    ap.add_argument("--gpus", type=int, default=1, help="GPUs of this node: scans are sharded one process per GPU, no collective")
    ap.add_argument("--surfaces", action="store_true", help="the inputs are triangle meshes: super-sample them at --dst (MeshSupSamp) first")
    ap.add_argument("--pattern", default="scan{scan}.ply", help="input file name, formatted with the scan number, e.g. "
                    "'tola{scan:03d}_l3_surf_11_trim_8.ply' (default scan{scan}.ply)")
    ap.add_argument("--error-clouds", default=None, metavar="DIR", help="also write BaseEval2Obj_web's coloured clouds "
                    "<method>2Stl_<N>.ply and Stl2<method>_<N>.ply (binary PLY) into DIR")
    ap.add_argument("--method", default="rcmvsnet", help="method name in the --error-clouds file names")
    ap.add_argument("--results-dir", default=None, help=argparse.SUPPRESS)      # ranks' results for the parent's summary
    args = ap.parse_args(argv)
    argv = sys.argv[1:] if argv is None else list(argv)
    scans = [int(s) for s in args.scans.split(",") if s.strip()]
    try:
        args.pattern.format(scan=scans[0] if scans else 1)
    except (KeyError, IndexError, ValueError) as e:
        ap.error(f"--pattern {args.pattern!r}: {e!r} (the one field is {{scan}})")
    from .sharding import launch_ranks, launched, rank_env, shard_items
    if args.gpus > 1 and not launched():
        with tempfile.TemporaryDirectory() as tmp:
            rc = launch_ranks("rc_mvsnet_amd.dtu_eval", args.gpus, argv + ["--results-dir", tmp], module=True)
            if rc:
                raise SystemExit(rc)
            results = []
            for name in sorted(os.listdir(tmp)):
                with open(os.path.join(tmp, name)) as f:
                    results += json.load(f)
        results.sort(key=lambda r: scans.index(r["scan"]))
        if results:
            print(json.dumps(dict(summary=True, scans=len(results), **summarize(results))), flush=True)
        return results
    rank, local, world = rank_env()
    if not torch.cuda.is_available():
        raise SystemExit("dtu_eval: needs a GPU (the scorer has no CPU fallback)")
    device = "cuda:%d" % local
    torch.cuda.set_device(device)
    _lib.load()
    results = []
    for scan in shard_items(scans, rank, world):
        r = evaluate_files(args.plydir, args.gtpath, scan, device=device, dst=args.dst, outlier=args.outlier, seed=args.seed,
                           pattern=args.pattern, surfaces=args.surfaces, error_clouds=args.error_clouds, method=args.method)
        results.append(r)
        print(json.dumps(r), flush=True)
    if args.results_dir:
        with open(os.path.join(args.results_dir, f"rank{rank:04d}.json"), "w") as f:
            json.dump(results, f)
    elif world == 1 and results:
        print(json.dumps(dict(summary=True, scans=len(results), **summarize(results))), flush=True)
    return results


if __name__ == "__main__":
    main()
