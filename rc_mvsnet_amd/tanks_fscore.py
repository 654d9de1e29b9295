"""Tanks and Temples F-score of fused point clouds on the HIP path.

The benchmark scores a reconstruction with its python_toolbox/evaluation (Open3D): align the estimate to the ground truth through
the camera trajectory, refine the alignment with three rounds of ICP on cropped, down-sampled clouds, then crop, voxel down-sample
at tau / 2, take both nearest-neighbour distance sets and report precision (estimate within tau of the ground truth), recall
(ground truth within tau of the estimate) and their harmonic mean.  Neither the toolbox nor Open3D is part of the reference; the
arithmetic is stated here and in csrc/pc_register_math.h, and restated in fp64 numpy by tests/tanks_fscore_oracle.py:

1. ``crop``: Open3D's SelectionPolygonVolume (an axis range and an even-odd polygon test) on the optionally transformed points.
2. ``voxel_down_sample``: one point per occupied voxel of edge ``voxel`` (lattice origin = the cloud's minimum - voxel / 2), the
   fp64 mean of the voxel's points added in input order, voxels in ascending (kz, ky, kx) order.
3. ``icp``: Open3D's registration_icp loop (point to point, with scaling); every evaluation is one ``rcmvs_pc_icp_step`` whose 18
   fp64 moments are the only thing the host reads per iteration; the update is Umeyama's closed form on the host.
4. ``register``: the toolbox's three refinement rounds; ``evaluate``: the score and the two cumulative curves.

Known differences from the toolbox are listed in DESIGN.md (no RANSAC in the trajectory alignment, no normals, fp32 clouds).
CUDA tensors only; no CPU fallback.  ``python -m rc_mvsnet_amd.tanks_fscore --plydir OUT --gtpath trainingdata`` scores
``<plydir>/<scene>.ply`` against ``<gtpath>/<scene>/``.
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

from . import _lib, dtu_eval
from .ops import _chk, _stream

BLOCK, SCAN_TILE = 256, _lib.CONSTANTS["RCMVS_PC_SCAN_TILE"]        # csrc/pc_register.hip
MAX_POLYGON = _lib.CONSTANTS["RCMVS_PC_MAX_POLYGON"]
MAX_VOXELS_PER_AXIS = _lib.CONSTANTS["RCMVS_PC_MAX_VOXELS_PER_AXIS"]
ICP_BLOCKS, ICP_MOMENTS = _lib.CONSTANTS["RCMVS_PC_ICP_BLOCKS"], _lib.CONSTANTS["RCMVS_PC_ICP_MOMENTS"]
HIST_MAX_BINS = _lib.CONSTANTS["RCMVS_PC_HIST_MAX_BINS"]
MAX_POSES = 1600                                   # beyond it the toolbox resamples a video log (out of scope)
# the benchmark's per-scene distance threshold (python_toolbox/evaluation/config.py: scenes_tau_dict), training scenes
SCENE_TAU = {"Barn": 0.01, "Caterpillar": 0.005, "Church": 0.025, "Courthouse": 0.025, "Ignatius": 0.003, "Meetingroom": 0.01,
             "Truck": 0.005}


def _cdiv(a, b):
    return (a + b - 1) // b


_points, _bbox, _Grid = dtu_eval._points, dtu_eval.bbox, dtu_eval.Grid


def _matrix(T, name):
    T = np.asarray(T, dtype=np.float64)
    if T.shape != (4, 4) or not np.isfinite(T).all():
        raise _lib.RcmvsError(f"{name}: expected a finite 4x4 matrix, got shape {T.shape}")
    return np.ascontiguousarray(T)


# ---- readers ----------------------------------------------------------------------------------------------------------
def make_volume(axis, axis_min, axis_max, polygon):
    """A crop volume: axis 0 / 1 / 2 (or "X" / "Y" / "Z"), the range along it, polygon (m,2) = the (u, v) vertices in the plane of
    the two other axes (in axis order) or (m,3) xyz vertices."""
    if isinstance(axis, str):
        if axis.upper() not in ("X", "Y", "Z"):
            raise _lib.RcmvsError(f"crop volume: orthogonal_axis {axis!r} (X, Y or Z)")
        axis = "XYZ".index(axis.upper())
    if axis not in (0, 1, 2):
        raise _lib.RcmvsError(f"crop volume: orthogonal axis {axis!r} (0, 1 or 2)")
    poly = np.asarray(polygon, dtype=np.float64)
    if poly.ndim == 2 and poly.shape[1] == 3:
        poly = poly[:, [a for a in range(3) if a != axis]]
    if poly.ndim != 2 or poly.shape[1] != 2 or len(poly) < 3 or not np.isfinite(poly).all():
        raise _lib.RcmvsError(f"crop volume: bounding_polygon must be at least 3 finite vertices, got shape {poly.shape}")
    if len(poly) > MAX_POLYGON:
        raise _lib.RcmvsError(f"crop volume: polygon of {len(poly)} vertices (at most {MAX_POLYGON})")
    lo, hi = float(axis_min), float(axis_max)
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise _lib.RcmvsError(f"crop volume: axis range {lo} .. {hi}")
    return {"axis": int(axis), "axis_min": lo, "axis_max": hi, "polygon": np.ascontiguousarray(poly)}


def read_crop_json(path):
    """Open3D's SelectionPolygonVolume JSON (<scene>.json) -> a crop volume (make_volume)."""
    try:
        with open(path) as f:
            j = json.load(f)
    except (OSError, ValueError) as e:
        raise _lib.RcmvsError(f"{path}: not a readable JSON file ({e})") from None
    if not isinstance(j, dict):
        raise _lib.RcmvsError(f"{path}: expected a JSON object")
    for k in ("axis_max", "axis_min", "bounding_polygon", "orthogonal_axis"):
        if k not in j:
            raise _lib.RcmvsError(f"{path}: no key {k!r}")
    try:
        poly = np.asarray(j["bounding_polygon"], dtype=np.float64)
        if poly.ndim != 2 or poly.shape[1] != 3:
            raise ValueError(f"bounding_polygon of shape {poly.shape}: a list of xyz triples expected")
        if not isinstance(j["orthogonal_axis"], str):
            raise ValueError(f"orthogonal_axis {j['orthogonal_axis']!r}")
        return make_volume(j["orthogonal_axis"], j["axis_min"], j["axis_max"], poly)
    except (TypeError, ValueError, _lib.RcmvsError) as e:
        raise _lib.RcmvsError(f"{path}: {e}") from None


def read_trajectory_log(path):
    """A .log camera trajectory -> (n,4,4) fp64 camera-to-world matrices: per camera one metadata line of three integers, then
    the four rows of the matrix."""
    try:
        with open(path) as f:
            lines = [ln.split() for ln in f if ln.strip()]
    except OSError as e:
        raise _lib.RcmvsError(f"{path}: {e}") from None
    if not lines or len(lines) % 5:
        raise _lib.RcmvsError(f"{path}: {len(lines)} non-empty lines (five per camera expected)")
    poses = np.empty((len(lines) // 5, 4, 4), dtype=np.float64)
    for c in range(len(poses)):
        meta, rows = lines[5 * c], lines[5 * c + 1:5 * c + 5]
        try:
            if len(meta) != 3:
                raise ValueError("metadata")
            [int(v) for v in meta]
            if any(len(r) != 4 for r in rows):
                raise ValueError("row")
            poses[c] = [[float(v) for v in r] for r in rows]
        except ValueError:
            raise _lib.RcmvsError(f"{path}: camera {c}: expected a line of three integers and four rows of four numbers") from None
    if not np.isfinite(poses).all():
        raise _lib.RcmvsError(f"{path}: non-finite matrix entries")
    return poses


def read_alignment(path):
    """<scene>_trans.txt -> (4,4) fp64."""
    try:
        T = np.loadtxt(path, dtype=np.float64)
    except (OSError, ValueError) as e:
        raise _lib.RcmvsError(f"{path}: not a readable matrix ({e})") from None
    if T.shape != (4, 4) or not np.isfinite(T).all():
        raise _lib.RcmvsError(f"{path}: expected a finite 4x4 matrix, got shape {T.shape}")
    return T


# ---- host alignment ---------------------------------------------------------------------------------------------------
def _umeyama(n, mu_s, mu_d, cov, var_s, with_scaling):
    """cov[a][b] = mean (s_a - mu_s_a)(d_b - mu_d_b), var_s = mean |s - mu_s|^2 -> 4x4 with d ~ c R s + t (Umeyama 1991)"""
    U, D, Vt = np.linalg.svd(cov.T)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    c = float(np.trace(np.diag(D) @ S) / var_s) if with_scaling else 1.0
    T = np.eye(4)
    T[:3, :3] = c * R
    T[:3, 3] = mu_d - c * (R @ mu_s)
    return T


def umeyama(src, dst, with_scaling=True):
    """The similarity (4x4 fp64) that maps src (n,3) onto dst (n,3) in the least-squares sense: numpy svd with the det < 0
    reflection fix, scale = trace(D S) / var(src)."""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    if src.ndim != 2 or src.shape[1] != 3 or src.shape != dst.shape or len(src) < 3:
        raise _lib.RcmvsError(f"umeyama: two (n,3) arrays with n >= 3 expected, got {src.shape} and {dst.shape}")
    n = len(src)
    mu_s, mu_d = src.mean(0), dst.mean(0)
    cov = (src - mu_s).T @ (dst - mu_d) / n
    var_s = float(((src - mu_s) ** 2).sum() / n)
    return _umeyama(n, mu_s, mu_d, cov, var_s, with_scaling)


def umeyama_from_moments(mom, with_scaling=True):
    """umeyama from rcmvs_pc_icp_step's 18 moments {count, sum d^2, sum s, sum t, sum s t^T, sum |s|^2}."""
    mom = np.asarray(mom, dtype=np.float64)
    n = mom[0]
    mu_s, mu_d = mom[2:5] / n, mom[5:8] / n
    cov = mom[8:17].reshape(3, 3) / n - np.outer(mu_s, mu_d)
    var_s = mom[17] / n - float(mu_s @ mu_s)
    return _umeyama(n, mu_s, mu_d, cov, var_s, with_scaling)


def trajectory_alignment(traj_est, traj_gt, gt_trans):
    """The toolbox's trajectory alignment without its RANSAC: the Umeyama fit (with scale) of the estimated camera centres to the
    gt_trans-transformed ground-truth centres, every camera a correspondence.  traj_*: (n,4,4) camera-to-world."""
    traj_est, traj_gt = np.asarray(traj_est, dtype=np.float64), np.asarray(traj_gt, dtype=np.float64)
    gt_trans = _matrix(gt_trans, "gt_trans")
    if traj_est.ndim != 3 or traj_est.shape[1:] != (4, 4) or traj_est.shape != traj_gt.shape:
        raise _lib.RcmvsError(f"trajectory_alignment: two (n,4,4) trajectories of one length expected, got {traj_est.shape} and {traj_gt.shape}")
    if len(traj_est) > MAX_POSES:
        raise _lib.RcmvsError(f"trajectory_alignment: {len(traj_est)} poses (at most {MAX_POSES}: the toolbox's video-log resampling is not provided)")
    if len(traj_est) < 3:
        raise _lib.RcmvsError(f"trajectory_alignment: {len(traj_est)} poses (at least 3)")
    src = traj_est[:, :3, 3]
    dst = (traj_gt[:, :, 3] @ gt_trans.T)[:, :3]
    return umeyama(src, dst, with_scaling=True)


# ---- device functions -------------------------------------------------------------------------------------------------
def transform_points(pts, T):
    """(n,3) fp32 -> T applied in fp64 as ((T0 x + T1 y) + T2 z) + T3 per row, rounded to fp32 once (elementwise: plumbing)."""
    T = _matrix(T, "transform")
    p = pts.to(torch.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return torch.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], 1).to(torch.float32).contiguous()


def crop(pts, volume, transform=None):
    """-> (flags (n,) bool, kept (k,3) fp32): the points, transformed first when a 4x4 is given (fp64, rounded to fp32 once), that
    lie inside the crop volume, in input order."""
    n = _points(pts, "pts")
    dev = pts.device
    if n == 0:
        return torch.zeros(0, device=dev, dtype=torch.bool), pts
    poly = np.ascontiguousarray(volume["polygon"], dtype=np.float64)
    m = len(poly)
    if not 3 <= m <= MAX_POLYGON:
        raise _lib.RcmvsError(f"crop: polygon of {m} vertices (3 .. {MAX_POLYGON})")
    T = None if transform is None else _matrix(transform, "transform")
    nblk = _cdiv(n, BLOCK)
    work = torch.empty(2 * nblk + 1 + _cdiv(nblk, SCAN_TILE) + 1, device=dev, dtype=torch.int32)
    flags = torch.empty(n, device=dev, dtype=torch.uint8)
    kept = torch.empty((n, 3), device=dev, dtype=torch.float32)
    _lib.call("rcmvs_pc_crop", _chk(pts, "pts"), n, None if T is None else T.ctypes.data_as(ctypes.c_void_p), int(volume["axis"]),
              float(volume["axis_min"]), float(volume["axis_max"]), poly.ctypes.data_as(ctypes.c_void_p), m,
              _chk(flags, "flags", torch.uint8), _chk(kept, "kept"), _chk(work, "work", torch.int32), _stream())
    k = int(work[2 * nblk])
    return flags.bool(), kept[:k]


def voxel_down_sample(pts, voxel):
    """One point per occupied voxel of edge ``voxel``: the fp64 mean of its points added in input order (rounded to fp32 once), in
    ascending (kz, ky, kx) order; the lattice starts at the cloud's minimum - voxel / 2.  Two runs give identical bits."""
    voxel = float(voxel)
    if not (voxel > 0 and math.isfinite(voxel)):
        raise _lib.RcmvsError(f"voxel_down_sample: voxel {voxel}")
    n = _points(pts, "pts")
    if n == 0:
        return pts
    if n > (1 << 31) - 256:
        raise _lib.RcmvsError(f"voxel_down_sample: {n} points (at most 2^31 - 256)")
    dev = pts.device
    lo, hi = _bbox(pts)
    org = lo.astype(np.float64) - voxel / 2
    dims = np.floor((hi.astype(np.float64) - org) / voxel) + 1.0
    if not np.isfinite(dims).all() or dims.max() > MAX_VOXELS_PER_AXIS:
        raise _lib.RcmvsError(f"voxel_down_sample: {dims.max():.0f} voxels on an axis (at most 2^21): voxel {voxel} is too small for the cloud's extent")
    lattice = (ctypes.c_double * 4)(*org.tolist(), voxel)
    gdims = (ctypes.c_longlong * 3)(*[int(d) for d in dims])
    nblk = _cdiv(n, BLOCK)
    key = [torch.empty(n, device=dev, dtype=torch.int64) for _ in range(2)]
    idx = [torch.empty(n, device=dev, dtype=torch.int32) for _ in range(2)]
    hist = torch.empty(256 * nblk, device=dev, dtype=torch.int32)
    hist_start = torch.empty(256 * nblk + 1, device=dev, dtype=torch.int32)
    scan_work = torch.empty(_cdiv(max(256 * nblk, n), SCAN_TILE) + 1, device=dev, dtype=torch.int32)
    head = torch.empty(n, device=dev, dtype=torch.int32)
    head_start = torch.empty(n + 1, device=dev, dtype=torch.int32)
    _lib.call("rcmvs_pc_voxel_sort", _chk(pts, "pts"), n, ctypes.cast(lattice, ctypes.c_void_p), ctypes.cast(gdims, ctypes.c_void_p),
              _chk(key[0], "key_a", torch.int64), _chk(idx[0], "idx_a", torch.int32), _chk(key[1], "key_b", torch.int64),
              _chk(idx[1], "idx_b", torch.int32), _chk(hist, "hist", torch.int32), _chk(hist_start, "hist_start", torch.int32),
              _chk(scan_work, "scan_work", torch.int32), _chk(head, "head", torch.int32), _chk(head_start, "head_start", torch.int32),
              _stream())
    m = int(head_start[n])                                      # the one host synchronisation
    out = torch.empty((m, 3), device=dev, dtype=torch.float32)
    _lib.call("rcmvs_pc_voxel_emit", _chk(pts, "pts"), n, _chk(key[0], "key", torch.int64), _chk(idx[0], "idx", torch.int32),
              _chk(head_start, "head_start", torch.int32), m, _chk(out, "out"), _stream())
    return out


def uniform_down_sample(pts, every_k):
    """Open3D's uniform_down_sample: every every_k-th point from the first (strided slicing: plumbing)."""
    every_k = int(every_k)
    if every_k < 1:
        raise _lib.RcmvsError(f"uniform_down_sample: every_k {every_k}")
    return pts[::every_k].contiguous()


class IcpTarget:
    """The target cloud of icp_step in a grid whose cell edge is about max_dist (at least the edge a point per cell gives)."""

    def __init__(self, target, max_dist):
        n = _points(target, "target")
        if n == 0:
            raise _lib.RcmvsError("IcpTarget: empty cloud")
        self.n = n
        self.grid = _Grid(target, h_min=1e-6 * float(max_dist))
        self.part = torch.empty(ICP_MOMENTS * ICP_BLOCKS, device=target.device, dtype=torch.float64)


def icp_step(source, target, T, max_dist, want_corr=False):
    """One evaluation: -> (18 moments as a numpy fp64 vector, corr (n,) int32 on the device or None).  target: an IcpTarget."""
    n = _points(source, "source")
    if n == 0:
        raise _lib.RcmvsError("icp_step: empty source")
    if not (max_dist > 0 and math.isfinite(max_dist)):
        raise _lib.RcmvsError(f"icp_step: max_dist {max_dist}")
    T = _matrix(T, "transform")
    g = target.grid
    dev = source.device
    corr = torch.empty(n, device=dev, dtype=torch.int32) if want_corr else None
    out = torch.empty(ICP_MOMENTS, device=dev, dtype=torch.float64)
    _lib.call("rcmvs_pc_icp_step", _chk(source, "source"), n, T.ctypes.data_as(ctypes.c_void_p), ctypes.cast(g._g, ctypes.c_void_p),
              ctypes.cast(g._d, ctypes.c_void_p), _chk(g.cell_start, "cell_start", torch.int32), _chk(g.sorted, "sorted"),
              _chk(g.sorted_idx, "sorted_idx", torch.int32), target.n, float(max_dist),
              None if corr is None else _chk(corr, "corr", torch.int32), _chk(target.part, "part", torch.float64),
              _chk(out, "out", torch.float64), _stream())
    return out.cpu().numpy(), corr


def _fitness_rmse(mom, n):
    return mom[0] / n, (math.sqrt(mom[1] / mom[0]) if mom[0] > 0 else 0.0)


def icp(source, target, max_dist, init, max_iter=20, with_scaling=True, rel_fitness=1e-6, rel_rmse=1e-6):
    """Open3D's registration_icp loop (point to point): evaluate at T; per iteration the Umeyama update from the moments of the
    current correspondences, T <- update T, re-evaluate, stop when |d fitness| < rel_fitness and |d rmse| < rel_rmse or at
    max_iter; fewer than 3 correspondences stop with the current T.  -> {transformation (4,4) numpy fp64, fitness, inlier_rmse,
    iterations}.  The host reads 18 doubles per evaluation: the only synchronisation."""
    T = _matrix(init, "init").copy()
    n = _points(source, "source")
    tgt = target if isinstance(target, IcpTarget) else IcpTarget(target, max_dist)
    mom, _ = icp_step(source, tgt, T, max_dist)
    fitness, rmse = _fitness_rmse(mom, n)
    iterations = 0
    for _ in range(int(max_iter)):
        if mom[0] < 3:
            break
        T = umeyama_from_moments(mom, with_scaling) @ T
        mom, _ = icp_step(source, tgt, T, max_dist)
        f2, r2 = _fitness_rmse(mom, n)
        iterations += 1
        done = abs(f2 - fitness) < rel_fitness and abs(r2 - rmse) < rel_rmse
        fitness, rmse = f2, r2
        if done:
            break
    return {"transformation": T, "fitness": float(fitness), "inlier_rmse": float(rmse), "iterations": iterations}


# ---- registration and scoring -------------------------------------------------------------------------------------------
def register(est, gt, init, volume, tau, max_iter=20):
    """The toolbox's three refinement rounds (voxel tau / threshold 80 tau, voxel tau / 2 / threshold 20 tau, uniform
    down-sample to about 4 M points / threshold 2 tau), each an icp with scaling from the previous round's T.  In a round the
    estimate is transformed by T, cropped, down-sampled and mapped back by T^-1; the ground truth is cropped and down-sampled.
    -> (T (4,4) numpy fp64, [per round icp result])."""
    T = _matrix(init, "init").copy()
    tau = float(tau)
    _, gt_c = crop(gt, volume)
    rounds = []
    for voxel, thr in ((tau, 80.0 * tau), (tau / 2.0, 20.0 * tau), (None, 2.0 * tau)):
        _, est_c = crop(est, volume, T)
        if len(est_c) == 0 or len(gt_c) == 0:
            break
        if voxel is None:
            s = uniform_down_sample(est_c, max(1, len(est_c) // 4_000_000))
            t = uniform_down_sample(gt_c, max(1, len(gt_c) // 4_000_000))
        else:
            s, t = voxel_down_sample(est_c, voxel), voxel_down_sample(gt_c, voxel)
        r = icp(transform_points(s, np.linalg.inv(T)), t, thr, T, max_iter=max_iter, with_scaling=True)
        T = r["transformation"]
        rounds.append(r)
    return T, rounds


def dist_hist(d, tau, nbins, w):
    """-> (counts (nbins,) numpy uint64 with counts[b] = #(floor(d / w) == b), #(d < tau)) of fp64 device distances."""
    n = d.numel()
    if n == 0:
        return np.zeros(nbins, dtype=np.uint64), 0
    if not 1 <= nbins <= HIST_MAX_BINS:
        raise _lib.RcmvsError(f"dist_hist: {nbins} bins (1 .. {HIST_MAX_BINS})")
    out = torch.empty(nbins + 1, device=d.device, dtype=torch.int64)
    _lib.call("rcmvs_pc_dist_hist", _chk(d, "d", torch.float64), n, float(tau), int(nbins), float(w), _chk(out[:nbins], "counts", torch.int64),
              _chk(out[nbins:], "below", torch.int64), _stream())
    o = out.cpu().numpy()
    return o[:nbins].astype(np.uint64), int(o[nbins])


def evaluate(est, gt, T, volume, tau, stretch=5, down_sample=True):
    """-> {precision, recall, fscore, n_est, n_gt, hist_est, hist_gt (numpy uint64, bin width tau / 100, 100 stretch - 1 bins),
    curve_est, curve_gt (their cumulative fractions)}.  The estimate is transformed by T, both clouds are cropped and voxel
    down-sampled at tau / 2 (down_sample=False: scored as cropped), distances are capped at stretch tau.  An empty cropped cloud
    gives zeros."""
    tau = float(tau)
    nbins, w = 100 * int(stretch) - 1, tau / 100.0
    _, e = crop(est, volume, T)
    _, g = crop(gt, volume)
    zero = np.zeros(nbins, dtype=np.uint64)
    if len(e) == 0 or len(g) == 0:
        return {"precision": 0.0, "recall": 0.0, "fscore": 0.0, "n_est": int(len(e)), "n_gt": int(len(g)), "hist_est": zero, "hist_gt": zero.copy(),
                "curve_est": np.zeros(nbins), "curve_gt": np.zeros(nbins)}
    if down_sample:
        e, g = voxel_down_sample(e, tau / 2.0), voxel_down_sample(g, tau / 2.0)
    cap = stretch * tau
    he, be = dist_hist(dtu_eval.nearest_distances(e, g, cap=cap), tau, nbins, w)
    hg, bg = dist_hist(dtu_eval.nearest_distances(g, e, cap=cap), tau, nbins, w)
    P, R = be / len(e), bg / len(g)
    F = 2.0 * P * R / (P + R) if P + R > 0 else 0.0
    return {"precision": P, "recall": R, "fscore": F, "n_est": int(len(e)), "n_gt": int(len(g)), "hist_est": he, "hist_gt": hg,
            "curve_est": np.cumsum(he) / len(e), "curve_gt": np.cumsum(hg) / len(g)}


# ---- files and command line -------------------------------------------------------------------------------------------
def scene_paths(plydir, gtpath, scene):
    d = os.path.join(gtpath, scene)
    return {"est": os.path.join(plydir, f"{scene}.ply"), "gt": os.path.join(d, f"{scene}.ply"), "crop": os.path.join(d, f"{scene}.json"),
            "trans": os.path.join(d, f"{scene}_trans.txt"), "log": os.path.join(d, f"{scene}_COLMAP_SfM.log")}


def evaluate_files(plydir, gtpath, scene, device="cuda:0", traj=None, do_register=True, tau=None, curves=None):
    """Score <plydir>/<scene>.ply against <gtpath>/<scene>/ -> the JSON-ready result of one scene.  traj: the estimate's camera
    log (default: the scene's COLMAP log, which the MVSNet-style methods reconstruct from); curves: a folder for
    <scene>.precision.npy / <scene>.recall.npy."""
    from .dtu_io import read_ply_xyz
    if tau is None:
        if scene not in SCENE_TAU:
            raise _lib.RcmvsError(f"{scene}: no tau for this scene (known: {', '.join(SCENE_TAU)}); pass one")
        tau = SCENE_TAU[scene]
    p = scene_paths(plydir, gtpath, scene)
    dev = torch.device(device)
    volume = read_crop_json(p["crop"])
    gt_trans = read_alignment(p["trans"])
    traj_gt = read_trajectory_log(p["log"])
    traj_est = traj_gt if traj is None else read_trajectory_log(traj)
    T = trajectory_alignment(traj_est, traj_gt, gt_trans)
    est = torch.from_numpy(read_ply_xyz(p["est"])).to(dev)
    gt = torch.from_numpy(read_ply_xyz(p["gt"])).to(dev)
    rounds = []
    if do_register:
        T, rounds = register(est, gt, T, volume, tau)
    r = evaluate(est, gt, T, volume, tau)
    if curves is not None:
        os.makedirs(curves, exist_ok=True)
        np.save(os.path.join(curves, f"{scene}.precision.npy"), r["curve_est"])
        np.save(os.path.join(curves, f"{scene}.recall.npy"), r["curve_gt"])
    return {"scene": scene, "tau": float(tau), "precision": r["precision"], "recall": r["recall"], "fscore": r["fscore"],
            "n_est": r["n_est"], "n_gt": r["n_gt"], "icp": [{k: v for k, v in rd.items() if k != "transformation"} for rd in rounds]}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Tanks and Temples precision / recall / F-score of fused point clouds, on the GPU")
    ap.add_argument("--plydir", required=True, help="folder of the estimates <scene>.ply (eval_driver --dataset tanks writes them)")
    ap.add_argument("--gtpath", required=True, help="the benchmark's training data: <scene>/<scene>.ply, .json, _trans.txt, _COLMAP_SfM.log")
    ap.add_argument("--scenes", default=",".join(SCENE_TAU), help="comma-separated scene names (default: the seven training scenes)")
    ap.add_argument("--traj", default=None, help="camera log of the estimate (default: the scene's COLMAP log); one scene only")
    ap.add_argument("--no-register", action="store_true", help="skip the three ICP rounds: score with the trajectory alignment alone")
    ap.add_argument("--curves", default=None, metavar="DIR", help="write the cumulative curves <scene>.precision.npy / .recall.npy into DIR")
    ap.add_argument("--gpus", type=int, default=1, help="GPUs of this node: scenes are sharded one process per GPU, no collective")
    ap.add_argument("--results-dir", default=None, help=argparse.SUPPRESS)      # ranks' results for the parent's summary
    args = ap.parse_args(argv)
    args.scenes = [s.strip() for s in args.scenes.split(",") if s.strip()]
    unknown = [s for s in args.scenes if s not in SCENE_TAU]
    if unknown:
        ap.error(f"--scenes: no tau for {', '.join(unknown)} (known: {', '.join(SCENE_TAU)})")
    if args.traj is not None and len(args.scenes) != 1:
        ap.error("--traj names one scene's log: give that scene with --scenes")
    if args.gpus < 1:
        ap.error("--gpus must be at least 1")
    return args


def summarize(results):
    return {"summary": True, "scenes": len(results), "mean_fscore": float(np.mean([r["fscore"] for r in results]))}


def main(argv=None):
    args = parse_args(argv)
    argv = sys.argv[1:] if argv is None else list(argv)
    scenes = args.scenes
    from .sharding import launch_ranks, launched, rank_env, shard_items
    if args.gpus > 1 and not launched():
        with tempfile.TemporaryDirectory() as tmp:
            rc = launch_ranks("rc_mvsnet_amd.tanks_fscore", args.gpus, argv + ["--results-dir", tmp], module=True)
            if rc:
                raise SystemExit(rc)
            results = []
            for name in sorted(os.listdir(tmp)):
                with open(os.path.join(tmp, name)) as f:
                    results += json.load(f)
        results.sort(key=lambda r: scenes.index(r["scene"]))
        if results:
            print(json.dumps(summarize(results)), flush=True)
        return results
    rank, local, world = rank_env()
    if not torch.cuda.is_available():
        raise SystemExit("tanks_fscore: needs a GPU (the scorer has no CPU fallback)")
    device = "cuda:%d" % local
    torch.cuda.set_device(device)
    _lib.load()
    results = []
    for scene in shard_items(scenes, rank, world):
        r = evaluate_files(args.plydir, args.gtpath, scene, device=device, traj=args.traj, do_register=not args.no_register, curves=args.curves)
        results.append(r)
        print(json.dumps(r), flush=True)
    if args.results_dir:
        with open(os.path.join(args.results_dir, f"rank{rank:04d}.json"), "w") as f:
            json.dump(results, f)
    elif world == 1 and results:
        print(json.dumps(summarize(results)), flush=True)
    return results


if __name__ == "__main__":
    main()
