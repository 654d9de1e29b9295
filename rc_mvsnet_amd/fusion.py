"""Depth-map fusion filter on the HIP path.

Same entry points as the reference's evaluation script (eval_rcmvsnet_dtu.py:281-446; eval_rcmvsnet_tanks.py:206-382 is the
same code): ``check_geometric_consistency`` for one pair of views and ``filter_depth`` for a scan laid out on disk
(pair.txt, cams/, images/, depth_est/*.pfm, confidence/*.pfm -> mask/*.png and one fused .ply).  The reference runs this
on the CPU, a ``multiprocessing.Pool`` of one process per scan, ~40 numpy passes per (reference, source) pair; here every
depth map of the scan is uploaded ONCE and stays in HBM, a reference view is one kernel over all of its source views
(``rcmvs_fuse_view``) plus an ordered compaction of the surviving points (``rcmvs_compact_points``), and scans shard over
GPUs with no collective (``filter_scans``).  No CPU fallback: without a GPU / the built library these functions raise.
"""
import ctypes
import os

import numpy as np
import torch
from PIL import Image

from . import _lib, scan_io
from .data_io import read_pfm
from .ops import _chk, _stream

MAX_SRC = _lib.CONSTANTS["RCMVS_FUSE_MAX_SRC"]
REF_MATS, SRC_MATS = 30, 42


def fusion_matrices(K_ref, E_ref, src_K, src_E):
    """The matrices of rcmvs_fuse_view as one float64 vector (30 + 42 N).  Inverses and products are taken in the dtype the
    reference has them in (float32 camera files -> float32 np.linalg.inv / np.matmul, eval_rcmvsnet_dtu.py:289-313) and only
    then promoted, so the per-pixel chain sees the same numbers."""
    K_ref, E_ref = np.asarray(K_ref), np.asarray(E_ref)
    E_ref_inv = np.linalg.inv(E_ref)
    out = [np.linalg.inv(K_ref).ravel(), K_ref.ravel(), E_ref_inv[:3, :4].ravel()]
    for K, E in zip(src_K, src_E):
        K, E = np.asarray(K), np.asarray(E)
        out += [np.matmul(E, E_ref_inv)[:3, :4].ravel(), K.ravel(), np.linalg.inv(K).ravel(),
                np.matmul(E_ref, np.linalg.inv(E))[:3, :4].ravel()]
    return np.concatenate([o.astype(np.float64) for o in out])


def _ptr(t, name, dtype):
    return ctypes.c_void_p(0) if t is None else _chk(t, name, dtype)


def fuse_view(depth_all, ref_idx, src_idx, conf, img, mats, prob_threshold, num_consistent, img_dist_thresh, depth_thresh, debug=False):
    """Device tensors in, device tensors out.  depth_all (n_views,H,W) fp32, conf (H,W) fp32, img (H,W,3) fp32 in [0,1] or
    None, mats float64 (30 + 42 N).  Returns dict: masks (3,H,W) uint8 [photo, geo, final], depth_avg (H,W), xyz (H,W,3),
    rgb (H,W,3) uint8 or None, and with debug=True depth_reprojected (N,H,W), geo (N,H,W) uint8, xy_src (N,H,W,2)."""
    N = len(src_idx)
    if not 1 <= N <= MAX_SRC:
        raise _lib.RcmvsError(f"fuse_view: {N} source views (1..{MAX_SRC})")
    n_views, H, W = depth_all.shape
    if max([ref_idx] + list(src_idx)) >= n_views:
        raise _lib.RcmvsError("fuse_view: view index beyond depth_all")
    if mats.numel() != REF_MATS + SRC_MATS * N:
        raise _lib.RcmvsError(f"fuse_view: mats has {mats.numel()} values, expected {REF_MATS + SRC_MATS * N}")
    dev = depth_all.device
    masks = torch.empty((3, H, W), device=dev, dtype=torch.uint8)
    depth_avg = torch.empty((H, W), device=dev, dtype=torch.float32)
    xyz = torch.empty((H, W, 3), device=dev, dtype=torch.float32)
    rgb = torch.empty((H, W, 3), device=dev, dtype=torch.uint8) if img is not None else None
    dbg_d = torch.empty((N, H, W), device=dev, dtype=torch.float32) if debug else None
    dbg_g = torch.empty((N, H, W), device=dev, dtype=torch.uint8) if debug else None
    dbg_xy = torch.empty((N, H, W, 2), device=dev, dtype=torch.float32) if debug else None
    idx = (ctypes.c_int * N)(*[int(i) for i in src_idx])
    _lib.call("rcmvs_fuse_view",
        _chk(depth_all, "depth_all"), int(ref_idx), ctypes.cast(idx, ctypes.c_void_p), _chk(conf, "conf"), _ptr(img, "img", torch.float32),
        _chk(mats, "mats", torch.float64), float(prob_threshold), int(num_consistent), float(img_dist_thresh), float(depth_thresh),
        _chk(masks, "masks", torch.uint8), _chk(depth_avg, "depth_avg"), _chk(xyz, "xyz"), _ptr(rgb, "rgb", torch.uint8),
        _ptr(dbg_d, "dbg_depth", torch.float32), _ptr(dbg_g, "dbg_geo", torch.uint8), _ptr(dbg_xy, "dbg_xy", torch.float32),
        N, H, W, _stream())
    out = {"masks": masks, "depth_avg": depth_avg, "xyz": xyz, "rgb": rgb}
    if debug:
        out.update({"depth_reprojected": dbg_d, "geo": dbg_g, "xy_src": dbg_xy})
    return out


METHODS = ("reference", "dynamic")
DYN_DEFAULTS = {"level_lo": 2, "level_hi": None, "dist_base": 0.25, "rel_base": 1.0 / 1300.0}      # the common published form of the dynamic check


def dynamic_params(dynamic, n_src):
    """The four parameters of the dynamic check for a view with ``n_src`` sources: DYN_DEFAULTS overridden by ``dynamic`` (a dict,
    unknown keys refused).  level_hi None means "as many levels as there are sources", but never fewer than level_lo: with one
    source and level_lo = 2 the only level is 2, which one source cannot reach, so nothing is consistent."""
    p = dict(DYN_DEFAULTS)
    for k, v in (dynamic or {}).items():
        if k not in p:
            raise _lib.RcmvsError(f"dynamic fusion: unknown parameter {k!r} (known: {', '.join(DYN_DEFAULTS)})")
        p[k] = v
    p["level_lo"] = int(p["level_lo"])
    p["level_hi"] = max(int(n_src), p["level_lo"]) if p["level_hi"] is None else int(p["level_hi"])
    p["dist_base"], p["rel_base"] = float(p["dist_base"]), float(p["rel_base"])
    return p


def check_levels(level_lo, level_hi, what="fuse_view_dynamic"):
    if not 1 <= level_lo <= level_hi <= MAX_SRC:
        raise _lib.RcmvsError(f"{what}: levels {level_lo}..{level_hi} (1 <= lo <= hi <= {MAX_SRC})")


def fuse_view_dynamic(depth_all, ref_idx, src_idx, conf, img, mats, prob_threshold, level_lo=2, level_hi=None, dist_base=0.25,
                      rel_base=1.0 / 1300.0, used=None, debug=False):
    """fuse_view with the dynamic consistency check and, with ``used``, one point per surface (csrc/fusion_dyn.h has the rule).
    Source i passes level n when dist_i < n * dist_base (fp64, pixels) and rel_i < n * rel_base (fp32); a pixel's level is the
    smallest n in [level_lo, level_hi] that n sources pass, 0 for none, and geo = level != 0.  level_hi None: max(N, level_lo).
    used: (n_views,H,W) uint8 on the device, zero-filled by the caller ONCE PER SCAN, or None.  A kept pixel marks the pixel it
    falls on in every source that passes level_hi; a pixel whose own byte is already set is ``claimed`` and dropped.  Within one
    call nothing depends on the schedule, but the result DOES depend on the order in which the reference views of a scan are
    passed: that order is pair.txt's, and every launch goes on the one current stream.
    Returns dict: masks (4,H,W) uint8 [photo, geo, final, claimed], level (H,W) uint8, depth_avg (H,W), xyz (H,W,3), rgb (H,W,3)
    uint8 or None, and with debug=True depth_reprojected (N,H,W) (0 where the source fails level_hi), src_level (N,H,W) uint8,
    xy_src (N,H,W,2)."""
    N = len(src_idx)
    if not 1 <= N <= MAX_SRC:
        raise _lib.RcmvsError(f"fuse_view_dynamic: {N} source views (1..{MAX_SRC})")
    level_lo = int(level_lo)
    level_hi = max(N, level_lo) if level_hi is None else int(level_hi)
    check_levels(level_lo, level_hi)
    n_views, H, W = depth_all.shape
    if not all(0 <= int(i) < n_views for i in [ref_idx] + list(src_idx)):
        raise _lib.RcmvsError(f"fuse_view_dynamic: view index outside the {n_views} views of depth_all")
    if mats.numel() != REF_MATS + SRC_MATS * N:
        raise _lib.RcmvsError(f"fuse_view_dynamic: mats has {mats.numel()} values, expected {REF_MATS + SRC_MATS * N}")
    if used is not None and tuple(used.shape) != (n_views, H, W):
        raise _lib.RcmvsError(f"fuse_view_dynamic: used is {tuple(used.shape)}, expected {(n_views, H, W)}")
    dev = depth_all.device
    masks = torch.empty((4, H, W), device=dev, dtype=torch.uint8)
    level = torch.empty((H, W), device=dev, dtype=torch.uint8)
    depth_avg = torch.empty((H, W), device=dev, dtype=torch.float32)
    xyz = torch.empty((H, W, 3), device=dev, dtype=torch.float32)
    rgb = torch.empty((H, W, 3), device=dev, dtype=torch.uint8) if img is not None else None
    dbg_d = torch.empty((N, H, W), device=dev, dtype=torch.float32) if debug else None
    dbg_l = torch.empty((N, H, W), device=dev, dtype=torch.uint8) if debug else None
    dbg_xy = torch.empty((N, H, W, 2), device=dev, dtype=torch.float32) if debug else None
    idx = (ctypes.c_int * N)(*[int(i) for i in src_idx])
    _lib.call("rcmvs_fuse_view_dyn",
        _chk(depth_all, "depth_all"), int(n_views), int(ref_idx), ctypes.cast(idx, ctypes.c_void_p), _chk(conf, "conf"), _ptr(img, "img", torch.float32),
        _chk(mats, "mats", torch.float64), ctypes.c_float(prob_threshold), level_lo, level_hi, ctypes.c_double(dist_base), ctypes.c_float(rel_base),
        _ptr(used, "used", torch.uint8), _chk(masks, "masks", torch.uint8), _chk(level, "level", torch.uint8), _chk(depth_avg, "depth_avg"),
        _chk(xyz, "xyz"), _ptr(rgb, "rgb", torch.uint8), _ptr(dbg_d, "dbg_depth", torch.float32), _ptr(dbg_l, "dbg_level", torch.uint8),
        _ptr(dbg_xy, "dbg_xy", torch.float32), N, H, W, _stream())
    out = {"masks": masks, "level": level, "depth_avg": depth_avg, "xyz": xyz, "rgb": rgb}
    if debug:
        out.update({"depth_reprojected": dbg_d, "src_level": dbg_l, "xy_src": dbg_xy})
    return out


def reference_bases(num_consistent, img_dist_thresh, depth_thresh):
    """(dist_base, rel_base) at which level k = num_consistent of the dynamic check has EXACTLY the fixed filter's thresholds:
    (double)k * dist_base == img_dist_thresh and (float)k * rel_base == float32(depth_thresh) in every bit, so that
    level_lo = level_hi = k keeps the pixels rcmvs_fuse_view keeps and averages the same depths.  t / k times k does not always
    round back to t; the few neighbours of t / k are tried, and where none gives t the combination is refused."""
    k = int(num_consistent)
    if not 1 <= k <= MAX_SRC:
        raise _lib.RcmvsError(f"dedup with method='reference' runs the fixed check as level {k} of the dynamic kernel, which has levels 1..{MAX_SRC}")

    def base(t, ftype):
        t, kk = ftype(t), ftype(k)
        b = t / kk
        cands = [b]
        for towards in (ftype(-np.inf), ftype(np.inf)):
            c = b
            for _ in range(3):
                c = np.nextafter(c, towards)
                cands.append(c)
        for c in cands:
            if kk * c == t:
                return float(c)
        raise _lib.RcmvsError(f"dedup with method='reference': no {ftype.__name__} base b has {k} * b == {t!r} exactly, so the dynamic kernel "
                              "cannot restate the fixed thresholds bit for bit; use method='dynamic' or drop dedup")
    return base(img_dist_thresh, np.float64), base(depth_thresh, np.float32)


def add_fusion_arguments(ap, dedup=True):
    """The fusion options of the drivers (eval_driver, tsdf_mesh): every default is None / False, so that fusion_options can tell
    "not given" from a value."""
    ap.add_argument("--fusion", choices=METHODS, default=None,
                    help="the consistency check of the fusion filter: reference (default: fixed thresholds, --num_consistency views) or dynamic "
                         "(n views within n times the base thresholds, for some n of --dyn-levels; no per-scene tuning)")
    if dedup:
        ap.add_argument("--fusion-dedup", action="store_true",
                        help="one point per surface: a fused point marks the source pixels it accounts for and later reference views skip them")
    ap.add_argument("--dyn-levels", type=int, nargs=2, default=None, metavar=("LO", "HI"),
                    help=f"--fusion dynamic: the levels tried (default 2 and the number of source views; at most {MAX_SRC})")
    ap.add_argument("--dyn-dist-base", type=float, default=None, help="--fusion dynamic: reprojection distance of level 1 in pixels (default 0.25)")
    ap.add_argument("--dyn-rel-base", type=float, default=None, help="--fusion dynamic: relative depth difference of level 1 (default 1/1300)")
    note = " (the fused point cloud only: a mesh is fused from the depth maps, not from the cloud, and ignores this)"
    ap.add_argument("--cloud-radius", nargs=2, default=None, metavar=("R", "N"), help="keep the points with at least N others within R" + note)
    ap.add_argument("--cloud-stat", nargs=2, default=None, metavar=("K", "RATIO"),
                    help="keep the points whose mean distance to their K nearest neighbours is at most mu + RATIO sigma" + note)
    ap.add_argument("--cloud-normals", type=int, default=None, metavar="K",
                    help="write nx ny nz from the K nearest neighbours, oriented towards the view that produced the point" + note)


def cloud_options(args, who):
    """The parsed --cloud-radius / --cloud-stat / --cloud-normals -> the ``clean`` keyword of filter_depth / filter_depth_tanks (None when
    none was given, so that a run without them does what it did before); argument errors end the run with one line."""
    from . import cloud_clean
    try:
        radius = None if args.cloud_radius is None else (float(args.cloud_radius[0]), int(args.cloud_radius[1]))
        stat = None if args.cloud_stat is None else (int(args.cloud_stat[0]), float(args.cloud_stat[1]))
    except ValueError:
        raise SystemExit(f"{who}: --cloud-radius takes a number and an integer, --cloud-stat an integer and a number") from None
    if radius is not None and not (radius[0] >= 0 and radius[1] >= 0):
        raise SystemExit(f"{who}: --cloud-radius {radius[0]} {radius[1]}: R >= 0 and N >= 0")
    if stat is not None and not (1 <= stat[0] <= cloud_clean.MAX_K and stat[1] >= 0):
        raise SystemExit(f"{who}: --cloud-stat {stat[0]} {stat[1]}: 1 <= K <= {cloud_clean.MAX_K} and RATIO >= 0")
    if args.cloud_normals is not None and not 1 <= args.cloud_normals <= cloud_clean.MAX_K:
        raise SystemExit(f"{who}: --cloud-normals {args.cloud_normals}: 1 <= K <= {cloud_clean.MAX_K}")
    return cloud_clean.clean_options(radius, stat, args.cloud_normals)


def camera_centre(extrinsic):
    """-R^T t of a world-to-camera extrinsic (4,4), in fp64 on the host"""
    E = np.asarray(extrinsic, dtype=np.float64)
    return -(E[:3, :3].T @ E[:3, 3])


def _write_cloud(plyfilename, pts, cols, centres, clean, stats, dev, poisson=None):
    """The end of filter_depth / filter_depth_tanks: the per-view points concatenated, cleaned when ``clean`` asks for it (view = the
    position of the point's reference view in pair.txt, centres = those views' camera centres), and written -> (xyz, rgb) as written.
    poisson: the keywords of poisson_mesh.reconstruct; the cleaned cloud, still on the device, is meshed with them and written next to
    the cloud as <name>_poisson.ply (needs the normals of ``clean``)."""
    xyz, rgb = np.concatenate(pts, 0), np.concatenate(cols, 0)
    normals = None
    if clean:
        from . import cloud_clean
        view = np.repeat(np.arange(len(pts), dtype=np.int32), [len(p) for p in pts])
        r = cloud_clean.clean_cloud(torch.from_numpy(np.ascontiguousarray(xyz, np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(rgb, np.uint8)).to(dev),
                                    torch.from_numpy(view).to(dev), np.stack(centres) if centres else np.zeros((0, 3)), **clean)
        xyz, rgb = r["xyz"].cpu().numpy(), r["rgb"].cpu().numpy()
        normals = None if r["normals"] is None else r["normals"].cpu().numpy()
        if stats is not None:
            stats["cloud"] = r["stats"]
    if poisson is not None:
        if normals is None:
            raise _lib.RcmvsError("fusion: poisson needs oriented normals: give clean={'normals': K} (--cloud-normals K)")
        from . import poisson_mesh, tsdf_mesh
        verts, faces, col, pstats = poisson_mesh.reconstruct(r["xyz"], r["normals"], r["rgb"], **poisson)
        with open(os.path.splitext(plyfilename)[0] + "_poisson.ply", "wb") as f:
            f.write(tsdf_mesh.mesh_ply_bytes(verts, faces, col))
        if stats is not None:
            stats["poisson"] = pstats
    with open(plyfilename, "wb") as f:
        f.write(ply_bytes(xyz, rgb, normals))
    return xyz, rgb


def fusion_options(args, who):
    """The parsed fusion options -> the keywords filter_depth / filter_depth_tanks take for them ({} when none was given, so that a run
    without them calls what it called before); argument errors end the run with one line."""
    dyn = {k: v for k, v in (("levels", args.dyn_levels), ("dist_base", args.dyn_dist_base), ("rel_base", args.dyn_rel_base)) if v is not None}
    dedup = bool(getattr(args, "fusion_dedup", False))
    if args.fusion is None and not dedup and not dyn:
        return {}
    method = args.fusion or "reference"
    if dyn and method != "dynamic":
        raise SystemExit(f"{who}: --dyn-levels, --dyn-dist-base and --dyn-rel-base belong to --fusion dynamic")
    dynamic = None
    if method == "dynamic":
        dynamic = {k: dyn[k] for k in ("dist_base", "rel_base") if k in dyn}
        if "levels" in dyn:
            lo, hi = dyn["levels"]
            if not 1 <= lo <= hi <= MAX_SRC:
                raise SystemExit(f"{who}: --dyn-levels {lo} {hi}: 1 <= LO <= HI <= {MAX_SRC}")
            dynamic.update({"level_lo": lo, "level_hi": hi})
    return {"method": method, "dynamic": dynamic, "dedup": dedup}


def fusion_summary(options, stats, fixed=None):
    """what a driver's summary reports as "fusion": method, levels, bases, dedup, points and claimed.  fixed = (num_consistent,
    img_dist_thresh, depth_thresh) of the reference method."""
    if options["method"] == "dynamic":
        p = dict(DYN_DEFAULTS, **(options["dynamic"] or {}))
        levels, dist_base, rel_base = [p["level_lo"], p["level_hi"]], p["dist_base"], p["rel_base"]      # level_hi None: the number of source views
    else:
        levels = [int(fixed[0])] * 2
        k = int(fixed[0])                                           # without dedup the fixed thresholds are used as they are: bases for the record
        dist_base, rel_base = reference_bases(*fixed) if options["dedup"] else ((fixed[1] / k, fixed[2] / k) if k else (None, None))
    return {"method": options["method"], "levels": levels, "dist_base": dist_base, "rel_base": rel_base, "dedup": bool(options["dedup"]),
            "points": int(stats.get("kept", 0)), "claimed": int(stats.get("claimed", 0))}


def _fuse_dyn(depth_all, ref_slot, src_slots, conf, img, mats, prob, method, dynamic, fixed, used):
    """one reference view through rcmvs_fuse_view_dyn for filter_depth / filter_depth_tanks: -> (result dict, parameters used)"""
    if method == "dynamic":
        p = dynamic_params(dynamic, len(src_slots))
    else:                                                           # the fixed check restated as one level (dedup=True only)
        k, dist_t, depth_t = fixed
        db, rb = reference_bases(k, dist_t, depth_t)
        p = {"level_lo": int(k), "level_hi": int(k), "dist_base": db, "rel_base": rb}
    check_levels(p["level_lo"], p["level_hi"], "filter_depth")
    r = fuse_view_dynamic(depth_all, ref_slot, src_slots, conf, img, mats, prob, p["level_lo"], p["level_hi"], p["dist_base"], p["rel_base"], used=used)
    return r, p


def _check_method(method, dynamic, dedup):
    if method not in METHODS:
        raise _lib.RcmvsError(f"fusion method {method!r} (one of {', '.join(METHODS)})")
    if dynamic is not None and method != "dynamic":
        raise _lib.RcmvsError("the `dynamic` parameters apply to method='dynamic' only")
    return method == "reference" and not dedup                      # True: today's path, rcmvs_fuse_view


def _compact_counted(masks, xyz, rgb):
    """compact_points on masks[2] plus the number of claimed pixels (masks[3]), both fetched in the view's one host read"""
    mask = masks[2]
    n = mask.numel()
    dev = mask.device
    out_xyz = torch.empty((n, 3), device=dev, dtype=torch.float32)
    out_rgb = torch.empty((n, 3), device=dev, dtype=torch.uint8)
    offsets = torch.empty((n + 255) // 256 + 1, device=dev, dtype=torch.int32)
    _lib.call("rcmvs_compact_points", _chk(mask, "mask", torch.uint8), _chk(xyz, "xyz"), _chk(rgb, "rgb", torch.uint8),
              _chk(out_xyz, "out_xyz"), _chk(out_rgb, "out_rgb", torch.uint8), _chk(offsets, "offsets", torch.int32), n, _stream())
    kept, claimed = torch.stack([offsets[-1].to(torch.int64), masks[3].sum(dtype=torch.int64)]).tolist()
    return out_xyz[:kept], out_rgb[:kept], kept, claimed


def _stats_add(stats, ref, kept, claimed):
    if stats is not None:
        stats.setdefault("views", []).append({"ref": int(ref), "kept": int(kept), "claimed": int(claimed)})
        stats["kept"] = stats.get("kept", 0) + int(kept)
        stats["claimed"] = stats.get("claimed", 0) + int(claimed)


def compact_points(mask, xyz, rgb=None):
    """numpy's ``xyz[mask]`` / ``rgb[mask]`` on the device, row-major order kept.  mask (H,W) uint8 -> (n,3) fp32[, (n,3) uint8]."""
    n = mask.numel()
    dev = mask.device
    out_xyz = torch.empty((n, 3), device=dev, dtype=torch.float32)
    out_rgb = torch.empty((n, 3), device=dev, dtype=torch.uint8) if rgb is not None else None
    offsets = torch.empty((n + 255) // 256 + 1, device=dev, dtype=torch.int32)
    _lib.call("rcmvs_compact_points", _chk(mask, "mask", torch.uint8), _chk(xyz, "xyz"), _ptr(rgb, "rgb", torch.uint8),
              _chk(out_xyz, "out_xyz"), _ptr(out_rgb, "out_rgb", torch.uint8),
              _chk(offsets, "offsets", torch.int32), n, _stream())
    kept = int(offsets[-1])                                     # the one host synchronisation of a reference view
    return out_xyz[:kept], (out_rgb[:kept] if rgb is not None else None)


def check_geometric_consistency(depth_ref, intrinsics_ref, extrinsics_ref, depth_src, intrinsics_src, extrinsics_src,
                                img_dist_thresh, depth_thresh, device="cuda:0"):
    """eval_rcmvsnet_dtu.py:324-338 for one (reference, source) pair of numpy arrays:
    -> mask (H,W) bool, depth_reprojected (H,W) fp32 (0 where inconsistent), x2d_src, y2d_src (H,W) fp32."""
    dev = torch.device(device)
    depth_all = torch.from_numpy(np.stack([depth_ref, depth_src]).astype(np.float32)).to(dev)
    mats = torch.from_numpy(fusion_matrices(intrinsics_ref, extrinsics_ref, [intrinsics_src], [extrinsics_src])).to(dev)
    conf = torch.zeros(depth_ref.shape, device=dev, dtype=torch.float32)
    r = fuse_view(depth_all, 0, [1], conf, None, mats, 0.0, 1, img_dist_thresh, depth_thresh, debug=True)
    xy = r["xy_src"][0].cpu().numpy()
    return r["geo"][0].cpu().numpy().astype(bool), r["depth_reprojected"][0].cpu().numpy(), xy[..., 0].copy(), xy[..., 1].copy()


def ply_bytes(xyz, rgb, normals=None):
    """Binary little-endian PLY with vertex properties x y z (float) red green blue (uchar): the file the reference writes
    through plyfile (eval_rcmvsnet_dtu.py:433-446).  normals (n,3) fp32: the vertex is x y z nx ny nz red green blue, the mesh
    writer's order (tsdf_mesh.mesh_ply_bytes); dtu_io.read_ply_xyz skips the extra properties."""
    n = len(xyz)
    geo = ("x", "y", "z") + (("nx", "ny", "nz") if normals is not None else ())
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n%s"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % (n, "".join("property float %s\n" % k for k in geo))).encode("ascii")
    rec = np.empty(n, dtype=[(k, "<f4") for k in geo] + [("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for i, k in enumerate(("x", "y", "z")):
        rec[k] = xyz[:, i]
    if normals is not None:
        if tuple(np.shape(normals)) != (n, 3):
            raise _lib.RcmvsError(f"ply_bytes: normals {tuple(np.shape(normals))} for {n} points")
        for i, k in enumerate(("nx", "ny", "nz")):
            rec[k] = np.asarray(normals, dtype=np.float32)[:, i]
    for i, k in enumerate(("red", "green", "blue")):
        rec[k] = rgb[:, i]
    return head + rec.tobytes()


def stage_colour(img, num_stage, shape):
    """The colour image at the depth map's resolution (eval_rcmvsnet_dtu.py:410-415)."""
    if num_stage == 1:
        img = img[1::4, 1::4, :]
    elif num_stage == 2:
        img = img[1::2, 1::2, :]
    if img.shape[:2] != tuple(shape):
        raise _lib.RcmvsError(f"filter_depth: image {img.shape[:2]} does not match the depth map {tuple(shape)}")
    return np.ascontiguousarray(img)


def filter_depth(pair_folder, scan_folder, out_folder, plyfilename, prob_threshold, num_consistent, img_dist_thresh, depth_thresh,
                 num_stage=3, device="cuda:0", save_masks=True, verbose=True, method="reference", dynamic=None, dedup=False, stats=None, clean=None, poisson=None):
    """eval_rcmvsnet_dtu.py:341-446: fuse one scan into ``plyfilename``; returns (xyz (n,3) fp32, rgb (n,3) uint8).
    method="reference" without dedup is the reference's filter (rcmvs_fuse_view), to the byte.  method="dynamic": the dynamic
    consistency check (fuse_view_dynamic) with the parameters of ``dynamic`` (a dict over DYN_DEFAULTS); prob_threshold stays the
    caller's, num_consistent and the two fixed thresholds are not used.  dedup=True: one point per surface, with either method (for
    "reference" the fixed check runs as one level of the dynamic kernel, see reference_bases); the cloud then depends on the order
    of pair.txt's reference views, which is the order of the launches, and a fourth mask image <view>_claimed.png is written.
    stats: a dict that receives "views" = [{"ref", "kept", "claimed"}], "kept" and "claimed".
    clean: a dict of cloud_clean.clean_cloud's options (radius, stat, normals): the concatenated cloud goes through it before the PLY
    is written (with normals: x y z nx ny nz red green blue), the returned cloud is the one written, and stats gains "cloud".
    poisson: a dict of poisson_mesh.reconstruct's keywords: the cleaned cloud with its normals (clean must ask for them) is meshed from
    the tensors still on the device, written as <plyfilename without .ply>_poisson.ply, and stats gains "poisson"."""
    plain = _check_method(method, dynamic, dedup)
    dev = torch.device(device)
    pairs = scan_io.read_pair_file(os.path.join(pair_folder, "pair.txt"))
    views = sorted({v for ref, srcs in pairs for v in [ref] + list(srcs)})
    slot = {v: i for i, v in enumerate(views)}
    cams = {v: scan_io.read_camera_parameters(os.path.join(scan_folder, "cams/{:0>8}_cam.txt".format(v))) for v in views}
    depth_all = torch.from_numpy(np.stack([read_pfm(os.path.join(out_folder, "depth_est/{:0>8}.pfm".format(v)))[0] for v in views])).to(dev)
    if save_masks:
        os.makedirs(os.path.join(out_folder, "mask"), exist_ok=True)
    used = torch.zeros(depth_all.shape, device=dev, dtype=torch.uint8) if dedup else None      # zero-filled once per scan
    kinds = ("photo", "geo", "final") + (("claimed",) if dedup else ())
    pts, cols = [], []
    for ref, srcs in pairs:
        if len(srcs) > MAX_SRC:
            raise _lib.RcmvsError(f"filter_depth: view {ref} lists {len(srcs)} source views (at most {MAX_SRC})")
        conf = torch.from_numpy(read_pfm(os.path.join(out_folder, "confidence/{:0>8}.pfm".format(ref)))[0]).to(dev)
        img = scan_io.read_img(os.path.join(scan_folder, "images/{:0>8}.jpg".format(ref)))
        img = torch.from_numpy(stage_colour(img, num_stage, conf.shape)).to(dev)
        mats = torch.from_numpy(fusion_matrices(cams[ref][0], cams[ref][1], [cams[s][0] for s in srcs], [cams[s][1] for s in srcs])).to(dev)
        if plain:
            r = fuse_view(depth_all, slot[ref], [slot[s] for s in srcs], conf, img, mats, prob_threshold, num_consistent, img_dist_thresh, depth_thresh)
            xyz, rgb = compact_points(r["masks"][2], r["xyz"], r["rgb"])
            _stats_add(stats, ref, len(xyz), 0)
        else:
            r, _ = _fuse_dyn(depth_all, slot[ref], [slot[s] for s in srcs], conf, img, mats, prob_threshold, method, dynamic,
                             (num_consistent, img_dist_thresh, depth_thresh), used)
            xyz, rgb, kept, claimed = _compact_counted(r["masks"], r["xyz"], r["rgb"])
            _stats_add(stats, ref, kept, claimed)
        pts.append(xyz.cpu().numpy())
        cols.append(rgb.cpu().numpy())
        if save_masks or verbose:
            m = r["masks"].cpu().numpy().astype(bool)
            if save_masks:
                for k, kind in enumerate(kinds):
                    scan_io.save_mask(os.path.join(out_folder, "mask/{:0>8}_{}.png".format(ref, kind)), m[k])
            if verbose:
                print("processing {}, ref-view{:0>2}, photo/geo/final-mask:{}/{}/{}".format(scan_folder, ref, m[0].mean(), m[1].mean(), m[2].mean()))
    xyz, rgb = _write_cloud(plyfilename, pts, cols, [camera_centre(cams[ref][1]) for ref, _ in pairs], clean, stats, dev, poisson)
    if verbose:
        print("saving the final model to", plyfilename)
    return xyz, rgb


def _tanks_filter(sizes, geo_mask, photo, geo_pixel, geo_depth):
    return {s: {"image_size": sizes[s], "geo_mask_thres": geo_mask[s], "photo_thres": photo[s], "geo_pixel_thres": geo_pixel[s],
                "geo_depth_thres": geo_depth[s]} for s in sizes}


# The per-scene settings of the reference's Tanks-and-Temples evaluation (eval_rcmvsnet_tanks.py:400-440 intermediate, :460-491
# advanced; they sit under ``if __name__ == '__main__'`` there): TANKS_FILTER[split][scene] -> original image size (w, h), number of
# consistent source views, confidence threshold, reprojection distance in pixels, relative depth difference.
TANKS_FILTER = {
    "intermediate": _tanks_filter(
        {"Family": (1920, 1080), "Francis": (1920, 1080), "Horse": (1920, 1080), "Lighthouse": (2048, 1080), "M60": (2048, 1080),
         "Panther": (2048, 1080), "Playground": (1920, 1080), "Train": (1920, 1080)},
        {"Family": 6, "Francis": 8, "Horse": 4, "Lighthouse": 7, "M60": 6, "Panther": 7, "Playground": 7, "Train": 6},
        {"Family": 0.9, "Francis": 0.8, "Horse": 0.8, "Lighthouse": 0.8, "M60": 0.9, "Panther": 0.9, "Playground": 0.85, "Train": 0.9},
        {"Family": 0.75, "Francis": 1.0, "Horse": 1.25, "Lighthouse": 1.0, "M60": 0.75, "Panther": 1.0, "Playground": 1.0, "Train": 1.5},
        {"Family": 0.01, "Francis": 0.01, "Horse": 0.01, "Lighthouse": 0.01, "M60": 0.005, "Panther": 0.01, "Playground": 0.01, "Train": 0.01}),
    "advanced": _tanks_filter(
        {"Auditorium": (1920, 1080), "Ballroom": (1920, 1080), "Courtroom": (1920, 1080), "Museum": (1920, 1080), "Palace": (1920, 1080),
         "Temple": (1920, 1080)},
        {"Auditorium": 3, "Ballroom": 4, "Courtroom": 3, "Museum": 4, "Palace": 5, "Temple": 3},
        {"Auditorium": 0.7, "Ballroom": 0.8, "Courtroom": 0.8, "Museum": 0.8, "Palace": 0.9, "Temple": 0.8},
        {"Auditorium": 4.0, "Ballroom": 4.0, "Courtroom": 3.0, "Museum": 4.0, "Palace": 4.0, "Temple": 4.0},
        {"Auditorium": 0.005, "Ballroom": 0.005, "Courtroom": 0.005, "Museum": 0.01, "Palace": 0.005, "Temple": 0.01}),
}


def _resident(maps, view, dev, what):
    """the (H,W) fp32 device tensor of ``view`` handed over by the caller, or None: then the PFM file is read"""
    t = None if maps is None else maps.get(view)
    if t is None:
        return None
    if t.dim() != 2 or t.dtype != torch.float32 or t.device != dev:
        raise _lib.RcmvsError(f"filter_depth_tanks: {what} of view {view} must be an (H,W) fp32 tensor on {dev}, got {tuple(t.shape)} {t.dtype} on {t.device}")
    return t.contiguous()


def filter_depth_tanks(scan_folder, out_folder, plyfilename, geo_pixel_thres, geo_depth_thres, photo_thres, img_wh, image_sizes,
                       geo_mask_thres, n_views=None, scan="", device="cuda:0", save_masks=True, verbose=True, depth_maps=None,
                       conf_maps=None, method="reference", dynamic=None, dedup=False, stats=None, clean=None, poisson=None):
    """eval_rcmvsnet_tanks.py:269-380, the Tanks-and-Temples form of filter_depth: pair.txt, cams_1/ and images/ live in
    ``scan_folder`` at the ORIGINAL image size ``image_sizes`` = (w, h); the depth maps under ``out_folder`` have the network
    size ``img_wh`` = (w, h), so the intrinsics' first two rows are rescaled and the colour image is resized (cv2.resize's
    rule, on the device).  Same kernels as filter_depth.  depth_maps / conf_maps: optional {view: (H,W) fp32 tensor on ``device``},
    the network's outputs still in HBM; where a view is present its PFM file is not read (PFM holds fp32 losslessly, so the
    cloud is the same to the byte).  method / dynamic / dedup / stats: as filter_depth's; with method="dynamic" photo_thres stays the
    scene's and geo_mask_thres, geo_pixel_thres and geo_depth_thres are not used.  clean: as filter_depth's.  Returns (xyz (n,3) fp32,
    rgb (n,3) uint8)."""
    from .mvs_dataset import prepare_image
    plain = _check_method(method, dynamic, dedup)
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    pairs = scan_io.read_pair_file(os.path.join(scan_folder, "pair.txt"))
    views = sorted({v for ref, srcs in pairs for v in [ref] + list(srcs)})
    slot = {v: i for i, v in enumerate(views)}
    ow, oh = image_sizes
    cams = {}
    for v in views:
        K, E = scan_io.read_camera_parameters(os.path.join(scan_folder, "cams_1/{:0>8}_cam.txt".format(v)))
        K[0] *= img_wh[0] / ow
        K[1] *= img_wh[1] / oh
        cams[v] = (K, E)
    planes = []
    for v in views:
        t = _resident(depth_maps, v, dev, "depth")
        if t is None:
            t = torch.from_numpy(np.ascontiguousarray(read_pfm(os.path.join(out_folder, "depth_est/{:0>8}.pfm".format(v)))[0])).to(dev)
        planes.append(t)
    depth_all = torch.stack(planes)
    del planes
    if tuple(depth_all.shape[1:]) != (img_wh[1], img_wh[0]):
        raise _lib.RcmvsError(f"filter_depth_tanks: depth maps are {tuple(depth_all.shape[1:])}, img_wh says {(img_wh[1], img_wh[0])}")
    if save_masks:
        os.makedirs(os.path.join(out_folder, "mask"), exist_ok=True)
    used = torch.zeros(depth_all.shape, device=dev, dtype=torch.uint8) if dedup else None      # zero-filled once per scan
    kinds = ("photo", "geo", "final") + (("claimed",) if dedup else ())
    pts, cols = [], []
    for ref, srcs in pairs:
        if len(srcs) > MAX_SRC:
            raise _lib.RcmvsError(f"filter_depth_tanks: view {ref} lists {len(srcs)} source views (at most {MAX_SRC})")
        conf = _resident(conf_maps, ref, dev, "confidence")
        if conf is None:
            conf = torch.from_numpy(np.ascontiguousarray(read_pfm(os.path.join(out_folder, "confidence/{:0>8}.pfm".format(ref)))[0])).to(dev)
        raw = np.array(Image.open(os.path.join(scan_folder, "images/{:0>8}.jpg".format(ref))), dtype=np.uint8)
        img = prepare_image(raw, (img_wh[1], img_wh[0]), dev, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)).permute(1, 2, 0).contiguous()
        mats = torch.from_numpy(fusion_matrices(cams[ref][0], cams[ref][1], [cams[s][0] for s in srcs], [cams[s][1] for s in srcs])).to(dev)
        if plain:
            r = fuse_view(depth_all, slot[ref], [slot[s] for s in srcs], conf, img, mats, photo_thres, geo_mask_thres, geo_pixel_thres, geo_depth_thres)
            xyz, rgb = compact_points(r["masks"][2], r["xyz"], r["rgb"])
            _stats_add(stats, ref, len(xyz), 0)
        else:
            r, _ = _fuse_dyn(depth_all, slot[ref], [slot[s] for s in srcs], conf, img, mats, photo_thres, method, dynamic,
                             (geo_mask_thres, geo_pixel_thres, geo_depth_thres), used)
            xyz, rgb, kept, claimed = _compact_counted(r["masks"], r["xyz"], r["rgb"])
            _stats_add(stats, ref, kept, claimed)
        pts.append(xyz.cpu().numpy())
        cols.append(rgb.cpu().numpy())
        if save_masks or verbose:
            m = r["masks"].cpu().numpy().astype(bool)
            if save_masks:
                for k, kind in enumerate(kinds):
                    scan_io.save_mask(os.path.join(out_folder, "mask/{:0>8}_{}.png".format(ref, kind)), m[k])
            if verbose:
                print("processing {}, ref-view{:0>2}, geo_mask:{:3f} photo_mask:{:3f} final_mask: {:3f}".format(
                    scan_folder, ref, m[1].mean(), m[0].mean(), m[2].mean()))
    os.makedirs(os.path.dirname(os.path.abspath(plyfilename)), exist_ok=True)
    xyz, rgb = _write_cloud(plyfilename, pts, cols, [camera_centre(cams[ref][1]) for ref, _ in pairs], clean, stats, dev, poisson)
    if verbose:
        print("saving the final model to", plyfilename)
    return xyz, rgb


def filter_scans(jobs, rank=None, world=None, **kwargs):
    """pcd_filter (eval_rcmvsnet_dtu.py:503-515) without the process pool: jobs = [dict of filter_depth arguments]; each rank
    (one process per GPU, RANK / WORLD_SIZE / LOCAL_RANK from the environment) takes every world-th scan, no collective."""
    from .sharding import shard_items
    rank = int(os.environ.get("RANK", "0")) if rank is None else rank
    world = int(os.environ.get("WORLD_SIZE", "1")) if world is None else world
    device = "cuda:%d" % int(os.environ.get("LOCAL_RANK", "0"))
    return [filter_depth(device=device, **dict(job, **kwargs)) for job in shard_items(list(jobs), rank, world)]
