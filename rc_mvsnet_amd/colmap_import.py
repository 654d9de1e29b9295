"""Import a COLMAP reconstruction as an MVSNet-style scan folder (``images/``, ``cams/%08d_cam.txt``, ``pair.txt``), the layout
``mvs_dataset.MVSDataset`` and ``eval_driver`` read.  The two passes that grow with the model run on the HIP path
(csrc/view_select.hip, arithmetic in csrc/view_select_math.h, restated in fp64 numpy by tests/colmap_oracle.py):

1. ``pair_scores``: for every image pair the sum, over the 3-D points both images observe, of a weight of the triangulation
   angle theta (degrees, ``atan2(|a x b|, a.b)`` of the two centre-to-point vectors): ``exp(-(theta - theta0)^2 / (2 sigma^2))``
   with ``sigma = sigma1`` up to ``theta0`` and ``sigma2`` beyond.
2. ``top_views``: per image the ``num_src`` best partners, score descending, the lower index first among equals; partners with
   score 0 are never listed.
3. ``depth_ranges``: per image the exact order statistics of its points' depths at the ranks ``int(c * 0.01)`` and
   ``int(c * 0.99)`` -> ``depth_min``, ``depth_max``; ``depth_interval = (depth_max - depth_min) / (max_d - 1) / interval_scale``.

With ``--undistort`` the polynomial (Brown) camera models ``SIMPLE_RADIAL``, ``RADIAL``, ``OPENCV`` and ``FULL_OPENCV`` are read
too, and every image with a non-zero coefficient (every image, when ``--focal-scale`` is not 1) is resampled on the GPU
(``undistort_image``: csrc/undistort.hip, arithmetic in csrc/undistort_math.h, restated by tests/undistort_oracle.py) to the
pinhole camera (s fx, s fy, cx, cy) of the same size, s = ``--focal-scale``: pixel centres at +0.5 as in COLMAP, bilinear with the
border pixel repeated, an output pixel whose source position is not inside the image is black and counted (``blank_fraction_max``
in the summary).  The undistorted image is saved as JPEG at quality 95; the other images are copied as before.

Limits: without ``--undistort`` ``SIMPLE_PINHOLE`` / ``PINHOLE`` cameras only; intrinsics are written as COLMAP states them (no
half-pixel shift).  The output camera is not chosen automatically (COLMAP's ``blank_pixels`` / ``min_scale`` search is not
implemented): pick ``--focal-scale`` and read ``blank_fraction_max``.  Very strong barrel distortion folds over far outside the
calibrated radius, as it does in COLMAP.  The fisheye models and ``FOV`` are refused.  CUDA tensors only; no CPU fallback.

    python -m rc_mvsnet_amd.colmap_import --model SPARSE --images DIR --out TESTPATH/SCENE [--undistort [--focal-scale S]]
"""
import argparse
import ctypes
import json
import math
import os
import shutil

import numpy as np
import torch

from . import _lib, colmap_io, scan_io
from .ops import _chk, _stream

MAX_IMAGES, MAX_SRC = _lib.CONSTANTS["RCMVS_VS_MAX_IMAGES"], _lib.CONSTANTS["RCMVS_VS_MAX_SRC"]


def _model_tensors(points, offsets, ids, n):
    if points.dim() != 2 or points.shape[1] != 3 or len(points) == 0:
        raise _lib.RcmvsError(f"points: expected (m,3) with m >= 1, got {tuple(points.shape)}")
    if offsets.dim() != 1 or len(offsets) != n + 1 or ids.dim() != 1 or len(ids) == 0:
        raise _lib.RcmvsError(f"offsets / ids: expected ({n + 1},) and a non-empty (nnz,), got {tuple(offsets.shape)} and {tuple(ids.shape)}")
    if not 1 <= n <= MAX_IMAGES:
        raise _lib.RcmvsError(f"{n} images (1 .. {MAX_IMAGES}, RCMVS_VS_MAX_IMAGES: the score table is (n,n) fp64)")
    off = offsets.cpu()
    if off.dtype != torch.int64 or int(off[0]) != 0 or int(off[-1]) != len(ids) or bool((off[1:] < off[:-1]).any()):
        raise _lib.RcmvsError("offsets: expected int64, ascending, from 0 to len(ids)")
    return len(points), len(ids)


def pair_scores(centres, points, offsets, ids, theta0=5.0, sigma1=1.0, sigma2=10.0):
    """centres (n,3) and points (m,3) fp64, offsets (n+1,) int64, ids (nnz,) int32 -> the symmetric (n,n) fp64 score table with a
    zero diagonal.  Two runs give the same bits."""
    n = len(centres)
    if centres.dim() != 2 or centres.shape[1] != 3:
        raise _lib.RcmvsError(f"centres: expected (n,3), got {tuple(centres.shape)}")
    m, nnz = _model_tensors(points, offsets, ids, n)
    for name, v in (("theta0", theta0), ("sigma1", sigma1), ("sigma2", sigma2)):
        if not math.isfinite(v) or (name != "theta0" and not v > 0):
            raise _lib.RcmvsError(f"pair_scores: {name} {v}")
    scores = torch.empty((n, n), device=centres.device, dtype=torch.float64)
    _lib.call("rcmvs_vs_pair_scores", _chk(centres, "centres", torch.float64), n, _chk(points, "points", torch.float64), m,
              _chk(offsets, "offsets", torch.int64), _chk(ids, "ids", torch.int32), nnz, float(theta0), float(sigma1), float(sigma2),
              _chk(scores, "scores", torch.float64), _stream())
    return scores


def top_views(scores, k):
    """(n,n) fp64 -> (ids (n,k) int32 with -1 where there is no partner, scores (n,k) fp64, counts (n,) int32 = the partners with
    score > 0): per row the k best in the order (score descending, index ascending)."""
    if scores.dim() != 2 or scores.shape[0] != scores.shape[1] or not 1 <= len(scores) <= MAX_IMAGES:
        raise _lib.RcmvsError(f"top_views: expected an (n,n) table with n in 1 .. {MAX_IMAGES}, got {tuple(scores.shape)}")
    k = int(k)
    if not 1 <= k <= MAX_SRC:
        raise _lib.RcmvsError(f"top_views: k={k} (1 .. {MAX_SRC}, RCMVS_VS_MAX_SRC)")
    n, dev = len(scores), scores.device
    ids = torch.empty((n, k), device=dev, dtype=torch.int32)
    top = torch.empty((n, k), device=dev, dtype=torch.float64)
    counts = torch.empty(n, device=dev, dtype=torch.int32)
    _lib.call("rcmvs_vs_top_views", _chk(scores, "scores", torch.float64), n, k, _chk(ids, "ids", torch.int32),
              _chk(top, "top_scores", torch.float64), _chk(counts, "counts", torch.int32), _stream())
    return ids, top, counts


def depth_ranges(points, zrows, offsets, ids, ranks):
    """zrows (n,4) fp64 = the third extrinsic row {r20, r21, r22, t2} per image, ranks (n,2) int32 -> (n,2) fp64: the order
    statistics of z = ((r20 x + r21 y) + r22 z) + t2 over each image's points at its two ranks, bit-identical to sorting."""
    n = len(zrows)
    if zrows.dim() != 2 or zrows.shape[1] != 4 or tuple(ranks.shape) != (n, 2):
        raise _lib.RcmvsError(f"depth_ranges: expected zrows (n,4) and ranks (n,2), got {tuple(zrows.shape)} and {tuple(ranks.shape)}")
    m, nnz = _model_tensors(points, offsets, ids, n)
    dev = points.device
    zkey = torch.empty(nnz, device=dev, dtype=torch.int64)
    out = torch.empty((n, 2), device=dev, dtype=torch.float64)
    _lib.call("rcmvs_vs_depth_ranks", _chk(points, "points", torch.float64), m, _chk(zrows, "zrows", torch.float64), n,
              _chk(offsets, "offsets", torch.int64), _chk(ids, "ids", torch.int32), nnz, _chk(ranks, "ranks", torch.int32),
              _chk(zkey, "zkey", torch.int64), _chk(out, "out", torch.float64), _stream())
    return out


def rank_pair(c):
    """the two 0-based ranks of an image with c points: int(c * 0.01), int(c * 0.99)"""
    return int(c * 0.01), int(c * 0.99)


def undistort_image(img, camera, dist, focal_scale=1.0):
    """img (H,W,3) uint8 of the camera (fx, fy, cx, cy) with distortion dist = (k1, k2, p1, p2, k3, k4, k5, k6) -> (out (H,W,3) uint8
    as seen by the pinhole camera (s fx, s fy, cx, cy), s = focal_scale; blank = the number of output pixels without a source,
    written (0, 0, 0)).  Two runs give the same bytes."""
    if img.dim() != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise _lib.RcmvsError(f"undistort_image: expected an (H,W,3) image, got {tuple(img.shape)}")
    H, W = int(img.shape[0]), int(img.shape[1])
    if H * W * 3 >= 1 << 31:
        raise _lib.RcmvsError(f"undistort_image: {H} x {W} x 3 bytes (below 2^31)")
    camera, dist = [float(v) for v in camera], [float(v) for v in dist]
    if len(camera) != 4 or len(dist) != 8:
        raise _lib.RcmvsError(f"undistort_image: expected camera (fx, fy, cx, cy) and 8 coefficients, got {len(camera)} and {len(dist)} numbers")
    if not all(math.isfinite(v) for v in camera + dist) or not (camera[0] > 0 and camera[1] > 0):
        raise _lib.RcmvsError(f"undistort_image: camera {camera}, coefficients {dist} (finite, focal lengths positive)")
    if not (math.isfinite(focal_scale) and focal_scale > 0):
        raise _lib.RcmvsError(f"undistort_image: focal_scale {focal_scale} (finite, positive)")
    fx, fy, cx, cy = camera
    src = _chk(img, "img", torch.uint8)
    out = torch.empty_like(img)
    blank = torch.empty(1, device=img.device, dtype=torch.int32)
    _lib.call("rcmvs_undistort_rgb8", src, _chk(out, "out", torch.uint8), H, W, fx, fy, cx, cy, float(focal_scale) * fx, float(focal_scale) * fy,
              (ctypes.c_double * 8)(*dist), _chk(blank, "blank", torch.int32), _stream())
    return out, int(blank.item())


# ---- files ------------------------------------------------------------------------------------------------------------
def write_pair_file(filename, lists):
    """lists: [(ref, [(src, score), ...])] of the images that have partners.  The first line counts the entries that follow (it is
    what scan_io.read_pair_file loops over), so it is the image count less the images without a partner."""
    with open(filename, "w") as f:
        f.write("%d\n" % len(lists))
        for ref, srcs in lists:
            f.write("%d\n%d %s\n" % (ref, len(srcs), " ".join("%d %r" % (int(s), float(v)) for s, v in srcs)))


def _copy_image(src, dst, size):
    from PIL import Image
    try:
        with Image.open(src) as im:
            if im.size != size:
                raise _lib.RcmvsError(f"{src}: size {im.size[0]} x {im.size[1]} differs from its camera's {size[0]} x {size[1]}")
            with open(src, "rb") as f:
                jpeg = f.read(3) == b"\xff\xd8\xff"
            if not jpeg:
                im.convert("RGB").save(dst, format="JPEG", quality=95)
    except OSError as e:
        raise _lib.RcmvsError(f"{src}: not a readable image ({e})") from None
    if jpeg:
        shutil.copyfile(src, dst)                                 # byte for byte


def _undistort_file(src, dst, size, K, dist, focal_scale, dev):
    """decode, check the size against the camera, resample on the device, save as JPEG at quality 95 -> blank pixel count"""
    from PIL import Image
    try:
        with Image.open(src) as im:
            if im.size != size:
                raise _lib.RcmvsError(f"{src}: size {im.size[0]} x {im.size[1]} differs from its camera's {size[0]} x {size[1]}")
            rgb = np.array(im.convert("RGB"), dtype=np.uint8)
    except OSError as e:
        raise _lib.RcmvsError(f"{src}: not a readable image ({e})") from None
    got, blank = undistort_image(torch.from_numpy(rgb).to(dev), (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), dist, focal_scale)
    Image.fromarray(got.cpu().numpy()).save(dst, format="JPEG", quality=95)
    return blank


def import_scene(model, images, out, max_d=192, interval_scale=1.0, num_src=10, theta0=5.0, sigma1=1.0, sigma2=10.0, device="cuda:0",
                 undistort=False, focal_scale=1.0):
    """COLMAP sparse model folder + image folder -> the scan folder ``out``; returns the summary dict the command line prints.
    ``undistort``: read the polynomial camera models too and resample their images to the pinhole camera (focal_scale fx,
    focal_scale fy, cx, cy), which is what ``cams/`` then states."""
    max_d, num_src = int(max_d), int(num_src)
    if max_d < 2 or not (interval_scale > 0 and math.isfinite(interval_scale)):
        raise _lib.RcmvsError(f"import_scene: max_d {max_d} (at least 2), interval_scale {interval_scale} (positive)")
    if not 1 <= num_src <= MAX_SRC:
        raise _lib.RcmvsError(f"import_scene: num_src {num_src} (1 .. {MAX_SRC}, RCMVS_VS_MAX_SRC)")
    focal_scale = float(focal_scale)
    if not (math.isfinite(focal_scale) and focal_scale > 0) or (focal_scale != 1.0 and not undistort):
        raise _lib.RcmvsError(f"import_scene: focal_scale {focal_scale} (finite, positive; another value than 1 needs undistort=True)")
    M = colmap_io.read_model(model, distortion=bool(undistort)) if isinstance(model, (str, os.PathLike)) else model
    n, names = len(M["image_ids"]), M["names"]
    if n == 0 or len(M["points"]) == 0:
        raise _lib.RcmvsError(f"{M['files']['images']}: {n} images and {len(M['points'])} points: nothing to import")
    counts = np.diff(M["offsets"])
    for k in np.flatnonzero(counts < 2):
        raise _lib.RcmvsError(f"image {int(M['image_ids'][k])} ({names[k]}): {int(counts[k])} 3-D points (at least 2 for a depth range)")
    dev = torch.device(device)
    points, offsets = torch.from_numpy(M["points"]).to(dev), torch.from_numpy(M["offsets"]).to(dev)
    ids = torch.from_numpy(M["ids"]).to(dev)
    ranks = np.array([rank_pair(int(c)) for c in counts], dtype=np.int32)
    zrows = np.ascontiguousarray(M["extrinsics"][:, 2, :])
    dr = depth_ranges(points, torch.from_numpy(zrows).to(dev), offsets, ids, torch.from_numpy(ranks).to(dev)).cpu().numpy()
    for k in range(n):
        if not dr[k, 0] > 0 or not np.isfinite(dr[k]).all():
            raise _lib.RcmvsError(f"image {int(M['image_ids'][k])} ({names[k]}): depth_min {dr[k, 0]} (the 1 % depth of its points must be "
                                  "positive: points behind the camera)")
    k_src = num_src
    scores = pair_scores(torch.from_numpy(M["centres"]).to(dev), points, offsets, ids, theta0, sigma1, sigma2)
    top_ids, top_scores, positive = (t.cpu().numpy() for t in top_views(scores, k_src))
    for sub in ("images", "cams"):
        os.makedirs(os.path.join(out, sub), exist_ok=True)
    lists, skipped, undistorted, blank_max = [], [], 0, 0.0
    dist = M.get("distortion") if undistort else None
    for k in range(n):
        listed = min(int(positive[k]), k_src)
        if listed == 0:
            skipped.append(k)
        else:
            lists.append((k, [(int(top_ids[k, r]), float(top_scores[k, r])) for r in range(listed)]))
        cam = np.zeros((2, 4, 4), dtype=np.float64)
        cam[0], cam[1, :3, :3] = M["extrinsics"][k], M["intrinsics"][k]
        cam[1, 0, 0], cam[1, 1, 1] = focal_scale * cam[1, 0, 0], focal_scale * cam[1, 1, 1]
        interval = (dr[k, 1] - dr[k, 0]) / (max_d - 1) / interval_scale
        cam[1, 3] = (dr[k, 0], interval, max_d, dr[k, 1])
        scan_io.write_cam(os.path.join(out, "cams", "%08d_cam.txt" % k), cam)
        src, dst, size = os.path.join(images, names[k]), os.path.join(out, "images", "%08d.jpg" % k), (int(M["sizes"][k, 0]), int(M["sizes"][k, 1]))
        if undistort and (focal_scale != 1.0 or (dist is not None and bool(np.any(dist[k] != 0)))):
            row = dist[k] if dist is not None else np.zeros(8)
            blank = _undistort_file(src, dst, size, M["intrinsics"][k], row, focal_scale, dev)
            undistorted, blank_max = undistorted + 1, max(blank_max, blank / (size[0] * size[1]))
        else:
            _copy_image(src, dst, size)
    write_pair_file(os.path.join(out, "pair.txt"), lists)
    summary = {"scene": os.fspath(out), "images": n, "points": int(len(M["points"])), "observations": int(len(M["ids"])), "num_src": num_src,
               "max_d": max_d, "interval_scale": float(interval_scale), "refs": len(lists), "skipped_refs": skipped,
               "depth_min": float(dr[:, 0].min()), "depth_max": float(dr[:, 1].max()),
               "image_names": {"%08d" % k: names[k] for k in range(n)}}
    if undistort:
        summary.update(undistorted=undistorted, focal_scale=focal_scale, blank_fraction_max=float(blank_max))
    return summary


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="COLMAP sparse model -> MVSNet-style scan folder (view selection and depth ranges on the GPU)")
    ap.add_argument("--model", required=True, help="folder of cameras / images / points3D as .txt or .bin (text wins if both exist)")
    ap.add_argument("--images", required=True, help="folder of the (undistorted) images the model names")
    ap.add_argument("--out", required=True, help="TESTPATH/SCENE: receives images/, cams/ and pair.txt")
    ap.add_argument("--max-d", type=int, default=192)
    ap.add_argument("--interval-scale", type=float, default=1.0)
    ap.add_argument("--num-src", type=int, default=10)
    ap.add_argument("--theta0", type=float, default=5.0)
    ap.add_argument("--sigma1", type=float, default=1.0)
    ap.add_argument("--sigma2", type=float, default=10.0)
    ap.add_argument("--undistort", action="store_true", help="read SIMPLE_RADIAL / RADIAL / OPENCV / FULL_OPENCV cameras too and resample their images "
                    "to the pinhole camera of the same principal point and size (GPU)")
    ap.add_argument("--focal-scale", type=float, default=None, metavar="S", help="with --undistort: the output focal lengths are S times the camera's "
                    "(default 1; below 1 keeps more of the field of view, above 1 crops blank borders away: read blank_fraction_max)")
    args = ap.parse_args(argv)
    if args.focal_scale is not None and not args.undistort:
        ap.error("--focal-scale needs --undistort")
    if args.focal_scale is None:
        args.focal_scale = 1.0
    return args


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("colmap_import: needs a GPU (view selection and depth ranges have no CPU fallback)")
    _lib.load()
    summary = import_scene(args.model, args.images, args.out, max_d=args.max_d, interval_scale=args.interval_scale, num_src=args.num_src,
                           theta0=args.theta0, sigma1=args.sigma1, sigma2=args.sigma2, undistort=args.undistort, focal_scale=args.focal_scale)
    print(json.dumps(summary), flush=True)
    return summary


if __name__ == "__main__":
    main()
