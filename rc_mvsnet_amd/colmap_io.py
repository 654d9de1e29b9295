"""Readers of a COLMAP sparse model (host only): ``cameras``, ``images`` and ``points3D`` as ``.txt`` or ``.bin``.

``read_model(dir)`` returns plain arrays for rc_mvsnet_amd/colmap_import.py: images renumbered 0..n-1 in ascending COLMAP image
id, points renumbered 0..m-1 in ascending point id, and per image an ascending duplicate-free list of point indices as CSR
(``offsets`` (n+1) int64, ``ids`` int32).  World-to-camera is ``x_cam = R(q) x_w + t`` with q = (w, x, y, z).

By default only ``SIMPLE_PINHOLE`` (f, cx, cy) and ``PINHOLE`` (fx, fy, cx, cy) cameras are accepted: images with any other model
must be undistorted first.  With ``distortion=True`` the readers also accept the polynomial (Brown) models ``SIMPLE_RADIAL``
(f, cx, cy, k), ``RADIAL`` (f, cx, cy, k1, k2), ``OPENCV`` (fx, fy, cx, cy, k1, k2, p1, p2) and ``FULL_OPENCV`` (... k3, k4, k5, k6),
and the model carries ``distortion`` (n, 8) fp64 in the fixed order k1, k2, p1, p2, k3, k4, k5, k6 (zeros where a model has no such
term) and ``models`` [n]; ``colmap_import.import_scene(undistort=True)`` resamples such images on the GPU.  The fisheye models and
``FOV`` are refused in both modes.  A truncated or malformed file, a non-finite number, an image whose camera is unknown and an
observation of an unknown point raise ``RcmvsError`` naming the file and the record.
"""
import os
import struct

import numpy as np

from ._lib import RcmvsError

# name -> (binary model id, number of parameters)
CAMERA_MODELS = {"SIMPLE_PINHOLE": (0, 3), "PINHOLE": (1, 4)}
# the polynomial (Brown) models the readers accept with distortion=True
DISTORTED_MODELS = {"SIMPLE_RADIAL": (2, 4), "RADIAL": (3, 5), "OPENCV": (4, 8), "FULL_OPENCV": (6, 12)}
_MODEL_NAMES = {0: "SIMPLE_PINHOLE", 1: "PINHOLE", 2: "SIMPLE_RADIAL", 3: "RADIAL", 4: "OPENCV", 5: "OPENCV_FISHEYE", 6: "FULL_OPENCV",
                7: "FOV", 8: "SIMPLE_RADIAL_FISHEYE", 9: "RADIAL_FISHEYE", 10: "THIN_PRISM_FISHEYE"}
_POINT2D = np.dtype([("x", "<f8"), ("y", "<f8"), ("id", "<i8")])


def _model_error(path, what, model, distortion=False):
    if distortion:
        return RcmvsError(f"{path}: {what}: camera model {model} is not supported (SIMPLE_PINHOLE, PINHOLE, {', '.join(DISTORTED_MODELS)}): "
                          "fisheye and FOV images must be undistorted first")
    return RcmvsError(f"{path}: {what}: camera model {model} is not supported (SIMPLE_PINHOLE and PINHOLE only): "
                      "the images must be undistorted first" +
                      (" (colmap_import --undistort does it for this model)" if model in DISTORTED_MODELS else ""))


def _models(distortion):
    return dict(CAMERA_MODELS, **DISTORTED_MODELS) if distortion else CAMERA_MODELS


def _finite(path, what, values):
    if not np.isfinite(np.asarray(values, dtype=np.float64)).all():
        raise RcmvsError(f"{path}: {what}: non-finite number")


def _text_records(path):
    """-> [(line number, text)] without the '#' comment lines; blank lines are kept (an image without points has an empty second line)"""
    try:
        with open(path) as f:
            return [(i + 1, ln.rstrip("\r\n")) for i, ln in enumerate(f) if not ln.lstrip().startswith("#")]
    except (OSError, UnicodeDecodeError) as e:
        raise RcmvsError(f"{path}: {e}") from None


class _Bin:
    """A little-endian binary file read with bounds: running past the end names the file and the record."""

    def __init__(self, path):
        self.path = path
        try:
            with open(path, "rb") as f:
                self.buf = f.read()
        except OSError as e:
            raise RcmvsError(f"{path}: {e}") from None
        self.at = 0

    def take(self, fmt, what):
        size = struct.calcsize(fmt)
        if self.at + size > len(self.buf):
            raise RcmvsError(f"{self.path}: {what}: the file is truncated ({len(self.buf)} bytes)")
        out = struct.unpack_from(fmt, self.buf, self.at)
        self.at += size
        return out

    def array(self, dtype, count, what):
        size = dtype.itemsize * count
        if count < 0 or self.at + size > len(self.buf):
            raise RcmvsError(f"{self.path}: {what}: the file is truncated ({len(self.buf)} bytes)")
        out = np.frombuffer(self.buf, dtype=dtype, count=count, offset=self.at)
        self.at += size
        return out

    def cstring(self, what):
        end = self.buf.find(b"\0", self.at)
        if end < 0:
            raise RcmvsError(f"{self.path}: {what}: the file is truncated (unterminated name)")
        s = self.buf[self.at:end].decode("utf-8", "replace")
        self.at = end + 1
        return s

    def done(self):
        if self.at != len(self.buf):
            raise RcmvsError(f"{self.path}: {len(self.buf) - self.at} bytes after the last record")


# ---- cameras ----------------------------------------------------------------------------------------------------------
def _camera(path, what, cid, model, w, h, params, distortion=False):
    models = _models(distortion)
    if model not in models:
        raise _model_error(path, what, model, distortion)
    if len(params) != models[model][1]:
        raise RcmvsError(f"{path}: {what}: {model} takes {models[model][1]} parameters, found {len(params)}")
    _finite(path, what, params)
    if w <= 0 or h <= 0:
        raise RcmvsError(f"{path}: {what}: size {w} x {h}")
    return {"id": int(cid), "model": model, "width": int(w), "height": int(h), "params": np.array(params, dtype=np.float64)}


def read_cameras_text(path, distortion=False):
    cams = {}
    for no, ln in _text_records(path):
        if not ln.strip():
            continue
        t, what = ln.split(), f"line {no}"
        try:
            cid, model, w, h, params = int(t[0]), t[1], int(t[2]), int(t[3]), [float(v) for v in t[4:]]
        except (ValueError, IndexError):
            raise RcmvsError(f"{path}: {what}: expected `id model width height params...`") from None
        cams[cid] = _camera(path, f"{what} (camera {cid})", cid, model, w, h, params, distortion)
    return cams


def read_cameras_binary(path, distortion=False):
    b, cams, models = _Bin(path), {}, _models(distortion)
    (n,) = b.take("<Q", "camera count")
    for k in range(n):
        what = f"camera record {k}"
        cid, mid, w, h = b.take("<iiQQ", what)
        name = _MODEL_NAMES.get(mid, f"id {mid}")
        if name not in models:
            raise _model_error(path, f"{what} (camera {cid})", name, distortion)
        params = b.take("<%dd" % models[name][1], what)
        cams[cid] = _camera(path, f"{what} (camera {cid})", cid, name, w, h, params, distortion)
    b.done()
    return cams


# ---- images -----------------------------------------------------------------------------------------------------------
def _image(path, what, iid, q, t, cid, name, p2d):
    _finite(path, what, q)
    _finite(path, what, t)
    _finite(path, what, p2d["x"])
    _finite(path, what, p2d["y"])
    return {"id": int(iid), "qvec": np.array(q, dtype=np.float64), "tvec": np.array(t, dtype=np.float64), "camera_id": int(cid),
            "name": name, "points2D": p2d}


def read_images_text(path):
    imgs, recs, k = [], _text_records(path), 0
    while k < len(recs):
        no, ln = recs[k]
        k += 1
        if not ln.strip():
            continue
        t, what = ln.split(), f"line {no}"
        try:
            if len(t) < 10:
                raise ValueError
            iid, q, tv, cid = int(t[0]), [float(v) for v in t[1:5]], [float(v) for v in t[5:8]], int(t[8])
            name = ln.split(None, 9)[9]
        except ValueError:
            raise RcmvsError(f"{path}: {what}: expected `id qw qx qy qz tx ty tz camera_id name`") from None
        what = f"{what} (image {iid})"
        if k >= len(recs):
            raise RcmvsError(f"{path}: {what}: the file is truncated (no line of 2-D points)")
        v = recs[k][1].split()
        k += 1
        p2d = np.empty(len(v) // 3, dtype=_POINT2D)
        try:
            if len(v) % 3:
                raise ValueError
            p2d["x"], p2d["y"] = [float(s) for s in v[0::3]], [float(s) for s in v[1::3]]
            p2d["id"] = [int(s) for s in v[2::3]]
        except ValueError:
            raise RcmvsError(f"{path}: {what}: the 2-D points are not `x y point3D_id` triples") from None
        imgs.append(_image(path, what, iid, q, tv, cid, name, p2d))
    return imgs


def read_images_binary(path):
    b, imgs = _Bin(path), []
    (n,) = b.take("<Q", "image count")
    for k in range(n):
        what = f"image record {k}"
        rec = b.take("<i7di", what)
        name = b.cstring(what)
        (m,) = b.take("<Q", what)
        p2d = b.array(_POINT2D, m, f"{what} (image {rec[0]})")
        imgs.append(_image(path, f"{what} (image {rec[0]})", rec[0], rec[1:5], rec[5:8], rec[8], name, p2d))
    b.done()
    return imgs


# ---- points -----------------------------------------------------------------------------------------------------------
def read_points3d_text(path):
    ids, xyz = [], []
    for no, ln in _text_records(path):
        if not ln.strip():
            continue
        t, what = ln.split(), f"line {no}"
        try:
            if len(t) < 8 or len(t) % 2:
                raise ValueError
            pid, p = int(t[0]), [float(v) for v in t[1:4]]
            [int(v) for v in t[4:7]]
            err = float(t[7])
            [int(v) for v in t[8:]]
        except ValueError:
            raise RcmvsError(f"{path}: {what}: expected `id x y z r g b error (image_id point2D_idx)...`") from None
        _finite(path, f"{what} (point {pid})", p + [err])
        ids.append(pid)
        xyz.append(p)
    return np.array(ids, dtype=np.int64), np.array(xyz, dtype=np.float64).reshape(-1, 3)


def read_points3d_binary(path):
    b = _Bin(path)
    (n,) = b.take("<Q", "point count")
    if n * 43 > len(b.buf):
        raise RcmvsError(f"{path}: point count {n}: the file is truncated ({len(b.buf)} bytes)")
    ids, xyz = np.empty(n, dtype=np.int64), np.empty((n, 3), dtype=np.float64)
    for k in range(n):
        what = f"point record {k}"
        pid, x, y, z, _, _, _, err, L = b.take("<Q3d3BdQ", what)
        if b.at + 8 * L > len(b.buf):
            raise RcmvsError(f"{path}: {what} (point {pid}): the file is truncated ({len(b.buf)} bytes)")
        b.at += 8 * L
        if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z) and np.isfinite(err)):
            raise RcmvsError(f"{path}: {what} (point {pid}): non-finite number")
        ids[k], xyz[k] = pid, (x, y, z)
    b.done()
    return ids, xyz


# ---- the model --------------------------------------------------------------------------------------------------------
def qvec_to_rotmat(q):
    """(w, x, y, z), normalised here -> the 3x3 rotation of x_cam = R x_w + t"""
    q = np.asarray(q, dtype=np.float64)
    norm = np.sqrt((q * q).sum())
    if not norm > 0:
        raise RcmvsError("qvec_to_rotmat: zero quaternion")
    w, x, y, z = q / norm
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * x * z + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
                     [2 * x * z - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]])


def camera_centre(R, t):
    """C = -R^T t"""
    return -(np.asarray(R, dtype=np.float64).T @ np.asarray(t, dtype=np.float64))


_ONE_FOCAL = ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL")


def intrinsic_matrix(cam):
    """K of a camera (the pinhole part of a distorted model), parameters unchanged (no half-pixel shift)"""
    p = cam["params"]
    fx, fy, cx, cy = (p[0], p[0], p[1], p[2]) if cam["model"] in _ONE_FOCAL else (p[0], p[1], p[2], p[3])
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def distortion_row(cam):
    """(8,) fp64 in the fixed order k1, k2, p1, p2, k3, k4, k5, k6; zeros where the camera's model has no such term"""
    p, d = cam["params"], np.zeros(8)
    if cam["model"] == "SIMPLE_RADIAL":
        d[0] = p[3]
    elif cam["model"] == "RADIAL":
        d[:2] = p[3:5]
    elif cam["model"] in ("OPENCV", "FULL_OPENCV"):
        d[:len(p) - 4] = p[4:]
    return d


def _pick(folder, stem):
    for ext, binary in ((".txt", False), (".bin", True)):                # text wins if both exist
        path = os.path.join(folder, stem + ext)
        if os.path.exists(path):
            return path, binary
    raise RcmvsError(f"{folder}: neither {stem}.txt nor {stem}.bin")


def read_model(folder, distortion=False):
    """-> dict: image_ids (n,) int64 ascending, names [n], camera_ids (n,), qvec (n,4), tvec (n,3), extrinsics (n,4,4), centres (n,3),
    intrinsics (n,3,3), sizes (n,2) int64 as (width, height), point_ids (m,) int64 ascending, points (m,3), offsets (n+1,) int64,
    ids int32, files {cameras, images, points3D}.  With ``distortion=True`` the polynomial camera models are read too, and the dict
    also has distortion (n,8) fp64 as k1, k2, p1, p2, k3, k4, k5, k6 and models [n]."""
    (pc, bc), (pi, bi), (pp, bp) = _pick(folder, "cameras"), _pick(folder, "images"), _pick(folder, "points3D")
    cams = (read_cameras_binary if bc else read_cameras_text)(pc, distortion)
    imgs = (read_images_binary if bi else read_images_text)(pi)
    pids, xyz = (read_points3d_binary if bp else read_points3d_text)(pp)
    order = np.argsort(pids, kind="stable")
    pids, xyz = pids[order], np.ascontiguousarray(xyz[order])
    if len(pids) > 1 and (pids[1:] == pids[:-1]).any():
        raise RcmvsError(f"{pp}: point {int(pids[1:][pids[1:] == pids[:-1]][0])} is listed twice")
    imgs.sort(key=lambda im: im["id"])
    n = len(imgs)
    for a, b in zip(imgs, imgs[1:]):
        if a["id"] == b["id"]:
            raise RcmvsError(f"{pi}: image {a['id']} is listed twice")
    E, C, K = np.zeros((n, 4, 4)), np.zeros((n, 3)), np.zeros((n, 3, 3))
    sizes, offsets, lists = np.zeros((n, 2), dtype=np.int64), np.zeros(n + 1, dtype=np.int64), []
    D, models = np.zeros((n, 8)), []
    for k, im in enumerate(imgs):
        if im["camera_id"] not in cams:
            raise RcmvsError(f"{pi}: image {im['id']} ({im['name']}): unknown camera id {im['camera_id']}")
        cam = cams[im["camera_id"]]
        try:
            R = qvec_to_rotmat(im["qvec"])
        except RcmvsError:
            raise RcmvsError(f"{pi}: image {im['id']} ({im['name']}): zero quaternion") from None
        E[k, :3, :3], E[k, :3, 3], E[k, 3, 3] = R, im["tvec"], 1.0
        C[k], K[k], sizes[k] = camera_centre(R, im["tvec"]), intrinsic_matrix(cam), (cam["width"], cam["height"])
        D[k] = distortion_row(cam)
        models.append(cam["model"])
        seen = im["points2D"]["id"]
        seen = np.unique(seen[seen != -1])
        at = np.searchsorted(pids, seen)
        bad = (at >= len(pids)) | (pids[np.minimum(at, max(len(pids) - 1, 0))] != seen) if len(pids) else np.ones(len(seen), dtype=bool)
        if bad.any():
            raise RcmvsError(f"{pi}: image {im['id']} ({im['name']}): observation of unknown point {int(seen[bad][0])}")
        lists.append(at.astype(np.int32))
        offsets[k + 1] = offsets[k] + len(at)
    M = {"image_ids": np.array([im["id"] for im in imgs], dtype=np.int64), "names": [im["name"] for im in imgs],
         "camera_ids": np.array([im["camera_id"] for im in imgs], dtype=np.int64),
         "qvec": np.array([im["qvec"] for im in imgs], dtype=np.float64).reshape(n, 4),
         "tvec": np.array([im["tvec"] for im in imgs], dtype=np.float64).reshape(n, 3),
         "extrinsics": E, "centres": C, "intrinsics": K, "sizes": sizes, "point_ids": pids, "points": xyz, "offsets": offsets,
         "ids": np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, dtype=np.int32),
         "files": {"cameras": pc, "images": pi, "points3D": pp}}
    if distortion:
        M["distortion"], M["models"] = D, models
    return M
