"""Normals of a triangle mesh on the HIP path (csrc/mesh_normals.hip; the contract and the rule are csrc/mesh_normals.h, the
per-element rules csrc/mesh_normals_math.h, restated by tests/mesh_normals_oracle.py): unit face normals, oriented per-vertex normals
under two weights, and the normal pass over views that ``mesh_render.render`` produced (a camera-frame normal map, a smooth headlight
shade and a colour-coded normal image).

``vertex_normals`` takes what ``TsdfVolume.extract``, ``mesh_clean.clean_mesh`` or ``mesh_decimate.decimate`` give (device tensors).
The extracted meshes are oriented from the inside to the outside, so the sum of a vertex's face vectors points out with no extra
work.  ``weight="area"`` sums the face vectors (an area-weighted mean); ``weight="sphere"`` uses Max's weights, which are exact for
vertices on a sphere and involve no transcendental function.  A vertex's corners are added one by one in a fixed order, in fp64,
with no floating-point atomic: every output is a function of the inputs alone.

    python -m rc_mvsnet_amd.mesh_normals --in a.ply --out b.ply --weight sphere

Limits: one lane walks the corners of a vertex (the fixed order forbids a tree); no crease angle and no splitting at sharp edges;
on inconsistently oriented input the normals cancel (such vertices are counted); 3 nf <= 2^31 - 256.  No CPU fallback."""
import argparse
import ctypes
import json

import numpy as np
import torch

from . import _lib, fusion
from .mesh_clean import _count, _mesh, _ptr, _real, _scan_work

STATS, MAX_CORNERS, SORT_BLOCK = (_lib.CONSTANTS["RCMVS_MN_" + k] for k in ("STATS", "MAX_CORNERS", "SORT_BLOCK"))
WEIGHTS = {"area": _lib.CONSTANTS["RCMVS_MN_WEIGHT_AREA"], "sphere": _lib.CONSTANTS["RCMVS_MN_WEIGHT_SPHERE"]}
PHASES = {k.lower(): _lib.CONSTANTS["RCMVS_MN_PHASE_" + k] for k in ("ALL", "INCIDENCE", "ACCUMULATE")}
STAT_NAMES = ("faces_invalid", "faces_nonfinite", "faces_degenerate", "corners_skipped", "vertices_with_normal", "vertices_unreferenced",
              "vertices_cancelled")
DEFAULT_NEAR = 1e-6                                              # mesh_render.DEFAULT_NEAR


def _sizes(verts, faces, what):
    nv, nf = _mesh(verts, faces, None, what)
    if 3 * nf > MAX_CORNERS:
        raise _lib.RcmvsError(f"{what}: {nf} faces (at most (2^31-256) / 3)")
    return nv, nf


def _weight(weight, what):
    if weight not in WEIGHTS:
        raise _lib.RcmvsError(f"{what}: weight = {weight!r} ('area' or 'sphere')")
    return WEIGHTS[weight]


def face_normals(verts, faces, _timed=None):
    """verts (nv,3) fp32, faces (nf,3) int32 on the device -> (nf,3) fp32 unit normals (b - a) x (c - a), zero for a face that is
    invalid, has a non-finite coordinate or no area"""
    what = "mesh_normals.face_normals"
    nv, nf = _sizes(verts, faces, what)
    out = torch.empty((nf, 3), device=verts.device, dtype=torch.float32)
    args = [_ptr(verts, "verts", torch.float32), _ptr(faces, "faces", torch.int32), nv, nf, _ptr(out, "face_normals", torch.float32)]
    if _timed is None:
        _lib.call("rcmvs_mn_face_normals", *args, fusion._stream())
    else:
        _lib.call("rcmvs_mn_face_normals_timed", *args, PHASES[_timed[0]], _timed[1], _timed[2], fusion._stream())
    return out


def vertex_normals_device(verts, faces, weight="area", _timed=None):
    """-> (normals (nv,3) fp32, stats (STATS,) int64), both on the device; nothing is read back"""
    what = "mesh_normals.vertex_normals"
    nv, nf = _sizes(verts, faces, what)
    w = _weight(weight, what)
    dev, n = verts.device, 3 * nf
    table = 256 * ((n + SORT_BLOCK - 1) // SORT_BLOCK)
    key = [torch.empty(n, device=dev, dtype=torch.int32) for _ in range(2)]
    idx = [torch.empty(n, device=dev, dtype=torch.int32) for _ in range(2)]
    hist, hist_start = torch.empty(table, device=dev, dtype=torch.int32), torch.empty(table + 1, device=dev, dtype=torch.int32)
    work = _scan_work(max(table, n), dev)
    seg = torch.empty(2 * nv, device=dev, dtype=torch.int32)
    normals = torch.empty((nv, 3), device=dev, dtype=torch.float32)
    stats = torch.empty(STATS, device=dev, dtype=torch.int64)
    args = [_ptr(verts, "verts", torch.float32), _ptr(faces, "faces", torch.int32), nv, nf, w, _ptr(key[0], "key_a", torch.int32),
            _ptr(idx[0], "idx_a", torch.int32), _ptr(key[1], "key_b", torch.int32), _ptr(idx[1], "idx_b", torch.int32), _ptr(hist, "hist", torch.int32),
            _ptr(hist_start, "hist_start", torch.int32), _ptr(work, "scan_work", torch.int32), _ptr(seg, "seg", torch.int32),
            _ptr(normals, "normals", torch.float32), fusion._chk(stats, "stats", torch.int64)]
    if _timed is None:
        _lib.call("rcmvs_mn_vertex_normals", *args, fusion._stream())
    else:
        _lib.call("rcmvs_mn_vertex_normals_timed", *args, PHASES[_timed[0]], _timed[1], _timed[2], fusion._stream())
    return normals, stats


def stats_dict(stats, weight):
    """the device counters -> a dict of STAT_NAMES with the weight (one host read)"""
    return dict({"weight": weight}, **dict(zip(STAT_NAMES, (int(x) for x in stats.cpu().tolist()))))


def vertex_normals(verts, faces, weight="area"):
    """verts (nv,3) fp32, faces (nf,3) int32 on the device; weight 'area' (the sum of the face vectors) or 'sphere' (Max's weights)
    -> (normals (nv,3) fp32 on the device, stats).  A vertex no usable face refers to has a zero normal and is counted as
    unreferenced; one whose corners cancel has a zero normal and is counted as cancelled.  Faces with a non-finite coordinate
    contribute nothing, so a NaN does not reach a neighbour's normal."""
    normals, stats = vertex_normals_device(verts, faces, weight)
    return normals, stats_dict(stats, weight)


def shade(verts, faces, normals, cams, face_image, near=DEFAULT_NEAR, background=(0, 0, 0), _timed=None):
    """The normal pass over rendered views.  normals: (nv,3) fp32 of ``vertex_normals``; cams (V,16) float64 on the host, near as
    given to ``mesh_render.render``; face_image: the render's "face" (V,H,W) int32 -> dict of device tensors: normal (V,H,W,3) fp32,
    the interpolated unit normal in the camera frame (zero where no face is seen); smooth (V,H,W) uint8, the headlight shade of
    that normal; normal_rgb (V,H,W,3) uint8, its colour code ((128, 128, 255) faces the camera; ``background`` where no face is
    seen, (128, 128, 128) where the interpolated normal vanishes)."""
    what = "mesh_normals.shade"
    nv, nf = _sizes(verts, faces, what)
    if not torch.is_tensor(normals) or normals.dtype != torch.float32 or tuple(normals.shape) != (nv, 3) or normals.device != verts.device:
        raise _lib.RcmvsError(f"{what}: normals must be an ({nv},3) float32 tensor on the mesh's device")
    if not torch.is_tensor(face_image) or face_image.dtype != torch.int32 or face_image.dim() != 3 or face_image.device != verts.device:
        raise _lib.RcmvsError(f"{what}: face_image must be a (V,H,W) int32 tensor on the mesh's device")
    cams = np.ascontiguousarray(np.asarray(cams, dtype=np.float64).reshape(-1, 16))
    V, H, W = (int(s) for s in face_image.shape)
    if len(cams) != V or V < 1 or H < 1 or W < 1:
        raise _lib.RcmvsError(f"{what}: {len(cams)} cameras for a face_image of {(V, H, W)} (one camera per view, at least one pixel)")
    near = _real(near, "near", what)
    if not near > 0:
        raise _lib.RcmvsError(f"{what}: near = {near} (finite and > 0)")
    bg = [_count(c, "background", what) for c in background]
    if len(bg) != 3 or max(bg) > 255:
        raise _lib.RcmvsError(f"{what}: background = {background!r} (three bytes)")
    dev = verts.device
    out = {"normal": torch.empty((V, H, W, 3), device=dev, dtype=torch.float32), "smooth": torch.empty((V, H, W), device=dev, dtype=torch.uint8),
           "normal_rgb": torch.empty((V, H, W, 3), device=dev, dtype=torch.uint8)}
    args = [_ptr(verts, "verts", torch.float32), _ptr(faces, "faces", torch.int32), _ptr(normals, "normals", torch.float32), nv, nf, V, H, W,
            cams.ctypes.data_as(ctypes.c_void_p), near, fusion._chk(face_image, "face_image", torch.int32), bg[0] | bg[1] << 8 | bg[2] << 16,
            fusion._chk(out["normal"], "normal_map"), fusion._chk(out["smooth"], "smooth", torch.uint8), fusion._chk(out["normal_rgb"], "normal_rgb", torch.uint8)]
    if _timed is None:
        _lib.call("rcmvs_mn_shade", *args, fusion._stream())
    else:
        _lib.call("rcmvs_mn_shade_timed", *args, PHASES[_timed[0]], _timed[1], _timed[2], fusion._stream())
    return out


def normals_options(weight=None):
    """The mesh path's option (``--normals area|sphere``) -> {"weight": ...} for the ``normals`` keyword, or None when it asks for
    nothing"""
    if weight is None or weight is False or weight == "":
        return None
    _weight(weight, "normals")
    return {"weight": weight}


def main(argv=None):
    from . import dtu_io, tsdf_mesh
    ap = argparse.ArgumentParser(description="add oriented per-vertex normals to a PLY mesh")
    ap.add_argument("--in", dest="src", required=True, help="the PLY to read (positions, triangles, vertex colours when it has them)")
    ap.add_argument("--out", required=True, help="the PLY to write: x y z nx ny nz red green blue")
    ap.add_argument("--weight", choices=sorted(WEIGHTS), default="area")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    verts, faces, rgb = dtu_io.read_ply_mesh_rgb(a.src)
    dev = torch.device(a.device)
    v = torch.from_numpy(np.ascontiguousarray(verts, np.float32)).to(dev)
    f = torch.from_numpy(np.ascontiguousarray(faces, np.int32)).to(dev)
    normals, stats = vertex_normals(v, f, a.weight)
    with open(a.out, "wb") as out:
        out.write(tsdf_mesh.mesh_ply_bytes(v, f, None if rgb is None else np.ascontiguousarray(rgb, np.uint8), normals=normals))
    summary = dict({"in": a.src, "out": a.out, "vertices": int(v.shape[0]), "faces": int(f.shape[0])}, **stats)
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
