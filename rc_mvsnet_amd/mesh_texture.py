"""A texture atlas for a triangle mesh from the images of a scan on the HIP path (csrc/mesh_texture.hip; the contract is
csrc/mesh_texture.h, the per-element rules csrc/mesh_texture_math.h, restated by tests/mesh_texture_oracle.py).

``texture`` renders the mesh into the views with ``mesh_render.render`` (a chunk of views at a time; the chunk size changes no bit),
lets every face vote for the eligible view that sees most of its samples, gives it a square cell whose side is a power of two chosen
from its longest edge in that view, lays the cells out along a Morton curve in descending size (no packing search, no overlap), and
fills every texel from the chosen view's image by bilinear interpolation in fp64.  Decisions are integers, the arithmetic is fp64 in
a stated order, the only atomic is an integer add: every output is a function of the inputs alone.

    python -m rc_mvsnet_amd.mesh_texture --mesh a.ply --pair-folder data/scan9 --scan-folder data/scan9 --out b.ply --size 1184 1600

Limits: per-face charts, so every edge is a seam under mip-mapping; no gutter along the legs of a chart (only along its diagonal);
no colour levelling between views and no smoothness term in the view choice; visibility at one sample per pixel, so a face that
owns no sample in any eligible view is unseen and keeps its vertex colours; the right angle of a chart is always at corner a, so thin
faces are stretched; most useful after decimation, where vertex colours have lost the detail.  No CPU fallback."""
import argparse
import ctypes
import json
import os

import numpy as np
import torch

from . import _lib, fusion, mesh_render
from .mesh_clean import _count, _mesh, _ptr, _real, _scan_work

MIN_CLASS, MAX_CLASS, MAX_SHIFT, MAX_ATLAS, MAX_FACES, STATS, TABLE, SORT_BLOCK = (_lib.CONSTANTS["RCMVS_MT_" + k] for k in (
    "MIN_CLASS", "MAX_CLASS", "MAX_SHIFT", "MAX_ATLAS", "MAX_FACES", "STATS", "TABLE", "SORT_BLOCK"))
PHASE_ALL = _lib.CONSTANTS["RCMVS_MT_PHASE_ALL"]
STAT_NAMES = ("faces_seen", "faces_unseen", "faces_invalid", "faces_capped", "texels_image", "texels_vertex", "texels_fallback")
PER_CLASS = 8                                                    # stats[PER_CLASS + k]: the faces of class k
T_TOTAL = 4 * (MAX_CLASS + 1)                                    # table[4 k ..]: start, faces, cells, base of class k; then total, m, S, Sy
DEFAULT_NEAR = mesh_render.DEFAULT_NEAR
DEFAULT_MAX_SIZE = 8192
DEFAULT_CHUNK = 4


def _sizes(verts, faces, rgb, what):
    nv, nf = _mesh(verts, faces, rgb, what)
    if nf > MAX_FACES:
        raise _lib.RcmvsError(f"{what}: {nf} faces (at most 2^30-256)")
    return nv, nf


def _cams(cams, what):
    cams = np.ascontiguousarray(np.asarray(cams, dtype=np.float64).reshape(-1, 16))
    if len(cams) < 1:
        raise _lib.RcmvsError(f"{what}: no views (cams must hold at least one row of 16)")
    return cams


def _near(near, what):
    near = _real(near, "near", what)
    if not near > 0:
        raise _lib.RcmvsError(f"{what}: near = {near} (finite and > 0)")
    return near


def _background(background, what):
    bg = [_count(c, "background", what) for c in background]
    if len(bg) != 3 or max(bg) > 255:
        raise _lib.RcmvsError(f"{what}: background = {background!r} (three bytes)")
    return bg[0] | bg[1] << 8 | bg[2] << 16


def _call(name, args, _timed):
    if _timed is None:
        _lib.call(name, *args, fusion._stream())
    else:
        _lib.call(name + "_timed", *args, PHASE_ALL, _timed[0], _timed[1], fusion._stream())


def vote(verts, faces, face_image, cams, near=DEFAULT_NEAR, first_view=0, best=None, _timed=None):
    """face_image: (n,H,W) int32, the "face" of ``mesh_render.render`` for the n views whose cameras are cams (n,16) on the host and
    whose numbers are first_view .. first_view + n - 1; best: the (nf,) int64 tensor of an earlier call over other views, or None
    -> best (count << 32 | 0xFFFFFFFF - view per face, 0 = unseen; read it as uint64)."""
    what = "mesh_texture.vote"
    nv, nf = _sizes(verts, faces, None, what)
    cams = _cams(cams, what)
    if not torch.is_tensor(face_image) or face_image.dtype != torch.int32 or face_image.dim() != 3 or face_image.device != verts.device:
        raise _lib.RcmvsError(f"{what}: face_image must be an (n,H,W) int32 tensor on the mesh's device")
    n, H, W = (int(s) for s in face_image.shape)
    if len(cams) != n or H < 1 or W < 1:
        raise _lib.RcmvsError(f"{what}: {len(cams)} cameras for a face_image of {(n, H, W)} (one camera per view, at least one pixel)")
    near, first_view = _near(near, what), _count(first_view, "first_view", what)
    reset = best is None
    if reset:
        best = torch.empty(nf, device=verts.device, dtype=torch.int64)
    elif not torch.is_tensor(best) or best.dtype != torch.int64 or tuple(best.shape) != (nf,) or best.device != verts.device:
        raise _lib.RcmvsError(f"{what}: best must be an ({nf},) int64 tensor on the mesh's device")
    count = torch.empty(nf, device=verts.device, dtype=torch.int32)
    args = [_ptr(verts, "verts", torch.float32), _ptr(faces, "faces", torch.int32), nv, nf, n, H, W, cams.ctypes.data_as(ctypes.c_void_p), near,
            fusion._chk(face_image, "face_image", torch.int32), first_view, int(reset), _ptr(count, "count", torch.int32), _ptr(best, "best", torch.int64)]
    _call("rcmvs_mt_vote", args, _timed)
    return best


def layout(verts, faces, best, cams, H, W, near=DEFAULT_NEAR, shift=0, _timed=None):
    """best: ``vote``'s; cams: all V cameras (host rows or a (V,16) float64 device tensor) -> dict of device tensors: klass (nf,) int32,
    order (nf,) int32 (the faces sorted by descending class, a class in face order, invalid faces last), table (TABLE,) int64,
    texel (nf,3,2) int32 and stats (STATS,) int64.  Nothing is read back (``table_dict`` does that)."""
    what = "mesh_texture.layout"
    nv, nf = _sizes(verts, faces, None, what)
    dev = verts.device
    cams_dev = cams if torch.is_tensor(cams) else torch.from_numpy(_cams(cams, what).copy()).to(dev)
    if cams_dev.dtype != torch.float64 or cams_dev.dim() != 2 or cams_dev.shape[1] != 16 or cams_dev.shape[0] < 1 or cams_dev.device != dev:
        raise _lib.RcmvsError(f"{what}: cams must be (V,16) float64 rows, on the host or on the mesh's device")
    V = int(cams_dev.shape[0])
    H, W, near, shift = _count(H, "H", what), _count(W, "W", what), _near(near, what), _count(shift, "shift", what)
    if shift > MAX_SHIFT:
        raise _lib.RcmvsError(f"{what}: shift = {shift} (0 .. {MAX_SHIFT})")
    if not torch.is_tensor(best) or best.dtype != torch.int64 or tuple(best.shape) != (nf,) or best.device != dev:
        raise _lib.RcmvsError(f"{what}: best must be an ({nf},) int64 tensor on the mesh's device")
    cells = 256 * ((nf + SORT_BLOCK - 1) // SORT_BLOCK)
    i32 = lambda n: torch.empty(n, device=dev, dtype=torch.int32)            # noqa: E731
    out = {"klass": i32(nf), "order": i32(nf), "table": torch.empty(TABLE, device=dev, dtype=torch.int64), "texel": torch.empty((nf, 3, 2), device=dev, dtype=torch.int32),
           "stats": torch.empty(STATS, device=dev, dtype=torch.int64), "cams": cams_dev, "shift": shift}
    key_a, idx_a, key_b, hist, hist_start, work = i32(nf), i32(nf), i32(nf), i32(cells), i32(cells + 1), _scan_work(max(cells, nf), dev)
    args = [_ptr(verts, "verts", torch.float32), _ptr(faces, "faces", torch.int32), nv, nf, V, H, W, fusion._chk(cams_dev, "cams", torch.float64), near,
            _ptr(best, "best", torch.int64), shift, _ptr(out["klass"], "klass", torch.int32), _ptr(key_a, "key_a", torch.int32), _ptr(idx_a, "idx_a", torch.int32),
            _ptr(key_b, "key_b", torch.int32), _ptr(out["order"], "order", torch.int32), _ptr(hist, "hist", torch.int32), _ptr(hist_start, "hist_start", torch.int32),
            _ptr(work, "scan_work", torch.int32), fusion._chk(out["table"], "table", torch.int64), _ptr(out["texel"], "texel", torch.int32),
            fusion._chk(out["stats"], "stats", torch.int64)]
    _call("rcmvs_mt_layout", args, _timed)
    return out


def table_dict(table):
    """the device table -> {"classes": {k: {start, faces, cells, base}}, "total", "m", "S", "Sy"} (one host read)"""
    t = [int(x) for x in table.cpu().tolist()]
    return {"classes": {k: dict(zip(("start", "faces", "cells", "base"), t[4 * k:4 * k + 4])) for k in range(MIN_CLASS, MAX_CLASS + 1)},
            "total": t[T_TOTAL], "m": t[T_TOTAL + 1], "S": t[T_TOTAL + 2], "Sy": t[T_TOTAL + 3]}


def fill(verts, faces, rgb, images, best, lay, S, Sy, near=DEFAULT_NEAR, background=(0, 0, 0), _timed=None):
    """images: (V,H,W,3) uint8 on the device; lay: ``layout``'s result; S, Sy: the atlas size its table states -> (atlas (Sy,S,3) uint8,
    owner (Sy,S) int32: the face of each texel, -1 for background).  The texel counters of lay["stats"] are filled."""
    what = "mesh_texture.fill"
    nv, nf = _sizes(verts, faces, rgb, what)
    dev = verts.device
    if not torch.is_tensor(images) or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3 or images.device != dev:
        raise _lib.RcmvsError(f"{what}: images must be a (V,H,W,3) uint8 tensor on the mesh's device")
    V, H, W = (int(s) for s in images.shape[:3])
    if V != int(lay["cams"].shape[0]) or V < 1 or H < 1 or W < 1:
        raise _lib.RcmvsError(f"{what}: {V} images of {(H, W)} for {int(lay['cams'].shape[0])} cameras (one image per view, at least one pixel)")
    S, Sy, near, bg = _count(S, "S", what), _count(Sy, "Sy", what), _near(near, what), _background(background, what)
    if not 1 <= S <= MAX_ATLAS:
        raise _lib.RcmvsError(f"{what}: S = {S} (1 .. {MAX_ATLAS})")
    atlas = torch.empty((Sy, S, 3), device=dev, dtype=torch.uint8)
    owner = torch.empty((Sy, S), device=dev, dtype=torch.int32)
    args = [_ptr(verts, "verts", torch.float32), _ptr(rgb, "rgb", torch.uint8), _ptr(faces, "faces", torch.int32), nv, nf, V, H, W,
            fusion._chk(lay["cams"], "cams", torch.float64), near, fusion._chk(images, "images", torch.uint8), _ptr(best, "best", torch.int64),
            _ptr(lay["order"], "order", torch.int32), fusion._chk(lay["table"], "table", torch.int64), S, Sy, bg, fusion._chk(atlas, "atlas", torch.uint8),
            fusion._chk(owner, "owner", torch.int32), fusion._chk(lay["stats"], "stats", torch.int64)]
    _call("rcmvs_mt_fill", args, _timed)
    return atlas, owner


def shade(verts, faces, cams, face_image, texel, atlas, near=DEFAULT_NEAR, background=(0, 0, 0), _timed=None):
    """The textured pass over rendered views.  cams (V,16) float64 on the host, near as given to ``mesh_render.render``; face_image:
    the render's "face" (V,H,W) int32; texel (nf,3,2) int32 and atlas (Sy,S,3) uint8 of ``texture`` -> tex_rgb (V,H,W,3) uint8:
    the atlas sampled bilinearly at each pixel's perspective-correct texel position, ``background`` where no face is seen."""
    what = "mesh_texture.shade"
    nv, nf = _sizes(verts, faces, None, what)
    dev = verts.device
    if not torch.is_tensor(face_image) or face_image.dtype != torch.int32 or face_image.dim() != 3 or face_image.device != dev:
        raise _lib.RcmvsError(f"{what}: face_image must be a (V,H,W) int32 tensor on the mesh's device")
    if not torch.is_tensor(texel) or texel.dtype != torch.int32 or tuple(texel.shape) != (nf, 3, 2) or texel.device != dev:
        raise _lib.RcmvsError(f"{what}: texel must be an ({nf},3,2) int32 tensor on the mesh's device")
    if not torch.is_tensor(atlas) or atlas.dtype != torch.uint8 or atlas.dim() != 3 or atlas.shape[2] != 3 or atlas.device != dev:
        raise _lib.RcmvsError(f"{what}: atlas must be an (Sy,S,3) uint8 tensor on the mesh's device")
    cams = _cams(cams, what)
    V, H, W = (int(s) for s in face_image.shape)
    if len(cams) != V or H < 1 or W < 1:
        raise _lib.RcmvsError(f"{what}: {len(cams)} cameras for a face_image of {(V, H, W)} (one camera per view, at least one pixel)")
    near, bg = _near(near, what), _background(background, what)
    Sy, S = int(atlas.shape[0]), int(atlas.shape[1])
    out = torch.empty((V, H, W, 3), device=dev, dtype=torch.uint8)
    args = [_ptr(verts, "verts", torch.float32), _ptr(faces, "faces", torch.int32), nv, nf, V, H, W, cams.ctypes.data_as(ctypes.c_void_p), near,
            fusion._chk(face_image, "face_image", torch.int32), _ptr(texel, "texel", torch.int32), fusion._chk(atlas, "atlas", torch.uint8), S, Sy, bg,
            fusion._chk(out, "tex_rgb", torch.uint8)]
    _call("rcmvs_mt_shade", args, _timed)
    return out


def stats_dict(stats):
    """the device counters -> a dict of STAT_NAMES and "faces_per_class" (one host read)"""
    s = [int(x) for x in stats.cpu().tolist()]
    return dict(dict(zip(STAT_NAMES, s)), faces_per_class={k: s[PER_CLASS + k] for k in range(MIN_CLASS, MAX_CLASS + 1)})


def texcoords(texel, S, Sy):
    """texel (nf,3,2) int32 -> (nf,3,2) float32 on the host: u = (x + 0.5) / S, v = 1 - (y + 0.5) / Sy (v up, as viewers read it)"""
    t = (texel.cpu().numpy() if torch.is_tensor(texel) else np.asarray(texel)).astype(np.float64).reshape(-1, 3, 2)
    return np.stack([(t[..., 0] + 0.5) / float(S), 1.0 - (t[..., 1] + 0.5) / float(Sy)], -1).astype(np.float32)


def _max_size(max_size, what):
    max_size = _count(max_size, "max_size", what)
    if not 1 <= max_size <= MAX_ATLAS:
        raise _lib.RcmvsError(f"{what}: max_size = {max_size} (1 .. {MAX_ATLAS})")
    return max_size


def texture(verts, faces, rgb, images, cams, near=DEFAULT_NEAR, max_size=DEFAULT_MAX_SIZE, shift=0, chunk=DEFAULT_CHUNK, cull="none", background=(0, 0, 0),
            face_images=None):
    """verts (nv,3) fp32, faces (nf,3) int32, rgb (nv,3) uint8 or None on the device; images (V,H,W,3) uint8 on the device; cams (V,16)
    float64 on the host, pixel centres at integers.  face_images: None, or the (V,H,W) int32 "face" of renders the caller already has
    (they are then not rendered again; the numbers are never trusted as addresses).  shift: halve the texel density per unit (0 .. 8); when the atlas would be wider
    than max_size the shift is raised until it fits, and a mesh that does not fit at shift 8 is refused with the size it needs.
    chunk: the views rendered at a time.  -> dict: atlas (Sy,S,3) uint8, owner (Sy,S) int32, texel (nf,3,2) int32, best (nf,) int64,
    klass, order (device tensors), uv (nf,3,2) float32 on the host, table (``table_dict``), stats (``stats_dict``), shift, size (Sy, S)."""
    what = "mesh_texture.texture"
    nv, nf = _sizes(verts, faces, rgb, what)
    cams = _cams(cams, what)
    if not torch.is_tensor(images) or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3 or images.device != verts.device:
        raise _lib.RcmvsError(f"{what}: images must be a (V,H,W,3) uint8 tensor on the mesh's device")
    V, H, W = (int(s) for s in images.shape[:3])
    if V != len(cams) or H < 1 or W < 1:
        raise _lib.RcmvsError(f"{what}: {V} images of {(H, W)} for {len(cams)} cameras (one image per view, at least one pixel)")
    max_size, shift, chunk, near = _max_size(max_size, what), _count(shift, "shift", what), _count(chunk, "chunk", what), _near(near, what)
    if shift > MAX_SHIFT:
        raise _lib.RcmvsError(f"{what}: shift = {shift} (0 .. {MAX_SHIFT})")
    if chunk < 1:
        raise _lib.RcmvsError(f"{what}: chunk = {chunk} (at least 1)")
    _background(background, what)
    images = images.contiguous()
    best = None
    if face_images is not None and (not torch.is_tensor(face_images) or face_images.dtype != torch.int32 or tuple(face_images.shape) != (V, H, W)):
        raise _lib.RcmvsError(f"{what}: face_images must be a ({V},{H},{W}) int32 tensor")
    for v0 in range(0, V, chunk):
        seen = face_images[v0:v0 + chunk].contiguous() if face_images is not None else \
            mesh_render.render(verts, faces, rgb, cams[v0:v0 + chunk], H, W, near=near, cull=cull)["face"]
        best = vote(verts, faces, seen, cams[v0:v0 + chunk], near, first_view=v0, best=best)
    cams_dev = torch.from_numpy(cams.copy()).to(verts.device)
    while True:
        lay = layout(verts, faces, best, cams_dev, H, W, near, shift)
        table = table_dict(lay["table"])
        if table["S"] <= max_size:
            break
        if shift == MAX_SHIFT:
            raise _lib.RcmvsError(f"{what}: the atlas needs {table['S']} x {table['Sy']} texels at shift {MAX_SHIFT} (max_size = {max_size})")
        shift += 1
    S, Sy = table["S"], table["Sy"]
    atlas, owner = fill(verts, faces, rgb, images, best, lay, S, Sy, near, background)
    return {"atlas": atlas, "owner": owner, "texel": lay["texel"], "best": best, "klass": lay["klass"], "order": lay["order"], "uv": texcoords(lay["texel"], S, Sy),
            "table": table, "stats": stats_dict(lay["stats"]), "shift": shift, "size": (Sy, S)}


def summary(tex):
    """the JSON-ready part of ``texture``'s result"""
    return dict(tex["stats"], atlas=[int(tex["size"][0]), int(tex["size"][1])], shift=tex["shift"], texels=tex["table"]["total"])


def write_obj(path, verts, faces, uv, texture_file):
    """<path> (Wavefront OBJ) and its .mtl next to it: v, vt (three per face), f a/ta b/tb c/tc (1-based); texture_file: the PNG's
    name as the .mtl refers to it"""
    verts = (verts.cpu().numpy() if torch.is_tensor(verts) else np.asarray(verts)).reshape(-1, 3)
    faces = (faces.cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)).reshape(-1, 3)
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    if len(uv) != 3 * len(faces):
        raise _lib.RcmvsError(f"mesh_texture.write_obj: {len(uv)} texture coordinates for {len(faces)} faces (three per face)")
    stem = os.path.splitext(os.path.basename(path))[0]
    lines = [f"mtllib {stem}.mtl", "usemtl textured"]
    lines += ["v %.9g %.9g %.9g" % tuple(float(x) for x in p) for p in verts]
    lines += ["vt %.9g %.9g" % (float(t[0]), float(t[1])) for t in uv]
    lines += ["f %d/%d %d/%d %d/%d" % (f[0] + 1, 3 * i + 1, f[1] + 1, 3 * i + 2, f[2] + 1, 3 * i + 3) for i, f in enumerate(faces.tolist())]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as out:
        out.write("\n".join(lines) + "\n")
    with open(os.path.join(os.path.dirname(os.path.abspath(path)), stem + ".mtl"), "w") as out:
        out.write(f"newmtl textured\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 0\nmap_Kd {texture_file}\n")


def write_textured(path, verts, faces, rgb, tex, normals=None, obj=False):
    """<path>.ply with per-face texcoords and ``comment TextureFile``, the atlas as <stem>.png next to it, with obj also <stem>.obj
    and <stem>.mtl -> the names written"""
    from . import tsdf_mesh
    from .depth_vis import save_png
    stem = os.path.splitext(os.path.abspath(path))[0]
    png = os.path.basename(stem) + ".png"
    data = tsdf_mesh.mesh_ply_bytes(verts, faces, rgb, normals=normals, texcoords=tex["uv"], texture_file=png)
    os.makedirs(os.path.dirname(stem), exist_ok=True)
    with open(path, "wb") as out:
        out.write(data)
    save_png(stem + ".png", tex["atlas"])
    written = [path, stem + ".png"]
    if obj:
        write_obj(stem + ".obj", verts, faces, tex["uv"], png)
        written += [stem + ".obj", stem + ".mtl"]
    return written


def read_textured(path, device):
    """A PLY that ``write_textured`` wrote and the atlas its ``comment TextureFile`` names, next to it -> (verts, faces, rgb or None,
    atlas (Sy,S,3) uint8, texel (nf,3,2) int32) on the device.  The texel centres are recovered exactly: u = (x + 0.5) / S with S a
    power of two at most 2^14 is a float32 without rounding, and so is v."""
    from PIL import Image
    from . import dtu_io
    v, f, c, _, uv, name = dtu_io.read_ply_mesh_texture(path)
    if uv is None or name is None:
        raise _lib.RcmvsError(f"mesh_texture.read_textured: {path} has no texcoords or no `comment TextureFile`")
    with Image.open(os.path.join(os.path.dirname(os.path.abspath(path)), name)) as im:
        atlas = np.ascontiguousarray(np.asarray(im.convert("RGB"), np.uint8))
    Sy, S = atlas.shape[:2]
    t = uv.astype(np.float64)
    texel = np.stack([np.rint(t[..., 0] * S - 0.5), np.rint((1.0 - t[..., 1]) * Sy - 0.5)], -1).astype(np.int32)
    dev = torch.device(device)
    put = lambda x: torch.from_numpy(np.array(x)).to(dev)                        # noqa: E731
    return put(v.astype(np.float32)), put(f.astype(np.int32)), None if c is None else put(c.astype(np.uint8)), put(atlas), put(texel)


def texture_options(enabled=False, max_size=None, shift=0):
    """The mesh path's option (``--texture [--texture-size N]``) -> the keywords of ``texture``, or None when it asks for nothing"""
    if not enabled:
        return None
    return {"max_size": _max_size(DEFAULT_MAX_SIZE if max_size is None else max_size, "texture"), "shift": shift}


def load_images(scan_folder, names, size=None):
    """the images S/images/<name>.jpg (or .png) as (V,H,W,3) uint8 on the host, resized to size (H, W) the way
    tsdf_mesh.filtered_views reads them -> (images, (sy, sx)): the factors the intrinsics' rows scale by"""
    from PIL import Image
    out, scale = [], (1.0, 1.0)
    for n in names:
        path = next((p for p in (os.path.join(scan_folder, "images", n + e) for e in (".jpg", ".png")) if os.path.exists(p)), None)
        if path is None:
            raise _lib.RcmvsError(f"mesh_texture: no image {n}.jpg or {n}.png under {os.path.join(scan_folder, 'images')}")
        img = Image.open(path).convert("RGB")
        if size is not None and (img.height, img.width) != tuple(size):
            scale = (size[0] / img.height, size[1] / img.width)
            img = img.resize((int(size[1]), int(size[0])), Image.BILINEAR)
        out.append(np.asarray(img, np.uint8))
    return np.stack(out), scale


def main(argv=None):
    from . import dtu_io, scan_io, tsdf_mesh
    ap = argparse.ArgumentParser(description="texture a PLY mesh from the images of a scan: a PLY with texcoords and its atlas PNG")
    ap.add_argument("--mesh", required=True, help="the PLY to texture")
    ap.add_argument("--pair-folder", required=True, help="folder of pair.txt")
    ap.add_argument("--scan-folder", required=True, help="folder of cams/ and images/")
    ap.add_argument("--out", required=True, help="the PLY to write; the atlas is written next to it as <name>.png")
    ap.add_argument("--size", type=int, nargs=2, default=None, metavar=("H", "W"), help="resize the images (the intrinsics are scaled); default: as stored")
    ap.add_argument("--max-size", type=int, default=DEFAULT_MAX_SIZE)
    ap.add_argument("--shift", type=int, default=0)
    ap.add_argument("--near", type=float, default=DEFAULT_NEAR)
    ap.add_argument("--cull", choices=sorted(mesh_render.CULL), default="none")
    ap.add_argument("--texture-obj", action="store_true", help="also write <name>.obj and <name>.mtl")
    ap.add_argument("--render", default=None, metavar="DIR", help="write the textured views there (render/<view>_tex.png)")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    dev = torch.device(a.device)
    pairs = scan_io.read_pair_file(os.path.join(a.pair_folder, "pair.txt"))
    views = sorted({v for ref, srcs in pairs for v in [ref] + list(srcs)})
    names = ["{:0>8}".format(v) for v in views]
    images, (sy, sx) = load_images(a.scan_folder, names, a.size)
    rows = []
    for n in names:
        K, E = scan_io.read_camera_parameters(os.path.join(a.scan_folder, "cams/{}_cam.txt".format(n)))
        K = np.array(K, np.float64)
        K[0] *= sx
        K[1] *= sy
        rows.append(tsdf_mesh.camera_row(K, E))
    cams = np.stack(rows)
    v, f, c = dtu_io.read_ply_mesh_rgb(a.mesh)
    verts, faces = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (v.astype(np.float32), f.astype(np.int32)))
    rgb = None if c is None else torch.from_numpy(np.ascontiguousarray(c, np.uint8)).to(dev)
    tex = texture(verts, faces, rgb, torch.from_numpy(images).to(dev), cams, near=a.near, max_size=a.max_size, shift=a.shift, cull=a.cull)
    written = write_textured(a.out, verts, faces, rgb, tex, obj=a.texture_obj)
    out = dict({"mesh": a.mesh, "out": a.out, "views": len(names), "vertices": int(verts.shape[0]), "faces": int(faces.shape[0])}, **summary(tex), written=written)
    if a.render is not None:
        H, W = images.shape[1:3]
        r = mesh_render.render(verts, faces, rgb, cams, int(H), int(W), near=a.near, cull=a.cull, texture=(tex["atlas"], tex["texel"]))
        mesh_render.write_views(r, a.render, names)
        out["render"] = a.render
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
