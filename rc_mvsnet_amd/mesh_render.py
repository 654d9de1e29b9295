"""A triangle mesh rendered into the cameras of a scan on the HIP path (csrc/mesh_render.hip; the contract and the rule are
csrc/mesh_render.h, the per-element rules csrc/mesh_render_math.h, restated by tests/mesh_render_oracle.py): per view the depth
map, the number of the face each pixel sees, the interpolated vertex colour and a headlight shade, and the comparison of rendered
depth maps with depth maps of the same views.

``render`` takes what ``TsdfVolume.extract``, ``mesh_clean.clean_mesh`` or ``dtu_io.read_ply_mesh_rgb`` give (device tensors) and
the camera rows of ``tsdf_mesh.camera_row``; ``compare`` fills a table of exact counts and one fp64 sum per view on the device and
reads it once.  Vertices are snapped to a lattice of 1/256 pixel, coverage is decided by int64 edge functions with a top-left rule,
visibility by a 64-bit integer minimum of (depth bits, face number): every output is a function of the inputs alone.

    python -m rc_mvsnet_amd.mesh_render --mesh a.ply --pair-folder data/scan9 --scan-folder data/scan9 --out out/scan9_render \\
        --depth-folder out/scan9

Limits: no near-plane clipping (a face with a vertex nearer than ``near`` or more than 2^16 pixels from the image origin is dropped
and counted as clipped); one sample per pixel, no anti-aliasing; the shade is flat, with a light at the camera; vertex colours unless
``texture`` is given (``--texture``, for a PLY with texcoords); smooth shading only with ``normals`` (``--normals``); H, W <= 16384; pinhole cameras only.  No CPU fallback."""
import argparse
import ctypes
import json
import math
import os

import numpy as np
import torch

from . import _lib, fusion
from .mesh_clean import _count, _mesh, _ptr, _real

MAX_SIDE, SMALL_SIDE, PROJ_BYTES, STATS, TRACE, TABLE, CMP_TILE = (_lib.CONSTANTS["RCMVS_MR_" + k] for k in
                                                                   ("MAX_SIDE", "SMALL_SIDE", "PROJ_BYTES", "STATS", "TRACE", "TABLE", "CMP_TILE"))
CMP_MAX_VIEWS = _lib.CONSTANTS["RCMVS_MR_CMP_MAX_VIEWS"]
CULL = {"none": _lib.CONSTANTS["RCMVS_MR_CULL_NONE"], "back": _lib.CONSTANTS["RCMVS_MR_CULL_BACK"]}
PHASES = {k.lower(): _lib.CONSTANTS["RCMVS_MR_PHASE_" + k] for k in ("ALL", "PROJECT", "SMALL", "LARGE", "RESOLVE")}
STAT_NAMES = ("faces_drawn", "faces_clipped", "faces_degenerate", "faces_culled", "faces_invalid", "faces_large", "pixels_covered")
TRACE_NAMES = ("samples_inside", "atomics_issued", "box_empty", "box_1", "box_2", "box_3_4", "box_5_8", "box_9_16", "box_17_64", "box_above_64")
DEFAULT_NEAR = 1e-6
DEFAULT_THRESHOLDS = (0.001, 0.01, 0.05)
_NULL = ctypes.c_void_p(0)


def _side(value, name, what):
    value = _count(value, name, what)
    if not 1 <= value <= MAX_SIDE:
        raise _lib.RcmvsError(f"{what}: {name} = {value} (1 .. {MAX_SIDE})")
    return value


def _arguments(verts, faces, rgb, cams, H, W, near, cull, background, what):
    nv, nf = _mesh(verts, faces, rgb, what)
    H, W = _side(H, "H", what), _side(W, "W", what)
    cams = np.ascontiguousarray(np.asarray(cams, dtype=np.float64).reshape(-1, 16))
    if len(cams) < 1:
        raise _lib.RcmvsError(f"{what}: no views (cams must hold at least one row of 16)")
    near = _real(near, "near", what)
    if not near > 0:
        raise _lib.RcmvsError(f"{what}: near = {near} (finite and > 0)")
    if cull not in CULL:
        raise _lib.RcmvsError(f"{what}: cull = {cull!r} ('none' or 'back')")
    bg = [_count(c, "background", what) for c in background]
    if len(bg) != 3 or max(bg) > 255:
        raise _lib.RcmvsError(f"{what}: background = {background!r} (three bytes)")
    return nv, nf, H, W, cams, near, CULL[cull], bg[0] | bg[1] << 8 | bg[2] << 16


def render(verts, faces, rgb, cams, H, W, near=DEFAULT_NEAR, cull="none", background=(0, 0, 0), trace=None, _timed=None, normals=None, texture=None):
    """verts (nv,3) fp32, faces (nf,3) int32, rgb (nv,3) uint8 or None on the device; cams (V,16) float64 on the host, the rows of
    tsdf_mesh.camera_row; cull 'none' or 'back' (back: only faces whose normal (b - a) x (c - a) points at the camera, which is how
    the extracted meshes are oriented) -> dict of device tensors: depth (V,H,W) fp32 (0 where no face is seen), face (V,H,W) int32
    (-1 there), rgb (V,H,W,3) uint8 (white faces without vertex colours, ``background`` where no face is seen), shade (V,H,W) uint8,
    keys (V,H,W) int64 (depth bits << 32 | face number, -1 where no face is seen) and stats (V, STATS) int64, the counters of
    STAT_NAMES per view (``stats_rows`` reads them).  trace: None, or a TRACE int64 device tensor that the call adds to
    (TRACE_NAMES).  _timed: (phase name, ev0, ev1) for tools/mesh_render_bench.py.  normals: None, or the (nv,3) fp32 vertex normals
    of mesh_normals.vertex_normals; the result then gains normal (V,H,W,3) fp32, smooth (V,H,W) uint8 and normal_rgb (V,H,W,3) uint8
    of mesh_normals.shade.  texture: None, or (atlas (Sy,S,3) uint8, texel (nf,3,2) int32) of mesh_texture.texture; the result then gains
    tex_rgb (V,H,W,3) uint8 of mesh_texture.shade."""
    what = "mesh_render.render"
    nv, nf, H, W, cams, near, cull, bg = _arguments(verts, faces, rgb, cams, H, W, near, cull, background, what)
    V, dev = len(cams), verts.device
    proj = torch.empty(max(nv, 1) * PROJ_BYTES // 8, device=dev, dtype=torch.int64)
    work = torch.empty(nf + 1, device=dev, dtype=torch.int32)
    out = {"depth": torch.empty((V, H, W), device=dev, dtype=torch.float32), "face": torch.empty((V, H, W), device=dev, dtype=torch.int32),
           "rgb": torch.empty((V, H, W, 3), device=dev, dtype=torch.uint8), "shade": torch.empty((V, H, W), device=dev, dtype=torch.uint8),
           "keys": torch.empty((V, H, W), device=dev, dtype=torch.int64), "stats": torch.empty((V, STATS), device=dev, dtype=torch.int64)}
    if trace is not None and (trace.dtype != torch.int64 or trace.numel() != TRACE):
        raise _lib.RcmvsError(f"{what}: trace must be {TRACE} int64")
    args = [_ptr(verts, "verts", torch.float32), _ptr(rgb, "rgb", torch.uint8), _ptr(faces, "faces", torch.int32), nv, nf, V, H, W,
            cams.ctypes.data_as(ctypes.c_void_p), near, cull, bg, fusion._chk(proj, "proj_work", torch.int64), fusion._chk(work, "list_work", torch.int32),
            fusion._chk(out["keys"], "keys", torch.int64), fusion._chk(out["depth"], "depth"), fusion._chk(out["face"], "face", torch.int32),
            fusion._chk(out["rgb"], "out_rgb", torch.uint8), fusion._chk(out["shade"], "shade", torch.uint8), fusion._chk(out["stats"], "stats", torch.int64),
            _ptr(trace, "trace", torch.int64)]
    if _timed is None:
        _lib.call("rcmvs_mr_render", *args, fusion._stream())
    else:
        _lib.call("rcmvs_mr_render_timed", *args, PHASES[_timed[0]], _timed[1], _timed[2], fusion._stream())
    if normals is not None:
        from . import mesh_normals
        out.update(mesh_normals.shade(verts, faces, normals, cams, out["face"], near=near, background=background))
    if texture is not None:
        from . import mesh_texture
        out["tex_rgb"] = mesh_texture.shade(verts, faces, cams, out["face"], texture[1], texture[0], near=near, background=background)
    return out


def stats_rows(out):
    """the counters of ``render``'s result as one dict per view (one host read)"""
    return [dict(zip(STAT_NAMES, (int(x) for x in row))) for row in out["stats"].cpu().tolist()]


def _thresholds(thresholds, what):
    th = [_real(t, "thresholds", what) for t in thresholds]
    if len(th) > 3 or any(t < 0 for t in th):
        raise _lib.RcmvsError(f"{what}: thresholds = {list(thresholds)!r} (at most three, each finite and >= 0)")
    return th


def compare_table(rendered, depth, thresholds=DEFAULT_THRESHOLDS, _timed=None):
    """-> the (V, TABLE) int64 device tensor of csrc/mesh_render.h; nothing is read back"""
    what = "mesh_render.compare"
    th = _thresholds(thresholds, what)
    if not torch.is_tensor(rendered) or not torch.is_tensor(depth) or rendered.dim() != 3 or rendered.shape != depth.shape or rendered.device != depth.device:
        raise _lib.RcmvsError(f"{what}: rendered and depth must be (V,H,W) fp32 tensors of one shape on one device")
    V, H, W = (int(s) for s in rendered.shape)
    if not 1 <= V <= CMP_MAX_VIEWS:
        raise _lib.RcmvsError(f"{what}: {V} views (1 .. {CMP_MAX_VIEWS})")
    _side(H, "H", what), _side(W, "W", what)
    dev = rendered.device
    tiles = (H * W + CMP_TILE - 1) // CMP_TILE
    partial = torch.empty(V * tiles, device=dev, dtype=torch.float64)
    table = torch.empty((V, TABLE), device=dev, dtype=torch.int64)
    tha = (ctypes.c_double * 3)(*(th + [0.0] * (3 - len(th))))
    args = [fusion._chk(rendered, "rendered"), fusion._chk(depth, "depth"), V, H, W, ctypes.cast(tha, ctypes.c_void_p), len(th),
            fusion._chk(partial, "partial_work", torch.float64), fusion._chk(table, "table", torch.int64)]
    if _timed is None:
        _lib.call("rcmvs_mr_compare", *args, fusion._stream())
    else:
        _lib.call("rcmvs_mr_compare_timed", *args, _timed[0], _timed[1], fusion._stream())
    return table


def table_rows(table, thresholds):
    """the device table -> one dict per view: both, only_mesh, only_map, within (one count per threshold), sum_abs (fp64) and
    mean_abs (sum_abs / both, None without a pixel with both)"""
    rows = []
    host = table.cpu().numpy()
    for row in host:
        both = int(row[0])
        sum_abs = float(row[6:7].view(np.float64)[0])
        rows.append({"both": both, "only_mesh": int(row[1]), "only_map": int(row[2]), "within": [int(row[3 + k]) for k in range(len(thresholds))],
                     "sum_abs": sum_abs, "mean_abs": sum_abs / both if both else None})
    return rows


def compare(rendered, depth, thresholds=DEFAULT_THRESHOLDS):
    """rendered: (V,H,W) fp32 from ``render`` (its "depth"), depth: (V,H,W) fp32 depth maps of the same views, both on the device;
    0, negative or non-finite means no depth.  thresholds: up to three relative thresholds t of |r - d| <= t d -> one dict per view
    (``table_rows``); the counts are exact, the sum has a fixed order."""
    th = _thresholds(thresholds, "mesh_render.compare")
    return table_rows(compare_table(rendered, depth, th), th)


def sum_rows(rows, thresholds):
    """the per-view dicts of ``compare`` summed over the views (sum_abs in view order)"""
    both, s = sum(r["both"] for r in rows), math.fsum(r["sum_abs"] for r in rows)
    return {"views": len(rows), "thresholds": [float(t) for t in thresholds], "both": both, "only_mesh": sum(r["only_mesh"] for r in rows),
            "only_map": sum(r["only_map"] for r in rows), "within": [sum(r["within"][k] for r in rows) for k in range(len(thresholds))], "sum_abs": s,
            "mean_abs": s / both if both else None}


def render_views(verts, faces, rgb, views, out_dir=None, near=DEFAULT_NEAR, cull="none", thresholds=DEFAULT_THRESHOLDS, names=None, png=True,
                 normals=None, texture=None):
    """The hook of tsdf_mesh and eval_driver: the mesh into the cameras of ``views`` (tsdf_mesh.filtered_views' dict) at the size of
    its depth maps, compared with them -> the summed table with the summed counters as "stats".  out_dir: depth_mesh/<name>.pfm and
    render/<name>_shade.png, <name>_rgb.png are written there; the names default to the views' numbers in pair.txt (``views["ids"]``),
    as the command line names them.  normals: the vertex normals of mesh_normals.vertex_normals; render/<name>_smooth.png and
    <name>_normal.png are written too.  texture: (atlas, texel) of mesh_texture.texture; render/<name>_tex.png is written too and the
    result gains "textured_views"."""
    depth = views["depth"]
    V, H, W = (int(s) for s in depth.shape)
    out = render(verts, faces, rgb, views["cams"], H, W, near=near, cull=cull, normals=normals, texture=texture)
    rows = compare(out["depth"], depth, thresholds)
    if out_dir is not None:
        write_views(out, out_dir, names if names is not None else ["{:0>8}".format(v) for v in views["ids"]], png)
    total = sum_rows(rows, thresholds)
    stats = stats_rows(out)
    total["stats"] = {k: sum(s[k] for s in stats) for k in STAT_NAMES}
    if texture is not None:
        total["textured_views"] = V
    return total


def write_views(out, out_dir, names, png=True):
    from .data_io import save_pfm
    from .depth_vis import save_png
    os.makedirs(os.path.join(out_dir, "depth_mesh"), exist_ok=True)
    depth = out["depth"].cpu().numpy()
    for i, name in enumerate(names):
        save_pfm(os.path.join(out_dir, "depth_mesh", f"{name}.pfm"), depth[i])
        if png:
            save_png(os.path.join(out_dir, "render", f"{name}_shade.png"), out["shade"][i])
            save_png(os.path.join(out_dir, "render", f"{name}_rgb.png"), out["rgb"][i])
            if "smooth" in out:
                save_png(os.path.join(out_dir, "render", f"{name}_smooth.png"), out["smooth"][i])
                save_png(os.path.join(out_dir, "render", f"{name}_normal.png"), out["normal_rgb"][i])
            if "tex_rgb" in out:
                save_png(os.path.join(out_dir, "render", f"{name}_tex.png"), out["tex_rgb"][i])


def main(argv=None):
    from . import dtu_io, scan_io, tsdf_mesh
    from .data_io import read_pfm
    ap = argparse.ArgumentParser(description="render a PLY mesh into the cameras of a scan: depth PFMs, shade and colour PNGs, comparison with depth maps")
    ap.add_argument("--mesh", required=True, help="the PLY to render")
    ap.add_argument("--pair-folder", required=True, help="folder of pair.txt")
    ap.add_argument("--scan-folder", required=True, help="folder of cams/")
    ap.add_argument("--out", required=True, help="folder for depth_mesh/ and render/")
    ap.add_argument("--depth-folder", default=None, help="folder of depth_est/: compare the rendered depth with these maps")
    ap.add_argument("--size", type=int, nargs=2, default=None, metavar=("H", "W"), help="default: the size of the first depth map of --depth-folder; required without one")
    ap.add_argument("--near", type=float, default=DEFAULT_NEAR)
    ap.add_argument("--cull", choices=sorted(CULL), default="none")
    ap.add_argument("--thresholds", type=float, nargs="*", default=list(DEFAULT_THRESHOLDS))
    ap.add_argument("--no-png", action="store_true")
    ap.add_argument("--normals", choices=("area", "sphere"), default=None, help="smooth shading: vertex normals of rc_mvsnet_amd.mesh_normals under this weight, "
                                                                                "<view>_smooth.png and <view>_normal.png")
    ap.add_argument("--texture", action="store_true", help="the PLY has texcoords (rc_mvsnet_amd.mesh_texture) and its atlas lies next to it: <view>_tex.png")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    dev = torch.device(a.device)
    pairs = scan_io.read_pair_file(os.path.join(a.pair_folder, "pair.txt"))
    views = sorted({v for ref, srcs in pairs for v in [ref] + list(srcs)})
    names = ["{:0>8}".format(v) for v in views]
    cams = np.stack([tsdf_mesh.camera_row(*scan_io.read_camera_parameters(os.path.join(a.scan_folder, "cams/{}_cam.txt".format(n)))) for n in names])
    maps = None
    if a.depth_folder is not None:
        maps = np.stack([read_pfm(os.path.join(a.depth_folder, "depth_est/{}.pfm".format(n)))[0] for n in names]).astype(np.float32)
    if a.size is not None:
        H, W = a.size
    elif maps is not None:
        H, W = maps.shape[1:]
    else:
        raise _lib.RcmvsError("mesh_render: give --size H W or --depth-folder (the size defaults to that of the first depth map)")
    v, f, c = dtu_io.read_ply_mesh_rgb(a.mesh)
    verts, faces, rgb = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (v.astype(np.float32), f.astype(np.int32), c.astype(np.uint8)))
    normals = None
    if a.normals is not None:
        from . import mesh_normals
        normals = mesh_normals.vertex_normals(verts, faces, a.normals)[0]
    texture = None
    if a.texture:
        from . import mesh_texture
        texture = mesh_texture.read_textured(a.mesh, dev)[3:]
    out = render(verts, faces, rgb, cams, int(H), int(W), near=a.near, cull=a.cull, normals=normals, texture=texture)
    write_views(out, a.out, names, png=not a.no_png)
    stats = stats_rows(out)
    total = {"views": len(names), "stats": {k: sum(s[k] for s in stats) for k in STAT_NAMES}}
    if maps is not None:
        if tuple(maps.shape[1:]) != (int(H), int(W)):
            raise _lib.RcmvsError(f"mesh_render: the depth maps are {tuple(maps.shape[1:])}, the render is {(int(H), int(W))}")
        rows = compare(out["depth"], torch.from_numpy(maps).to(dev), a.thresholds)
        for name, row, s in zip(names, rows, stats):
            print(json.dumps(dict({"view": name}, **row, stats=s)))
        total = dict(sum_rows(rows, a.thresholds), stats=total["stats"])
    print(json.dumps(total))
    return total


if __name__ == "__main__":
    main()
