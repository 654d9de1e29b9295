"""Clean-up of an extracted triangle mesh on the HIP path (csrc/mesh_clean.hip; the contract is csrc/mesh_clean.h, the per-element
rules csrc/mesh_clean_math.h, restated by tests/mesh_clean_oracle.py): connected components, removal of small ones, compaction of
faces and vertices, the 1-ring with edge multiplicities, Taubin smoothing.

``clean_mesh`` takes what ``TsdfVolume.extract`` returns and gives back the same three device tensors plus a dict of counts; the
parts -- ``components``, ``compact``, ``adjacency``, ``taubin`` -- are callable on their own.  Every output is defined exactly:
a vertex's label is the smallest vertex number of its component, kept faces and vertices stay in input order, a vertex's
neighbours are ascending, and a smoothing step sums them in that order in fp64.  The host reads the compacted component table
(one row per component, only for ``keep_largest``) and a handful of totals; there is no per-vertex or per-face host pass.

    python -m rc_mvsnet_amd.mesh_clean --in a.ply --out b.ply --min-faces 100 --smooth 10

Limits: connectivity is over vertices (two faces that share a vertex are one component); at most 2^31 - 1 directed 1-ring
entries, i.e. 357 913 941 faces; a vertex with more than 48 entries is sorted by a slower path whose time grows with the square
of its degree; the command line reads positions and faces only, so it writes white vertices.  Hole filling (``fill_holes``) is
rc_mvsnet_amd.mesh_holes', decimation rc_mvsnet_amd.mesh_decimate's.  No CPU fallback."""
import argparse
import ctypes
import json
import math

import numpy as np
import torch

from . import _lib, fusion

SCAN_TILE, SCAN_WORK, SORT_LIMIT, MAX_ENTRIES = (_lib.CONSTANTS["RCMVS_MC_" + k] for k in ("SCAN_TILE", "SCAN_WORK", "SORT_LIMIT", "MAX_ENTRIES"))
_NULL = ctypes.c_void_p(0)


def _ptr(t, name, dtype):
    """the device pointer of t, NULL for None and for a tensor without elements"""
    if t is None:
        return _NULL
    p = fusion._chk(t, name, dtype)
    return p if t.numel() else _NULL


def _scan_work(n, dev):
    """the work area of csrc/scan_sort.hip's scan of up to n elements (the three mesh families' scan_work arguments)"""
    return torch.empty(SCAN_WORK + (n + SCAN_TILE - 1) // SCAN_TILE + 1, device=dev, dtype=torch.int32)


def _faces(faces, what):
    if not torch.is_tensor(faces) or faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise _lib.RcmvsError(f"{what}: faces must be an (nf,3) int32 tensor, got "
                              f"{(tuple(faces.shape), faces.dtype) if torch.is_tensor(faces) else type(faces).__name__}")
    return int(faces.shape[0])


def _verts(verts, what):
    if not torch.is_tensor(verts) or verts.dtype != torch.float32 or verts.dim() != 2 or verts.shape[1] != 3:
        raise _lib.RcmvsError(f"{what}: verts must be an (nv,3) float32 tensor, got "
                              f"{(tuple(verts.shape), verts.dtype) if torch.is_tensor(verts) else type(verts).__name__}")
    return int(verts.shape[0])


def _mesh(verts, faces, rgb, what):
    nv = _verts(verts, what)
    nf = _faces(faces, what)
    if rgb is not None and (not torch.is_tensor(rgb) or rgb.dtype != torch.uint8 or tuple(rgb.shape) != (nv, 3)):
        raise _lib.RcmvsError(f"{what}: rgb must be an ({nv},3) uint8 tensor or None")
    if faces.device != verts.device or (rgb is not None and rgb.device != verts.device):
        raise _lib.RcmvsError(f"{what}: verts, faces and rgb must live on one device")
    return nv, nf


def _count(value, name, what):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 0:
        raise _lib.RcmvsError(f"{what}: {name} = {value!r} (an integer >= 0)")
    return int(value)


def _real(value, name, what):
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise _lib.RcmvsError(f"{what}: {name} = {value!r} (a finite number)") from None
    if not math.isfinite(value):
        raise _lib.RcmvsError(f"{what}: {name} = {value} (finite)")
    return value


def components(verts, faces):
    """-> dict: label (nv int32: the smallest vertex number of the vertex's component), face_ok (nf uint8: 1 = valid), comp_faces
    (nv int32: at a label, the valid faces whose first index carries it), counts (4 int64 on the device, [0] = invalid faces)"""
    nv, nf = _mesh(verts, faces, None, "mesh_clean.components")
    dev = verts.device
    label = torch.empty(nv, device=dev, dtype=torch.int32)
    face_ok = torch.empty(nf, device=dev, dtype=torch.uint8)
    comp_faces = torch.empty(nv, device=dev, dtype=torch.int32)
    counts = torch.empty(4, device=dev, dtype=torch.int64)
    _lib.call("rcmvs_mc_components", _ptr(faces, "faces", torch.int32), nv, nf, _ptr(label, "label", torch.int32), _ptr(face_ok, "face_ok", torch.uint8),
              _ptr(comp_faces, "comp_faces", torch.int32), _ptr(counts, "counts", torch.int64), fusion._stream())
    return {"label": label, "face_ok": face_ok, "comp_faces": comp_faces, "counts": counts}


def component_table(comp, capacity=None):
    """The components with at least one valid face -> (table (rows,2) int32 on the device: {label, faces} ascending by label,
    largest faces value).  One host read of the two totals."""
    label, comp_faces = comp["label"], comp["comp_faces"]
    nv, dev = int(label.shape[0]), label.device
    capacity = nv if capacity is None else int(capacity)
    flags = torch.empty(nv, device=dev, dtype=torch.uint8)
    rank = torch.empty(nv + 1, device=dev, dtype=torch.int32)
    table = torch.empty((capacity, 2), device=dev, dtype=torch.int32)
    totals = torch.empty(2, device=dev, dtype=torch.int64)
    work = _scan_work(nv, dev)
    _lib.call("rcmvs_mc_component_table", _ptr(label, "label", torch.int32), _ptr(comp_faces, "comp_faces", torch.int32), nv,
              _ptr(flags, "flags", torch.uint8), _ptr(rank, "rank", torch.int32), _ptr(work, "scan_work", torch.int32),
              _ptr(table, "table", torch.int32), capacity, _ptr(totals, "totals", torch.int64), fusion._stream())
    rows, most = (int(t) for t in totals.cpu())
    return table[:min(rows, capacity)], most


def compact(verts, faces, rgb, comp, *, min_faces=0, min_fraction=0.0, keep_largest=0, drop_unreferenced=True):
    """Keeps the valid faces of the selected components and (drop_unreferenced) the vertices they use, both in input order ->
    (verts, faces, rgb, info); info: components_in, components_kept, largest_component_faces, faces_out, vertices_out."""
    what = "mesh_clean.compact"
    nv, nf = _mesh(verts, faces, rgb, what)
    min_faces, keep_largest = _count(min_faces, "min_faces", what), _count(keep_largest, "keep_largest", what)
    min_fraction = _real(min_fraction, "min_fraction", what)
    dev = verts.device
    table, most = component_table(comp, capacity=min(nv, nf))
    rows = int(table.shape[0])
    k_faces = k_label = 0
    if keep_largest > 0 and rows > 0:                            # the one table the host reads: one row per component
        t = table.cpu().numpy()
        order = np.lexsort((t[:, 0], -t[:, 1].astype(np.int64)))
        k_label, k_faces = (int(x) for x in t[order[min(keep_largest, rows) - 1]])
    face_keep = torch.empty(nf, device=dev, dtype=torch.uint8)
    vert_keep = torch.empty(nv, device=dev, dtype=torch.uint8)
    face_rank = torch.empty(nf + 1, device=dev, dtype=torch.int32)
    vert_rank = torch.empty(nv + 1, device=dev, dtype=torch.int32)
    totals = torch.empty(3, device=dev, dtype=torch.int64)
    work = _scan_work(max(nv, nf), dev)
    _lib.call("rcmvs_mc_select", _ptr(faces, "faces", torch.int32), _ptr(comp["face_ok"], "face_ok", torch.uint8), _ptr(comp["label"], "label", torch.int32),
              _ptr(comp["comp_faces"], "comp_faces", torch.int32), nv, nf, min_faces, min_fraction, most, keep_largest, k_faces, k_label,
              1 if drop_unreferenced else 0, _ptr(face_keep, "face_keep", torch.uint8), _ptr(vert_keep, "vert_keep", torch.uint8),
              _ptr(face_rank, "face_rank", torch.int32), _ptr(vert_rank, "vert_rank", torch.int32),
              _ptr(work, "scan_work", torch.int32), _ptr(totals, "totals", torch.int64), fusion._stream())
    nf_out, nv_out, kept = (int(t) for t in totals.cpu())         # the final sizes
    out_verts = torch.empty((nv_out, 3), device=dev, dtype=torch.float32)
    out_faces = torch.empty((nf_out, 3), device=dev, dtype=torch.int32)
    out_rgb = None if rgb is None else torch.empty((nv_out, 3), device=dev, dtype=torch.uint8)
    _lib.call("rcmvs_mc_gather", _ptr(verts, "verts", torch.float32), _ptr(rgb, "rgb", torch.uint8), _ptr(faces, "faces", torch.int32),
              _ptr(face_keep, "face_keep", torch.uint8), _ptr(face_rank, "face_rank", torch.int32), _ptr(vert_keep, "vert_keep", torch.uint8),
              _ptr(vert_rank, "vert_rank", torch.int32), nv, nf, nv_out, nf_out, _ptr(out_verts, "out_verts", torch.float32),
              _ptr(out_rgb, "out_rgb", torch.uint8), _ptr(out_faces, "out_faces", torch.int32), fusion._stream())
    info = {"components_in": rows, "components_kept": kept, "largest_component_faces": most, "faces_out": nf_out, "vertices_out": nv_out}
    return out_verts, out_faces, out_rgb, info


def adjacency(verts_n, faces):
    """The 1-ring of a mesh of verts_n vertices -> dict: row_start (verts_n + 1), row_len (verts_n), nbr and mult (6 nf; a vertex's
    distinct neighbours ascending from row_start, each with the number of faces on that edge, then -1 / 0), on_boundary (verts_n
    uint8), all on the device, and the integers edges, boundary_edges, nonmanifold_edges, referenced_vertices, long_segments."""
    what = "mesh_clean.adjacency"
    nf = _faces(faces, what)
    nv = _count(verts_n, "verts_n", what)
    if 6 * nf > MAX_ENTRIES:
        raise _lib.RcmvsError(f"{what}: {nf} faces (at most {MAX_ENTRIES // 6}: 2^31 - 1 directed entries)")
    dev = faces.device
    row_start = torch.empty(nv + 1, device=dev, dtype=torch.int32)
    row_len = torch.empty(nv, device=dev, dtype=torch.int32)
    nbr = torch.empty(6 * nf, device=dev, dtype=torch.int32)
    mult = torch.empty(6 * nf, device=dev, dtype=torch.int32)
    on_boundary = torch.empty(nv, device=dev, dtype=torch.uint8)
    cursor = torch.empty(nv, device=dev, dtype=torch.int32)
    heavy = torch.empty(6 * nf // (SORT_LIMIT + 1) + 1, device=dev, dtype=torch.int32)
    stats = torch.empty(6, device=dev, dtype=torch.int64)
    work = _scan_work(nv, dev)
    _lib.call("rcmvs_mc_adjacency", _ptr(faces, "faces", torch.int32), nv, nf, _ptr(row_start, "row_start", torch.int32), _ptr(row_len, "row_len", torch.int32),
              _ptr(nbr, "nbr", torch.int32), _ptr(mult, "mult", torch.int32), _ptr(on_boundary, "on_boundary", torch.uint8),
              _ptr(cursor, "cursor", torch.int32), _ptr(heavy, "heavy", torch.int32), int(heavy.numel()),
              _ptr(work, "scan_work", torch.int32), _ptr(stats, "stats", torch.int64), fusion._stream())
    e, b, m, r, h, _ = (int(t) for t in stats.cpu())
    return {"verts_n": nv, "row_start": row_start, "row_len": row_len, "nbr": nbr, "mult": mult, "on_boundary": on_boundary, "edges": e,
            "boundary_edges": b, "nonmanifold_edges": m, "referenced_vertices": r, "long_segments": h}


def taubin(verts, adj, iterations=10, lam=0.5, mu=-0.53, pin_boundary=True):
    """``iterations`` rounds of a lambda step then a mu step (Jacobi, fp64 per coordinate, fp32 between steps) -> new (nv,3) fp32
    positions; the input is not written.  pin_boundary: vertices with an edge of multiplicity 1 stay where they are."""
    what = "mesh_clean.taubin"
    nv = _verts(verts, what)
    iterations = _count(iterations, "iterations", what)
    lam, mu = _real(lam, "lam", what), _real(mu, "mu", what)
    if adj["verts_n"] != nv:
        raise _lib.RcmvsError(f"{what}: the adjacency is of {adj['verts_n']} vertices, verts has {nv}")
    fusion._chk(verts, "verts", torch.float32)
    cur, nxt = verts, None
    pinned = _ptr(adj["on_boundary"], "on_boundary", torch.uint8) if pin_boundary else _NULL
    for step in range(2 * iterations):
        if nxt is None or nxt is verts:
            nxt = torch.empty_like(verts)
        _lib.call("rcmvs_mc_taubin_step", _ptr(cur, "src", torch.float32), _ptr(nxt, "dst", torch.float32), nv, _ptr(adj["row_start"], "row_start", torch.int32),
                  _ptr(adj["row_len"], "row_len", torch.int32), _ptr(adj["nbr"], "nbr", torch.int32), int(adj["nbr"].numel()), pinned,
                  lam if step % 2 == 0 else mu, fusion._stream())
        cur, nxt = nxt, cur
    return cur if iterations else verts.clone()


def clean_mesh(verts, faces, rgb=None, *, min_faces=0, min_fraction=0.0, keep_largest=0, drop_unreferenced=True, smooth_iterations=0, lam=0.5,
               mu=-0.53, pin_boundary=True, fill_holes=0):
    """Removes invalid faces and the components the three rules reject (faces >= min_faces; faces >= min_fraction * the largest
    component's; among the keep_largest largest, ties to the smaller label; the defaults keep everything), drops the vertices no
    kept face uses (drop_unreferenced), closes the boundary loops of at most fill_holes edges (mesh_holes.fill_holes; 0: none, and
    nothing new runs), then runs smooth_iterations rounds of Taubin smoothing on the filled mesh, whose 1-ring and counts the stats
    describe -> (verts, faces, rgb, stats); with fill_holes, stats["holes"] are mesh_holes' counts."""
    what = "mesh_clean.clean_mesh"
    nv, nf = _mesh(verts, faces, rgb, what)
    for name, value in (("min_faces", min_faces), ("keep_largest", keep_largest)):
        _count(value, name, what)
    smooth_iterations = _count(smooth_iterations, "smooth_iterations", what)
    if _count(fill_holes, "fill_holes", what):
        from . import mesh_holes
        fill_holes = mesh_holes.max_edges_argument(fill_holes, what)
    for name, value in (("min_fraction", min_fraction), ("lam", lam), ("mu", mu)):
        _real(value, name, what)
    comp = components(verts, faces)
    v, f, c, info = compact(verts, faces, rgb, comp, min_faces=min_faces, min_fraction=min_fraction, keep_largest=keep_largest,
                            drop_unreferenced=drop_unreferenced)
    holes = None
    if fill_holes:
        v, f, c, holes = mesh_holes.fill_holes(v, f, c, max_edges=fill_holes)
    adj = adjacency(int(v.shape[0]), f)
    if smooth_iterations:
        v = taubin(v, adj, smooth_iterations, lam, mu, pin_boundary)
    stats = {"vertices_in": nv, "vertices_out": int(v.shape[0]), "faces_in": nf, "faces_out": int(f.shape[0]),
             "invalid_faces": int(comp["counts"][:1].cpu()[0]), "components_in": info["components_in"], "components_kept": info["components_kept"],
             "largest_component_faces": info["largest_component_faces"], "unreferenced_removed": nv - info["vertices_out"], "edges": adj["edges"],
             "boundary_edges": adj["boundary_edges"], "nonmanifold_edges": adj["nonmanifold_edges"],
             "euler_characteristic": adj["referenced_vertices"] - adj["edges"] + int(f.shape[0]), "smooth_iterations": smooth_iterations}
    if holes is not None:
        stats["holes"] = holes
    return v, f, c, stats


def clean_options(min_faces=0, min_fraction=0.0, keep_largest=0, smooth=0, fill_holes=0):
    """The mesh path's five options -> the keyword arguments of clean_mesh, or None when none of them asks for anything;
    fill_holes is among them only when it is not 0"""
    if not (min_faces or min_fraction or keep_largest or smooth or fill_holes):
        return None
    options = {"min_faces": min_faces, "min_fraction": min_fraction, "keep_largest": keep_largest, "smooth_iterations": smooth}
    if fill_holes:
        options["fill_holes"] = fill_holes
    return options


def main(argv=None):
    from . import dtu_io, tsdf_mesh
    ap = argparse.ArgumentParser(description="remove small components and unreferenced vertices of a PLY mesh, Taubin-smooth it")
    ap.add_argument("--in", dest="src", required=True, help="the PLY to read (positions and triangles)")
    ap.add_argument("--out", required=True, help="the PLY to write")
    ap.add_argument("--min-faces", type=int, default=0, help="drop components with fewer faces")
    ap.add_argument("--min-fraction", type=float, default=0.0, help="drop components with fewer than this fraction of the largest one's faces")
    ap.add_argument("--keep-largest", type=int, default=0, help="keep only the K components with most faces (0: no limit)")
    ap.add_argument("--smooth", type=int, default=0, help="rounds of Taubin smoothing")
    ap.add_argument("--fill-holes", type=int, default=0, help="close boundary loops of at most N edges (3 .. 4096) before smoothing; 0: none")
    ap.add_argument("--lambda", dest="lam", type=float, default=0.5)
    ap.add_argument("--mu", type=float, default=-0.53)
    ap.add_argument("--no-pin-boundary", action="store_true", help="also move vertices on boundary edges")
    ap.add_argument("--keep-unreferenced", action="store_true", help="keep every vertex, filter faces only")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    verts, faces = dtu_io.read_ply_mesh(a.src)
    dev = torch.device(a.device)
    v, f, _, stats = clean_mesh(torch.from_numpy(np.ascontiguousarray(verts, np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(faces, np.int32)).to(dev),
                                None, min_faces=a.min_faces, min_fraction=a.min_fraction, keep_largest=a.keep_largest,
                                drop_unreferenced=not a.keep_unreferenced, smooth_iterations=a.smooth, lam=a.lam, mu=a.mu,
                                pin_boundary=not a.no_pin_boundary, fill_holes=a.fill_holes)
    with open(a.out, "wb") as out:
        out.write(tsdf_mesh.mesh_ply_bytes(v, f, None))
    summary = dict({"in": a.src, "out": a.out}, **stats)
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
