"""Decimation of a triangle mesh on the HIP path (csrc/mesh_decimate.hip; the contract is csrc/mesh_decimate.h, the per-element
rules and their operation order csrc/mesh_decimate_math.h, restated by tests/mesh_decimate_oracle.py): vertex clustering on a
regular lattice of edge ``cell`` with quadric-error placement (Lindstrom's out-of-core simplification).

``decimate`` takes what ``TsdfVolume.extract`` or ``mesh_clean.clean_mesh`` returns and gives back the same three device tensors
plus a dict of counts; the parts -- ``bounds``, ``cluster``, ``classify_faces``, ``quadrics``, ``place`` -- are callable on their
own.  The result is defined exactly: the lattice starts half a cell below the minimum of the finite vertices, the clusters are
the occupied cells in ascending (kz, ky, kx) order, a cluster's members and its faces' corners are added in ascending vertex /
(face, corner) order in fp64, a face survives when its three clusters differ and no earlier face has the same triple up to
rotation, and surviving faces keep their input order.  The host reads four small things -- the box (32 bytes), the number of
clusters, the two final sizes, the seven counters in one transfer -- and the result's edge statistics from mesh_clean.adjacency;
there is no per-vertex or per-face host pass.

    python -m rc_mvsnet_amd.mesh_decimate --in a.ply --out b.ply --cell 0.004

Limits: clustering preserves no features (one vertex per occupied cell, so two sheets closer than a cell merge and thin parts
can collapse; rc_mvsnet_amd.mesh_simplify collapses edges instead); clustering can create non-manifold edges, which the stats count; at most 2^21 cells per axis; at most 2^31 - 256
vertices and (2^31 - 256) / 3 faces.  No CPU fallback."""
import argparse
import ctypes
import json
import math

import numpy as np
import torch

from . import _lib, fusion, mesh_clean
from .mesh_clean import _count, _mesh, _ptr, _real, _scan_work

SCAN_TILE, SCAN_WORK, SORT_BLOCK, MAX_ELEMENTS, MAX_CELLS_PER_AXIS = (_lib.CONSTANTS["RCMVS_MD_" + k] for k in (
    "SCAN_TILE", "SCAN_WORK", "SORT_BLOCK", "MAX_ELEMENTS", "MAX_CELLS_PER_AXIS"))
FACE_KEPT, FACE_INVALID, FACE_UNCLUSTERED, FACE_COLLAPSED, FACE_DUPLICATE = (_lib.CONSTANTS["RCMVS_MD_FACE_" + k] for k in (
    "KEPT", "INVALID", "UNCLUSTERED", "COLLAPSED", "DUPLICATE"))
VIA_QUADRIC, VIA_NO_FACES, VIA_SINGULAR, VIA_OUTSIDE, VIA_MEAN = (_lib.CONSTANTS["RCMVS_MD_VIA_" + k] for k in (
    "QUADRIC", "NO_FACES", "SINGULAR", "OUTSIDE", "MEAN"))
PLACEMENTS = {"quadric": _lib.CONSTANTS["RCMVS_MD_PLACE_QUADRIC"], "mean": _lib.CONSTANTS["RCMVS_MD_PLACE_MEAN"]}
DEFAULT_REG = 1e-3                                               # md::DEFAULT_REG of csrc/mesh_decimate_math.h


def _cdiv(a, b):
    return (a + b - 1) // b


def _sort_buffers(n, dev):
    """hist, hist_start and a scan_work for a radix sort of n pairs (and for scans of up to n elements)"""
    table = 256 * _cdiv(n, SORT_BLOCK)
    return (torch.empty(table, device=dev, dtype=torch.int32), torch.empty(table + 1, device=dev, dtype=torch.int32), _scan_work(max(table, n), dev))


def _positive(value, name, what):
    value = _real(value, name, what)
    if not value > 0:
        raise _lib.RcmvsError(f"{what}: {name} = {value} (finite, > 0)")
    return value


def _sizes(nv, nf, what):
    if nv > MAX_ELEMENTS or 3 * nf > MAX_ELEMENTS:
        raise _lib.RcmvsError(f"{what}: {nv} vertices, {nf} faces (at most 2^31 - 256 vertices and (2^31 - 256) / 3 faces)")


def _host_lattice(lattice):
    origin, cell, dims = lattice["origin"], lattice["cell"], lattice["dims"]
    lat = (ctypes.c_double * 4)(*[float(o) for o in origin], float(cell))
    g = (ctypes.c_longlong * 3)(*[int(d) for d in dims])
    return lat, g, ctypes.cast(lat, ctypes.c_void_p), ctypes.cast(g, ctypes.c_void_p)


def bounds(verts):
    """-> (lo (3,) float32, hi (3,) float32, finite): the box of the vertices whose three coordinates are finite (lo, hi None when
    there is none) and their number.  -0.0 orders below +0.0.  One host read of 32 bytes."""
    what = "mesh_decimate.bounds"
    nv = mesh_clean._verts(verts, what)
    _sizes(nv, 0, what)
    out = torch.empty(8, device=verts.device, dtype=torch.int32)
    _lib.call("rcmvs_md_bounds", _ptr(verts, "verts", torch.float32), nv, _ptr(out, "bounds", torch.int32), fusion._stream())
    k = out.cpu().numpy().view(np.uint32)
    finite = int(k[6])
    if finite == 0:
        return None, None, 0
    keys = k[:6]
    raw = np.where(keys & np.uint32(0x80000000), keys & np.uint32(0x7fffffff), ~keys).astype(np.uint32)      # md::unordered
    box = raw.view(np.float32)
    return box[:3].copy(), box[3:].copy(), finite


def lattice(lo, hi, cell):
    """The lattice of the box lo .. hi (float32) for cells of edge ``cell`` -> dict: origin (3 floats, lo - cell / 2 in fp64), cell,
    dims (3 ints, floor((hi - origin) / cell) + 1).  Refused, naming the axis, when an axis would have more than 2^21 cells."""
    what = "mesh_decimate.lattice"
    cell = _positive(cell, "cell", what)
    box = (ctypes.c_float * 6)(*[float(v) for v in lo], *[float(v) for v in hi])
    lat, g = (ctypes.c_double * 4)(), (ctypes.c_longlong * 3)()
    _lib.call("rcmvs_md_lattice", ctypes.cast(box, ctypes.c_void_p), cell, ctypes.cast(lat, ctypes.c_void_p), ctypes.cast(g, ctypes.c_void_p))
    return {"origin": [lat[0], lat[1], lat[2]], "cell": lat[3], "dims": [int(g[0]), int(g[1]), int(g[2])]}


def cluster(verts, lat):
    """The vertices on the lattice ``lat`` (of ``lattice``) -> dict: cluster (nv int32: the vertex's cluster, -1 for a vertex with a
    coordinate that is not finite or outside the lattice), order (nv int32: the vertices by (cell key, vertex number)),
    cluster_start (m + 1 int32: cluster r's members are order[cluster_start[r] : cluster_start[r + 1]]), cluster_key (m int64: (kz
    gy + ky) gx + kx, ascending), all on the device, and the integers m and clustered.  One host read of the two."""
    what = "mesh_decimate.cluster"
    nv = mesh_clean._verts(verts, what)
    _sizes(nv, 0, what)
    dev = verts.device
    lat_host, dims_host, plat, pg = _host_lattice(lat)            # the host arrays plat / pg point into stay alive until the call has returned
    key = [torch.empty(nv, device=dev, dtype=torch.int64) for _ in range(2)]
    idx = [torch.empty(nv, device=dev, dtype=torch.int32) for _ in range(2)]
    hist, hist_start, work = _sort_buffers(nv, dev)
    head = torch.empty(nv, device=dev, dtype=torch.uint8)
    head_rank = torch.empty(nv + 1, device=dev, dtype=torch.int32)
    cl = torch.empty(nv, device=dev, dtype=torch.int32)
    order = torch.empty(nv, device=dev, dtype=torch.int32)
    start = torch.empty(nv + 1, device=dev, dtype=torch.int32)
    ckey = torch.empty(nv, device=dev, dtype=torch.int64)
    totals = torch.empty(2, device=dev, dtype=torch.int64)
    _lib.call("rcmvs_md_cluster", _ptr(verts, "verts", torch.float32), nv, plat, pg, _ptr(key[0], "key_a", torch.int64), _ptr(idx[0], "idx_a", torch.int32),
              _ptr(key[1], "key_b", torch.int64), _ptr(idx[1], "idx_b", torch.int32), _ptr(hist, "hist", torch.int32),
              _ptr(hist_start, "hist_start", torch.int32), _ptr(work, "scan_work", torch.int32), _ptr(head, "head", torch.uint8),
              _ptr(head_rank, "head_rank", torch.int32), _ptr(cl, "cluster", torch.int32), _ptr(order, "order", torch.int32),
              _ptr(start, "cluster_start", torch.int32), _ptr(ckey, "cluster_key", torch.int64), _ptr(totals, "totals", torch.int64), fusion._stream())
    m, clustered = (int(t) for t in totals.cpu())                 # the number of clusters: the sizes of everything that follows
    return {"cluster": cl, "order": order, "cluster_start": start[:m + 1], "cluster_key": ckey[:m], "m": m, "clustered": clustered, "verts_n": nv}


def classify_faces(verts_n, faces, cl):
    """-> dict: cface ((nf,3) int32: the three clusters of a valid face, -1 for an invalid one), face_class (nf uint8: FACE_KEPT,
    FACE_INVALID, FACE_UNCLUSTERED, FACE_COLLAPSED or FACE_DUPLICATE, the first that applies), counts (4 int64 on the device:
    invalid, unclustered, collapsed, duplicate)"""
    what = "mesh_decimate.classify_faces"
    nf = mesh_clean._faces(faces, what)
    nv = _count(verts_n, "verts_n", what)
    _sizes(nv, nf, what)
    if cl["verts_n"] != nv:
        raise _lib.RcmvsError(f"{what}: the clusters are of {cl['verts_n']} vertices, not {nv}")
    dev = faces.device
    cface = torch.empty((nf, 3), device=dev, dtype=torch.int32)
    face_class = torch.empty(nf, device=dev, dtype=torch.uint8)
    capacity = 1 << max(1, (2 * nf).bit_length())                # a power of two above 2 nf: the table at most half full
    table = torch.empty(capacity, device=dev, dtype=torch.int32)
    counts = torch.empty(4, device=dev, dtype=torch.int64)
    _lib.call("rcmvs_md_classify_faces", _ptr(faces, "faces", torch.int32), nv, nf, _ptr(cl["cluster"], "cluster", torch.int32),
              _ptr(cface, "cface", torch.int32), _ptr(face_class, "face_class", torch.uint8), _ptr(table, "table", torch.int32), capacity,
              _ptr(counts, "counts", torch.int64), fusion._stream())
    return {"cface": cface, "face_class": face_class, "counts": counts}


def quadrics(verts, faces, cl, lat):
    """-> (m, 9) float64 on the device: per cluster A00 A01 A02 A11 A12 A22 b0 b1 b2, the sums of its corners' plane quadrics in the
    cluster's own frame (units of the cell), added in ascending (face, corner) order"""
    what = "mesh_decimate.quadrics"
    nv, nf = _mesh(verts, faces, None, what)
    _sizes(nv, nf, what)
    dev, m = verts.device, cl["m"]
    quad = torch.empty((m, 9), device=dev, dtype=torch.float64)
    if m == 0:
        return quad
    lat_host, dims_host, plat, pg = _host_lattice(lat)            # the host arrays plat / pg point into stay alive until the call has returned
    n = 3 * nf
    key = [torch.empty(n, device=dev, dtype=torch.int32) for _ in range(2)]
    idx = [torch.empty(n, device=dev, dtype=torch.int32) for _ in range(2)]
    hist, hist_start, work = _sort_buffers(n, dev)
    seg = torch.empty(2 * m, device=dev, dtype=torch.int32)
    _lib.call("rcmvs_md_quadrics", _ptr(verts, "verts", torch.float32), _ptr(faces, "faces", torch.int32), nv, nf, _ptr(cl["cluster"], "cluster", torch.int32),
              _ptr(cl["cluster_key"], "cluster_key", torch.int64), m, plat, pg, _ptr(key[0], "ckey_a", torch.int32), _ptr(idx[0], "cidx_a", torch.int32),
              _ptr(key[1], "ckey_b", torch.int32), _ptr(idx[1], "cidx_b", torch.int32), _ptr(hist, "hist", torch.int32),
              _ptr(hist_start, "hist_start", torch.int32), _ptr(work, "scan_work", torch.int32), _ptr(seg, "seg", torch.int32),
              _ptr(quad, "quad", torch.float64), fusion._stream())
    return quad


def place(verts, rgb, cl, lat, quad=None, placement="quadric", reg=DEFAULT_REG):
    """One vertex per cluster -> (verts (m,3) float32, rgb (m,3) uint8 or None, via (m uint8: VIA_QUADRIC, VIA_NO_FACES,
    VIA_SINGULAR, VIA_OUTSIDE or VIA_MEAN), counts (3 int64 on the device: the clusters that fell back for no faces, a singular
    system, a minimiser outside the cell)).  placement "mean" needs no quad."""
    what = "mesh_decimate.place"
    nv = mesh_clean._verts(verts, what)
    _sizes(nv, 0, what)
    if placement not in PLACEMENTS:
        raise _lib.RcmvsError(f"{what}: placement = {placement!r} (quadric or mean)")
    reg = _real(reg, "reg", what)
    if reg < 0:
        raise _lib.RcmvsError(f"{what}: reg = {reg} (finite, >= 0)")
    if placement == "quadric" and quad is None:
        raise _lib.RcmvsError(f"{what}: quadric placement needs the clusters' quadrics")
    dev, m = verts.device, cl["m"]
    lat_host, dims_host, plat, pg = _host_lattice(lat)            # the host arrays plat / pg point into stay alive until the call has returned
    out_verts = torch.empty((m, 3), device=dev, dtype=torch.float32)
    out_rgb = None if rgb is None else torch.empty((m, 3), device=dev, dtype=torch.uint8)
    via = torch.empty(m, device=dev, dtype=torch.uint8)
    counts = torch.empty(3, device=dev, dtype=torch.int64)
    _lib.call("rcmvs_md_place", _ptr(verts, "verts", torch.float32), _ptr(rgb, "rgb", torch.uint8), nv, _ptr(cl["order"], "order", torch.int32),
              fusion._chk(cl["cluster_start"], "cluster_start", torch.int32), _ptr(cl["cluster_key"], "cluster_key", torch.int64), m, plat, pg,
              _ptr(quad if placement == "quadric" else None, "quad", torch.float64), PLACEMENTS[placement], reg, _ptr(out_verts, "out_verts", torch.float32),
              _ptr(out_rgb, "out_rgb", torch.uint8), _ptr(via, "via", torch.uint8), _ptr(counts, "counts", torch.int64), fusion._stream())
    return out_verts, out_rgb, via, counts


def _compact(cverts, crgb, fc, m, nf, drop_unreferenced):
    """the kept faces in input order and (drop_unreferenced) the clusters they use, through mesh_clean's gather"""
    dev = cverts.device
    face_keep = torch.empty(nf, device=dev, dtype=torch.uint8)
    vert_keep = torch.empty(m, device=dev, dtype=torch.uint8)
    face_rank = torch.empty(nf + 1, device=dev, dtype=torch.int32)
    vert_rank = torch.empty(m + 1, device=dev, dtype=torch.int32)
    totals = torch.empty(2, device=dev, dtype=torch.int64)
    work = _scan_work(max(m, nf), dev)
    _lib.call("rcmvs_md_select", _ptr(fc["cface"], "cface", torch.int32), _ptr(fc["face_class"], "face_class", torch.uint8), m, nf,
              1 if drop_unreferenced else 0, _ptr(face_keep, "face_keep", torch.uint8), _ptr(vert_keep, "vert_keep", torch.uint8),
              _ptr(face_rank, "face_rank", torch.int32), _ptr(vert_rank, "vert_rank", torch.int32), _ptr(work, "scan_work", torch.int32),
              _ptr(totals, "totals", torch.int64), fusion._stream())
    nf_out, nv_out = (int(t) for t in totals.cpu())               # the final sizes
    out_verts = torch.empty((nv_out, 3), device=dev, dtype=torch.float32)
    out_faces = torch.empty((nf_out, 3), device=dev, dtype=torch.int32)
    out_rgb = None if crgb is None else torch.empty((nv_out, 3), device=dev, dtype=torch.uint8)
    _lib.call("rcmvs_mc_gather", _ptr(cverts, "verts", torch.float32), _ptr(crgb, "rgb", torch.uint8), _ptr(fc["cface"], "faces", torch.int32),
              _ptr(face_keep, "face_keep", torch.uint8), _ptr(face_rank, "face_rank", torch.int32), _ptr(vert_keep, "vert_keep", torch.uint8),
              _ptr(vert_rank, "vert_rank", torch.int32), m, nf, nv_out, nf_out, _ptr(out_verts, "out_verts", torch.float32),
              _ptr(out_rgb, "out_rgb", torch.uint8), _ptr(out_faces, "out_faces", torch.int32), fusion._stream())
    return out_verts, out_faces, out_rgb


def decimate(verts, faces, rgb=None, *, cell, placement="quadric", reg=DEFAULT_REG, drop_unreferenced=True):
    """One vertex per occupied lattice cell of edge ``cell``, placed at the minimiser of the cluster's regularised quadric (or at the
    members' mean: placement="mean", and wherever the quadric has no answer inside the cell); the faces whose three clusters
    differ, without repetitions, in input order; drop_unreferenced removes the clusters no surviving face uses
    -> (verts, faces, rgb, stats)."""
    what = "mesh_decimate.decimate"
    nv, nf = _mesh(verts, faces, rgb, what)
    _sizes(nv, nf, what)
    cell = _positive(cell, "cell", what)
    reg = _real(reg, "reg", what)
    if reg < 0:
        raise _lib.RcmvsError(f"{what}: reg = {reg} (finite, >= 0)")
    if placement not in PLACEMENTS:
        raise _lib.RcmvsError(f"{what}: placement = {placement!r} (quadric or mean)")
    lo, hi, finite = bounds(verts)
    stats = {"vertices_in": nv, "faces_in": nf, "cell": cell, "placement": placement}
    # no finite vertex: nothing to put a lattice round; on any lattice every vertex is unclustered and the result is the empty mesh
    lat = lattice(lo, hi, cell) if finite else {"origin": [0.0, 0.0, 0.0], "cell": cell, "dims": [1, 1, 1]}
    cl = cluster(verts, lat)
    m, clustered = cl["m"], cl["clustered"]
    fc = classify_faces(nv, faces, cl)
    quad = quadrics(verts, faces, cl, lat) if placement == "quadric" else None
    cverts, crgb, _, pcounts = place(verts, rgb, cl, lat, quad, placement, reg)
    v, f, c = _compact(cverts, crgb, fc, m, nf, drop_unreferenced)
    adj = mesh_clean.adjacency(int(v.shape[0]), f)
    invalid, unclustered, collapsed, duplicate, *fallbacks = (int(t) for t in torch.cat([fc["counts"], pcounts]).cpu())      # the seven counters, one read
    stats.update({"vertices_out": int(v.shape[0]), "faces_out": int(f.shape[0]), "clusters": m, "unclustered_vertices": nv - clustered,
                  "invalid_faces": invalid, "unclustered_faces": unclustered, "collapsed_faces": collapsed, "duplicate_faces": duplicate,
                  "fallback_no_faces": fallbacks[0], "fallback_singular": fallbacks[1], "fallback_outside": fallbacks[2], "edges": adj["edges"],
                  "boundary_edges": adj["boundary_edges"], "nonmanifold_edges": adj["nonmanifold_edges"],
                  "euler_characteristic": adj["referenced_vertices"] - adj["edges"] + int(f.shape[0])})
    return v, f, c, stats


def decimate_options(cell=0.0, voxels=0.0):
    """The mesh path's two options (an absolute cell edge, or one in voxels of the volume, not both) -> {"cell": ...} or {"voxels":
    ...} for decimate_mesh_path, or None when neither asks for anything"""
    if cell and voxels:
        raise _lib.RcmvsError("decimate: give the cell in world units or in voxels, not both")
    for name, value in (("cell", cell), ("voxels", voxels)):
        if value and not (math.isfinite(float(value)) and float(value) > 0):
            raise _lib.RcmvsError(f"decimate: {name} = {value} (finite, > 0)")
    if cell:
        return {"cell": float(cell)}
    if voxels:
        return {"voxels": float(voxels)}
    return None


def decimate_mesh_path(verts, faces, rgb, options, voxel):
    """decimate for the mesh path: ``options`` from decimate_options, ``voxel`` the volume's voxel edge -> (verts, faces, rgb, stats)"""
    cell = options["cell"] if "cell" in options else options["voxels"] * float(voxel)
    return decimate(verts, faces, rgb, cell=cell)


def main(argv=None):
    from . import dtu_io, tsdf_mesh
    ap = argparse.ArgumentParser(description="decimate a PLY mesh by vertex clustering with quadric placement")
    ap.add_argument("--in", dest="src", required=True, help="the PLY to read (positions, triangles, vertex colours when it has them)")
    ap.add_argument("--out", required=True, help="the PLY to write")
    ap.add_argument("--cell", type=float, required=True, help="edge of the clustering lattice's cells, world units")
    ap.add_argument("--placement", choices=sorted(PLACEMENTS), default="quadric")
    ap.add_argument("--reg", type=float, default=DEFAULT_REG, help="regularisation of the quadric towards the members' mean")
    ap.add_argument("--keep-unreferenced", action="store_true", help="keep the clusters no surviving face uses")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    verts, faces, rgb = dtu_io.read_ply_mesh_rgb(a.src)
    dev = torch.device(a.device)
    v, f, c, stats = decimate(torch.from_numpy(np.ascontiguousarray(verts, np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(faces, np.int32)).to(dev),
                              None if rgb is None else torch.from_numpy(np.ascontiguousarray(rgb, np.uint8)).to(dev), cell=a.cell, placement=a.placement,
                              reg=a.reg, drop_unreferenced=not a.keep_unreferenced)
    with open(a.out, "wb") as out:
        out.write(tsdf_mesh.mesh_ply_bytes(v, f, c))
    summary = dict({"in": a.src, "out": a.out}, **stats)
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
