"""Hole filling of an extracted triangle mesh on the HIP path (csrc/mesh_holes.hip; the contract and the rule are
csrc/mesh_holes.h, the per-element rules csrc/mesh_holes_math.h, restated by tests/mesh_holes_oracle.py): the boundary half-edges
(edges of multiplicity 1 in mesh_clean's 1-ring), the closed loops they form, and over every loop of at most ``max_edges`` edges
one reversed face (three edges) or a fan of triangles round the members' mean.

``fill_holes`` takes what ``TsdfVolume.extract`` or ``mesh_clean.compact`` returns and gives back the same three device tensors,
the input in every bit followed by the new vertices and faces in ascending order of each loop's smallest vertex number, plus a
dict of counts; ``boundary`` is callable on its own.  The host reads a handful of totals; there is no per-vertex host pass.

    python -m rc_mvsnet_amd.mesh_clean --in a.ply --out b.ply --keep-largest 1 --fill-holes 64

Limits: a fan from the centroid is right for small, roughly flat, star-shaped holes and folds on others; the rim of an open patch
shorter than ``max_edges`` is a loop too and gets closed, so run this after component removal and choose ``max_edges`` below the
rim of the observed region; a loop through a complex vertex (a bow-tie, a non-manifold edge's fan, neighbours of inconsistent
orientation) is skipped and counted; a lone triangle becomes two-sided; at most 4096 edges a loop.  No CPU fallback."""
import torch

from . import _lib, fusion, mesh_clean
from .mesh_clean import _count, _faces, _mesh, _ptr, _scan_work

MAX_EDGES, SCAN_TILE, SCAN_WORK = (_lib.CONSTANTS["RCMVS_MH_" + k] for k in ("MAX_EDGES", "SCAN_TILE", "SCAN_WORK"))
NONE, SIMPLE, COMPLEX = (_lib.CONSTANTS["RCMVS_MH_" + k] for k in ("NONE", "SIMPLE", "COMPLEX"))
MAX_COUNT = 2 ** 31                                               # a mesh whose vertices or faces would reach this is refused


def max_edges_argument(value, what):
    """the loop length limit as an int, refused outside 3 .. MAX_EDGES"""
    value = _count(value, "max_edges", what)
    if not 3 <= value <= MAX_EDGES:
        raise _lib.RcmvsError(f"{what}: max_edges = {value} (3 .. {MAX_EDGES})")
    return value


def check_output_counts(nv, nf, vertices_added, faces_added, what):
    if nv + vertices_added >= MAX_COUNT or nf + faces_added >= MAX_COUNT:
        raise _lib.RcmvsError(f"{what}: {nv} + {vertices_added} vertices, {nf} + {faces_added} faces (each sum must stay below 2^31)")


def boundary(verts_n, faces, adj=None):
    """The boundary half-edges of a mesh of verts_n vertices (adj: mesh_clean.adjacency of the same faces, built when None) -> dict:
    succ and pred (verts_n int32: the next / previous vertex along the boundary at a simple vertex, -1 elsewhere), flags (verts_n
    uint8: NONE / SIMPLE / COMPLEX), out_count and in_count (verts_n int32), all on the device, and the integers boundary_edges and
    complex_vertices."""
    what = "mesh_holes.boundary"
    nf = _faces(faces, what)
    nv = _count(verts_n, "verts_n", what)
    if adj is None:
        adj = mesh_clean.adjacency(nv, faces)
    if adj["verts_n"] != nv or int(adj["nbr"].numel()) != 6 * nf:
        raise _lib.RcmvsError(f"{what}: the adjacency is of {adj['verts_n']} vertices and {int(adj['nbr'].numel()) // 6} faces, the mesh has {nv} and {nf}")
    dev = faces.device
    out_count, in_count, succ, pred = (torch.empty(nv, device=dev, dtype=torch.int32) for _ in range(4))
    flags = torch.empty(nv, device=dev, dtype=torch.uint8)
    counts = torch.empty(2, device=dev, dtype=torch.int64)
    _lib.call("rcmvs_mh_boundary", _ptr(faces, "faces", torch.int32), nv, nf, fusion._chk(adj["row_start"], "row_start", torch.int32),
              _ptr(adj["row_len"], "row_len", torch.int32), _ptr(adj["nbr"], "nbr", torch.int32), _ptr(adj["mult"], "mult", torch.int32), 6 * nf,
              _ptr(out_count, "out_count", torch.int32), _ptr(in_count, "in_count", torch.int32), _ptr(succ, "succ", torch.int32),
              _ptr(pred, "pred", torch.int32), _ptr(flags, "flags", torch.uint8), _ptr(counts, "counts", torch.int64), fusion._stream())
    edges, complex_vertices = (int(t) for t in counts.cpu())
    return {"verts_n": nv, "succ": succ, "pred": pred, "flags": flags, "out_count": out_count, "in_count": in_count, "boundary_edges": edges,
            "complex_vertices": complex_vertices}


def leaders(bnd, max_edges):
    """The loops of at most max_edges edges of ``boundary``'s result -> dict: loop_len (verts_n int32: the length at a filled loop's
    smallest vertex, 0 elsewhere), vert_rank and face_rank (verts_n + 1 int32: where each loop's new vertex and faces go, the
    totals last), and the integers vertices_added, faces_added, loops_filled, loops_filled_by_one_face, longest_filled."""
    what = "mesh_holes.leaders"
    max_edges = max_edges_argument(max_edges, what)
    nv, succ = bnd["verts_n"], bnd["succ"]
    dev = succ.device
    loop_len = torch.empty(nv, device=dev, dtype=torch.int32)
    vert_count = torch.empty(nv, device=dev, dtype=torch.uint8)
    face_count = torch.empty(nv, device=dev, dtype=torch.int32)
    vert_rank = torch.empty(nv + 1, device=dev, dtype=torch.int32)
    face_rank = torch.empty(nv + 1, device=dev, dtype=torch.int32)
    totals = torch.empty(5, device=dev, dtype=torch.int64)
    work = _scan_work(nv, dev)
    _lib.call("rcmvs_mh_leaders", _ptr(succ, "succ", torch.int32), _ptr(bnd["pred"], "pred", torch.int32), nv, max_edges,
              _ptr(loop_len, "loop_len", torch.int32), _ptr(vert_count, "vert_count", torch.uint8), _ptr(face_count, "face_count", torch.int32),
              fusion._chk(vert_rank, "vert_rank", torch.int32), fusion._chk(face_rank, "face_rank", torch.int32),
              fusion._chk(work, "scan_work", torch.int32), _ptr(totals, "totals", torch.int64), fusion._stream())
    va, fa, loops, single, longest = (int(t) for t in totals.cpu())
    return {"loop_len": loop_len, "vert_rank": vert_rank, "face_rank": face_rank, "vertices_added": va, "faces_added": fa, "loops_filled": loops,
            "loops_filled_by_one_face": single, "longest_filled": longest}


def emit(verts, faces, rgb, bnd, led):
    """The input mesh followed by the new vertices and faces of ``leaders``' loops -> (verts, faces, rgb)"""
    what = "mesh_holes.emit"
    nv, nf = _mesh(verts, faces, rgb, what)
    if bnd["verts_n"] != nv:
        raise _lib.RcmvsError(f"{what}: the boundary is of {bnd['verts_n']} vertices, verts has {nv}")
    check_output_counts(nv, nf, led["vertices_added"], led["faces_added"], what)
    dev = verts.device
    nv_out, nf_out = nv + led["vertices_added"], nf + led["faces_added"]
    out_verts = torch.empty((nv_out, 3), device=dev, dtype=torch.float32)
    out_faces = torch.empty((nf_out, 3), device=dev, dtype=torch.int32)
    out_rgb = None if rgb is None else torch.empty((nv_out, 3), device=dev, dtype=torch.uint8)
    _lib.call("rcmvs_mh_emit", _ptr(verts, "verts", torch.float32), _ptr(rgb, "rgb", torch.uint8), _ptr(faces, "faces", torch.int32), nv, nf,
              _ptr(bnd["succ"], "succ", torch.int32), _ptr(led["loop_len"], "loop_len", torch.int32), fusion._chk(led["vert_rank"], "vert_rank", torch.int32),
              fusion._chk(led["face_rank"], "face_rank", torch.int32), nv_out, nf_out, _ptr(out_verts, "out_verts", torch.float32),
              _ptr(out_rgb, "out_rgb", torch.uint8), _ptr(out_faces, "out_faces", torch.int32), fusion._stream())
    return out_verts, out_faces, out_rgb


def fill_holes(verts, faces, rgb=None, *, max_edges):
    """Closes every boundary loop of at most ``max_edges`` edges (3 .. 4096): a loop of three with one reversed face, a longer one
    with a fan round the members' mean, whose colour is the members' mean colour -> (verts, faces, rgb, stats).  The input comes
    first in every bit; loops through complex vertices stay open and are counted in stats["complex_vertices"]."""
    what = "mesh_holes.fill_holes"
    nv, nf = _mesh(verts, faces, rgb, what)
    max_edges = max_edges_argument(max_edges, what)
    bnd = boundary(nv, faces, mesh_clean.adjacency(nv, faces))
    led = leaders(bnd, max_edges)
    v, f, c = emit(verts, faces, rgb, bnd, led)
    closed = led["faces_added"] + 2 * led["loops_filled_by_one_face"]          # the filled loops' lengths: L faces each, 1 for L == 3
    stats = {"boundary_edges": bnd["boundary_edges"], "complex_vertices": bnd["complex_vertices"],
             "loops_filled": led["loops_filled"], "loops_filled_by_one_face": led["loops_filled_by_one_face"], "longest_filled": led["longest_filled"],
             "vertices_added": led["vertices_added"], "faces_added": led["faces_added"], "boundary_edges_left": bnd["boundary_edges"] - closed}
    return v, f, c, stats
