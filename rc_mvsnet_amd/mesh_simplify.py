"""Simplification of a triangle mesh on the HIP path (csrc/mesh_simplify.hip; the contract is csrc/mesh_simplify.h, the per-element
rules and their operation order csrc/mesh_simplify_math.h, restated by tests/mesh_simplify_oracle.py): quadric edge collapse, one
independent set of edges a round ("Mesh simplification").

``simplify`` takes what ``TsdfVolume.extract``, ``mesh_clean.clean_mesh`` or ``mesh_decimate.decimate`` returns and gives back the
same three device tensors plus a dict of counts; ``begin``, ``round`` and ``finish`` are its parts, callable on their own.  The
result is defined exactly: quadrics live in the frame of the finite vertices' box, a vertex's quadric is the fp64 sum of its
corners' planes in ascending (face, corner) order, a round collapses the edges that are the cheapest candidate within the closed
rings of both their ends (first to last CSR entry up to the budget), and the survivors keep their input order.  A vertex on the
rim, on a non-manifold edge or with a non-finite coordinate is locked: it keeps its position in every bit and is never removed.
The host reads the box (32 bytes), the init counters, one array of 16 counters per round -- the loop's only read -- and the two
final sizes.

    python -m rc_mvsnet_amd.mesh_simplify --in a.ply --out b.ply --ratio 0.25

``max_error`` bounds an edge's cost: the sum over the planes merged into its two ends of (2 area x distance to the plane) ^ 2 at
the new position, all lengths in units of the longest side of the mesh's box.

Limits: 6 nf <= 2^31 - 1; one lane per edge and per vertex segment (a vertex of very high valence is slow); the rim and the
non-manifold parts stay at full resolution; a colour is the mean of the merged vertices' colours, not an attribute of the quadric; a
round collapses only edges that are no neighbours of each other, so a low ratio takes tens of rounds.  No CPU fallback."""
import argparse
import ctypes
import json
import math

import numpy as np
import torch

from . import _lib, fusion, mesh_clean, mesh_decimate
from .mesh_clean import _count, _mesh, _ptr, _scan_work

C = _lib.CONSTANTS
SORT_BLOCK, MAX_CORNERS, QUADRIC_DOUBLES, COUNTS = (C["RCMVS_MS_" + k] for k in ("SORT_BLOCK", "MAX_CORNERS", "QUADRIC_DOUBLES", "COUNTS"))
PATH_LOCKED, PATH_QUADRIC, PATH_MIDPOINT, PATH_END_U, PATH_END_V = (C["RCMVS_MS_PATH_" + k] for k in ("LOCKED", "QUADRIC", "MIDPOINT", "END_U", "END_V"))
EDGE_OK, EDGE_COST, EDGE_LINK, EDGE_FLIP, EDGE_NONE = (C["RCMVS_MS_EDGE_" + k] for k in ("OK", "COST", "LINK", "FLIP", "NONE"))
COUNT = {k[len("RCMVS_MS_COUNT_"):].lower(): v for k, v in C.items() if k.startswith("RCMVS_MS_COUNT_")}
PATH_NAMES = ("locked", "quadric", "midpoint", "end_u", "end_v")
NO_KEY = 2 ** 64 - 1
STOPS = ("target", "nothing_selected", "max_rounds")


def _sizes(nv, nf, what):
    if 6 * nf > mesh_clean.MAX_ENTRIES or 3 * nf > MAX_CORNERS:
        raise _lib.RcmvsError(f"{what}: {nf} faces (at most {mesh_clean.MAX_ENTRIES // 6}: 2^31 - 1 directed entries)")


def frame(lo, hi):
    """ms::centre and ms::side of the box lo .. hi (float32, or None for no finite vertex) -> [centre x, y, z, side]"""
    if lo is None:
        return [0.0, 0.0, 0.0, 1.0]
    lo, hi = np.asarray(lo, np.float32).astype(np.float64), np.asarray(hi, np.float32).astype(np.float64)
    side = float(np.max(hi - lo))
    return [float(c) for c in (lo + hi) * 0.5] + [side if side > 0.0 else 1.0]


def unordered_cost(bits):
    """the fp32 cost behind the high half of a key (md::ordered bits; 0: none) -> float"""
    bits = int(bits)
    if bits == 0:
        return 0.0
    raw = (bits & 0x7fffffff) if bits & 0x80000000 else (~bits & 0xffffffff)
    return float(np.array([raw], np.uint32).view(np.float32)[0])


def begin(verts, faces, rgb=None):
    """The state a simplification carries from round to round -> dict: verts (a copy that the rounds write), faces (the current
    face array), quad (nv, 10) float64, members (nv) int32, csum (nv, 3) int64 or None, live (the valid faces), frame,
    nonfinite_faces, nonfinite_vertices, and the work buffers.  One host read of the box, one of the four counters."""
    what = "mesh_simplify.begin"
    nv, nf = _mesh(verts, faces, rgb, what)
    _sizes(nv, nf, what)
    dev = verts.device
    lo, hi, _ = mesh_decimate.bounds(verts)
    fr = frame(lo, hi)
    n, e = 3 * nf, 6 * nf
    table = 256 * ((n + SORT_BLOCK - 1) // SORT_BLOCK)
    i32 = lambda *shape: torch.empty(shape, device=dev, dtype=torch.int32)       # noqa: E731
    i64 = lambda *shape: torch.empty(shape, device=dev, dtype=torch.int64)       # noqa: E731
    u8 = lambda *shape: torch.empty(shape, device=dev, dtype=torch.uint8)        # noqa: E731
    s = {"nv": nv, "nf": nf, "frame": fr, "verts": verts.clone(), "faces": faces.clone(), "faces_next": torch.empty_like(faces),
         "quad": torch.empty((nv, QUADRIC_DOUBLES), device=dev, dtype=torch.float64), "members": i32(nv), "csum": None if rgb is None else i64(nv, 3),
         "live_dev": i64(1), "key_a": i32(n), "idx_a": i32(n), "key_b": i32(n), "idx_b": i32(n), "hist": i32(table), "hist_start": i32(table + 1),
         "scan_work": _scan_work(max(e, table, nv), dev), "seg": i32(2 * nv), "row_start": i32(nv + 1), "row_len": i32(nv), "nbr": i32(e), "mult": i32(e),
         "on_boundary": u8(nv), "cursor": i32(nv), "heavy": i32(e // (mesh_clean.SORT_LIMIT + 1) + 1), "adj_stats": i64(6), "locked": u8(nv), "edge": u8(e),
         "key": i64(e), "best1": i64(nv), "best2": i64(nv), "selected": u8(e), "rank": i32(e + 1), "applied": u8(e), "remap": i32(nv), "counts": i64(COUNTS)}
    s["frame_host"] = (ctypes.c_double * 4)(*fr)                 # stays alive with the state
    stats = i64(4)
    _lib.call("rcmvs_ms_init", _ptr(s["verts"], "verts", torch.float32), _ptr(s["faces"], "faces", torch.int32), _ptr(rgb, "rgb", torch.uint8), nv, nf,
              ctypes.cast(s["frame_host"], ctypes.c_void_p), *_sort_args(s), _ptr(s["seg"], "seg", torch.int32), _ptr(s["quad"], "quad", torch.float64),
              _ptr(s["members"], "members", torch.int32), _ptr(s["csum"], "csum", torch.int64), _ptr(s["live_dev"], "live", torch.int64),
              _ptr(stats, "stats", torch.int64), fusion._stream())
    s["nonfinite_faces"], s["nonfinite_vertices"], s["live"], _ = (int(t) for t in stats.cpu())
    return s


def _sort_args(s):
    return [_ptr(s[k], k, torch.int32) for k in ("key_a", "idx_a", "key_b", "idx_b", "hist", "hist_start", "scan_work")]


def round(state, target_faces, max_error=math.inf, timed=None):
    """One round on the state of ``begin``: topology, candidates, the independent set, the budget, the collapses -> dict of this
    round's device arrays (views of the state's buffers, valid until the next round: row_start, row_len, nbr, mult, locked, edge,
    key, best1, best2, selected, applied, remap) and the host integers of its counters (locked, candidates, reject_cost,
    reject_link, reject_flip, paths (5), selected, applied, max_cost, live, live_before).  The state's verts, quad, members, csum
    and faces are the mesh after the round.  One host read of the 16 counters.  timed: (phase, ev0, ev1) for the _timed twin (a
    RCMVS_MS_PHASE_* value and two event handles that bracket that phase's launches)."""
    what = "mesh_simplify.round"
    s = state
    target_faces = _count(target_faces, "target_faces", what)
    max_error = _max_error(max_error, what)
    p32 = lambda k: _ptr(s[k], k, torch.int32)                   # noqa: E731
    p64 = lambda k: _ptr(s[k], k, torch.int64)                   # noqa: E731
    p8 = lambda k: _ptr(s[k], k, torch.uint8)                    # noqa: E731
    _lib.call("rcmvs_ms_round" if timed is None else "rcmvs_ms_round_timed", _ptr(s["verts"], "verts", torch.float32), p32("faces"), p32("faces_next"), s["nv"], s["nf"],
              ctypes.cast(s["frame_host"], ctypes.c_void_p), _ptr(s["quad"], "quad", torch.float64), p32("members"), p64("csum") if s["csum"] is not None else _ptr(None, "", None),
              target_faces, max_error, p32("row_start"), p32("row_len"), p32("nbr"), p32("mult"), p8("on_boundary"), p32("cursor"), p32("heavy"),
              int(s["heavy"].numel()), p64("adj_stats"), *_sort_args(s), p32("seg"), p8("locked"), p8("edge"), p64("key"), p64("best1"), p64("best2"),
              p8("selected"), p32("rank"), p8("applied"), p32("remap"), p64("live_dev"), p64("counts"), *(() if timed is None else timed), fusion._stream())
    s["faces"], s["faces_next"] = s["faces_next"], s["faces"]
    c = [int(t) for t in s["counts"].cpu()]                      # the round's only read
    s["live"] = c[COUNT["live"]]
    out = {k: s[k] for k in ("row_start", "row_len", "nbr", "mult", "locked", "edge", "key", "best1", "best2", "selected", "applied", "remap")}
    out.update({"locked_vertices": c[COUNT["locked"]], "candidates": c[COUNT["candidates"]], "reject_cost": c[COUNT["reject_cost"]],
                "reject_link": c[COUNT["reject_link"]], "reject_flip": c[COUNT["reject_flip"]], "paths": c[COUNT["path"]:COUNT["path"] + 5],
                "selected_edges": c[COUNT["selected"]], "applied_edges": c[COUNT["applied"]], "max_cost": unordered_cost(c[COUNT["max_cost"]]),
                "live": c[COUNT["live"]], "live_before": c[COUNT["live_before"]]})
    return out


def finish(state, drop_unreferenced=True):
    """The mesh of the state: the valid faces and (drop_unreferenced) the vertices they use, else every vertex that was not merged
    away, in input order through mesh_clean's gather; colours from the sums -> (verts, faces, rgb).  One host read of the sizes."""
    s = state
    nv, nf, dev = s["nv"], s["nf"], s["verts"].device
    face_keep = torch.empty(nf, device=dev, dtype=torch.uint8)
    vert_keep = torch.empty(nv, device=dev, dtype=torch.uint8)
    face_rank = torch.empty(nf + 1, device=dev, dtype=torch.int32)
    vert_rank = torch.empty(nv + 1, device=dev, dtype=torch.int32)
    rgb = None if s["csum"] is None else torch.empty((nv, 3), device=dev, dtype=torch.uint8)
    totals = torch.empty(2, device=dev, dtype=torch.int64)
    work = _scan_work(max(nv, nf), dev)
    _lib.call("rcmvs_ms_finish", _ptr(s["faces"], "faces", torch.int32), nv, nf, _ptr(s["members"], "members", torch.int32), _ptr(s["csum"], "csum", torch.int64),
              1 if drop_unreferenced else 0, _ptr(face_keep, "face_keep", torch.uint8), _ptr(vert_keep, "vert_keep", torch.uint8),
              _ptr(face_rank, "face_rank", torch.int32), _ptr(vert_rank, "vert_rank", torch.int32), _ptr(work, "scan_work", torch.int32),
              _ptr(rgb, "out_rgb", torch.uint8), _ptr(totals, "totals", torch.int64), fusion._stream())
    nf_out, nv_out = (int(t) for t in totals.cpu())               # the final sizes
    out_verts = torch.empty((nv_out, 3), device=dev, dtype=torch.float32)
    out_faces = torch.empty((nf_out, 3), device=dev, dtype=torch.int32)
    out_rgb = None if rgb is None else torch.empty((nv_out, 3), device=dev, dtype=torch.uint8)
    _lib.call("rcmvs_mc_gather", _ptr(s["verts"], "verts", torch.float32), _ptr(rgb, "rgb", torch.uint8), _ptr(s["faces"], "faces", torch.int32),
              _ptr(face_keep, "face_keep", torch.uint8), _ptr(face_rank, "face_rank", torch.int32), _ptr(vert_keep, "vert_keep", torch.uint8),
              _ptr(vert_rank, "vert_rank", torch.int32), nv, nf, nv_out, nf_out, _ptr(out_verts, "out_verts", torch.float32),
              _ptr(out_rgb, "out_rgb", torch.uint8), _ptr(out_faces, "out_faces", torch.int32), fusion._stream())
    return out_verts, out_faces, out_rgb


def _max_error(value, what):
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise _lib.RcmvsError(f"{what}: max_error = {value!r} (a number >= 0, inf allowed)") from None
    if not value >= 0.0:
        raise _lib.RcmvsError(f"{what}: max_error = {value} (>= 0, inf allowed)")
    return value


def _target(target_faces, ratio, what):
    """exactly one of the two -> ("faces", n) or ("ratio", r)"""
    if (target_faces is None) == (ratio is None):
        raise _lib.RcmvsError(f"{what}: give exactly one of target_faces and ratio")
    if target_faces is not None:
        return "faces", _count(target_faces, "target_faces", what)
    ratio = mesh_clean._real(ratio, "ratio", what)
    if not 0.0 <= ratio <= 1.0:
        raise _lib.RcmvsError(f"{what}: ratio = {ratio} (0 .. 1)")
    return "ratio", ratio


def simplify(verts, faces, rgb=None, *, target_faces=None, ratio=None, max_error=math.inf, max_rounds=256, drop_unreferenced=True):
    """Collapses edges, cheapest first within every neighbourhood, until at most ``target_faces`` valid faces are left (``ratio``:
    floor(ratio x the valid faces)), no edge can be collapsed at a cost of at most ``max_error``, or ``max_rounds`` rounds have run
    -> (verts, faces, rgb, stats); stats["stop"] says which."""
    what = "mesh_simplify.simplify"
    nv, nf = _mesh(verts, faces, rgb, what)
    _sizes(nv, nf, what)
    kind, goal = _target(target_faces, ratio, what)
    max_error = _max_error(max_error, what)
    max_rounds = _count(max_rounds, "max_rounds", what)
    s = begin(verts, faces, rgb)
    valid = s["live"]
    target = goal if kind == "faces" else int(math.floor(goal * valid))
    stats = {"vertices_in": nv, "faces_in": nf, "valid_faces_in": valid, "target_faces": target, "max_error": max_error, "max_rounds": max_rounds,
             "nonfinite_faces": s["nonfinite_faces"], "nonfinite_vertices": s["nonfinite_vertices"]}
    collapses, locked, rejected, paths, worst, stop = [], 0, [0, 0, 0], [0] * 5, 0.0, None
    while stop is None:
        if s["live"] <= target:
            stop = "target"
        elif len(collapses) >= max_rounds:
            stop = "max_rounds"
        else:
            r = round(s, target, max_error)
            if not collapses:
                locked = r["locked_vertices"]
            collapses.append(r["applied_edges"])
            rejected = [a + r[k] for a, k in zip(rejected, ("reject_cost", "reject_link", "reject_flip"))]
            paths = [a + b for a, b in zip(paths, r["paths"])]
            worst = max(worst, r["max_cost"])
            if r["selected_edges"] == 0:
                stop = "nothing_selected"
    v, f, c = finish(s, drop_unreferenced)
    stats.update({"vertices_out": int(v.shape[0]), "faces_out": int(f.shape[0]), "rounds": len(collapses), "collapses": collapses, "locked_vertices": locked,
                  "rejected_cost": rejected[0], "rejected_link": rejected[1], "rejected_flip": rejected[2],
                  **{"placed_" + name: paths[i] for i, name in enumerate(PATH_NAMES)}, "max_cost": worst, "stop": stop})
    return v, f, c, stats


def simplify_options(faces=0, ratio=0.0, max_error=None):
    """The mesh path's options (a face count or a ratio, not both) -> the keywords of ``simplify``, or None when neither asks for
    anything"""
    if faces and ratio:
        raise _lib.RcmvsError("simplify: give the target as a face count or as a ratio, not both")
    if not faces and not ratio:
        if max_error is not None:
            raise _lib.RcmvsError("simplify: max_error needs a target (a face count or a ratio)")
        return None
    kind, goal = _target(faces or None, ratio or None, "simplify")
    kw = {"target_faces": goal} if kind == "faces" else {"ratio": goal}
    if max_error is not None:
        kw["max_error"] = _max_error(max_error, "simplify")
    return kw


def main(argv=None):
    from . import dtu_io, tsdf_mesh
    ap = argparse.ArgumentParser(description="simplify a PLY mesh by quadric edge collapse in independent sets")
    ap.add_argument("--in", dest="src", required=True, help="the PLY to read (positions, triangles, vertex colours when it has them)")
    ap.add_argument("--out", required=True, help="the PLY to write")
    goal = ap.add_mutually_exclusive_group(required=True)
    goal.add_argument("--faces", type=int, default=None, help="the number of faces to reach")
    goal.add_argument("--ratio", type=float, default=None, help="the fraction of the valid faces to reach")
    ap.add_argument("--max-error", type=float, default=math.inf, help="no collapse above this cost (module docstring)")
    ap.add_argument("--max-rounds", type=int, default=256)
    ap.add_argument("--keep-unreferenced", action="store_true", help="keep the surviving vertices no face uses")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    verts, faces, rgb = dtu_io.read_ply_mesh_rgb(a.src)
    dev = torch.device(a.device)
    v, f, c, stats = simplify(torch.from_numpy(np.ascontiguousarray(verts, np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(faces, np.int32)).to(dev),
                              None if rgb is None else torch.from_numpy(np.ascontiguousarray(rgb, np.uint8)).to(dev), target_faces=a.faces, ratio=a.ratio,
                              max_error=a.max_error, max_rounds=a.max_rounds, drop_unreferenced=not a.keep_unreferenced)
    with open(a.out, "wb") as out:
        out.write(tsdf_mesh.mesh_ply_bytes(v, f, c))
    summary = dict({"in": a.src, "out": a.out}, **stats)
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
