"""numpy restatement of the hole-filling pass (csrc/mesh_holes.h; rc_mvsnet_amd/mesh_holes.py): boundary half-edges from the edge
multiplicities of the valid faces, simple and complex vertices, the loops of simple vertices found by plain walks in ascending
vertex order, one reversed face or a fan round the members' mean per loop of at most max_edges edges.  Integers throughout; the
mean is summed member by member in fp64 in loop order from the leader and rounded to fp32 once.  Compaction, the 1-ring and the
smoothing of the clean-up composite are tests/mesh_clean_oracle.py's."""
import numpy as np

import mesh_clean_oracle as MCO

MAX_EDGES = 4096
NONE, SIMPLE, COMPLEX = 0, 1, 2


class Refused(ValueError):
    pass


def boundary(nv, faces):
    """-> dict: succ, pred (nv int32), flags (nv uint8), out_count, in_count (nv int32), boundary_edges, complex_vertices"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[MCO.valid_faces(f, nv)]
    tail, head = f.ravel(), f[:, [1, 2, 0]].ravel()               # a->b, b->c, c->a of every valid face
    key = np.minimum(tail, head) * max(nv, 1) + np.maximum(tail, head)
    _, inverse, count = np.unique(key, return_inverse=True, return_counts=True)
    alone = count[inverse.reshape(-1)] == 1 if len(key) else np.zeros(0, bool)
    tail, head = tail[alone], head[alone]
    out_count = np.bincount(tail, minlength=nv).astype(np.int32) if nv else np.zeros(0, np.int32)
    in_count = np.bincount(head, minlength=nv).astype(np.int32) if nv else np.zeros(0, np.int32)
    simple = (out_count == 1) & (in_count == 1)
    flags = np.where(simple, SIMPLE, np.where((out_count > 0) | (in_count > 0), COMPLEX, NONE)).astype(np.uint8)
    succ, pred = np.full(nv, -1, np.int32), np.full(nv, -1, np.int32)
    leaves, arrives = simple[tail] if nv else np.zeros(0, bool), simple[head] if nv else np.zeros(0, bool)
    succ[tail[leaves]] = head[leaves]
    pred[head[arrives]] = tail[arrives]
    return {"succ": succ, "pred": pred, "flags": flags, "out_count": out_count, "in_count": in_count, "boundary_edges": int(len(tail)),
            "complex_vertices": int((flags == COMPLEX).sum())}


def loops(bnd):
    """every loop of simple vertices as the list of its vertices from its smallest one, in ascending order of that vertex"""
    succ, flags = bnd["succ"], bnd["flags"]
    seen = np.zeros(len(succ), bool)
    found = []
    for v in np.nonzero(flags == SIMPLE)[0]:
        if seen[v]:
            continue
        chain, cur = [int(v)], int(succ[v])
        seen[v] = True
        while cur != v and flags[cur] == SIMPLE and not seen[cur]:
            chain.append(cur)
            seen[cur] = True
            cur = int(succ[cur])
        if cur == v:
            assert len(chain) >= 3 and min(chain) == chain[0]
            found.append(chain)
    return found


def fill_holes(verts, faces, rgb=None, max_edges=None):
    """-> verts, faces, rgb, stats (as mesh_holes.fill_holes), and the filled loops"""
    if isinstance(max_edges, bool) or not isinstance(max_edges, (int, np.integer)) or not 3 <= max_edges <= MAX_EDGES:
        raise Refused(f"max_edges = {max_edges!r} (3 .. {MAX_EDGES})")
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    c = None if rgb is None else np.asarray(rgb, np.uint8).reshape(-1, 3)
    nv = len(v)
    bnd = boundary(nv, f)
    filled = [loop for loop in loops(bnd) if len(loop) <= max_edges]
    new_v, new_c, new_f = [], [], []
    for loop in filled:
        L = len(loop)
        if L == 3:
            new_f.append([loop[0], loop[2], loop[1]])
            continue
        centre = nv + len(new_v)
        s = np.zeros(3, np.float64)
        with np.errstate(all="ignore"):
            for u in loop:
                s = s + v[u].astype(np.float64)
            new_v.append((s / np.float64(L)).astype(np.float32))
        if c is not None:
            total = c[loop].astype(np.int64).sum(0)
            new_c.append(((2 * total + L) // (2 * L)).astype(np.uint8))
        new_f.extend([loop[(i + 1) % L], loop[i], centre] for i in range(L))
    if nv + len(new_v) >= 2 ** 31 or len(f) + len(new_f) >= 2 ** 31:
        raise Refused("the filled mesh would reach 2^31 vertices or faces")
    out_v = np.concatenate([v, np.asarray(new_v, np.float32).reshape(-1, 3)])
    out_f = np.concatenate([f, np.asarray(new_f, np.int32).reshape(-1, 3)])
    out_c = None if c is None else np.concatenate([c, np.asarray(new_c, np.uint8).reshape(-1, 3)])
    closed = sum(len(loop) for loop in filled)
    stats = {"boundary_edges": bnd["boundary_edges"], "complex_vertices": bnd["complex_vertices"], "loops_filled": len(filled),
             "loops_filled_by_one_face": sum(len(loop) == 3 for loop in filled), "longest_filled": max((len(loop) for loop in filled), default=0),
             "vertices_added": len(new_v), "faces_added": len(new_f), "boundary_edges_left": bnd["boundary_edges"] - closed}
    return out_v, out_f, out_c, stats, filled


_fill = fill_holes                                                # clean_mesh's option carries the function's name


def clean_mesh(verts, faces, rgb=None, min_faces=0, min_fraction=0.0, keep_largest=0, drop_unreferenced=True, smooth_iterations=0, lam=0.5, mu=-0.53,
               pin_boundary=True, fill_holes=0):
    """mesh_clean.clean_mesh with the filling between the compaction and the smoothing step's 1-ring"""
    if not fill_holes:
        return MCO.clean_mesh(verts, faces, rgb, min_faces, min_fraction, keep_largest, drop_unreferenced, smooth_iterations, lam, mu, pin_boundary)
    nv, nf = len(np.asarray(verts).reshape(-1, 3)), len(np.asarray(faces).reshape(-1, 3))
    v, f, c, info = MCO.compact(verts, faces, rgb, min_faces, min_fraction, keep_largest, drop_unreferenced)
    removed = nv - len(v)
    v, f, c, holes, _ = _fill(v, f, c, fill_holes)
    adj = MCO.adjacency(len(v), f)
    if smooth_iterations:
        v = MCO.taubin(v, adj, smooth_iterations, lam, mu, pin_boundary)
    stats = {"vertices_in": nv, "vertices_out": len(v), "faces_in": nf, "faces_out": len(f), "invalid_faces": info["invalid_faces"],
             "components_in": info["components_in"], "components_kept": info["components_kept"],
             "largest_component_faces": info["largest_component_faces"], "unreferenced_removed": removed, "edges": adj["edges"],
             "boundary_edges": adj["boundary_edges"], "nonmanifold_edges": adj["nonmanifold_edges"],
             "euler_characteristic": adj["referenced_vertices"] - adj["edges"] + len(f), "smooth_iterations": smooth_iterations, "holes": holes}
    return v, f, c, stats
