"""numpy restatement of the mesh clean-up pass (csrc/mesh_clean.h; rc_mvsnet_amd/mesh_clean.py): validation, connected components
over vertices with the smallest vertex number as the label, the three selection rules, stable compaction, the 1-ring with edge
multiplicities and Taubin smoothing.  Integers throughout, fp64 where the contract says fp64, and the smoothing adds the k-th
neighbour of every vertex in a loop over the rank k, so the order of the additions is the contract's."""
import numpy as np


def valid_faces(faces, nv):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    inside = ((f >= 0) & (f < nv)).all(1)
    distinct = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    return inside & distinct


def union_find_labels(nv, f):
    """integer union-find over the valid faces f, the smaller root wins -> label (nv int64)"""
    parent = np.arange(nv, dtype=np.int64)

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for a, b, c in f:
        for u, w in ((a, b), (b, c)):
            ru, rw = find(u), find(w)
            if ru != rw:
                parent[max(ru, rw)] = min(ru, rw)
    return np.array([find(v) for v in range(nv)], dtype=np.int64).reshape(-1)


def csgraph_labels(nv, f):
    """the same labels through scipy.sparse.csgraph (None when scipy does not import): its component numbers -> smallest member"""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        return None
    if nv == 0:
        return np.zeros(0, np.int64)
    src, dst = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
    _, comp = connected_components(coo_matrix((np.ones(len(src), np.int8), (src, dst)), shape=(nv, nv)), directed=False)
    smallest = np.full(int(comp.max()) + 1, nv, np.int64)
    np.minimum.at(smallest, comp, np.arange(nv))
    return smallest[comp]


def components(nv, faces, use_scipy=True):
    """-> label (nv int32), face_ok (nf uint8), comp_faces (nv int32), invalid (int)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = valid_faces(f, nv)
    label = csgraph_labels(nv, f[ok]) if use_scipy else None
    if label is None:
        label = union_find_labels(nv, f[ok])
    comp_faces = np.zeros(nv, np.int64)
    if ok.any():
        np.add.at(comp_faces, label[f[ok, 0]], 1)
    return label.astype(np.int32), ok.astype(np.uint8), comp_faces.astype(np.int32), int((~ok).sum())


def component_table(label, comp_faces):
    rows = np.nonzero((label == np.arange(len(label))) & (comp_faces > 0))[0]
    return np.stack([rows, comp_faces[rows]], 1).astype(np.int32).reshape(-1, 2)


def kept_labels(table, min_faces=0, min_fraction=0.0, keep_largest=0):
    """-> the set of kept labels"""
    if len(table) == 0:
        return set()
    most = int(table[:, 1].max())
    keep = (table[:, 1] >= min_faces) & (table[:, 1].astype(np.float64) >= np.float64(min_fraction) * np.float64(most))
    if keep_largest > 0:
        order = np.lexsort((table[:, 0], -table[:, 1].astype(np.int64)))
        top = np.zeros(len(table), bool)
        top[order[:keep_largest]] = True
        keep &= top
    return set(int(l) for l in table[keep, 0])


def compact(verts, faces, rgb, min_faces=0, min_fraction=0.0, keep_largest=0, drop_unreferenced=True):
    """-> verts, faces, rgb, info (as mesh_clean.compact)"""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    nv = len(verts)
    label, ok, comp_faces, invalid = components(nv, f)
    table = component_table(label, comp_faces)
    kept = kept_labels(table, min_faces, min_fraction, keep_largest)
    first = np.where(ok != 0, f[:, 0], 0)
    face_keep = (ok != 0) & np.isin(label[first] if nv else first, sorted(kept))
    vert_keep = np.zeros(nv, bool) if drop_unreferenced else np.ones(nv, bool)
    if drop_unreferenced:
        vert_keep[f[face_keep].ravel()] = True
    rank = np.cumsum(vert_keep) - vert_keep
    out_f = rank[f[face_keep]].astype(np.int32).reshape(-1, 3)
    info = {"components_in": len(table), "components_kept": len(kept), "largest_component_faces": int(table[:, 1].max()) if len(table) else 0,
            "faces_out": int(face_keep.sum()), "vertices_out": int(vert_keep.sum()), "invalid_faces": invalid}
    return verts[vert_keep], out_f, None if rgb is None else np.asarray(rgb, np.uint8).reshape(-1, 3)[vert_keep], info


def adjacency(nv, faces):
    """-> dict as mesh_clean.adjacency, numpy arrays"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[valid_faces(f, nv)]
    src = np.concatenate([f[:, 0], f[:, 0], f[:, 1], f[:, 1], f[:, 2], f[:, 2]])
    dst = np.concatenate([f[:, 1], f[:, 2], f[:, 0], f[:, 2], f[:, 0], f[:, 1]])
    raw = np.bincount(src, minlength=nv).astype(np.int64) if nv else np.zeros(0, np.int64)
    row_start = np.concatenate([[0], np.cumsum(raw)]).astype(np.int32)
    entries = 6 * len(np.asarray(faces).reshape(-1, 3))
    nbr, mult = np.full(entries, -1, np.int32), np.zeros(entries, np.int32)
    row_len, on_boundary = np.zeros(nv, np.int32), np.zeros(nv, np.uint8)
    nbr[int(row_start[-1]):], mult[int(row_start[-1]):] = -7, -7                   # beyond the last segment nothing is defined
    code, counts = np.unique(src * max(nv, 1) + dst, return_counts=True)
    pairs = np.stack([code // max(nv, 1), code % max(nv, 1)], 1)
    if nv:
        row_len = np.bincount(pairs[:, 0], minlength=nv).astype(np.int32)
        on_boundary = (np.bincount(pairs[:, 0], weights=(counts == 1), minlength=nv) > 0).astype(np.uint8)
        at = row_start[:-1].astype(np.int64)[pairs[:, 0]] + np.arange(len(pairs)) - (np.cumsum(row_len) - row_len)[pairs[:, 0]]
        nbr[at], mult[at] = pairs[:, 1], counts
    once = pairs[:, 0] < pairs[:, 1]
    return {"verts_n": nv, "row_start": row_start, "row_len": row_len, "nbr": nbr, "mult": mult, "on_boundary": on_boundary, "defined": int(row_start[-1]),
            "edges": int(once.sum()), "boundary_edges": int((counts[once] == 1).sum()), "nonmanifold_edges": int((counts[once] > 2).sum()),
            "referenced_vertices": int((row_len > 0).sum())}


def taubin_step(verts, adj, factor, pinned):
    p = np.asarray(verts, np.float32)
    nv = len(p)
    row_start, row_len, nbr = adj["row_start"].astype(np.int64), adj["row_len"].astype(np.int64), adj["nbr"]
    s = np.zeros((nv, 3), np.float64)
    with np.errstate(all="ignore"):
        for k in range(int(row_len.max()) if nv else 0):
            has = np.nonzero(row_len > k)[0]
            s[has] = s[has] + p[nbr[row_start[has] + k]].astype(np.float64)
        move = row_len >= 1
        if pinned is not None:
            move &= np.asarray(pinned) == 0
        out = p.copy()
        pm = p[move].astype(np.float64)
        m = s[move] / row_len[move].astype(np.float64)[:, None]
        out[move] = (pm + np.float64(factor) * (m - pm)).astype(np.float32)
    return out


def taubin(verts, adj, iterations=10, lam=0.5, mu=-0.53, pin_boundary=True):
    p = np.asarray(verts, np.float32).copy()
    pinned = adj["on_boundary"] if pin_boundary else None
    for _ in range(iterations):
        p = taubin_step(p, adj, lam, pinned)
        p = taubin_step(p, adj, mu, pinned)
    return p


def clean_mesh(verts, faces, rgb=None, min_faces=0, min_fraction=0.0, keep_largest=0, drop_unreferenced=True, smooth_iterations=0, lam=0.5, mu=-0.53,
               pin_boundary=True):
    nv, nf = len(np.asarray(verts).reshape(-1, 3)), len(np.asarray(faces).reshape(-1, 3))
    v, f, c, info = compact(verts, faces, rgb, min_faces, min_fraction, keep_largest, drop_unreferenced)
    adj = adjacency(len(v), f)
    if smooth_iterations:
        v = taubin(v, adj, smooth_iterations, lam, mu, pin_boundary)
    stats = {"vertices_in": nv, "vertices_out": len(v), "faces_in": nf, "faces_out": len(f), "invalid_faces": info["invalid_faces"],
             "components_in": info["components_in"], "components_kept": info["components_kept"],
             "largest_component_faces": info["largest_component_faces"], "unreferenced_removed": nv - len(v), "edges": adj["edges"],
             "boundary_edges": adj["boundary_edges"], "nonmanifold_edges": adj["nonmanifold_edges"],
             "euler_characteristic": adj["referenced_vertices"] - adj["edges"] + len(f), "smooth_iterations": smooth_iterations}
    return v, f, c, stats
