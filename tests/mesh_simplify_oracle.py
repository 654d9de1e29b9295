"""The restatement of csrc/mesh_simplify_math.h and of the contract of csrc/mesh_simplify.h in Python: integers and IEEE fp64 scalars,
one operation a time in the header's order (Python floats are fp64 and never fuse a multiply with an add), fp32 only where the
header rounds (np.float32).  Written from the two headers, not from the kernels: plain loops over vertices, edges and faces.

    begin(verts, faces, rgb) -> state;  round_(state, target_faces, max_error) -> what a round decides, the state advanced;
    finish(state, drop_unreferenced) -> the mesh;  simplify(...) -> (verts, faces, rgb, stats, rounds)"""
import math

import numpy as np

PATH_LOCKED, PATH_QUADRIC, PATH_MIDPOINT, PATH_END_U, PATH_END_V = range(5)
FROM_X, FROM_U, FROM_V = range(3)
EDGE_OK, EDGE_COST, EDGE_LINK, EDGE_FLIP, EDGE_NONE = 0, 1, 2, 3, 255
DET_EPS, FAR = 1e-9, 4.0
NO_KEY = 2 ** 64 - 1
PATH_NAMES = ("locked", "quadric", "midpoint", "end_u", "end_v")


# ---- md:: pieces the header borrows -------------------------------------------------------------------------------------------
def finite_rows(v):
    bits = np.ascontiguousarray(v, np.float32).view(np.uint32).reshape(-1, 3)
    return ((bits & 0x7f800000) != 0x7f800000).all(1)


def ordered32(x):
    """md::ordered of one fp32 value -> int"""
    u = int(np.array([x], np.float32).view(np.uint32)[0])
    return (~u & 0xffffffff) if u & 0x80000000 else (u | 0x80000000)


def bounds(v):
    """the box of the finite vertices by md::ordered keys (-0.0 below +0.0) -> (lo, hi) float32 or (None, None)"""
    v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
    fin = v[finite_rows(v)]
    if not len(fin):
        return None, None
    u = fin.view(np.uint32)
    keys = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    back = lambda k: np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(np.float32)      # noqa: E731
    return back(keys.min(0)), back(keys.max(0))


def frame(lo, hi):
    if lo is None:
        return [0.0, 0.0, 0.0, 1.0]
    c = [(float(lo[a]) + float(hi[a])) * 0.5 for a in range(3)]
    s = float(hi[0]) - float(lo[0])
    for a in (1, 2):
        t = float(hi[a]) - float(lo[a])
        if t > s:
            s = t
    return c + [s if s > 0.0 else 1.0]


def local(p, ctr, side):
    return (float(p) - ctr) / side


def world(ctr, side, x):
    with np.errstate(all="ignore"):
        return np.float32(ctr + side * x)


def colour(s, c):
    return (2 * s + c) // (2 * c)


def face_valid(a, b, c, nv):
    return 0 <= a < nv and 0 <= b < nv and 0 <= c < nv and a != b and b != c and a != c


# ---- ms:: ---------------------------------------------------------------------------------------------------------------------
def cross(q0, q1, q2):
    ux, uy, uz = q1[0] - q0[0], q1[1] - q0[1], q1[2] - q0[2]
    vx, vy, vz = q2[0] - q0[0], q2[1] - q0[1], q2[2] - q0[2]
    return [uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx]


def add_corner(Q, q0, q1, q2):
    nx, ny, nz = cross(q0, q1, q2)
    d = -((nx * q0[0] + ny * q0[1]) + nz * q0[2])
    for j, t in enumerate((nx * nx, nx * ny, nx * nz, ny * ny, ny * nz, nz * nz, nx * d, ny * d, nz * d, d * d)):
        Q[j] = Q[j] + t


def cost(Q, x):
    r0 = (Q[0] * x[0] + Q[1] * x[1]) + Q[2] * x[2]
    r1 = (Q[1] * x[0] + Q[3] * x[1]) + Q[4] * x[2]
    r2 = (Q[2] * x[0] + Q[4] * x[1]) + Q[5] * x[2]
    quad = (x[0] * r0 + x[1] * r1) + x[2] * r2
    lin = (Q[6] * x[0] + Q[7] * x[1]) + Q[8] * x[2]
    v = (quad + 2.0 * lin) + Q[9]
    return 0.0 if v < 0.0 else v


def solve(Q, mid, len2):
    trace = (Q[0] + Q[3]) + Q[5]
    if not math.isfinite(trace) or not trace > 0.0:
        return None
    m00, m01, m02, m11, m12, m22 = Q[0], Q[1], Q[2], Q[3], Q[4], Q[5]
    r0, r1, r2 = -Q[6], -Q[7], -Q[8]
    c00 = m11 * m22 - m12 * m12
    c01 = m01 * m22 - m12 * m02
    c02 = m01 * m12 - m11 * m02
    det = (m00 * c00 - m01 * c01) + m02 * c02
    if not math.isfinite(det) or not det > DET_EPS * ((trace * trace) * trace):
        return None
    s12 = r1 * m22 - m12 * r2
    s21 = r1 * m12 - m11 * r2
    s02 = m01 * r2 - r1 * m02
    x0 = ((r0 * c00 - m01 * s12) + m02 * s21) / det
    x1 = ((m00 * s12 - r0 * c01) + m02 * s02) / det
    x2 = ((m00 * (m11 * r2 - r1 * m12) - m01 * s02) + r0 * c02) / det
    if not (math.isfinite(x0) and math.isfinite(x1) and math.isfinite(x2)):
        return None
    e0, e1, e2 = x0 - mid[0], x1 - mid[1], x2 - mid[2]
    if not ((e0 * e0 + e1 * e1) + e2 * e2) <= FAR * len2:
        return None
    return [x0, x1, x2]


def place(Q, pu, pv, locked_u, locked_v):
    """-> (path, from, x or None)"""
    if locked_u:
        return PATH_LOCKED, FROM_U, None
    if locked_v:
        return PATH_LOCKED, FROM_V, None
    mid = [(pu[a] + pv[a]) * 0.5 for a in range(3)]
    e0, e1, e2 = pv[0] - pu[0], pv[1] - pu[1], pv[2] - pu[2]
    len2 = (e0 * e0 + e1 * e1) + e2 * e2
    x = solve(Q, mid, len2)
    if x is not None:
        return PATH_QUADRIC, FROM_X, x
    cm, cu, cv = cost(Q, mid), cost(Q, pu), cost(Q, pv)
    path, best = PATH_MIDPOINT, cm
    if cu < best:
        path, best = PATH_END_U, cu
    if cv < best:
        path, best = PATH_END_V, cv
    if path == PATH_MIDPOINT:
        return path, FROM_X, mid
    return path, (FROM_U if path == PATH_END_U else FROM_V), None


def keeps_side(q, k, t):
    n = cross(q[0], q[1], q[2])
    moved = [t if j == k else q[j] for j in range(3)]
    m = cross(moved[0], moved[1], moved[2])
    return ((m[0] * n[0] + m[1] * n[1]) + m[2] * n[2]) > 0.0


def link_ok(shared, lu, lv):
    return shared == 2 and lu + lv - 4 >= 3


def key(c, entry):
    with np.errstate(all="ignore"):
        return (ordered32(np.float32(c)) << 32) | entry


def budget(live, target):
    return (live - target + 1) // 2 if live > target else 0


# ---- the state ------------------------------------------------------------------------------------------------------------------
def corners_of(faces, nv):
    """per vertex its corners 3 f + k in the valid faces, ascending"""
    at = [[] for _ in range(nv)]
    for f, (a, b, c) in enumerate(faces.tolist()):
        if face_valid(a, b, c, nv):
            at[a].append(3 * f)
            at[b].append(3 * f + 1)
            at[c].append(3 * f + 2)
    return at


def begin(verts, faces, rgb=None):
    v = np.array(verts, np.float32).reshape(-1, 3)
    f = np.array(faces, np.int32).reshape(-1, 3)
    nv = len(v)
    fr = frame(*bounds(v))
    fin = finite_rows(v)
    P = _locals(v, fr)
    quad = [[0.0] * 10 for _ in range(nv)]
    fl = f.tolist()
    bad = valid = 0
    for a, b, c in fl:
        if face_valid(a, b, c, nv):
            valid += 1
            bad += not (fin[a] and fin[b] and fin[c])
    for w, es in enumerate(corners_of(f, nv)):
        for e in es:
            a, b, c = fl[e // 3]
            if fin[a] and fin[b] and fin[c]:
                add_corner(quad[w], P[a], P[b], P[c])
    return {"nv": nv, "verts": v, "faces": f, "frame": fr, "quad": quad, "members": [1] * nv,
            "csum": None if rgb is None else [[int(x) for x in row] for row in np.asarray(rgb).reshape(-1, 3)], "live": valid,
            "nonfinite_faces": int(bad), "nonfinite_vertices": int((~fin).sum())}


def _locals(v, fr):
    with np.errstate(all="ignore"):
        return ((v.astype(np.float64) - np.array(fr[:3])) / fr[3]).tolist()


def adjacency(faces, nv):
    """mesh_clean.h's CSR 1-ring -> (row_start, row_len, nbr, mult) as lists"""
    count = [0] * nv
    ring = [dict() for _ in range(nv)]
    for a, b, c in faces.tolist():
        if face_valid(a, b, c, nv):
            for p, q in ((a, b), (a, c), (b, a), (b, c), (c, a), (c, b)):
                count[p] += 1
                ring[p][q] = ring[p].get(q, 0) + 1
    row_start = [0]
    for n in count:
        row_start.append(row_start[-1] + n)
    entries = 6 * len(faces)
    nbr, mult, row_len = [-1] * entries, [0] * entries, []
    for w in range(nv):
        ks = sorted(ring[w])
        row_len.append(len(ks))
        for j, x in enumerate(ks):
            nbr[row_start[w] + j] = x
            mult[row_start[w] + j] = ring[w][x]
    return row_start, row_len, nbr, mult


def edge_target(S, P, u, v, locked_u, locked_v):
    """-> (path, the target's fp32 values, the target in the frame, the summed quadric, the cost)"""
    fr = S["frame"]
    Q = [a + b for a, b in zip(S["quad"][u], S["quad"][v])]
    path, frm, x = place(Q, P[u], P[v], locked_u, locked_v)
    if frm == FROM_X:
        t = [world(fr[a], fr[3], x[a]) for a in range(3)]
        xt = [local(t[a], fr[a], fr[3]) for a in range(3)]
    else:
        src = u if frm == FROM_U else v
        t, xt = S["verts"][src].copy(), P[src]
    return path, t, xt, Q, cost(Q, xt)


def round_(S, target_faces, max_error=math.inf):
    """One round: the dict of what it decides (numpy arrays named as mesh_simplify.round's) and S advanced in place"""
    nv, faces = S["nv"], S["faces"]
    fl = faces.tolist()
    entries = 6 * len(fl)
    row_start, row_len, nbr, mult = adjacency(faces, nv)
    at = corners_of(faces, nv)
    P = _locals(S["verts"], S["frame"])
    fin = finite_rows(S["verts"])
    rings = [nbr[row_start[w]:row_start[w] + row_len[w]] for w in range(nv)]
    locked = [int((not fin[w]) or any(m != 2 for m in mult[row_start[w]:row_start[w] + row_len[w]])) for w in range(nv)]
    edge, keys = [EDGE_NONE] * entries, [NO_KEY] * entries
    counts = {"candidates": 0, "reject_cost": 0, "reject_link": 0, "reject_flip": 0, "paths": [0] * 5}
    found = {}

    def sides(w, other, xt):
        for e in at[w]:
            a, b, c = fl[e // 3]
            if other in (a, b, c):
                continue
            if not keeps_side((P[a], P[b], P[c]), e % 3, xt):
                return False
        return True

    for u in range(nv):
        for j, v in enumerate(rings[u]):
            i = row_start[u] + j
            if not (u < v and mult[i] == 2 and not (locked[u] and locked[v])):
                continue
            path, t, xt, Q, c = edge_target(S, P, u, v, locked[u], locked[v])
            counts["candidates"] += 1
            counts["paths"][path] += 1
            if not c <= max_error:
                edge[i] = EDGE_COST
            elif not link_ok(len(set(rings[u]) & set(rings[v])), row_len[u], row_len[v]):
                edge[i] = EDGE_LINK
            elif not (sides(u, v, xt) and sides(v, u, xt)):
                edge[i] = EDGE_FLIP
            else:
                edge[i] = EDGE_OK
                keys[i] = keys[row_start[v] + rings[v].index(u)] = key(c, i)
                found[i] = (u, v, t, Q, c)
            if edge[i] != EDGE_OK:
                counts[("reject_cost", "reject_link", "reject_flip")[edge[i] - 1]] += 1
    best1 = [min(keys[row_start[w]:row_start[w] + row_len[w]], default=NO_KEY) for w in range(nv)]
    best2 = [min([best1[w]] + [best1[x] for x in rings[w]]) for w in range(nv)]
    selected = [0] * entries
    for i, (u, v, *_) in found.items():
        selected[i] = int(keys[i] == best2[u] == best2[v])
    allowed, taken = budget(S["live"], target_faces), 0
    applied, remap, worst = [0] * entries, list(range(nv)), 0
    for i in range(entries):
        if selected[i]:
            if taken < allowed:
                applied[i] = 1
                u, v, t, Q, c = found[i]
                s, g = (v, u) if locked[v] else (u, v)
                S["verts"][s] = t
                S["quad"][s] = Q
                S["members"][s] = S["members"][u] + S["members"][v]
                S["members"][g] = 0
                if S["csum"] is not None:
                    S["csum"][s] = [a + b for a, b in zip(S["csum"][u], S["csum"][v])]
                remap[g] = s
                with np.errstate(all="ignore"):
                    worst = max(worst, ordered32(np.float32(c)))
            taken += 1
    new = faces.copy()
    ok = (new >= 0) & (new < nv)
    new[ok] = np.array(remap, np.int32)[new[ok]] if nv else new[ok]
    live_before = S["live"]
    S["faces"] = new
    S["live"] = sum(face_valid(a, b, c, nv) for a, b, c in new.tolist())
    u64 = lambda x: np.array(x, np.uint64)                       # noqa: E731
    return {"row_start": np.array(row_start, np.int32), "row_len": np.array(row_len, np.int32).reshape(-1), "nbr": np.array(nbr, np.int32).reshape(-1),
            "mult": np.array(mult, np.int32).reshape(-1), "locked": np.array(locked, np.uint8).reshape(-1), "edge": np.array(edge, np.uint8).reshape(-1),
            "key": u64(keys).reshape(-1), "best1": u64(best1).reshape(-1), "best2": u64(best2).reshape(-1), "selected": np.array(selected, np.uint8).reshape(-1),
            "applied": np.array(applied, np.uint8).reshape(-1), "remap": np.array(remap, np.int32).reshape(-1), "locked_vertices": sum(locked),
            "candidates": counts["candidates"], "reject_cost": counts["reject_cost"], "reject_link": counts["reject_link"], "reject_flip": counts["reject_flip"],
            "paths": counts["paths"], "selected_edges": sum(selected), "applied_edges": sum(applied), "max_cost": unordered_cost(worst), "live": S["live"],
            "live_before": live_before}


def unordered_cost(bits):
    if bits == 0:
        return 0.0
    raw = (bits & 0x7fffffff) if bits & 0x80000000 else (~bits & 0xffffffff)
    return float(np.array([raw], np.uint32).view(np.float32)[0])


def snapshot(S):
    """the state as numpy arrays: verts, faces, quad, members, csum"""
    return {"verts": S["verts"].copy(), "faces": S["faces"].copy(), "quad": np.array(S["quad"], np.float64).reshape(-1, 10),
            "members": np.array(S["members"], np.int32).reshape(-1), "csum": None if S["csum"] is None else np.array(S["csum"], np.int64).reshape(-1, 3)}


def finish(S, drop_unreferenced=True):
    nv, f = S["nv"], S["faces"]
    keep_f = np.array([face_valid(a, b, c, nv) for a, b, c in f.tolist()], bool).reshape(-1)
    if drop_unreferenced:
        keep_v = np.zeros(nv, bool)
        keep_v[f[keep_f].reshape(-1)] = True
    else:
        keep_v = np.array(S["members"], np.int64).reshape(-1) > 0
    rank = np.cumsum(keep_v) - 1
    out_f = rank[f[keep_f]].astype(np.int32).reshape(-1, 3)
    out_v = S["verts"][keep_v]
    out_c = None
    if S["csum"] is not None:
        out_c = np.array([[colour(s, S["members"][w]) for s in S["csum"][w]] for w in np.nonzero(keep_v)[0]], np.uint8).reshape(-1, 3)
    return out_v, out_f, out_c


def simplify(verts, faces, rgb=None, *, target_faces=None, ratio=None, max_error=math.inf, max_rounds=256, drop_unreferenced=True, keep_rounds=True):
    """-> (verts, faces, rgb, stats, rounds): rounds, a list of (what round_ returned, the snapshot after it)"""
    assert (target_faces is None) != (ratio is None)
    S = begin(verts, faces, rgb)
    valid = S["live"]
    target = int(target_faces) if target_faces is not None else int(math.floor(float(ratio) * valid))
    stats = {"vertices_in": S["nv"], "faces_in": len(S["faces"]), "valid_faces_in": valid, "target_faces": target, "max_error": float(max_error),
             "max_rounds": max_rounds, "nonfinite_faces": S["nonfinite_faces"], "nonfinite_vertices": S["nonfinite_vertices"]}
    rounds, collapses, locked, rejected, paths, worst, stop = [], [], 0, [0, 0, 0], [0] * 5, 0.0, None
    first = snapshot(S)
    while stop is None:
        if S["live"] <= target:
            stop = "target"
        elif len(collapses) >= max_rounds:
            stop = "max_rounds"
        else:
            r = round_(S, target, float(max_error))
            if keep_rounds:
                rounds.append((r, snapshot(S)))
            if not collapses:
                locked = r["locked_vertices"]
            collapses.append(r["applied_edges"])
            rejected = [a + r[k] for a, k in zip(rejected, ("reject_cost", "reject_link", "reject_flip"))]
            paths = [a + b for a, b in zip(paths, r["paths"])]
            worst = max(worst, r["max_cost"])
            if r["selected_edges"] == 0:
                stop = "nothing_selected"
    v, f, c = finish(S, drop_unreferenced)
    stats.update({"vertices_out": len(v), "faces_out": len(f), "rounds": len(collapses), "collapses": collapses, "locked_vertices": locked,
                  "rejected_cost": rejected[0], "rejected_link": rejected[1], "rejected_flip": rejected[2],
                  **{"placed_" + name: paths[i] for i, name in enumerate(PATH_NAMES)}, "max_cost": worst, "stop": stop})
    return v, f, c, stats, {"first": first, "rounds": rounds}
