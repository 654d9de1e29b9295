"""MeshSupSamp (matlab_eval/MeshSupSamp_web/MeshSupSamp/MeshSupSamp.cpp: SubTri and mexFunction) restated twice, the yardstick
of rc_mvsnet_amd.dtu_eval.sample_mesh: ``literal`` with Python floats and the loops as written, ``vectorised`` in numpy fp64.
Both take fp32 vertices (promoted to fp64) and 0-based faces and return fp64 points: the vertices, then the samples of every
face in order.  The kernels round each point to fp32 once, so ``points.astype(np.float32)`` is what they must give, bit for bit.
TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np


def _div(a, b):
    """IEEE a / b (Python raises on a zero divisor)"""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _floor(x):
    return x if math.isnan(x) or math.isinf(x) else float(math.floor(x))


def _norm(v):
    return math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def sub_tri(Q0, Q1, Q2, thresh):
    """SubTri: the samples of one triangle, in the loops' order"""
    v1 = [Q1[k] - Q0[k] for k in range(3)]
    l1 = _norm(v1)
    v2 = [Q2[k] - Q0[k] for k in range(3)]
    l2 = _norm(v2)
    cross = [v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]]
    area2 = _norm(cross)
    ratio = _div(l1 * l2, area2)
    thr = thresh * math.sqrt(ratio)
    n1 = _floor(_div(l1, thr))
    n2 = _floor(_div(l2, thr))
    out = []
    c1 = 0.0
    while c1 <= n1:
        c2 = 0.0
        while c2 <= n2:
            k1 = _div(c1 + 0.5, n1)
            k2 = _div(c2 + 0.5, n2)
            if k1 + k2 < 1:
                out.append([(k1 * v1[k] + k2 * v2[k]) + Q0[k] for k in range(3)])
            c2 += 1
        c1 += 1
    return out


def literal(verts, faces, dst):
    """mexFunction: -> (nv + samples, 3) fp64"""
    qs = [[float(c) for c in v] for v in np.asarray(verts, dtype=np.float32)]
    out = [list(q) for q in qs]
    for f in np.asarray(faces, dtype=np.int64).reshape(-1, 3):
        out += sub_tri(qs[f[0]], qs[f[1]], qs[f[2]], float(dst))
    return np.array(out, dtype=np.float64).reshape(-1, 3)


def face_params(verts, faces, dst):
    """per face (q0, v1, v2, n1, n2), vectorised in SubTri's operation order"""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    q0 = v[f[:, 0]]
    v1 = v[f[:, 1]] - q0
    v2 = v[f[:, 2]] - q0

    def norm(a):
        return np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])

    cross = np.stack([v1[:, 1] * v2[:, 2] - v1[:, 2] * v2[:, 1], v1[:, 2] * v2[:, 0] - v1[:, 0] * v2[:, 2],
                      v1[:, 0] * v2[:, 1] - v1[:, 1] * v2[:, 0]], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        l1, l2 = norm(v1), norm(v2)
        thr = float(dst) * np.sqrt((l1 * l2) / norm(cross))
        n1, n2 = np.floor(l1 / thr), np.floor(l2 / thr)
    return q0, v1, v2, n1, n2


def vectorised(verts, faces, dst, chunk=1 << 22):
    """the same points: every (face, c1, c2) candidate of the loops expanded, c1-major, then the keep test; chunks of faces
    bound the candidates held at once (about ``chunk``)"""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    q0, v1, v2, n1, n2 = face_params(verts, faces, dst)
    e1 = np.where(n1 >= 0, n1 + 1, 0).astype(np.int64)             # loop extents (NaN: none)
    e2 = np.where(n2 >= 0, n2 + 1, 0).astype(np.int64)
    cand = e1 * e2
    out = [v]
    ends = np.cumsum(cand)
    cuts = np.unique(np.concatenate([[0], np.searchsorted(ends, np.arange(chunk, int(ends[-1]) if len(ends) else 0, chunk), side="right"), [len(cand)]]))
    for start, stop in zip(cuts[:-1], cuts[1:]):
        cnt = cand[start:stop]
        tri = np.repeat(np.arange(start, stop), cnt)
        local = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        c1 = (local // e2[tri]).astype(np.float64)
        c2 = (local % e2[tri]).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            k1 = (c1 + 0.5) / n1[tri]
            k2 = (c2 + 0.5) / n2[tri]
            keep = k1 + k2 < 1
        k1, k2, tri = k1[keep, None], k2[keep, None], tri[keep]
        out.append((k1 * v1[tri] + k2 * v2[tri]) + q0[tri])
    return np.concatenate(out).reshape(-1, 3)

