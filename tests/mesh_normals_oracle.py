"""The rules of the mesh normals (rc_mvsnet_amd/csrc/mesh_normals_math.h, contract in csrc/mesh_normals.h) restated in numpy with
int64 and float64 scalars only, one face, one corner, one pixel after another: the oracle of tests/mesh_normals_cases.py.  Every
expression is written in the header's operation order -- no np.cross, no reduction with a free order, the sums over a vertex's
corners explicit and sequential in ascending corner number -- so face normals, vertex normals, counters, normal-map floats, smooth
bytes and colour bytes can be demanded equal in every bit."""
import math

import numpy as np

import mesh_render_oracle as RO

STAT_NAMES = ("faces_invalid", "faces_nonfinite", "faces_degenerate", "corners_skipped", "vertices_with_normal", "vertices_unreferenced",
              "vertices_cancelled")
F64_MAX = np.finfo(np.float64).max
D = np.float64


def finite9(pts):
    return all(math.isfinite(float(x)) for p in pts for x in p)


def cross_at(p, q, r):
    """(q - p) x (r - p) of three fp32 points -> (n (3 float64), l1, l2)"""
    with np.errstate(all="ignore"):
        ux, uy, uz = (D(q[k]) - D(p[k]) for k in range(3))
        vx, vy, vz = (D(r[k]) - D(p[k]) for k in range(3))
        n = (uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx)
        l1 = (ux * ux + uy * uy) + uz * uz
        l2 = (vx * vx + vy * vy) + vz * vz
    return n, l1, l2


def length2(v):
    with np.errstate(all="ignore"):
        return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]


def unit(v):
    """-> ((3,) float32, usable)"""
    len2 = length2(v)
    if not (len2 > 0.0 and len2 <= F64_MAX):
        return np.zeros(3, np.float32), False
    with np.errstate(all="ignore"):
        ln = np.sqrt(len2)
        return np.array([np.float32(v[0] / ln), np.float32(v[1] / ln), np.float32(v[2] / ln)], np.float32), True


def classify(verts, faces):
    """per face: 'invalid', 'nonfinite' or 'ok', and F for the ok ones"""
    nv = len(verts)
    out = []
    for a, b, c in np.asarray(faces).reshape(-1, 3).tolist():
        if not RO.face_valid(a, b, c, nv):
            out.append(("invalid", None))
            continue
        pts = (verts[a], verts[b], verts[c])
        if not finite9(pts):
            out.append(("nonfinite", None))
            continue
        out.append(("ok", cross_at(*pts)[0]))
    return out


def face_normals(verts, faces):
    verts, faces = np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    out = np.zeros((len(faces), 3), np.float32)
    for f, (kind, F) in enumerate(classify(verts, faces)):
        if kind == "ok":
            out[f] = unit(F)[0]
    return out


def vertex_normals(verts, faces, weight):
    """-> (normals (nv,3) float32, stats dict of STAT_NAMES plus the weight)"""
    assert weight in ("area", "sphere")
    verts, faces = np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    nv = len(verts)
    stats = dict.fromkeys(STAT_NAMES, 0)
    sums = [[D(0.0), D(0.0), D(0.0)] for _ in range(nv)]
    used = [0] * nv
    for f, (kind, F) in enumerate(classify(verts, faces)):            # ascending face, then corner 0, 1, 2: ascending 3 face + corner per vertex
        if kind != "ok":
            stats["faces_" + kind] += 1
            continue
        if F[0] == 0.0 and F[1] == 0.0 and F[2] == 0.0:
            stats["faces_degenerate"] += 1
        t = [int(i) for i in faces[f]]
        for k in range(3):
            if weight == "area":
                c = F
            else:
                C, l1, l2 = cross_at(verts[t[k]], verts[t[(k + 1) % 3]], verts[t[(k + 2) % 3]])
                with np.errstate(all="ignore"):
                    d = l1 * l2
                    if not d > 0.0:
                        stats["corners_skipped"] += 1
                        continue
                    c = (C[0] / d, C[1] / d, C[2] / d)
            s = sums[t[k]]
            with np.errstate(all="ignore"):
                s[0], s[1], s[2] = s[0] + c[0], s[1] + c[1], s[2] + c[2]
            used[t[k]] += 1
    normals = np.zeros((nv, 3), np.float32)
    for v in range(nv):
        if not used[v]:
            stats["vertices_unreferenced"] += 1
            continue
        normals[v], ok = unit(sums[v])
        stats["vertices_with_normal" if ok else "vertices_cancelled"] += 1
    return normals, dict({"weight": weight}, **stats)


def byte_of(x):
    return int(255.0 if x >= 255.0 else (x if x >= 0.0 else 0.0))


def shade(verts, faces, normals, cams, face_image, near, background=(0, 0, 0)):
    """-> dict normal (V,H,W,3) float32, smooth (V,H,W) uint8, normal_rgb (V,H,W,3) uint8"""
    verts, faces = np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    normals = np.asarray(normals, np.float32).reshape(-1, 3)
    cams = np.asarray(cams, np.float64).reshape(-1, 16)
    face_image = np.asarray(face_image, np.int32)
    V, H, W = face_image.shape
    nv, nf = len(verts), len(faces)
    out = {"normal": np.zeros((V, H, W, 3), np.float32), "smooth": np.zeros((V, H, W), np.uint8), "normal_rgb": np.empty((V, H, W, 3), np.uint8)}
    out["normal_rgb"][:] = np.asarray(background, np.uint8)
    for v in range(V):
        c = cams[v]
        xc, yc, zc = RO.camera(c, verts) if nv else (np.zeros(0),) * 3
        X, Y, ok = RO.project(c, near, xc, yc, zc) if nv else (np.zeros(0, np.int64),) * 3
        for f in np.unique(face_image[v]).tolist():
            if not 0 <= f < nf:
                continue
            a, b, c_ = (int(i) for i in faces[f])
            if not RO.face_valid(a, b, c_, nv) or not (ok[a] and ok[b] and ok[c_]):
                continue
            a2, edges, iz, _ = RO.face_setup((X, Y, zc), a, b, c_)
            if a2 == 0:
                continue
            ys, xs = np.nonzero(face_image[v] == f)
            w, _ = RO.weights(edges, xs.astype(np.int64), ys.astype(np.int64))
            na, nb, nc = (normals[i].astype(np.float64) for i in (a, b, c_))
            with np.errstate(all="ignore"):
                q = [w[k].astype(np.float64) * iz[k] for k in range(3)]
                m = [(q[0] * na[k] + q[1] * nb[k]) + q[2] * nc[k] for k in range(3)]
                g = [(c[3 * r] * m[0] + c[3 * r + 1] * m[1]) + c[3 * r + 2] * m[2] for r in range(3)]
                len2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
                good = (len2 > 0.0) & (len2 <= F64_MAX)
                ln = np.sqrt(np.where(good, len2, 1.0))
                e = [g[k] / ln for k in range(3)]
                smooth = np.floor(255.0 * np.abs(g[2]) / ln + 0.5)
                col = [np.floor(127.5 * (e[0] + 1.0) + 0.5), np.floor(127.5 * (-e[1] + 1.0) + 0.5), np.floor(127.5 * (-e[2] + 1.0) + 0.5)]
            for i in range(len(xs)):
                y, x = int(ys[i]), int(xs[i])
                if not good[i]:
                    out["normal_rgb"][v, y, x] = 128
                    continue
                out["normal"][v, y, x] = [np.float32(e[k][i]) for k in range(3)]
                out["smooth"][v, y, x] = byte_of(smooth[i])
                out["normal_rgb"][v, y, x] = [byte_of(col[k][i]) for k in range(3)]
    return out
