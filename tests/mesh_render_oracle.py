"""The rasteriser's rules (rc_mvsnet_amd/csrc/mesh_render_math.h, contract in csrc/mesh_render.h) restated in numpy with int64 and
float64 only, one face after another: the oracle of tests/mesh_render_cases.py.  Every expression is written in the header's
operation order, so keys, depths, face numbers, colour bytes, shade bytes and counters can be demanded equal in every bit."""
import math

import numpy as np

SUB = 256
GUARD = 65536.0
MAX_SIDE = 16384
SMALL_SIDE = 8
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
STAT_NAMES = ("faces_drawn", "faces_clipped", "faces_degenerate", "faces_culled", "faces_invalid", "faces_large", "pixels_covered")
F64_MAX = np.finfo(np.float64).max
F32_MAX = np.finfo(np.float32).max


class Refused(Exception):
    pass


def camera(c, verts):
    """(nv,3) fp32 -> xc, yc, zc (nv,) fp64, in tsdf_mesh_math.h's order"""
    x, y, z = (verts[:, k].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        xc = ((c[0] * x + c[1] * y) + c[2] * z) + c[9]
        yc = ((c[3] * x + c[4] * y) + c[5] * z) + c[10]
        zc = ((c[6] * x + c[7] * y) + c[8] * z) + c[11]
    return xc, yc, zc


def project(c, near, xc, yc, zc):
    """-> X, Y (int64), usable (bool)"""
    with np.errstate(all="ignore"):
        ok = (zc >= near) & (zc <= F64_MAX)
        u = c[12] * (xc / zc) + c[14]
        v = c[13] * (yc / zc) + c[15]
        ok &= (np.abs(u) <= GUARD) & (np.abs(v) <= GUARD)
        X = np.where(ok, np.floor(np.where(ok, u, 0.0) * float(SUB) + 0.5), 0.0).astype(np.int64)
        Y = np.where(ok, np.floor(np.where(ok, v, 0.0) * float(SUB) + 0.5), 0.0).astype(np.int64)
    return X, Y, ok


def face_valid(a, b, c, nv):
    return 0 <= a < nv and 0 <= b < nv and 0 <= c < nv and a != b and b != c and a != c


def floor_pixel(a):
    return a // SUB                                                # Python's floor division


def ceil_pixel(a):
    return -((-a) // SUB)


def face_setup(P, a, b, c):
    """P: (X, Y, zc) -> area2, the three edges (dx, dy, px, py, min_w) after the negation, iz (3,), |area2|; Python ints"""
    X, Y, zc = P
    pts = [(int(X[i]), int(Y[i])) for i in (a, b, c)]
    (xa, ya), (xb, yb), (xc_, yc_) = pts
    a2 = (xb - xa) * (yc_ - ya) - (xc_ - xa) * (yb - ya)
    sign = -1 if a2 < 0 else 1
    edges = []
    for p, q in ((pts[1], pts[2]), (pts[2], pts[0]), (pts[0], pts[1])):
        dx, dy = sign * (q[0] - p[0]), sign * (q[1] - p[1])
        edges.append((dx, dy, p[0], p[1], 0 if (dy < 0 or (dy == 0 and dx > 0)) else 1))
    iz = [1.0 / float(zc[i]) for i in (a, b, c)]
    return a2, edges, iz, sign * a2


def weights(edges, px, py):
    """px, py: int64 arrays of pixel numbers -> w (3, ...) int64, inside"""
    Px, Py = px.astype(np.int64) * SUB, py.astype(np.int64) * SUB
    w = [np.int64(dx) * (Py - np.int64(qy)) - np.int64(dy) * (Px - np.int64(qx)) for dx, dy, qx, qy, _ in edges]
    inside = (w[0] >= edges[0][4]) & (w[1] >= edges[1][4]) & (w[2] >= edges[2][4])
    return w, inside


def bounding_box(pts, H, W):
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    return max(ceil_pixel(min(xs)), 0), max(ceil_pixel(min(ys)), 0), min(floor_pixel(max(xs)), W - 1), min(floor_pixel(max(ys)), H - 1)


def check_arguments(H, W, n, near, cull):
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE) or n < 1 or not (near > 0 and math.isfinite(near)) or cull not in ("none", "back"):
        raise Refused((H, W, n, near, cull))


def render_view(verts, faces, rgb, c, H, W, near, cull="none", background=(0, 0, 0)):
    """one view -> dict: keys (H,W) uint64, depth fp32, face int32, rgb (H,W,3) uint8, shade uint8, stats (dict of STAT_NAMES)"""
    nv = len(verts)
    xc, yc, zc = camera(c, verts) if nv else (np.zeros(0),) * 3
    X, Y, ok = project(c, near, xc, yc, zc) if nv else (np.zeros(0, np.int64),) * 3
    keys = np.full((H, W), EMPTY, np.uint64)
    stats = dict.fromkeys(STAT_NAMES, 0)
    for f, (a, b, c_) in enumerate(np.asarray(faces).tolist()):
        if not face_valid(a, b, c_, nv):
            stats["faces_invalid"] += 1
            continue
        if not (ok[a] and ok[b] and ok[c_]):
            stats["faces_clipped"] += 1
            continue
        a2, edges, iz, abs_a2 = face_setup((X, Y, zc), a, b, c_)
        if a2 == 0:
            stats["faces_degenerate"] += 1
            continue
        if cull == "back" and a2 > 0:
            stats["faces_culled"] += 1
            continue
        stats["faces_drawn"] += 1
        x0, y0, x1, y1 = bounding_box([(int(X[i]), int(Y[i])) for i in (a, b, c_)], H, W)
        if x0 > x1 or y0 > y1:
            continue
        if not (x1 - x0 < SMALL_SIDE and y1 - y0 < SMALL_SIDE):
            stats["faces_large"] += 1
        py, px = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.int64), np.arange(x0, x1 + 1, dtype=np.int64), indexing="ij")
        w, inside = weights(edges, px, py)
        with np.errstate(all="ignore"):
            s = (w[0].astype(np.float64) * iz[0] + w[1].astype(np.float64) * iz[1]) + w[2].astype(np.float64) * iz[2]
            d = (np.float64(abs_a2) / s).astype(np.float32)
            good = inside & (d > 0) & (d <= F32_MAX)
        k = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
        sub = keys[y0:y1 + 1, x0:x1 + 1]
        sub[good] = np.minimum(sub[good], k[good])
    return resolve_view(verts, faces, rgb, c, H, W, near, keys, background, stats, (xc, yc, zc), (X, Y))


def resolve_view(verts, faces, rgb, c, H, W, near, keys, background, stats, cam_pts, lattice):
    xc, yc, zc = cam_pts
    X, Y = lattice
    depth, face = np.zeros((H, W), np.float32), np.full((H, W), -1, np.int32)
    out_rgb = np.empty((H, W, 3), np.uint8)
    out_rgb[:] = np.asarray(background, np.uint8)
    shade = np.zeros((H, W), np.uint8)
    covered = keys != EMPTY
    stats["pixels_covered"] = int(covered.sum())
    depth[covered] = (keys[covered] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    face[covered] = (keys[covered] & np.uint64(0xFFFFFFFF)).astype(np.int64).astype(np.int32)
    for f in np.unique(face[covered]).tolist():
        a, b, c_ = (int(i) for i in faces[f])
        ys, xs = np.nonzero(face == f)
        A, B, C = ((xc[i], yc[i], zc[i]) for i in (a, b, c_))
        shade[ys, xs] = shade_of(A, B, C)
        if rgb is None:
            out_rgb[ys, xs] = 255
            continue
        _, edges, iz, _ = face_setup((X, Y, zc), a, b, c_)
        w, _ = weights(edges, xs.astype(np.int64), ys.astype(np.int64))
        with np.errstate(all="ignore"):
            q = [w[k].astype(np.float64) * iz[k] for k in range(3)]
            den = (q[0] + q[1]) + q[2]
            for ch in range(3):
                c0, c1, c2 = (float(rgb[i, ch]) for i in (a, b, c_))
                num = (q[0] * c0 + q[1] * c1) + q[2] * c2
                x = np.floor(num / den + 0.5)
                out_rgb[ys, xs, ch] = np.where(x >= 255.0, 255.0, np.where(x >= 0.0, x, 0.0)).astype(np.uint8)
    return {"keys": keys, "depth": depth, "face": face, "rgb": out_rgb, "shade": shade, "stats": stats}


def shade_of(A, B, C):
    with np.errstate(all="ignore"):
        ux, uy, uz = (np.float64(B[k]) - np.float64(A[k]) for k in range(3))
        vx, vy, vz = (np.float64(C[k]) - np.float64(A[k]) for k in range(3))
        nx, ny, nz = uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx
        len2 = (nx * nx + ny * ny) + nz * nz
        if not (len2 > 0.0 and len2 <= F64_MAX):
            return 0
        x = np.floor(255.0 * np.abs(nz) / np.sqrt(len2) + 0.5)
    return int(255.0 if x >= 255.0 else (x if x >= 0.0 else 0.0))


def render(verts, faces, rgb, cams, H, W, near, cull="none", background=(0, 0, 0)):
    """-> dict of stacked arrays over the views, stats a list of dicts"""
    cams = np.asarray(cams, np.float64).reshape(-1, 16)
    check_arguments(H, W, len(cams), near, cull)
    views = [render_view(np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3), rgb, c, H, W, near, cull, background)
             for c in cams]
    out = {k: np.stack([v[k] for v in views]) for k in ("keys", "depth", "face", "rgb", "shade")}
    out["stats"] = [v["stats"] for v in views]
    return out


def compare(rendered, depth, thresholds):
    """-> one dict per view; counts exact, sum_abs by math.fsum (the exact sum correctly rounded)"""
    rows = []
    for r, d in zip(np.asarray(rendered, np.float32), np.asarray(depth, np.float32)):
        with np.errstate(all="ignore"):
            hr, hd = (r > 0) & (r <= F32_MAX), (d > 0) & (d <= F32_MAX)
            both = hr & hd
            diff = np.abs(r[both].astype(np.float64) - d[both].astype(np.float64))
            within = [int((diff <= np.float64(t) * d[both].astype(np.float64)).sum()) for t in thresholds]
        s = math.fsum(diff.tolist())
        n = int(both.sum())
        rows.append({"both": n, "only_mesh": int((hr & ~hd).sum()), "only_map": int((hd & ~hr).sum()), "within": within, "sum_abs": s,
                     "mean_abs": s / n if n else None})
    return rows
