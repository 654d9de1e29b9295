"""The rules of the mesh texturing (rc_mvsnet_amd/csrc/mesh_texture_math.h, contract in csrc/mesh_texture.h) restated in numpy with
Python integers, int64 and float64 only: the oracle of tests/mesh_texture_cases.py.  It is written from the rule, not from the
kernels: the vote counts with a bincount, the atlas is filled face by face (each face paints the texels of its half cell) where the
kernel asks every texel for its face, Morton indices are decoded bit by bit.  Every floating-point expression is written in the
header's operation order, so every best, class, sorted index, table entry, texel coordinate, owner, atlas byte, counter and
textured pixel can be demanded equal in every bit."""
import numpy as np

import mesh_render_oracle as RO

MIN_CLASS, MAX_CLASS, MAX_SHIFT = 2, 10, 8
STAT_NAMES = ("faces_seen", "faces_unseen", "faces_invalid", "faces_capped", "texels_image", "texels_vertex", "texels_fallback")
F64_MAX = np.finfo(np.float64).max
D = np.float64


class Refused(Exception):
    pass


def _mesh(verts, faces):
    return np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)


def lattice(verts, cam, near):
    """-> X, Y (int64), usable, zc of every vertex in one view"""
    if not len(verts):
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, bool), np.zeros(0)
    xc, yc, zc = RO.camera(cam, verts)
    X, Y, ok = RO.project(cam, near, xc, yc, zc)
    return X, Y, ok, zc


def eligible(P, tri, H, W):
    X, Y, ok, _ = P
    return all(bool(ok[i]) and 0 <= int(X[i]) <= 256 * (W - 1) and 0 <= int(Y[i]) <= 256 * (H - 1) for i in tri)


# ---- 1. one view per face ----------------------------------------------------------------------------------------------------------
def vote(verts, faces, face_images, cams, near, first_view=0, best=None):
    """face_images (n,H,W) int32 of the views first_view .. -> best, a list of Python ints (count << 32 | 0xFFFFFFFF - view; 0 unseen)"""
    verts, faces = _mesh(verts, faces)
    cams = np.asarray(cams, np.float64).reshape(-1, 16)
    face_images = np.asarray(face_images, np.int32)
    n, H, W = face_images.shape
    nv, nf = len(verts), len(faces)
    best = [0] * nf if best is None else list(best)
    for v in range(n):
        img = face_images[v].ravel().astype(np.int64)
        count = np.bincount(img[(img >= 0) & (img < nf)], minlength=nf) if nf else np.zeros(0, np.int64)
        P = lattice(verts, cams[v], near)
        for f in np.nonzero(count)[0].tolist():
            tri = [int(i) for i in faces[f]]
            if RO.face_valid(*tri, nv) and eligible(P, tri, H, W):
                best[f] = max(best[f], (int(count[f]) << 32) | (0xFFFFFFFF - (first_view + v)))
    return best


def chosen(verts, faces, best, cams, H, W, near):
    """per face: -2 invalid, -1 unseen, else the view whose key it carries, below V and eligible -> (list, the views' lattices)"""
    verts, faces = _mesh(verts, faces)
    cams = np.asarray(cams, np.float64).reshape(-1, 16)
    V, nv = len(cams), len(verts)
    Ps = [lattice(verts, c, near) for c in cams]
    out = []
    for f, tri in enumerate(faces.tolist()):
        if not RO.face_valid(*tri, nv):
            out.append(-2)
            continue
        view = 0xFFFFFFFF - (int(best[f]) & 0xFFFFFFFF)
        out.append(view if int(best[f]) != 0 and view < V and eligible(Ps[view], tri, H, W) else -1)
    return out, Ps


# ---- 2. a size class per face ------------------------------------------------------------------------------------------------------
def size_class(e2, shift):
    """-> (k, capped)"""
    for k in range(MIN_CLASS, MAX_CLASS + 1):
        if (((1 << k) - 3) << (8 + shift)) ** 2 >= e2:
            return k, False
    return MAX_CLASS, True


def classes(faces, views, Ps, shift):
    """-> (klass list, capped list)"""
    klass, capped = [], []
    for f, tri in enumerate(np.asarray(faces).reshape(-1, 3).tolist()):
        if views[f] == -2:
            k, c = 0, False
        elif views[f] == -1:
            k, c = MIN_CLASS, False
        else:
            X, Y = Ps[views[f]][0], Ps[views[f]][1]
            pts = [(int(X[i]), int(Y[i])) for i in tri]
            e2 = max((pts[q][0] - pts[p][0]) ** 2 + (pts[q][1] - pts[p][1]) ** 2 for p, q in ((0, 1), (1, 2), (2, 0)))
            k, c = size_class(e2, shift)
        klass.append(k)
        capped.append(c)
    return klass, capped


# ---- 3. the atlas ------------------------------------------------------------------------------------------------------------------
def morton_xy(m):
    x = y = 0
    for b in range(32):
        x |= ((m >> (2 * b)) & 1) << b
        y |= ((m >> (2 * b + 1)) & 1) << b
    return x, y


def layout(klass):
    """-> order (the face numbers sorted by descending class, stable, invalid last), table (dict), texel (nf,3,2) int32"""
    nf = len(klass)
    order = sorted(range(nf), key=lambda f: (klass[f] == 0, -klass[f]))
    table = {"classes": {}}
    start = base = 0
    for k in range(MAX_CLASS, MIN_CLASS - 1, -1):
        n = sum(1 for c in klass if c == k)
        cells = (n + 1) // 2
        table["classes"][k] = {"start": start, "faces": n, "cells": cells, "base": base}
        start += n
        base += cells * 4 ** k
    m = 0
    while 4 ** m < base:
        m += 1
    S = 2 ** m
    table.update(total=base, m=m, S=S, Sy=S // 2 if S >= 2 and 2 * base <= S * S else S)
    texel = np.zeros((nf, 3, 2), np.int32)
    for k, row in table["classes"].items():
        s, L = 1 << k, (1 << k) - 3
        for r in range(row["faces"]):
            f = order[row["start"] + r]
            ox, oy = morton_xy(row["base"] + (r >> 1) * 4 ** k)
            if r & 1 == 0:
                texel[f] = [(ox, oy), (ox + L, oy), (ox, oy + L)]
            else:
                texel[f] = [(ox + s - 1, oy + s - 1), (ox + s - 1 - L, oy + s - 1), (ox + s - 1, oy + s - 1 - L)]
    return order, table, texel


# ---- 4. texel fill -----------------------------------------------------------------------------------------------------------------
def bilinear(img, u, v):
    """img (H,W,3) uint8, u in [0, W-1], v in [0, H-1] (float64 arrays) -> (n,3) uint8"""
    H, W = img.shape[:2]
    x0 = np.clip(np.floor(u).astype(np.int64), 0, max(W - 2, 0))
    y0 = np.clip(np.floor(v).astype(np.int64), 0, max(H - 2, 0))
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    fx, fy = u - x0.astype(D), v - y0.astype(D)
    out = np.empty((len(u), 3), np.uint8)
    for ch in range(3):
        p = img[..., ch].astype(D)
        top = (1.0 - fx) * p[y0, x0] + fx * p[y0, x1]
        bottom = (1.0 - fx) * p[y1, x0] + fx * p[y1, x1]
        out[:, ch] = byte_of(np.floor(((1.0 - fy) * top + fy * bottom) + 0.5))
    return out


def byte_of(x):
    with np.errstate(all="ignore"):
        return np.where(x >= 255.0, 255.0, np.where(x >= 0.0, x, 0.0)).astype(np.uint8)


def clamp_to(x, hi):
    return np.where(x < 0.0, 0.0, np.where(x > hi, hi, x))


def fill(verts, faces, rgb, images, cams, near, views, order, table, texel, background=(0, 0, 0)):
    """-> atlas (Sy,S,3) uint8, owner (Sy,S) int32, the three texel counters"""
    verts, faces = _mesh(verts, faces)
    cams = np.asarray(cams, np.float64).reshape(-1, 16)
    images = np.asarray(images, np.uint8)
    H, W = images.shape[1:3]
    S, Sy = table["S"], table["Sy"]
    atlas = np.empty((Sy, S, 3), np.uint8)
    atlas[:] = np.asarray(background, np.uint8)
    owner = np.full((Sy, S), -1, np.int32)
    counts = {"texels_image": 0, "texels_vertex": 0, "texels_fallback": 0}
    for k, row in table["classes"].items():
        s, L = 1 << k, (1 << k) - 3
        jj, ii = (g.ravel() for g in np.meshgrid(np.arange(s), np.arange(s), indexing="ij"))
        lower = ii + jj <= s - 2
        for r in range(row["faces"]):
            f = order[row["start"] + r]
            ox, oy = morton_xy(row["base"] + (r >> 1) * 4 ** k)
            mine = lower if r & 1 == 0 else ~lower
            i, j = ii[mine], jj[mine]
            ip, jp = (i, j) if r & 1 == 0 else (s - 1 - i, s - 1 - j)
            assert (owner[oy + j, ox + i] == -1).all()
            owner[oy + j, ox + i] = f
            with np.errstate(all="ignore"):
                wb, wc = ip.astype(D) / D(L), jp.astype(D) / D(L)
                wa = (1.0 - wb) - wc
                a, b, c = (int(q) for q in faces[f])
                if rgb is None:
                    vcol = np.full((len(i), 3), 255, np.uint8)
                else:
                    vcol = np.stack([byte_of(np.floor(((wa * D(rgb[a, ch]) + wb * D(rgb[b, ch])) + wc * D(rgb[c, ch])) + 0.5)) for ch in range(3)], 1)
                if views[f] < 0:
                    atlas[oy + j, ox + i] = vcol
                    counts["texels_vertex"] += len(i)
                    continue
                cam = cams[views[f]]
                A, B, C = (verts[q].astype(D) for q in (a, b, c))
                p = [(wa * A[q] + wb * B[q]) + wc * C[q] for q in range(3)]
                xc = ((cam[0] * p[0] + cam[1] * p[1]) + cam[2] * p[2]) + cam[9]
                yc = ((cam[3] * p[0] + cam[4] * p[1]) + cam[5] * p[2]) + cam[10]
                zc = ((cam[6] * p[0] + cam[7] * p[1]) + cam[8] * p[2]) + cam[11]
                u = cam[12] * (xc / zc) + cam[14]
                v = cam[13] * (yc / zc) + cam[15]
                good = (zc >= near) & (np.abs(u) <= F64_MAX) & (np.abs(v) <= F64_MAX)
                u, v = clamp_to(np.where(good, u, 0.0), D(W - 1)), clamp_to(np.where(good, v, 0.0), D(H - 1))
                col = bilinear(images[views[f]], u, v)
            atlas[oy + j, ox + i] = np.where(good[:, None], col, vcol)
            counts["texels_image"] += int(good.sum())
            counts["texels_fallback"] += int((~good).sum())
    return atlas, owner, counts


# ---- 5. textured views -------------------------------------------------------------------------------------------------------------
def shade(verts, faces, cams, face_image, texel, atlas, near, background=(0, 0, 0)):
    """-> tex_rgb (V,H,W,3) uint8"""
    verts, faces = _mesh(verts, faces)
    cams = np.asarray(cams, np.float64).reshape(-1, 16)
    face_image = np.asarray(face_image, np.int32)
    V, H, W = face_image.shape
    nv, nf = len(verts), len(faces)
    Sy, S = atlas.shape[:2]
    out = np.empty((V, H, W, 3), np.uint8)
    out[:] = np.asarray(background, np.uint8)
    for v in range(V):
        X, Y, ok, zc = lattice(verts, cams[v], near)
        for f in np.unique(face_image[v]).tolist():
            if not 0 <= f < nf:
                continue
            a, b, c = (int(i) for i in faces[f])
            if not RO.face_valid(a, b, c, nv) or not (ok[a] and ok[b] and ok[c]):
                continue
            a2, edges, iz, _ = RO.face_setup((X, Y, zc), a, b, c)
            if a2 == 0:
                continue
            ys, xs = np.nonzero(face_image[v] == f)
            w, _ = RO.weights(edges, xs.astype(np.int64), ys.astype(np.int64))
            T = texel[f].astype(D)
            with np.errstate(all="ignore"):
                q = [w[k].astype(D) * iz[k] for k in range(3)]
                den = (q[0] + q[1]) + q[2]
                tx = ((q[0] * T[0, 0] + q[1] * T[1, 0]) + q[2] * T[2, 0]) / den
                ty = ((q[0] * T[0, 1] + q[1] * T[1, 1]) + q[2] * T[2, 1]) / den
                good = (np.abs(tx) <= F64_MAX) & (np.abs(ty) <= F64_MAX)
                col = bilinear(atlas, clamp_to(np.where(good, tx, 0.0), D(S - 1)), clamp_to(np.where(good, ty, 0.0), D(Sy - 1)))
            out[v, ys[good], xs[good]] = col[good]
    return out


# ---- the whole path ----------------------------------------------------------------------------------------------------------------
def texture(verts, faces, rgb, images, cams, near, max_size=8192, shift=0, cull="none", background=(0, 0, 0), face_images=None):
    """-> dict: best (uint64), klass, order (int32), table, texel, atlas, owner, stats (dict of STAT_NAMES and faces_per_class), shift,
    uv (nf,3,2) float32.  face_images: used in place of the oracle rasteriser's (hostile face images)."""
    verts, faces = _mesh(verts, faces)
    cams = np.asarray(cams, np.float64).reshape(-1, 16)
    images = np.asarray(images, np.uint8)
    V, H, W = images.shape[:3]
    if face_images is None:
        face_images = RO.render(verts, faces, rgb, cams, H, W, near, cull)["face"]
    best = vote(verts, faces, face_images, cams, near)
    views, Ps = chosen(verts, faces, best, cams, H, W, near)
    while True:
        klass, capped = classes(faces, views, Ps, shift)
        order, table, texel = layout(klass)
        if table["S"] <= max_size:
            break
        if shift == MAX_SHIFT:
            raise Refused((table["S"], table["Sy"]))
        shift += 1
    atlas, owner, counts = fill(verts, faces, rgb, images, cams, near, views, order, table, texel, background)
    stats = {"faces_seen": sum(1 for v in views if v >= 0), "faces_unseen": views.count(-1), "faces_invalid": views.count(-2), "faces_capped": sum(capped)}
    stats.update(counts)
    stats["faces_per_class"] = {k: table["classes"][k]["faces"] for k in range(MIN_CLASS, MAX_CLASS + 1)}
    t = texel.astype(D)
    uv = np.stack([(t[..., 0] + 0.5) / D(table["S"]), 1.0 - (t[..., 1] + 0.5) / D(table["Sy"])], -1).astype(np.float32)
    return {"best": np.array(best, np.uint64).reshape(-1), "views": views, "klass": np.array(klass, np.int32).reshape(-1), "order": np.array(order, np.int32).reshape(-1),
            "table": table, "texel": texel, "atlas": atlas, "owner": owner, "stats": stats, "shift": shift, "uv": uv, "face_images": face_images}
