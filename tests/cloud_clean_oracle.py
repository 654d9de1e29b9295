"""numpy restatement of the point-cloud clean-up (csrc/cloud_knn.hip; the rules of csrc/cloud_knn_math.h operation by operation):
brute-force fp64 distances, the (d2, index) order, the mean distance, rcmvs_pc_moments' summation tree, the statistical bound, the
radius count, and the normal of a neighbourhood (covariance, cyclic Jacobi, choice and orientation of the eigenvector).  Every
function returns what the kernels must give in every bit."""
import math

import numpy as np

MAX_SWEEPS = 32
DEGENERATE = 1e-12
COUNTER_NAMES = ("with_normal", "too_few", "degenerate", "unconverged", "unoriented", "flipped", "oriented")


def finite(pts):
    return np.isfinite(np.asarray(pts, np.float32)).all(axis=1)


def dist2(pts):
    """(n,n) fp64: ((dx dx + dy dy) + dz dz) of the fp32 coordinates promoted to fp64"""
    p = np.asarray(pts, np.float32).astype(np.float64)
    d = p[:, None, 0] - p[None, :, 0]
    out = d * d
    d = p[:, None, 1] - p[None, :, 1]
    out = out + d * d
    d = p[:, None, 2] - p[None, :, 2]
    return out + d * d


def knn(pts, k):
    """-> idx (n,k) int32, d2 (n,k) fp64, mean (n,) fp64"""
    n = len(pts)
    idx = np.full((n, k), -1, np.int32)
    d2 = np.full((n, k), np.inf, np.float64)
    if n > 1:
        D = dist2(pts)
        assert np.isfinite(D).all()
        D[np.arange(n), np.arange(n)] = np.inf                    # the point itself: last in a stable sort, and never taken
        order = np.argsort(D, axis=1, kind="stable")[:, :min(k, n - 1)]
        idx[:, :order.shape[1]] = order
        d2[:, :order.shape[1]] = np.take_along_axis(D, order, axis=1)
    s = np.zeros(n, np.float64)
    for j in range(k):
        s = s + np.sqrt(d2[:, j])
    mean = s / np.float64(k)
    mean[(idx < 0).any(axis=1)] = np.nan
    return idx, d2, mean


def tree_sum(x):
    """rcmvs_pc_moments' order: lane t of 65536 adds x[t], x[t + 65536], ... from 0.0; a block of 256 lanes halves down; the 256
    block sums are added in order from 0.0"""
    T = 65536
    lane = np.zeros(T, np.float64)
    for r in range(0, len(x), T):
        c = x[r:r + T]
        lane[:len(c)] = lane[:len(c)] + c
    sh = lane.reshape(256, 256).copy()
    o = 128
    while o > 0:
        sh[:, :o] = sh[:, :o] + sh[:, o:2 * o]
        o >>= 1
    s = np.float64(0.0)
    for b in range(256):
        s = s + sh[b, 0]
    return s


def moments(x):
    """-> (n, mean, variance N - 1): NaN for none, variance 0 for one"""
    x = np.asarray(x, np.float64)
    n = len(x)
    with np.errstate(all="ignore"):
        mean = tree_sum(x) / np.float64(n) if n > 0 else np.float64(np.nan)
        d = x - mean
        s2 = tree_sum(d * d)
        var = s2 / np.float64(n - 1) if n > 1 else (np.float64(0.0) if n == 1 else np.float64(np.nan))
    return n, mean, var


def threshold(mu, sigma, ratio):
    if ratio == np.inf:
        return np.float64(np.inf)
    with np.errstate(all="ignore"):
        return np.float64(mu) + np.float64(ratio) * np.float64(sigma)


def statistical(mean, ratio):
    """-> keep (n,) uint8, (valid, mu, sigma, threshold)"""
    mean = np.asarray(mean, np.float64)
    valid = ~np.isnan(mean)
    n, mu, var = moments(mean[valid])
    with np.errstate(all="ignore"):
        sigma = np.sqrt(var)
        thr = threshold(mu, sigma, ratio)
        keep = valid & (mean <= thr)
    return keep.astype(np.uint8), (n, mu, sigma, thr)


def radius(pts, r, cap):
    """-> counts (n,) int32 saturating at cap, keep (n,) uint8"""
    n = len(pts)
    r2 = np.float64(r) * np.float64(r)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.uint8)
    D = dist2(pts)
    inside = D <= r2
    inside[np.arange(n), np.arange(n)] = False
    c = np.minimum(inside.sum(axis=1), cap).astype(np.int32)
    return c, (c >= cap).astype(np.uint8)


def _rotate(a, p, q, r, v):
    """one Jacobi rotation on the symmetric matrix a (3,3 list of python floats kept symmetric by hand) and the columns v[p], v[q]"""
    theta = (a[q][q] - a[p][p]) / (float(2.0) * a[p][q])
    den = abs(theta) + math.sqrt(theta * theta + float(1.0))
    t = float(1.0) / den if theta >= 0.0 else float(-1.0) / den
    c = float(1.0) / math.sqrt(t * t + float(1.0))
    s = t * c
    h = t * a[p][q]
    a[p][p] = a[p][p] - h
    a[q][q] = a[q][q] + h
    a[p][q] = a[q][p] = float(0.0)
    rp, rq = a[r][p], a[r][q]
    a[r][p] = a[p][r] = c * rp - s * rq
    a[r][q] = a[q][r] = s * rp + c * rq
    for i in range(3):
        x, y = v[p][i], v[q][i]
        v[p][i] = c * x - s * y
        v[q][i] = s * x + c * y


def jacobi(cov):
    """cov: (xx, xy, xz, yy, yz, zz) -> (lam [3], v: v[c] = column c, converged, sweeps)"""
    xx, xy, xz, yy, yz, zz = (float(t) for t in cov)
    a = [[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]
    v = [[float(1.0 if i == j else 0.0) for i in range(3)] for j in range(3)]
    done, sweeps = False, 0
    with np.errstate(all="ignore"):
        while sweeps < MAX_SWEEPS and not done:
            done = True
            for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
                if a[p][q] != 0.0:
                    _rotate(a, p, q, r, v)
                    done = False
            sweeps += 1
    conv = done or (a[0][1] == 0.0 and a[0][2] == 0.0 and a[1][2] == 0.0)
    return [a[0][0], a[1][1], a[2][2]], v, conv, sweeps


def normal_of(cov):
    """-> (n [3] fp64, what: 0 with a normal / 2 degenerate, converged, (l0, l1, l2))"""
    lam, v, conv, _ = jacobi(cov)
    lo = 0
    if lam[1] < lam[lo]:
        lo = 1
    if lam[2] < lam[lo]:
        lo = 2
    hi = 2
    if lam[1] > lam[hi]:
        hi = 1
    if lam[0] > lam[hi]:
        hi = 0
    mid = 3 - lo - hi
    l1, l2 = lam[mid], lam[hi]
    zero = [float(0.0)] * 3
    with np.errstate(all="ignore"):
        if l2 == 0.0 or not (l1 > float(DEGENERATE) * l2):
            return zero, 2, conv, (lam[lo], l1, l2)
        x, y, z = v[lo]
        ln = math.sqrt((x * x + y * y) + z * z)
        if not ln > 0.0:
            return zero, 2, conv, (lam[lo], l1, l2)
        u = [x / ln, y / ln, z / ln]
    ax, ay, az = (abs(t) for t in u)
    big = u[0] if (ax >= ay and ax >= az) else (u[1] if ay >= az else u[2])
    if big < 0.0:
        u = [-t for t in u]
    return u, 0, conv, (lam[lo], l1, l2)


def covariance(pts, i, nbrs):
    """the point i first, then its existing neighbours in slot order -> (m, (xx, xy, xz, yy, yz, zz))"""
    p = pts if isinstance(pts, list) else np.asarray(pts, np.float32).astype(np.float64).tolist()
    rows = [i] + [int(j) for j in nbrs if 0 <= j < len(p)]
    m = len(rows)
    s = [p[i][0], p[i][1], p[i][2]]
    for j in rows[1:]:
        s = [s[0] + p[j][0], s[1] + p[j][1], s[2] + p[j][2]]
    if m < 3:
        return m, None
    md = float(m)
    mean = [s[0] / md, s[1] / md, s[2] / md]
    c = [float(0.0)] * 6
    for j in rows:
        dx, dy, dz = p[j][0] - mean[0], p[j][1] - mean[1], p[j][2] - mean[2]
        c = [c[0] + dx * dx, c[1] + dx * dy, c[2] + dx * dz, c[3] + dy * dy, c[4] + dy * dz, c[5] + dz * dz]
    return m, [t / md for t in c]


def normals(pts, idx, view=None, centres=None, details=False):
    """-> normals (n,3) fp32, counters dict; details: also the per-point (l0, l1, l2) and fp64 normals"""
    pts = np.asarray(pts, np.float32)
    n = len(pts)
    out = np.zeros((n, 3), np.float32)
    full = np.zeros((n, 3), np.float64)
    lams = np.full((n, 3), np.nan)
    cnt = dict.fromkeys(COUNTER_NAMES, 0)
    cen = None if centres is None else np.asarray(centres, np.float64).reshape(-1, 3)
    plist = pts.astype(np.float64).tolist()
    with np.errstate(all="ignore"):
        for i in range(n):
            m, cov = covariance(plist, i, idx[i])
            if m < 3:
                cnt["too_few"] += 1
                continue
            u, what, conv, lam = normal_of(cov)
            lams[i] = lam
            cnt["unconverged"] += 0 if conv else 1
            if what != 0:
                cnt["degenerate"] += 1
                continue
            cnt["with_normal"] += 1
            if view is not None:
                w = int(view[i])
                if not 0 <= w < len(cen):
                    cnt["unoriented"] += 1
                else:
                    p = plist[i]
                    dx, dy, dz = float(cen[w, 0]) - p[0], float(cen[w, 1]) - p[1], float(cen[w, 2]) - p[2]
                    d = (u[0] * dx + u[1] * dy) + u[2] * dz
                    if d < 0.0:
                        u = [-t for t in u]
                        cnt["flipped"] += 1
                    else:
                        cnt["oriented"] += 1
            full[i] = u
            out[i] = np.array(u, np.float64).astype(np.float32)
    return (out, cnt, lams, full) if details else (out, cnt)


def clean_cloud(xyz, rgb=None, view=None, centres=None, radius_opt=None, stat=None, normals_k=None):
    """the steps of cloud_clean.clean_cloud -> dict of numpy arrays xyz, rgb, view, normals, index and the figures of every step"""
    xyz = np.asarray(xyz, np.float32)
    index = np.arange(len(xyz), dtype=np.int32)
    info = {}

    def cut(keep):
        nonlocal xyz, rgb, view, index
        keep = keep.astype(bool)
        xyz, index = xyz[keep], index[keep]
        rgb = None if rgb is None else rgb[keep]
        view = None if view is None else view[keep]

    f = finite(xyz)
    info["finite_removed"] = int((~f).sum())
    cut(f)
    if radius_opt is not None:
        cut(radius(xyz, radius_opt[0], radius_opt[1])[1])
        info["radius_out"] = len(xyz)
    if stat is not None:
        keep, (nv, mu, sigma, thr) = statistical(knn(xyz, stat[0])[2], stat[1])
        cut(keep)
        info.update(valid=nv, mu=mu, sigma=sigma, threshold=thr, stat_out=len(xyz))
    nrm = None
    if normals_k is not None:
        nrm, cnt = normals(xyz, knn(xyz, normals_k)[0], view, centres if view is not None else None)
        info["counters"] = cnt
    return {"xyz": xyz, "rgb": rgb, "view": view, "normals": nrm, "index": index, "info": info}
