"""numpy restatement of csrc/poisson_math.h and of the order in which csrc/poisson.hip applies it: the classes of the points, the
fixed-point splats (np.rint to int64, integer sums), the planes, the right-hand side, the multigrid cycle with its mirrored ghost, the
isovalue through rcmvs_pc_moments' summation tree, and the field.  Planes are stored as fp32 and every expression is fp64 in the
header's order, so the kernels are expected to give the same bits.  Arrays of voxels are flat, voxel (i, j, k) at i + gx (j + gy k);
inside the functions they are viewed as (gz, gy, gx)."""
import numpy as np

from cloud_clean_oracle import tree_sum

F32, F64 = np.float32, np.float64
FIX, CFIX = F64(2.0 ** 28), F64(2.0 ** 20)
FIX_INV, CFIX_INV = F64(1.0) / FIX, F64(1.0) / CFIX
OMEGA = F64(6.0) / F64(7.0)
COARSEST_SWEEPS = 64
MAX_LEVELS = 16
SPLATTED, NON_FINITE, ZERO_NORMAL, OUTSIDE = 0, 1, 2, 3


def levels(dims):
    out = [[int(d) for d in dims]]
    while len(out) < MAX_LEVELS and all(d % 2 == 0 and d // 2 >= 4 for d in out[-1]):
        out.append([d // 2 for d in out[-1]])
    return out


# ---- the points ---------------------------------------------------------------------------------------------------------------------
def cells(xyz, grid, dims):
    """-> (inside (n,), b (n,3) int64, w (n,3,2) fp64) of po::cell_of; b and w are meaningful where inside"""
    p = np.asarray(xyz, F32).astype(F64)
    o, h = np.asarray(grid[:3], F64), F64(grid[3])
    with np.errstate(all="ignore"):
        u = (p - o) / h - F64(0.5)
        f = np.floor(u)
        inside = ((f >= 0.0) & (f <= (np.asarray(dims, F64) - 2.0))).all(axis=1)
        fi = np.where(inside[:, None], f, 0.0)
        w1 = np.where(inside[:, None], u - fi, 0.0)
    return inside, fi.astype(np.int64), np.stack([F64(1.0) - w1, w1], axis=2)


def classify(xyz, normals, grid, dims):
    p, n = np.asarray(xyz, F32).astype(F64), np.asarray(normals, F32).astype(F64)
    with np.errstate(all="ignore"):
        l2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    finite = np.isfinite(p).all(axis=1) & np.isfinite(n).all(axis=1)
    inside, b, w = cells(xyz, grid, dims)
    what = np.where(~finite, NON_FINITE, np.where(l2 == 0.0, ZERO_NORMAL, np.where(inside, SPLATTED, OUTSIDE)))
    return what, b, w, l2


def corner(b, w, code, dims):
    """-> (weights (m,), voxel numbers (m,)) of corner `code` of the cells b, w"""
    dx, dy, dz = code & 1, (code >> 1) & 1, code >> 2
    wt = (w[:, 0, dx] * w[:, 1, dy]) * w[:, 2, dz]
    vox = (b[:, 0] + dx) + dims[0] * ((b[:, 1] + dy) + dims[1] * (b[:, 2] + dz))
    return wt, vox


def interpolate(plane, b, w, dims):
    """the sum over the corners in code order of weight * (double)plane, from 0.0"""
    s = np.zeros(len(b), F64)
    for code in range(8):
        wt, vox = corner(b, w, code, dims)
        s = s + wt * plane[vox].astype(F64)
    return s


def splat(xyz, normals, rgb, grid, dims, density_weight=True):
    """-> dict: acc (planes, voxels) int64, W, V (3, voxels), C (3, voxels) or None (fp32), point (n,2) fp64, counters (8,) int64"""
    voxels = int(np.prod(dims))
    n = len(xyz)
    what, b, w, l2 = classify(xyz, normals, grid, dims)
    ok = what == SPLATTED
    b, w = b[ok], w[ok]
    nrm = np.asarray(normals, F32).astype(F64)[ok]
    acc = np.zeros((7 if rgb is not None else 4, voxels), np.int64)
    for code in range(8):
        wt, vox = corner(b, w, code, dims)
        np.add.at(acc[0], vox, np.rint(wt * FIX).astype(np.int64))
    W = (acc[0].astype(F64) * FIX_INV).astype(F32)
    wp = interpolate(W, b, w, dims)
    s = F64(1.0) / wp if density_weight else np.ones(len(wp), F64)
    point = np.zeros((n, 2), F64)
    point[ok, 0], point[ok, 1] = s, wp
    root = np.sqrt(l2[ok])
    for a in range(3):
        nc = nrm[:, a] / root
        for code in range(8):
            wt, vox = corner(b, w, code, dims)
            np.add.at(acc[1 + a], vox, np.rint(((s * wt) * nc) * FIX).astype(np.int64))
            if rgb is not None:
                np.add.at(acc[4 + a], vox, np.rint((wt * np.asarray(rgb)[ok, a].astype(F64)) * CFIX).astype(np.int64))
    V = (acc[1:4].astype(F64) * FIX_INV).astype(F32)
    C = None
    if rgb is not None:
        with np.errstate(all="ignore"):
            C = ((acc[4:7].astype(F64) * CFIX_INV) / (acc[0].astype(F64) * FIX_INV)).astype(F32)
        C[:, acc[0] == 0] = F32(128.0)
    counters = np.zeros(8, np.int64)
    counters[:4] = np.bincount(what, minlength=4)
    return {"acc": acc, "W": W, "V": V, "C": C, "point": point, "counters": counters, "what": what}


# ---- the grid -----------------------------------------------------------------------------------------------------------------------
def _shape(dims):
    return (int(dims[2]), int(dims[1]), int(dims[0]))


def rhs(V, grid, dims):
    h = F64(grid[3])
    p = [np.pad(V[c].astype(F64).reshape(_shape(dims)), 1) for c in range(3)]
    b = (((p[0][1:-1, 1:-1, 2:] - p[0][1:-1, 1:-1, :-2]) + (p[1][1:-1, 2:, 1:-1] - p[1][1:-1, :-2, 1:-1])) + (p[2][2:, 1:-1, 1:-1] - p[2][:-2, 1:-1, 1:-1])) / (F64(2.0) * h)
    return b.astype(F32).reshape(-1)


def six(x):
    """x (gz, gy, gx) fp64 -> the six neighbours added in the order -x +x -y +y -z +z, the ghost MINUS the cell itself"""
    p = np.pad(x, 1)
    p[0], p[-1] = -p[1], -p[-2]
    p[:, 0], p[:, -1] = -p[:, 1], -p[:, -2]
    p[:, :, 0], p[:, :, -1] = -p[:, :, 1], -p[:, :, -2]
    return ((((p[1:-1, 1:-1, :-2] + p[1:-1, 1:-1, 2:]) + p[1:-1, :-2, 1:-1]) + p[1:-1, 2:, 1:-1]) + p[:-2, 1:-1, 1:-1]) + p[2:, 1:-1, 1:-1]


def sweep(x, b, h2):
    """x, b (gz, gy, gx) fp32 -> the next x, fp32"""
    xd = x.astype(F64)
    return ((F64(1.0) - OMEGA) * xd + (OMEGA * (six(xd) - h2 * b.astype(F64))) / F64(6.0)).astype(F32)


def residual(x, b, h2):
    xd = x.astype(F64)
    return b.astype(F64) - (six(xd) - F64(6.0) * xd) / h2


def restrict(x, b, h2):
    r = residual(x, b, h2)
    s = np.zeros(tuple(n // 2 for n in r.shape), F64)
    for code in range(8):
        dx, dy, dz = code & 1, (code >> 1) & 1, code >> 2
        s = s + r[dz::2, dy::2, dx::2]
    return (F64(0.125) * s).astype(F32)


def _prolong_axis(e, axis):
    e = np.moveaxis(e, axis, 0)
    p = np.concatenate([-e[:1], e, -e[-1:]])
    out = np.empty((2 * e.shape[0],) + e.shape[1:], F64)
    out[0::2] = F64(0.75) * e + F64(0.25) * p[:-2]
    out[1::2] = F64(0.75) * e + F64(0.25) * p[2:]
    return np.moveaxis(out, 0, axis)


def prolong(x, e):
    """x fine fp32, e coarse fp32 -> x + the interpolated e, fp32: per axis 3/4 parent + 1/4 neighbour, x then y then z"""
    v = _prolong_axis(_prolong_axis(_prolong_axis(e.astype(F64), 2), 1), 0)
    return (x.astype(F64) + v).astype(F32)


def cycle(x, b, grid, dims):
    """one V(2,2) cycle -> (x flat fp32, coarse: the flat {x, tmp, b} of every coarser level as the kernels leave them, max |residual|)"""
    lv = levels(dims)
    L = len(lv)
    xs, bs, tmps = [None] * L, [None] * L, [None] * L
    xs[0], bs[0] = np.asarray(x, F32).reshape(_shape(dims)), np.asarray(b, F32).reshape(_shape(dims))
    h = F64(grid[3])
    h2 = []
    for l in range(L):
        h2.append(h * h)
        h = F64(2.0) * h

    def sweeps(l, count):
        for _ in range(count // 2):                               # x -> tmp -> x
            tmps[l] = sweep(xs[l], bs[l], h2[l])
            xs[l] = sweep(tmps[l], bs[l], h2[l])

    for l in range(L - 1):
        if l > 0:
            xs[l] = np.zeros(_shape(lv[l]), F32)
        sweeps(l, 2)
        bs[l + 1] = restrict(xs[l], bs[l], h2[l])
    if L > 1:
        xs[L - 1] = np.zeros(_shape(lv[L - 1]), F32)
    sweeps(L - 1, COARSEST_SWEEPS)
    for l in range(L - 2, -1, -1):
        xs[l] = prolong(xs[l], xs[l + 1])
        sweeps(l, 2)
    coarse = np.concatenate([np.zeros(0, F32)] + [a.reshape(-1) for l in range(1, L) for a in (xs[l], tmps[l], bs[l])])
    return xs[0].reshape(-1), coarse, F64(np.abs(residual(xs[0], bs[0], h2[0])).max())


def solve(b, grid, dims, cycles):
    """-> (x, [x after every cycle], [coarse after every cycle], [residual after every cycle])"""
    x = np.zeros(int(np.prod(dims)), F32)
    xs, coarse, resid = [], [], []
    for _ in range(cycles):
        x, c, r = cycle(x, b, grid, dims)
        xs.append(x)
        coarse.append(c)
        resid.append(r)
    return x, xs, coarse, resid


# ---- the isovalue and the field -----------------------------------------------------------------------------------------------------
def iso_stats(xyz, point, chi, grid, dims):
    """-> (stats (8,) fp64 as rcmvs_po_iso leaves them, terms (4, n))"""
    n = len(xyz)
    inside, b, w = cells(xyz, grid, dims)
    ok = (point[:, 0] > 0.0) & inside
    terms = np.zeros((4, n), F64)
    xp = interpolate(np.asarray(chi, F32), b[ok], w[ok], dims)
    terms[0, ok] = point[ok, 0] * xp
    terms[1, ok] = point[ok, 0]
    terms[2, ok] = point[ok, 1]
    terms[3, ok] = 1.0
    r = [tree_sum(terms[q]) for q in range(4)]
    stats = np.zeros(8, F64)
    stats[0] = r[0] / r[1] if r[1] > 0 else 0.0
    stats[1:5] = r
    stats[5] = r[2] / r[3] if r[3] > 0 else 0.0
    stats[6] = terms[2, ok].min() if ok.any() else np.inf
    return stats, terms


def dilate(W, dims):
    """the maximum of W over every voxel's 3 x 3 x 3 neighbourhood inside the grid (W >= 0)"""
    p = np.pad(np.asarray(W, F32).reshape(_shape(dims)), 1)
    gz, gy, gx = _shape(dims)
    out = np.zeros((gz, gy, gx), F32)
    for a in range(3):
        for bb in range(3):
            for c in range(3):
                out = np.maximum(out, p[a:a + gz, bb:bb + gy, c:c + gx])
    return out.reshape(-1)


def field(chi, W, iso, trim, dims):
    """-> (dsum, wsum fp32, trimmed voxels)"""
    dsum = (np.asarray(chi, F32).astype(F64) - F64(iso)).astype(F32)
    wsum = (dilate(W, dims).astype(F64) >= F64(trim)).astype(F32)
    return dsum, wsum, int((wsum == 0).sum())


def reconstruct(xyz, normals, rgb, grid, dims, cycles=8, trim=0.0, trim_relative=None, density_weight=True):
    """every stage of the pipeline -> dict (the splat's entries, b, x, xs, coarse, resid, stats, trim, dsum, wsum, trimmed)"""
    r = splat(xyz, normals, rgb, grid, dims, density_weight)
    r["b"] = rhs(r["V"], grid, dims)
    r["x"], r["xs"], r["coarse"], r["resid"] = solve(r["b"], grid, dims, cycles)
    r["stats"], r["terms"] = iso_stats(xyz, r["point"], r["x"], grid, dims)
    r["trim"] = float(trim_relative) * float(r["stats"][5]) if trim_relative is not None else float(trim)
    r["dsum"], r["wsum"], r["trimmed"] = field(r["x"], r["W"], r["stats"][0], r["trim"], dims)
    return r
