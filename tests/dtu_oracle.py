"""fp64 numpy restatement of the DTU scorer (matlab_eval/PointCompareMain.m, reducePts_haa.m, MaxDistCP.m,
ComputeStat_web_pt.m), the yardstick of rc_mvsnet_amd/dtu_eval.py.  Same operation order as csrc/pointcloud_math.h.
TEST INFRASTRUCTURE ONLY."""
import numpy as np


def _d2(a, b):
    """squared distances (len(a), len(b)) of fp32 points, ((dx*dx + dy*dy) + dz*dz) in fp64"""
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    b = np.asarray(b, dtype=np.float32).astype(np.float64)
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def neighbours(pts, dst, chunk=1024):
    """rangesearch(pts, pts, dst): for every point the indices within dst (itself included)."""
    out = []
    for s in range(0, len(pts), chunk):
        m = np.sqrt(_d2(pts[s:s + chunk], pts)) <= dst
        out += [np.nonzero(r)[0] for r in m]
    return out


def greedy_reduce(pts, order, dst, nbrs=None):
    """reducePts_haa without chunks: visit points in order; a point still set clears its neighbours and keeps itself."""
    nbrs = neighbours(pts, dst) if nbrs is None else nbrs
    keep = np.ones(len(pts), dtype=bool)
    for i in order:
        if keep[i]:
            keep[nbrs[i]] = False
            keep[i] = True
    return keep


def matlab_chunked_reduce(pts, order, dst, chunk, nbrs=None):
    """reducePts_haa as written, with min(4e6, n-1) replaced by ``chunk``: Chunks = 1:chunk:n, Chunks(end) = n, and
    each Range = Chunks(c):Chunks(c+1) -- consecutive ranges share one point."""
    nbrs = neighbours(pts, dst) if nbrs is None else nbrs
    n = len(pts)
    keep = np.ones(n, dtype=bool)
    chunks = list(range(1, n + 1, min(chunk, n - 1)))
    chunks[-1] = n
    for c in range(len(chunks) - 1):
        for pos in range(chunks[c], chunks[c + 1] + 1):           # 1-based positions of RandOrd
            i = order[pos - 1]
            if keep[i]:
                keep[nbrs[i]] = False
                keep[i] = True
    return keep


def nearest(q_from, q_to, cap, lattice=None, chunk=1024):
    """min(NN distance, cap) in fp64; lattice = (lo, hi): from-points outside [lo, hi) get cap."""
    q_from = np.asarray(q_from, dtype=np.float32)
    out = np.full(len(q_from), float(cap))
    if len(q_to):
        for s in range(0, len(q_from), chunk):
            out[s:s + chunk] = np.minimum(np.sqrt(_d2(q_from[s:s + chunk], q_to).min(axis=1)), cap)
    if lattice is not None:
        lo, hi = (np.asarray(v, dtype=np.float64) for v in lattice)
        q = q_from.astype(np.float64)
        inside = np.all((q >= lo) & (q < hi), axis=1)
        out[~inside] = cap
    return out


def lattice(bb, edge=60.0):
    bb = np.asarray(bb, dtype=np.float64).reshape(2, 3)
    return bb[0], (bb[0] + np.floor((bb[1] - bb[0]) / edge) * edge) + edge


def matlab_round(x):
    """MATLAB round: half away from zero (exact; numpy's round is half-to-even and floor(x + 0.5) misrounds 0.49999999999999994)."""
    x = np.asarray(x, dtype=np.float64)
    t = np.trunc(x)
    return t + np.sign(x) * (np.abs(x - t) >= 0.5)


def data_in_mask(q, bb, res, obs_mask):
    """PointCompareMain's DataInMask; obs_mask indexed [x, y, z] (MATLAB's ObsMask(x, y, z) one-based)."""
    q = np.asarray(q, dtype=np.float32).astype(np.float64)
    bb0 = np.asarray(bb, dtype=np.float64).reshape(2, 3)[0]
    v = matlab_round((q - bb0) / res + 1.0)
    size = np.array(obs_mask.shape)
    ok = np.all((v >= 1) & (v <= size), axis=1)
    out = np.zeros(len(q), dtype=bool)
    vi = v[ok].astype(np.int64) - 1
    out[ok] = obs_mask[vi[:, 0], vi[:, 1], vi[:, 2]]
    return out


def stl_above_plane(q, P):
    q = np.asarray(q, dtype=np.float32).astype(np.float64)
    P = np.asarray(P, dtype=np.float64).ravel()
    return ((P[0] * q[:, 0] + P[1] * q[:, 1]) + P[2] * q[:, 2]) + P[3] > 0


def stats(d):
    """ComputeStat_web_pt's n / mean / var (N - 1) / median of one selected set; NaN for an empty set, var 0 for one value."""
    d = np.asarray(d, dtype=np.float64)
    if d.size == 0:
        return 0, np.nan, np.nan, np.nan
    var = float(np.var(d, ddof=1)) if d.size > 1 else 0.0
    return d.size, float(np.mean(d)), var, float(np.median(d))


def evaluate_scan(data, stl, obs_mask, bb, res, plane, order, dst=0.2, outlier=20.0, cap=60.0):
    """The whole scan: reduce, both distance passes (lattice rule), masks, statistics -> BaseStat's fields + per-point arrays."""
    keep = greedy_reduce(data, order, dst)
    qdata = np.asarray(data, dtype=np.float32)[keep]
    lat = lattice(bb)
    ddata = nearest(qdata, stl, cap, lat)
    dstl = nearest(stl, qdata, cap, lat)
    in_mask = data_in_mask(qdata, bb, res, obs_mask)
    above = stl_above_plane(stl, plane)
    nd, md, vd, medd = stats(ddata[in_mask & (ddata < outlier)])
    ns, ms, vs, meds = stats(dstl[above & (dstl < outlier)])
    return {"nStl": ns, "nData": nd, "MeanStl": ms, "MeanData": md, "VarStl": vs, "VarData": vd, "MedStl": meds, "MedData": medd,
            "keep": keep, "Ddata": ddata, "Dstl": dstl, "DataInMask": in_mask, "StlAbovePlane": above}
