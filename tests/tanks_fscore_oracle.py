"""fp64 numpy restatement of the Tanks and Temples F-score (rc_mvsnet_amd/tanks_fscore.py): the comparator of the kernel tests.
Plain numpy, brute force, the operation order of csrc/pc_register_math.h; imports nothing from the kernels."""
import numpy as np


def transform(pts, T):
    """((T0 x + T1 y) + T2 z) + T3 per row in fp64 -> (n,3) fp64 (not rounded)"""
    p = np.asarray(pts).astype(np.float64)
    T = np.asarray(T, dtype=np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], 1)


def crop(pts, axis, axis_min, axis_max, polygon, T=None):
    """-> (flags (n,) bool, the transformed points as fp32 (n,3)).  polygon (m,2): (u, v) in the plane of the two other axes."""
    q = np.asarray(pts, dtype=np.float32) if T is None else transform(pts, T).astype(np.float32)
    p = q.astype(np.float64)
    uv = [a for a in range(3) if a != axis]
    pu, pv = p[:, uv[0]], p[:, uv[1]]
    poly = np.asarray(polygon, dtype=np.float64)
    m = len(poly)
    odd = np.zeros(len(p), dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(m):
            j = (i - 1) % m
            ui, vi, uj, vj = poly[i, 0], poly[i, 1], poly[j, 0], poly[j, 1]
            straddle = ((vi < pv) & (vj >= pv)) | ((vj < pv) & (vi >= pv))
            x = ui + (pv - vi) / (vj - vi) * (uj - ui)
            odd ^= straddle & (x < pu)
    flags = (p[:, axis] >= axis_min) & (p[:, axis] <= axis_max) & odd
    return flags, q


def voxel_down_sample(pts, voxel):
    """one fp32 point per occupied voxel, ascending (kz, ky, kx): fp64 sums by np.add.at in index order, one division"""
    pts = np.asarray(pts, dtype=np.float32)
    if len(pts) == 0:
        return pts
    p = pts.astype(np.float64)
    org = pts.min(0).astype(np.float64) - voxel / 2
    k = np.floor((p - org) / voxel).astype(np.int64)
    g = np.floor((pts.max(0).astype(np.float64) - org) / voxel).astype(np.int64) + 1
    key = (k[:, 2] * g[1] + k[:, 1]) * g[0] + k[:, 0]
    uniq, inv = np.unique(key, return_inverse=True)
    sums = np.zeros((len(uniq), 3))
    np.add.at(sums, inv.ravel(), p)
    cnt = np.bincount(inv.ravel(), minlength=len(uniq)).astype(np.float64)
    return (sums / cnt[:, None]).astype(np.float32)


BRUTE_LIMIT = 4_000_000        # pairs; above it nearest() narrows every query to 8 candidates with a k-d tree first


def nearest(q, t, chunk=512, brute=None):
    """q (n,3) fp64, t (m,3) fp32 -> (index of the nearest t (the lower index wins ties), squared distance ((dx2 + dy2) + dz2)).
    Brute force over all pairs.  Large problems (the ICP loop's repeated searches) take the 8 nearest candidates of a
    scipy cKDTree first and apply the same arithmetic and tie rule to those: identical unless more than 8 targets tie
    (tests/test_tanks_fscore_cpu.py compares the two forms)."""
    q = np.asarray(q, dtype=np.float64)
    t = np.asarray(t).astype(np.float64)
    if brute is None:
        brute = len(q) * len(t) <= BRUTE_LIMIT
    if not brute and len(t) > 8:
        from scipy.spatial import cKDTree
        _, cand = cKDTree(t).query(q, k=8)
        cand = np.sort(cand, axis=1)
        d = q[:, None, :] - t[cand]
        dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        i = np.argmin(dd, axis=1)
        rows = np.arange(len(q))
        return cand[rows, i].astype(np.int64), dd[rows, i]
    idx = np.empty(len(q), dtype=np.int64)
    d2 = np.empty(len(q))
    for a in range(0, len(q), chunk):
        d = q[a:a + chunk, None, :] - t[None, :, :]
        dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        i = np.argmin(dd, axis=1)                       # the first minimum: the lower index
        idx[a:a + chunk] = i
        d2[a:a + chunk] = dd[np.arange(len(i)), i]
    return idx, d2


def nearest_two(q, t, chunk=512):
    """the two smallest squared distances of every q (for the tests' knife-edge checks on their own input)"""
    q = np.asarray(q, dtype=np.float64)
    t = np.asarray(t).astype(np.float64)
    out = np.empty((len(q), 2))
    for a in range(0, len(q), chunk):
        d = q[a:a + chunk, None, :] - t[None, :, :]
        dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        out[a:a + chunk] = np.sort(dd, axis=1)[:, :2] if t.shape[0] > 1 else np.concatenate([dd, np.full_like(dd, np.inf)], 1)
    return out


def icp_step(src, tgt, T, max_dist):
    """-> (18 moments {count, sum d2, sum s', sum t, sum s' t^T (a-major), sum |s'|2}, corr (n,) with -1 for none)"""
    s = transform(src, T)
    idx, d2 = nearest(s, tgt)
    ok = np.sqrt(d2) < max_dist
    corr = np.where(ok, idx, -1).astype(np.int32)
    sm, tm = s[ok], np.asarray(tgt).astype(np.float64)[idx[ok]]
    mom = np.zeros(18)
    mom[0] = ok.sum()
    mom[1] = d2[ok].sum()
    mom[2:5] = sm.sum(0)
    mom[5:8] = tm.sum(0)
    mom[8:17] = (sm[:, :, None] * tm[:, None, :]).sum(0).ravel()
    mom[17] = ((sm[:, 0] * sm[:, 0] + sm[:, 1] * sm[:, 1]) + sm[:, 2] * sm[:, 2]).sum()
    return mom, corr


def umeyama_from_moments(mom, with_scaling=True):
    n = mom[0]
    mu_s, mu_d = mom[2:5] / n, mom[5:8] / n
    cov = mom[8:17].reshape(3, 3) / n - np.outer(mu_s, mu_d)
    var_s = mom[17] / n - float(mu_s @ mu_s)
    U, D, Vt = np.linalg.svd(cov.T)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    c = float(np.trace(np.diag(D) @ S) / var_s) if with_scaling else 1.0
    T = np.eye(4)
    T[:3, :3] = c * R
    T[:3, 3] = mu_d - c * (R @ mu_s)
    return T


def icp(src, tgt, max_dist, init, max_iter=20, with_scaling=True, rel_fitness=1e-6, rel_rmse=1e-6):
    T = np.array(init, dtype=np.float64)
    n = len(src)

    def ev(T):
        mom, _ = icp_step(src, tgt, T, max_dist)
        return mom, mom[0] / n, (np.sqrt(mom[1] / mom[0]) if mom[0] > 0 else 0.0)

    mom, fit, rmse = ev(T)
    it = 0
    for _ in range(max_iter):
        if mom[0] < 3:
            break
        T = umeyama_from_moments(mom, with_scaling) @ T
        mom, f2, r2 = ev(T)
        it += 1
        done = abs(f2 - fit) < rel_fitness and abs(r2 - rmse) < rel_rmse
        fit, rmse = f2, r2
        if done:
            break
    return {"transformation": T, "fitness": float(fit), "inlier_rmse": float(rmse), "iterations": it}


def register(est, gt, init, vol, tau, max_iter=20):
    """vol = (axis, axis_min, axis_max, polygon (m,2))"""
    T = np.array(init, dtype=np.float64)
    f, q = crop(gt, *vol)
    gt_c = q[f]
    rounds = []
    for voxel, thr in ((tau, 80.0 * tau), (tau / 2.0, 20.0 * tau), (None, 2.0 * tau)):
        f, q = crop(est, *vol, T=T)
        est_c = q[f]
        if len(est_c) == 0 or len(gt_c) == 0:
            break
        if voxel is None:
            s, t = est_c[::max(1, len(est_c) // 4_000_000)], gt_c[::max(1, len(gt_c) // 4_000_000)]
        else:
            s, t = voxel_down_sample(est_c, voxel), voxel_down_sample(gt_c, voxel)
        r = icp(transform(s, np.linalg.inv(T)).astype(np.float32), t, thr, T, max_iter=max_iter)
        T = r["transformation"]
        rounds.append(r)
    return T, rounds


def capped_distances(q, t, cap):
    _, d2 = nearest(np.asarray(q).astype(np.float64), t)
    d = np.sqrt(d2)
    return np.where(d < cap, d, cap)


def evaluate(est, gt, T, vol, tau, stretch=5, down_sample=True):
    """down_sample=False scores the cropped clouds as they are (the known-answer cases with voxels off)"""
    nbins, w = 100 * stretch - 1, tau / 100.0
    f, q = crop(est, *vol, T=T)
    e = q[f]
    f, q = crop(gt, *vol)
    g = q[f]
    zero = np.zeros(nbins, dtype=np.uint64)
    if len(e) == 0 or len(g) == 0:
        return {"precision": 0.0, "recall": 0.0, "fscore": 0.0, "n_est": len(e), "n_gt": len(g), "hist_est": zero, "hist_gt": zero}
    if down_sample:
        e, g = voxel_down_sample(e, tau / 2.0), voxel_down_sample(g, tau / 2.0)
    cap = stretch * tau
    de, dg = capped_distances(e, g, cap), capped_distances(g, e, cap)
    edges = np.arange(nbins + 1) * w
    he = np.histogram(de, bins=edges)[0].astype(np.uint64)
    hg = np.histogram(dg, bins=edges)[0].astype(np.uint64)
    P, R = int((de < tau).sum()) / len(e), int((dg < tau).sum()) / len(g)
    F = 2.0 * P * R / (P + R) if P + R > 0 else 0.0
    return {"precision": P, "recall": R, "fscore": F, "n_est": len(e), "n_gt": len(g), "hist_est": he, "hist_gt": hg}
