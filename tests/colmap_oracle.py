"""fp64 numpy restatement of the COLMAP import (rc_mvsnet_amd/colmap_import.py): the comparator of the kernel tests.  Plain numpy,
the operation order of csrc/view_select_math.h; imports nothing from the kernels."""
import numpy as np

DEG = 180.0 / np.pi


def quat_to_rotmat(q):
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def angle_deg(ci, cj, x):
    """atan2(|a x b|, a.b) in degrees for a = ci - x, b = cj - x; x (k,3)"""
    a, b = ci[None, :] - x, cj[None, :] - x
    c0 = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    c1 = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    c2 = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    cross = np.sqrt((c0 * c0 + c1 * c1) + c2 * c2)
    dot = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
    return np.arctan2(cross, dot) * DEG


def weight(theta, theta0=5.0, sigma1=1.0, sigma2=10.0):
    sigma = np.where(theta <= theta0, sigma1, sigma2)
    d = theta - theta0
    return np.exp(-(d * d) / (2.0 * sigma * sigma))


def pair_scores(centres, points, offsets, ids, theta0=5.0, sigma1=1.0, sigma2=10.0):
    """-> (scores (n,n) fp64, common (n,n) int64 = the number of shared points)"""
    n, m = len(centres), len(points)
    S, K = np.zeros((n, n)), np.zeros((n, n), dtype=np.int64)
    mask = np.zeros(m, dtype=bool)
    for i in range(n):
        li = ids[offsets[i]:offsets[i + 1]]
        mask[li] = True
        for j in range(i + 1, n):
            lj = ids[offsets[j]:offsets[j + 1]]
            common = lj[mask[lj]]
            if len(common):
                s = weight(angle_deg(centres[i], centres[j], points[common]), theta0, sigma1, sigma2).sum()
                S[i, j] = S[j, i] = s
                K[i, j] = K[j, i] = len(common)
        mask[li] = False
    return S, K


def top_views(scores, k):
    """-> ([per row the partner ids, score descending then index ascending, score > 0 only, at most k], counts)"""
    lists, counts = [], []
    for i, row in enumerate(scores):
        cand = [j for j in range(len(row)) if j != i and row[j] > 0]
        cand.sort(key=lambda j: (-row[j], j))
        lists.append(cand[:k])
        counts.append(len(cand))
    return lists, np.array(counts)


def depths(points, zrow, ids):
    """((r20 x + r21 y) + r22 z) + t2, left to right"""
    p = points[ids]
    return ((zrow[0] * p[:, 0] + zrow[1] * p[:, 1]) + zrow[2] * p[:, 2]) + zrow[3]


def ranks(c):
    return int(c * 0.01), int(c * 0.99)


def depth_ranks(points, zrows, offsets, ids, rk):
    """-> (n,2): np.sort of every image's z at its two ranks"""
    out = np.zeros((len(zrows), 2))
    for i in range(len(zrows)):
        z = np.sort(depths(points, zrows[i], ids[offsets[i]:offsets[i + 1]]))
        out[i] = z[rk[i, 0]], z[rk[i, 1]]
    return out
