"""The exact oracle of the depth-map fusion kernels (csrc/fusion.hip: rcmvs_fuse_view, rcmvs_compact_points): vectorised numpy that
restates the per-pixel rule of csrc/fusion_math.h without calling it, so that every output of the kernel, of the g++ loop harness and
of the CPU emulation can be compared with it in every bit at every pixel.

The rule.  The chain is float64; every product and every sum is one rounded operation, taken left to right as written below (numpy
rounds each ufunc call once and never fuses a multiply with an add); the float32 cast points are the reference's
(eval_rcmvsnet_dtu.py:281-338, :369-425): the source position, the sampled source depth, the reprojected depth, the reprojected
position, the relative depth difference, the sum over the source views (sequential, float32, starting from 0) and its sum with the
reference depth.  The source depth is sampled as cv2.remap(INTER_LINEAR) does: positions times 32 in float32, rounded to the nearest
integer with ties to even (np.rint), a float32 weight table of 1/32 steps, taps outside the image 0, positions that are NaN or at
least 1e9 / 32 pixels away 0.  Comparisons with NaN are false.  The colour bytes truncate img * 255 (float32)."""
import numpy as np

REF_MATS, SRC_MATS = 30, 42
FAR = np.iinfo(np.int64).min                                         # ix / iy of a position remap_linear treats as outside before rounding

F32 = np.float32


def _mul3(m, a, b, c):
    """(3x3 row-major) * (a, b, c): ((m0 a + m1 b) + m2 c)"""
    return [m[3 * r] * a + m[3 * r + 1] * b + m[3 * r + 2] * c for r in range(3)]


def _mul34(m, v):
    """(3x4 row-major) * (v, 1): (((m0 v0 + m1 v1) + m2 v2) + m3)"""
    return [m[4 * r] * v[0] + m[4 * r + 1] * v[1] + m[4 * r + 2] * v[2] + m[4 * r + 3] for r in range(3)]


def remap_exact(img, x, y):
    """one float32 plane sampled at float32 positions (x, y) -> (value float32, ix, iy int64 with FAR where the position is NaN or too far)"""
    H, W = img.shape
    fx, fy = x * F32(32.0), y * F32(32.0)
    far = ~(np.abs(fx) < F32(1.0e9)) | ~(np.abs(fy) < F32(1.0e9))
    sx = np.rint(np.where(far, F32(0.0), fx)).astype(np.int64)
    sy = np.rint(np.where(far, F32(0.0), fy)).astype(np.int64)
    ix, iy = sx >> 5, sy >> 5
    ax, ay = (sx & 31).astype(F32) * F32(1.0 / 32.0), (sy & 31).astype(F32) * F32(1.0 / 32.0)
    outside = far | (ix >= W) | (ix + 1 < 0) | (iy >= H) | (iy + 1 < 0)
    one = F32(1.0)
    w = [(one - ay) * (one - ax), (one - ay) * ax, ay * (one - ax), ay * ax]
    taps = []
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        xx, yy = ix + dx, iy + dy
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        taps.append(np.where(inside, img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], F32(0.0)).astype(F32))
    val = taps[0] * w[0] + taps[1] * w[1] + taps[2] * w[2] + taps[3] * w[3]
    assert val.dtype == np.float32
    return np.where(outside, F32(0.0), val), np.where(far, FAR, ix), np.where(far, FAR, iy)


def fuse_view_exact(depth_all, ref, srcs, conf, img, mats, prob, ncons, dist_t, depth_t):
    """depth_all (V,H,W) fp32, ref / srcs view numbers, conf (H,W) fp32, img (H,W,3) fp32 or None, mats the float64 vector of
    fusion.fusion_matrices, the four thresholds as the entry point takes them (prob and depth_t are rounded to float32, dist_t stays
    float64).  Returns at ALL pixels: masks (3,H,W) uint8 [photo, geo, final], depth_avg (H,W) fp32, xyz (H,W,3) fp32, rgb (H,W,3) uint8
    or None, the debug outputs depth_reprojected (N,H,W) fp32, geo (N,H,W) uint8, xy_src (N,H,W,2) fp32, and for building cases dist
    (N,H,W) fp64, rel (N,H,W) fp32, z_src (N,H,W) fp64 (the point's z in the source camera), ix / iy (N,H,W) int64 (the top-left tap)."""
    depth_all = np.asarray(depth_all)
    conf = np.asarray(conf)
    mats = np.asarray(mats)
    assert depth_all.dtype == np.float32 and conf.dtype == np.float32 and mats.dtype == np.float64
    V, H, W = depth_all.shape
    N = len(srcs)
    assert mats.shape == (REF_MATS + SRC_MATS * N,) and conf.shape == (H, W)
    prob, depth_t, dist_t = F32(prob), F32(depth_t), np.float64(dist_t)
    rm = mats[:REF_MATS]
    yi, xi = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x, y = xi.astype(np.float64), yi.astype(np.float64)
    d_ref = depth_all[ref]
    d = d_ref.astype(np.float64)
    out = {k: [] for k in ("depth_reprojected", "geo", "xy_src", "dist", "rel", "z_src", "ix", "iy")}
    geo_sum = np.zeros((H, W), np.int32)
    acc = np.zeros((H, W), np.float32)
    with np.errstate(all="ignore"):
        p_ref = _mul3(rm, x * d, y * d, d)
        for n, s in enumerate(srcs):
            sm = mats[REF_MATS + n * SRC_MATS:REF_MATS + (n + 1) * SRC_MATS]
            q = _mul34(sm, p_ref)
            k = _mul3(sm[12:21], q[0], q[1], q[2])
            xs, ys = k[0] / k[2], k[1] / k[2]
            x_src, y_src = xs.astype(F32), ys.astype(F32)
            sampled, ix, iy = remap_exact(depth_all[s], x_src, y_src)
            sd = sampled.astype(np.float64)
            p = _mul3(sm[21:30], xs * sd, ys * sd, sd)
            qb = _mul34(sm[30:42], p)
            d_rep = qb[2].astype(F32)
            kb = _mul3(rm[9:18], qb[0], qb[1], qb[2])
            xr, yr = (kb[0] / kb[2]).astype(F32), (kb[1] / kb[2]).astype(F32)
            dx, dy = xr.astype(np.float64) - x, yr.astype(np.float64) - y
            dist = np.sqrt(dx * dx + dy * dy)
            rel = np.abs(d_rep - d_ref) / d_ref
            assert rel.dtype == np.float32 and dist.dtype == np.float64
            ok = (dist < dist_t) & (rel < depth_t)
            depth = np.where(ok, d_rep, F32(0.0))
            geo_sum = geo_sum + ok.astype(np.int32)
            acc = acc + depth
            for key, val in (("depth_reprojected", depth), ("geo", ok.astype(np.uint8)), ("xy_src", np.stack([x_src, y_src], -1)), ("dist", dist),
                             ("rel", rel), ("z_src", q[2] + np.zeros((H, W))), ("ix", ix), ("iy", iy)):
                out[key].append(val)
        assert acc.dtype == np.float32
        avg = (acc + d_ref).astype(np.float64) / (geo_sum + 1).astype(np.float64)
        photo, geo = conf > prob, geo_sum >= int(ncons)
        w = _mul34(rm[18:30], _mul3(rm, x * avg, y * avg, avg))
        res = {k: np.stack(v) for k, v in out.items()}
        res.update({"masks": np.stack([photo, geo, photo & geo]).astype(np.uint8), "depth_avg": avg.astype(F32),
                    "xyz": np.stack(w, -1).astype(F32), "rgb": None, "geo_sum": geo_sum})
        if img is not None:
            img = np.asarray(img)
            assert img.dtype == np.float32 and img.shape == (H, W, 3)
            res["rgb"] = (img * F32(255.0)).astype(np.int32).astype(np.uint8)
    return res


def compact_exact(mask, xyz, rgb=None):
    """numpy's xyz[mask != 0] over the flattened pixels -> (n,3) fp32, (n,3) uint8 or None"""
    keep = np.asarray(mask).reshape(-1) != 0
    return np.asarray(xyz).reshape(-1, 3)[keep], (None if rgb is None else np.asarray(rgb).reshape(-1, 3)[keep])


def equal_exact(got, want):
    """Float arrays: equal in every bit, the sign of zero included, with NaN exactly where `want` has NaN (any payload).  Integer and
    byte arrays: equal."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if want.dtype.kind != "f":
        return bool(np.array_equal(got, want))
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    u = {4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
    return bool(np.array_equal(np.ascontiguousarray(got).view(u)[~nan], np.ascontiguousarray(want).view(u)[~nan]))


def first_differences(got, want, limit=5):
    """the indices, and both values, of the first few places where equal_exact fails: for the message of a failed assert"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"shape / dtype {got.shape} {got.dtype} against {want.shape} {want.dtype}"
    if want.dtype.kind == "f":
        u = {4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
        bad = np.where(np.isnan(want), ~np.isnan(got), np.ascontiguousarray(got).view(u) != np.ascontiguousarray(want).view(u))
    else:
        bad = got != want
    at = np.argwhere(bad)
    return f"{len(at)} differ; first at " + "; ".join(f"{tuple(i)}: got {got[tuple(i)]!r} want {want[tuple(i)]!r}" for i in at[:limit])
