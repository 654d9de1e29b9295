"""The exact oracle of the dynamic depth-map fusion kernel (csrc/fusion_dyn.hip: rcmvs_fuse_view_dyn): vectorised numpy that restates
the per-pixel rule of csrc/fusion_dyn_math.h without calling it or the kernel, so that every output -- the `used` array included --
can be compared in every bit at every pixel.

The rule.  The chain of one (reference pixel, source view) pair up to dist (fp64), rel (fp32), d_rep, x_src and y_src is the one
tests/fusion_oracle.py states: float64, every product and sum one rounded operation taken left to right, the float32 cast points
the reference's, the source depth sampled as cv2.remap(INTER_LINEAR) does.  Then, with level_lo <= level_hi, dist_base (fp64) and
rel_base (fp32): source i passes level n when dist_i < float64(n) * dist_base and rel_i < float32(n) * rel_base (each product
rounded once, comparisons with NaN false); count_n = sources that pass level n; level = the smallest n of [level_lo, level_hi] with
count_n >= n, 0 for none; geo = level != 0.  acc = the float32 sequential sum from 0 of d_rep over the sources that pass level_hi (a
failing source adds 0), avg = float64(acc + d_ref) / float64(count_hi + 1); world point and colour bytes as in the fixed filter.
With a `used` array (V,H,W) uint8 and reference view r: claimed = photo & geo & (used[r] != 0), final = photo & geo & ~claimed; a
final pixel stores 1 at used[src_i][my, mx], mx = rint(x_src), my = rint(y_src) (ties to even), for every source i that passes
level_hi, with src_i != r, whose position passes remap's far guard (|32 x| < 1e9 in float32, not NaN) and lies in the image.  The
marks of a view are written after all of its reads: the launch reads plane r only and writes other planes only."""
import numpy as np

from fusion_oracle import REF_MATS, SRC_MATS, _mul3, _mul34, equal_exact, remap_exact   # noqa: F401  (equal_exact: for the cases)

F32 = np.float32
MAX_LEVEL = 16


def fuse_view_dyn_exact(depth_all, ref, srcs, conf, img, mats, prob, level_lo, level_hi, dist_base, rel_base, used=None):
    """depth_all (V,H,W) fp32, ref / srcs view numbers, conf (H,W) fp32, img (H,W,3) fp32 or None, mats the float64 vector of
    fusion.fusion_matrices; prob and rel_base are rounded to float32, dist_base stays float64.  used: (V,H,W) uint8 or None; it is NOT
    modified, the array after the launch is returned as "used".  Returns at ALL pixels masks (4,H,W) uint8 [photo, geo, final, claimed],
    level (H,W) uint8, depth_avg, xyz, rgb or None, the debug outputs depth_reprojected (N,H,W), src_level (N,H,W) uint8, xy_src
    (N,H,W,2), and dist (N,H,W) fp64, rel (N,H,W) fp32, passes (N,16,H,W) bool (source i passes level n + 1; False outside
    [level_lo, level_hi]), counts (16,H,W) int32, count_hi, and marks: the list of (source view, my, mx, y, x) -- the byte stored and the reference pixel that
    stored it -- duplicates kept."""
    depth_all, conf, mats = np.asarray(depth_all), np.asarray(conf), np.asarray(mats)
    assert depth_all.dtype == np.float32 and conf.dtype == np.float32 and mats.dtype == np.float64
    V, H, W = depth_all.shape
    N = len(srcs)
    assert mats.shape == (REF_MATS + SRC_MATS * N,) and conf.shape == (H, W) and 1 <= level_lo <= level_hi <= MAX_LEVEL
    prob, rel_base, dist_base = F32(prob), F32(rel_base), np.float64(dist_base)
    rm = mats[:REF_MATS]
    yi, xi = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x, y = xi.astype(np.float64), yi.astype(np.float64)
    d_ref = depth_all[ref]
    d = d_ref.astype(np.float64)
    out = {k: [] for k in ("depth_reprojected", "src_level", "xy_src", "dist", "rel", "passes")}
    counts = np.zeros((MAX_LEVEL, H, W), np.int32)
    acc = np.zeros((H, W), np.float32)
    pass_hi = []
    with np.errstate(all="ignore"):
        dist_t = [np.float64(n) * dist_base for n in range(1, MAX_LEVEL + 1)]
        rel_t = [F32(n) * rel_base for n in range(1, MAX_LEVEL + 1)]
        assert all(t.dtype == np.float32 for t in rel_t)
        p_ref = _mul3(rm, x * d, y * d, d)
        for n, s in enumerate(srcs):
            sm = mats[REF_MATS + n * SRC_MATS:REF_MATS + (n + 1) * SRC_MATS]
            q = _mul34(sm, p_ref)
            k = _mul3(sm[12:21], q[0], q[1], q[2])
            xs, ys = k[0] / k[2], k[1] / k[2]
            x_src, y_src = xs.astype(F32), ys.astype(F32)
            sampled, _, _ = remap_exact(depth_all[s], x_src, y_src)
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
            passes = np.stack([(dist < dist_t[m - 1]) & (rel < rel_t[m - 1]) if level_lo <= m <= level_hi else np.zeros((H, W), bool)
                               for m in range(1, MAX_LEVEL + 1)])
            counts = counts + passes.astype(np.int32)
            first = np.zeros((H, W), np.uint8)
            for m in range(MAX_LEVEL, 0, -1):
                first = np.where(passes[m - 1], np.uint8(m), first)
            hi = passes[level_hi - 1]
            depth = np.where(hi, d_rep, F32(0.0))
            acc = acc + depth
            pass_hi.append(hi)
            for key, val in (("depth_reprojected", depth), ("src_level", first), ("xy_src", np.stack([x_src, y_src], -1)), ("dist", dist),
                             ("rel", rel), ("passes", passes)):
                out[key].append(val)
        assert acc.dtype == np.float32
        count_hi = counts[level_hi - 1]
        avg = (acc + d_ref).astype(np.float64) / (count_hi + 1).astype(np.float64)
        level = np.zeros((H, W), np.uint8)
        for m in range(level_hi, level_lo - 1, -1):
            level = np.where(counts[m - 1] >= m, np.uint8(m), level)
        photo, geo = conf > prob, level != 0
        claimed = photo & geo & (np.asarray(used)[ref] != 0) if used is not None else np.zeros((H, W), bool)
        final = photo & geo & ~claimed
        w = _mul34(rm[18:30], _mul3(rm, x * avg, y * avg, avg))
        res = {k: np.stack(v) for k, v in out.items()}
        res.update({"masks": np.stack([photo, geo, final, claimed]).astype(np.uint8), "level": level, "depth_avg": avg.astype(F32),
                    "xyz": np.stack(w, -1).astype(F32), "rgb": None, "counts": counts, "count_hi": count_hi, "used": None, "marks": []})
        if img is not None:
            img = np.asarray(img)
            assert img.dtype == np.float32 and img.shape == (H, W, 3)
            res["rgb"] = (img * F32(255.0)).astype(np.int32).astype(np.uint8)
        if used is not None:
            after = np.array(used, np.uint8)
            assert after.shape == (V, H, W)
            for n, s in enumerate(srcs):
                if s == ref:
                    continue
                xf, yf = res["xy_src"][n, ..., 0], res["xy_src"][n, ..., 1]
                near = (np.abs(xf * F32(32.0)) < F32(1.0e9)) & (np.abs(yf * F32(32.0)) < F32(1.0e9))
                mx = np.rint(np.where(near, xf, F32(0.0))).astype(np.int64)
                my = np.rint(np.where(near, yf, F32(0.0))).astype(np.int64)
                hit = final & pass_hi[n] & near & (mx >= 0) & (mx < W) & (my >= 0) & (my < H)
                after[s, my[hit], mx[hit]] = 1
                res["marks"] += [(int(s), int(my[a, b]), int(mx[a, b]), int(a), int(b)) for a, b in np.argwhere(hit)]
            res["used"] = after
    return res


def fuse_scan_exact(depth_all, pairs, conf, imgs, mats_of, prob, params_of, dedup=True):
    """The views of a pair.txt in order, with one `used` array for the scan (dedup=False: none).  pairs: [(ref, srcs)]; conf / imgs: indexed by
    view; mats_of(ref, srcs) -> the float64 vector; params_of(n_src) -> (level_lo, level_hi, dist_base, rel_base).
    -> [per view result of fuse_view_dyn_exact], each with "used" the array AFTER that view (None without dedup)."""
    used = np.zeros(np.asarray(depth_all).shape, np.uint8) if dedup else None
    results = []
    for ref, srcs in pairs:
        r = fuse_view_dyn_exact(depth_all, ref, srcs, conf[ref], None if imgs is None else imgs[ref], mats_of(ref, srcs), prob, *params_of(len(srcs)), used=used)
        used = r["used"]
        results.append(r)
    return results
