"""The cases and checks of the depth-map fusion kernels (csrc/fusion.hip: rcmvs_fuse_view, rcmvs_compact_points), shared by
tests/test_gpu_fusion.py (device "cuda:0") and tests/test_fusion_emu_cpu.py (the CPU emulation, device "cpu"), against
tests/fusion_oracle.py.  Every comparison with the oracle is FO.equal_exact: floats equal in every bit with the sign of zero, NaN
exactly where the oracle has NaN, bytes and integers equal -- at every pixel, with no allowance for flipped masks.  Every case first
asserts ON THE ORACLE ALONE that it holds what it is named for (case_asserts), so that none can pass vacuously; tests/test_fusion_cpu.py
runs the same cases through the g++ loop harness.

The kernels are called through the C entry points with every output buffer pre-filled (FILL), so that an element the kernel did
not write shows; the Python wrappers (fusion.fuse_view, compact_points, filter_depth, filter_depth_tanks) are compared too."""
import ctypes
import functools
import os

import numpy as np
import torch

import fusion_oracle as FO
from oracle import dataset as OD, fusion as OF
from rc_mvsnet_amd import _lib, fusion, scan_io, synthetic

PROB, NCONS, DIST, DEPTH = 0.8, 3, 0.5, 0.01
FILL = {torch.float32: -7.0, torch.uint8: 99, torch.int32: -7}
OUTPUTS = ("masks", "depth_avg", "xyz", "rgb")
DEBUG = ("depth_reprojected", "geo", "xy_src")
NULL = ctypes.c_void_p(0)
F32 = np.float32


def frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


# ---- building cases ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scan(H=20, W=28, seed=9):
    return synthetic.fusion_scan(V=5, H=H, W=W, seed=seed, n_src=4)


def make_case(depth_all, ref, srcs, conf, img, K, E, prob=PROB, ncons=NCONS, dist=DIST, depth_t=DEPTH):
    mats = fusion.fusion_matrices(K[ref], E[ref], [K[i] for i in srcs], [E[i] for i in srcs])
    return {"depth_all": frozen(np.asarray(depth_all, F32)), "ref": int(ref), "srcs": tuple(int(s) for s in srcs), "conf": frozen(np.asarray(conf, F32)),
            "img": None if img is None else frozen(np.asarray(img, F32)), "mats": frozen(mats), "prob": prob, "ncons": ncons, "dist": dist, "depth_t": depth_t}


def scan_case(s=None, pair=0, depth=None, E=None, srcs=None, img="scan", **thresholds):
    s = s or scan()
    ref, own = s["pairs"][pair]
    if isinstance(img, str):
        img = s["img"][ref].astype(F32) / F32(255.0)
    return make_case(s["depth"] if depth is None else depth, ref, own if srcs is None else srcs, s["conf"][ref], img, s["K"], s["E"] if E is None else E, **thresholds)


def oracle(c):
    r = FO.fuse_view_exact(c["depth_all"], c["ref"], c["srcs"], c["conf"], c["img"], c["mats"], c["prob"], c["ncons"], c["dist"], c["depth_t"])
    for v in r.values():
        if v is not None:
            v.setflags(write=False)
    return r


def mixed(r):
    """at least one consistent and one inconsistent pixel for every source view, and kept and dropped pixels in every mask"""
    g = r["geo"].reshape(len(r["geo"]), -1)
    m = r["masks"].reshape(3, -1)
    return bool((g.any(1) & ~g.all(1)).all() and (m.any(1) & ~m.all(1)).all())


# ---- the cases: name -> builder; case_asserts holds what each is named for -------------------------------------------------------------
def _holes():
    s = scan()
    ref, srcs = s["pairs"][0]
    d = s["depth"].copy()
    d[ref, 3:5, 5:11] = 0.0
    d[srcs[0], :, :7] = 0.0
    for k, v in enumerate((np.nan, np.inf, -np.inf, -600.0, 1e-30, 3e38)):
        d[ref, 7:9, 2 + 4 * k:4 + 4 * k] = v
    d[srcs[1], 10:14, 10:16] = np.nan
    d[srcs[2], 12:17, 2:8] = np.inf
    d[srcs[3], 15:19, 18:24] = -np.inf
    return scan_case(depth=d)


def _geometry():
    s = scan()
    ref, srcs = s["pairs"][0]
    E = s["E"].copy()
    E[srcs[1], :3, 3] += np.array([4.0e4, 0.0, 0.0], F32)              # out of frame
    E[srcs[2], 2, 3] -= F32(2000.0)                                    # the surface (z about 650) lies behind this camera
    return scan_case(E=E, ncons=2)


IDENT_H, IDENT_W = 7, 9


def _identity_depths(V, seed):
    """view 0: depth 1 everywhere; the others 1 + k / 128, k in 0..63: every bilinear sample is exact in float32"""
    rng = np.random.default_rng(seed)
    d = np.ones((V, IDENT_H, IDENT_W), F32)
    d[1:] = 1.0 + rng.integers(0, 64, (V - 1, IDENT_H, IDENT_W)) / 128.0
    return d


def _q2_zero():
    """identity intrinsics, depth 1, the source translated by -1 along z: the point's z in the source camera is exactly 0"""
    K = np.broadcast_to(np.eye(3, dtype=F32), (2, 3, 3)).copy()
    E = np.broadcast_to(np.eye(4, dtype=F32), (2, 4, 4)).copy()
    E[1, 2, 3] = -1.0
    conf = np.full((IDENT_H, IDENT_W), 0.9, F32)
    return make_case(_identity_depths(2, 1), 0, [1], conf, None, K, E, ncons=1)


def border_shifts():
    W = IDENT_W
    return (-1.0, -1.0 + 1.0 / 64, -0.5, 0.5, 1.0, 1.0 / 64, 3.0 / 64, W - 1.0, float(W), 1e8, -1e8, 4e7)


def _borders():
    """identity cameras, reference depth 1, source n shifted by (t, t / 2): x_src = x + t and y_src = y + t / 2 exactly"""
    ts = border_shifts()
    V = len(ts) + 1
    K = np.broadcast_to(np.eye(3, dtype=F32), (V, 3, 3)).copy()
    E = np.broadcast_to(np.eye(4, dtype=F32), (V, 4, 4)).copy()
    for n, t in enumerate(ts):
        E[n + 1, 0, 3], E[n + 1, 1, 3] = t, t / 2
    conf = (0.55 + 0.45 * np.random.default_rng(3).random((IDENT_H, IDENT_W))).astype(F32)
    img = np.random.default_rng(4).random((IDENT_H, IDENT_W, 3)).astype(F32)
    return make_case(_identity_depths(V, 2), 0, list(range(1, V)), conf, img, K, E, ncons=2, dist=0.25, depth_t=0.3)


@functools.lru_cache(maxsize=None)
def knife_pixel(which):
    """A pixel of the friendly scan at which source 0 is consistent with dist > 0 and rel > 0, exactly num_consistent sources are (the geo
    mask follows each of them), and source 0 has the largest dist (which == "dist") or rel ("depth") of them, so that a threshold one
    ulp above its value keeps the others: (y, x, dist fp64, rel fp32, conf fp32)"""
    c = scan_case()
    r = oracle(c)
    ok = (r["geo"][0] == 1) & (r["dist"][0] > 0) & (r["rel"][0] > 0) & (r["geo_sum"] == c["ncons"])
    for key in {"dist": ("dist",), "depth": ("rel",), "prob": ()}[which]:
        ok &= r[key][0] == np.where(r["geo"] == 1, r[key], -np.inf).max(0)
    y, x = np.argwhere(ok)[0]
    return int(y), int(x), r["dist"][0, y, x], r["rel"][0, y, x], c["conf"][y, x]


def _knife(which, side):
    y, x, dist, rel, conf = knife_pixel(which)
    if which == "dist":
        return scan_case(dist=float(dist if side == "at" else np.nextafter(dist, np.inf)))
    if which == "depth":
        return scan_case(depth_t=float(rel if side == "at" else np.nextafter(rel, F32(np.inf))))
    return scan_case(prob=float(conf if side == "at" else np.nextafter(conf, F32(-np.inf))))


def _colour():
    """all 256 levels k / 255, 0.0 and 1.0, the float32 just below each level, then random values below 1"""
    s = scan()
    levels = np.arange(256, dtype=F32) / F32(255.0)
    vals = np.concatenate([levels, [0.0, 1.0], np.nextafter(levels[1:], F32(0.0)), np.arange(256) / 255.0]).astype(F32)
    img = np.random.default_rng(5).random(20 * 28 * 3).astype(F32)
    img[:len(vals)] = vals
    return scan_case(img=img.reshape(20, 28, 3))


def _self_source():
    s = scan()
    ref, srcs = s["pairs"][0]
    return scan_case(srcs=[ref] + srcs[:2])


SHAPES = ((1, 1), (1, 300), (300, 1), (3, 257), (16, 16), (1, 257))

CASES = {
    "friendly": scan_case,
    "friendly_no_img": lambda: scan_case(img=None),
    "friendly_pair_3": lambda: scan_case(pair=3),
    "holes": _holes,
    "geometry": _geometry,
    "q2_zero": _q2_zero,
    "borders": _borders,
    "colour": _colour,
    "one_source": lambda: scan_case(srcs=scan()["pairs"][0][1][:1], ncons=1),
    "sixteen_sources": lambda: scan_case(srcs=(scan()["pairs"][0][1] * 4)[:16], ncons=9),
    "self_source": _self_source,
    "ncons_0": lambda: dict(_holes(), ncons=0),
    "ncons_N": lambda: scan_case(ncons=4),
    "ncons_N_plus_1": lambda: scan_case(ncons=5),
}
for _which in ("dist", "depth", "prob"):
    for _side in ("at", "past"):
        CASES[f"knife_{_which}_{_side}"] = functools.partial(_knife, _which, _side)
for _H, _W in SHAPES:
    CASES[f"shape_{_H}x{_W}"] = functools.partial(lambda H, W: scan_case(scan(H, W)), _H, _W)

GROUPS = {
    "friendly": ("friendly", "friendly_no_img", "friendly_pair_3"),
    "holes": ("holes",),
    "geometry": ("geometry", "q2_zero"),
    "borders": ("borders",),
    "knife": tuple(n for n in CASES if n.startswith("knife_")),
    "counts": ("one_source", "sixteen_sources", "self_source", "ncons_0", "ncons_N", "ncons_N_plus_1"),
    "shapes": tuple(n for n in CASES if n.startswith("shape_")),
    "colour": ("colour",),
}
assert sorted(n for g in GROUPS.values() for n in g) == sorted(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    r = oracle(case(name))
    case_asserts(name, case(name), r)
    return r


def case_asserts(name, c, r):
    """what the case is named for, on the oracle alone"""
    d_ref = c["depth_all"][c["ref"]]
    N, (H, W) = len(c["srcs"]), d_ref.shape
    geo, masks = r["geo"], r["masks"]
    assert np.array_equal(masks[2], masks[0] & masks[1]) and np.array_equal(r["geo_sum"], geo.sum(0)), name
    assert np.array_equal(r["depth_reprojected"] != 0, geo == 1) or name in ("holes", "ncons_0"), name
    if name.startswith("friendly") or name.startswith("ncons_N") or name in ("one_source", "sixteen_sources", "colour"):
        assert np.isfinite(r["xyz"]).all() and (d_ref > 0).all()
    if name.startswith("friendly") or name in ("one_source", "sixteen_sources", "colour", "holes", "ncons_N"):
        assert mixed(r), name
    if name == "friendly_no_img":
        assert r["rgb"] is None
    if name == "holes":
        assert not masks[1][3:5, 5:11].any() and not geo[:, 3:5, 5:11].any()                       # a hole in the reference map: 0 / 0 in the relative test
        avg = r["depth_avg"][7:9]
        assert np.isnan(avg[:, 2:4]).all() and np.isnan(r["xyz"][7:9, 2:4]).all()                    # NaN reference depth
        assert np.isposinf(avg[:, 6:8]).all() and np.isneginf(avg[:, 10:12]).all()                   # +Inf, -Inf
        assert not geo[:, 7:9, 2:4].any() and not geo[:, 7:9, 6:8].any() and not geo[:, 7:9, 10:12].any()
        assert np.isfinite(avg[:, 14:16]).all() and (avg[:, 18:20] > 0).all() and (avg[:, 22:24] > 1e37).all() and (r["xyz"][7:9, 22:24, 2] > 1e37).all()   # -600, 1e-30, 3e38
        for n, (y0, y1, x0, x1) in enumerate(((0, H, 0, 7), (10, 14, 10, 16), (12, 17, 2, 8), (15, 19, 18, 24))):      # the patches of the four sources
            ix, iy = r["ix"][n], r["iy"][n]
            fully = (ix >= x0) & (ix + 1 < x1) & (iy >= y0) & (iy + 1 < y1)                        # all four taps in the patch
            assert fully.sum() >= 1 and not geo[n][fully].any(), (name, n, int(fully.sum()))
    if name == "geometry":
        ix = r["ix"][1]
        assert ((ix == FO.FAR) | (ix >= W) | (ix < -1)).all() and not geo[1].any()                  # out of frame
        assert (r["z_src"][2] < 0).all() and (r["z_src"][[0, 1, 3]] > 0).all()                      # behind the camera
        assert geo[0].any() and geo[3].any() and masks[1].any() and not masks[1].all()
    if name == "q2_zero":
        assert (r["z_src"] == 0).all() and not np.isfinite(r["xy_src"]).any() and np.isnan(r["xy_src"][0, 0, 0, 0]) and np.isposinf(r["xy_src"][0, 0, 1, 0])
        assert (r["ix"] == FO.FAR).all() and not geo.any() and (r["depth_avg"] == 1).all()
    if name == "borders":
        ts = border_shifts()
        y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        for n, t in enumerate(ts):
            assert np.array_equal(r["xy_src"][n, ..., 0], (x + t).astype(F32)) and np.array_equal(r["xy_src"][n, ..., 1], (y + t / 2).astype(F32)), t
        ix, iy = r["ix"], r["iy"]
        at = {t: n for n, t in enumerate(ts)}
        assert (ix[at[-1.0]][:, 0] == -1).all() and (ix[at[-0.5]][:, 0] == -1).all() and (iy[at[-1.0]][0] == -1).all()      # the left and the top tap outside
        assert (ix[at[-1.0 + 1.0 / 64]][:, 0] == -1).all()                                          # -31.5 rounds to the even -32
        for t, frac in ((1.0 / 64, 0), (3.0 / 64, 2), (-1.0 + 1.0 / 64, 0)):                        # ties of the 1/32 rounding go to the even side
            fx = r["xy_src"][at[t], ..., 0] * F32(32.0)
            assert (fx - np.floor(fx) == 0.5).all() and (np.rint(fx).astype(np.int64) & 31 == frac).all(), t
        assert (ix[at[W - 1.0]][:, 0] == W - 1).all() and (ix[at[float(W)]][:, 0] == W).all() and not geo[at[float(W)]].any()
        assert (iy[at[W - 1.0]] >= H - 3).all() and (iy[at[W - 1.0]][3:] >= H).all()                # x and y edges at once
        for t in (1e8, -1e8, 4e7):
            assert (ix[at[t]] == FO.FAR).all() and not geo[at[t]].any()
        assert geo.any() and masks[1].any() and not masks[1].all() and masks[2].any()
        for t in (-1.0, -0.5, 0.5, 1.0, 1.0 / 64, 3.0 / 64):
            assert geo[at[t]].any() and not geo[at[t]].all(), t
    if name.startswith("knife_"):
        which, side = name.split("_")[1:]
        y, x, dist, rel, conf = knife_pixel(which)
        want = 0 if side == "at" else 1                                                             # strict <, strict >
        if which == "prob":
            assert r["masks"][0, y, x] == want and r["masks"][1, y, x] == 1 and F32(c["prob"]) == (conf if side == "at" else np.nextafter(conf, F32(-np.inf)))
        else:
            assert geo[0, y, x] == want and r["masks"][1, y, x] == want, name
            assert r["dist"][0, y, x] == dist and r["rel"][0, y, x] == rel
            assert (c["dist"] == dist) if (which, side) == ("dist", "at") else (c["dist"] > dist)
            assert (F32(c["depth_t"]) == rel) if (which, side) == ("depth", "at") else (F32(c["depth_t"]) > rel)
    if name == "one_source":
        assert N == 1
    if name == "sixteen_sources":
        assert N == 16 == fusion.MAX_SRC and np.array_equal(geo[:4], geo[12:]) and int(r["geo_sum"].max()) == 16
    if name == "self_source":
        assert c["srcs"][0] == c["ref"] and np.isfinite(d_ref).all() and geo[0].all()               # every finite pixel is consistent with itself
    if name == "ncons_0":
        assert masks[1].all() and np.isnan(r["depth_avg"]).any() and np.array_equal(masks[2], masks[0])
    if name == "ncons_N":
        assert c["ncons"] == N
    if name == "ncons_N_plus_1":
        assert c["ncons"] == N + 1 and not masks[1].any() and not masks[2].any() and geo.any()
    if name.startswith("shape_"):
        assert f"shape_{H}x{W}" == name and np.isfinite(r["xyz"]).all() and r["xyz"][-1, -1].all() and r["rgb"][-1, -1].any()
        blocks = (H * W + 255) // 256
        assert blocks == {1: 1, 300: 2, 771: 4, 256: 1, 257: 2}[H * W]
    if name == "colour":
        flat, b = c["img"].reshape(-1), r["rgb"].reshape(-1)
        assert np.array_equal(flat[:256], np.arange(256, dtype=F32) / F32(255.0)) and flat[256] == 0.0 and flat[257] == 1.0
        assert b[256] == 0 and b[257] == 255 and b[0] == 0 and b[255] == 255 and c["img"].min() == 0.0 and c["img"].max() == 1.0
        assert np.array_equal(b[258:513], np.arange(255))                                           # just below level k: k - 1
        level = b[:256].astype(int) - np.arange(256)
        print(f"colour: {int((level == 0).sum())} of the 256 levels k / 255 give the byte k, {int((level == -1).sum())} give k - 1")
        assert ((level == 0) | (level == -1)).all() and len(set(b.tolist())) == 256


# ---- running the kernel --------------------------------------------------------------------------------------------------------------
def host(t):
    return None if t is None else t.cpu().numpy()


def to_dev(dev, a):
    return torch.from_numpy(np.array(a)).to(dev)


def filled(shape, dtype, dev):
    return torch.full(shape, FILL[dtype], dtype=dtype).to(dev)


def fuse_args(dev, c, debug=True, with_img=None):
    """device inputs, pre-filled device outputs and the argument list of rcmvs_fuse_view"""
    V, H, W = c["depth_all"].shape
    N = len(c["srcs"])
    has_img = (c["img"] is not None) if with_img is None else with_img
    t = {"depth_all": to_dev(dev, c["depth_all"]), "conf": to_dev(dev, c["conf"]), "mats": to_dev(dev, c["mats"]),
         "img": to_dev(dev, c["img"]) if has_img else None}
    o = {"masks": filled((3, H, W), torch.uint8, dev), "depth_avg": filled((H, W), torch.float32, dev), "xyz": filled((H, W, 3), torch.float32, dev),
         "rgb": filled((H, W, 3), torch.uint8, dev) if has_img else None,
         "depth_reprojected": filled((N, H, W), torch.float32, dev) if debug else None, "geo": filled((N, H, W), torch.uint8, dev) if debug else None,
         "xy_src": filled((N, H, W, 2), torch.float32, dev) if debug else None}
    p = lambda x, dtype=torch.float32: NULL if x is None else fusion._chk(x, "tensor", dtype)      # noqa: E731
    idx = (ctypes.c_int * max(N, 1))(*c["srcs"])
    a = {"depth_all": p(t["depth_all"]), "ref": c["ref"], "idx": ctypes.cast(idx, ctypes.c_void_p), "conf": p(t["conf"]), "img": p(t["img"]),
         "mats": p(t["mats"], torch.float64), "prob": float(c["prob"]), "ncons": int(c["ncons"]), "dist": float(c["dist"]), "depth_t": float(c["depth_t"]),
         "masks": p(o["masks"], torch.uint8), "depth_avg": p(o["depth_avg"]), "xyz": p(o["xyz"]), "rgb": p(o["rgb"], torch.uint8),
         "dbg_d": p(o["depth_reprojected"]), "dbg_g": p(o["geo"], torch.uint8), "dbg_xy": p(o["xy_src"]), "N": N, "H": H, "W": W}
    return t, o, a, idx


FUSE_ORDER = ("depth_all", "ref", "idx", "conf", "img", "mats", "prob", "ncons", "dist", "depth_t", "masks", "depth_avg", "xyz", "rgb", "dbg_d", "dbg_g", "dbg_xy",
              "N", "H", "W")


def call_fuse(a):
    _lib.call("rcmvs_fuse_view", *[a[k] for k in FUSE_ORDER], fusion._stream())


def run(dev, c, debug=True):
    """rcmvs_fuse_view on pre-filled buffers -> host arrays (None for the outputs not asked for)"""
    t, o, a, idx = fuse_args(dev, c, debug)
    call_fuse(a)
    return {k: host(v) for k, v in o.items()}


def run_wrapper(dev, c, debug=True):
    t = lambda a: None if a is None else to_dev(dev, a)                                              # noqa: E731
    r = fusion.fuse_view(t(c["depth_all"]), c["ref"], list(c["srcs"]), t(c["conf"]), t(c["img"]), t(c["mats"]), c["prob"], c["ncons"], c["dist"], c["depth_t"], debug=debug)
    return {k: host(v) for k, v in r.items()}


def assert_outputs(got, want, what, keys=OUTPUTS + DEBUG):
    for k in keys:
        if want[k] is None:
            assert got[k] is None, (what, k)
            continue
        ok = FO.equal_exact(got[k], want[k])
        if not ok:
            print(what, k, FO.first_differences(got[k], want[k]))
        assert ok, (what, k)


def check_case(dev, name):
    want = reference(name)
    assert_outputs(run(dev, case(name)), want, name)


def check_group(dev, group):
    for name in GROUPS[group]:
        check_case(dev, name)


def check_friendly(dev):
    """the friendly scan with img and without, through the entry point and through fusion.fuse_view, with debug=True and without:
    the non-debug outputs are the oracle's either way, and nothing is written to outputs that were not asked for"""
    check_group(dev, "friendly")
    for name in GROUPS["friendly"]:
        want = reference(name)
        plain = run(dev, case(name), debug=False)
        assert_outputs(plain, want, (name, "debug=False"), OUTPUTS)
        assert all(plain[k] is None for k in DEBUG)
        for debug in (False, True):
            got = run_wrapper(dev, case(name), debug)
            assert_outputs(got, want, (name, "fuse_view", debug), OUTPUTS + (DEBUG if debug else ()))
            assert debug or not any(k in got for k in DEBUG)
    c = case("friendly")                                                 # check_geometric_consistency is source 0 of the debug outputs
    s, r = scan(), reference("friendly")
    ref, src = c["ref"], c["srcs"][0]
    m, back, xs, ys = fusion.check_geometric_consistency(s["depth"][ref], s["K"][ref], s["E"][ref], s["depth"][src], s["K"][src], s["E"][src], DIST, DEPTH, device=dev)
    assert m.dtype == bool and np.array_equal(m, r["geo"][0] == 1) and FO.equal_exact(back, r["depth_reprojected"][0])
    assert FO.equal_exact(xs, r["xy_src"][0, ..., 0]) and FO.equal_exact(ys, r["xy_src"][0, ..., 1])


# ---- compaction ----------------------------------------------------------------------------------------------------------------------
BLOCK = 256
# n = 256 b + r elements are b + 1 blocks, the last holding r: one element, all but one, all.  scan_kernel splits the blocks' counts into
# 1024 chunks, of one count up to 1024 blocks (b = 1023) and of two from 1025 (b = 1024); at b = 2048 the last chunks are empty.
COMPACT_SIZES = tuple(BLOCK * b + r for b in (0, 1, 2, 1022, 1023, 1024, 2048) for r in ((1, 256) if b == 2048 else (1, 255, 256)))
COMPACT_LARGEST = tuple(n for n in COMPACT_SIZES if n > BLOCK * 2048)    # the two that the emulation keeps for RCMVS_EMU_FULL=1
COMPACT_MAX = max(COMPACT_SIZES)
MASKS = ("ones", "zeros", "first", "last", "lane_0", "lane_63", "alternate_waves", "alternate_blocks", "random", "bytes_2_255")


def compact_mask(kind, n):
    i = np.arange(n)
    if kind == "random":
        return (np.random.default_rng(n).random(n) < 0.5).astype(np.uint8)
    if kind == "bytes_2_255":
        return np.random.default_rng(n + 1).choice(np.array([0, 2, 255], np.uint8), n)
    m = {"ones": i >= 0, "zeros": i < 0, "first": i == 0, "last": i == n - 1, "lane_0": i % 64 == 0, "lane_63": i % 64 == 63,
         "alternate_waves": (i // 64) % 2 == 0, "alternate_blocks": (i // BLOCK) % 2 == 1}[kind]
    return m.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def compact_source():
    """(COMPACT_MAX, 3) fp32 of random bit patterns (NaNs of every payload, infinities, denormals: a copy must keep them all) and bytes"""
    rng = np.random.default_rng(11)
    xyz = rng.integers(-2 ** 31, 2 ** 31, (COMPACT_MAX, 3), dtype=np.int64).astype(np.int32).view(F32)
    rgb = rng.integers(0, 256, (COMPACT_MAX, 3), dtype=np.int64).astype(np.uint8)
    return frozen(xyz), frozen(rgb)


@functools.lru_cache(maxsize=2)
def compact_source_on(dev):
    xyz, rgb = compact_source()
    return to_dev(dev, xyz), to_dev(dev, rgb)


def compact_blocks(n):
    return (n + BLOCK - 1) // BLOCK


QUICK_MASKS = ("random", "last")                                         # what the emulation runs at the large sizes without RCMVS_EMU_FULL=1


def check_compaction(dev, n, masks=MASKS, both=True):
    """every mask at n elements, with rgb and without (both=False: with rgb for every other mask): the kept rows in order, the rows past
    the kept count untouched, the block offsets the exclusive prefix sums of the blocks' counts and offsets[-1] the count; then the
    Python wrapper"""
    nblk = compact_blocks(n)
    assert n in COMPACT_SIZES
    src_xyz, src_rgb = compact_source()
    all_xyz, all_rgb = compact_source_on(dev)
    xyz, rgb = all_xyz[:n], all_rgb[:n]
    bits = lambda a: np.ascontiguousarray(a).view(np.int32)                                          # noqa: E731
    fill_bits = int(np.array(FILL[torch.float32], F32).view(np.int32))
    for kind in masks:
        mask = compact_mask(kind, n)
        want_xyz, want_rgb = FO.compact_exact(mask, src_xyz[:n], src_rgb[:n])
        kept = len(want_xyz)
        assert kept == {"ones": n, "zeros": 0, "first": 1, "last": 1}.get(kind, kept), (kind, n)
        assert kind in ("zeros", "first", "last", "ones") or n <= 2 * BLOCK or 0 < kept < n, (kind, n)
        if kind == "bytes_2_255":
            assert 1 not in mask and (n < 64 or {0, 2, 255} == set(mask.tolist()))
        counts = np.add.reduceat((mask != 0).astype(np.int64), np.arange(0, n, BLOCK))
        want_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        tm = to_dev(dev, mask)
        for with_rgb in ((True, False) if both else (MASKS.index(kind) % 2 == 0,)):
            out_xyz, out_rgb = filled((n, 3), torch.float32, dev), filled((n, 3), torch.uint8, dev) if with_rgb else None
            offsets = filled((nblk + 1,), torch.int32, dev)
            _lib.call("rcmvs_compact_points", fusion._chk(tm, "mask", torch.uint8), fusion._chk(xyz, "xyz"), fusion._chk(rgb, "rgb", torch.uint8) if with_rgb else NULL,
                      fusion._chk(out_xyz, "out_xyz"), fusion._chk(out_rgb, "out_rgb", torch.uint8) if with_rgb else NULL,
                      fusion._chk(offsets, "offsets", torch.int32), n, fusion._stream())
            what = (kind, n, with_rgb)
            off, gx = host(offsets), bits(host(out_xyz))
            assert int(off[-1]) == kept and np.array_equal(off, want_off), what
            assert np.array_equal(gx[:kept], bits(want_xyz)) and (gx[kept:] == fill_bits).all(), what
            if with_rgb:
                gr = host(out_rgb)
                assert np.array_equal(gr[:kept], want_rgb) and (gr[kept:] == FILL[torch.uint8]).all(), what
        if both and kind in ("random", "bytes_2_255"):
            wx, wr = fusion.compact_points(tm, xyz, rgb)
            assert np.array_equal(bits(host(wx)), bits(want_xyz)) and np.array_equal(host(wr), want_rgb)
            wx, wr = fusion.compact_points(tm, xyz)
            assert wr is None and np.array_equal(bits(host(wx)), bits(want_xyz))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def check_refusals(dev):
    """arguments that the entry points refuse before any launch (the RCMVS_REQUIRE lines of csrc/fusion.hip stand before the launches):
    each with the library's message, and nothing written by a refused call"""
    c = case("friendly")
    t, o, good, idx = fuse_args(dev, c)
    neg = (ctypes.c_int * 4)(c["srcs"][0], -1, c["srcs"][2], c["srcs"][3])
    many = (ctypes.c_int * 17)(*([1] * 17))
    bad = [({"N": 0}, "0 source views"), ({"N": 17, "idx": ctypes.cast(many, ctypes.c_void_p)}, "17 source views"), ({"N": -1}, "-1 source views"),
           ({"ref": -1}, "bad dims"), ({"idx": ctypes.cast(neg, ctypes.c_void_p)}, "negative source index"),
           ({"rgb": NULL}, "img and rgb must be given together"), ({"img": NULL}, "img and rgb must be given together"),
           ({"H": 32768, "W": 32768}, "bad dims"),                       # H * W == 2^30: refused whatever the buffers hold
           ({"H": 0}, "bad dims"), ({"W": 0}, "bad dims"), ({"H": -20}, "bad dims")]
    bad += [({k: NULL}, "null pointer") for k in ("depth_all", "idx", "conf", "mats", "masks", "depth_avg", "xyz")]
    for kw, pattern in bad:
        try:
            call_fuse(dict(good, **kw))
        except _lib.RcmvsError as e:
            assert pattern in str(e), (kw, str(e))
        else:
            raise AssertionError(f"a bad argument was accepted: {kw}")
    for k, v in o.items():
        assert bool((v == FILL[v.dtype]).all()), k
    call_fuse(good)                                                      # and the good arguments are taken
    assert_outputs({k: host(v) for k, v in o.items()}, reference("friendly"), "after the refusals")
    # the wrapper's own refusals
    dt, ct, mt = to_dev(dev, c["depth_all"]), to_dev(dev, c["conf"]), to_dev(dev, c["mats"])
    for call, pattern in ((lambda: fusion.fuse_view(dt, 0, [], ct, None, mt, PROB, NCONS, DIST, DEPTH), "0 source views"),
                          (lambda: fusion.fuse_view(dt, 0, [1] * 17, ct, None, mt, PROB, NCONS, DIST, DEPTH), "17 source views"),
                          (lambda: fusion.fuse_view(dt, 0, [1, 2, 3, 5], ct, None, mt, PROB, NCONS, DIST, DEPTH), "beyond depth_all"),
                          (lambda: fusion.fuse_view(dt, 0, [1, 2, 3], ct, None, mt, PROB, NCONS, DIST, DEPTH), "mats has"),
                          (lambda: fusion.fuse_view(dt, 0, [1, -2, 3, 4], ct, None, mt, PROB, NCONS, DIST, DEPTH), "negative source index"),
                          (lambda: fusion.fuse_view(dt, -1, [1, 2, 3, 4], ct, None, mt, PROB, NCONS, DIST, DEPTH), "bad dims")):
        try:
            call()
        except _lib.RcmvsError as e:
            assert pattern in str(e), (pattern, str(e))
        else:
            raise AssertionError(f"a bad argument was accepted ({pattern})")
    # compaction
    n = 300
    xyz, rgb = (a[:n] for a in compact_source_on(dev))
    tm = to_dev(dev, compact_mask("random", n))
    out_xyz, out_rgb, offsets = filled((n, 3), torch.float32, dev), filled((n, 3), torch.uint8, dev), filled((3,), torch.int32, dev)
    good = {"mask": fusion._chk(tm, "mask", torch.uint8), "xyz": fusion._chk(xyz, "xyz"), "rgb": fusion._chk(rgb, "rgb", torch.uint8), "out_xyz": fusion._chk(out_xyz, "out_xyz"),
            "out_rgb": fusion._chk(out_rgb, "out_rgb", torch.uint8), "offsets": fusion._chk(offsets, "offsets", torch.int32), "n": n}
    bad = [({"n": 0}, "n=0"), ({"n": -1}, "n=-1"), ({"n": 2 ** 31}, "n=2147483648"), ({"rgb": NULL}, "given together"), ({"out_rgb": NULL}, "given together")]
    bad += [({k: NULL}, "null pointer") for k in ("mask", "xyz", "out_xyz", "offsets")]
    for kw, pattern in bad:
        a = dict(good, **kw)
        try:
            _lib.call("rcmvs_compact_points", *[a[k] for k in ("mask", "xyz", "rgb", "out_xyz", "out_rgb", "offsets", "n")], fusion._stream())
        except _lib.RcmvsError as e:
            assert pattern in str(e), (kw, str(e))
        else:
            raise AssertionError(f"a bad argument was accepted: {kw}")
    for v in (out_xyz, out_rgb, offsets):
        assert bool((v == FILL[v.dtype]).all())


# ---- whole scans through the files ---------------------------------------------------------------------------------------------------
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fusion.npz"))


def _read_masks(out_folder, V):
    from PIL import Image
    got = np.zeros((V, 3) + np.array(Image.open(os.path.join(out_folder, "mask", "{:0>8}_final.png".format(0)))).shape, np.uint8)
    for v in range(V):
        for k, kind in enumerate(("photo", "geo", "final")):
            got[v, k] = np.array(Image.open(os.path.join(out_folder, "mask", "{:0>8}_{}.png".format(v, kind)))) > 0
    return got


def _exact_scan(s, imgs, K, prob, ncons, dist, depth_t):
    """the exact oracle over every reference view of a scan -> masks (V,3,H,W), the concatenated kept points and colours"""
    masks, pts, cols = [], [], []
    for ref, srcs in s["pairs"]:
        r = oracle(make_case(s["depth"], ref, srcs, s["conf"][ref], imgs[ref], K, s["E"], prob, ncons, dist, depth_t))
        xyz, rgb = FO.compact_exact(r["masks"][2], r["xyz"], r["rgb"])
        masks.append(r["masks"])
        pts.append(xyz)
        cols.append(rgb)
    return np.stack(masks), np.concatenate(pts), np.concatenate(cols)


def check_filter_depth(dev, tmp_path):
    """filter_depth on the golden-sized scan: every mask PNG is the exact oracle's mask and the PLY holds its compacted points, byte for byte"""
    V, H, W, seed, n_src = [int(x) for x in GOLD["dims"]]
    s = synthetic.fusion_scan(V=V, H=H, W=W, seed=seed, n_src=n_src)
    pair_folder, out_folder = str(tmp_path / "data" / "scan1"), str(tmp_path / "out" / "scan1")
    synthetic.write_fusion_scan(s, pair_folder, out_folder)
    imgs = [scan_io.read_img(os.path.join(out_folder, "images", "{:0>8}.jpg".format(v))) for v in range(V)]
    assert imgs[0].dtype == np.float32 and np.array_equal(imgs[1], s["img"][1].astype(F32) / F32(255.0))
    masks, want_xyz, want_rgb = _exact_scan(s, imgs, s["K"], PROB, NCONS, DIST, DEPTH)
    assert 0 < len(want_xyz) < V * H * W and all(m.any() and not m.all() for m in masks.reshape(V * 3, -1))
    ply = str(tmp_path / "out" / "fused.ply")
    xyz, rgb = fusion.filter_depth(pair_folder, out_folder, out_folder, ply, PROB, NCONS, DIST, DEPTH, device=dev, verbose=False)
    assert np.array_equal(_read_masks(out_folder, V), masks)
    assert FO.equal_exact(xyz, want_xyz) and np.array_equal(rgb, want_rgb)
    with open(ply, "rb") as f:
        assert f.read() == OF.ply_bytes(want_xyz, want_rgb)


def check_filter_depth_tanks(dev, tmp_path):
    """filter_depth_tanks: masks and xyz bit-equal to the exact oracle; the colour within 1 level of the oracle's on the image resized by
    oracle/dataset.resize_linear (the resize is another kernel, with tests of its own)"""
    V, h, w, oh, ow, seed, n_src = [int(x) for x in GOLD["tanks:dims"]]
    pix, dth, photo, ncons = [float(x) for x in GOLD["tanks:thresholds"]]
    s = synthetic.tanks_fusion_scan(V=V, hw=(h, w), orig_hw=(oh, ow), seed=seed, n_src=n_src)
    scan_folder, out_folder = str(tmp_path / "tt" / "intermediate" / "Horse"), str(tmp_path / "out" / "Horse")
    synthetic.write_tanks_fusion_scan(s, scan_folder, out_folder)
    K = s["K"].copy()                                                    # float32 rows scaled by python floats, as the driver and the reference do
    K[:, 0] *= w / ow
    K[:, 1] *= h / oh
    imgs = [OD.resize_linear(s["img"][v].astype(F32) / F32(255.0), (w, h)) for v in range(V)]
    masks, want_xyz, want_rgb = _exact_scan(s, imgs, K, photo, int(ncons), pix, dth)
    assert 0 < len(want_xyz) < V * h * w
    ply = str(tmp_path / "ply" / "Horse.ply")
    xyz, rgb = fusion.filter_depth_tanks(scan_folder, out_folder, ply, pix, dth, photo, (w, h), (ow, oh), int(ncons), V, "Horse", device=dev, verbose=False)
    assert np.array_equal(_read_masks(out_folder, V), masks)
    assert FO.equal_exact(xyz, want_xyz)
    off = np.abs(rgb.astype(int) - want_rgb.astype(int))
    print(f"tanks colour: {int((off > 0).sum())} of {off.size} bytes differ from the oracle's resize, by at most {int(off.max())}")
    assert off.max() <= 1
    with open(ply, "rb") as f:
        assert f.read() == OF.ply_bytes(want_xyz, rgb)
