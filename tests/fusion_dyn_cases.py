"""The cases and checks of the dynamic depth-map fusion kernel (csrc/fusion_dyn.hip: rcmvs_fuse_view_dyn), shared by
tests/test_gpu_fusion_dyn.py (device "cuda:0") and tests/test_fusion_dyn_emu_cpu.py (the CPU emulation, device "cpu"), against
tests/fusion_dyn_oracle.py.  Every comparison with the oracle is equal_exact: floats equal in every bit, bytes equal, at every pixel, with
every output buffer pre-filled -- the whole `used` array included, so that a stray or a missing mark shows.  Every case first asserts
ON THE ORACLE ALONE that it holds what it is named for.  The scans are the builders of tests/fusion_cases.py, reused unchanged."""
import ctypes
import functools
import os

import numpy as np
import torch

import fusion_cases as FC
import fusion_dyn_oracle as DO
from oracle import dataset as OD, fusion as OF
from rc_mvsnet_amd import _lib, fusion, scan_io, synthetic

F32 = np.float32
NULL = FC.NULL
FILL = FC.FILL
DIST_BASE, REL_BASE = fusion.DYN_DEFAULTS["dist_base"], fusion.DYN_DEFAULTS["rel_base"]
OUTPUTS = ("masks", "level", "depth_avg", "xyz", "rgb")
DEBUG = ("depth_reprojected", "src_level", "xy_src")
EXISTING = ("friendly", "friendly_pair_3", "holes", "geometry", "q2_zero", "borders", "one_source", "sixteen_sources", "self_source", "colour") + \
    tuple(f"shape_{H}x{W}" for H, W in FC.SHAPES)


def dyn_case(base, lo=2, hi=None, dist_base=DIST_BASE, rel_base=REL_BASE, used="zeros", **over):
    """a case of tests/fusion_cases.py (its fixed thresholds dropped) plus the four parameters and the `used` array before the launch
    ("zeros": zero-filled, None: a NULL pointer, or the array)"""
    c = {k: base[k] for k in ("depth_all", "ref", "srcs", "conf", "img", "mats", "prob")}
    c.update(over)
    N = len(c["srcs"])
    if isinstance(used, str):
        used = np.zeros(c["depth_all"].shape, np.uint8)
    c.update({"lo": int(lo), "hi": max(N, int(lo)) if hi is None else int(hi), "dist_base": float(dist_base), "rel_base": float(rel_base),
              "used": None if used is None else FC.frozen(np.asarray(used, np.uint8))})
    return c


def oracle(c):
    r = DO.fuse_view_dyn_exact(c["depth_all"], c["ref"], c["srcs"], c["conf"], c["img"], c["mats"], c["prob"], c["lo"], c["hi"], c["dist_base"],
                               c["rel_base"], c["used"])
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def _graded():
    """the sources' depth maps scaled band by band: rows 0-4 untouched, then by 1 + 2.4 / 1300, 1 + 3.4 / 1300 and 1.02, so that the first
    level that four sources pass is 2, 3, 4 and none"""
    s = FC.scan()
    ref, srcs = s["pairs"][0]
    d = s["depth"].copy()
    for rows, f in ((slice(5, 10), 1 + 2.4 / 1300), (slice(10, 15), 1 + 3.4 / 1300), (slice(15, 20), 1.02)):
        for v in srcs:
            d[v, rows] = (d[v, rows].astype(np.float64) * f).astype(F32)
    return dyn_case(FC.scan_case(depth=d))


@functools.lru_cache(maxsize=None)
def knife_pixel(which):
    """A pixel of the friendly scan, under the defaults, whose level is 2 with exactly two sources passing level 2, one of which (source i)
    has the larger dist (which == "dist") or rel ("rel") of the two, both above 0: (y, x, i, dist fp64, rel fp32)"""
    r = reference("friendly")
    p2 = r["passes"][:, 1]
    key = r[which]
    top = np.where(p2, key, -np.inf).max(0)
    for i in range(len(p2)):
        ok = (r["level"] == 2) & (r["counts"][1] == 2) & p2[i] & (key[i] == top) & (r["dist"][i] > 0) & (r["rel"][i] > 0) & ((np.where(p2, key, -np.inf) == top).sum(0) == 1)
        if ok.any():
            y, x = np.argwhere(ok)[0]
            return int(y), int(x), i, r["dist"][i, y, x], r["rel"][i, y, x]
    raise AssertionError("no knife pixel")


def _knife(which, side):
    """level 2's threshold on the pixel's own value (2 * base == value exactly: the strict < fails) and one ulp of the base past it"""
    y, x, i, dist, rel = knife_pixel(which)
    if which == "dist":
        b = dist / np.float64(2.0)
        return dyn_case(FC.case("friendly"), dist_base=float(b if side == "at" else np.nextafter(b, np.inf)))
    b = rel / F32(2.0)
    return dyn_case(FC.case("friendly"), rel_base=float(b if side == "at" else np.nextafter(b, F32(np.inf))))


def _stripes():
    c = FC.case("friendly")
    used = np.zeros(c["depth_all"].shape, np.uint8)
    for k, v in enumerate((0, 1, 2, 255)):
        used[:, :, k::4] = v
    return dyn_case(c, used=used)


def _borders():
    """One level, 2, with thresholds 0.25 pixel and 0.2: loose enough for the shifted sources to pass and mark at their exact .5 positions.
    A position of -0.5 or W - 0.5 rounds INTO the image (ties to even: 0 and, W being odd, W - 1), so the bounds test alone would let it
    mark; it marks nothing because half of its sample lies outside the image, which halves the sampled depth (rel >= 0.25)."""
    return dyn_case(FC.case("borders"), lo=2, hi=2, dist_base=0.125, rel_base=0.1)


def _four_times():
    s = FC.scan()
    ref, srcs = s["pairs"][0]
    return dyn_case(FC.scan_case(srcs=[srcs[0]] * 4))


KNOWN_SHIFTS, KNOWN_H, KNOWN_W = (0, 3, 7, 12), 6, 40


@functools.lru_cache(maxsize=None)
def known_scan():
    """four cameras of focal length 64 look at the plane z = 4, shifted along x by k / 16: pixel x of view k sees lattice column x + k, every
    disparity is an integer and every number of the chain is exact"""
    V = len(KNOWN_SHIFTS)
    K = np.broadcast_to(np.array([[64, 0, 0], [0, 64, 0], [0, 0, 1]], F32), (V, 3, 3)).copy()
    E = np.broadcast_to(np.eye(4, dtype=F32), (V, 4, 4)).copy()
    for v, k in enumerate(KNOWN_SHIFTS):
        E[v, 0, 3] = -k / 16.0
    depth = np.full((V, KNOWN_H, KNOWN_W), 4.0, F32)
    conf = np.full((V, KNOWN_H, KNOWN_W), 0.9, F32)
    pairs = [(v, [u for u in range(V) if u != v]) for v in range(V)]
    return {"K": K, "E": E, "depth": depth, "conf": conf, "pairs": pairs}


CASES = {f"scan_{n}": functools.partial(lambda n: dyn_case(FC.case(n)), n) for n in EXISTING}
CASES.update({
    "friendly": lambda: dyn_case(FC.case("friendly")),                   # == scan_friendly; the name the other cases refer to
    "null_used": lambda: dyn_case(FC.case("friendly"), used=None),
    "no_img_null_used": lambda: dyn_case(FC.case("friendly_no_img"), used=None),
    "graded": _graded,
    "levels_1_1": lambda: dyn_case(FC.case("friendly"), lo=1, hi=1),
    "levels_lo_1": lambda: dyn_case(FC.case("friendly"), lo=1),
    "levels_hi_below_N": lambda: dyn_case(FC.case("friendly"), lo=2, hi=3),
    "levels_hi_above_N": lambda: dyn_case(FC.case("friendly"), lo=3, hi=6, dist_base=1.0, rel_base=0.01),
    "levels_hi_16": lambda: dyn_case(FC.case("sixteen_sources"), lo=2, hi=16),
    "stripes": _stripes,
    "self_source": lambda: dyn_case(FC.case("self_source")),
    "four_times": _four_times,
    "borders": _borders,
})
for _which in ("dist", "rel"):
    for _side in ("at", "past"):
        CASES[f"knife_{_which}_{_side}"] = functools.partial(_knife, _which, _side)

GROUPS = {
    "scans": tuple(n for n in CASES if n.startswith("scan_") and not n.startswith("scan_shape_")),
    "shapes": tuple(n for n in CASES if n.startswith("scan_shape_")),
    "graded": ("graded",),
    "knife": tuple(n for n in CASES if n.startswith("knife_")),
    "levels": tuple(n for n in CASES if n.startswith("levels_")),
    "suppression": ("friendly", "null_used", "no_img_null_used", "stripes", "self_source", "four_times", "borders"),
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


def origins(r):
    return {(y, x) for _, _, _, y, x in r["marks"]}


def case_asserts(name, c, r):
    """what the case is named for, on the oracle alone"""
    N, (V, H, W) = len(c["srcs"]), c["depth_all"].shape
    photo, geo, final, claimed = (r["masks"][k].astype(bool) for k in range(4))
    level, counts = r["level"], r["counts"]
    # the rule's own invariants
    assert np.array_equal(geo, level != 0) and np.array_equal(final, photo & geo & ~claimed) and not (final & claimed).any(), name
    assert ((level == 0) | ((level >= c["lo"]) & (level <= c["hi"]))).all() and (counts[:c["lo"] - 1] == 0).all() and (counts[c["hi"]:] == 0).all(), name
    assert np.array_equal(r["depth_reprojected"] != 0, r["passes"][:, c["hi"] - 1]) or name in ("scan_holes",), name
    assert np.array_equal(r["count_hi"], r["passes"][:, c["hi"] - 1].sum(0)), name
    if c["used"] is None:
        assert r["used"] is None and not r["marks"] and not claimed.any(), name                     # a NULL `used`: nothing claimed
    else:
        before, after = c["used"], r["used"]
        assert np.array_equal(after[c["ref"]], before[c["ref"]]), name                              # the plane the launch reads is never written
        assert all(final[y, x] for y, x in origins(r)) and all(s != c["ref"] and 0 <= my < H and 0 <= mx < W for s, my, mx, _, _ in r["marks"]), name
        changed = np.argwhere(after != before)
        assert {tuple(i) for i in changed} <= {(s, my, mx) for s, my, mx, _, _ in r["marks"]} and all(after[s, my, mx] == 1 for s, my, mx, _, _ in r["marks"]), name
        assert not any(claimed[y, x] or not photo[y, x] for y, x in origins(r)), name               # claimed or photometrically failed: no marks
    if name in ("friendly", "scan_friendly"):
        fixed = FC.reference("friendly")["masks"][1].astype(bool)
        assert (geo & ~fixed).any() and (geo & fixed).any() and r["marks"] and (geo & ~photo).any()  # the dynamic rule keeps what the fixed one drops
        assert len({s for s, *_ in r["marks"]}) == N
    if name == "scan_geometry":
        fixed = FC.reference("geometry")["masks"][1].astype(bool)
        assert (fixed & ~geo).any() and (fixed & geo).any()                                           # ... and drops what the fixed one keeps
    if name == "scan_q2_zero":
        assert not r["marks"] and not np.isfinite(r["xy_src"]).any() and np.isnan(r["xy_src"]).any() and not geo.any()      # NaN / Inf positions mark nothing
    if name == "scan_one_source":
        assert N == 1 and c["hi"] == 2 and not geo.any() and r["passes"][:, 1].any()                 # level 2 of one source: never reached
    if name in ("scan_sixteen_sources", "levels_hi_16"):
        assert N == 16 and c["hi"] == 16 and int(level.max()) > 2 and (level == 2).any()
    if name == "levels_hi_16":
        assert (level == 16).any() or int(level.max()) >= 4
    if name.startswith("scan_shape_"):
        assert (H * W + 255) // 256 == {1: 1, 300: 2, 771: 4, 256: 1, 257: 2}[H * W] and np.isfinite(r["xyz"]).all()
    if name == "graded":
        hist = np.bincount(level.reshape(-1), minlength=5)
        print("graded: level histogram", hist.tolist())
        assert (hist[[0, 2, 3, 4]] > 0).all() and hist[1] == 0, hist
    if name.startswith("knife_"):
        which, side = name.split("_")[1:]
        y, x, i, dist, rel = knife_pixel(which)
        assert r["dist"][i, y, x] == dist and r["rel"][i, y, x] == rel
        if which == "dist":
            assert np.float64(2.0) * np.float64(c["dist_base"]) == (dist if side == "at" else np.nextafter(dist, np.inf))
        else:
            assert F32(2.0) * F32(c["rel_base"]) == (rel if side == "at" else np.nextafter(rel, F32(np.inf)))
        assert bool(r["passes"][i, 1, y, x]) == (side == "past") and (level[y, x] == 2) == (side == "past"), (name, int(level[y, x]))
    if name == "levels_1_1":
        assert set(np.unique(level)) == {0, 1} and np.array_equal(geo, counts[0] >= 1)
    if name == "levels_lo_1":
        assert c["hi"] == N and (level == 1).any() and int(level.max()) <= N
    if name == "levels_hi_below_N":
        assert c["hi"] == 3 < N and int(level.max()) <= 3 and (r["count_hi"] == 4).any()
    if name == "levels_hi_above_N":
        assert c["hi"] == 6 > N and int(level.max()) <= N and (counts[4:6] > 0).any() and (counts[4:6] <= N).all() and (level == 0).any() and geo.any()
    if name == "stripes":
        assert {0, 1, 2, 255} == set(np.unique(c["used"][c["ref"]]))
        for v in (1, 2, 255):                                                                        # any non-zero byte counts as used
            sel = photo & geo & (c["used"][c["ref"]] == v)
            assert sel.any() and claimed[sel].all(), v
        assert not claimed[c["used"][c["ref"]] == 0].any() and final.any() and r["marks"]
    if name == "self_source":
        assert c["srcs"][0] == c["ref"] and r["passes"][0, c["hi"] - 1][final].all() and r["marks"] and all(s != c["ref"] for s, *_ in r["marks"])
    if name == "four_times":
        assert len(set(c["srcs"])) == 1 and {s for s, *_ in r["marks"]} == {c["srcs"][0]} and (r["count_hi"] == 4).any()
        assert len(r["marks"]) == 4 * len(origins(r))                                                # one byte stored four times
        untouched = [v for v in range(V) if v != c["srcs"][0]]
        assert np.array_equal(r["used"][untouched], c["used"][untouched])
    if name == "borders":
        at = {t: n for n, t in enumerate(FC.border_shifts())}
        xs = r["xy_src"][..., 0]
        half = [(s, my, mx, y, x) for s, my, mx, y, x in r["marks"] if s == at[0.5] + 1]              # x_src = x + 0.5, y_src = y + 0.25
        assert half and all(mx % 2 == 0 and mx in (x, x + 1) and my == y for _, my, mx, y, x in half)  # ties go to even
        assert (xs[at[0.5]][:, W - 1] == W - 0.5).all() and (xs[at[-0.5]][:, 0] == -0.5).all()
        for n, col in ((at[0.5], W - 1), (at[-0.5], 0)):                                              # W - 0.5 and -0.5: half outside, inconsistent, no mark
            assert not any(s == n + 1 and x == col for s, _, _, _, x in r["marks"])
        for t in (1e8, -1e8, 4e7):
            assert not any(s == at[t] + 1 for s, *_ in r["marks"])
        assert {s for s, *_ in r["marks"]} >= {at[t] + 1 for t in (-1.0, -0.5, 0.5, 1.0)}


# ---- running the kernel --------------------------------------------------------------------------------------------------------------
ORDER = ("depth_all", "n_views", "ref", "idx", "conf", "img", "mats", "prob", "lo", "hi", "dist_base", "rel_base", "used", "masks", "level", "depth_avg", "xyz",
         "rgb", "dbg_d", "dbg_l", "dbg_xy", "N", "H", "W")


def dyn_args(dev, c, debug=True, used_dev=None):
    """device inputs, pre-filled device outputs and the arguments of rcmvs_fuse_view_dyn.  used_dev: the scan's array already on the device."""
    V, H, W = c["depth_all"].shape
    N = len(c["srcs"])
    has_img = c["img"] is not None
    t = {"depth_all": FC.to_dev(dev, c["depth_all"]), "conf": FC.to_dev(dev, c["conf"]), "mats": FC.to_dev(dev, c["mats"]),
         "img": FC.to_dev(dev, c["img"]) if has_img else None}
    o = {"masks": FC.filled((4, H, W), torch.uint8, dev), "level": FC.filled((H, W), torch.uint8, dev), "depth_avg": FC.filled((H, W), torch.float32, dev),
         "xyz": FC.filled((H, W, 3), torch.float32, dev), "rgb": FC.filled((H, W, 3), torch.uint8, dev) if has_img else None,
         "depth_reprojected": FC.filled((N, H, W), torch.float32, dev) if debug else None, "src_level": FC.filled((N, H, W), torch.uint8, dev) if debug else None,
         "xy_src": FC.filled((N, H, W, 2), torch.float32, dev) if debug else None,
         "used": used_dev if used_dev is not None else (None if c["used"] is None else FC.to_dev(dev, c["used"]))}
    p = lambda x, dtype=torch.float32: NULL if x is None else fusion._chk(x, "tensor", dtype)      # noqa: E731
    idx = (ctypes.c_int * max(N, 1))(*c["srcs"])
    a = {"depth_all": p(t["depth_all"]), "n_views": V, "ref": c["ref"], "idx": ctypes.cast(idx, ctypes.c_void_p), "conf": p(t["conf"]), "img": p(t["img"]),
         "mats": p(t["mats"], torch.float64), "prob": ctypes.c_float(c["prob"]), "lo": c["lo"], "hi": c["hi"], "dist_base": ctypes.c_double(c["dist_base"]),
         "rel_base": ctypes.c_float(c["rel_base"]), "used": p(o["used"], torch.uint8), "masks": p(o["masks"], torch.uint8), "level": p(o["level"], torch.uint8),
         "depth_avg": p(o["depth_avg"]), "xyz": p(o["xyz"]), "rgb": p(o["rgb"], torch.uint8), "dbg_d": p(o["depth_reprojected"]),
         "dbg_l": p(o["src_level"], torch.uint8), "dbg_xy": p(o["xy_src"]), "N": N, "H": H, "W": W}
    return t, o, a, idx


def call_dyn(a):
    _lib.call("rcmvs_fuse_view_dyn", *[a[k] for k in ORDER], fusion._stream())


def run(dev, c, debug=True, used_dev=None):
    t, o, a, idx = dyn_args(dev, c, debug, used_dev)
    call_dyn(a)
    return {k: FC.host(v) for k, v in o.items()}


def run_wrapper(dev, c, debug=True):
    t = lambda a: None if a is None else FC.to_dev(dev, a)                                           # noqa: E731
    used = t(c["used"])
    r = fusion.fuse_view_dynamic(t(c["depth_all"]), c["ref"], list(c["srcs"]), t(c["conf"]), t(c["img"]), t(c["mats"]), c["prob"], c["lo"], c["hi"],
                                 c["dist_base"], c["rel_base"], used=used, debug=debug)
    out = {k: FC.host(v) for k, v in r.items()}
    out["used"] = FC.host(used)
    return out


def assert_outputs(got, want, what, keys=OUTPUTS + DEBUG + ("used",)):
    FC.assert_outputs(got, want, what, keys)


def check_case(dev, name):
    assert_outputs(run(dev, case(name)), reference(name), name)


def check_group(dev, group):
    for name in GROUPS[group]:
        check_case(dev, name)


def check_wrapper(dev):
    """fusion.fuse_view_dynamic with debug and without, with `used` and without: the oracle's outputs, nothing else written; level_hi=None is
    max(N, level_lo)"""
    for name in ("friendly", "null_used", "no_img_null_used", "stripes"):
        want = reference(name)
        plain = run(dev, case(name), debug=False)
        assert_outputs(plain, want, (name, "debug=False"), OUTPUTS + ("used",))
        assert all(plain[k] is None for k in DEBUG)
        for debug in (False, True):
            got = run_wrapper(dev, case(name), debug)
            assert_outputs(got, want, (name, "fuse_view_dynamic", debug), OUTPUTS + ("used",) + (DEBUG if debug else ()))
            assert debug or not any(k in got for k in DEBUG)
    c = case("scan_one_source")
    t = lambda a: FC.to_dev(dev, a)                                                                  # noqa: E731
    r = fusion.fuse_view_dynamic(t(c["depth_all"]), c["ref"], list(c["srcs"]), t(c["conf"]), t(c["img"]), t(c["mats"]), c["prob"])
    assert_outputs({k: FC.host(v) for k, v in r.items()}, reference("scan_one_source"), "defaults", OUTPUTS)


# ---- a whole scan in order -------------------------------------------------------------------------------------------------------------
def scan_oracle(s, imgs, K, prob, dynamic=None, dedup=True, fixed=None):
    """fuse_scan_exact over the pairs of a scan dict.  fixed = (k, dist_t, depth_t): the fixed check as level k (fusion.reference_bases)"""
    def params(n):
        if fixed is not None:
            return (fixed[0], fixed[0]) + fusion.reference_bases(*fixed)
        p = fusion.dynamic_params(dynamic, n)
        return p["level_lo"], p["level_hi"], p["dist_base"], p["rel_base"]
    mats_of = lambda ref, srcs: fusion.fusion_matrices(K[ref], s["E"][ref], [K[i] for i in srcs], [s["E"][i] for i in srcs])      # noqa: E731
    return DO.fuse_scan_exact(s["depth"], s["pairs"], s["conf"], imgs, mats_of, prob, params, dedup)


def compacted(results):
    pts, cols = zip(*[FC.FO.compact_exact(r["masks"][2], r["xyz"], r["rgb"]) for r in results])
    return np.concatenate(pts), (None if cols[0] is None else np.concatenate(cols))


def check_scan_in_order(dev):
    """the five views of the friendly scan, launch by launch, one `used` array on the device: every output and the whole array after every view"""
    s = FC.scan()
    imgs = [s["img"][v].astype(F32) / F32(255.0) for v in range(len(s["depth"]))]
    want = scan_oracle(s, imgs, s["K"], FC.PROB)
    plain = scan_oracle(s, imgs, s["K"], FC.PROB, dedup=False)
    kept, kept_plain = [int(r["masks"][2].sum()) for r in want], [int(r["masks"][2].sum()) for r in plain]
    claimed = [int(r["masks"][3].sum()) for r in want]
    print(f"friendly scan: {sum(kept_plain)} points without suppression, {sum(kept)} with it, {sum(claimed)} claimed")
    assert claimed[0] == 0 and all(c > 0 for c in claimed[1:]) and sum(kept) + sum(claimed) == sum(kept_plain) and kept[0] == kept_plain[0]
    used_dev = FC.to_dev(dev, np.zeros(s["depth"].shape, np.uint8))
    for (ref, srcs), w in zip(s["pairs"], want):
        c = dyn_case(FC.make_case(s["depth"], ref, srcs, s["conf"][ref], imgs[ref], s["K"], s["E"], prob=FC.PROB), used=None)
        got = run(dev, c, used_dev=used_dev)
        assert_outputs(got, w, ("scan in order", ref))


def check_known_answer(dev):
    """the plane seen by four shifted cameras: without suppression every view keeps the columns that two more views see; with it the cloud
    is exactly H points per lattice column seen by at least three views, every z is 4.0f, and no two points are equal"""
    s = known_scan()
    V, H, W = s["depth"].shape
    seen = lambda col: sum(1 for k in KNOWN_SHIFTS if k <= col < k + W)                              # noqa: E731
    cols3 = [col for col in range(max(KNOWN_SHIFTS) + W) if seen(col) >= 3]
    per_view = [H * sum(1 for col in cols3 if k <= col < k + W) for k in KNOWN_SHIFTS]
    for dedup, total in ((False, sum(per_view)), (True, H * len(cols3))):
        want = scan_oracle(s, None, s["K"], 0.8, dedup=dedup)
        for r in want:
            on = r["passes"][:, 1]
            assert (r["dist"][on] == 0).all() and (r["rel"][on] == 0).all()                          # integer disparities: both distances exactly 0
        if not dedup:
            assert [int(r["masks"][2].sum()) for r in want] == per_view
        xyz, _ = compacted(want)
        assert len(xyz) == total and (xyz[:, 2] == F32(4.0)).all(), (dedup, len(xyz), total)
        if dedup:
            assert len(np.unique(xyz, axis=0)) == len(xyz)
            assert sorted(set((xyz[:, 0] * 16).tolist())) == [float(c) for c in cols3]
        used_dev = FC.to_dev(dev, np.zeros(s["depth"].shape, np.uint8)) if dedup else None
        for (ref, srcs), w in zip(s["pairs"], want):
            c = dyn_case(FC.make_case(s["depth"], ref, srcs, s["conf"][ref], None, s["K"], s["E"], prob=0.8), used=None)
            assert_outputs(run(dev, c, used_dev=used_dev), w, ("known answer", dedup, ref))
    assert (sum(per_view), H * len(cols3)) == (816, 216)


def check_large_view(dev):
    """one 296 x 400 view with 4 sources (more than one row of blocks), with marks"""
    s = synthetic.fusion_scan(V=5, H=296, W=400, seed=3, n_src=4)
    ref, srcs = s["pairs"][1]
    c = dyn_case(FC.make_case(s["depth"], ref, srcs, s["conf"][ref], s["img"][ref].astype(F32) / F32(255.0), s["K"], s["E"], prob=FC.PROB))
    want = oracle(c)
    hist = np.bincount(want["level"].reshape(-1), minlength=5)
    assert (hist[[0, 2]] > 0).all() and len(want["marks"]) > 1000 and want["masks"][2].any()
    assert_outputs(run(dev, c), want, "296x400")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def check_refusals(dev):
    """arguments refused before any launch, through the C entry point and through the wrapper: the library's message, and nothing written"""
    c = case("friendly")
    t, o, good, idx = dyn_args(dev, c)
    V = c["depth_all"].shape[0]
    many = (ctypes.c_int * 17)(*([1] * 17))
    neg = (ctypes.c_int * 4)(c["srcs"][0], -1, c["srcs"][2], c["srcs"][3])
    beyond = (ctypes.c_int * 4)(c["srcs"][0], V, c["srcs"][2], c["srcs"][3])
    cast = lambda arr: ctypes.cast(arr, ctypes.c_void_p)                                             # noqa: E731
    bad = [({"N": 0}, "0 source views"), ({"N": 17, "idx": cast(many)}, "17 source views"), ({"N": -1}, "-1 source views"),
           ({"lo": 0}, "levels 0.."), ({"lo": 3, "hi": 2}, "levels 3..2"), ({"hi": 17}, "levels 2..17"), ({"lo": -1, "hi": -1}, "levels -1..-1"),
           ({"ref": -1}, "reference view index -1"), ({"ref": V}, f"reference view index {V}"), ({"idx": cast(neg)}, "source view index -1"),
           ({"idx": cast(beyond)}, f"source view index {V}"), ({"n_views": 1}, "outside the 1 views"), ({"n_views": 0}, "bad dims"),
           ({"rgb": NULL}, "img and rgb must be given together"), ({"img": NULL}, "img and rgb must be given together"),
           ({"H": 32768, "W": 32768}, "bad dims"), ({"H": 0}, "bad dims"), ({"W": 0}, "bad dims"), ({"H": -20}, "bad dims")]
    bad += [({k: NULL}, "null pointer") for k in ("depth_all", "idx", "conf", "mats", "masks", "level", "depth_avg", "xyz")]
    for kw, pattern in bad:
        try:
            call_dyn(dict(good, **kw))
        except _lib.RcmvsError as e:
            assert pattern in str(e), (kw, str(e))
        else:
            raise AssertionError(f"a bad argument was accepted: {kw}")
    for k, v in o.items():
        assert bool((v == (0 if k == "used" else FILL[v.dtype])).all()), k
    call_dyn(good)                                                       # and the good arguments are taken
    assert_outputs({k: FC.host(v) for k, v in o.items()}, reference("friendly"), "after the refusals")
    dt, ct, mt = FC.to_dev(dev, c["depth_all"]), FC.to_dev(dev, c["conf"]), FC.to_dev(dev, c["mats"])
    f = lambda src, ref=0, **kw: (lambda: fusion.fuse_view_dynamic(dt, ref, src, ct, None, mt, FC.PROB, **kw))      # noqa: E731
    for call, pattern in ((f([]), "0 source views"), (f([1] * 17), "17 source views"), (f([1, 2, 3, 5]), "view index outside"), (f([1, -2, 3, 4]), "view index outside"),
                          (f([1, 2, 3, 4], ref=-1), "view index outside"), (f([1, 2, 3, 4], ref=5), "view index outside"), (f([1, 2, 3]), "mats has"),
                          (f([1, 2, 3, 4], level_lo=0), "levels 0.."), (f([1, 2, 3, 4], level_lo=3, level_hi=2), "levels 3..2"),
                          (f([1, 2, 3, 4], level_hi=17), "levels 2..17"), (f([1, 2, 3, 4], used=torch.zeros(2, 2, 2, dtype=torch.uint8)), "used is")):
        try:
            call()
        except _lib.RcmvsError as e:
            assert pattern in str(e), (pattern, str(e))
        else:
            raise AssertionError(f"a bad argument was accepted ({pattern})")


# ---- whole scans through the files ---------------------------------------------------------------------------------------------------
def _read_dir(folder):
    return {n: open(os.path.join(folder, n), "rb").read() for n in sorted(os.listdir(folder))}


def _read_masks(out_folder, V, kinds):
    from PIL import Image
    return np.stack([np.stack([np.array(Image.open(os.path.join(out_folder, "mask", "{:0>8}_{}.png".format(v, kind)))) > 0 for kind in kinds]) for v in range(V)])


MODES = (("dynamic", False), ("dynamic", True), ("reference", True))
DYNAMIC = {"level_lo": 2, "level_hi": 3, "dist_base": 0.3, "rel_base": 0.002}


def _check_modes(s, imgs, K, prob, fixed, run_filter, out_folder, V, colour_slack):
    """run_filter(tag, **kwargs) -> (xyz, rgb, ply bytes): defaults against explicit "reference", then the three other modes against fuse_scan_exact"""
    xyz0, rgb0, ply0 = run_filter("default")
    masks0 = _read_dir(os.path.join(out_folder, "mask"))
    stats = {}
    xyz1, rgb1, ply1 = run_filter("explicit", method="reference", dynamic=None, dedup=False, stats=stats)
    assert ply0 == ply1 and masks0 == _read_dir(os.path.join(out_folder, "mask")) and sorted(masks0) == sorted("{:0>8}_{}.png".format(v, k) for v in range(V) for k in ("photo", "geo", "final"))
    assert stats["kept"] == len(xyz0) and stats["claimed"] == 0 and [v["ref"] for v in stats["views"]] == [ref for ref, _ in s["pairs"]]
    plain_fixed = FC._exact_scan(s, imgs, K, prob, fixed[0], fixed[1], fixed[2])[0][:, 2].astype(bool)
    for method, dedup in MODES:
        dynamic = DYNAMIC if method == "dynamic" else None
        want = scan_oracle(s, imgs, K, prob, dynamic=dynamic, dedup=dedup, fixed=fixed if method == "reference" else None)
        want_xyz, want_rgb = compacted(want)
        assert 0 < len(want_xyz) < s["depth"].size
        stats = {}
        xyz, rgb, ply = run_filter(f"{method}-{dedup}", method=method, dynamic=dynamic, dedup=dedup, stats=stats)
        kinds = ("photo", "geo", "final") + (("claimed",) if dedup else ())
        assert np.array_equal(_read_masks(out_folder, V, kinds), np.stack([r["masks"][:len(kinds)] for r in want]).astype(bool)), (method, dedup)
        assert DO.equal_exact(xyz, want_xyz), (method, dedup)
        off = np.abs(rgb.astype(int) - want_rgb.astype(int))
        assert off.max() <= colour_slack and ply == OF.ply_bytes(want_xyz, rgb), (method, dedup)
        assert stats["views"] == [{"ref": ref, "kept": int(r["masks"][2].sum()), "claimed": int(r["masks"][3].sum())} for (ref, _), r in zip(s["pairs"], want)]
        assert stats["kept"] == len(want_xyz) and stats["claimed"] == sum(int(r["masks"][3].sum()) for r in want) and (stats["claimed"] > 0) == dedup
        if method == "reference":                                        # the fixed rule as one level: what is kept or claimed is what the fixed filter keeps
            both = np.stack([r["masks"][2] | r["masks"][3] for r in want]).astype(bool)
            assert np.array_equal(both, plain_fixed)
            assert stats["kept"] + stats["claimed"] == len(xyz0)


def check_filter_depth(dev, tmp_path):
    V, H, W, seed, n_src = [int(x) for x in FC.GOLD["dims"]]
    s = synthetic.fusion_scan(V=V, H=H, W=W, seed=seed, n_src=n_src)
    pair_folder, out_folder = str(tmp_path / "data" / "scan1"), str(tmp_path / "out" / "scan1")
    synthetic.write_fusion_scan(s, pair_folder, out_folder)
    imgs = [scan_io.read_img(os.path.join(out_folder, "images", "{:0>8}.jpg".format(v))) for v in range(V)]

    def run_filter(tag, **kw):
        import shutil
        shutil.rmtree(os.path.join(out_folder, "mask"), ignore_errors=True)
        ply = str(tmp_path / f"{tag}.ply")
        xyz, rgb = fusion.filter_depth(pair_folder, out_folder, out_folder, ply, FC.PROB, FC.NCONS, FC.DIST, FC.DEPTH, device=dev, verbose=False, **kw)
        return xyz, rgb, open(ply, "rb").read()

    _check_modes(s, imgs, s["K"], FC.PROB, (FC.NCONS, FC.DIST, FC.DEPTH), run_filter, out_folder, V, 0)
    for kw, pattern in (({"method": "fast"}, "fusion method"), ({"dynamic": DYNAMIC}, "method='dynamic' only"),
                        ({"method": "dynamic", "dynamic": {"levels": 2}}, "unknown parameter"),
                        ({"dedup": True, "method": "reference", "num_consistent": 17}, "levels 1..16")):
        args = dict(num_consistent=FC.NCONS)
        args.update(kw)
        k = args.pop("num_consistent")
        try:
            fusion.filter_depth(pair_folder, out_folder, out_folder, str(tmp_path / "bad.ply"), FC.PROB, k, FC.DIST, FC.DEPTH, device=dev, verbose=False, save_masks=False, **args)
        except _lib.RcmvsError as e:
            assert pattern in str(e), (pattern, str(e))
        else:
            raise AssertionError(f"accepted: {kw}")


def check_filter_depth_tanks(dev, tmp_path):
    V, h, w, oh, ow, seed, n_src = [int(x) for x in FC.GOLD["tanks:dims"]]
    pix, dth, photo, ncons = [float(x) for x in FC.GOLD["tanks:thresholds"]]
    s = synthetic.tanks_fusion_scan(V=V, hw=(h, w), orig_hw=(oh, ow), seed=seed, n_src=n_src)
    scan_folder, out_folder = str(tmp_path / "tt" / "intermediate" / "Horse"), str(tmp_path / "out" / "Horse")
    synthetic.write_tanks_fusion_scan(s, scan_folder, out_folder)
    K = s["K"].copy()
    K[:, 0] *= w / ow
    K[:, 1] *= h / oh
    imgs = [OD.resize_linear(s["img"][v].astype(F32) / F32(255.0), (w, h)) for v in range(V)]

    def run_filter(tag, **kw):
        import shutil
        shutil.rmtree(os.path.join(out_folder, "mask"), ignore_errors=True)
        ply = str(tmp_path / "ply" / f"{tag}.ply")
        xyz, rgb = fusion.filter_depth_tanks(scan_folder, out_folder, ply, pix, dth, photo, (w, h), (ow, oh), int(ncons), V, "Horse", device=dev, verbose=False, **kw)
        return xyz, rgb, open(ply, "rb").read()

    _check_modes(s, imgs, K, photo, (int(ncons), pix, dth), run_filter, out_folder, V, 1)
