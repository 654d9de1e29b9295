"""The cases of the point-cloud clean-up (csrc/cloud_knn.hip through rc_mvsnet_amd/cloud_clean.py) and the checks that take a device:
tests/test_gpu_cloud_clean.py runs them on the MI355X, tests/test_cloud_clean_emu_cpu.py on the CPU emulation.  Every output is
compared with tests/cloud_clean_oracle.py in every bit; the known answers and the independent checks (a k-d tree, numpy's eigh) are
asserted on the oracle alone first, so that a failure says which side is wrong.  No cloud has more than 4 097 points (the size that
crosses the 2 048 scan tile and the 256-thread blocks) except the fused scan of the end-to-end checks, whose size the scan decides."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

import cloud_clean_oracle as O
from rc_mvsnet_amd import _lib, cloud_clean as CC, dtu_io, fusion, synthetic

F32 = np.float32
ONE = 1e300                                                       # a cell edge that puts any finite fp32 cloud into one cell
NULL = ctypes.c_void_p(0)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(got, want):
    """equal in every bit; a NaN matches a NaN (its payload is the hardware's)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != "f":
        return bool(np.array_equal(got, want))
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan]))


def _uniform(n, seed):
    return np.random.default_rng(seed).random((n, 3)).astype(F32)


def plane_grid():
    """a 20 x 20 planar grid of spacing 1 at z = 0"""
    g = np.stack(np.meshgrid(np.arange(20.0), np.arange(20.0), indexing="ij"), -1).reshape(-1, 2)
    return np.concatenate([g, np.zeros((400, 1))], 1).astype(F32)


FAR5 = np.array([[3, 3, 40], [10, 10, 45], [15, 5, 50], [5, 15, -40], [10, 3, -60]], F32)
SPHERE_CAMS = 3.0 * np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)


@functools.lru_cache(maxsize=None)
def cloud(name):
    rng = np.random.default_rng(7)
    if name.startswith("u"):
        return _uniform(int(name[1:]), 1000 + int(name[1:]))
    if name.startswith("n"):
        return _uniform(int(name[1:]), 5)
    if name == "dup40":
        return np.tile(np.array([[0.25, -1.5, 3.0]], F32), (40, 1))
    if name == "lattice":
        return np.stack(np.meshgrid(*[np.arange(9.0)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(F32)
    if name == "clusters":
        a = rng.normal(size=(30, 3))
        b = rng.normal(size=(30, 3)) + np.array([1e6, 0, 0])
        lone = np.array([[5e5, 3e5, -2e5], [2.5e5, 0, 0], [-1e5, 1e5, 7e5]])
        return np.concatenate([a, lone[:1], b, lone[1:]]).astype(F32)
    if name == "borders":
        return (rng.integers(0, 9, (300, 3)) * 0.5).astype(F32)
    if name == "zeros":
        v = np.array([-0.0, 0.0, 1.0, -1.0], F32)
        return np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3).copy()
    if name == "huge":
        d = np.float32(1e-45)
        return np.array([[1e30, 0, 0], [-1e30, 1e30, 0], [3.4e38, 0, 0], [-3.4e38, 3.4e38, -3.4e38], [d, 0, 0], [0, 2 * d, 0], [1e-40, 1e-40, -1e-40],
                         [0, 0, 0], [1, 1, 1], [-1, 2, 0.5], [3.4e38, 3.4e38, 3.4e38], [1e30, 1e30, 1e30], [2 * d, 0, 0]], F32)
    if name == "plane":
        return plane_grid()
    if name == "plane_far":
        return np.concatenate([plane_grid(), FAR5])
    if name == "loop":                                            # 40 points, unit spacing, on the boundary of a 10 x 10 square
        t = np.arange(10.0)
        z = np.zeros(10)
        return np.concatenate([np.stack([t, z, z], 1), np.stack([z + 10, t, z], 1), np.stack([10 - t, z + 10, z], 1), np.stack([z, 10 - t, z], 1)]).astype(F32)
    if name == "line":
        t = np.arange(50.0)
        return np.concatenate([np.stack([t, 2 * t, 3 * t], 1), np.stack([t * 0.37, np.full(50, 7.0), np.full(50, -2.0)], 1)]).astype(F32)
    if name == "sphere":
        d = rng.normal(size=(1500, 3))
        return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    raise KeyError(name)


def tiny(name):
    """the small cell edge of a case: the lattice's spacing (every point on a cell border), else 1/48 of the largest extent"""
    if name == "lattice":
        return 1.0
    if name == "borders":
        return 0.5
    p = cloud(name).astype(np.float64)
    ext = float((p.max(0) - p.min(0)).max()) if len(p) else 0.0
    return ext / 48 if ext > 0 else 1.0


def cells(name):
    return (tiny(name), None, ONE)


KNN_CASES = ([("n0", 8), ("n1", 8), ("n2", 8), ("n8", 8), ("n9", 8), ("dup40", 8), ("dup40", 32), ("clusters", 8), ("borders", 8), ("zeros", 8), ("huge", 8)] +
             [("lattice", k) for k in (6, 7, 26, 32)] + [(f"u{n}", k) for n in (255, 256, 257, 2047, 2048, 2049, 4097) for k in (1, 8, 20, 32)])


@functools.lru_cache(maxsize=None)
def reference_knn(name, k):
    return O.knn(cloud(name), k)


def dev_cloud(name, dev):
    return torch.from_numpy(cloud(name).copy()).to(dev)


def _knn(t, k, cell):
    r = CC.knn_device(t, k, cell, want=("idx", "d2", "mean"))
    return tuple(r[key].cpu().numpy() for key in ("idx", "d2", "mean")), r["grid"]


def check_knn(dev, name, k, twice=True):
    """idx, d2 and mean equal the oracle in every bit under the tiny, the default and the single cell; two runs are identical"""
    want = reference_knn(name, k)
    t = dev_cloud(name, dev)
    grids = []
    for cell in cells(name):
        got, grid = _knn(t, k, cell)
        grids.append(grid)
        for g, w, what in zip(got, want, ("idx", "d2", "mean")):
            assert same(g, w), f"{name} k={k} cell={cell}: {what} differs from the oracle"
    if len(t) > 40:
        assert grids[2]["cells"] == 1 and grids[0]["cells"] > grids[1]["cells"] >= 1, grids
    if twice:
        a, b = _knn(t, k, None)[0], _knn(t, k, None)[0]
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def check_knn_outputs(dev):
    """every combination of the nullable outputs gives the same values, and the counters count"""
    name, k = "u2049", 20
    want = dict(zip(("idx", "d2", "mean"), reference_knn(name, k)))
    t = dev_cloud(name, dev)
    for combo in (("mean",), ("idx",), ("d2",), ("idx", "mean"), ()):
        r = CC.knn_device(t, k, want=combo)
        assert all((r[key] is None) == (key not in combo) for key in want)
        assert all(same(r[key].cpu().numpy(), want[key]) for key in combo)
    counters = torch.zeros(2, dtype=torch.int64).to(dev)
    CC.knn_device(t, k, want=("mean",), counters=counters)
    cells_read, tested = counters.cpu().tolist()
    print(f"knn {name} k={k}: {cells_read / len(t):.1f} cells and {tested / len(t):.1f} candidates per query")
    assert cells_read >= len(t) and k * len(t) <= tested < len(t) * len(t)
    CC.knn_device(t, k, cell=ONE, want=("mean",), counters=counters)
    assert counters.cpu().tolist() == [cells_read + len(t), tested + len(t) * (len(t) - 1)]


def check_finite(dev):
    """NaN and +-inf points are removed and counted, and the rest equals the run without them"""
    base = cloud("u257")
    pts = np.concatenate([base[:100], [[np.nan, 0, 0]], base[100:200], [[0, np.inf, 0], [1, 2, -np.inf]], base[200:], [[np.nan, np.inf, 3]]]).astype(F32)
    rgb = (np.arange(len(pts) * 3) % 251).astype(np.uint8).reshape(-1, 3)
    view = np.arange(len(pts), dtype=np.int32) * 3
    ok = O.finite(pts)
    assert (~ok).sum() == 4 and np.array_equal(pts[ok], base)
    flags, count = CC.finite_flags(torch.from_numpy(pts).to(dev))
    assert count == 257 and np.array_equal(flags.cpu().numpy(), ok.astype(np.uint8))
    r = CC.finite_points(torch.from_numpy(pts).to(dev), torch.from_numpy(rgb).to(dev), torch.from_numpy(view).to(dev))
    assert r["removed"] == 4 and np.array_equal(bits(r["xyz"].cpu().numpy()), bits(base))
    assert np.array_equal(r["rgb"].cpu().numpy(), rgb[ok]) and np.array_equal(r["view"].cpu().numpy(), view[ok])
    assert np.array_equal(r["index"].cpu().numpy(), np.nonzero(ok)[0].astype(np.int32))
    got = _knn(r["xyz"], 8, None)[0]
    assert all(same(g, w) for g, w in zip(got, reference_knn("u257", 8)))
    with pytest.raises(_lib.RcmvsError, match="non-finite"):
        CC.knn(torch.from_numpy(pts).to(dev), 8)
    none = CC.finite_points(torch.from_numpy(np.full((5, 3), np.nan, F32)).to(dev))
    assert none["removed"] == 5 and tuple(none["xyz"].shape) == (0, 3)
    plain = CC.finite_points(torch.from_numpy(base.copy()).to(dev))
    assert plain["removed"] == 0 and plain["rgb"] is None and plain["view"] is None and np.array_equal(bits(plain["xyz"].cpu().numpy()), bits(base))


def check_kdtree(dev):
    """an independent check: scipy's k-d tree gives the same index rows on the 4 097-point cloud (all d2 of a row's first k + 1 distinct)"""
    from scipy.spatial import cKDTree
    name = "u4097"
    pts = cloud(name)
    p64 = pts.astype(np.float64)
    for k in (1, 8, 20, 32):
        idx, d2, _ = reference_knn(name, k)
        assert (np.diff(d2, axis=1) > 0).all() and (d2[:, 0] > 0).all()              # the precondition (0 for the point itself, then k distinct), on the oracle alone
        tree = cKDTree(p64).query(p64, k + 1)[1]
        assert np.array_equal(tree[:, 0], np.arange(len(pts))) and np.array_equal(tree[:, 1:], idx)
        got = CC.knn(dev_cloud(name, dev), k)[0].cpu().numpy()
        assert np.array_equal(got, tree[:, 1:])


RADIUS_CASES = (("lattice", 1.0, 6), ("lattice", 1.0, 7), ("lattice", np.sqrt(2.0), 18), ("dup40", 0.0, 1), ("dup40", 0.0, 40), ("zeros", 0.0, 3),
                ("u257", np.inf, 300), ("u257", np.inf, 256), ("u257", 0.1, 0), ("u2049", 0.08, 5), ("clusters", 10.0, 2), ("huge", 1.0, 1), ("n1", 1.0, 1), ("n0", 1.0, 1))


def check_radius(dev, name, r, cap):
    want_c, want_k = O.radius(cloud(name), r, cap)
    t = dev_cloud(name, dev)
    for cell in cells(name):
        keep, counts = CC.radius_outliers(t, r, cap, cell)
        assert np.array_equal(counts.cpu().numpy(), want_c) and np.array_equal(keep.cpu().numpy(), want_k), (name, r, cap, cell)
    if (name, r, cap) == ("lattice", 1.0, 6):                      # d2 == r r counts: the 7^3 interior points have their six neighbours
        assert int(want_k.sum()) == 343
    if name == "dup40":
        assert (want_c == min(cap, 39)).all()
    if cap == 0:
        assert want_k.all() and not want_c.any()


STAT_CASES = (("u2049", 8, 2.0), ("u257", 20, 0.0), ("u257", 20, np.inf), ("u4097", 32, 1.0), ("n8", 8, 2.0), ("n9", 8, 2.0), ("n2", 1, 0.5), ("dup40", 8, 0.0),
              ("clusters", 8, 1.0), ("plane_far", 8, 2.0), ("loop", 2, 0.0), ("n0", 8, 2.0))


def check_stat(dev, name, k, ratio):
    mean = reference_knn(name, k)[2]
    want_keep, (nv, mu, sigma, thr) = O.statistical(mean, ratio)
    if name == "n8":
        assert nv == 0 and np.isnan(mu) and not want_keep.any()
    if name == "plane_far":                                       # the known answer: exactly the five far points go
        assert np.array_equal(want_keep, np.r_[np.ones(400, np.uint8), np.zeros(5, np.uint8)])
    if name == "loop":                                            # all means equal: sigma is 0 and `<=` keeps every point
        assert (mean == 1.0).all() and sigma == 0.0 and want_keep.all()
    if ratio == np.inf:
        assert want_keep.all() and thr == np.inf
    if name == "dup40":
        assert mu == 0.0 and sigma == 0.0 and want_keep.all()
    keep, info = CC.statistical_outliers(dev_cloud(name, dev), k, ratio)
    print(f"stat {name} k={k} ratio={ratio}: valid {info['valid']} mu {info['mu']!r} sigma {info['sigma']!r} threshold {info['threshold']!r} kept {int(want_keep.sum())}")
    assert np.array_equal(keep.cpu().numpy(), want_keep) and info["valid"] == nv
    assert same(np.array([info["mu"], info["sigma"], info["threshold"]]), np.array([mu, sigma, thr], np.float64))
    keep2, info2 = CC.statistical_outliers(dev_cloud(name, dev), k, ratio, cell=tiny(name))
    assert np.array_equal(keep2.cpu().numpy(), want_keep) and same(np.array([info2["mu"], info2["sigma"]]), np.array([mu, sigma], np.float64))


def views_for(name):
    """a view number per point (some outside 0 .. nc-1) and the centres, for the orientation cases"""
    n = len(cloud(name))
    rng = np.random.default_rng(11)
    centres = rng.normal(size=(4, 3)) * 3.0
    view = rng.integers(0, 4, n).astype(np.int32)
    view[::17] = -1
    view[5::23] = 4
    return view, centres


NORMAL_CASES = (("u4097", 16, False), ("u257", 16, True), ("u2049", 8, True), ("lattice", 6, True), ("dup40", 8, True), ("line", 6, False), ("n2", 4, True),
                ("n1", 4, False), ("n0", 4, True), ("plane", 8, False), ("zeros", 8, False), ("huge", 8, True), ("clusters", 8, True), ("sphere", 12, False))


@functools.lru_cache(maxsize=None)
def reference_normals(name, k, oriented):
    view, centres = views_for(name) if oriented else (None, None)
    return O.normals(cloud(name), reference_knn(name, k)[0], view, centres, details=True)


def check_normals(dev, name, k, oriented):
    want, cnt, _, _ = reference_normals(name, k, oriented)
    assert cnt["unconverged"] == 0
    n = len(cloud(name))
    if name == "dup40":
        assert cnt["degenerate"] == n and not want.any()
    if name == "line":                                            # all but the few points whose neighbours come from both lines
        assert cnt["degenerate"] >= 90 and cnt["degenerate"] + cnt["with_normal"] == n
    if name in ("n1", "n2"):
        assert cnt["too_few"] == n
    if name == "plane":
        assert np.array_equal(want, np.tile(np.array([[0, 0, 1]], F32), (n, 1)))
    if oriented and n > 100:
        assert cnt["unoriented"] > 0 and cnt["flipped"] > 0 and cnt["oriented"] > 0
    view, centres = views_for(name) if oriented else (None, None)
    t = dev_cloud(name, dev)
    got, info = CC.estimate_normals(t, k, None if view is None else torch.from_numpy(view).to(dev), centres)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want)), f"{name} k={k}: normals differ from the oracle"
    assert {key: info[key] for key in O.COUNTER_NAMES} == cnt, (info, cnt)
    got2, _ = CC.estimate_normals(t, k, None if view is None else torch.from_numpy(view).to(dev), centres, cell=tiny(name))
    assert np.array_equal(bits(got2.cpu().numpy()), bits(want))


def check_plane_orientation(dev):
    """the planar grid: (0, 0, 1) with a centre above, (0, 0, -1) below, and a centre exactly in the plane (dot 0) flips nothing"""
    pts = cloud("plane")
    n = len(pts)
    centres = np.array([[10, 10, 5], [10, 10, -5], [3, 4, 0]], np.float64)
    for w, z, counted in ((0, 1.0, "oriented"), (1, -1.0, "flipped"), (2, 1.0, "oriented")):
        view = np.full(n, w, np.int32)
        want, cnt = O.normals(pts, reference_knn("plane", 8)[0], view, centres)
        assert np.array_equal(want, np.tile(np.array([[0, 0, z]], F32), (n, 1))) and cnt[counted] == n
        got, info = CC.estimate_normals(dev_cloud("plane", dev), 8, torch.from_numpy(view).to(dev), centres)
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)) and info[counted] == n and info["unconverged"] == 0


def sphere_views():
    p = cloud("sphere").astype(np.float64)
    return np.argmax(p @ SPHERE_CAMS.T, axis=1).astype(np.int32)


def check_sphere(dev):
    """a sphere sampled from outside cameras: every normal looks at its camera and along the radius"""
    pts, view = cloud("sphere"), sphere_views()
    got, info = CC.estimate_normals(dev_cloud("sphere", dev), 12, torch.from_numpy(view).to(dev), SPHERE_CAMS)
    want, cnt = O.normals(pts, reference_knn("sphere", 12)[0], view, SPHERE_CAMS)
    g = got.cpu().numpy()
    assert np.array_equal(bits(g), bits(want)) and info["with_normal"] == len(pts) and info["unconverged"] == 0 and info["unoriented"] == 0
    p = pts.astype(np.float64)
    to_cam = SPHERE_CAMS[view] - p
    assert ((g * to_cam).sum(1) > 0).all() and ((g * p).sum(1) > 0).all()


# The largest sin(angle) c_measured 2^-52 lambda2 / (lambda1 - lambda0) between the oracle's fp64 normal and numpy.linalg.eigh's
# vector, measured with the ORACLE alone on the CPU: 1.8724 over u4097 (k = 16) and 1.9112 over the sphere (k = 12), so c_measured =
# 1.9112 (check_eigh prints both again; profiles/cloud_clean_pytest_gpu.txt).  EIGH_C = 8 c_measured = 15.29: both solvers are only
# backward stable.  The kernel's fp32 normals carry one more rounding per component, which the bound on them adds.
EIGH_MEASURED = 1.9112
EIGH_C = 8 * EIGH_MEASURED
FP32_ROUNDING = 2.0 ** -23                                        # one fp32 rounding per component of a unit vector: below sqrt(3) 2^-24


@functools.lru_cache(maxsize=None)
def eigh_data(name, k):
    """numpy.linalg.eigh of every neighbourhood's covariance (the oracle's) -> eigenvalues (n,3) ascending, the first eigenvector (n,3)"""
    pts, idx = cloud(name), reference_knn(name, k)[0]
    plist = pts.astype(np.float64).tolist()
    covs = np.array([O.covariance(plist, i, idx[i])[1] for i in range(len(pts))])
    mats = covs[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)
    w, v = np.linalg.eigh(mats)
    return w, v[:, :, 0]


def eigh_figures(name, k, normals64):
    """per point: sin of the angle between normals64 and eigh's vector of the smallest eigenvalue, and lambda2 / (lambda1 - lambda0);
    the neighbourhoods with (lambda1 - lambda0) >= 1e-6 lambda2 only -> (sines, ratios, the fraction of points left out)"""
    w, v0 = eigh_data(name, k)
    ok = (w[:, 1] - w[:, 0]) >= 1e-6 * w[:, 2]
    sines = np.linalg.norm(np.cross(normals64[ok], v0[ok]), axis=1)
    return sines, w[ok, 2] / (w[ok, 1] - w[ok, 0]), 1.0 - ok.mean()


def check_eigh(dev, name, k):
    _, _, _, full = reference_normals(name, k, False)
    sines, ratios, left_out = eigh_figures(name, k, full)
    measured = float((sines / (2.0 ** -52 * ratios)).max())
    print(f"eigh {name} k={k}: oracle against numpy.linalg.eigh: largest sin / (2^-52 lambda2 / (lambda1 - lambda0)) = {measured:.3f} (c = {EIGH_C}), "
          f"{100 * left_out:.2f} % of the points outside the condition")
    assert left_out <= 0.05 and (sines <= EIGH_C * 2.0 ** -52 * ratios).all()
    got = CC.estimate_normals(dev_cloud(name, dev), k)[0].cpu().numpy().astype(np.float64)
    s2, r2, _ = eigh_figures(name, k, got)
    assert (s2 <= EIGH_C * 2.0 ** -52 * r2 + FP32_ROUNDING).all()


def check_refusals(dev):
    """the wrapper's and the C ABI's refusals, with the argument named and nothing written"""
    t = dev_cloud("u257", dev)
    for k, pattern in ((0, "k = 0"), (33, "k = 33"), (True, "k = True"), (2.0, "k = 2.0")):
        with pytest.raises(_lib.RcmvsError, match=pattern):
            CC.knn(t, k)
    for call, pattern in ((lambda: CC.radius_outliers(t, -1.0, 3), "radius = -1.0"), (lambda: CC.radius_outliers(t, np.nan, 3), "radius = nan"),
                          (lambda: CC.radius_outliers(t, 1.0, -1), "min_points = -1"), (lambda: CC.statistical_outliers(t, 8, -0.5), "ratio = -0.5"),
                          (lambda: CC.statistical_outliers(t, 8, np.nan), "ratio = nan"), (lambda: CC.knn(t.double(), 8), "float32"),
                          (lambda: CC.knn(t, 8, cell=0.0), "cell = 0.0"), (lambda: CC.estimate_normals(t, 8, view=torch.zeros(257, dtype=torch.int32).to(dev)), "come together"),
                          (lambda: CC.clean_cloud(t, centres=np.zeros((1, 3))), "come together")):
        with pytest.raises(_lib.RcmvsError, match=pattern):
            call()
    # the C ABI
    n, k = 257, 8
    grid = CC.Grid(t)
    fill = {torch.uint8: 99, torch.int32: -7, torch.int64: -7, torch.float32: -7.0, torch.float64: -7.0}
    mk = lambda count, dtype: torch.full((count,), fill[dtype], dtype=dtype).to(dev)                       # noqa: E731
    untouched = lambda *ts: all(bool((x == fill[x.dtype]).all()) for x in ts)                              # noqa: E731
    p = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)                                               # noqa: E731
    idx, d2, mean, counters = mk(n * k, torch.int32), mk(n * k, torch.float64), mk(n, torch.float64), mk(2, torch.int64)
    g, d = grid.host()

    def refused(name, order, good, bad, timed_bad=()):
        for kw, pattern in bad:
            with pytest.raises(_lib.RcmvsError, match=pattern):
                _lib.call(name, *[dict(good, **kw)[key] for key in order], NULL)
        for kw, pattern in timed_bad:
            with pytest.raises(_lib.RcmvsError, match=pattern):
                _lib.call(name + "_timed", *[dict(good, **kw)[key] for key in order], dict(good, **kw)["phase"], NULL, NULL, NULL)

    good = dict(n=n, k=k, g=g, d=d, cs=p(grid.cell_start), so=p(grid.sorted), si=p(grid.sorted_idx), idx=p(idx), d2=p(d2), mean=p(mean), cnt=p(counters), phase=0)
    order = ("n", "k", "g", "d", "cs", "so", "si", "idx", "d2", "mean", "cnt")
    refused("rcmvs_ck_knn", order, good,
            [({"k": 0}, "k = 0"), ({"k": 33}, "k = 33"), ({"n": -1}, "n = -1"), ({"n": 1 << 31}, "n = 2147483648"), ({"n": 70000000, "k": 32}, "n k = 2240000000"),
             ({"g": NULL}, "null pointer"), ({"d": NULL}, "null pointer"), ({"cs": NULL}, "null pointer"), ({"so": NULL}, "null pointer"), ({"si": NULL}, "null pointer"),
             ({"d2": p(d2, 4)}, "d2 must be 8-byte aligned"), ({"mean": p(mean, 4)}, "mean must be 8-byte aligned"), ({"idx": p(idx, 2)}, "idx must be 4-byte aligned"),
             ({"so": p(grid.sorted, 4)}, "sorted must be 16-byte aligned"), ({"cnt": p(counters, 4)}, "counters must be 8-byte aligned"),
             ({"idx": p(d2)}, "overlaps"), ({"mean": p(d2, 8)}, "overlaps"), ({"idx": p(grid.sorted_idx)}, "overlaps"), ({"d2": p(grid.sorted)}, "overlaps")],
            [({"phase": 1}, "phase = 1"), ({"phase": -1}, "phase = -1")])
    assert untouched(idx, d2, mean, counters)
    _lib.call("rcmvs_ck_knn", *[good[key] for key in order], NULL)
    want = reference_knn("u257", k)
    assert same(idx.cpu().numpy().reshape(n, k), want[0]) and same(d2.cpu().numpy().reshape(n, k), want[1]) and same(mean.cpu().numpy(), want[2])

    count, keep = mk(n, torch.int32), mk(n, torch.uint8)
    good = dict(n=n, r2=0.01, cap=3, g=g, d=d, cs=p(grid.cell_start), so=p(grid.sorted), si=p(grid.sorted_idx), count=p(count), keep=p(keep), phase=0)
    order = ("n", "r2", "cap", "g", "d", "cs", "so", "si", "count", "keep")
    refused("rcmvs_ck_radius", order, good,
            [({"r2": -1.0}, "r2 = -1"), ({"r2": float("nan")}, "r2 = nan"), ({"cap": -1}, "cap = -1"), ({"n": -2}, "n = -2"), ({"count": NULL}, "null pointer"),
             ({"cs": NULL}, "null pointer"), ({"count": p(count, 2)}, "count must be 4-byte aligned"), ({"keep": p(count)}, "overlaps"), ({"count": p(grid.sorted)}, "overlaps")],
            [({"phase": 2}, "phase = 2")])
    assert untouched(count, keep)

    flags, offsets, vm, part, stats, skeep = mk(n, torch.uint8), mk(n + 1, torch.int32), mk(n, torch.float64), mk(CC.MOMENT_BLOCKS, torch.float64), mk(8, torch.float64), mk(n, torch.uint8)
    work = CC._scan_work(n, dev)
    good = dict(mean=p(mean), n=n, ratio=2.0, flags=p(flags), off=p(offsets), work=p(work), vm=p(vm), part=p(part), stats=p(stats), keep=p(skeep), phase=0)
    order = ("mean", "n", "ratio", "flags", "off", "work", "vm", "part", "stats", "keep")
    refused("rcmvs_ck_stat", order, good,
            [({"ratio": -1.0}, "ratio = -1"), ({"ratio": float("nan")}, "ratio = nan"), ({"n": -1}, "n = -1"), ({"mean": NULL}, "null pointer"), ({"off": NULL}, "null pointer"),
             ({"work": NULL}, "null pointer"), ({"work": p(work, 4)}, "scan_work must be 8-byte aligned"), ({"stats": p(stats, 4)}, "stats must be 8-byte aligned"),
             ({"vm": p(mean)}, "overlaps"), ({"keep": p(flags)}, "overlaps"), ({"stats": p(part, 8)}, "overlaps")],
            [({"phase": 1}, "phase = 1")])
    assert untouched(flags, offsets, vm, part, stats, skeep)

    normals, ncnt, view, cen = mk(3 * n, torch.float32), mk(CC.COUNTERS, torch.int64), torch.zeros(n, dtype=torch.int32).to(dev), torch.zeros(6, dtype=torch.float64).to(dev)
    good = dict(pts=p(t), n=n, k=k, idx=p(idx), view=p(view), cen=p(cen), nc=2, out=p(normals), cnt=p(ncnt), phase=0)
    order = ("pts", "n", "k", "idx", "view", "cen", "nc", "out", "cnt")
    refused("rcmvs_ck_normals", order, good,
            [({"k": 0}, "k = 0"), ({"k": 33}, "k = 33"), ({"nc": -1}, "nc = -1"), ({"n": -1}, "n = -1"), ({"cnt": NULL}, "null pointer"), ({"pts": NULL}, "null pointer"),
             ({"idx": NULL}, "null pointer"), ({"out": NULL}, "null pointer"), ({"view": NULL}, "come together"), ({"cen": NULL}, "come together"),
             ({"cnt": p(ncnt, 4)}, "counters must be 8-byte aligned"), ({"out": p(normals, 2)}, "normals must be 4-byte aligned"), ({"out": p(t)}, "overlaps"),
             ({"cnt": p(cen)}, "overlaps"), ({"out": p(idx)}, "overlaps")],
            [({"phase": 1}, "phase = 1")])
    assert untouched(normals, ncnt)

    ckeep = torch.ones(n, dtype=torch.uint8).to(dev)
    rgb, oxyz, orgb, oview, oindex, total = (torch.zeros(3 * n, dtype=torch.uint8).to(dev), mk(3 * n, torch.float32), mk(3 * n, torch.uint8), mk(n, torch.int32),
                                             mk(n, torch.int32), mk(1, torch.int64))
    good = dict(keep=p(ckeep), xyz=p(t), rgb=p(rgb), view=p(view), n=n, off=p(offsets), work=p(work), oxyz=p(oxyz), orgb=p(orgb), oview=p(oview), oindex=p(oindex),
                total=p(total), phase=0)
    order = ("keep", "xyz", "rgb", "view", "n", "off", "work", "oxyz", "orgb", "oview", "oindex", "total")
    refused("rcmvs_ck_compact", order, good,
            [({"n": -1}, "n = -1"), ({"keep": NULL}, "null pointer"), ({"xyz": NULL}, "null pointer"), ({"oxyz": NULL}, "null pointer"), ({"oindex": NULL}, "null pointer"),
             ({"total": NULL}, "null pointer"), ({"off": NULL}, "null pointer"), ({"work": NULL}, "null pointer"), ({"orgb": NULL}, "come together"),
             ({"view": NULL}, "come together"), ({"total": p(total, 4)}, "total must be 8-byte aligned"), ({"oxyz": p(t)}, "overlaps"), ({"oview": p(oindex)}, "overlaps"),
             ({"orgb": p(rgb)}, "overlaps")],
            [({"phase": 3}, "phase = 3")])
    assert untouched(offsets, oxyz, orgb, oview, oindex, total)

    fflags, fcount = mk(n, torch.uint8), mk(1, torch.int32)
    good = dict(pts=p(t), n=n, flags=p(fflags), count=p(fcount), phase=0)
    order = ("pts", "n", "flags", "count")
    refused("rcmvs_ck_finite", order, good,
            [({"n": -1}, "n = -1"), ({"count": NULL}, "null pointer"), ({"pts": NULL}, "null pointer"), ({"flags": NULL}, "null pointer"),
             ({"count": p(fcount, 2)}, "count must be 4-byte aligned"), ({"flags": p(t)}, "overlaps")],
            [({"phase": 1}, "phase = 1")])
    assert untouched(fflags, fcount)


def check_clean_cloud(dev):
    """the four steps in their order on a hostile cloud: equal to the oracle's steps, input order kept, stats in and out per step"""
    rng = np.random.default_rng(3)
    base = np.concatenate([cloud("u2049") * 10.0, (rng.random((40, 3)) * 200 - 100).astype(F32), [[np.nan, 1, 2], [3, np.inf, 4]]]).astype(F32)
    perm = rng.permutation(len(base))
    xyz = base[perm]
    rgb = rng.integers(0, 256, (len(xyz), 3)).astype(np.uint8)
    view = rng.integers(0, 3, len(xyz)).astype(np.int32)
    centres = np.array([[5, 5, 30], [-20, 5, 5], [5, 40, 5]], np.float64)
    opts = dict(radius=(1.0, 3), stat=(12, 1.5), normals=10)
    want = O.clean_cloud(xyz, rgb, view, centres, opts["radius"], opts["stat"], opts["normals"])
    assert 0 < len(want["xyz"]) < 2049 and want["info"]["finite_removed"] == 2
    r = CC.clean_cloud(torch.from_numpy(xyz).to(dev), torch.from_numpy(rgb).to(dev), torch.from_numpy(view).to(dev), centres, **opts)
    for key in ("xyz", "rgb", "view", "normals", "index"):
        assert np.array_equal(bits(r[key].cpu().numpy()), bits(want[key])), key
    s, info = r["stats"], want["info"]
    print("clean_cloud:", json.dumps(s))
    assert s["in"] == len(xyz) and s["finite"]["removed"] == 2 and s["radius"]["out"] == info["radius_out"] == s["stat"]["in"] and s["stat"]["out"] == info["stat_out"] == s["out"]
    assert same(np.array([s["stat"]["mu"], s["stat"]["sigma"], s["stat"]["threshold"]]), np.array([info["mu"], info["sigma"], info["threshold"]], np.float64))
    assert {k: s["normals"][k] for k in O.COUNTER_NAMES} == info["counters"] and s["radius"]["grid"]["cells"] >= 1
    assert np.array_equal(xyz[want["index"]], want["xyz"], equal_nan=True)
    nothing = CC.clean_cloud(torch.from_numpy(xyz).to(dev))
    assert nothing["normals"] is None and nothing["rgb"] is None and int(nothing["xyz"].shape[0]) == len(xyz) - 2 and set(nothing["stats"]) == {"in", "finite", "out"}


PROB, NCONS, DIST, DEPTH = 0.8, 3, 0.5, 0.01                      # tests/fusion_cases.py's thresholds
TANKS_PIX, TANKS_DEPTH, TANKS_PHOTO, TANKS_NCONS = 0.75, 0.01, 0.8, 3


def _check_driver_pair(dev, tmp_path, plain_call, clean_call, centres, n_views):
    opts = dict(radius=(8.0, 4), stat=(8, 2.0), normals=12)
    plain_ply, clean_ply = str(tmp_path / "plain.ply"), str(tmp_path / "clean.ply")
    stats0 = {}
    xyz0, rgb0 = plain_call(plain_ply, stats0)
    with open(plain_ply, "rb") as f:
        assert f.read() == fusion.ply_bytes(xyz0, rgb0)            # without `clean`: today's bytes, and no "cloud" key
    assert "cloud" not in stats0 and len(xyz0) > 500
    stats = {}
    xyz, rgb = clean_call(clean_ply, stats, opts)
    counts = [v["kept"] for v in stats["views"]]
    view = np.repeat(np.arange(n_views, dtype=np.int32), counts)
    assert len(view) == len(xyz0)
    want = CC.clean_cloud(torch.from_numpy(xyz0).to(dev), torch.from_numpy(rgb0).to(dev), torch.from_numpy(view).to(dev), centres, **opts)
    assert np.array_equal(bits(xyz), bits(want["xyz"].cpu().numpy())) and np.array_equal(rgb, want["rgb"].cpu().numpy())
    assert json.dumps(stats["cloud"]) == json.dumps(want["stats"]) and 0 < stats["cloud"]["out"] < len(xyz0)
    rx, rrgb, rn = dtu_io.read_ply_cloud_normals(clean_ply)
    assert np.array_equal(bits(rx), bits(xyz)) and np.array_equal(rrgb, rgb) and np.array_equal(bits(rn), bits(want["normals"].cpu().numpy()))
    assert np.array_equal(bits(dtu_io.read_ply_xyz(clean_ply)), bits(xyz))
    with open(clean_ply, "rb") as f:
        assert f.read() == fusion.ply_bytes(xyz, rgb, rn)
    v = want["view"].cpu().numpy()
    to_cam = centres[v] - xyz.astype(np.float64)
    dots = (rn.astype(np.float64) * to_cam).sum(1)
    has = np.abs(rn).sum(1) > 0
    print(f"driver: {len(xyz0)} fused points, {len(xyz)} written, {int(has.sum())} with a normal; cloud stats {json.dumps(stats['cloud'])}")
    assert has.mean() > 0.95 and (dots[has] > 0).all()
    return xyz0, rgb0, opts, stats


def check_filter_depth(dev, tmp_path):
    s = synthetic.fusion_scan(V=5, H=48, W=64)
    pair_folder, out_folder = str(tmp_path / "data" / "scan1"), str(tmp_path / "out" / "scan1")
    synthetic.write_fusion_scan(s, pair_folder, out_folder)
    centres = np.stack([fusion.camera_centre(s["E"][ref]) for ref, _ in s["pairs"]])
    E = s["E"][0].astype(np.float64)
    assert np.allclose(E[:3, :3] @ centres[0] + E[:3, 3], 0.0, atol=1e-9)            # the centre is the point the camera maps to its origin
    call = lambda ply, stats, **kw: fusion.filter_depth(pair_folder, out_folder, out_folder, ply, PROB, NCONS, DIST, DEPTH, device=dev, verbose=False,    # noqa: E731
                                                         save_masks=False, stats=stats, **kw)
    xyz0, rgb0, opts, stats = _check_driver_pair(dev, tmp_path, lambda ply, st: call(ply, st), lambda ply, st, o: call(ply, st, clean=o), centres, len(s["pairs"]))
    # the command line of the cloud tool on the plain PLY: the summary carries the counts the API gave
    out = str(tmp_path / "cli.ply")
    argv = ["--in", str(tmp_path / "plain.ply"), "--out", out, "--radius", "8.0", "4", "--stat", "8", "2.0", "--normals", "12", "--viewpoint", "0", "0", "0", "--device", str(dev)]
    summary = CC.main(argv)
    want = CC.clean_cloud(torch.from_numpy(xyz0).to(dev), torch.from_numpy(rgb0).to(dev), torch.zeros(len(xyz0), dtype=torch.int32).to(dev), np.zeros((1, 3)), **opts)
    assert json.dumps(summary["cloud"]) == json.dumps(want["stats"])
    rx, rrgb, rn = dtu_io.read_ply_cloud_normals(out)
    assert np.array_equal(bits(rx), bits(want["xyz"].cpu().numpy())) and np.array_equal(rrgb, want["rgb"].cpu().numpy())
    assert np.array_equal(bits(rn), bits(want["normals"].cpu().numpy()))


def check_filter_depth_tanks(dev, tmp_path):
    V, h, w, oh, ow = 5, 64, 96, 75, 100
    s = synthetic.tanks_fusion_scan(V=V, hw=(h, w), orig_hw=(oh, ow))
    scan_folder, out_folder = str(tmp_path / "tt" / "intermediate" / "Horse"), str(tmp_path / "out" / "Horse")
    synthetic.write_tanks_fusion_scan(s, scan_folder, out_folder)
    centres = np.stack([fusion.camera_centre(s["E"][ref]) for ref, _ in s["pairs"]])
    call = lambda ply, stats, **kw: fusion.filter_depth_tanks(scan_folder, out_folder, ply, TANKS_PIX, TANKS_DEPTH, TANKS_PHOTO, (w, h), (ow, oh), TANKS_NCONS, V, "Horse", device=dev,      # noqa: E731
                                                               verbose=False, save_masks=False, stats=stats, **kw)
    _check_driver_pair(dev, tmp_path, lambda ply, st: call(ply, st), lambda ply, st, o: call(ply, st, clean=o), centres, len(s["pairs"]))
