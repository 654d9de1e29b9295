"""The cases of the Poisson reconstruction (csrc/poisson.hip through rc_mvsnet_amd/poisson_mesh.py) and the checks that take a
device: tests/test_gpu_poisson.py runs them on the MI355X, tests/test_poisson_emu_cpu.py on the CPU emulation.  Every accumulator,
plane, level, residual, isovalue, field and mesh is compared with tests/poisson_oracle.py in every bit; the known answers are
asserted on the oracle alone first, so that a failure says which side is wrong.  Grids are 6^3 to 32 x 16 x 16 / 16 x 32 x 48 and no
cloud has more than 4 097 points.

The levels.  The rule (coarsen while every side is even and the smallest coarser side is >= 4) gives 16^3 -> 8^3 -> 4^3, 24^3 ->
12^3 -> 6^3, 32 x 16 x 16 -> 16 x 8 x 8 -> 8 x 4 x 4, 16 x 32 x 48 -> 8 x 16 x 24 -> 4 x 8 x 12, and ONE coarsening for 8^3 and 12^3
(4^3 and 6^3 are coarsest levels).  6^3, 10 x 6 x 12 (its coarser 5 x 3 x 6 has a side below 4) and 9 x 8 x 8 are the grids with no coarsening.

Bounds, each from the oracle's own figure (fp32 planes, fp64 arithmetic) with a margin of 1.5, written where they are used."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import poisson_oracle as O
import tsdf_oracle as T
from rc_mvsnet_amd import _lib, poisson_mesh as PM

F32, F64 = np.float32, np.float64
NULL = ctypes.c_void_p(0)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and bool(np.array_equal(bits(got), bits(want)))


def cube(r, side=2.5):
    """the box of side `side` about the origin as r x r x r voxels (r: an int or three)"""
    dims = [r] * 3 if isinstance(r, int) else list(r)
    h = side / max(dims)
    return [-0.5 * dims[0] * h, -0.5 * dims[1] * h, -0.5 * dims[2] * h, h], dims


def sphere_points(n, seed=1):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)


def _hazards(grid, dims):
    """points on voxel centres and cell faces (weights exactly 0 and 1), in the outermost layer, one ulp inside and outside the
    splattable region, and hostile normals and coordinates"""
    o, h = np.array(grid[:3]), grid[3]
    centre = lambda i, j, k: o + (np.array([i, j, k]) + 0.5) * h          # noqa: E731
    up, down = (lambda v: np.nextafter(F32(v), F32(np.inf))), (lambda v: np.nextafter(F32(v), F32(-np.inf)))      # noqa: E731
    g = dims
    lo, hi = F32(o[0] + 0.5 * h), F32(o[0] + (g[0] - 0.5) * h)             # the first and the last voxel centre along x
    pts = [centre(3, 4, 5), centre(3, 4, 5) + [0.5 * h, 0, 0], centre(0, 0, 0), centre(g[0] - 2, g[1] - 2, g[2] - 2), centre(g[0] - 1, 3, 3),
           [lo, 0.1, 0.1], [down(lo), 0.1, 0.1], [up(lo), 0.1, 0.1], [hi, 0.1, 0.1], [down(hi), 0.1, 0.1], [up(hi), 0.1, 0.1],
           o + 0.75 * h, o + [0.75 * h, 3 * h, 3 * h], [0.3, 0.2, 0.1], [0.3, 0.2, 0.1], [0.3, 0.2, 0.1], [0.3, 0.2, 0.1], [0.3, 0.2, 0.1], [0.3, 0.2, 0.1],
           [0.3, 0.2, 0.1], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e30, 0, 0], [-1e30, 1e30, 1e30], [-0.4, 0.5, 0.6], [-0.4, 0.5, 0.6]]
    nrm = [[0, 0, 1], [1, 0, 0], [0, 1, 0], [0, 0, -1], [1, 1, 1], [1, 0, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 1, 0],
           [0, 0, 0], [np.nan, 0, 1], [np.inf, 0, 0], [0, -np.inf, 0], [1e-30, 0, 0], [1e30, -1e30, 1e30], [3, 4, 12], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1],
           [0, 0, 1], [-0.0, 0.0, -0.0], [1e-45, 0, 0]]
    return np.array(pts, F64).astype(F32), np.array(nrm, F64).astype(F32)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: xyz, normals, rgb (or None), grid, dims, cycles, trim (a number, "exact" or "above"), trim_relative, density_weight"""
    rng = np.random.default_rng(11)
    c = {"rgb": None, "cycles": 2, "trim": 0.0, "trim_relative": None, "density_weight": True}
    c["grid"], c["dims"] = cube(16)
    colours = lambda n: rng.integers(0, 256, (n, 3)).astype(np.uint8)                                       # noqa: E731
    if name == "empty":
        c["xyz"], c["normals"] = np.zeros((0, 3), F32), np.zeros((0, 3), F32)
    elif name == "one":
        c["xyz"], c["normals"], c["cycles"] = np.array([[0.11, -0.23, 0.31]], F32), np.array([[0.0, 0.6, 0.8]], F32), 8
    elif name == "opposite":
        c["xyz"], c["normals"] = np.array([[0.11, -0.23, 0.31]] * 2, F32), np.array([[0.3, 0.6, 0.8], [-0.3, -0.6, -0.8]], F32)
    elif name == "dup40":
        c["xyz"], c["normals"], c["rgb"] = np.tile(np.array([[0.4, 0.1, -0.7]], F32), (40, 1)), np.tile(np.array([[1, 2, -2]], F32), (40, 1)), colours(40)
    elif name == "n4097":
        c["grid"], c["dims"] = cube((32, 16, 16))
        c["xyz"] = ((rng.random((4097, 3)) - 0.5) * np.array([2.3, 1.1, 1.1])).astype(F32)
        c["normals"], c["rgb"] = rng.normal(size=(4097, 3)).astype(F32), colours(4097)
    elif name in ("hazards", "hazards_grey"):
        c["xyz"], c["normals"] = _hazards(c["grid"], c["dims"])
        c["rgb"] = colours(len(c["xyz"])) if name == "hazards" else None
    elif name == "contention":
        c["grid"], c["dims"] = cube(8)
        o, h = np.array(c["grid"][:3]), c["grid"][3]
        c["xyz"] = (o + (np.array([3.5, 2.5, 4.5]) + rng.random((1000, 3))) * h).astype(F32)
        c["normals"], c["rgb"] = rng.normal(size=(1000, 3)).astype(F32), colours(1000)
    elif name.startswith("grid_"):                                   # 600 points of the unit sphere in the box of side 2.5
        dims = tuple(int(v) for v in name[5:].split("x"))
        c["grid"], c["dims"] = cube(dims if len(dims) == 3 else dims[0])
        c["xyz"] = sphere_points(600, 3) * np.array(c["dims"], F32) / F32(max(c["dims"]))
        c["normals"], c["cycles"] = sphere_points(600, 3), 3
    elif name.startswith("sphere16"):                                # sphere16, _c0, _c1, _c8, _exact, _above, _flat, _rel
        c["xyz"], c["normals"], c["rgb"] = sphere_points(300, 5), sphere_points(300, 5), colours(300)
        tail = name[8:]
        c["cycles"] = {"_c0": 0, "_c1": 1, "_c8": 8}.get(tail, 2)
        c["trim"] = {"_exact": "exact", "_above": "above"}.get(tail, 0.0)
        c["density_weight"] = tail != "_flat"
        c["trim_relative"] = 0.25 if tail == "_rel" else None
    else:
        raise KeyError(name)
    c["xyz"], c["normals"] = np.ascontiguousarray(c["xyz"], F32), np.ascontiguousarray(c["normals"], F32)
    return c


PIPELINE_CASES = ["empty", "one", "opposite", "dup40", "n4097", "hazards", "hazards_grey", "contention", "grid_16", "grid_32x16x16", "grid_16x32x48", "grid_24",
                  "grid_8", "grid_12", "grid_6", "grid_10x6x12", "grid_9x8x8", "sphere16_c0", "sphere16_c1", "sphere16_c8", "sphere16_exact", "sphere16_above",
                  "sphere16_flat", "sphere16_rel"]


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle's every stage for a case, computed once and left unchanged"""
    c = case(name)
    trim = c["trim"]
    if isinstance(trim, str):                                        # a threshold that is exactly one voxel's dilated density, or one ulp above it
        D = O.dilate(O.splat(c["xyz"], c["normals"], c["rgb"], c["grid"], c["dims"], c["density_weight"])["W"], c["dims"])
        v = F64(np.sort(D[D > 0])[len(D[D > 0]) // 2])
        trim = float(v if trim == "exact" else np.nextafter(v, np.inf))
    r = O.reconstruct(c["xyz"], c["normals"], c["rgb"], c["grid"], c["dims"], c["cycles"], trim, c["trim_relative"], c["density_weight"])
    r["mesh"] = T.extract(r["dsum"], r["wsum"], None if r["C"] is None else list(r["C"]), c["grid"], c["dims"], 1, sparse=True)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def tensors(c, dev):
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)                                        # noqa: E731
    return t(c["xyz"]), t(c["normals"]), t(c["rgb"])


def run(dev, name, stepwise):
    """the case through PoissonVolume -> dict of host arrays named as the oracle names them.  stepwise: one cycle per call, x and the
    coarser levels read after each; else one call"""
    c = case(name)
    ref = reference(name)
    vol = PM.PoissonVolume(c["grid"][:3], c["grid"][3], c["dims"], dev)
    vol.splat(*tensors(c, dev), density_weight=c["density_weight"])
    host = lambda t: t.cpu().numpy().copy()                                                                # noqa: E731
    out = {"acc": host(vol.acc).reshape(-1, vol.voxels), "W": host(vol.W), "V": np.stack([host(v) for v in vol.V]), "C": None if vol.C is None else np.stack([host(v) for v in vol.C]),
           "point": host(vol.point), "b": host(vol.b), "counters": [vol.stats[k] for k in PM.COUNTER_NAMES], "xs": [], "coarse": []}
    if stepwise:
        vol.solve(0)
        for _ in range(c["cycles"]):
            vol.solve(1)
            out["xs"].append(host(vol.x))
            out["coarse"].append(host(vol.coarse))
    else:
        vol.solve(c["cycles"])
    out["x"], out["resid"] = host(vol.x), list(vol.stats["residual"])
    out["stats"] = host(vol.isovalue())
    tv = vol.field(ref["trim"]) if c["trim_relative"] is None else vol.field(trim_relative=c["trim_relative"])
    out["trim"], out["trimmed"], out["dsum"], out["wsum"] = vol.stats["trim"], vol.stats["trimmed_voxels"], host(tv.dsum), host(tv.wsum)
    verts, faces, rgb = tv.extract(1)
    out["mesh"] = {"verts": host(verts), "faces": host(faces), "rgb": None if rgb is None else host(rgb)}
    out["levels"] = vol.stats["levels"]
    return out


def check_pipeline(dev, name):
    """every stage equal to the oracle in every bit; one call of `cycles` cycles equal to `cycles` calls of one; two runs identical"""
    c, ref = case(name), reference(name)
    got = run(dev, name, True)
    assert got["levels"] == O.levels(c["dims"])
    assert got["counters"] == ref["counters"][:4].tolist(), (got["counters"], ref["counters"])
    for key in ("acc", "W", "V", "point", "b"):
        assert same(got[key], ref[key]), key
    assert (got["C"] is None) == (ref["C"] is None) and (ref["C"] is None or same(got["C"], ref["C"]))
    for k in range(c["cycles"]):
        assert same(got["xs"][k], ref["xs"][k]), ("x after cycle", k)
        assert same(got["coarse"][k], ref["coarse"][k]), ("coarser levels after cycle", k)
    assert same(got["x"], ref["x"]) and same(np.array(got["resid"], F64), np.array(ref["resid"], F64)), (got["resid"], ref["resid"])
    assert same(got["stats"], ref["stats"]), (got["stats"], ref["stats"])
    assert got["trim"] == ref["trim"] and got["trimmed"] == ref["trimmed"] and same(got["dsum"], ref["dsum"]) and same(got["wsum"], ref["wsum"])
    want = ref["mesh"]
    assert same(got["mesh"]["verts"], want["verts"]) and np.array_equal(got["mesh"]["faces"], want["faces"])
    assert (want["rgb"] is None) == (got["mesh"]["rgb"] is None) and (want["rgb"] is None or np.array_equal(got["mesh"]["rgb"], want["rgb"]))
    again = run(dev, name, False)
    for key in ("acc", "W", "V", "point", "b", "x", "stats", "dsum", "wsum"):
        assert same(again[key], got[key]), ("second run", key)
    assert again["resid"] == got["resid"] and same(again["mesh"]["verts"], got["mesh"]["verts"]) and np.array_equal(again["mesh"]["faces"], got["mesh"]["faces"])
    print(f"{name}: dims {c['dims']} levels {len(got['levels'])} counters {got['counters']} residuals {['%.3g' % r for r in got['resid']]} iso {got['stats'][0]:.6g} "
          f"trimmed {got['trimmed']} mesh {len(want['verts'])} / {len(want['faces'])}")


def check_case_answers():
    """what the cases are there to show, on the oracle"""
    r = reference("empty")
    assert r["counters"][:4].tolist() == [0, 0, 0, 0] and not r["x"].any() and r["stats"][0] == 0 and len(r["mesh"]["faces"]) == 0
    r = reference("one")
    assert r["counters"][0] == 1 and r["point"][0, 1] >= 0.125 and abs(r["acc"][0].sum() - 2 ** 28) <= 8
    assert r["resid"][-1] < 1e-3 * np.abs(r["b"]).max()                   # the dipole's field: eight cycles solve it
    r = reference("opposite")
    assert r["counters"][0] == 2 and not r["acc"][1:4].any() and not r["V"].any() and not r["x"].any()
    r = reference("dup40")
    assert r["counters"][0] == 40 and (r["acc"][0] % 40 == 0).all() and same(r["point"][1:], r["point"][:-1])
    r, c = reference("hazards"), case("hazards")
    assert r["what"].tolist() == [0, 0, 0, 0, 3, 0, 3, 0, 3, 0, 3, 0, 0, 2, 1, 1, 1, 0, 0, 0, 1, 1, 1, 3, 3, 2, 0], r["what"].tolist()
    assert r["counters"][:4].tolist() == [13, 6, 2, 6], r["counters"]
    assert r["acc"][0, 3 + 16 * (4 + 16 * 5)] >= 2 ** 28 and r["C"] is not None and (r["C"][:, r["acc"][0] == 0] == 128).all()
    r = reference("contention")
    assert r["counters"][0] == 1000 and (r["acc"][0] != 0).sum() == 8 and abs(int(r["acc"][0].sum()) - 1000 * 2 ** 28) <= 8000
    assert [len(O.levels(case(n)["dims"])) for n in ("grid_16", "grid_32x16x16", "grid_16x32x48", "grid_24", "grid_8", "grid_12", "grid_6", "grid_10x6x12", "grid_9x8x8")] == \
        [3, 3, 3, 3, 2, 2, 1, 1, 1]
    a, b = reference("sphere16_exact"), reference("sphere16_above")
    assert b["trimmed"] > a["trimmed"] and same(a["dsum"], b["dsum"])
    assert not same(reference("sphere16_flat")["V"], reference("sphere16")["V"]) and (reference("sphere16_flat")["point"][:, 0] == 1).all()
    assert reference("sphere16_c0")["resid"] == [] and not reference("sphere16_c0")["x"].any()


# ---- known answers ------------------------------------------------------------------------------------------------------------------
# The oracle's figures (fp32 planes, fp64 arithmetic), measured by check_known_answers_oracle and printed there:
#   max | |v| - 1 | over the vertices: 16^3, 1 500 points: see SPHERE_BOUND; the bound is 1.5 x that, never above 0.5 h
#   the residual's largest ratio over cycles 1 .. 4: see CONVERGENCE; the bound is 1.5 x that
SPHERES = {16: 1500, 24: 4000}
SPHERE_MEASURED = {16: 0.2569, 24: 0.2665}                            # in voxels, the oracle's (an all-fp64 prototype gave 0.257 and 0.260)
SPHERE_BOUND = {r: min(0.5, 1.5 * v) for r, v in SPHERE_MEASURED.items()}
CONVERGENCE_MEASURED = {16: 0.2117, 24: 0.2322}                         # the largest residual ratio of cycles 1 .. 4, the oracle's
CONVERGENCE_BOUND = {r: 1.5 * v for r, v in CONVERGENCE_MEASURED.items()}
PLANE_MEASURED = 0.2348                                                # max |z| of the trimmed plane patch in voxels, the oracle's
PLANE_BOUND = min(0.5, 1.5 * PLANE_MEASURED)


def sphere_input(r, cap=None):
    d = sphere_points(SPHERES[r], 1)
    if cap is not None:
        d = d[d[:, 2] < cap]
    return np.ascontiguousarray(d)


@functools.lru_cache(maxsize=None)
def sphere_reference(r, cap=None, trim_relative=None):
    d = sphere_input(r, cap)
    grid, dims = cube(r)
    ref = O.reconstruct(d, d, None, grid, dims, 8, 0.0, trim_relative)
    ref["mesh"] = T.extract(ref["dsum"], ref["wsum"], None, grid, dims, 1, sparse=True)
    return ref


def sphere_run(dev, r, cap=None, trim_relative=None):
    d = torch.from_numpy(sphere_input(r, cap)).to(dev)
    verts, faces, _, stats = PM.reconstruct(d, d, None, cycles=8, trim_relative=trim_relative, grid=(cube(r)[0][:3], cube(r)[0][3], cube(r)[1]))
    return {"verts": verts.cpu().numpy(), "faces": faces.cpu().numpy()}, stats["residual"]


def assert_sphere(mesh, resid, r, what):
    h = 2.5 / r
    v, f = mesh["verts"], mesh["faces"]
    closed, euler = T.closed_and_oriented(f)
    outward, inward, degenerate = T.normals_outward(v, f, np.zeros(3))
    dist = float(np.abs(np.linalg.norm(v.astype(F64), axis=1) - 1.0).max() / h)
    ratios = [resid[k] / resid[k - 1] for k in range(1, 4)]
    print(f"{what} sphere {r}^3: {len(v)} vertices, {len(f)} faces, closed {closed}, Euler {euler}, outward {outward} inward {inward} degenerate {degenerate}, "
          f"max | |v| - 1 | = {dist:.4f} h (bound {SPHERE_BOUND[r]:.4f} h), residuals {['%.3e' % x for x in resid]}, ratios of cycles 2 .. 4 to the one before "
          f"{['%.3f' % x for x in ratios]} (bound {CONVERGENCE_BOUND[r]:.3f})")
    assert closed and euler == 2 and inward == 0 and outward + degenerate == len(f) and outward > 0
    assert dist <= SPHERE_BOUND[r]
    return ratios


def assert_convergence(resid, b_max, r, what):
    """the max-norm residual falls by at least the factor per cycle over cycles 1 .. 4 (cycle 1 against the right-hand side, whose
    max norm is the residual of chi = 0)"""
    ratios = [resid[0] / b_max] + [resid[k] / resid[k - 1] for k in range(1, 4)]
    print(f"{what} sphere {r}^3: residual ratios of cycles 1 .. 4 {['%.3f' % x for x in ratios]} (bound {CONVERGENCE_BOUND[r]:.3f}); later cycles {['%.3e' % x for x in resid[4:]]}")
    assert max(ratios) <= CONVERGENCE_BOUND[r], ratios


def check_sphere(dev, r):
    """dev None: the oracle alone"""
    ref = sphere_reference(r)
    b_max = float(np.abs(ref["b"]).max())
    assert_sphere(ref["mesh"], ref["resid"], r, "oracle")
    assert_convergence(ref["resid"], b_max, r, "oracle")
    if dev is None:
        return
    mesh, resid = sphere_run(dev, r)
    assert same(mesh["verts"], ref["mesh"]["verts"]) and np.array_equal(mesh["faces"], ref["mesh"]["faces"]) and resid == [float(x) for x in ref["resid"]]
    assert_sphere(mesh, resid, r, "kernels")
    assert_convergence(resid, b_max, r, "kernels")


def assert_trim(get, r, what):
    """get(cap, trim_relative) -> mesh"""
    h = 2.5 / r
    for f in (0.05, 0.25):
        m = get(None, f)
        closed, euler = T.closed_and_oriented(m["faces"])
        print(f"{what} sphere {r}^3 trim_relative {f}: {len(m['faces'])} faces, closed {closed}, Euler {euler}")
        assert closed and euler == 2
    m = get(0.6, None)
    closed, euler = T.closed_and_oriented(m["faces"])
    print(f"{what} sphere {r}^3 without z >= 0.6, trim 0: {len(m['faces'])} faces, closed {closed}, Euler {euler}")
    assert closed and euler == 2
    m = get(0.6, 0.05)
    closed, euler = T.closed_and_oriented(m["faces"])
    top = float(m["verts"][:, 2].max())
    print(f"{what} sphere {r}^3 without z >= 0.6, trim_relative 0.05: {len(m['faces'])} faces, closed {closed}, highest vertex {top:.4f} (bound {0.6 + 2 * h:.4f})")
    assert not closed and len(m["faces"]) > 0 and top < 0.6 + 2 * h


def check_trim(dev, r):
    assert_trim(lambda cap, f: sphere_reference(r, cap, f)["mesh"], r, "oracle")
    if dev is not None:
        assert_trim(lambda cap, f: sphere_run(dev, r, cap, f)[0], r, "kernels")


@functools.lru_cache(maxsize=None)
def plane_input():
    """a patch of the plane z = 0.1 seen from above: 2 000 points, |x|, |y| <= 0.8, normals (0, 0, 1), one colour"""
    rng = np.random.default_rng(2)
    xyz = np.concatenate([(rng.random((2000, 2)) - 0.5) * 1.6, np.full((2000, 1), 0.1)], axis=1).astype(F32)
    return xyz, np.tile(np.array([[0, 0, 1]], F32), (2000, 1)), np.tile(np.array([[200, 100, 50]], np.uint8), (2000, 1))


def assert_plane(mesh, W, grid, dims, what):
    h = grid[3]
    v = mesh["verts"].astype(F64)
    dist = float(np.abs(v[:, 2] - F64(F32(0.1))).max() / h)
    print(f"{what} plane patch: {len(v)} vertices, {len(mesh['faces'])} faces, max |z - 0.1| = {dist:.4f} h (bound {PLANE_BOUND:.4f} h)")
    assert len(mesh["faces"]) > 100 and dist <= PLANE_BOUND
    # a vertex lies on a grid edge; where both its voxels hold samples its colour is the cloud's
    u = (v - np.array(grid[:3])) / h - 0.5
    lo, hi = np.floor(u + 1e-9).astype(int), np.ceil(u - 1e-9).astype(int)
    num = lambda q: q[:, 0] + dims[0] * (q[:, 1] + dims[1] * q[:, 2])                                       # noqa: E731
    both = (W[num(lo)] > 0) & (W[num(hi)] > 0)
    print(f"{what} plane patch: {int(both.sum())} vertices between two voxels with samples")
    assert both.sum() > 50 and (mesh["rgb"][both] == np.array([200, 100, 50], np.uint8)).all()


def check_plane(dev):
    xyz, nrm, rgb = plane_input()
    grid, dims = cube(16)
    ref = O.reconstruct(xyz, nrm, rgb, grid, dims, 8, 0.0, 0.25)
    mesh = T.extract(ref["dsum"], ref["wsum"], list(ref["C"]), grid, dims, 1, sparse=True)
    assert_plane(mesh, ref["W"], grid, dims, "oracle")
    if dev is None:
        return
    t = [torch.from_numpy(a).to(dev) for a in (xyz, nrm, rgb)]
    verts, faces, col, _ = PM.reconstruct(*t, cycles=8, trim_relative=0.25, grid=(grid[:3], grid[3], dims))
    got = {"verts": verts.cpu().numpy(), "faces": faces.cpu().numpy(), "rgb": col.cpu().numpy()}
    assert same(got["verts"], mesh["verts"]) and np.array_equal(got["faces"], mesh["faces"]) and np.array_equal(got["rgb"], mesh["rgb"])
    assert_plane(got, ref["W"], grid, dims, "kernels")


def check_keep_largest(dev):
    """two spheres (radius 1 and 0.5) and three stray oriented points: one closed surface per sphere before, one after"""
    big, small = sphere_points(1500, 1), sphere_points(500, 4)
    stray = np.array([[0.0, 2.0, 0.0], [2.6, 2.0, 0.3], [1.3, -1.8, -0.5]], F32)
    xyz = np.concatenate([big, small * F32(0.5) + np.array([2.6, 0, 0], F32), stray]).astype(F32)
    nrm = np.concatenate([big, small, np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1]], F32)]).astype(F32)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (xyz, nrm)]
    out = {}
    for name, clean in (("before", {}), ("after", {"keep_largest": 1})):
        verts, faces, _, stats = PM.reconstruct(*t, resolution=32, cycles=8, trim_relative=0.05, clean=dict(clean))
        out[name] = (verts.cpu().numpy(), faces.cpu().numpy(), stats)
        c = stats["clean"]
        print(f"two spheres {name}: grid {stats['levels'][0]}, {c['components_in']} components in, {c['components_kept']} kept, {stats['faces']} faces, Euler {c['euler_characteristic']}, "
              f"boundary edges {c['boundary_edges']}")
    before, after = out["before"][2]["clean"], out["after"][2]["clean"]
    assert before["components_kept"] == 2 and before["boundary_edges"] == 0 and before["euler_characteristic"] == 4
    assert after["components_in"] == 2 and after["components_kept"] == 1 and after["boundary_edges"] == 0 and after["euler_characteristic"] == 2
    v = out["after"][0].astype(F64)
    assert T.closed_and_oriented(out["after"][1])[0] and np.abs(np.linalg.norm(v, axis=1) - 1.0).max() < 0.5 * out["after"][2]["voxel"]


def check_write_cloud(dev, tmp_path):
    """the end of filter_depth / filter_depth_tanks with ``poisson``: a sphere seen by six cameras, each point given to the camera it
    faces, cleaned with normals and meshed from the tensors on the device; without ``poisson`` the cloud's bytes are what they were
    and no second file appears; without normals it is refused"""
    from rc_mvsnet_amd import dtu_io, fusion
    d = sphere_points(1500, 1)
    cams = 3.0 * np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F64)
    view = np.argmax(d.astype(F64) @ cams.T, axis=1)
    pts = [d[view == v] for v in range(6)]
    cols = [np.full((len(p), 3), 40 * v + 10, np.uint8) for v, p in enumerate(pts)]
    plain, both = str(tmp_path / "plain.ply"), str(tmp_path / "both.ply")
    fusion._write_cloud(plain, pts, cols, list(cams), {"normals": 12}, {}, torch.device(dev))
    stats = {}
    fusion._write_cloud(both, pts, cols, list(cams), {"normals": 12}, stats, torch.device(dev), {"resolution": 16, "cycles": 8, "trim_relative": None})
    assert open(plain, "rb").read() == open(both, "rb").read() and not (tmp_path / "plain_poisson.ply").exists()
    verts, faces, rgb = dtu_io.read_ply_mesh_rgb(str(tmp_path / "both_poisson.ply"))
    p = stats["poisson"]
    closed, euler = T.closed_and_oriented(faces)
    outward, inward, _ = T.normals_outward(verts, faces, np.zeros(3))
    dist = float(np.abs(np.linalg.norm(verts.astype(F64), axis=1) - 1.0).max() / p["voxel"])
    print(f"driver: {stats['cloud']['out']} points with normals -> grid {p['levels'][0]}, {p['splatted']} splatted, {len(verts)} vertices, {len(faces)} faces, closed {closed}, "
          f"Euler {euler}, inward {inward}, max | |v| - 1 | = {dist:.4f} h")
    assert p["vertices"] == len(verts) and p["faces"] == len(faces) and p["splatted"] == 1500 and rgb is not None
    assert closed and euler == 2 and inward == 0 and outward > 0 and dist <= 0.5
    with pytest.raises(_lib.RcmvsError, match="needs oriented normals"):
        fusion._write_cloud(both, pts, cols, list(cams), None, {}, torch.device(dev), {"resolution": 16})


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def check_refusals(dev):
    """the wrapper's and the C ABI's refusals, with the argument named and nothing written"""
    grid, dims = cube(8)
    n, voxels = 5, 512
    xyz = torch.from_numpy(sphere_points(n)).to(dev)
    with pytest.raises(_lib.RcmvsError, match="at most 2\\^27"):
        PM.PoissonVolume(grid[:3], grid[3], [1024, 512, 512], dev)
    with pytest.raises(_lib.RcmvsError, match="sides >= 1"):
        PM.PoissonVolume(grid[:3], grid[3], [8, 0, 8], dev)
    for h in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(_lib.RcmvsError, match="voxel"):
            PM.PoissonVolume(grid[:3], h, dims, dev)
    vol = PM.PoissonVolume(grid[:3], grid[3], dims, dev)
    with pytest.raises(_lib.RcmvsError, match="5 points, 4 normals"):
        vol.splat(xyz, xyz[:4].contiguous())
    with pytest.raises(_lib.RcmvsError, match="float32"):
        vol.splat(xyz.double(), xyz)
    with pytest.raises(_lib.RcmvsError, match="rgb must be"):
        vol.splat(xyz, xyz, torch.zeros((4, 3), dtype=torch.uint8).to(dev))
    with pytest.raises(_lib.RcmvsError, match="splat\\(\\) comes first"):
        vol.solve(1)
    vol.splat(xyz, xyz)
    with pytest.raises(_lib.RcmvsError, match="solve\\(\\) comes first"):
        vol.field()
    for cycles in (-1, 65, 1.5, True):
        with pytest.raises(_lib.RcmvsError, match="cycles = "):
            vol.solve(cycles)
    vol.solve(1)
    for trim in (-1.0, np.nan, np.inf):
        with pytest.raises(_lib.RcmvsError, match="trim = "):
            vol.field(trim)
    with pytest.raises(_lib.RcmvsError, match="trim_relative = "):
        vol.field(trim_relative=-0.5)
    with pytest.raises(_lib.RcmvsError, match="resolution = 0"):
        PM.plan_grid([0, 0, 0], [1, 1, 1], resolution=0)
    with pytest.raises(_lib.RcmvsError, match="at most 2\\^27"):
        PM.plan_grid([0, 0, 0], [1, 1, 1], resolution=1024)
    # the C ABI
    fill = {torch.uint8: 99, torch.int64: -7, torch.float32: -7.0, torch.float64: -7.0}
    mk = lambda count, dtype: torch.full((count,), fill[dtype], dtype=dtype).to(dev)                       # noqa: E731
    untouched = lambda *ts: all(bool((x == fill[x.dtype]).all()) for x in ts)                              # noqa: E731
    p = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)                                               # noqa: E731
    g, d = (ctypes.c_double * 4)(*grid), (ctypes.c_int * 3)(*dims)
    gp, dp = ctypes.cast(g, ctypes.c_void_p), ctypes.cast(d, ctypes.c_void_p)
    keep = [(ctypes.c_int * 3)(1024, 512, 512), (ctypes.c_int * 3)(8, 0, 8), (ctypes.c_double * 4)(0, 0, 0, 0.0), (ctypes.c_double * 4)(0, 0, 0, float("nan")),
            (ctypes.c_double * 4)(float("inf"), 0, 0, 1.0)]
    big, zero, h0, hnan, oinf = (ctypes.cast(k, ctypes.c_void_p) for k in keep)

    def refused(name, order, good, bad, timed_bad=()):
        for kw, pattern in bad:
            with pytest.raises(_lib.RcmvsError, match=pattern):
                _lib.call(name, *[dict(good, **kw)[key] for key in order], NULL)
        for kw, pattern in timed_bad:
            with pytest.raises(_lib.RcmvsError, match=pattern):
                _lib.call(name + "_timed", *[dict(good, **kw)[key] for key in order], dict(good, **kw)["phase"], NULL, NULL, NULL)

    grids = [({"g": NULL}, "null pointer"), ({"d": NULL}, "null pointer"), ({"d": big}, "at most 2\\^27"), ({"d": zero}, "every side >= 1"), ({"g": h0}, "h > 0"),
             ({"g": hnan}, "h > 0"), ({"g": oinf}, "finite origin")]
    nrm, rgb = xyz.clone(), mk(3 * n, torch.uint8)
    acc, planes, point, counters = mk(7 * voxels, torch.int64), [mk(voxels, torch.float32) for _ in range(7)], mk(2 * n, torch.float64), mk(8, torch.int64)
    good = dict(xyz=p(xyz), nrm=p(nrm), rgb=p(rgb), n=n, dw=1, g=gp, d=dp, acc=p(acc), W=p(planes[0]), Vx=p(planes[1]), Vy=p(planes[2]), Vz=p(planes[3]), Cr=p(planes[4]),
                Cg=p(planes[5]), Cb=p(planes[6]), point=p(point), cnt=p(counters), phase=0)
    order = ("xyz", "nrm", "rgb", "n", "dw", "g", "d", "acc", "W", "Vx", "Vy", "Vz", "Cr", "Cg", "Cb", "point", "cnt")
    refused("rcmvs_po_splat", order, good, grids + [
        ({"n": -1}, "n = -1"), ({"n": 1 << 31}, "n = 2147483648"), ({"dw": 2}, "density_weight = 2"), ({"xyz": NULL}, "null pointer"), ({"nrm": NULL}, "null pointer"),
        ({"acc": NULL}, "null pointer"), ({"W": NULL}, "null pointer"), ({"Vz": NULL}, "null pointer"), ({"point": NULL}, "null pointer"), ({"cnt": NULL}, "null pointer"),
        ({"rgb": NULL}, "come together"), ({"Cg": NULL}, "come together"), ({"Cr": NULL, "Cg": NULL, "Cb": NULL}, "come together"),
        ({"acc": p(acc, 4)}, "acc must be 8-byte aligned"), ({"point": p(point, 4)}, "point must be 8-byte aligned"), ({"W": p(planes[0], 2)}, "a plane must be 4-byte aligned"),
        ({"xyz": p(xyz, 2)}, "xyz must be 4-byte aligned"), ({"cnt": p(counters, 4)}, "counters must be 8-byte aligned"),
        ({"Vx": p(planes[0])}, "overlaps"), ({"W": p(acc)}, "overlaps"), ({"point": p(xyz)}, "overlaps"), ({"Cb": p(planes[4], 4)}, "overlaps")],
        [({"phase": 3}, "phase = 3"), ({"phase": -1}, "phase = -1")])
    assert untouched(acc, point, counters, *planes)
    b = mk(voxels, torch.float32)
    good = dict(Vx=p(planes[1]), Vy=p(planes[2]), Vz=p(planes[3]), g=gp, d=dp, b=p(b), phase=0)
    refused("rcmvs_po_rhs", ("Vx", "Vy", "Vz", "g", "d", "b"), good, grids + [({"Vx": NULL}, "null pointer"), ({"b": NULL}, "null pointer"), ({"b": p(planes[2])}, "overlaps"),
                                                                               ({"b": p(b, 2)}, "4-byte aligned")], [({"phase": 1}, "phase = 1")])
    x, tmp, coarse, part, resid = mk(voxels, torch.float32), mk(voxels, torch.float32), mk(3 * 64, torch.float32), mk(1024, torch.float64), mk(8, torch.float64)
    good = dict(x=p(x), tmp=p(tmp), b=p(b), coarse=p(coarse), g=gp, d=dp, cycles=2, part=p(part), resid=p(resid), phase=0)
    refused("rcmvs_po_solve", ("x", "tmp", "b", "coarse", "g", "d", "cycles", "part", "resid"), good, grids + [
        ({"cycles": -1}, "cycles = -1"), ({"cycles": 65}, "cycles = 65"), ({"x": NULL}, "null pointer"), ({"tmp": NULL}, "null pointer"), ({"b": NULL}, "null pointer"),
        ({"coarse": NULL}, "null pointer"), ({"part": NULL}, "null pointer"), ({"resid": NULL}, "null pointer"), ({"tmp": p(x)}, "overlaps"), ({"x": p(b)}, "overlaps"),
        ({"coarse": p(tmp)}, "overlaps"), ({"resid": p(part, 64)}, "overlaps"), ({"x": p(x, 2)}, "x must be 4-byte aligned"), ({"resid": p(resid, 4)}, "resid must be 8-byte aligned")],
        [({"phase": 4}, "phase = 4"), ({"phase": -1}, "phase = -1")])
    assert untouched(x, tmp, coarse, part, resid)
    terms, tpart, stats = mk(4 * n, torch.float64), mk(5 * 256, torch.float64), mk(8, torch.float64)
    good = dict(xyz=p(xyz), point=p(point), n=n, chi=p(x), g=gp, d=dp, terms=p(terms), part=p(tpart), stats=p(stats), phase=0)
    refused("rcmvs_po_iso", ("xyz", "point", "n", "chi", "g", "d", "terms", "part", "stats"), good, grids + [
        ({"n": -1}, "n = -1"), ({"xyz": NULL}, "null pointer"), ({"point": NULL}, "null pointer"), ({"chi": NULL}, "null pointer"), ({"terms": NULL}, "null pointer"),
        ({"stats": NULL}, "null pointer"), ({"terms": p(point)}, "overlaps"), ({"stats": p(tpart)}, "overlaps"), ({"terms": p(terms, 4)}, "terms must be 8-byte aligned")],
        [({"phase": 1}, "phase = 1")])
    assert untouched(terms, tpart, stats)
    dsum, wsum, trimmed = mk(voxels, torch.float32), mk(voxels, torch.float32), mk(1, torch.int64)
    good = dict(chi=p(x), W=p(planes[0]), stats=p(stats), trim=0.5, d=dp, dsum=p(dsum), wsum=p(wsum), trimmed=p(trimmed), phase=0)
    refused("rcmvs_po_field", ("chi", "W", "stats", "trim", "d", "dsum", "wsum", "trimmed"), good, [
        ({"trim": -0.5}, "trim = -0.5"), ({"trim": float("nan")}, "trim = nan"), ({"trim": float("inf")}, "trim = inf"), ({"d": NULL}, "null pointer"), ({"d": big}, "at most 2\\^27"),
        ({"d": zero}, "every side >= 1"), ({"chi": NULL}, "null pointer"), ({"W": NULL}, "null pointer"), ({"stats": NULL}, "null pointer"), ({"dsum": NULL}, "null pointer"),
        ({"trimmed": NULL}, "null pointer"), ({"dsum": p(x)}, "overlaps"), ({"wsum": p(dsum)}, "overlaps"), ({"trimmed": p(trimmed, 4)}, "trimmed must be 8-byte aligned")],
        [({"phase": 1}, "phase = 1")])
    assert untouched(dsum, wsum, trimmed)
