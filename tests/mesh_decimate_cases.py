"""The cases and checks of the mesh decimation kernels (csrc/mesh_decimate.hip through rc_mvsnet_amd/mesh_decimate.py), shared by
tests/test_gpu_mesh_decimate.py (device "cuda:0") and tests/test_mesh_decimate_emu_cpu.py (the CPU emulation, device "cpu"),
against tests/mesh_decimate_oracle.py.  Every comparison is bit equality: cluster numbers, orders, keys, flags, counters, faces and
colours as integers, quadrics and positions as their bit patterns, a NaN equal to any NaN.  The only tolerances are those of the
properties that hold by construction (a vertex inside its cell up to the final rounding to fp32)."""
import functools

import numpy as np
import torch

import mesh_clean_cases as MCC
import mesh_decimate_oracle as O
from rc_mvsnet_amd import _lib, mesh_decimate as MD

INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
same_bits, to_dev, host = MCC.same_bits, MCC.to_dev, MCC.host


def same_bits64(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan])


def _colours(nv, seed):
    return np.random.default_rng(seed + 1).integers(0, 256, (nv, 3), dtype=np.uint8)


def _mesh(v, faces, seed=0):
    v = np.asarray(v, np.float32).reshape(-1, 3)
    return v, np.asarray(faces, np.int32).reshape(-1, 3), _colours(len(v), seed)


# ---- builders ---------------------------------------------------------------------------------------------------------------
def strip(nv, order="ascending"):
    """nv - 2 triangles along a zigzag strip of nv vertices 0.37 apart in x, numbered along it ascending, descending or shuffled:
    with cell = 1 some 0.37 nv cells on x and 2 on y, clusters of 1 to 3 members"""
    pos = np.arange(nv)
    number = {"ascending": pos, "descending": nv - 1 - pos, "shuffled": np.random.default_rng(nv).permutation(nv)}[order]
    p = np.zeros((nv, 3))
    p[number] = np.stack([0.37 * pos, 0.5 * (pos % 2), 0.1 * np.sin(pos)], 1)
    faces = np.stack([number[:-2], number[1:-1], number[2:]], 1)
    if order == "shuffled":
        faces = faces[np.random.default_rng(nv + 1).permutation(nv - 2)]
    return _mesh(p, faces, nv)


def specks(n):
    """n single triangles, each wholly inside a cell of its own (cell = 1): centres 3 apart on a 17 x 17 x ... grid, 0 faces out,
    n clusters of 3 members; the lattice has some 10^5 cells (3 radix passes)"""
    i = np.arange(n)
    centre = 3.0 * np.stack([i % 17, (i // 17) % 17, i // 289], 1)
    tri = np.array([[0.0, 0.0, 0.0], [0.3, 0.05, 0.1], [0.1, 0.3, -0.1]])
    p = (centre[:, None, :] + tri[None]).reshape(-1, 3)
    return _mesh(p, np.arange(3 * n).reshape(n, 3), n)


def patch_600_in_one_cell():
    """a 26 x 27 height field whose inner 24 x 25 vertices lie inside one cell (cell = 1) and whose rim lies in the cells around:
    one cluster of 600 members and some 3 600 corners"""
    x = np.concatenate([[-1.0], np.linspace(-0.45, 0.45, 24), [1.0]])
    y = np.concatenate([[-1.0], np.linspace(-0.45, 0.45, 25), [1.0]])
    rng = np.random.default_rng(600)
    gy, gx = np.meshgrid(y, x, indexing="ij")
    p = np.stack([gx.ravel(), gy.ravel(), 0.05 * rng.standard_normal(gx.size)], 1)
    idx = np.arange(gx.size).reshape(gx.shape)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    return _mesh(p, np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)]), 600)


def grid_sheet(m, z=0.0, spacing=0.5, first=0):
    idx = first + np.arange(m * m).reshape(m, m)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    y, x = np.divmod(np.arange(m * m), m)
    return np.stack([spacing * x, spacing * y, np.full(m * m, z)], 1), np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)])


def on_borders():
    """a 9 x 9 sheet 0.5 apart, cell = 1: the lattice starts at -0.5, so every second row and column lies exactly on a border"""
    p, f = grid_sheet(9)
    return _mesh(p, f, 9)


def two_sheets():
    """two sheets 0.25 apart with the same winding: under cell = 1 they fall into the same clusters and every face of the second
    repeats one of the first"""
    p0, f0 = grid_sheet(9, 0.0)
    p1, f1 = grid_sheet(9, 0.25, first=81)
    return _mesh(np.concatenate([p0, p1]), np.concatenate([f0, f1]), 81)


def duplicates():
    """four vertices in four cells; faces repeated in the same rotation class and in the opposite orientation"""
    p = [[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 2]]
    return _mesh(p, [(0, 1, 2), (1, 2, 0), (0, 2, 1), (2, 0, 1), (0, 1, 3), (2, 1, 0), (3, 0, 1)], 4)


def invalid_faces():
    v, f, rgb = MCC.invalid_faces()
    return v, f, rgb


def nonfinite():
    """NaN and infinite coordinates: their vertices are unclustered and every face that touches one is counted"""
    p, f = grid_sheet(6)
    p = p.copy()
    p[3] = [np.nan, 0.5, 0.0]
    p[8] = [0.5, np.inf, 0.0]
    p[20] = [-np.inf, np.nan, np.inf]
    p[35, 2] = -np.inf
    return _mesh(p, f, 6)


def all_nonfinite():
    return _mesh(np.full((4, 3), np.nan), [(0, 1, 2), (1, 2, 3), (0, 0, 1), (0, 1, 9)], 4)


def huge():
    """coordinates of the order 1e30 (cell = 1e30), one vertex at a denormal"""
    rng = np.random.default_rng(30)
    p = (3e30 * rng.standard_normal((40, 3))).astype(np.float32)
    p[7] = [1e-45, -1e-40, 0.0]
    return _mesh(p, rng.integers(0, 40, (90, 3)), 30)


def tiny():
    """coordinates of the order 1e-30 (cell = 1e-30) and denormals"""
    rng = np.random.default_rng(31)
    p = (3e-30 * rng.standard_normal((40, 3))).astype(np.float32)
    p[5] = [1e-45, -1e-40, -0.0]
    p[6] = [-1e-45, 1e-39, 1e-38]
    return _mesh(p, rng.integers(0, 40, (90, 3)), 31)


def minus_zero():
    """-0.0 and +0.0 both present as the smallest coordinate: the minimum is -0.0 in every bit"""
    p = [[0.0, -0.0, 0.0], [-0.0, 0.0, 1.0], [1.0, 0.0, -0.0], [1.0, 1.0, 1.0]]
    return _mesh(p, [(0, 1, 2), (1, 2, 3)], 2)


def lattice_2_21(extra=0):
    """two far-apart vertices and cell = 2^-10: exactly 2^21 cells on every axis (keys of 63 bits, 8 radix passes); extra = 1 puts
    the far vertex one cell further: refused"""
    far = (2 ** 21 - 1 + extra) / 1024.0
    return _mesh([[0, 0, 0], [far, far, far], [far, 0, 0], [0, far, 0]], [(0, 1, 2), (0, 3, 1)], 21)


def rounding_colours():
    """clusters of two whose channel sums are odd (x.5 rounds up), and of one"""
    p = [[0, 0, 0], [0.1, 0, 0], [2, 0, 0], [2.1, 0.1, 0], [0, 2, 0], [0.1, 2.1, 0], [5, 5, 5]]
    v, f, _ = _mesh(p, [(0, 2, 4), (1, 3, 5), (0, 3, 6)], 1)
    rgb = np.array([[1, 254, 0], [2, 255, 1], [7, 0, 255], [8, 1, 255], [100, 101, 3], [101, 104, 4], [9, 8, 7]], np.uint8)
    return v, f, rgb


PLAIN = {"cell": 1.0}
# name -> (builder, option sets of decimate; every set runs under both placements)
CASES = {
    "empty": (lambda: _mesh(np.zeros((0, 3)), np.zeros((0, 3))), [PLAIN]),
    "no_faces": (lambda: _mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]], np.zeros((0, 3))), [{"cell": 0.5}, {"cell": 0.5, "drop_unreferenced": False}]),
    "one_triangle": (lambda: _mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [(0, 1, 2)]), [{"cell": 0.6}, {"cell": 10.0}, {"cell": 10.0, "drop_unreferenced": False}]),
    "invalid_faces": (invalid_faces, [{"cell": 0.7}, {"cell": 0.7, "drop_unreferenced": False}]),
    "nonfinite": (nonfinite, [PLAIN, {"cell": 0.3}]),
    "all_nonfinite": (all_nonfinite, [PLAIN]),
    "huge": (huge, [{"cell": 1e30}, {"cell": 4e30}]),
    "tiny": (tiny, [{"cell": 1e-30}, {"cell": 3e-30}, {"cell": 1e30}]),
    "minus_zero": (minus_zero, [{"cell": 0.75}]),
    "on_borders": (on_borders, [PLAIN, {"cell": 1.0, "reg": 0.0}, {"cell": 0.5}]),
    "two_sheets": (two_sheets, [PLAIN]),
    "duplicates": (duplicates, [PLAIN, {"cell": 1.0, "drop_unreferenced": False}]),
    "rounding_colours": (rounding_colours, [PLAIN]),
    "patch_600_in_one_cell": (patch_600_in_one_cell, [PLAIN, {"cell": 1.0, "reg": 0.1}]),
    "specks_4097": (functools.partial(specks, 4097), [PLAIN]),
    "lattice_2_21": (lattice_2_21, [{"cell": 2.0 ** -10}]),
}
# the sort's 256-element blocks and the scan tiles of the (digit, block) table (2048 entries at exactly 8 blocks)
for _nv in (255, 256, 257, 2047, 2048, 2049, 4097):
    for _order in ("ascending", "descending", "shuffled"):
        CASES[f"strip_{_nv}_{_order}"] = (functools.partial(strip, _nv, _order), [PLAIN, {"cell": 0.25}] if _nv == 2049 else [PLAIN])

# what a case is there for, asserted on the oracle's result of its FIRST option set under quadric placement
KNOWN = {
    "empty": {"vertices_out": 0, "faces_out": 0, "clusters": 0},
    "no_faces": {"clusters": 5, "vertices_out": 0, "fallback_no_faces": 5},
    "one_triangle": {"faces_out": 1, "vertices_out": 3, "clusters": 3, "boundary_edges": 3},
    "invalid_faces": {"invalid_faces": 8},
    "nonfinite": {"unclustered_vertices": 4, "invalid_faces": 0},
    "all_nonfinite": {"unclustered_vertices": 4, "clusters": 0, "invalid_faces": 2, "unclustered_faces": 2, "faces_out": 0, "vertices_out": 0},
    "two_sheets": {"duplicate_faces": 32, "faces_out": 32, "clusters": 25},
    "duplicates": {"duplicate_faces": 4, "faces_out": 3, "collapsed_faces": 0},
    "patch_600_in_one_cell": {"clusters": 9, "faces_out": 8, "largest_cluster": 600, "corners_of_largest_cluster": 3600},
    "specks_4097": {"clusters": 4097, "faces_out": 0, "collapsed_faces": 4097, "vertices_out": 0},
    "lattice_2_21": {"clusters": 4, "faces_out": 2},
}
PASSES = {"strip_255_shuffled": 1, "strip_255_descending": 1, "strip_2049_shuffled": 2, "strip_4097_ascending": 2, "specks_4097": 3, "lattice_2_21": 8}      # ceil(bits(cells) / 8) of the first option set


@functools.lru_cache(maxsize=None)
def case(name):
    v, f, rgb = CASES[name][0]()
    for a in (v, f, rgb):
        a.setflags(write=False)
    return v, f, rgb


@functools.lru_cache(maxsize=None)
def reference(name, k, placement):
    v, f, rgb = case(name)
    return O.decimate(v, f, rgb, placement=placement, **CASES[name][1][k])


def known_value(name, key):
    """a KNOWN entry of a case: a stat of the oracle's result of its first option set under quadric placement, or one of the two
    figures of its largest cluster: its members (from cluster_start) and the face corners that contribute to its quadric"""
    _, _, _, wstats, parts = reference(name, 0, "quadric")
    if key not in ("largest_cluster", "corners_of_largest_cluster"):
        return wstats[key]
    cl = parts["cluster"]
    size = np.diff(cl["cluster_start"].astype(np.int64))
    if key == "largest_cluster":
        return int(size.max())
    contributing = parts["cface"][np.isin(parts["face_class"], (O.KEPT, O.COLLAPSED, O.DUPLICATE))]
    return int((contributing == int(size.argmax())).sum())


def case_keys():
    return [(name, k) for name in CASES for k in range(len(CASES[name][1]))]


def passes_of(lat):
    g = lat["dims"]
    return max(1, ((g[0] * g[1] * g[2]).bit_length() + 7) // 8)


# ---- properties that hold by construction -----------------------------------------------------------------------------------
def check_properties(v, f, out_v, out_f, parts, what):
    """on the result and the parts of one decimation (numpy arrays, from the oracle or from the device)"""
    lat, cl = parts["lattice"], parts["cluster"]
    cell = np.float64(lat["cell"])
    # every cluster vertex lies within its own cell, widened by the final rounding to fp32
    if cl["m"]:
        ctr = O.centres(cl, lat)
        cv = np.asarray(parts["cluster_verts"], np.float32)
        with np.errstate(all="ignore"):
            slack = np.spacing(np.abs(cv)).astype(np.float64) + 1e-12 * cell + 4 * np.spacing(np.abs(ctr))
            assert (np.abs(cv.astype(np.float64) - ctr) <= 0.5 * cell + slack).all(), what
    # no face with a repeated index, no two faces equal up to rotation
    assert ((out_f[:, 0] != out_f[:, 1]) & (out_f[:, 1] != out_f[:, 2]) & (out_f[:, 0] != out_f[:, 2])).all(), what
    rot = O.rotate_min_first(out_f)
    assert len(np.unique(rot, axis=0)) == len(rot), what
    # every output face is the image of an input face, in input order
    kept_ids = np.nonzero(parts["vert_keep"])[0]
    back = kept_ids[out_f] if len(out_f) else np.zeros((0, 3), np.int64)
    nv, i = len(v), 0
    for t in back:
        while i < len(f):
            a = f[i]
            i += 1
            if ((a >= 0) & (a < nv)).all() and np.array_equal(cl["cluster"][a], t):
                break
        else:
            raise AssertionError((what, "a face that is no image of a later input face", t.tolist()))
    assert out_f.size == 0 or (0 <= out_f.min() and out_f.max() < len(out_v)), what


# ---- the checks -----------------------------------------------------------------------------------------------------------
def device_parts(dev, v, f, rgb, lat, placement, reg):
    """the parts called on their own -> the dict of numpy arrays that O.decimate returns as parts"""
    tv, tf, tc = to_dev(dev, v, f, rgb)
    cl = MD.cluster(tv, lat)
    fc = MD.classify_faces(len(v), tf, cl)
    quad = MD.quadrics(tv, tf, cl, lat) if placement == "quadric" else None
    cv, crgb, via, pcounts = MD.place(tv, tc, cl, lat, quad, placement, reg)
    return {"cluster": {k: (host(x) if torch.is_tensor(x) else x) for k, x in cl.items()}, "cface": host(fc["cface"]), "face_class": host(fc["face_class"]),
            "fcounts": host(fc["counts"]).tolist(), "quad": None if quad is None else host(quad), "cluster_verts": host(cv),
            "cluster_rgb": None if crgb is None else host(crgb), "via": host(via), "pcounts": host(pcounts).tolist()}


def check_case(dev, name, k, twice=False):
    """decimate with option set k of the case under both placements, and its parts: everything equal to the oracle's in every bit"""
    v, f, rgb = case(name)
    opts = CASES[name][1][k]
    for placement in ("quadric", "mean"):
        what = (name, opts, placement)
        wv, wf, wc, wstats, wparts = reference(name, k, placement)
        if k == 0 and placement == "quadric":
            for key, value in KNOWN.get(name, {}).items():
                assert known_value(name, key) == value, (name, key, known_value(name, key), value)
            if name in PASSES:
                assert passes_of(wparts["lattice"]) == PASSES[name], (name, wparts["lattice"])
        check_properties(v, f, wv, wf, wparts, what)
        tv, tf, tc = to_dev(dev, v, f, rgb)
        lo, hi, finite = MD.bounds(tv)
        assert finite == wparts["finite"] and (finite == 0 or (same_bits(lo, wparts["lo"]) and same_bits(hi, wparts["hi"]))), what
        if finite:
            lat = MD.lattice(lo, hi, opts["cell"])
            assert lat == wparts["lattice"], (what, lat, wparts["lattice"])
            got = device_parts(dev, v, f, rgb, lat, placement, opts.get("reg", O.DEFAULT_REG))
            wcl = wparts["cluster"]
            for key in ("cluster", "order", "cluster_start"):
                assert np.array_equal(got["cluster"][key], wcl[key]), (what, key)
            assert np.array_equal(got["cluster"]["cluster_key"].view(np.uint64), wcl["cluster_key"]) and got["cluster"]["m"] == wcl["m"], what
            assert np.array_equal(got["cface"], wparts["cface"]) and np.array_equal(got["face_class"], wparts["face_class"]), what
            if placement == "quadric":
                assert same_bits64(got["quad"], wparts["quad"]), what
            assert np.array_equal(got["via"], wparts["via"]), (what, got["via"].tolist(), wparts["via"].tolist())
            assert same_bits(got["cluster_verts"], wparts["cluster_verts"]) and np.array_equal(got["cluster_rgb"], wparts["cluster_rgb"]), what
        gv, gf, gc, gstats = MD.decimate(tv, tf, tc, placement=placement, **opts)
        print(f"{name} {opts} {placement}: {gstats}")
        assert gv.dtype == torch.float32 and gf.dtype == torch.int32 and gc.dtype == torch.uint8
        assert gstats == wstats, (what, gstats, wstats)
        assert same_bits(host(gv), wv) and np.array_equal(host(gf), wf) and np.array_equal(host(gc), wc), what
        plain = MD.decimate(tv, tf, None, placement=placement, **opts)
        assert plain[2] is None and plain[3] == gstats and torch.equal(plain[0].view(torch.int32), gv.view(torch.int32)) and torch.equal(plain[1], gf)
        if twice:
            again = MD.decimate(*to_dev(dev, v, f, rgb), placement=placement, **opts)
            assert again[3] == gstats and torch.equal(again[0].view(torch.int32), gv.view(torch.int32)) and torch.equal(again[1], gf) and \
                torch.equal(again[2], gc), what


def check_refusals(dev):
    """one cell too many on an axis, named; bad arguments of the module"""
    v, f, rgb = lattice_2_21(extra=1)
    tv, tf, tc = to_dev(dev, v, f, rgb)
    for axis in "xyz":
        sub = torch.zeros((2, 3)).to(tv.device)
        sub[1, "xyz".index(axis)] = float(v[1, 0])
        try:
            MD.decimate(sub, tf[:0], None, cell=2.0 ** -10)
        except _lib.RcmvsError as e:
            assert f"axis {axis}" in str(e) and "2097153 cells" in str(e), str(e)
        else:
            raise AssertionError(f"2^21 + 1 cells on {axis} were accepted")
    try:
        O.decimate(v, f, rgb, cell=2.0 ** -10)
    except O.Refused as e:
        assert "axis x" in str(e)
    else:
        raise AssertionError("the oracle accepted 2^21 + 1 cells")
    for kw, pattern in (({"cell": 0.0}, "cell"), ({"cell": -1.0}, "cell"), ({"cell": float("nan")}, "cell"), ({"cell": float("inf")}, "cell"),
                        ({"cell": 1.0, "reg": -1e-3}, "reg"), ({"cell": 1.0, "reg": float("nan")}, "reg"), ({"cell": 1.0, "placement": "median"}, "placement"),
                        ({"cell": 1e-30}, "cells on axis")):
        try:
            MD.decimate(tv, tf, tc, **kw)
        except _lib.RcmvsError as e:
            assert pattern in str(e), (kw, str(e))
        else:
            raise AssertionError(f"{kw} was accepted")


def check_identity_when_every_vertex_is_alone(dev):
    """mean placement with a cell so small that every vertex has its own: the input mesh compacted and reordered by key, positions
    and colours bit for bit"""
    v, f, rgb = case("strip_2049_shuffled")
    v = v.copy()
    v[7] = [-0.0, 0.5, 1e-45]                                     # bits that arithmetic would not give back
    f = np.concatenate([f, [[0, 1, 1], [0, 1, 5000]]]).astype(np.int32)
    tv, tf, tc = to_dev(dev, v, f, rgb)
    gv, gf, gc, stats = MD.decimate(tv, tf, tc, cell=1e-3, placement="mean")
    _, _, _, wstats, parts = O.decimate(v, f, rgb, cell=1e-3, placement="mean")
    cl = parts["cluster"]
    assert stats == wstats and stats["clusters"] == len(v) == stats["vertices_out"] and stats["faces_out"] == len(f) - 2 and stats["invalid_faces"] == 2
    assert same_bits(host(gv), v[cl["order"]]) and np.array_equal(host(gc), rgb[cl["order"]])
    assert np.array_equal(host(gf), cl["cluster"][f[:-2]])
    kv, kf, kc, kstats = MCC.O.clean_mesh(v, f, rgb)                 # the compaction of mesh_clean keeps input order: the same set of records
    assert {r.tobytes() for r in MCC.bits(kv)} == {r.tobytes() for r in MCC.bits(host(gv))} and kstats["faces_out"] == stats["faces_out"]


# ---- a real extraction ------------------------------------------------------------------------------------------------------
def check_extraction(dev):
    """the two spheres and the speck of mesh_clean_cases.check_extraction, decimated at 2 and 3 voxels under both placements"""
    verts, faces, rgb = MCC.scene_volume(dev).extract(1)
    v, f, c = host(verts), host(faces), host(rgb)
    for voxels in (2.0, 3.0):
        for placement in ("quadric", "mean"):
            wv, wf, wc, wstats, wparts = O.decimate(v, f, c, cell=voxels, placement=placement)
            gv, gf, gc, gstats = MD.decimate(verts, faces, rgb, cell=voxels, placement=placement)
            print(f"extraction {voxels} {placement}: {gstats}")
            assert gstats == wstats and same_bits(host(gv), wv) and np.array_equal(host(gf), wf) and np.array_equal(host(gc), wc), (voxels, placement)
            check_properties(v, f, wv, wf, wparts, ("extraction", voxels, placement))
            assert 0 < gstats["faces_out"] < gstats["faces_in"] / 3 and gstats["invalid_faces"] == 0 and gstats["unclustered_vertices"] == 0


# ---- end to end -------------------------------------------------------------------------------------------------------------
def check_end_to_end(dev, tmp_path, sparse):
    """mesh_scan(..., decimate_voxels=2) on the small scan of tsdf_cases.check_end_to_end, dense or sparse: the PLY is the oracle's
    decimation of the mesh mesh_scan writes without the option, colours included, and the summary carries the stats; without the
    option (decimate_options answering None) the PLY and the summary are what they were"""
    import unittest.mock as mock
    import tsdf_cases as C
    from rc_mvsnet_amd import dtu_io, tsdf_mesh as TM
    pair_folder, out_folder = C.write_scan(tmp_path)
    raw, again, ply = (str(tmp_path / "out" / n) for n in ("raw.ply", "again.ply", "decimated.ply"))
    kw = dict(resolution=32, device=dev, sparse=sparse)
    plain = TM.mesh_scan(pair_folder, out_folder, out_folder, raw, C.PROB, C.NCONS, C.DIST, C.DEPTH, **kw)
    with mock.patch.object(MD, "decimate_options", lambda *a, **k: None):
        off = TM.mesh_scan(pair_folder, out_folder, out_folder, again, C.PROB, C.NCONS, C.DIST, C.DEPTH, decimate_voxels=2, **kw)
    assert open(raw, "rb").read() == open(again, "rb").read() and dict(off, mesh=raw) == plain and "decimate" not in plain
    summary = TM.mesh_scan(pair_folder, out_folder, out_folder, ply, C.PROB, C.NCONS, C.DIST, C.DEPTH, decimate_voxels=2, **kw)
    assert set(summary) == set(plain) | {"decimate"}
    verts, faces, rgb = dtu_io.read_ply_mesh_rgb(raw)
    wv, wf, wc, wstats, _ = O.decimate(verts, faces, rgb, cell=2 * plain["voxel"])
    gv, gf, gc = dtu_io.read_ply_mesh_rgb(ply)
    print("end to end:", summary["decimate"])
    assert summary["decimate"] == wstats and 0 < wstats["faces_out"] < wstats["faces_in"] and wstats["cell"] == 2 * summary["voxel"]
    assert same_bits(gv, wv) and np.array_equal(gf, wf) and np.array_equal(gc, wc)
    assert summary["vertices"] == len(gv) == wstats["vertices_out"] and summary["faces"] == len(gf) == wstats["faces_out"]
    assert {k: v for k, v in summary.items() if k not in ("decimate", "mesh", "vertices", "faces", "unreferenced_vertices")} == \
           {k: v for k, v in plain.items() if k not in ("mesh", "vertices", "faces", "unreferenced_vertices")}
    return pair_folder, out_folder, summary
