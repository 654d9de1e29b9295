"""The cases and checks of the mesh clean-up kernels (csrc/mesh_clean.hip through rc_mvsnet_amd/mesh_clean.py), shared by
tests/test_gpu_mesh_clean.py (device "cuda:0") and tests/test_mesh_clean_emu_cpu.py (the CPU emulation, device "cpu"), against
tests/mesh_clean_oracle.py.  Every comparison is bit equality: labels, flags, counts, ranks, neighbours, multiplicities, faces
and colours as integers, positions as their 32-bit patterns, a NaN equal to any NaN.  There are no tolerances."""
import functools

import numpy as np
import torch

import mesh_clean_oracle as O
import tsdf_cases as C
from rc_mvsnet_amd import _lib, dtu_io, fusion, mesh_clean as MC, tsdf_mesh as TM

TILE, LIMIT = MC.SCAN_TILE, MC.SORT_LIMIT
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    """equal in every bit, NaNs compared as NaNs (the sign and payload of a NaN that an operation produces are the processor's)"""
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


def _positions(nv, seed):
    return np.random.default_rng(seed).standard_normal((nv, 3)).astype(np.float32)


def _colours(nv, seed):
    return np.random.default_rng(seed + 1).integers(0, 256, (nv, 3), dtype=np.uint8)


def _mesh(nv, faces, seed=0):
    return _positions(nv, seed), np.asarray(faces, np.int32).reshape(-1, 3), _colours(nv, seed)


# ---- builders ---------------------------------------------------------------------------------------------------------------
def strip(n, descending=True, shuffle_seed=None):
    """n triangles (p, p + 1, p + 2) along a strip of n + 2 vertices whose numbers run descending along it: every hook links a root
    under the next smaller vertex, the longest parent chains a union-find can build"""
    pos = np.arange(n + 2)
    number = (n + 1 - pos) if descending else pos
    faces = np.stack([number[:-2], number[1:-1], number[2:]], 1)
    if shuffle_seed is not None:
        rng = np.random.default_rng(shuffle_seed)
        faces = rng.permutation(n + 2)[faces][rng.permutation(n)]
    return _mesh(n + 2, faces, n)


def specks_and_fan(n, extra_verts=0, fan_at=1000):
    """n isolated triangles and one open fan of 10 faces, the fan's vertices numbered after the first min(fan_at, n) triangles,
    extra_verts unreferenced vertices at the end"""
    k = min(fan_at, n)
    tri = lambda first, count: first + np.arange(3 * count).reshape(count, 3)          # noqa: E731
    c = 3 * k
    fan = np.stack([np.full(10, c), c + 1 + np.arange(10), c + 2 + np.arange(10)], 1)
    faces = np.concatenate([tri(0, k), fan, tri(c + 12, n - k)])
    return _mesh(3 * n + 12 + extra_verts, faces, n)


def fan(n, closed=False):
    """n triangles round vertex 0: its segment of the 1-ring has 2 n entries"""
    ring = 1 + np.arange(n)
    nxt = 1 + (np.arange(n) + 1) % n if closed else ring + 1
    return _mesh(n + 1 if closed else n + 2, np.stack([np.zeros(n, np.int64), ring, nxt], 1), n)


def tet_strip(k, drop_face=None):
    """the boundary of k tetrahedra (i, i+1, i+2, i+3) glued face to face: a closed surface of Euler characteristic 2; drop_face
    removes one triangle and leaves a hole of three boundary edges"""
    count = {}
    for i in range(k):
        for tri in ((i, i + 1, i + 2), (i, i + 1, i + 3), (i, i + 2, i + 3), (i + 1, i + 2, i + 3)):
            count[tri] = count.get(tri, 0) + 1
    faces = [t for t, c in sorted(count.items()) if c == 1]
    if drop_face is not None:
        del faces[drop_face]
    return _mesh(k + 3, faces, k)


def grid_patch(m):
    """an m x m-vertex height field, two triangles per cell: an open surface, its rim on boundary edges"""
    idx = np.arange(m * m).reshape(m, m)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    v, f, rgb = _mesh(m * m, np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)]), m)
    y, x = np.divmod(np.arange(m * m), m)
    v = (np.stack([x, y, np.zeros(m * m)], 1) + 0.2 * v).astype(np.float32)
    return v, f, rgb


def hostile_positions():
    v, f, rgb = tet_strip(12)
    v = v.copy()
    v[1] = [np.nan, 1.0, -1.0]
    v[4] = [np.inf, -np.inf, 0.0]
    v[7] = [1e30, -1e30, 3e38]
    v[9] = [1e-45, -1e-40, -0.0]
    v[12] = [3.4e38, 3.4e38, -3.4e38]
    return v, f, rgb


def invalid_faces():
    nv = 9
    faces = [(0, 1, 2), (3, 3, 4), (2, 3, 4), (5, 6, 5), (-1, 0, 1), (0, nv, 1), (4, 5, INT_MAX), (INT_MIN, 1, 2), (6, 7, 7), (6, 7, 8), (0, 0, 0)]
    return _mesh(nv, faces, 3)


def all_invalid():
    return _mesh(4, [(0, 0, 1), (1, 2, 4), (-1, 2, 3), (INT_MAX, INT_MIN, 0)], 4)


def unreferenced():
    """vertices 0, 1 (start), 5, 6 (middle) and 10, 11 (end) belong to no face"""
    return _mesh(12, [(2, 3, 4), (3, 4, 7), (8, 9, 7)], 5)


def nonmanifold(n):
    return _mesh(2 + n, [(0, 1, 2 + i) for i in range(n)], n)


DEFAULT = {}
# name -> (builder, option sets of clean_mesh)
CASES = {
    "nf_0": (lambda: _mesh(5, np.zeros((0, 3)), 1), [DEFAULT, {"drop_unreferenced": False, "smooth_iterations": 1}]),
    "nv_0": (lambda: _mesh(0, np.zeros((0, 3)), 1), [DEFAULT, {"keep_largest": 1, "smooth_iterations": 1}]),
    "nv_0_with_faces": (lambda: _mesh(0, [(0, 1, 2), (0, 0, 0)], 1), [DEFAULT]),
    "one_triangle": (lambda: _mesh(3, [(0, 1, 2)], 2), [DEFAULT, {"smooth_iterations": 1, "pin_boundary": False}]),
    "share_vertex": (lambda: _mesh(5, [(0, 1, 2), (2, 3, 4)], 2), [DEFAULT, {"min_faces": 2}]),
    "share_edge": (lambda: _mesh(4, [(0, 1, 2), (2, 1, 3)], 2), [DEFAULT, {"min_faces": 2}]),
    "disjoint": (lambda: _mesh(6, [(0, 1, 2), (3, 4, 5)], 2), [DEFAULT, {"min_faces": 2}, {"keep_largest": 1}]),
    "invalid_faces": (invalid_faces, [DEFAULT, {"drop_unreferenced": False}, {"keep_largest": 1}]),
    "all_invalid": (all_invalid, [DEFAULT, {"drop_unreferenced": False}]),
    "unreferenced": (unreferenced, [DEFAULT, {"drop_unreferenced": False}, {"keep_largest": 1}, {"keep_largest": 1, "drop_unreferenced": False}]),
    "strip_descending": (lambda: strip(5000), [DEFAULT]),
    "strip_shuffled": (lambda: strip(5000, shuffle_seed=11), [DEFAULT]),
    "fan_300": (lambda: fan(300, closed=True), [DEFAULT, {"smooth_iterations": 1, "pin_boundary": False}]),
    "fan_at_limit": (lambda: fan(LIMIT // 2), [DEFAULT, {"smooth_iterations": 1, "pin_boundary": False}]),
    "fan_past_limit": (lambda: fan(LIMIT // 2 + 1), [DEFAULT, {"smooth_iterations": 1, "pin_boundary": False}]),
    "nonmanifold_3": (lambda: nonmanifold(3), [DEFAULT]),
    "nonmanifold_4": (lambda: nonmanifold(4), [DEFAULT, {"smooth_iterations": 2}]),
    "tets_closed": (lambda: tet_strip(9), [DEFAULT, {"smooth_iterations": 3}]),
    "tets_hole": (lambda: tet_strip(9, drop_face=7), [DEFAULT, {"smooth_iterations": 3}, {"smooth_iterations": 3, "pin_boundary": False}]),
    "grid_patch": (lambda: grid_patch(19), [{"smooth_iterations": 1}, {"smooth_iterations": 3}, {"smooth_iterations": 3, "pin_boundary": False},
                                            {"smooth_iterations": 2, "lam": 0.33, "mu": -0.34}, {"smooth_iterations": 1, "lam": 0.0, "mu": 0.0}]),
    "hostile_positions": (hostile_positions, [{"smooth_iterations": 1}, {"smooth_iterations": 3}, {"smooth_iterations": 3, "pin_boundary": False},
                                              {"smooth_iterations": 1, "lam": 0.9, "mu": -1.1}]),
}
SELECT = [{"min_faces": 2}, {"keep_largest": 1}, {"keep_largest": 3}, {"min_fraction": 0.5}]
# the scans' tiles: faces = n + 10 and vertices = 3 n + 12 (+ extra) at a tile, one short of it, one past it, and across two tiles
for _name, _n, _extra in (("tiles_4097", 4097, 0), ("tiles_faces_tile_minus_1", TILE - 11, 0), ("tiles_faces_tile", TILE - 10, 0),
                          ("tiles_faces_tile_plus_1", TILE - 9, 0), ("tiles_verts_tile_minus_1", 678, TILE - 1 - 2046), ("tiles_verts_tile", 678, TILE - 2046),
                          ("tiles_verts_tile_plus_1", 678, TILE + 1 - 2046)):
    CASES[_name] = (functools.partial(specks_and_fan, _n, _extra), SELECT + ([DEFAULT, {"drop_unreferenced": False, "keep_largest": 3}] if _extra else []))

# what a case is there for, asserted on the oracle's result of its FIRST option set
KNOWN = {
    "one_triangle": {"components_in": 1, "boundary_edges": 3, "edges": 3, "euler_characteristic": 1},
    "share_vertex": {"components_in": 1, "faces_out": 2},
    "share_edge": {"components_in": 1, "boundary_edges": 4, "edges": 5},
    "disjoint": {"components_in": 2, "faces_out": 2},
    "invalid_faces": {"invalid_faces": 8, "faces_out": 3},
    "all_invalid": {"invalid_faces": 4, "faces_out": 0, "vertices_out": 0, "components_in": 0},
    "unreferenced": {"unreferenced_removed": 6, "vertices_out": 6},
    "strip_descending": {"components_in": 1, "faces_out": 5000, "euler_characteristic": 1},
    "strip_shuffled": {"components_in": 1, "faces_out": 5000, "euler_characteristic": 1},
    "nonmanifold_3": {"nonmanifold_edges": 1, "boundary_edges": 6},
    "nonmanifold_4": {"nonmanifold_edges": 1, "boundary_edges": 8},
    "tets_closed": {"boundary_edges": 0, "euler_characteristic": 2, "nonmanifold_edges": 0},
    "tets_hole": {"boundary_edges": 3, "euler_characteristic": 1},
    "tiles_4097": {"components_in": 4098, "components_kept": 1, "faces_out": 10, "largest_component_faces": 10},
}


@functools.lru_cache(maxsize=None)
def case(name):
    v, f, rgb = CASES[name][0]()
    for a in (v, f, rgb):
        a.setflags(write=False)
    return v, f, rgb


@functools.lru_cache(maxsize=None)
def reference(name, k):
    """the oracle's clean_mesh of option set k of a case, and the oracle's parts of the input mesh"""
    v, f, rgb = case(name)
    return O.clean_mesh(v, f, rgb, **CASES[name][1][k])


def to_dev(dev, v, f, rgb):
    return (torch.from_numpy(np.array(v)).to(dev), torch.from_numpy(np.array(f)).to(dev), None if rgb is None else torch.from_numpy(np.array(rgb)).to(dev))


def host(t):
    return t.cpu().numpy()


def compare_adjacency(got, want, what):
    n = want["defined"]
    for k in ("row_start", "row_len", "on_boundary"):
        assert np.array_equal(host(got[k]), want[k]), (what, k)
    for k in ("nbr", "mult"):
        assert np.array_equal(host(got[k])[:n], want[k][:n]), (what, k)
    for k in ("edges", "boundary_edges", "nonmanifold_edges", "referenced_vertices"):
        assert got[k] == want[k], (what, k, got[k], want[k])


def check_parts(dev, name):
    """components and the 1-ring of the case's input mesh, each called on its own: every array equal to the oracle's"""
    v, f, rgb = case(name)
    tv, tf, _ = to_dev(dev, v, f, rgb)
    label, ok, comp_faces, invalid = O.components(len(v), f)
    assert np.array_equal(label, O.components(len(v), f, use_scipy=False)[0])            # the two restatements agree
    comp = MC.components(tv, tf)
    assert np.array_equal(host(comp["label"]), label) and np.array_equal(host(comp["face_ok"]), ok), name
    assert np.array_equal(host(comp["comp_faces"]), comp_faces) and int(comp["counts"][0]) == invalid, name
    table, most = MC.component_table(comp)
    want_table = O.component_table(label, comp_faces)
    assert np.array_equal(host(table), want_table) and most == (int(want_table[:, 1].max()) if len(want_table) else 0), name
    adj, want = MC.adjacency(len(v), tf), O.adjacency(len(v), f)
    compare_adjacency(adj, want, name)
    heavy = int(((want["row_start"][1:] - want["row_start"][:-1]) > LIMIT).sum())
    assert adj["long_segments"] == heavy, name
    if name == "fan_300":
        assert heavy == 1 and int(want["row_len"][0]) == 300
    if name == "fan_at_limit":
        assert heavy == 0 and int(want["row_start"][1]) == LIMIT
    if name == "fan_past_limit":
        assert heavy == 1 and int(want["row_start"][1]) == LIMIT + 2                   # a segment's length is even: two entries per face


def check_scan_third_level(dev):
    """rcmvs_mc_component_table on TILE * TILE + TILE + 1 vertices that are all roots: the smallest scan whose upper two levels run
    two workgroups, the second partly filled, over two top sums.  Flags, ranks and totals against torch.cumsum in int64."""
    nv = TILE * TILE + TILE + 1
    v = torch.arange(nv, device=dev, dtype=torch.int32)
    label, comp_faces = v, torch.where(v % 3 == 0, 1 + v % 5, torch.zeros_like(v))
    want_flags = comp_faces > 0
    want_rank = torch.cumsum(want_flags.to(torch.int64), 0) - want_flags.to(torch.int64)
    count = int(want_flags.sum())

    def run():
        flags, rank = torch.empty(nv, device=dev, dtype=torch.uint8), torch.empty(nv + 1, device=dev, dtype=torch.int32)
        totals, work = torch.empty(2, device=dev, dtype=torch.int64), MC._scan_work(nv, dev)
        _lib.call("rcmvs_mc_component_table", MC._ptr(label, "label", torch.int32), MC._ptr(comp_faces, "comp_faces", torch.int32), nv,
                  MC._ptr(flags, "flags", torch.uint8), MC._ptr(rank, "rank", torch.int32), MC._ptr(work, "scan_work", torch.int32),
                  MC._ptr(None, "table", torch.int32), 0, MC._ptr(totals, "totals", torch.int64), fusion._stream())
        return flags, rank, totals

    flags, rank, totals = run()
    print(f"third level: nv = {nv}, flagged = {count}, totals = {totals.tolist()}, rank[nv] = {int(rank[nv])}")
    assert count == (nv + 2) // 3 and torch.equal(flags, want_flags.to(torch.uint8))
    assert torch.equal(rank[:nv].to(torch.int64), want_rank)
    assert int(rank[nv]) == count and totals.tolist() == [count, 5]
    assert all(torch.equal(a, b) for a, b in zip(run(), (flags, rank, totals)))


def check_clean(dev, name, k, twice=False):
    """clean_mesh with option set k of the case: positions, faces, colours and every count equal to the oracle's"""
    v, f, rgb = case(name)
    opts = CASES[name][1][k]
    wv, wf, wc, wstats = reference(name, k)
    if k == 0:
        for key, value in KNOWN.get(name, {}).items():
            assert wstats[key] == value, (name, key, wstats[key], value)
    if name.startswith("tiles") and opts == {"keep_largest": 3}:
        assert wstats["components_kept"] == 3 and wstats["faces_out"] == 12 and np.array_equal(wf[:2], [[0, 1, 2], [3, 4, 5]])     # ties: the smaller labels
    got = MC.clean_mesh(*to_dev(dev, v, f, rgb), **opts)
    gv, gf, gc, gstats = got
    print(f"{name} {opts}: {gstats}")
    assert gv.dtype == torch.float32 and gf.dtype == torch.int32 and gc.dtype == torch.uint8
    assert gstats == wstats, (name, opts, gstats, wstats)
    if not same_bits(host(gv), wv):
        rows = np.nonzero((bits(host(gv)) != bits(wv)).any(1))[0]
        print("positions differ at", rows.tolist(), "got", bits(host(gv))[rows].tolist(), "want", bits(wv)[rows].tolist())
    assert same_bits(host(gv), wv) and np.array_equal(host(gf), wf) and np.array_equal(host(gc), wc), (name, opts)
    plain = MC.clean_mesh(*to_dev(dev, v, f, None), **opts)
    assert plain[2] is None and torch.equal(plain[0].view(torch.int32), gv.view(torch.int32)) and torch.equal(plain[1], gf)      # same device: NaN bits too
    if twice:
        again = MC.clean_mesh(*to_dev(dev, v, f, rgb), **opts)
        assert again[3] == gstats and torch.equal(again[0].view(torch.int32), gv.view(torch.int32)) and torch.equal(again[1], gf) and torch.equal(again[2], gc)


def case_keys():
    return [(name, k) for name in CASES for k in range(len(CASES[name][1]))]


def check_smoothing_parts(dev):
    """taubin on its own: iterations = 0 and lam = mu = 0 return the input in every bit, pinned vertices never move, and the
    input tensor is not written"""
    v, f, _ = case("grid_patch")
    tv, tf, _ = to_dev(dev, v, f, None)
    adj = MC.adjacency(len(v), tf)
    keep = tv.clone()
    for kw in ({"iterations": 0}, {"iterations": 2, "lam": 0.0, "mu": 0.0}):
        out = MC.taubin(tv, adj, **kw)
        assert out.data_ptr() != tv.data_ptr() and same_bits(host(out), v), kw
    out = MC.taubin(tv, adj, 3)
    pinned = host(adj["on_boundary"]) != 0
    assert pinned.sum() == 4 * 18 and same_bits(host(out)[pinned], v[pinned]) and not np.array_equal(bits(host(out)[~pinned]), bits(v[~pinned]))
    assert same_bits(host(out), O.taubin(v, O.adjacency(len(v), f), 3)) and torch.equal(tv, keep)


# ---- a real extraction ------------------------------------------------------------------------------------------------------
SCENE_DIMS, SCENE_GRID = (20, 13, 13), C.UNIT
SCENE_SPHERES = (((6.2, 6.4, 6.6), 4.1), ((15.4, 6.3, 6.1), 2.6), ((11.3, 2.2, 2.4), 0.9))        # two spheres and a speck


def scene_volume(dev):
    f = np.minimum.reduce([C.sphere_field(SCENE_DIMS, SCENE_GRID, c, r) for c, r in SCENE_SPHERES])
    rng = np.random.default_rng(7)
    csum = [rng.integers(0, 256, f.size).astype(np.float32) for _ in range(3)]
    return C.load_volume(dev, SCENE_DIMS, SCENE_GRID, f.astype(np.float32).ravel(), np.ones(f.size, np.float32), csum)


def check_extraction(dev):
    """two spheres of different radius and a speck in one volume: three closed components; keep_largest = 1 leaves the large sphere,
    closed, of Euler characteristic 2, every surviving vertex record, colour and face equal to the oracle's"""
    verts, faces, rgb = scene_volume(dev).extract(1)
    v, f, c = host(verts), host(faces), host(rgb)
    for opts in ({"keep_largest": 1}, {"min_fraction": 0.2, "smooth_iterations": 2}, {}):
        wv, wf, wc, wstats = O.clean_mesh(v, f, c, **opts)
        gv, gf, gc, gstats = MC.clean_mesh(verts, faces, rgb, **opts)
        print(f"extraction {opts}: {gstats}")
        assert gstats == wstats and same_bits(host(gv), wv) and np.array_equal(host(gf), wf) and np.array_equal(host(gc), wc), opts
        assert gstats["components_in"] == 3 and gstats["boundary_edges"] == 0 and gstats["nonmanifold_edges"] == 0 and gstats["invalid_faces"] == 0
        if opts == {"keep_largest": 1}:
            assert gstats["components_kept"] == 1 and gstats["euler_characteristic"] == 2 and 0 < gstats["faces_out"] < gstats["faces_in"]
            centre, radius = SCENE_SPHERES[0]
            assert np.abs(np.linalg.norm(host(gv).astype(np.float64) - np.asarray(centre), axis=1) - radius).max() < np.sqrt(3.0)
            records = {r.tobytes() for r in np.concatenate([bits(v), c.astype(np.uint32)], 1)}
            assert all(r.tobytes() in records for r in np.concatenate([bits(host(gv)), host(gc).astype(np.uint32)], 1))      # colours carried through
        elif opts:
            assert gstats["components_kept"] == 2 and gstats["euler_characteristic"] == 4
        else:
            assert gstats["components_kept"] == 3 and gstats["euler_characteristic"] == 6 and gstats["faces_out"] == gstats["faces_in"]


# ---- end to end -------------------------------------------------------------------------------------------------------------
def check_end_to_end(dev, tmp_path):
    """mesh_scan(..., keep_largest=1, smooth=2) on the small scan of tsdf_cases.check_end_to_end: the PLY is the oracle's clean-up
    of the mesh mesh_scan writes without the options, and the summary carries the stats"""
    pair_folder, out_folder = C.write_scan(tmp_path)
    raw, ply = str(tmp_path / "out" / "raw.ply"), str(tmp_path / "out" / "clean.ply")
    plain = TM.mesh_scan(pair_folder, out_folder, out_folder, raw, C.PROB, C.NCONS, C.DIST, C.DEPTH, resolution=48, device=dev)
    summary = TM.mesh_scan(pair_folder, out_folder, out_folder, ply, C.PROB, C.NCONS, C.DIST, C.DEPTH, resolution=48, device=dev, keep_largest=1, smooth=2)
    assert "clean" not in plain and set(summary) == set(plain) | {"clean"}
    verts, faces = dtu_io.read_ply_mesh(raw)
    wv, wf, _, wstats = O.clean_mesh(verts, faces, None, keep_largest=1, smooth_iterations=2)
    gv, gf = dtu_io.read_ply_mesh(ply)
    print("end to end:", summary["clean"])
    assert summary["clean"] == wstats and wstats["components_kept"] == 1 and wstats["faces_out"] > 1000 and wstats["smooth_iterations"] == 2
    assert same_bits(gv, wv) and np.array_equal(gf, wf)
    assert summary["vertices"] == len(gv) == wstats["vertices_out"] and summary["faces"] == len(gf) and summary["unreferenced_vertices"] == 0
    assert {k: v for k, v in summary.items() if k not in ("clean", "mesh", "vertices", "faces", "unreferenced_vertices")} == \
           {k: v for k, v in plain.items() if k not in ("mesh", "vertices", "faces", "unreferenced_vertices")}
