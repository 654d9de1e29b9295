"""The cases and checks of the hole-filling kernels (csrc/mesh_holes.hip through rc_mvsnet_amd/mesh_holes.py), shared by
tests/test_gpu_mesh_holes.py (device "cuda:0") and tests/test_mesh_holes_emu_cpu.py (the CPU emulation, device "cpu"), against
tests/mesh_holes_oracle.py.  Every comparison is bit equality as in tests/mesh_clean_cases.py: successors, flags, counts, faces
and colours as integers, positions as their 32-bit patterns, a NaN equal to any NaN.  The one tolerance, of the area check on the
flat grid, is derived next to its assert."""
import functools

import numpy as np
import torch

import mesh_clean_cases as MCC
import mesh_holes_oracle as O
import tsdf_cases as C
import tsdf_oracle as TO
from mesh_clean_cases import INT_MAX, INT_MIN, _mesh, bits, host, same_bits, to_dev
from rc_mvsnet_amd import _lib, dtu_io, mesh_clean as MC, mesh_holes as MH, tsdf_mesh as TM

TILE = MH.SCAN_TILE


# ---- builders ---------------------------------------------------------------------------------------------------------------
def relabel(mesh, perm):
    """the same mesh with vertex i renamed perm[i]"""
    v, f, rgb = mesh
    perm = np.asarray(perm)
    out_v, out_c = np.empty_like(v), np.empty_like(rgb)
    out_v[perm], out_c[perm] = v, rgb
    return out_v, perm[f].astype(np.int32), out_c


def fan_numbered(n, how):
    """an open fan of n triangles, its rim a loop of n + 2 edges through every vertex, under four numberings of the same vertices"""
    nv = n + 2
    perm = {"ascending": np.arange(nv), "descending": nv - 1 - np.arange(nv), "shuffled": np.random.default_rng(5).permutation(nv),
            "rotated": (np.arange(nv) + nv // 2) % nv}[how]                  # rotated: the smallest number in the middle of the rim
    return relabel(MCC.fan(n), perm)


def flat_grid(rows, cols, removed=(), h=np.float32(0.1)):
    """rows x cols vertices at (h i, h j, 0), two triangles per cell, without the cells (r, c) of ``removed``"""
    idx = np.arange(rows * cols).reshape(rows, cols)
    keep = np.ones((rows - 1, cols - 1), bool)
    for r, c in removed:
        keep[r, c] = False
    a, b, c_, d = (x[keep] for x in (idx[:-1, :-1], idx[:-1, 1:], idx[1:, :-1], idx[1:, 1:]))
    faces = np.stack([np.stack([a, b, c_], 1), np.stack([b, d, c_], 1)], 1).reshape(-1, 3)
    v, f, rgb = _mesh(rows * cols, faces, rows + cols)
    y, x = np.divmod(np.arange(rows * cols), cols)
    v = np.stack([x.astype(np.float32) * h, y.astype(np.float32) * h, np.zeros(rows * cols, np.float32)], 1).astype(np.float32)
    return v, f, rgb


GRID_M = 9
GRID_HOLES = [[(1, 1)], [(1, 4), (1, 5)], [(5, 2), (5, 3), (5, 4)]]          # holes of 4, 6 and 8 edges, all convex


def grid_with_holes():
    return flat_grid(GRID_M, GRID_M, [cell for hole in GRID_HOLES for cell in hole])


def isolated(n, corners, extra=0):
    """n isolated triangles (corners = 3) or open quads of two triangles (corners = 4), then ``extra`` unreferenced vertices"""
    base = corners * np.arange(n)[:, None]
    if corners == 3:
        faces = base + np.array([0, 1, 2])
    else:
        faces = np.stack([base + np.array([0, 1, 2]), base + np.array([2, 1, 3])], 1).reshape(-1, 3)
    return _mesh(corners * n + extra, faces, n)


def flipped_patch():
    """an open patch with every third face reversed, the first among them: the rim changes direction, so it is no loop"""
    v, f, rgb = MCC.grid_patch(6)
    f = f.copy()
    f[::3] = f[::3, ::-1]
    return v, f, rgb


def hostile(which):
    v, f, rgb = MCC.fan(10)
    v = v.copy()
    if which == "nan":
        v[3] = [np.nan, 1.0, -1.0]
    elif which == "inf":
        v[2], v[7] = [np.inf, -np.inf, np.inf], [np.inf, -np.inf, -np.inf]          # inf, -inf, and inf - inf = NaN
    elif which == "huge":
        v[1], v[4], v[5], v[9] = [1e30, -1e30, 1e30], [3.4e38, -3.4e38, 3.4e38], [3.4e38, -3.4e38, -3.4e38], [3.4e38, -3.4e38, 1.0]
    else:
        v[:] = np.array([1e-45, -1e-40, -0.0], np.float32)
        v[6] = [1e-38, 3e-45, 0.0]
    return v, f, rgb


SPHERE_CAPS = ((6.3, 6.6, 11.1), (10.3, 6.6, 7.1), (6.3, 2.6, 7.1))


def extraction(name, cap_radius=None):
    """a mesh of tests/tsdf_cases.py through tests/tsdf_oracle.py; cap_radius: without the faces whose centroid lies within it of one
    of SPHERE_CAPS"""
    r = C.extract_reference(name)
    v, f, rgb = np.array(r["verts"]), np.array(r["faces"]), np.array(r["rgb"])
    if cap_radius is not None:
        centroid = v[f].astype(np.float64).mean(1)
        near = np.zeros(len(f), bool)
        for p in SPHERE_CAPS:
            near |= np.linalg.norm(centroid - np.asarray(p), axis=1) < cap_radius
        f = f[~near]
    return v, f, rgb


# name -> (builder, the values of max_edges)
CASES = {
    "nv_0": (lambda: _mesh(0, np.zeros((0, 3)), 1), [8]),
    "nf_0": (lambda: _mesh(5, np.zeros((0, 3)), 1), [8]),
    "nv_0_with_faces": (lambda: _mesh(0, [(0, 1, 2), (0, 0, 0)], 1), [8]),
    "all_invalid": (lambda: _mesh(4, [(0, 0, 1), (1, 2, 4), (-1, 2, 3), (INT_MAX, INT_MIN, 0), (2, 3, 2), (0, 1, INT_MAX), (INT_MIN, 1, 2)], 4), [8]),
    "tets_closed": (lambda: MCC.tet_strip(9), [8, 4096]),
    "one_triangle": (lambda: MCC.case("one_triangle"), [3, 8]),
    "tets_hole": (lambda: MCC.tet_strip(9, drop_face=7), [3]),
    "open_quad": (lambda: _mesh(4, [(0, 1, 2), (2, 1, 3)], 2), [4, 3]),
    "fan_rim_at_max": (lambda: MCC.fan(8), [10]),
    "fan_rim_past_max": (lambda: MCC.fan(9), [10]),
    "grid_holes": (grid_with_holes, [8, 7, 32]),
    "fan_ascending": (lambda: fan_numbered(12, "ascending"), [14]),
    "fan_descending": (lambda: fan_numbered(12, "descending"), [14]),
    "fan_shuffled": (lambda: fan_numbered(12, "shuffled"), [14]),
    "fan_rotated": (lambda: fan_numbered(12, "rotated"), [14]),
    "strip_rim_4096": (lambda: flat_grid(2, 2048), [4096, 4095]),
    "strip_rim_4098": (lambda: flat_grid(2, 2049), [4096]),
    "holes_share_vertex": (lambda: flat_grid(5, 5, [(1, 1), (2, 2)]), [8]),
    "nonmanifold_3": (lambda: MCC.nonmanifold(3), [8]),
    "share_vertex": (lambda: MCC.case("share_vertex"), [8]),
    "flipped_patch": (flipped_patch, [64]),
    "invalid_among_valid": (MCC.invalid_faces, [8]),
    "triangles_4097": (lambda: isolated(4097, 3), [3]),
    "quads_2047": (lambda: isolated(2047, 4), [4]),
    "quads_2048": (lambda: isolated(2048, 4), [4]),
    "quads_2049": (lambda: isolated(2049, 4), [4]),
    "quads_4097": (lambda: isolated(4097, 4), [4]),
    "quads_nv_tile_minus_1": (lambda: isolated(TILE // 4 - 1, 4, 3), [4]),
    "quads_nv_tile": (lambda: isolated(TILE // 4, 4), [4]),
    "quads_nv_tile_plus_1": (lambda: isolated(TILE // 4, 4, 1), [4]),
    "hostile_nan": (lambda: hostile("nan"), [12]),
    "hostile_inf": (lambda: hostile("inf"), [12]),
    "hostile_huge": (lambda: hostile("huge"), [12]),
    "hostile_denormal": (lambda: hostile("denormal"), [12]),
    "extraction_hole": (lambda: extraction("hole"), [64, 8]),
    "extraction_min_weight_2": (lambda: extraction("min_weight_2"), [64, 8]),
    "extraction_two_sheets": (lambda: extraction("two_sheets"), [64, 8]),
    "sphere_caps_0.8": (lambda: extraction("sphere_13x13x14", 0.8), [64, 8]),
    "sphere_caps_1.6": (lambda: extraction("sphere_13x13x14", 1.6), [64, 8]),
    "sphere_caps_2.5": (lambda: extraction("sphere_13x13x14", 2.5), [64, 8]),
}

# what a case is there for: the oracle's stats of its FIRST max_edges (only the listed keys), the lengths of the filled loops in
# leader order, (vertices, faces) out, and for a closed result its Euler characteristic (vertices - edges + faces of the 1-ring)
KNOWN = {
    "one_triangle": ({"boundary_edges": 3, "loops_filled_by_one_face": 1, "vertices_added": 0, "faces_added": 1, "boundary_edges_left": 0}, [3], (3, 2), None),
    "tets_hole": ({"boundary_edges": 3, "vertices_added": 0, "faces_added": 1, "boundary_edges_left": 0}, [3], (12, 20), 2),
    "open_quad": ({"boundary_edges": 4, "vertices_added": 1, "faces_added": 4, "boundary_edges_left": 0}, [4], (5, 6), 2),
    "fan_rim_at_max": ({"loops_filled": 1, "longest_filled": 10, "boundary_edges_left": 0}, [10], (11, 18), 2),
    "fan_rim_past_max": ({"boundary_edges": 11, "loops_filled": 0, "faces_added": 0, "boundary_edges_left": 11}, [], (11, 9), None),
    "grid_holes": ({"boundary_edges": 18 + 4 * (GRID_M - 1), "complex_vertices": 0, "loops_filled": 3, "longest_filled": 8, "vertices_added": 3,
                    "faces_added": 18, "boundary_edges_left": 4 * (GRID_M - 1)}, [4, 6, 8], None, None),
    "strip_rim_4096": ({"boundary_edges": 4096, "loops_filled": 1, "longest_filled": 4096, "faces_added": 4096, "boundary_edges_left": 0}, [4096], None, 2),
    "strip_rim_4098": ({"boundary_edges": 4098, "loops_filled": 0, "boundary_edges_left": 4098}, [], None, None),
    "holes_share_vertex": ({"complex_vertices": 1, "loops_filled": 0, "faces_added": 0, "boundary_edges": 8 + 16, "boundary_edges_left": 24}, [], None, None),
    "nonmanifold_3": ({"complex_vertices": 2, "boundary_edges": 6, "faces_added": 0}, [], None, None),
    "share_vertex": ({"complex_vertices": 1, "boundary_edges": 6, "faces_added": 0}, [], None, None),
    "flipped_patch": ({"loops_filled": 0, "vertices_added": 0, "faces_added": 0}, [], None, None),
    "triangles_4097": ({"loops_filled": 4097, "loops_filled_by_one_face": 4097, "vertices_added": 0, "faces_added": 4097}, [3] * 4097, None, None),
    "quads_4097": ({"loops_filled": 4097, "loops_filled_by_one_face": 0, "vertices_added": 4097, "faces_added": 4 * 4097}, [4] * 4097, None, None),
    "extraction_hole": ({"complex_vertices": 0, "boundary_edges_left": 0}, [32, 32], (918, 1832), 2),
    "extraction_min_weight_2": ({"complex_vertices": 0, "boundary_edges_left": 0}, [58], (449, 894), 2),
    "extraction_two_sheets": ({"complex_vertices": 0, "boundary_edges_left": 0}, [52, 52], None, 4),
    "sphere_caps_0.8": ({"complex_vertices": 0, "boundary_edges_left": 0}, [15, 14, 12], None, 2),
    "sphere_caps_1.6": ({"complex_vertices": 0, "boundary_edges_left": 0}, [24, 25, 25], None, 2),
    "sphere_caps_2.5": ({"complex_vertices": 1, "boundary_edges_left": 40}, [33, 41], None, None),
}
UNCHANGED_AT_8 = ("extraction_hole", "extraction_min_weight_2", "extraction_two_sheets", "sphere_caps_0.8", "sphere_caps_1.6", "sphere_caps_2.5")
NOTHING_ADDED = ("nv_0", "nf_0", "nv_0_with_faces", "all_invalid", "tets_closed", "holes_share_vertex", "nonmanifold_3", "share_vertex", "flipped_patch",
                 "fan_rim_past_max", "strip_rim_4098")


@functools.lru_cache(maxsize=None)
def case(name):
    v, f, rgb = CASES[name][0]()
    for a in (v, f, rgb):
        a.setflags(write=False)
    return v, f, rgb


@functools.lru_cache(maxsize=None)
def reference(name, k):
    """the oracle's fill_holes of the k-th max_edges of a case, and its boundary"""
    v, f, rgb = case(name)
    return O.fill_holes(v, f, rgb, CASES[name][1][k]), O.boundary(len(v), f)


def case_keys():
    return [(name, k) for name in CASES for k in range(len(CASES[name][1]))]


def check_known(name, k):
    """the hand answers, on the oracle alone"""
    v, f, rgb = case(name)
    (wv, wf, wc, wstats, loops), wbnd = reference(name, k)
    nv, nf = len(v), len(f)
    assert same_bits(wv[:nv], v) and np.array_equal(wf[:nf], f) and np.array_equal(wc[:nv], rgb), name                     # the input comes first, in every bit
    assert len(wv) == nv + wstats["vertices_added"] and len(wf) == nf + wstats["faces_added"] and wstats["loops_filled"] == len(loops), name
    assert wstats["boundary_edges_left"] == wstats["boundary_edges"] - sum(len(loop) for loop in loops), name
    leaders = [loop[0] for loop in loops]
    assert leaders == sorted(leaders) and all(loop[0] == min(loop) for loop in loops), name
    assert MCC.O.adjacency(len(wv), wf)["boundary_edges"] == wstats["boundary_edges_left"], name                          # what the 1-ring of the result says
    if name in NOTHING_ADDED or (name in UNCHANGED_AT_8 and CASES[name][1][k] == 8):
        assert wstats["faces_added"] == wstats["vertices_added"] == 0 and same_bits(wv, v) and np.array_equal(wf, f) and np.array_equal(wc, rgb), name
    if name == "flipped_patch":
        assert wstats["complex_vertices"] > 0 and wstats["boundary_edges"] == 20
    if k == 0 and name in KNOWN:
        stats, lengths, sizes, euler = KNOWN[name]
        assert {key: wstats[key] for key in stats} == stats, (name, wstats)
        assert [len(loop) for loop in loops] == lengths, (name, [len(loop) for loop in loops])
        assert sizes is None or (len(wv), len(wf)) == sizes, (name, len(wv), len(wf))
        if euler is not None:
            ring = MCC.O.adjacency(len(wv), wf)
            assert ring["boundary_edges"] == ring["nonmanifold_edges"] == 0 and ring["referenced_vertices"] - ring["edges"] + len(wf) == euler, name
            if name != "tets_hole":                                               # tet_strip's faces are not consistently oriented
                assert TO.closed_and_oriented(wf) == (True, euler), (name, TO.closed_and_oriented(wf))
    if name == "tets_hole":
        dropped = MCC.tet_strip(9)[1][7]
        assert sorted(wf[-1].tolist()) == sorted(dropped.tolist())
    if name.startswith("fan_") and name[4:] in ("ascending", "descending", "shuffled", "rotated"):
        # the same hole under every numbering: the same new position up to the order of the sum, the walk from the smallest number
        assert len(loops) == 1 and loops[0][0] == 0 and wf[nf].tolist() == [loops[0][1], 0, nv]
        if name == "fan_rotated":
            assert 0 not in f[:4] and loops[0][len(loops[0]) // 2] == f[0, 0]    # the leader lies in the middle of the rim as the faces run
        ref = reference("fan_ascending", 0)[0][0][-1].astype(np.float64)
        assert np.abs(wv[-1].astype(np.float64) - ref).max() <= 4 * np.spacing(np.abs(case("fan_ascending")[0]).max())
    if name == "grid_holes":
        check_grid(v, f, wv, wf, wstats, CASES[name][1][k])
    if name.startswith("hostile") and k == 0:
        assert wstats["loops_filled"] == 1 and wstats["vertices_added"] == 1
        with np.errstate(all="ignore"):
            new = wv[-1]
        if name == "hostile_nan":
            assert np.isnan(new[0]) and np.isfinite(new[1:]).all()
        if name == "hostile_inf":
            assert new[0] == np.inf and new[1] == -np.inf and np.isnan(new[2])
        if name == "hostile_huge":
            assert np.isfinite(new).all() and new[0] > 5e37 and new[1] < -5e37
        if name == "hostile_denormal":
            assert (np.abs(new) < 1e-38).all()


def check_grid(v, f, wv, wf, wstats, max_edges):
    """the flat grid at z = 0 with convex holes of 4, 6 and 8 edges"""
    nv, nf = len(v), len(f)
    rim = 4 * (GRID_M - 1)
    if max_edges == 7:
        assert wstats["loops_filled"] == 2 and wstats["longest_filled"] == 6 and wstats["boundary_edges_left"] == rim + 8
        return
    if max_edges == 32:
        assert wstats["loops_filled"] == 4 and wstats["longest_filled"] == rim and wstats["boundary_edges_left"] == 0     # the rim is a loop too
        return
    assert wstats["boundary_edges_left"] == rim                                        # max_edges = 8 is below the rim's length: it stays open
    assert (bits(wv[nv:, 2]) == 0).all() and len(wv) == nv + 3                           # every new vertex has z = +0.0 in every bit
    area = lambda p, t: 0.5 * np.linalg.norm(np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]), axis=1)      # noqa: E731
    present = set(map(tuple, f.tolist()))
    removed = np.array([t for t in flat_grid(GRID_M, GRID_M)[1].tolist() if tuple(t) not in present])
    assert len(removed) == 2 * 6
    p = wv.astype(np.float64)
    added, want = area(p, wf[nf:]).sum(), area(p, removed).sum()
    # Tolerance.  With the exact mean c inside a convex hole the fan's triangles tile the hole, so the two areas are equal.  The
    # stored c is that mean rounded to fp32: each coordinate moves by at most half an ulp, 2^-24 |c| <= 2^-24 X with X the largest
    # coordinate of the grid, so c moves by at most d = sqrt(2) 2^-24 X in the plane.  A triangle (u, w, c) changes its area by at
    # most |w - u| d / 2 when c moves by d; summed over the fans that is (the holes' perimeters) d / 2.  The holes' edges are grid
    # edges of length h, 18 in all.  The fp64 evaluation of 30 triangle areas adds rounding of the order 30 * 2^-52 X^2, covered
    # by doubling.
    h, X = np.float64(np.float32(0.1)), np.float64(np.abs(v).max())
    tol = 2.0 * (18 * h) * (np.sqrt(2.0) * 2.0 ** -24 * X) / 2.0
    print(f"grid: removed area {want:.17g}, added {added:.17g}, difference {abs(added - want):.3g}, tolerance {tol:.3g}")
    assert abs(added - want) <= tol


def check_case(dev, name, k, twice=False):
    """boundary and fill_holes of the k-th max_edges of the case, with and without colours: everything equal to the oracle's"""
    v, f, rgb = case(name)
    max_edges = CASES[name][1][k]
    check_known(name, k)
    (wv, wf, wc, wstats, _), wbnd = reference(name, k)
    tv, tf, tc = to_dev(dev, v, f, rgb)
    bnd = MH.boundary(len(v), tf)
    for key in ("succ", "pred", "flags", "out_count", "in_count"):
        assert np.array_equal(host(bnd[key]), wbnd[key]), (name, key)
    assert bnd["boundary_edges"] == wbnd["boundary_edges"] and bnd["complex_vertices"] == wbnd["complex_vertices"], name
    assert bnd["flags"].dtype == torch.uint8 and bnd["succ"].dtype == torch.int32
    gv, gf, gc, gstats = MH.fill_holes(tv, tf, tc, max_edges=max_edges)
    print(f"{name} max_edges={max_edges}: {gstats}")
    assert gv.dtype == torch.float32 and gf.dtype == torch.int32 and gc.dtype == torch.uint8
    assert gstats == wstats and list(gstats) == list(wstats), (name, gstats, wstats)
    if not same_bits(host(gv), wv):
        rows = np.nonzero((bits(host(gv)) != bits(wv)).any(1))[0]
        print("positions differ at", rows.tolist(), "got", bits(host(gv))[rows].tolist(), "want", bits(wv)[rows].tolist())
    assert same_bits(host(gv), wv) and np.array_equal(host(gf), wf) and np.array_equal(host(gc), wc), name
    plain = MH.fill_holes(tv, tf, None, max_edges=max_edges)
    assert plain[2] is None and plain[3] == gstats and torch.equal(plain[0].view(torch.int32), gv.view(torch.int32)) and torch.equal(plain[1], gf)
    assert torch.equal(tv.view(torch.int32), torch.from_numpy(np.array(v)).view(torch.int32).to(dev)) and torch.equal(tf.cpu(), torch.from_numpy(np.array(f)))
    if twice:
        again = MH.fill_holes(*to_dev(dev, v, f, rgb), max_edges=max_edges)
        assert again[3] == gstats and torch.equal(again[0].view(torch.int32), gv.view(torch.int32)) and torch.equal(again[1], gf) and \
            torch.equal(again[2], gc), name


def check_refusals(dev):
    """bad arguments of the module, on the device's path"""
    tv, tf, tc = to_dev(dev, *case("open_quad"))
    for kw, pattern in (({"max_edges": 2}, "max_edges"), ({"max_edges": 0}, "max_edges"), ({"max_edges": MH.MAX_EDGES + 1}, "max_edges"),
                        ({"max_edges": -1}, "max_edges"), ({"max_edges": 8.0}, "max_edges"), ({"max_edges": True}, "max_edges")):
        for call in (lambda **a: MH.fill_holes(tv, tf, tc, **a), lambda **a: MC.clean_mesh(tv, tf, tc, fill_holes=a["max_edges"])):
            try:
                call(**kw)
            except _lib.RcmvsError as e:
                assert pattern in str(e) or "fill_holes" in str(e), (kw, str(e))
            else:
                assert kw == {"max_edges": 0}, f"{kw} was accepted"                 # fill_holes = 0 turns the step off in clean_mesh
        try:
            O.fill_holes(*case("open_quad"), **kw)
        except O.Refused:
            pass
        else:
            raise AssertionError(f"the oracle accepted {kw}")
    bnd = MH.boundary(4, tf)
    for bad in (lambda: MH.boundary(5, tf, MC.adjacency(4, tf)), lambda: MH.boundary(4, tf[:1], MC.adjacency(4, tf)),
                lambda: MH.emit(tv[:3], tf, None, bnd, MH.leaders(bnd, 4)), lambda: MH.boundary(-1, tf)):
        try:
            bad()
        except _lib.RcmvsError:
            pass
        else:
            raise AssertionError("a mismatched adjacency or boundary was accepted")
    for nv, nf, va, fa in ((2 ** 31 - 1, 5, 1, 0), (5, 2 ** 31 - 4, 0, 4)):
        try:
            MH.check_output_counts(nv, nf, va, fa, "test")
        except _lib.RcmvsError as e:
            assert "2^31" in str(e)
        else:
            raise AssertionError("a count of 2^31 was accepted")
    MH.check_output_counts(2 ** 31 - 2, 2 ** 31 - 5, 1, 4, "test")


# ---- the clean-up composite ---------------------------------------------------------------------------------------------------
CAP_AT, CAP_RADIUS = (6.2, 6.4, 10.7), 1.3                                       # on the large sphere of mesh_clean_cases' scene


def check_clean_composite(dev):
    """clean_mesh(keep_largest=1, fill_holes=64, smooth_iterations=2) on the two spheres and the speck with a cap removed from the
    large sphere: the oracle's composite in every bit; the hole is closed, and its former rim, pinned without the filling, has moved"""
    verts, faces, rgb = MCC.scene_volume(dev).extract(1)
    v, f, c = host(verts), host(faces), host(rgb)
    f = f[np.linalg.norm(v[f].astype(np.float64).mean(1) - np.asarray(CAP_AT), axis=1) >= CAP_RADIUS]
    tf = torch.from_numpy(f).to(verts.device)
    opts = dict(keep_largest=1, fill_holes=64, smooth_iterations=2)
    wv, wf, wc, wstats = O.clean_mesh(v, f, c, **opts)
    gv, gf, gc, gstats = MC.clean_mesh(verts, tf, rgb, **opts)
    print("composite:", gstats)
    assert gstats == wstats and list(gstats) == list(wstats) and same_bits(host(gv), wv) and np.array_equal(host(gf), wf) and np.array_equal(host(gc), wc)
    holes = wstats["holes"]
    assert holes["loops_filled"] == 1 and holes["boundary_edges_left"] == 0 and holes["complex_vertices"] == 0 and 8 < holes["longest_filled"] <= 64
    assert wstats["boundary_edges"] == 0 and wstats["euler_characteristic"] == 2 and wstats["components_kept"] == 1
    assert wstats["vertices_out"] == wstats["vertices_in"] - wstats["unreferenced_removed"] + 1
    open_v, open_f, _, open_stats = MCC.O.clean_mesh(v, f, c, keep_largest=1, smooth_iterations=2)
    compact_v, compact_f, _, _ = MCC.O.compact(v, f, c, keep_largest=1)
    rim = MCC.O.adjacency(len(compact_v), compact_f)["on_boundary"] != 0
    assert rim.sum() == holes["longest_filled"] == open_stats["boundary_edges"] and "holes" not in open_stats
    n = len(compact_v)
    assert same_bits(open_v[rim], compact_v[rim]) and (bits(wv[:n][rim]) != bits(compact_v[rim])).any(1).all()
    again = MC.clean_mesh(verts, tf, rgb, **opts)
    assert again[3] == gstats and torch.equal(again[0].view(torch.int32), gv.view(torch.int32)) and torch.equal(again[1], gf) and torch.equal(again[2], gc)


def check_off_is_today(dev):
    """fill_holes = 0: the result and the stats of three of the clean-up suite's cases as they are without the argument"""
    for name, k in (("tets_hole", 1), ("grid_patch", 2), ("invalid_faces", 0)):
        v, f, rgb = MCC.case(name)
        opts = MCC.CASES[name][1][k]
        wv, wf, wc, wstats = MCC.reference(name, k)
        gv, gf, gc, gstats = MC.clean_mesh(*to_dev(dev, v, f, rgb), fill_holes=0, **opts)
        assert gstats == wstats and list(gstats) == list(wstats) and "holes" not in gstats, name
        assert same_bits(host(gv), wv) and np.array_equal(host(gf), wf) and np.array_equal(host(gc), wc), name
        assert O.clean_mesh(v, f, rgb, fill_holes=0, **opts)[3] == wstats


# ---- end to end -------------------------------------------------------------------------------------------------------------
def check_end_to_end(dev, tmp_path, sparse):
    """mesh_scan(..., keep_largest=1, fill_holes=64) on the small scan of tsdf_cases.check_end_to_end, dense or sparse: the PLY is
    the oracle's composite of the mesh mesh_scan writes without the options, colours included, and the summary's "clean" carries
    the stats with "holes"; without fill_holes the summary has no new key"""
    pair_folder, out_folder = C.write_scan(tmp_path)
    raw, kept, ply = (str(tmp_path / "out" / n) for n in ("raw.ply", "kept.ply", "filled.ply"))
    kw = dict(resolution=32, device=dev, sparse=sparse)
    plain = TM.mesh_scan(pair_folder, out_folder, out_folder, raw, C.PROB, C.NCONS, C.DIST, C.DEPTH, **kw)
    off = TM.mesh_scan(pair_folder, out_folder, out_folder, kept, C.PROB, C.NCONS, C.DIST, C.DEPTH, keep_largest=1, **kw)
    summary = TM.mesh_scan(pair_folder, out_folder, out_folder, ply, C.PROB, C.NCONS, C.DIST, C.DEPTH, keep_largest=1, fill_holes=64, **kw)
    assert "clean" not in plain and set(summary) == set(off) == set(plain) | {"clean"}
    assert "holes" not in off["clean"] and set(summary["clean"]) == set(off["clean"]) | {"holes"}
    verts, faces, rgb = dtu_io.read_ply_mesh_rgb(raw)
    wv, wf, wc, wstats = O.clean_mesh(verts, faces, rgb, keep_largest=1, fill_holes=64)
    assert off["clean"] == MCC.O.clean_mesh(verts, faces, rgb, keep_largest=1)[3]
    gv, gf, gc = dtu_io.read_ply_mesh_rgb(ply)
    print("end to end:", summary["clean"])
    assert summary["clean"] == wstats and summary["clean"]["holes"] == wstats["holes"]
    assert same_bits(gv, wv) and np.array_equal(gf, wf) and np.array_equal(gc, wc)
    assert summary["vertices"] == len(gv) == wstats["vertices_out"] and summary["faces"] == len(gf) == wstats["faces_out"]
    assert {k: v for k, v in summary.items() if k not in ("clean", "mesh", "vertices", "faces", "unreferenced_vertices")} == \
           {k: v for k, v in plain.items() if k not in ("mesh", "vertices", "faces", "unreferenced_vertices")}
    return pair_folder, out_folder, summary


def check_command_line_round_trip(dev, tmp_path):
    """python -m rc_mvsnet_amd.mesh_clean --fill-holes on a written PLY: positions and faces of the oracle's composite"""
    v, f, rgb = case("sphere_caps_0.8")
    src, dst = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    with open(src, "wb") as fh:
        fh.write(TM.mesh_ply_bytes(v, f, rgb))
    summary = MC.main(["--in", src, "--out", dst, "--fill-holes", "64", "--device", dev])
    wv, wf, _, wstats = O.clean_mesh(v, f, None, fill_holes=64)
    gv, gf = dtu_io.read_ply_mesh(dst)
    assert same_bits(gv, wv) and np.array_equal(gf, wf) and summary["holes"] == wstats["holes"] and wstats["holes"]["loops_filled"] == 3
    assert "holes" not in MC.main(["--in", src, "--out", dst, "--device", dev])
