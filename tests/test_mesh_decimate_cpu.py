"""tests/mesh_decimate_oracle.py itself, on answers that can be checked by hand, and the parts of rc_mvsnet_amd/mesh_decimate.py that
need no kernel: the options, the default-off plumbing, the coloured PLY reader and the header's place in _lib.EXT_HEADERS.  The
kernels inherit every property below through bit equality with this oracle (tests/test_mesh_decimate_emu_cpu.py,
tests/test_gpu_mesh_decimate.py)."""
import inspect

import numpy as np
import pytest

import mesh_decimate_cases as MDC
import mesh_decimate_oracle as O
import tsdf_cases as C
import tsdf_oracle as TO
from rc_mvsnet_amd import _lib, dtu_io, eval_driver, mesh_decimate as MD, tsdf_mesh as TM


def test_every_case_says_what_it_is_there_for():
    for name, want in MDC.KNOWN.items():
        got = {k: MDC.known_value(name, k) for k in want}
        assert got == want, (name, got)
    for name, passes in MDC.PASSES.items():
        assert MDC.passes_of(MDC.reference(name, 0, "quadric")[4]["lattice"]) == passes, name


@pytest.mark.parametrize("name,k", MDC.case_keys())
def test_properties_hold_on_the_oracle(name, k):
    v, f, _ = MDC.case(name)
    for placement in ("quadric", "mean"):
        wv, wf, _, _, parts = MDC.reference(name, k, placement)
        MDC.check_properties(v, f, wv, wf, parts, (name, k, placement))


def test_lattice_and_keys_by_hand():
    lo, hi, n = O.bounds(np.array([[0, 0, 0], [2.5, 1, 0], [np.nan, 9, 9], [1, np.inf, -7]], np.float32))
    assert lo.tolist() == [0, 0, 0] and hi.tolist() == [2.5, 1, 0] and n == 2          # a vertex with one bad coordinate counts on no axis
    lat = O.lattice(lo, hi, 1.0)
    assert lat == {"origin": [-0.5, -0.5, -0.5], "cell": 1.0, "dims": [4, 2, 1]}     # floor((2.5 + 0.5) / 1) + 1 = 4: 2.5 is on a border and goes up
    v = np.array([[2.5, 1, 0], [0, 0, 0], [np.nan, 0, 0], [0.4, 0.4, 0.4], [2.49, 0.5, 0]], np.float32)
    cl = O.cluster(v, lat)
    assert cl["cluster"].tolist() == [2, 0, -1, 0, 1] and cl["order"].tolist() == [1, 3, 4, 0, 2] and cl["cluster_start"].tolist() == [0, 2, 3, 4]
    assert cl["cluster_key"].tolist() == [0, 4 + 2, 4 + 3] and cl["m"] == 3 and cl["clustered"] == 4
    with pytest.raises(O.Refused, match="axis y"):
        O.lattice([0, 0, 0], [1, 2 ** 21 * 0.5, 1], 0.5)
    assert O.lattice([0, 0, 0], [1, (2 ** 21 - 1) * 0.5, 1], 0.5)["dims"] == [3, 2 ** 21, 3]


def test_minus_zero_is_the_minimum_in_every_bit():
    v, _, _ = MDC.case("minus_zero")
    lo, hi, _ = O.bounds(v)
    assert np.signbit(lo).tolist() == [True, True, True] and lo.tolist() == [0, 0, 0] and hi.tolist() == [1, 1, 1]
    assert O.ordered(np.float32(-0.0)) < O.ordered(np.float32(0.0)) and O.unordered(O.ordered(v)).view(np.uint32).tolist() == v.view(np.uint32).tolist()


def test_faces_by_hand():
    cl = {"cluster": np.array([0, 1, 2, 3, 1, -1], np.int32)}
    faces = [(0, 1, 2), (1, 2, 0), (0, 2, 1), (0, 4, 2), (1, 4, 2), (0, 1, 5), (0, 0, 1), (0, 1, 6), (2, 3, 0)]
    cface, cls, counts = O.classify_faces(6, faces, cl)
    assert cls.tolist() == [O.KEPT, O.DUPLICATE, O.KEPT, O.DUPLICATE, O.COLLAPSED, O.UNCLUSTERED, O.INVALID, O.INVALID, O.KEPT]
    assert counts == [2, 1, 1, 2] and cface[3].tolist() == [0, 1, 2] and cface[6].tolist() == [-1, -1, -1]
    assert O.rotate_min_first([(5, 3, 9), (3, 9, 5), (9, 5, 3), (3, 5, 9)]).tolist() == [[3, 9, 5]] * 3 + [[3, 5, 9]]


def test_colour_rounds_half_up_in_integers():
    v, f, rgb = MDC.case("rounding_colours")
    _, _, _, _, parts = O.decimate(v, f, rgb, cell=1.0, drop_unreferenced=False)
    assert parts["cluster_rgb"].tolist() == [[2, 255, 1], [8, 1, 255], [101, 103, 4], [9, 8, 7]]      # 1.5 -> 2, 254.5 -> 255, 0.5 -> 1, 102.5 -> 103


def plane_grid(m, height):
    """an m x m grid 1 apart, z = height(x, y): exactly representable coordinates"""
    p, f = MDC.grid_sheet(m, spacing=1.0)
    p[:, 2] = height(p[:, 0], p[:, 1])
    return p.astype(np.float32), f.astype(np.int32)


@pytest.mark.parametrize("which,height,normal,offset", [("level", lambda x, y: 0.375 + 0 * x, (0, 0, 1), 0.375),
                                                        ("diagonal", lambda x, y: x + 0.25, (-1, 0, 1), 0.25)])
def test_planar_grid(which, height, normal, offset):
    """a 17 x 17 grid with cell = 2: the lattice starts at -1, so an axis has the clusters {0}, {1, 2}, ..., {15, 16}: 9 per axis, 81 in
    all, of 1, 2 or 4 members; two faces survive at each of the 8 x 8 corners where four clusters meet and every other face has
    two vertices in one cluster: 128 faces.  Every quadric-placed vertex lies on the plane."""
    v, f = plane_grid(17, height)
    for cell in (2.0, 4.0):
        k = 9 if cell == 2.0 else 5                                  # cell = 4: {0, 1}, {2 .. 5}, ..., {14, 15, 16}
        out_v, out_f, _, stats, parts = O.decimate(v, f, None, cell=cell)
        assert stats["clusters"] == k * k and stats["faces_out"] == 2 * (k - 1) ** 2 and stats["duplicate_faces"] == 0, (cell, stats)
        assert stats["collapsed_faces"] == 2 * 16 * 16 - 2 * (k - 1) ** 2 and stats["nonmanifold_edges"] == 0 and stats["euler_characteristic"] == 1
        assert (parts["via"] == O.VIA_QUADRIC).all() and stats["vertices_out"] == k * k, (cell, np.bincount(parts["via"]))
        n = np.asarray(normal, np.float64)
        dist = np.abs(out_v.astype(np.float64) @ n - offset) / np.linalg.norm(n)
        print(which, cell, "largest distance to the plane / cell:", dist.max() / cell)
        assert dist.max() <= 1e-9 * cell


def cube_corner(c, m=6, h=0.1):
    """three m x m-vertex patches on the planes x = c[0], y = c[1], z = c[2], each starting at the corner c and running h apart
    into the positive directions, sharing their edge vertices"""
    index, p, faces = {}, [], []

    def vid(q):
        key = tuple(int(round(t)) for t in q)
        if key not in index:
            index[key] = len(p)
            p.append([c[a] + h * key[a] for a in range(3)])
        return index[key]

    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for i in range(m - 1):
            for j in range(m - 1):
                def at(di, dj):
                    q = [0, 0, 0]
                    q[u], q[w] = i + di, j + dj
                    return vid(q)
                faces += [(at(0, 0), at(1, 0), at(0, 1)), (at(1, 0), at(1, 1), at(0, 1))]
    return np.asarray(p, np.float32), np.asarray(faces, np.int32)


def test_cube_corner():
    """Three equal patches meeting at c inside one cell: the cluster of the corner's cell has A = w I (the three planes with equal
    weights), so the regularised minimiser misses the corner by 3 reg / (1 + 3 reg) of the mean's miss.  The corner lies within
    3 / 1024 of the origin, where fp32 is 2^-32 apart: the final rounding of the position to fp32 (some 1e-10) stays below the
    1e-9 cell the bound allows, which it would not at a corner of the order of the cell."""
    c = np.array([1.0, 2.0, 3.0]) / 1024.0
    v, f = cube_corner(c, m=5, h=0.125)                           # vertices at c .. c + 0.5: the lattice starts at c - 0.5, the first cell ends at c + 0.5
    cell = 1.0
    for reg in (1e-3, 1e-2):
        _, _, _, sq, pq = O.decimate(v, f, None, cell=cell, reg=reg, drop_unreferenced=False)
        _, _, _, sm, pm = O.decimate(v, f, None, cell=cell, placement="mean", drop_unreferenced=False)
        assert sq["clusters"] == 7 and pq["via"][0] == O.VIA_QUADRIC                   # the corner's cell (key 0) and the six it touches
        miss_q = np.linalg.norm(pq["cluster_verts"][0].astype(np.float64) - c)
        miss_m = np.linalg.norm(pm["cluster_verts"][0].astype(np.float64) - c)
        print("reg", reg, "quadric misses by", miss_q, "the mean by", miss_m, "bound", 3 * reg / (1 + 3 * reg) * miss_m + 1e-9 * cell)
        assert miss_m > 0.1 and miss_q <= 3 * reg / (1 + 3 * reg) * miss_m + 1e-9 * cell


SPHERE_DIMS, SPHERE_CENTRE, SPHERE_RADIUS = (28, 28, 28), (14.3, 13.8, 14.1), 10.4


def sphere_mesh():
    f = C.sphere_field(SPHERE_DIMS, C.UNIT, SPHERE_CENTRE, SPHERE_RADIUS)
    r = TO.extract(f.astype(np.float32).ravel(), np.ones(f.size, np.float32), None, C.UNIT, SPHERE_DIMS, 1)
    return r["verts"], r["faces"]


def test_sphere_quadric_placement_is_closer_than_the_mean():
    """A sphere of radius 10.4 voxels extracted by the marching-tetrahedra oracle (6 092 vertices, 12 180 faces) and decimated at 2
    voxels.  The oracle gives 441 vertices and 891 faces, and of the 441 referenced clusters ONE falls back to the mean
    (fallback_outside = 1, fallback_no_faces = fallback_singular = 0; SPHERE_COUNTS below), far fewer than a tenth, so the
    comparison is about quadric placement: the RMS of | |x - centre| - R | is strictly smaller under quadric placement (0.0202
    voxels when this was written) than under the mean (0.0337), compared with no constant."""
    v, f = sphere_mesh()
    rms, stats = {}, {}
    for placement in ("quadric", "mean"):
        out_v, out_f, _, stats[placement], parts = O.decimate(v, f, None, cell=2.0, placement=placement)
        d = np.abs(np.linalg.norm(out_v.astype(np.float64) - np.asarray(SPHERE_CENTRE), axis=1) - SPHERE_RADIUS)
        rms[placement] = float(np.sqrt((d * d).mean()))
        if placement == "quadric":
            via = parts["via"][parts["vert_keep"]]
            fallbacks = int((via != O.VIA_QUADRIC).sum())
    s = stats["quadric"]
    counts = {"vertices_in": s["vertices_in"], "faces_in": s["faces_in"], "vertices_out": s["vertices_out"], "faces_out": s["faces_out"],
              "fallbacks_among_referenced": fallbacks, "fallback_no_faces": s["fallback_no_faces"], "fallback_singular": s["fallback_singular"],
              "fallback_outside": s["fallback_outside"]}
    print(counts, rms)
    assert counts == SPHERE_COUNTS
    assert s["fallback_no_faces"] + s["fallback_singular"] + s["fallback_outside"] < s["vertices_out"] / 10
    assert stats["mean"]["faces_out"] == s["faces_out"] and s["boundary_edges"] == 0
    assert rms["quadric"] < rms["mean"]


SPHERE_COUNTS = {'vertices_in': 6092, 'faces_in': 12180, 'vertices_out': 441, 'faces_out': 891, 'fallbacks_among_referenced': 1, 'fallback_no_faces': 0,
                 'fallback_singular': 0, 'fallback_outside': 1}


# ---- host logic -------------------------------------------------------------------------------------------------------------
def test_options():
    assert MD.decimate_options() is None and MD.decimate_options(0.0, 0.0) is None and MD.decimate_options(0, 0) is None
    assert MD.decimate_options(cell=0.004) == {"cell": 0.004} and MD.decimate_options(voxels=2) == {"voxels": 2.0}
    for kw, pattern in (({"cell": 1.0, "voxels": 2.0}, "not both"), ({"cell": -1.0}, "cell"), ({"voxels": float("nan")}, "voxels"), ({"cell": float("inf")}, "cell")):
        with pytest.raises(_lib.RcmvsError, match=pattern):
            MD.decimate_options(**kw)
    assert MD.DEFAULT_REG == O.DEFAULT_REG == 1e-3
    assert inspect.signature(MD.decimate).parameters["reg"].default == MD.DEFAULT_REG
    p = inspect.signature(MD.decimate).parameters
    assert p["cell"].kind is inspect.Parameter.KEYWORD_ONLY and p["cell"].default is inspect.Parameter.empty
    assert p["placement"].default == "quadric" and p["drop_unreferenced"].default is True


def test_decimation_is_off_by_default():
    """without the options mesh_scan hands _mesh_views exactly the arguments it handed it before; with one, the options as
    ``decimate``; the voxel option is multiplied by the volume's voxel edge"""
    for fn in (TM.mesh_scan, TM.mesh_scan_tanks):
        p = inspect.signature(fn).parameters
        assert [p[k].default for k in ("decimate_cell", "decimate_voxels")] == [0.0, 0.0]
    assert inspect.signature(TM._mesh_views).parameters["decimate"].default is None
    seen = {}

    def views_only(*args, **kw):
        seen["args"], seen["kw"] = args, kw
        return {"mesh": args[1]}

    import unittest.mock as mock
    with mock.patch.object(TM, "filtered_views", lambda *a, **k: {}), mock.patch.object(TM, "_mesh_views", views_only):
        TM.mesh_scan("p", "s", "o", "m.ply", 0.8, 3, 0.5, 0.01)
        assert seen["kw"] == {} and len(seen["args"]) == 10 and seen["args"][-1] is None
        TM.mesh_scan("p", "s", "o", "m.ply", 0.8, 3, 0.5, 0.01, decimate_voxels=2)
        assert seen["kw"] == {"decimate": {"voxels": 2.0}} and seen["args"][-1] is None
        TM.mesh_scan("p", "s", "o", "m.ply", 0.8, 3, 0.5, 0.01, decimate_cell=0.5, smooth=1)
        assert seen["kw"] == {"decimate": {"cell": 0.5}} and seen["args"][-1]["smooth_iterations"] == 1
        with pytest.raises(_lib.RcmvsError, match="not both"):
            TM.mesh_scan("p", "s", "o", "m.ply", 0.8, 3, 0.5, 0.01, decimate_cell=0.5, decimate_voxels=2)
    calls = []
    with mock.patch.object(MD, "decimate", lambda v, f, c, **kw: calls.append(kw) or (v, f, c, {})):
        MD.decimate_mesh_path(1, 2, 3, {"voxels": 2.0}, 0.25)
        MD.decimate_mesh_path(1, 2, 3, {"cell": 0.3}, 0.25)
    assert calls == [{"cell": 0.5}, {"cell": 0.3}]


def test_command_lines_know_the_options(capsys):
    for argv in (["--decimate-cell", "1", "--decimate-voxels", "2"],):
        with pytest.raises(SystemExit):
            TM.main(["--pair-folder", "p", "--scan-folder", "s", "--out-folder", "o", "--mesh", "m.ply"] + argv)
    assert "not allowed with" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        MD.main(["--in", "a.ply", "--out", "b.ply"])              # --cell is required
    assert "--cell" in capsys.readouterr().err


def test_eval_driver_hands_the_option_to_both_mesh_paths(tmp_path):
    """eval_driver --mesh-decimate-voxels K through its own argument parser: run_scans (DTU layout) and run_tanks call mesh_scan /
    mesh_scan_tanks with decimate_voxels = K, and with 0.0 when the option is absent.  The loaders, the fusion step and the two mesh
    functions are replaced by recorders; no view is read and no network runs."""
    import unittest.mock as mock
    import torch
    from rc_mvsnet_amd import fusion, mvs_dataset
    scene = next(iter(fusion.TANKS_FILTER["intermediate"]))
    folder = tmp_path / "tanks" / "intermediate" / scene
    folder.mkdir(parents=True)
    (folder / "pair.txt").write_text("0\n")
    testlist = tmp_path / "list.txt"
    testlist.write_text("scan1\n")

    class NoViews(list):
        metas = []

        def __init__(self, *a, **k):
            super().__init__()

    for extra, want in ((["--mesh-decimate-voxels", "2.5"], 2.5), ([], 0.0)):
        argv = ["--dataset", "tanks", "--testpath", str(tmp_path / "tanks"), "--scenes", scene, "--outdir", str(tmp_path / "out"), "--mesh", "--filter",
                "--testlist", str(testlist)] + extra
        with mock.patch.object(eval_driver, "run_tanks", lambda model, args, device, rank, world: args):
            args = eval_driver.main(argv)                            # the parser's own namespace, defaults filled in
        assert args.mesh_decimate_voxels == want
        seen = {}
        record = lambda which: (lambda *a, **kw: seen.__setitem__(which, kw) or {"mesh": which})        # noqa: E731
        with mock.patch.object(mvs_dataset, "MVSDataset", NoViews), mock.patch.object(mvs_dataset, "TanksDataset", NoViews), \
                mock.patch.object(mvs_dataset, "prefetch", lambda ds, **k: iter(())), mock.patch.object(fusion, "filter_depth", lambda *a, **k: None), \
                mock.patch.object(fusion, "filter_depth_tanks", lambda *a, **k: None), mock.patch.object(TM, "mesh_scan", record("dtu")), \
                mock.patch.object(TM, "mesh_scan_tanks", record("tanks")):
            eval_driver.run_tanks(None, args, torch.device("cpu"), 0, 1)
            eval_driver.run_scans(None, args, torch.device("cpu"), 0, 1)
        assert seen["dtu"]["decimate_voxels"] == want and seen["tanks"]["decimate_voxels"] == want
        assert "decimate_cell" not in seen["dtu"] and seen["dtu"]["smooth"] == 0


def test_coloured_ply_reader(tmp_path):
    v, f, rgb = MDC.case("rounding_colours")
    path = str(tmp_path / "a.ply")
    with open(path, "wb") as fh:
        fh.write(TM.mesh_ply_bytes(v, f, rgb))
    gv, gf, gc = dtu_io.read_ply_mesh_rgb(path)
    assert MDC.same_bits(gv, v) and np.array_equal(gf, f) and np.array_equal(gc, rgb) and gc.dtype == np.uint8
    plain = dtu_io.read_ply_mesh(path)
    assert MDC.same_bits(plain[0], v) and np.array_equal(plain[1], f)
    text = "ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
    faces = "element face 1\nproperty list uchar int vertex_indices\nend_header\n"
    with open(path, "w") as fh:
        fh.write(text + "property uchar red\nproperty uchar green\nproperty uchar blue\n" + faces + "0 0 0 1 2 3\n1 0 0 4 5 6\n0 1 0 7 8 255\n3 0 1 2\n")
    gv, gf, gc = dtu_io.read_ply_mesh_rgb(path)
    assert gc.tolist() == [[1, 2, 3], [4, 5, 6], [7, 8, 255]] and gf.tolist() == [[0, 1, 2]] and gv[2].tolist() == [0, 1, 0]
    with open(path, "w") as fh:
        fh.write(text + faces + "0 0 0\n1 0 0\n0 1 0\n3 0 1 2\n")
    assert dtu_io.read_ply_mesh_rgb(path)[2] is None


def test_header_is_an_extension_header():
    assert any(p.endswith("mesh_decimate.h") for p in _lib.EXT_HEADERS)
    for n in ("bounds", "cluster", "classify_faces", "quadrics", "place", "select"):
        plain, timed = _lib.EXT_SIGNATURES["rcmvs_md_" + n], _lib.EXT_SIGNATURES["rcmvs_md_" + n + "_timed"]
        assert timed[:len(plain) - 1] == plain[:-1] and len(timed) == len(plain) + 2
    assert "rcmvs_md_lattice" in _lib.EXT_SIGNATURES and _lib.CONSTANTS["RCMVS_VERSION"] == 106
    assert MD.MAX_CELLS_PER_AXIS == 2 ** 21 == O.MAX_CELLS == _lib.CONSTANTS["RCMVS_PC_MAX_VOXELS_PER_AXIS"] and MD.MAX_ELEMENTS == 2 ** 31 - 256
    assert (MD.FACE_KEPT, MD.FACE_INVALID, MD.FACE_UNCLUSTERED, MD.FACE_COLLAPSED, MD.FACE_DUPLICATE) == (O.KEPT, O.INVALID, O.UNCLUSTERED, O.COLLAPSED, O.DUPLICATE)
    assert (MD.VIA_QUADRIC, MD.VIA_NO_FACES, MD.VIA_SINGULAR, MD.VIA_OUTSIDE, MD.VIA_MEAN) == (O.VIA_QUADRIC, O.VIA_NO_FACES, O.VIA_SINGULAR, O.VIA_OUTSIDE, O.VIA_MEAN)
