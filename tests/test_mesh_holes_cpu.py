"""Hole filling without a device: tests/mesh_holes_oracle.py against hand answers (the cases of tests/mesh_holes_cases.py, which the
CPU emulation and the GPU run against that oracle), the options and their way through mesh_scan and the three command lines, and
the header's place in the binding."""
import inspect
import unittest.mock as mock

import numpy as np
import pytest

import mesh_clean_cases as MCC
import mesh_holes_cases as MHC
import mesh_holes_oracle as O
from rc_mvsnet_amd import _lib, eval_driver, mesh_clean as MC, mesh_holes as MH, tsdf_mesh as TM


# ---- the oracle -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", MHC.case_keys())
def test_oracle_gives_the_hand_answers(name, k):
    MHC.check_known(name, k)


def test_oracle_by_hand_on_an_open_quad():
    """(0, 1, 2), (2, 1, 3): the rim runs 0 -> 1 -> 3 -> 2 -> 0; the new vertex is the mean, its colour the mean rounded half up"""
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [2, 2, 1]], np.float32)
    rgb = np.array([[0, 10, 255], [1, 20, 255], [2, 30, 255], [2, 41, 254]], np.uint8)
    f = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    b = O.boundary(4, f)
    assert b["succ"].tolist() == [1, 3, 0, 2] and b["pred"].tolist() == [2, 0, 3, 1] and b["flags"].tolist() == [O.SIMPLE] * 4
    assert O.loops(b) == [[0, 1, 3, 2]]
    wv, wf, wc, stats, loops = O.fill_holes(v, f, rgb, 4)
    assert wv[4].tolist() == [1.0, 1.0, 0.25] and wc[4].tolist() == [1, 25, 255]
    assert wf[2:].tolist() == [[1, 0, 4], [3, 1, 4], [2, 3, 4], [0, 2, 4]]
    assert stats == {"boundary_edges": 4, "complex_vertices": 0, "loops_filled": 1, "loops_filled_by_one_face": 0, "longest_filled": 4, "vertices_added": 1,
                     "faces_added": 4, "boundary_edges_left": 0}
    assert O.fill_holes(v, f, rgb, 3)[3]["boundary_edges_left"] == 4
    tri = O.fill_holes(v[:3], f[:1], None, 3)
    assert tri[1].tolist() == [[0, 1, 2], [0, 2, 1]] and tri[2] is None and len(tri[0]) == 3


def test_oracle_sums_in_loop_order_from_the_leader():
    """members whose fp64 sum depends on the order: 1e30 first or last changes the mean; the oracle's is the loop order's"""
    v, f, rgb = MCC.fan(4)                                       # the rim 0 -> 1 -> ... -> 5 -> 0
    v = v.copy()
    v[:, 0] = [1e30, 1.0, -1e30, 1.0, 1.0, 1.0]
    wv = O.fill_holes(v, f, rgb, 6)[0]
    s = np.float64(0.0)
    for u in range(6):
        s = s + np.float64(v[u, 0])
    assert wv[6, 0] == np.float32(s / 6.0) and wv[6, 0] == np.float32(0.5) and np.float32(sum(sorted(np.float64(v[:, 0]))) / 6.0) != wv[6, 0]


def test_composite_oracle_is_the_clean_up_oracle_when_off():
    v, f, rgb = MCC.case("tets_hole")
    off, plain = O.clean_mesh(v, f, rgb, smooth_iterations=2), MCC.O.clean_mesh(v, f, rgb, smooth_iterations=2)
    assert off[3] == plain[3] and MCC.same_bits(off[0], plain[0]) and "holes" not in off[3]
    on = O.clean_mesh(v, f, rgb, smooth_iterations=2, fill_holes=3)
    assert on[3]["holes"]["faces_added"] == 1 and on[3]["boundary_edges"] == 0 and on[3]["euler_characteristic"] == 2 and on[3]["faces_out"] == len(f) + 1
    assert not MCC.same_bits(on[0], plain[0])                   # the former rim is no longer pinned


# ---- host logic -------------------------------------------------------------------------------------------------------------
def test_options():
    assert MC.clean_options() is None and MC.clean_options(0, 0.0, 0, 0, 0) is None and MC.clean_options(fill_holes=0) is None
    assert MC.clean_options(keep_largest=1) == {"min_faces": 0, "min_fraction": 0.0, "keep_largest": 1, "smooth_iterations": 0}
    assert MC.clean_options(fill_holes=64) == {"min_faces": 0, "min_fraction": 0.0, "keep_largest": 0, "smooth_iterations": 0, "fill_holes": 64}
    assert MC.clean_options(1, 0.5, 2, 3, 4) == {"min_faces": 1, "min_fraction": 0.5, "keep_largest": 2, "smooth_iterations": 3, "fill_holes": 4}
    assert inspect.signature(MC.clean_mesh).parameters["fill_holes"].default == 0
    p = inspect.signature(MH.fill_holes).parameters
    assert p["max_edges"].kind is inspect.Parameter.KEYWORD_ONLY and p["max_edges"].default is inspect.Parameter.empty and p["rgb"].default is None
    assert MH.MAX_EDGES == O.MAX_EDGES == 4096 and (MH.NONE, MH.SIMPLE, MH.COMPLEX) == (O.NONE, O.SIMPLE, O.COMPLEX)
    for value in (2, MH.MAX_EDGES + 1, -1, 3.0, True, None):
        with pytest.raises(_lib.RcmvsError, match="max_edges"):
            MH.max_edges_argument(value, "test")
        with pytest.raises(O.Refused):
            O.fill_holes(np.zeros((3, 3), np.float32), np.array([[0, 1, 2]]), None, value)
    assert MH.max_edges_argument(3, "test") == 3 and MH.max_edges_argument(np.int64(4096), "test") == 4096
    with pytest.raises(_lib.RcmvsError, match="2\\^31"):
        MH.check_output_counts(2 ** 31 - 1, 0, 1, 0, "test")
    with pytest.raises(_lib.RcmvsError, match="2\\^31"):
        MH.check_output_counts(0, 2 ** 31 - 4096, 0, 4096, "test")
    MH.check_output_counts(2 ** 31 - 2, 2 ** 31 - 4097, 1, 4096, "test")


def test_argument_refusals():
    import torch
    v, f = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    rgb = torch.zeros((3, 3), dtype=torch.uint8)
    bad = [((v.double(), f), {"max_edges": 8}, "verts"), ((v, f.long()), {"max_edges": 8}, "faces"), ((v, f, rgb[:2]), {"max_edges": 8}, "rgb"),
           ((v, f), {"max_edges": 2}, "max_edges"), ((v, f), {"max_edges": 4097}, "max_edges"), ((v, f), {"max_edges": 8.5}, "max_edges")]
    for args, kw, pattern in bad:
        with pytest.raises(_lib.RcmvsError, match=pattern):
            MH.fill_holes(*args, **kw)
    with pytest.raises(TypeError):
        MH.fill_holes(v, f)                                       # max_edges has no default
    for value, pattern in ((-1, "fill_holes"), (1.5, "fill_holes"), (2, "max_edges"), (4097, "max_edges")):
        with pytest.raises(_lib.RcmvsError, match=pattern):
            MC.clean_mesh(v, f, fill_holes=value)
    with pytest.raises(_lib.RcmvsError, match="GPU"):                        # a CPU tensor outside the emulation: no fallback
        MH.fill_holes(v, f, max_edges=8)
    with pytest.raises(_lib.RcmvsError, match="GPU"):
        MH.boundary(3, f)


def test_hole_filling_is_off_by_default():
    """without the option mesh_scan hands _mesh_views what it handed it before; with it, the clean-up options carry fill_holes; and
    clean_mesh with 0 never reaches mesh_holes"""
    for fn in (TM.mesh_scan, TM.mesh_scan_tanks):
        assert inspect.signature(fn).parameters["fill_holes"].default == 0
    seen = {}

    def views_only(*args, **kw):
        seen["args"], seen["kw"] = args, kw
        return {"mesh": args[1]}

    with mock.patch.object(TM, "filtered_views", lambda *a, **k: {}), mock.patch.object(TM, "_mesh_views", views_only):
        TM.mesh_scan("p", "s", "o", "m.ply", 0.8, 3, 0.5, 0.01)
        assert seen["kw"] == {} and len(seen["args"]) == 10 and seen["args"][-1] is None
        TM.mesh_scan("p", "s", "o", "m.ply", 0.8, 3, 0.5, 0.01, smooth=1)
        assert seen["args"][-1] == {"min_faces": 0, "min_fraction": 0.0, "keep_largest": 0, "smooth_iterations": 1}
        TM.mesh_scan("p", "s", "o", "m.ply", 0.8, 3, 0.5, 0.01, fill_holes=32)
        assert seen["kw"] == {} and seen["args"][-1] == {"min_faces": 0, "min_fraction": 0.0, "keep_largest": 0, "smooth_iterations": 0, "fill_holes": 32}
    with mock.patch.object(TM, "filtered_views_tanks", lambda *a, **k: {"lo": (0.0, 0.0, 0.0)}), mock.patch.object(TM, "_mesh_views", views_only):
        TM.mesh_scan_tanks("s", "o", "m.ply", 1, 0.01, 0.3, (2, 2), None, 1, fill_holes=16, keep_largest=1)
        assert seen["args"][-1]["fill_holes"] == 16 and seen["args"][-1]["keep_largest"] == 1

    def never(*a, **k):
        raise AssertionError("mesh_holes ran without the option")

    info = {"components_in": 0, "components_kept": 0, "largest_component_faces": 0, "faces_out": 0, "vertices_out": 0}
    import torch
    v, f = torch.zeros((0, 3)), torch.zeros((0, 3), dtype=torch.int32)
    adj = {"edges": 0, "boundary_edges": 0, "nonmanifold_edges": 0, "referenced_vertices": 0}
    with mock.patch.object(MC, "components", lambda *a: {"counts": torch.zeros(4, dtype=torch.int64)}), \
            mock.patch.object(MC, "compact", lambda *a, **k: (v, f, None, info)), mock.patch.object(MC, "adjacency", lambda *a: adj), \
            mock.patch.object(MH, "fill_holes", never):
        stats = MC.clean_mesh(v, f)[3]
        assert list(stats) == ["vertices_in", "vertices_out", "faces_in", "faces_out", "invalid_faces", "components_in", "components_kept",
                               "largest_component_faces", "unreferenced_removed", "edges", "boundary_edges", "nonmanifold_edges", "euler_characteristic",
                               "smooth_iterations"]
        assert MC.clean_mesh(v, f, fill_holes=0)[3] == stats
        with pytest.raises(AssertionError, match="without the option"):
            MC.clean_mesh(v, f, fill_holes=8)


def test_command_lines_know_the_option(tmp_path, capsys):
    seen = {}
    record = lambda which: (lambda *a, **kw: seen.__setitem__(which, kw) or {"mesh": which})        # noqa: E731
    base = ["--pair-folder", "p", "--scan-folder", "s", "--out-folder", "o", "--mesh", "m.ply"]
    for sparse in ([], ["--sparse"]):
        for extra, want in ((["--fill-holes", "48"], 48), ([], 0)):
            with mock.patch.object(TM, "mesh_scan", record("tsdf")):
                TM.main(base + sparse + extra)
            assert seen["tsdf"]["fill_holes"] == want and seen["tsdf"]["sparse"] == bool(sparse)
    with pytest.raises(SystemExit):
        TM.main(base + ["--fill-holes", "many"])
    assert "--fill-holes" in capsys.readouterr().err
    clean = {}
    from rc_mvsnet_amd import dtu_io
    with mock.patch.object(MC, "clean_mesh", lambda v, f, c, **kw: clean.update(kw) or (v, f, c, {})), mock.patch.object(TM, "mesh_ply_bytes", lambda *a: b""), \
            mock.patch.object(dtu_io, "read_ply_mesh", lambda path: (np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.int32))):
        for extra, want in ((["--fill-holes", "12"], 12), ([], 0)):
            MC.main(["--in", "a.ply", "--out", str(tmp_path / "b.ply"), "--device", "cpu"] + extra)
            assert clean["fill_holes"] == want


def test_eval_driver_hands_the_option_to_both_mesh_paths(tmp_path):
    """eval_driver --mesh-fill-holes N through its own argument parser: run_scans (DTU layout) and run_tanks call mesh_scan /
    mesh_scan_tanks with fill_holes = N, and with 0 when the option is absent (the recorders of test_mesh_decimate_cpu.py)"""
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

    for extra, want in ((["--mesh-fill-holes", "40"], 40), ([], 0)):
        argv = ["--dataset", "tanks", "--testpath", str(tmp_path / "tanks"), "--scenes", scene, "--outdir", str(tmp_path / "out"), "--mesh", "--filter",
                "--testlist", str(testlist)] + extra
        with mock.patch.object(eval_driver, "run_tanks", lambda model, args, device, rank, world: args):
            args = eval_driver.main(argv)
        assert args.mesh_fill_holes == want
        seen = {}
        record = lambda which: (lambda *a, **kw: seen.__setitem__(which, kw) or {"mesh": which})        # noqa: E731
        with mock.patch.object(mvs_dataset, "MVSDataset", NoViews), mock.patch.object(mvs_dataset, "TanksDataset", NoViews), \
                mock.patch.object(mvs_dataset, "prefetch", lambda ds, **k: iter(())), mock.patch.object(fusion, "filter_depth", lambda *a, **k: None), \
                mock.patch.object(fusion, "filter_depth_tanks", lambda *a, **k: None), mock.patch.object(TM, "mesh_scan", record("dtu")), \
                mock.patch.object(TM, "mesh_scan_tanks", record("tanks")):
            eval_driver.run_tanks(None, args, torch.device("cpu"), 0, 1)
            eval_driver.run_scans(None, args, torch.device("cpu"), 0, 1)
        assert seen["dtu"]["fill_holes"] == want and seen["tanks"]["fill_holes"] == want and seen["dtu"]["smooth"] == 0


def test_header_is_an_extension_header():
    assert any(p.endswith("mesh_holes.h") for p in _lib.EXT_HEADERS)
    for n in ("boundary", "leaders", "emit"):
        plain, timed = _lib.EXT_SIGNATURES["rcmvs_mh_" + n], _lib.EXT_SIGNATURES["rcmvs_mh_" + n + "_timed"]
        assert timed[:len(plain) - 1] == plain[:-1] and len(timed) == len(plain) + 2
    assert sorted(k for k in _lib.EXT_SIGNATURES if k.startswith("rcmvs_mh_")) == sorted("rcmvs_mh_" + n + t for n in ("boundary", "leaders", "emit")
                                                                                       for t in ("", "_timed"))
    assert not any(k.startswith("rcmvs_mh_") for k in _lib.SIGNATURES) and _lib.CONSTANTS["RCMVS_VERSION"] == 106 and len(_lib.SIGNATURES) == 105
    assert _lib.CONSTANTS["RCMVS_MH_MAX_EDGES"] == 4096 and MH.SCAN_TILE == MC.SCAN_TILE
