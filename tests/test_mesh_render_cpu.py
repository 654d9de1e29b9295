"""The mesh rasteriser without a device: tests/mesh_render_oracle.py against hand answers (the cases of tests/mesh_render_cases.py,
which the CPU emulation and the GPU run against that oracle), the options and their way through mesh_scan and the command lines,
and the header's place in the binding."""
import inspect
import unittest.mock as mock

import numpy as np
import pytest

import mesh_render_cases as MRC
import mesh_render_oracle as O
from rc_mvsnet_amd import _lib, eval_driver, mesh_render as MR, tsdf_mesh as TM


# ---- the oracle -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,W,H,cull", MRC.case_keys())
def test_oracle_gives_the_hand_answers(name, W, H, cull):
    MRC.check_known(name, W, H, cull)


def test_oracle_by_hand_on_one_pixel():
    """the triangle (0,0), (2,0), (0,2) at depths 1, 2, 4 on a 2 x 2 image: the vertex (0,0) lies on a top and a left edge, so pixel
    (0,0) is inside with the weights (area2, 0, 0) and depth exactly 1; pixel (1,0) lies on the top edge, halfway: 1 / z is the mean
    of 1 and 1/2; pixel (0,1) on the left edge: the mean of 1 and 1/4; pixel (1,1) lies on the hypotenuse, which owns nothing"""
    v, f, c = MRC.pix_mesh([(0, 0, 1), (2, 0, 2), (0, 2, 4)], [(0, 1, 2)])
    c = np.array([[10, 0, 0], [20, 0, 0], [40, 0, 0]], np.uint8)
    r = O.render(v, f, c, MRC.PIX[None], 2, 2, 0.5)
    assert r["face"][0].tolist() == [[0, 0], [0, -1]]
    assert r["depth"][0].tolist() == [[1.0, np.float32(1 / 0.75)], [np.float32(1 / 0.625), 0.0]]
    assert int(r["keys"][0, 0, 0]) == (0x3F800000 << 32) and int(r["keys"][0, 1, 1]) == 2 ** 64 - 1
    # perspective-correct colours: (1 * 10 + 0.5 * 20) / 1.5 = 13.33 -> 13; (1 * 10 + 0.25 * 40) / 1.25 = 16
    assert r["rgb"][0][..., 0].tolist() == [[10, 13], [16, 0]]
    assert r["stats"] == [{"faces_drawn": 1, "faces_clipped": 0, "faces_degenerate": 0, "faces_culled": 0, "faces_invalid": 0, "faces_large": 0, "pixels_covered": 3}]
    # the normal of ((0,0,1), (4,0,2), (0,8,4)): (1,0,... ) x ... = (-8, -12, 32): |nz| / |n| = 32 / sqrt(1232) -> 232
    assert r["shade"][0].tolist() == [[232, 232], [232, 0]]
    back = O.render(v, f, c, MRC.PIX[None], 2, 2, 0.5, "back")               # (b - a) x (c - a) has nz > 0: it points away from the camera
    assert back["stats"][0]["faces_culled"] == 1 and (back["face"] == -1).all()
    flipped = O.render(v, f[:, ::-1], c, MRC.PIX[None], 2, 2, 0.5, "back")
    assert np.array_equal(flipped["depth"], r["depth"]) and np.array_equal(flipped["keys"], r["keys"])


def test_oracle_lattice_and_guard():
    c = MRC.PIX
    xc, yc, zc = (np.array(a, np.float64) for a in ([1.0, 2.0 ** 17, np.nextafter(2.0 ** 17, np.inf), 3.0 / 512 * 2], [0.0] * 4, [2.0] * 4))
    X, Y, ok = O.project(c, 0.5, xc, yc, zc)
    assert ok.tolist() == [True, True, False, True] and X.tolist() == [128, 2 ** 24, 0, 2]      # 3/512 px is 1.5 lattice steps: half rounds up
    assert O.floor_pixel(-1) == -1 and O.ceil_pixel(-1) == 0 and O.floor_pixel(255) == 0 and O.ceil_pixel(257) == 2 and O.ceil_pixel(-256) == -1


def test_oracle_compare_by_hand():
    r = np.array([[[2.0, 0.0, 3.0, np.nan, 1.0, 4.05]]], np.float32)
    d = np.array([[[2.0, 1.0, 0.0, 5.0, -1.0, 4.0]]], np.float32)
    row = O.compare(r, d, (0.0, 0.01, 0.02))[0]
    assert (row["both"], row["only_mesh"], row["only_map"], row["within"]) == (2, 2, 2, [1, 1, 2])
    assert row["sum_abs"] == float(np.float32(4.05)) - 4.0 and row["mean_abs"] == row["sum_abs"] / 2


# ---- host logic -------------------------------------------------------------------------------------------------------------
def test_constants_agree():
    assert (MR.MAX_SIDE, MR.SMALL_SIDE) == (O.MAX_SIDE, O.SMALL_SIDE) == (16384, 8) and MR.STAT_NAMES == O.STAT_NAMES and len(MR.STAT_NAMES) < MR.STATS
    assert len(MR.TRACE_NAMES) == MR.TRACE and MR.PROJ_BYTES % 8 == 0 and MR.CULL == {"none": 0, "back": 1}
    p = inspect.signature(MR.render).parameters
    assert p["cull"].default == "none" and p["background"].default == (0, 0, 0) and p["near"].default > 0


def test_argument_refusals_and_no_fallback():
    import torch
    v, f = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    rgb = torch.zeros((3, 3), dtype=torch.uint8)
    cams = MRC.PIX[None]
    bad = [((v.double(), f, None, cams, 4, 4), {}, "verts"), ((v, f.long(), None, cams, 4, 4), {}, "faces"), ((v, f, rgb[:2], cams, 4, 4), {}, "rgb"),
           ((v, f, rgb, cams, 0, 4), {}, "H"), ((v, f, rgb, cams, 4, 16385), {}, "W"), ((v, f, rgb, cams, 4, 4), {"near": 0.0}, "near"),
           ((v, f, rgb, cams, 4, 4), {"near": "close"}, "near"), ((v, f, rgb, np.zeros((0, 16)), 4, 4), {}, "views"), ((v, f, rgb, cams, 4, 4), {"cull": "front"}, "cull"),
           ((v, f, rgb, cams, 4, 4), {"background": (1, 2)}, "background")]
    for args, kw, pattern in bad:
        with pytest.raises(_lib.RcmvsError, match=pattern):
            MR.render(*args, **kw)
    with pytest.raises(_lib.RcmvsError, match="GPU"):                        # a CPU tensor outside the emulation: no fallback
        MR.render(v, f, rgb, cams, 4, 4)
    with pytest.raises(_lib.RcmvsError, match="GPU"):
        MR.compare(torch.zeros((1, 2, 2)), torch.zeros((1, 2, 2)))
    with pytest.raises(_lib.RcmvsError, match="thresholds"):
        MR.compare(torch.zeros((1, 2, 2)), torch.zeros((1, 2, 2)), (0.1, 0.2, 0.3, 0.4))


def test_sum_rows():
    rows = [{"both": 2, "only_mesh": 1, "only_map": 0, "within": [1, 2], "sum_abs": 0.5, "mean_abs": 0.25},
            {"both": 0, "only_mesh": 0, "only_map": 3, "within": [0, 0], "sum_abs": 0.0, "mean_abs": None}]
    assert MR.sum_rows(rows, (0.1, 0.2)) == {"views": 2, "thresholds": [0.1, 0.2], "both": 2, "only_mesh": 1, "only_map": 3, "within": [1, 2], "sum_abs": 0.5,
                                             "mean_abs": 0.25}
    assert MR.sum_rows(rows[1:], (0.1, 0.2))["mean_abs"] is None


def test_the_hook_names_its_files_by_the_views_numbers():
    """render_views writes <view>.pfm under the reference views' numbers of pair.txt, which need not be 0 .. V-1 in order"""
    import torch
    seen = {}
    views = {"depth": torch.zeros((3, 2, 2)), "cams": np.zeros((3, 16)), "ids": [7, 0, 12]}
    out = {"depth": views["depth"], "stats": torch.zeros((3, MR.STATS), dtype=torch.int64)}
    row = {"both": 0, "only_mesh": 0, "only_map": 0, "within": [0, 0, 0], "sum_abs": 0.0, "mean_abs": None}
    with mock.patch.object(MR, "render", lambda *a, **k: out), mock.patch.object(MR, "compare", lambda *a, **k: [row] * 3), \
            mock.patch.object(MR, "write_views", lambda out, out_dir, names, png=True: seen.update(names=names, dir=out_dir)):
        total = MR.render_views(None, None, None, views, "dir")
        assert seen == {"names": ["00000007", "00000000", "00000012"], "dir": "dir"} and total["views"] == 3
        seen.clear()
        MR.render_views(None, None, None, views)
        assert seen == {}


def test_rendering_is_off_by_default():
    """without the option mesh_scan hands _mesh_views what it handed it before, and _mesh_views never reaches mesh_render"""
    for fn in (TM.mesh_scan, TM.mesh_scan_tanks):
        assert inspect.signature(fn).parameters["render_dir"].default is None
    assert inspect.signature(TM._mesh_views).parameters["render"].default is None
    seen = {}

    def views_only(*args, **kw):
        seen["args"], seen["kw"] = args, kw
        return {"mesh": args[1]}

    with mock.patch.object(TM, "filtered_views", lambda *a, **k: {}), mock.patch.object(TM, "_mesh_views", views_only):
        TM.mesh_scan("p", "s", "o", "m.ply", 0.8, 3, 0.5, 0.01)
        assert seen["kw"] == {} and len(seen["args"]) == 10
        TM.mesh_scan("p", "s", "o", "m.ply", 0.8, 3, 0.5, 0.01, render_dir="r")
        assert seen["kw"] == {"render": "r"} and len(seen["args"]) == 10
    with mock.patch.object(TM, "filtered_views_tanks", lambda *a, **k: {"lo": (0.0, 0.0, 0.0)}), mock.patch.object(TM, "_mesh_views", views_only):
        TM.mesh_scan_tanks("s", "o", "m.ply", 1, 0.01, 0.3, (2, 2), None, 1)
        assert seen["kw"] == {}
        TM.mesh_scan_tanks("s", "o", "m.ply", 1, 0.01, 0.3, (2, 2), None, 1, render_dir="t")
        assert seen["kw"] == {"render": "t"}


def test_command_lines_know_the_option(capsys):
    seen = {}
    record = lambda which: (lambda *a, **kw: seen.__setitem__(which, kw) or {"mesh": which})        # noqa: E731
    base = ["--pair-folder", "p", "--scan-folder", "s", "--out-folder", "o", "--mesh", "m.ply"]
    for extra, want in ((["--render", "dir"], "dir"), ([], None)):
        with mock.patch.object(TM, "mesh_scan", record("tsdf")):
            TM.main(base + extra)
        assert seen["tsdf"]["render_dir"] == want
    with pytest.raises(SystemExit):
        MR.main(["--mesh", "a.ply"])
    assert "--pair-folder" in capsys.readouterr().err


def test_eval_driver_hands_the_option_to_both_mesh_paths(tmp_path):
    """eval_driver --mesh-render DIR through its own argument parser: run_scans and run_tanks call mesh_scan / mesh_scan_tanks with
    render_dir = DIR/<scan>, and with None when the option is absent (the recorders of test_mesh_holes_cpu.py)"""
    import os

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

    for extra, want in ((["--mesh-render", "rr"], "rr"), ([], None)):
        argv = ["--dataset", "tanks", "--testpath", str(tmp_path / "tanks"), "--scenes", scene, "--outdir", str(tmp_path / "out"), "--mesh", "--filter",
                "--testlist", str(testlist)] + extra
        with mock.patch.object(eval_driver, "run_tanks", lambda model, args, device, rank, world: args):
            args = eval_driver.main(argv)
        assert args.mesh_render == want
        seen = {}
        record = lambda which: (lambda *a, **kw: seen.__setitem__(which, kw) or {"mesh": which})        # noqa: E731
        with mock.patch.object(mvs_dataset, "MVSDataset", NoViews), mock.patch.object(mvs_dataset, "TanksDataset", NoViews), \
                mock.patch.object(mvs_dataset, "prefetch", lambda ds, **k: iter(())), mock.patch.object(fusion, "filter_depth", lambda *a, **k: None), \
                mock.patch.object(fusion, "filter_depth_tanks", lambda *a, **k: None), mock.patch.object(TM, "mesh_scan", record("dtu")), \
                mock.patch.object(TM, "mesh_scan_tanks", record("tanks")):
            eval_driver.run_tanks(None, args, torch.device("cpu"), 0, 1)
            eval_driver.run_scans(None, args, torch.device("cpu"), 0, 1)
        assert seen["dtu"]["render_dir"] == (None if want is None else os.path.join(want, "scan1"))
        assert seen["tanks"]["render_dir"] == (None if want is None else os.path.join(want, scene))


def test_header_is_an_extension_header():
    assert any(p.endswith("mesh_render.h") for p in _lib.EXT_HEADERS)
    names = sorted(k for k in _lib.EXT_SIGNATURES if k.startswith("rcmvs_mr_"))
    assert names == ["rcmvs_mr_compare", "rcmvs_mr_compare_timed", "rcmvs_mr_render", "rcmvs_mr_render_timed"]
    plain, timed = _lib.EXT_SIGNATURES["rcmvs_mr_render"], _lib.EXT_SIGNATURES["rcmvs_mr_render_timed"]
    assert timed[:len(plain) - 1] == plain[:-1] and len(timed) == len(plain) + 3                   # the phase, ev0, ev1
    plain, timed = _lib.EXT_SIGNATURES["rcmvs_mr_compare"], _lib.EXT_SIGNATURES["rcmvs_mr_compare_timed"]
    assert timed[:len(plain) - 1] == plain[:-1] and len(timed) == len(plain) + 2
    assert not any(k.startswith("rcmvs_mr_") for k in _lib.SIGNATURES) and _lib.CONSTANTS["RCMVS_VERSION"] == 106 and len(_lib.SIGNATURES) == 105
