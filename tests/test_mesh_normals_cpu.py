"""Host logic of rc_mvsnet_amd/mesh_normals.py and its hooks, without a GPU and without the emulation: the oracle's known answers,
the PLY bytes with and without normals and their readers, the options' way through tsdf_mesh, mesh_render and eval_driver, the
command lines' arguments, the header's place among the extension headers."""
import inspect
import os
import unittest.mock as mock

import numpy as np
import pytest
import torch

import mesh_normals_cases as MNC
from rc_mvsnet_amd import _lib, dtu_io, eval_driver, mesh_normals as MN, mesh_render as MR, tsdf_mesh as TM


@pytest.mark.parametrize("name,weight", MNC.case_keys())
def test_known_answers_of_the_oracle(name, weight):
    MNC.check_known(name, weight)


def test_oracle_strip_orders_and_flip():
    """the three face orders of one strip agree to rounding; swapping b and c negates the AREA normals exactly"""
    ref = {o: MNC.reference(f"strip_{o}", "area")[0].astype(np.float64) for o in ("ascending", "descending", "shuffled")}
    assert np.abs(ref["descending"] - ref["ascending"]).max() < 1e-6 and np.abs(ref["shuffled"] - ref["ascending"]).max() < 1e-6
    for name in ("fan_50", "uv_sphere", "hostile"):
        v, f = MNC.case(name)
        a, b = MNC.O.vertex_normals(v, f, "area"), MNC.O.vertex_normals(v, f[:, [0, 2, 1]], "area")
        assert (a[0] == -b[0]).all() and a[1] == b[1]


def _header(nv, nf, normals):
    extra = "property float nx\nproperty float ny\nproperty float nz\n" if normals else ""
    return (f"ply\nformat binary_little_endian 1.0\nelement vertex {nv}\nproperty float x\nproperty float y\nproperty float z\n{extra}"
            f"property uchar red\nproperty uchar green\nproperty uchar blue\nelement face {nf}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")


def test_ply_bytes_without_normals_are_what_they_were_and_with_normals_round_trip(tmp_path):
    v, f = MNC.case("uv_sphere")
    rgb = np.random.default_rng(0).integers(0, 256, (len(v), 3), dtype=np.uint8)
    n = MNC.reference("uv_sphere", "sphere")[0].copy()
    n[3] = (-0.0, 0.0, 1.0)                                          # a signed zero survives
    # without normals: the header and the records restated here, byte for byte, with colours and without
    for colours in (rgb, None):
        rec = np.empty(len(v), dtype=[("p", "<f4", (3,)), ("c", "u1", (3,))])
        rec["p"], rec["c"] = v, (255 if colours is None else colours)
        faces = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
        faces["n"], faces["i"] = 3, f
        want = _header(len(v), len(f), False) + rec.tobytes() + faces.tobytes()
        assert TM.mesh_ply_bytes(v, f, colours) == want == TM.mesh_ply_bytes(torch.from_numpy(v.copy()), torch.from_numpy(f.copy()), colours, normals=None)
    # with normals
    rec = np.empty(len(v), dtype=[("p", "<f4", (3,)), ("n", "<f4", (3,)), ("c", "u1", (3,))])
    rec["p"], rec["n"], rec["c"] = v, n, rgb
    got = TM.mesh_ply_bytes(v, f, rgb, normals=torch.from_numpy(n))
    assert got == _header(len(v), len(f), True) + rec.tobytes() + faces.tobytes()
    path = tmp_path / "n.ply"
    path.write_bytes(got)
    bv, bf, bc, bn = dtu_io.read_ply_mesh_normals(str(path))
    assert np.array_equal(MNC.bits(bv), MNC.bits(v)) and np.array_equal(bf, f) and np.array_equal(bc, rgb) and np.array_equal(MNC.bits(bn), MNC.bits(n))
    cv, cf, cc = dtu_io.read_ply_mesh_rgb(str(path))
    dv, df = dtu_io.read_ply_mesh(str(path))
    assert np.array_equal(MNC.bits(cv), MNC.bits(v)) and np.array_equal(cf, f) and np.array_equal(cc, rgb) and np.array_equal(MNC.bits(dv), MNC.bits(v)) and np.array_equal(df, f)
    assert np.array_equal(dtu_io.read_ply_xyz(str(path)), v)
    # a PLY without normals, an ascii one with them, an empty mesh
    plain = tmp_path / "plain.ply"
    plain.write_bytes(TM.mesh_ply_bytes(v, f, rgb))
    assert dtu_io.read_ply_mesh_normals(str(plain))[3] is None
    ascii_ply = tmp_path / "a.ply"
    ascii_ply.write_text("ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\n"
                         "property float nz\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n0 0 0 0 0 1\n1 0 0 0 0.6 0.8\n0 1 0 -1 0 0\n3 0 1 2\n")
    av, af, ac, an = dtu_io.read_ply_mesh_normals(str(ascii_ply))
    assert ac is None and np.array_equal(an, np.array([[0, 0, 1], [0, 0.6, 0.8], [-1, 0, 0]], np.float32)) and af.tolist() == [[0, 1, 2]]
    empty = TM.mesh_ply_bytes(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), None, normals=np.zeros((0, 3), np.float32))
    assert empty == _header(0, 0, True)
    for bad in (n[:-1], n.astype(np.float64)):
        with pytest.raises(_lib.RcmvsError, match="normals"):
            TM.mesh_ply_bytes(v, f, rgb, normals=bad)


def test_normals_are_off_by_default():
    """without the option mesh_scan hands _mesh_views what it handed it before, and _mesh_views never reaches mesh_normals"""
    for fn in (TM.mesh_scan, TM.mesh_scan_tanks):
        assert inspect.signature(fn).parameters["normals"].default is None
    assert inspect.signature(TM._mesh_views).parameters["normals"].default is None
    for fn in (MR.render, MR.render_views):
        assert inspect.signature(fn).parameters["normals"].default is None
    assert inspect.signature(TM.mesh_ply_bytes).parameters["normals"].default is None
    seen = {}

    def views_only(*args, **kw):
        seen["args"], seen["kw"] = args, kw
        return {"mesh": args[1]}

    with mock.patch.object(TM, "filtered_views", lambda *a, **k: {}), mock.patch.object(TM, "_mesh_views", views_only):
        TM.mesh_scan("p", "s", "o", "m.ply", 0.8, 3, 0.5, 0.01)
        assert seen["kw"] == {} and len(seen["args"]) == 10
        TM.mesh_scan("p", "s", "o", "m.ply", 0.8, 3, 0.5, 0.01, normals="sphere", render_dir="r")
        assert seen["kw"] == {"render": "r", "normals": {"weight": "sphere"}} and len(seen["args"]) == 10
        with pytest.raises(_lib.RcmvsError, match="weight"):
            TM.mesh_scan("p", "s", "o", "m.ply", 0.8, 3, 0.5, 0.01, normals="angle")
    with mock.patch.object(TM, "filtered_views_tanks", lambda *a, **k: {"lo": (0.0, 0.0, 0.0)}), mock.patch.object(TM, "_mesh_views", views_only):
        TM.mesh_scan_tanks("s", "o", "m.ply", 1, 0.01, 0.3, (2, 2), None, 1)
        assert seen["kw"] == {}
        TM.mesh_scan_tanks("s", "o", "m.ply", 1, 0.01, 0.3, (2, 2), None, 1, normals="area")
        assert seen["kw"] == {"normals": {"weight": "area"}}


def test_write_views_adds_the_two_images_only_with_normals(tmp_path):
    out = {"depth": torch.zeros((1, 2, 3)), "shade": torch.zeros((1, 2, 3), dtype=torch.uint8), "rgb": torch.zeros((1, 2, 3, 3), dtype=torch.uint8)}
    MR.write_views(out, str(tmp_path / "a"), ["v"])
    assert sorted(os.listdir(tmp_path / "a" / "render")) == ["v_rgb.png", "v_shade.png"]
    out.update(smooth=torch.zeros((1, 2, 3), dtype=torch.uint8), normal_rgb=torch.zeros((1, 2, 3, 3), dtype=torch.uint8), normal=torch.zeros((1, 2, 3, 3)))
    MR.write_views(out, str(tmp_path / "b"), ["v"])
    assert sorted(os.listdir(tmp_path / "b" / "render")) == ["v_normal.png", "v_rgb.png", "v_shade.png", "v_smooth.png"]


def test_command_lines_know_the_option(capsys):
    seen = {}
    record = lambda which: (lambda *a, **kw: seen.__setitem__(which, kw) or {"mesh": which})        # noqa: E731
    base = ["--pair-folder", "p", "--scan-folder", "s", "--out-folder", "o", "--mesh", "m.ply"]
    for extra, want in ((["--normals", "sphere"], "sphere"), (["--normals", "area", "--render", "d"], "area"), ([], None)):
        with mock.patch.object(TM, "mesh_scan", record("tsdf")):
            TM.main(base + extra)
        assert seen["tsdf"]["normals"] == want
    for main, argv in ((TM.main, base + ["--normals", "angle"]), (MN.main, ["--in", "a.ply"]), (MN.main, ["--in", "a.ply", "--out", "b.ply", "--weight", "angle"]),
                       (MR.main, ["--mesh", "a.ply", "--pair-folder", "p", "--scan-folder", "s", "--out", "o", "--normals", "angle"])):
        with pytest.raises(SystemExit):
            main(argv)
    assert "--normals" in capsys.readouterr().err


def test_eval_driver_hands_the_option_to_both_mesh_paths(tmp_path):
    """eval_driver --mesh-normals through its own argument parser: run_scans and run_tanks call mesh_scan / mesh_scan_tanks with
    normals = the weight, and with None when the option is absent (the recorders of test_mesh_render_cpu.py)"""
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

    for extra, want in ((["--mesh-normals", "sphere"], "sphere"), ([], None)):
        argv = ["--dataset", "tanks", "--testpath", str(tmp_path / "tanks"), "--scenes", scene, "--outdir", str(tmp_path / "out"), "--mesh", "--filter",
                "--testlist", str(testlist)] + extra
        with mock.patch.object(eval_driver, "run_tanks", lambda model, args, device, rank, world: args):
            args = eval_driver.main(argv)
        assert args.mesh_normals == want
        seen = {}
        record = lambda which: (lambda *a, **kw: seen.__setitem__(which, kw) or {"mesh": which})        # noqa: E731
        with mock.patch.object(mvs_dataset, "MVSDataset", NoViews), mock.patch.object(mvs_dataset, "TanksDataset", NoViews), \
                mock.patch.object(mvs_dataset, "prefetch", lambda ds, **k: iter(())), mock.patch.object(fusion, "filter_depth", lambda *a, **k: None), \
                mock.patch.object(fusion, "filter_depth_tanks", lambda *a, **k: None), mock.patch.object(TM, "mesh_scan", record("dtu")), \
                mock.patch.object(TM, "mesh_scan_tanks", record("tanks")):
            eval_driver.run_tanks(None, args, torch.device("cpu"), 0, 1)
            eval_driver.run_scans(None, args, torch.device("cpu"), 0, 1)
        assert seen["dtu"]["normals"] == want and seen["tanks"]["normals"] == want


def test_header_is_an_extension_header():
    assert any(p.endswith("mesh_normals.h") for p in _lib.EXT_HEADERS)
    names = sorted(k for k in _lib.EXT_SIGNATURES if k.startswith("rcmvs_mn_"))
    assert names == ["rcmvs_mn_face_normals", "rcmvs_mn_face_normals_timed", "rcmvs_mn_shade", "rcmvs_mn_shade_timed", "rcmvs_mn_vertex_normals",
                     "rcmvs_mn_vertex_normals_timed"]
    for name in names[::2]:
        plain, timed = _lib.EXT_SIGNATURES[name], _lib.EXT_SIGNATURES[name + "_timed"]
        assert timed[:len(plain) - 1] == plain[:-1] and len(timed) == len(plain) + 3                   # the phase, ev0, ev1
    assert not any(k.startswith("rcmvs_mn_") for k in _lib.SIGNATURES) and _lib.CONSTANTS["RCMVS_VERSION"] == 106 and len(_lib.SIGNATURES) == 105
    assert MN.STATS == 8 and len(MN.STAT_NAMES) == 7 and MN.STAT_NAMES == MNC.O.STAT_NAMES and MN.WEIGHTS == {"area": 0, "sphere": 1}
    assert MN.MAX_CORNERS == 2 ** 31 - 256 and MNC.radix_passes(255) == 1 and MNC.radix_passes(256) == 2 and MNC.radix_passes(65536) == 3
