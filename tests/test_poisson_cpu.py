"""Host logic of the Poisson reconstruction (rc_mvsnet_amd/poisson_mesh.py, fusion.py, eval_driver.py) without a GPU: the binding of
csrc/poisson.h, the refusals of the C entry points (they check their arguments on the host), the grid plan and the levels, the command
line's refusal of a cloud without normals, the evaluation driver's options through its parser, the oracle's own known answers, and
csrc/poisson_math.h under the address and undefined-behaviour sanitizers as a stand-alone program."""
import argparse
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import poisson_cases as C
import poisson_oracle as O
from rc_mvsnet_amd import _lib, eval_driver, fusion, poisson_mesh as PM

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "rc_mvsnet_amd", "csrc")


def test_the_header_is_bound_and_its_entry_points_are_exported():
    assert os.path.join(CSRC, "poisson.h") in _lib.EXT_HEADERS and _lib.REQUIRED_VERSION == 106
    names = [n for n in _lib.EXT_SIGNATURES if n.startswith("rcmvs_po_")]
    assert sorted(names) == sorted(f"rcmvs_po_{f}{t}" for f in ("splat", "rhs", "solve", "iso", "field") for t in ("", "_timed"))
    for n in names:
        if not n.endswith("_timed"):                             # a twin is its entry point plus (phase, ev0, ev1) before the stream
            assert _lib.EXT_SIGNATURES[n + "_timed"] == _lib.EXT_SIGNATURES[n][:-1] + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert (PM.MAX_VOXELS, PM.MAX_CYCLES, PM.ACC, PM.COUNTERS, PM.STATS) == (2 ** 27, 64, 7, 8, 8)
    assert _lib.CONSTANTS["RCMVS_PO_COARSEST_SWEEPS"] == O.COARSEST_SWEEPS and PM.MAX_LEVELS == O.MAX_LEVELS
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, n) for n in names)


def test_refused_before_any_launch():
    """the C entry points check their arguments on the host: no GPU is needed to be refused"""
    lib = _lib.load()
    g, big, zero = (ctypes.c_double * 4)(0, 0, 0, 1.0), (ctypes.c_int * 3)(1024, 512, 512), (ctypes.c_int * 3)(8, 0, 8)
    d, h0 = (ctypes.c_int * 3)(8, 8, 8), (ctypes.c_double * 4)(0, 0, 0, 0.0)
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)                                                           # noqa: E731
    err = lib.rcmvs_last_error_string
    none17 = [None] * 10
    assert lib.rcmvs_po_splat(None, None, None, -1, 1, p(g), p(d), *none17, None) < 0 and b"n = -1" in err()
    assert lib.rcmvs_po_splat(None, None, None, 1 << 31, 1, p(g), p(d), *none17, None) < 0 and b"n = 2147483648" in err()
    assert lib.rcmvs_po_splat(None, None, None, 4, 1, p(g), p(big), *none17, None) < 0 and b"at most 2^27 voxels" in err()
    assert lib.rcmvs_po_splat(None, None, None, 4, 1, p(g), p(zero), *none17, None) < 0 and b"every side >= 1" in err()
    assert lib.rcmvs_po_splat(None, None, None, 4, 1, p(h0), p(d), *none17, None) < 0 and b"h > 0" in err()
    assert lib.rcmvs_po_splat(None, None, None, 4, 1, p(g), p(d), *none17, None) < 0 and b"null pointer" in err()
    assert lib.rcmvs_po_rhs(None, None, None, p(g), p(d), None, None) < 0 and b"null pointer" in err()
    assert lib.rcmvs_po_solve(None, None, None, None, p(g), p(d), 65, None, None, None) < 0 and b"cycles = 65" in err()
    assert lib.rcmvs_po_solve(None, None, None, None, p(g), p(d), -1, None, None, None) < 0 and b"cycles = -1" in err()
    assert lib.rcmvs_po_solve(None, None, None, None, p(g), p(big), 1, None, None, None) < 0 and b"at most 2^27 voxels" in err()
    assert lib.rcmvs_po_iso(None, None, -1, None, p(g), p(d), None, None, None, None) < 0 and b"n = -1" in err()
    assert lib.rcmvs_po_field(None, None, None, -0.5, p(d), None, None, None, None) < 0 and b"trim = -0.5" in err()
    assert lib.rcmvs_po_field(None, None, None, float("nan"), p(d), None, None, None, None) < 0 and b"trim = nan" in err()
    assert lib.rcmvs_po_field(None, None, None, 0.0, p(zero), None, None, None, None) < 0 and b"every side >= 1" in err()
    assert lib.rcmvs_po_field_timed(None, None, None, 0.0, p(d), None, None, None, 1, None, None, None) < 0 and b"phase = 1" in err()


def test_the_levels_and_the_grid_plan():
    assert PM.level_dims([16, 16, 16]) == [[16] * 3, [8] * 3, [4] * 3] == O.levels([16, 16, 16])
    assert PM.level_dims([512, 512, 512])[-1] == [4, 4, 4] and len(PM.level_dims([512] * 3)) == 8
    for dims in ([32, 16, 16], [16, 32, 48], [24] * 3, [8] * 3, [12] * 3, [6] * 3, [10, 6, 12], [9, 8, 8], [1, 1, 1], [256, 256, 176]):
        assert PM.level_dims(dims) == O.levels(dims)
    origin, h, dims = PM.plan_grid([-1, -1, -1], [1, 1, 1], resolution=256)
    assert dims == [256] * 3 and h == 2.5 / 256 and origin == [-1.25] * 3
    origin, h, dims = PM.plan_grid([0, 0, 0], [4, 2, 1], resolution=100, scale=1.0, multiple=16)
    assert h == 0.04 and dims == [112, 64, 32] and np.allclose(origin, [2 - 56 * h, 1 - 32 * h, 0.5 - 16 * h])
    assert all(lo <= 0 and lo + n * h >= s for lo, n, s in zip(origin, dims, (4, 2, 1)))
    for bad in (dict(lo=[0, 0, 0], hi=[0, 0, 0]), dict(lo=[0, 0, np.nan], hi=[1, 1, 1]), dict(lo=[1, 0, 0], hi=[0, 1, 1]), dict(lo=[0] * 3, hi=[1] * 3, scale=0.5),
                dict(lo=[0] * 3, hi=[1] * 3, multiple=0), dict(lo=[0] * 3, hi=[1] * 3, resolution=2.5)):
        with pytest.raises(_lib.RcmvsError, match="plan_grid"):
            PM.plan_grid(**bad)


def test_the_oracles_known_answers():
    C.check_case_answers()
    C.check_sphere(None, 16)
    C.check_trim(None, 16)
    C.check_plane(None)


def test_the_command_line_refuses_a_cloud_without_normals(tmp_path, capsys):
    xyz = C.sphere_points(20)
    src = str(tmp_path / "cloud.ply")
    with open(src, "wb") as f:
        f.write(fusion.ply_bytes(xyz, np.zeros((20, 3), np.uint8)))
    with pytest.raises(SystemExit):
        PM.main(["--in", src, "--out", str(tmp_path / "mesh.ply")])
    assert "cloud_clean --normals" in capsys.readouterr().err and not os.path.exists(tmp_path / "mesh.ply")
    with pytest.raises(SystemExit):
        PM.main(["--in", src, "--out", str(tmp_path / "mesh.ply"), "--trim", "0.1", "--trim-relative", "0.1"])
    assert "not allowed with" in capsys.readouterr().err


def test_driver_options(tmp_path, capsys):
    assert PM.poisson_options() is None and PM.poisson_options(False, 512, 0.1, 4) is None
    assert PM.poisson_options(True) == {"resolution": 256, "trim_relative": None, "cycles": 8}
    assert PM.poisson_options(True, 128, 0.05, 4) == {"resolution": 128, "trim_relative": 0.05, "cycles": 4}
    for fn in (fusion.filter_depth, fusion.filter_depth_tanks, fusion._write_cloud):
        assert inspect.signature(fn).parameters["poisson"].default is None
    opts, stats = {"resolution": 64, "trim_relative": None, "cycles": 8}, {}
    ns = argparse.Namespace(cloud_options={"normals": 8}, fusion_options={}, poisson_options=opts)
    assert eval_driver.cloud_keywords(ns, stats) == {"clean": {"normals": 8}, "stats": stats, "poisson": opts}
    ns = argparse.Namespace(cloud_options={"normals": 8}, fusion_options={}, poisson_options=None)
    assert eval_driver.cloud_keywords(ns, stats) == {"clean": {"normals": 8}, "stats": stats}
    assert eval_driver.cloud_summary({"cloud": {"out": 3}, "poisson": {"faces": 9}, "views": []}) == {"cloud": {"out": 3}, "poisson": {"faces": 9}}
    assert eval_driver.cloud_summary({"cloud": {"out": 3}}) == {"cloud": {"out": 3}}
    # --poisson without --cloud-normals is a parser error
    with pytest.raises(SystemExit) as e:
        eval_driver.main(["--outdir", str(tmp_path), "--filter", "--poisson"])
    assert e.value.code == 2 and "--cloud-normals" in capsys.readouterr().err


def test_eval_driver_hands_the_options_to_both_fusion_paths(tmp_path):
    """eval_driver --poisson through its own argument parser: the options reach run_tanks as poisson_options, and without --poisson they
    are None, so that filter_depth / filter_depth_tanks are called with what they were called with before"""
    from unittest import mock
    scene = next(iter(fusion.TANKS_FILTER["intermediate"]))
    folder = tmp_path / "tanks" / "intermediate" / scene
    folder.mkdir(parents=True)
    (folder / "pair.txt").write_text("0\n")
    testlist = tmp_path / "list.txt"
    testlist.write_text("scan1\n")
    base = ["--dataset", "tanks", "--testpath", str(tmp_path / "tanks"), "--scenes", scene, "--outdir", str(tmp_path / "out"), "--filter", "--testlist", str(testlist),
            "--cloud-normals", "16"]
    for extra, want in ((["--poisson", "--poisson-resolution", "128", "--poisson-trim-relative", "0.05", "--poisson-cycles", "6"],
                         {"resolution": 128, "trim_relative": 0.05, "cycles": 6}), (["--poisson"], {"resolution": 256, "trim_relative": None, "cycles": 8}), ([], None)):
        with mock.patch.object(eval_driver, "run_tanks", lambda model, args, device, rank, world: args):
            args = eval_driver.main(base + extra)
        assert args.poisson_options == want and args.cloud_options == {"normals": 16}
        assert ("poisson" in eval_driver.cloud_keywords(args, {})) == (want is not None)


def test_the_math_header_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """csrc/poisson_math.h is plain C++: a stand-alone host program with its own main walks it under -fsanitize=address,undefined"""
    cxx = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    exe = str(tmp_path / "poisson_math_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-I", CSRC,
                    os.path.join(REPO, "tests", "poisson_math_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok ") and int(run.stdout.split()[1]) >= 30 and run.stderr == "", (run.stdout, run.stderr)
