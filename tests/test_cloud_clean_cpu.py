"""Host logic of the point-cloud clean-up (rc_mvsnet_amd/cloud_clean.py, fusion.py, dtu_io.py) without a GPU: the binding of
csrc/cloud_knn.h, the PLY with normals and its readers, the drivers' options, the oracle's own known answers, and csrc/cloud_knn_math.h
under the address and undefined-behaviour sanitizers as a stand-alone program."""
import argparse
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import cloud_clean_cases as C
import cloud_clean_oracle as O
from rc_mvsnet_amd import _lib, cloud_clean as CC, dtu_io, eval_driver, fusion, tsdf_mesh

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "rc_mvsnet_amd", "csrc")


def test_the_header_is_bound_and_its_entry_points_are_exported():
    assert os.path.join(CSRC, "cloud_knn.h") in _lib.EXT_HEADERS and _lib.REQUIRED_VERSION == 106
    names = [n for n in _lib.EXT_SIGNATURES if n.startswith("rcmvs_ck_")]
    assert sorted(names) == sorted(f"rcmvs_ck_{f}{t}" for f in ("finite", "knn", "radius", "stat", "normals", "compact") for t in ("", "_timed"))
    for n in names:
        if not n.endswith("_timed"):                             # a twin is its entry point plus (phase, ev0, ev1) before the stream
            assert _lib.EXT_SIGNATURES[n + "_timed"] == _lib.EXT_SIGNATURES[n][:-1] + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert (CC.MAX_K, CC.MAX_NK, CC.MAX_SWEEPS, CC.COUNTERS) == (32, 2 ** 31 - 256, O.MAX_SWEEPS, 8) and CC.COUNTER_NAMES == O.COUNTER_NAMES
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, n) for n in names)


def test_refused_before_any_launch():
    """the C entry points check their arguments on the host: no GPU is needed to be refused"""
    lib = _lib.load()
    assert lib.rcmvs_ck_knn(10, 0, None, None, None, None, None, None, None, None, None, None) < 0 and b"k = 0" in lib.rcmvs_last_error_string()
    assert lib.rcmvs_ck_knn(70000000, 32, None, None, None, None, None, None, None, None, None, None) < 0 and b"n k = 2240000000" in lib.rcmvs_last_error_string()
    assert lib.rcmvs_ck_knn(10, 8, None, None, None, None, None, None, None, None, None, None) < 0 and b"null pointer" in lib.rcmvs_last_error_string()
    assert lib.rcmvs_ck_radius(10, -1.0, 1, None, None, None, None, None, None, None, None) < 0 and b"r2 = -1" in lib.rcmvs_last_error_string()
    assert lib.rcmvs_ck_stat(None, 10, -1.0, None, None, None, None, None, None, None, None) < 0 and b"ratio = -1" in lib.rcmvs_last_error_string()
    assert lib.rcmvs_ck_normals(None, 10, 33, None, None, None, 0, None, None, None) < 0 and b"k = 33" in lib.rcmvs_last_error_string()
    assert lib.rcmvs_ck_compact(None, None, None, None, -1, None, None, None, None, None, None, None, None) < 0 and b"n = -1" in lib.rcmvs_last_error_string()
    assert lib.rcmvs_ck_finite(None, 1 << 31, None, None, None) < 0 and b"n = 2147483648" in lib.rcmvs_last_error_string()


def _legacy_ply_bytes(xyz, rgb):
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % len(xyz)).encode("ascii")
    body = b"".join(np.asarray(p, "<f4").tobytes() + np.asarray(c, "u1").tobytes() for p, c in zip(xyz, rgb))
    return head + body


def test_ply_bytes_without_normals_is_what_it_was_and_with_normals_round_trips(tmp_path):
    rng = np.random.default_rng(0)
    xyz = rng.normal(size=(37, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (37, 3)).astype(np.uint8)
    nrm = rng.normal(size=(37, 3)).astype(np.float32)
    nrm[0] = [-0.0, 0.0, 1e-45]                                   # the bits survive: a negative zero and a denormal
    nrm[1] = 0.0
    assert fusion.ply_bytes(xyz, rgb) == fusion.ply_bytes(xyz, rgb, None) == _legacy_ply_bytes(xyz, rgb)
    assert fusion.ply_bytes(xyz[:0], rgb[:0]) == _legacy_ply_bytes(xyz[:0], rgb[:0])
    data = fusion.ply_bytes(xyz, rgb, nrm)
    assert b"property float z\nproperty float nx\nproperty float ny\nproperty float nz\nproperty uchar red\n" in data and len(data) == data.index(b"end_header\n") + 11 + 37 * 27
    path = str(tmp_path / "n.ply")
    with open(path, "wb") as f:
        f.write(data)
    rx, rrgb, rn = dtu_io.read_ply_cloud_normals(path)
    assert np.array_equal(C.bits(rx), C.bits(xyz)) and np.array_equal(rrgb, rgb) and np.array_equal(C.bits(rn), C.bits(nrm))
    assert np.array_equal(C.bits(dtu_io.read_ply_xyz(path)), C.bits(xyz))
    with open(path, "wb") as f:
        f.write(fusion.ply_bytes(xyz, rgb))
    rx, rrgb, rn = dtu_io.read_ply_cloud_normals(path)
    assert rn is None and np.array_equal(rrgb, rgb) and np.array_equal(C.bits(rx), C.bits(xyz))
    with pytest.raises(_lib.RcmvsError, match="normals"):
        fusion.ply_bytes(xyz, rgb, nrm[:5])


def test_driver_options():
    ap = argparse.ArgumentParser()
    fusion.add_fusion_arguments(ap)
    none = ap.parse_args([])
    assert fusion.cloud_options(none, "t") is None and fusion.fusion_options(none, "t") == {}
    a = ap.parse_args(["--cloud-radius", "2.5", "4", "--cloud-stat", "20", "2.0", "--cloud-normals", "16"])
    assert fusion.cloud_options(a, "t") == {"radius": (2.5, 4), "stat": (20, 2.0), "normals": 16} and fusion.fusion_options(a, "t") == {}
    assert fusion.cloud_options(ap.parse_args(["--cloud-normals", "8"]), "t") == {"normals": 8}
    for argv, text in ((["--cloud-radius", "x", "4"], "takes a number"), (["--cloud-radius", "-1", "4"], "R >= 0"), (["--cloud-stat", "0", "2"], "1 <= K"),
                       (["--cloud-stat", "33", "2"], "1 <= K"), (["--cloud-stat", "8", "-1"], "RATIO >= 0"), (["--cloud-normals", "40"], "1 <= K")):
        with pytest.raises(SystemExit, match=text):
            fusion.cloud_options(ap.parse_args(argv), "t")
    help_text = " ".join(ap.format_help().split())
    assert help_text.count("a mesh is fused from the depth maps, not from the cloud") == 3
    assert CC.clean_options() is None and CC.clean_options(stat=(8, 1)) == {"stat": (8, 1.0)}
    for fn in (fusion.filter_depth, fusion.filter_depth_tanks):
        assert inspect.signature(fn).parameters["clean"].default is None
    ns = argparse.Namespace(cloud_options={"normals": 8}, fusion_options={})
    stats = {}
    assert eval_driver.cloud_keywords(ns, stats) == {"clean": {"normals": 8}, "stats": stats}
    assert eval_driver.cloud_keywords(argparse.Namespace(cloud_options={"normals": 8}, fusion_options={"method": "dynamic"}), stats) == {"clean": {"normals": 8}}
    assert eval_driver.cloud_keywords(argparse.Namespace(cloud_options=None, fusion_options={}), stats) == {}
    assert eval_driver.cloud_summary({}) == {} and eval_driver.cloud_summary({"cloud": {"out": 3}}) == {"cloud": {"out": 3}}
    assert "--cloud-radius" in inspect.getsource(fusion.add_fusion_arguments) and "cloud_radius" not in inspect.getsource(tsdf_mesh.main)


def test_eval_driver_refuses_cloud_options_without_filter(tmp_path):
    with pytest.raises(SystemExit, match="give --filter"):
        eval_driver.main(["--outdir", str(tmp_path), "--cloud-normals", "8"])


def test_eval_driver_hands_the_options_to_both_fusion_paths(tmp_path, capsys):
    """eval_driver --cloud-* through its own argument parser: run_scans and run_tanks call filter_depth / filter_depth_tanks with
    clean = the options and print the summary line with "cloud"; without the options neither the keyword nor the line is there"""
    import json
    from unittest import mock

    import torch

    from rc_mvsnet_amd import mvs_dataset
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

    want = {"radius": (2.0, 4), "stat": (20, 2.0), "normals": 16}
    for extra, clean in ((["--cloud-radius", "2", "4", "--cloud-stat", "20", "2", "--cloud-normals", "16"], want), ([], None)):
        argv = ["--dataset", "tanks", "--testpath", str(tmp_path / "tanks"), "--scenes", scene, "--outdir", str(tmp_path / "out"), "--filter",
                "--testlist", str(testlist)] + extra
        with mock.patch.object(eval_driver, "run_tanks", lambda model, args, device, rank, world: args):
            args = eval_driver.main(argv)
        assert args.cloud_options == clean
        seen = {}

        def record(which):
            def call(*a, **kw):
                seen[which] = kw
                if "clean" in kw:
                    kw["stats"]["cloud"] = {"in": 9, "out": 7}
            return call

        with mock.patch.object(mvs_dataset, "MVSDataset", NoViews), mock.patch.object(mvs_dataset, "TanksDataset", NoViews), \
                mock.patch.object(mvs_dataset, "prefetch", lambda ds, **k: iter(())), mock.patch.object(fusion, "filter_depth", record("dtu")), \
                mock.patch.object(fusion, "filter_depth_tanks", record("tanks")):
            capsys.readouterr()
            eval_driver.run_tanks(None, args, torch.device("cpu"), 0, 1)
            eval_driver.run_scans(None, args, torch.device("cpu"), 0, 1)
        lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{") and '"cloud"' in ln]
        if clean is None:
            assert "clean" not in seen["dtu"] and "clean" not in seen["tanks"] and "stats" not in seen["dtu"] and not lines
        else:
            assert seen["dtu"]["clean"] == clean and seen["tanks"]["clean"] == clean
            assert {"scan": "scan1", "cloud": {"in": 9, "out": 7}} in lines and {"scene": scene, "cloud": {"in": 9, "out": 7}} in lines


def test_camera_centre_is_minus_rt_t_in_fp64():
    E = np.array([[0, -1, 0, 3], [1, 0, 0, -2], [0, 0, 1, 0.5], [0, 0, 0, 1]], np.float32)
    c = fusion.camera_centre(E)
    assert c.dtype == np.float64 and np.array_equal(c, [2.0, 3.0, -0.5])


def test_the_oracle_knows_its_answers():
    """the oracle alone: the order by (d2, index), the moments' tree against math.fsum, the loop of equal means, the planar grid"""
    import math
    idx, d2, mean = O.knn(C.cloud("lattice"), 7)
    assert (d2[0] == [1, 1, 1, 2, 2, 2, 3]).all() and idx[0].tolist() == [1, 9, 81, 10, 82, 90, 91] and mean[0] == (3 + 3 * math.sqrt(2.0) + math.sqrt(3.0)) / 7
    idx, d2, mean = O.knn(C.cloud("dup40"), 8)
    assert idx[5].tolist() == [0, 1, 2, 3, 4, 6, 7, 8] and not d2.any() and not mean.any()
    idx, d2, mean = O.knn(C.cloud("n2"), 8)
    assert idx.tolist() == [[1] + [-1] * 7, [0] + [-1] * 7] and np.isinf(d2[:, 1:]).all() and np.isnan(mean).all()
    x = np.random.default_rng(1).random(70001)
    n, mu, var = O.moments(x)
    assert abs(mu - math.fsum(x) / n) < 1e-14 and abs(var - np.var(x, ddof=1)) < 1e-14 and O.moments(x[:1])[2] == 0.0 and np.isnan(O.moments(x[:0])[1])
    for name, k, ratio in C.STAT_CASES:
        if name in ("plane_far", "loop"):
            keep, _ = O.statistical(C.reference_knn(name, k)[2], ratio)
            assert keep.sum() == {"plane_far": 400, "loop": 40}[name]


def test_the_math_header_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """csrc/cloud_knn_math.h is plain C++: a stand-alone host program with its own main walks it under -fsanitize=address,undefined"""
    cxx = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    exe = str(tmp_path / "cloud_knn_math_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-I", CSRC,
                    os.path.join(REPO, "tests", "cloud_knn_math_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok ") and int(run.stdout.split()[1]) >= 18 and run.stderr == "", (run.stdout, run.stderr)
