"""Dynamic depth-map fusion without a GPU and without the emulation: the drivers' options and refusals, the summaries' keys, the bases that
restate the fixed thresholds, the oracle's own known answers, and csrc/fusion_dyn_math.h under the address and undefined-behaviour
sanitizers in a stand-alone program."""
import argparse
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import fusion_dyn_cases as DC
from conftest import REPO
from rc_mvsnet_amd import _lib, eval_driver, fusion, tsdf_mesh

CSRC = os.path.join(REPO, "rc_mvsnet_amd", "csrc")


def _parse(argv, dedup=True):
    ap = argparse.ArgumentParser()
    fusion.add_fusion_arguments(ap, dedup=dedup)
    return ap.parse_args(argv)


def test_fusion_options_are_empty_without_an_option_and_complete_with_one():
    assert fusion.fusion_options(_parse([]), "x") == {}
    assert fusion.fusion_options(_parse([], dedup=False), "x") == {}
    assert fusion.fusion_options(_parse(["--fusion", "reference"]), "x") == {"method": "reference", "dynamic": None, "dedup": False}
    assert fusion.fusion_options(_parse(["--fusion-dedup"]), "x") == {"method": "reference", "dynamic": None, "dedup": True}
    assert fusion.fusion_options(_parse(["--fusion", "dynamic"]), "x") == {"method": "dynamic", "dynamic": {}, "dedup": False}
    got = fusion.fusion_options(_parse(["--fusion", "dynamic", "--fusion-dedup", "--dyn-levels", "2", "5", "--dyn-dist-base", "0.5", "--dyn-rel-base", "0.002"]), "x")
    assert got == {"method": "dynamic", "dynamic": {"dist_base": 0.5, "rel_base": 0.002, "level_lo": 2, "level_hi": 5}, "dedup": True}
    for argv, pattern in ((["--dyn-dist-base", "0.5"], "belong to --fusion dynamic"), (["--fusion", "reference", "--dyn-levels", "2", "3"], "belong to --fusion dynamic"),
                          (["--fusion", "dynamic", "--dyn-levels", "3", "2"], "1 <= LO <= HI <= 16"), (["--fusion", "dynamic", "--dyn-levels", "0", "2"], "1 <= LO"),
                          (["--fusion", "dynamic", "--dyn-levels", "2", "17"], "HI <= 16")):
        with pytest.raises(SystemExit, match=pattern):
            fusion.fusion_options(_parse(argv), "x")
    with pytest.raises(SystemExit):
        _parse(["--fusion", "fast"])
    assert fusion.dynamic_params(None, 4) == {"level_lo": 2, "level_hi": 4, "dist_base": 0.25, "rel_base": 1.0 / 1300.0}
    assert fusion.dynamic_params({"level_lo": 3}, 1)["level_hi"] == 3 and fusion.dynamic_params(None, 1)["level_hi"] == 2
    with pytest.raises(_lib.RcmvsError, match="unknown parameter"):
        fusion.dynamic_params({"levels": (2, 3)}, 4)


def test_eval_driver_refuses_before_it_builds_anything(tmp_path):
    out = ["--outdir", str(tmp_path)]
    with pytest.raises(SystemExit, match="does not go with --mesh.*EVERY observation"):
        eval_driver.main(out + ["--testpath", str(tmp_path), "--filter", "--mesh", "--fusion-dedup"])
    with pytest.raises(SystemExit, match="give --filter"):
        eval_driver.main(out + ["--fusion", "dynamic"])
    with pytest.raises(SystemExit, match="belong to --fusion dynamic"):
        eval_driver.main(out + ["--filter", "--dyn-rel-base", "0.001"])
    with pytest.raises(SystemExit, match="1 <= LO <= HI"):
        eval_driver.main(out + ["--filter", "--fusion", "dynamic", "--dyn-levels", "4", "3"])
    ns = argparse.Namespace(fusion_options={"method": "dynamic", "dynamic": {"level_lo": 2}, "dedup": True})
    assert eval_driver.mesh_fusion_options(ns) == {"method": "dynamic", "dynamic": {"level_lo": 2}}          # the method, never the dedup
    assert eval_driver.mesh_fusion_options(argparse.Namespace(fusion_options={})) == {}
    src = inspect.getsource(eval_driver)
    assert src.count("**(dict(args.fusion_options, stats=fstats) if args.fusion_options else {})") == 2 and src.count("**mesh_fusion_options(args)") == 2


def test_tsdf_mesh_takes_the_method_and_refuses_the_dedup(tmp_path, monkeypatch):
    base = ["--pair-folder", "p", "--scan-folder", "s", "--out-folder", "o", "--mesh", str(tmp_path / "m.ply")]
    with pytest.raises(SystemExit, match="EVERY observation"):
        tsdf_mesh.main(base + ["--fusion-dedup"])
    with pytest.raises(SystemExit, match="belong to --fusion dynamic"):
        tsdf_mesh.main(base + ["--dyn-levels", "2", "3"])
    seen, real_mesh_scan = [], tsdf_mesh.mesh_scan
    monkeypatch.setattr(tsdf_mesh, "mesh_scan", lambda *a, **kw: seen.append(kw) or {"mesh": "m"})
    tsdf_mesh.main(base)
    tsdf_mesh.main(base + ["--fusion", "dynamic", "--dyn-levels", "2", "4"])
    assert "method" not in seen[0] and "dynamic" not in seen[0]
    assert seen[1]["method"] == "dynamic" and seen[1]["dynamic"] == {"level_lo": 2, "level_hi": 4}
    for fn in (real_mesh_scan, tsdf_mesh.mesh_scan_tanks):
        p = inspect.signature(fn).parameters
        assert p["method"].default is None and p["dynamic"].default is None and "dedup" not in p
    for fn in (tsdf_mesh.filtered_views, tsdf_mesh.filtered_views_tanks):
        p = inspect.signature(fn).parameters
        assert p["method"].default == "reference" and p["dynamic"].default is None and "dedup" not in p
    for fn in (fusion.filter_depth, fusion.filter_depth_tanks):
        p = inspect.signature(fn).parameters
        assert (p["method"].default, p["dynamic"].default, p["dedup"].default, p["stats"].default) == ("reference", None, False, None)


def test_mesh_summary_gains_fusion_only_with_an_option(monkeypatch):
    import torch
    calls = []

    def views(*a, **kw):
        calls.append(kw)
        if kw.get("stats") is not None:
            kw["stats"]["kept"] = 123
        return {"depth": torch.zeros(2, 4, 4), "lo": np.zeros(3), "hi": np.ones(3)}

    monkeypatch.setattr(tsdf_mesh, "filtered_views", views)
    monkeypatch.setattr(tsdf_mesh, "_mesh_views", lambda *a, **kw: {"mesh": "m", "faces": 0})
    plain = tsdf_mesh.mesh_scan("p", "s", "o", "m.ply", 0.8, 3, 0.5, 0.01)
    assert plain == {"mesh": "m", "faces": 0} and calls[0] == {}
    got = tsdf_mesh.mesh_scan("p", "s", "o", "m.ply", 0.8, 3, 0.5, 0.01, method="dynamic", dynamic={"level_hi": 4})
    assert set(got) == {"mesh", "faces", "fusion"} and calls[1]["method"] == "dynamic"
    assert got["fusion"] == {"method": "dynamic", "levels": [2, 4], "dist_base": 0.25, "rel_base": 1.0 / 1300.0, "dedup": False, "points": 123, "claimed": 0}
    got = tsdf_mesh.mesh_scan("p", "s", "o", "m.ply", 0.8, 3, 0.5, 0.01, method="reference")
    assert got["fusion"]["method"] == "reference" and got["fusion"]["levels"] == [3, 3] and got["fusion"]["dedup"] is False
    s = fusion.fusion_summary({"method": "reference", "dynamic": None, "dedup": True}, {"kept": 5, "claimed": 2}, (3, 0.5, 0.01))
    assert sorted(s) == ["claimed", "dedup", "dist_base", "levels", "method", "points", "rel_base"] and (s["points"], s["claimed"], s["dedup"]) == (5, 2, True)
    assert (s["dist_base"], s["rel_base"]) == fusion.reference_bases(3, 0.5, 0.01)


def test_reference_bases_restate_the_fixed_thresholds_in_every_bit():
    """k * base == threshold exactly, in the kernel's types, for the DTU defaults and every Tanks-and-Temples scene; where no base does, a refusal"""
    settings = [(3, 0.5, 0.01), (2, 0.25, 0.3), (1, 0.5, 0.01), (16, 1.0, 0.01)]
    settings += [(f["geo_mask_thres"], f["geo_pixel_thres"], f["geo_depth_thres"]) for split in fusion.TANKS_FILTER.values() for f in split.values()]
    for k, dist_t, depth_t in settings:
        db, rb = fusion.reference_bases(k, dist_t, depth_t)
        assert np.float64(k) * np.float64(db) == np.float64(dist_t) and np.float32(k) * np.float32(rb) == np.float32(depth_t), (k, dist_t, depth_t)
        assert np.float32(rb) == rb                                      # a float32 value: the entry point's cast changes nothing
    for k in (0, 17, -1):
        with pytest.raises(_lib.RcmvsError, match="levels 1..16"):
            fusion.reference_bases(k, 0.5, 0.01)
    with pytest.raises(_lib.RcmvsError, match="no float64 base"):
        fusion.reference_bases(3, 5e-324, 0.01)                          # the smallest denormal is no multiple of 3


def test_the_entry_point_is_declared_next_to_its_kernel():
    assert any(p.endswith("fusion_dyn.h") for p in _lib.EXT_HEADERS) and _lib.CONSTANTS["RCMVS_VERSION"] == 106
    p, i, f, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double
    assert _lib.EXT_SIGNATURES["rcmvs_fuse_view_dyn"] == [p, i, i, p, p, p, p, f, i, i, d, f, p, p, p, p, p, p, p, p, p, i, i, i, p]
    assert "rcmvs_fuse_view_dyn" not in _lib.SIGNATURES


def test_oracle_known_answer_and_case_asserts_need_no_kernel():
    """what every case is named for holds on the oracle alone; the plane seen by four cameras gives 816 points, and 216 with suppression"""
    for name in DC.CASES:
        DC.reference(name)
    s = DC.known_scan()
    totals = {}
    for dedup in (False, True):
        xyz, _ = DC.compacted(DC.scan_oracle(s, None, s["K"], 0.8, dedup=dedup))
        totals[dedup] = len(xyz)
        assert (xyz[:, 2] == np.float32(4.0)).all()
    assert totals == {False: 816, True: 216}


def test_refusals_of_the_built_library_need_no_gpu():
    """the entry point rejects bad arguments on the host, before any launch"""
    _lib.build()
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    err = lib.rcmvs_last_error_string
    idx = (ctypes.c_int * 17)(*([1] * 17))
    ip = ctypes.cast(idx, ctypes.c_void_p)

    def call(n_views=5, ref=0, idx=ip, lo=2, hi=4, N=4, H=8, W=8, masks=one, level=one, img=None, rgb=None):
        return lib.rcmvs_fuse_view_dyn(one, n_views, ref, idx, one, img, one, 0.8, lo, hi, 0.25, 0.001, None, masks, level, one, one, rgb, None, None, None, N, H, W, None)

    assert call(N=17) < 0 and b"17 source views" in err()
    assert call(N=0) < 0 and b"0 source views" in err()
    assert call(lo=0) < 0 and b"levels 0..4" in err()
    assert call(lo=5, hi=4) < 0 and b"levels 5..4" in err()
    assert call(hi=17) < 0 and b"levels 2..17" in err()
    assert call(masks=None) < 0 and b"null pointer" in err()
    assert call(level=None) < 0 and b"null pointer" in err()
    assert call(idx=None) < 0 and b"null pointer" in err()
    assert call(img=one) < 0 and b"together" in err()
    assert call(ref=5) < 0 and b"reference view index 5" in err()
    assert call(ref=-1) < 0 and b"reference view index -1" in err()
    assert call(n_views=1) < 0 and b"source view index 1 outside the 1 views" in err()
    assert call(H=0) < 0 and b"bad dims" in err()
    assert call(H=32768, W=32768) < 0 and b"bad dims" in err()


def test_the_math_header_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """csrc/fusion_dyn_math.h is plain C++: a stand-alone host program with its own main walks it over hostile numbers under
    -fsanitize=address,undefined"""
    cxx = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    exe = str(tmp_path / "fusion_dyn_math_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-I", CSRC,
                    os.path.join(REPO, "tests", "fusion_dyn_math_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok ") and int(run.stdout.split()[1]) >= 1000 and run.stderr == "", (run.stdout, run.stderr)
