"""Mesh simplification without a GPU: properties of tests/mesh_simplify_oracle.py (the restatement of csrc/mesh_simplify_math.h) that
hold by construction, the host logic of rc_mvsnet_amd/mesh_simplify.py, the wiring of the option into the mesh path's command lines,
and the math header itself under AddressSanitizer and UndefinedBehaviorSanitizer in a stand-alone host program."""
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import mesh_simplify_cases as MSC
import mesh_simplify_oracle as O
from rc_mvsnet_amd import _lib, eval_driver, mesh_simplify as MS, tsdf_mesh as TM

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "rc_mvsnet_amd", "csrc")
SMALL = [key for key in MSC.case_keys() if not key[0].startswith(("sheet_2", "sheet_4", "strip_2", "strip_4", "specks", "plane_17", "cube_9", "fan_600"))]


def test_the_oracle_states_the_headers_constants():
    text = open(os.path.join(CSRC, "mesh_simplify_math.h")).read()
    assert float(re.search(r"DET_EPS = ([0-9.e+-]+);", text).group(1)) == O.DET_EPS and float(re.search(r"FAR = ([0-9.e+-]+);", text).group(1)) == O.FAR
    for name in ("PATH_LOCKED", "PATH_QUADRIC", "PATH_MIDPOINT", "PATH_END_U", "PATH_END_V", "EDGE_OK", "EDGE_COST", "EDGE_LINK", "EDGE_FLIP", "EDGE_NONE"):
        assert getattr(O, name) == getattr(MS, name) == _lib.CONSTANTS["RCMVS_MS_" + name], name
        assert re.search(r"\b%s = %d\b" % (name, getattr(O, name)), text), name
    assert O.NO_KEY == MS.NO_KEY and tuple(O.PATH_NAMES) == tuple(MS.PATH_NAMES) and _lib.REQUIRED_VERSION == 106
    assert {"rcmvs_ms_init", "rcmvs_ms_init_timed", "rcmvs_ms_round", "rcmvs_ms_round_timed", "rcmvs_ms_finish", "rcmvs_ms_finish_timed"} <= set(_lib.EXT_SIGNATURES)


@pytest.mark.parametrize("name,k", SMALL)
def test_every_round_of_the_oracle_is_independent_and_keeps_closed_surfaces_closed(name, k):
    """no two applied edges within each other's closed rings; live faces fall by twice the applied edges; closed manifolds keep
    0 boundary edges, 0 non-manifold edges, their Euler characteristic and their orientation after every round"""
    v, f, _ = MSC.case(name)
    wv, wf, wc, stats, run = MSC.reference(name, k)
    MSC.check_rounds(name, f, len(v), run["rounds"], (name, k))
    assert stats["rounds"] == len(stats["collapses"]) == len(run["rounds"]) and stats["stop"] in MS.STOPS
    assert stats["faces_out"] == stats["valid_faces_in"] - 2 * sum(stats["collapses"]) and stats["faces_out"] == len(wf)
    if stats["stop"] == "target":
        assert stats["faces_out"] <= stats["target_faces"] or stats["rounds"] == 0
        assert stats["rounds"] == 0 or stats["faces_out"] >= stats["target_faces"] - 1      # the budget never overshoots by more than the odd face
    assert len(wv) == len(wc) and (wf.size == 0 or (0 <= wf.min() and wf.max() < len(wv)))


def test_a_tetrahedron_comes_back_as_it_went_in():
    v, f, rgb = MSC.case("tetrahedron")
    wv, wf, wc, stats, _ = MSC.reference("tetrahedron", 0)
    assert MSC.same_bits(wv, v) and np.array_equal(wf, f) and np.array_equal(wc, rgb) and stats["rejected_link"] == 6 and stats["collapses"] == [0]


def test_numbering_changes_the_choice_not_the_surface():
    """the same sheet numbered along its rows and shuffled: both runs keep the rim, in every bit, and reach the same face count"""
    a, b = MSC.reference("sheet_257", 0), MSC.reference("sheet_257_ascending", 0)
    va, vb = MSC.case("sheet_257")[0], MSC.case("sheet_257_ascending")[0]
    assert {r.tobytes() for r in va} == {r.tobytes() for r in vb}
    assert a[3]["locked_vertices"] == b[3]["locked_vertices"] == 2 * 8 + 2 * 32 - 4
    first = b[4]["rounds"][0][0]
    rim = {va_.tobytes() for va_ in vb[first["locked"] == 1]}
    assert rim <= {r.tobytes() for r in a[0]} and rim <= {r.tobytes() for r in b[0]}


def test_plane_and_cube_known_answers_hold_in_the_oracle():
    """the small plane and cube, exact arithmetic: z = +0.0, twice the area 2; on the cube, six times the volume 6, corners kept"""
    wv, wf, _, stats, _ = MSC.reference("plane_9", 0)
    assert (wv[:, 2].view(np.uint32) == 0).all() and stats["max_cost"] == 0.0 and len(wv) < 81
    P = MSC.frac(wv)
    assert sum((P[b][0] - P[a][0]) * (P[c][1] - P[a][1]) - (P[b][1] - P[a][1]) * (P[c][0] - P[a][0]) for a, b, c in wf.tolist()) == 2
    wv, wf, _, stats, _ = MSC.reference("cube_5", 0)
    assert MSC.on_cube(wv).all() and MSC.cube_corner_miss(wv) == 0.0 and MSC.edge_stats(wf, len(wv)) == (0, 0, 2, True) and len(wf) < 192
    P = MSC.frac(wv)
    det = lambda a, b, c: (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]))      # noqa: E731
    assert sum(det(P[a], P[b], P[c]) for a, b, c in wf.tolist()) == Fraction(6)


def test_host_logic():
    assert MS.frame(None, None) == [0.0, 0.0, 0.0, 1.0] == O.frame(None, None)
    lo, hi = np.array([-0.0, 1.0, -2.0], np.float32), np.array([0.0, 1.0, 6.0], np.float32)
    assert MS.frame(lo, hi) == O.frame(lo, hi) == [0.0, 1.0, 2.0, 8.0] and MS.frame(lo, lo)[3] == 1.0
    for x in (0.0, 1e-30, 1.0, 3.5e37, math.inf):
        assert MS.unordered_cost(O.ordered32(np.float32(x))) == float(np.float32(x)) == O.unordered_cost(O.ordered32(np.float32(x)))
    assert MS.unordered_cost(0) == 0.0
    assert MS._target(10, None, "t") == ("faces", 10) and MS._target(None, 0.25, "t") == ("ratio", 0.25)
    for bad in ((None, None), (1, 0.5), (-1, None), (None, 1.5), (None, float("nan")), (True, None)):
        with pytest.raises(_lib.RcmvsError):
            MS._target(*bad, "t")
    assert MS._max_error(math.inf, "t") == math.inf and MS._max_error(0, "t") == 0.0
    for bad in (-1e-9, float("nan"), "x", None):
        with pytest.raises(_lib.RcmvsError, match="max_error"):
            MS._max_error(bad, "t")
    assert O.budget(10, 4) == 3 and O.budget(11, 4) == 4 and O.budget(4, 4) == 0 and O.budget(3, 4) == 0


def test_the_option_is_off_by_default_on_every_command_line():
    assert MS.simplify_options() is None and TM._simplify_argument(0, 0.0, None) == {} and TM._simplify_argument(0, 0.25, None) == {"simplify": {"ratio": 0.25}}
    assert TM._simplify_argument(500, 0.0, 1e-6) == {"simplify": {"target_faces": 500, "max_error": 1e-6}}
    with pytest.raises(_lib.RcmvsError, match="needs a target"):
        TM._simplify_argument(0, 0.0, 1e-6)
    import inspect
    for fn in (TM.mesh_scan, TM.mesh_scan_tanks):
        p = inspect.signature(fn).parameters
        assert p["simplify_faces"].default == 0 and p["simplify_ratio"].default == 0.0 and p["simplify_max_error"].default is None
    assert inspect.signature(TM._mesh_views).parameters["simplify"].default is None
    src = inspect.getsource(eval_driver)
    assert '"--mesh-simplify-ratio", type=float, default=0.0' in src and src.count('if args.mesh_simplify_ratio else {}') == 2


def test_the_math_header_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """csrc/mesh_simplify_math.h is plain C++: a stand-alone host program with its own main walks it under -fsanitize=address,undefined"""
    cxx = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    exe = str(tmp_path / "mesh_simplify_math_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-I", CSRC,
                    os.path.join(REPO, "tests", "mesh_simplify_math_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok ") and int(run.stdout.split()[1]) >= 25 and run.stderr == "", (run.stdout, run.stderr)
