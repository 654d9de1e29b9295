"""The Tanks and Temples F-score on the GPU (rc_mvsnet_amd/tanks_fscore.py, csrc/pc_register.hip) against the fp64 oracle
(tests/tanks_fscore_oracle.py): crop flags, voxel outputs and ICP correspondences bit for bit, moments within 1e-12 relative,
histograms and counts exactly, the ICP loop's iteration counts and its final matrix within 1e-9."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tanks_fscore_oracle as O
from rc_mvsnet_amd import _lib, synthetic, tanks_fscore as F

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def sim(deg, scale, shift, axis=(0.3, 0.5, -0.8)):
    return synthetic._similarity(axis, deg, scale, shift)


# ---- crop -------------------------------------------------------------------------------------------------------------
L_POLY = np.array([[0.1, 0.1], [0.9, 0.1], [0.9, 0.5], [0.5, 0.5], [0.5, 0.9], [0.1, 0.9]])
TRIANGLE = np.array([[0.05, 0.1], [0.95, 0.2], [0.3, 0.9]])
STAR = np.stack([0.5 + np.where(np.arange(F.MAX_POLYGON) % 2, 0.2, 0.45) * np.cos(2 * np.pi * np.arange(F.MAX_POLYGON) / F.MAX_POLYGON),
                 0.5 + np.where(np.arange(F.MAX_POLYGON) % 2, 0.2, 0.45) * np.sin(2 * np.pi * np.arange(F.MAX_POLYGON) / F.MAX_POLYGON)], 1)
LO, HI = float(np.float32(0.2)), float(np.float32(0.8))


def crop_points(n, seed=0):
    """random points in the unit cube with, where n allows, points exactly at axis_min / axis_max, points whose coordinate
    equals a vertex's (0.1, 0.5, 0.9) and points on the L's vertical edges"""
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)).astype(np.float32)
    k = min(n // 8, 60)
    for j, (col, val) in enumerate(((2, LO), (2, HI), (0, LO), (1, HI), (1, 0.5), (0, 0.5), (2, 0.5), (1, 0.1), (0, 0.9), (2, 0.9))):
        p[j * k // 2:(j + 1) * k // 2, col] = np.float32(val)
    return p


def check_crop(pts, axis, lo, hi, poly, T=None, some=True):
    vol = F.make_volume(axis, lo, hi, poly)
    flags, kept = F.crop(dev(pts), vol, T)
    want, q = O.crop(pts, axis, lo, hi, poly, T)
    assert flags.dtype == torch.bool and np.array_equal(flags.cpu().numpy(), want)
    assert np.array_equal(bits(kept.cpu().numpy()), bits(q[want]))
    if some:
        assert 0 < want.sum() < len(pts)
    return want


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("poly", [L_POLY, TRIANGLE, STAR], ids=["L", "triangle", "bound"])
def test_crop_axes_and_polygons(axis, poly):
    pts = crop_points(20011, seed=axis)
    want = check_crop(pts, axis, LO, HI, poly)
    edge = (pts[:, axis] == np.float32(LO)) | (pts[:, axis] == np.float32(HI))
    assert edge.sum() >= 30 and want[edge].any()                 # both ends of the axis range are inclusive


@pytest.mark.parametrize("n", [1, 257, 20011])
def test_crop_sizes_and_transform(n):
    pts = crop_points(n, seed=5) if n > 1 else np.array([[0.3, 0.3, 0.5]], dtype=np.float32)
    check_crop(pts, 2, LO, HI, L_POLY, some=n > 1)
    T = sim(25.0, 1.3, (0.35, -0.1, 0.05))
    check_crop(pts, 1, LO, HI, L_POLY, T, some=n > 1)
    check_crop(pts, 0, 0.1, 1.2, TRIANGLE, sim(-10.0, 1.3, (0.0, 0.1, 0.2)), some=n > 1)


def test_crop_keeps_nothing_and_refusals():
    pts = crop_points(1000)
    want = check_crop(pts, 2, 2.0, 3.0, L_POLY, some=False)
    assert want.sum() == 0
    flags, kept = F.crop(dev(pts), F.make_volume(0, LO, HI, L_POLY + 5.0))
    assert not flags.any() and kept.shape == (0, 3)
    flags, kept = F.crop(torch.zeros((0, 3), device=DEV), F.make_volume(0, LO, HI, L_POLY))
    assert flags.shape == (0,) and kept.shape == (0, 3)
    with pytest.raises(_lib.RcmvsError):
        F.make_volume(2, LO, HI, np.zeros((F.MAX_POLYGON + 1, 2)))
    with pytest.raises(_lib.RcmvsError):
        F.crop(dev(pts), {"axis": 2, "axis_min": LO, "axis_max": HI, "polygon": L_POLY[:2]})
    with pytest.raises(_lib.RcmvsError):
        F.crop(dev(pts), F.make_volume(2, LO, HI, L_POLY), np.full((4, 4), np.nan))


# ---- voxel down-sample ------------------------------------------------------------------------------------------------
def check_voxel(pts, voxel):
    got = F.voxel_down_sample(dev(pts), voxel).cpu().numpy()
    want = O.voxel_down_sample(pts, voxel)
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
    return got


def test_voxel_one_point_and_one_voxel():
    assert len(check_voxel(np.array([[1.5, -2.0, 3.0]], dtype=np.float32), 0.1)) == 1
    rng = np.random.default_rng(0)
    pts = (rng.random((700, 3)) * 0.4).astype(np.float32)
    pts[0] = 0.0                                                 # the minimum: every point lies in [min - v / 2, min + v / 2)
    assert len(check_voxel(pts, 1.0)) == 1


def test_voxel_faces_and_negative_coordinates():
    voxel = 0.25
    rng = np.random.default_rng(1)
    k = rng.integers(-20, 21, (3000, 3))
    pts = (k * (voxel / 2) - 1.125).astype(np.float32)           # multiples of voxel / 2 from the minimum: on faces and centres
    pts[0] = -20 * (voxel / 2) - 1.125
    out = check_voxel(pts, voxel)
    assert 500 < len(out) < 3000 and (pts < 0).any() and (pts > 0).any()


def test_voxel_long_segment_next_to_singletons():
    rng = np.random.default_rng(2)
    dense = rng.random((5000, 3)) * 0.0049                       # with the minimum (0, 0, 0) the voxel [-0.005, 0.005)^3 holds all of them
    g = np.arange(3000)
    single = np.stack([(g % 15 + 2) * 0.02, (g // 15 % 15 + 2) * 0.02, (g // 225 + 2) * 0.02], 1) + 0.001
    pts = np.concatenate([dense, single]).astype(np.float32)
    pts = np.concatenate([np.zeros((1, 3), np.float32), pts])[rng.permutation(8001)]
    out = check_voxel(pts, 0.01)
    assert len(out) == 3001


def test_voxel_lattice_beyond_2_32():
    rng = np.random.default_rng(3)
    pts = (rng.random((5000, 3)) * 40.0 - 20.0).astype(np.float32)
    pts[:2] = [[-20, -20, -20], [20, 20, 20]]
    voxel = 0.0015                                               # 26 667 voxels per axis: 1.9e13 voxels, a 45-bit key
    assert (40.0 / voxel) ** 3 > 2.0 ** 32
    check_voxel(pts, voxel)


def test_voxel_duplicates_random_and_reproducible():
    rng = np.random.default_rng(4)
    base = rng.random((500, 3)).astype(np.float32)
    check_voxel(np.concatenate([base, base, base[:100]]), 0.05)
    pts = (rng.random((60000, 3)) * np.cbrt(20000.0) * 0.1).astype(np.float32)      # 20 000 voxels of edge 0.1: about 3 points each
    a = check_voxel(pts, 0.1)
    assert 2.5 < len(pts) / len(a) < 3.6
    b = F.voxel_down_sample(dev(pts), 0.1).cpu().numpy()
    assert np.array_equal(bits(a), bits(b))


def test_voxel_refusals():
    pts = dev(np.random.default_rng(5).random((100, 3)).astype(np.float32))
    for voxel in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.RcmvsError, match="voxel"):
            F.voxel_down_sample(pts, voxel)
    bad = pts.clone()
    bad[3, 1] = float("nan")
    with pytest.raises(_lib.RcmvsError, match="finite"):
        F.voxel_down_sample(bad, 0.1)
    with pytest.raises(_lib.RcmvsError, match="2\\^21"):
        F.voxel_down_sample(pts, 1e-7)                           # extent 1 / 1e-7 = 1e7 voxels on an axis
    assert F.voxel_down_sample(torch.zeros((0, 3), device=DEV), 0.1).shape == (0, 3)


# ---- ICP step ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def icp_problem():
    """4 000 source points against 6 000 targets (100 of them exact duplicates of others), all coordinates in [1, 2.1] so that no
    sum cancels; max_dist is the 70 % quantile of the nearest distances"""
    rng = np.random.default_rng(6)
    tgt = (rng.random((5900, 3)) + 1.0).astype(np.float32)
    tgt = np.concatenate([tgt, tgt[:100]])
    src = (tgt[rng.integers(0, len(tgt), 4000)] + rng.normal(0, 0.02, (4000, 3))).astype(np.float32)
    T = sim(1.0, 1.002, (0.004, -0.003, 0.002))
    s = O.transform(src, T)
    two = np.sqrt(O.nearest_two(s, tgt))
    max_dist = float(np.quantile(two[:, 0], 0.7))
    want, corr = O.icp_step(src, tgt, T, max_dist)
    return {"src": src, "tgt": tgt, "T": T, "two": two, "max_dist": max_dist, "mom": want, "corr": corr}


def test_icp_step_against_oracle(icp_problem):
    p = icp_problem
    idx, _ = O.nearest(O.transform(p["src"], p["T"]), p["tgt"])
    dup = np.zeros(len(p["tgt"]), dtype=bool)
    dup[:100] = dup[5900:] = True
    gap = p["two"][:, 1] - p["two"][:, 0]
    assert np.all((gap > 1e-9) | (dup[idx] & (gap == 0.0)))      # the input has no near-tie but the exact duplicates
    assert (dup[idx] & (gap == 0.0)).sum() > 20
    assert np.all(np.abs(p["two"][:, 0] - p["max_dist"]) > 1e-9)
    assert 0.6 < p["mom"][0] / len(p["src"]) < 0.8
    target = F.IcpTarget(dev(p["tgt"]), p["max_dist"])
    mom, corr = F.icp_step(dev(p["src"]), target, p["T"], p["max_dist"], want_corr=True)
    assert np.array_equal(corr.cpu().numpy(), p["corr"])
    assert mom[0] == p["mom"][0]
    assert np.all(np.abs(mom[1:] - p["mom"][1:]) <= 1e-12 * np.abs(p["mom"][1:]))
    again, none = F.icp_step(dev(p["src"]), target, p["T"], p["max_dist"])
    assert none is None and np.array_equal(mom.view(np.uint64), again.view(np.uint64))


def test_icp_step_no_correspondence_and_single_target(icp_problem):
    p = icp_problem
    far = np.eye(4)
    far[:3, 3] = 50.0
    mom, corr = F.icp_step(dev(p["src"]), F.IcpTarget(dev(p["tgt"]), 0.05), far, 0.05, want_corr=True)
    assert np.array_equal(mom, np.zeros(18)) and bool((corr == -1).all())
    one = p["tgt"][:1]
    mom, corr = F.icp_step(dev(p["src"]), F.IcpTarget(dev(one), 0.3), np.eye(4), 0.3, want_corr=True)
    want, wcorr = O.icp_step(p["src"], one, np.eye(4), 0.3)
    assert 0 < want[0] < len(p["src"]) and np.array_equal(corr.cpu().numpy(), wcorr) and mom[0] == want[0]
    assert np.all(np.abs(mom[1:] - want[1:]) <= 1e-12 * np.abs(want[1:]))
    r = F.icp(dev(p["src"]), dev(p["tgt"]), 0.05, far)
    assert r["iterations"] == 0 and r["fitness"] == 0.0 and np.array_equal(r["transformation"], far)


# ---- ICP loop, register, evaluate -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    s = synthetic.tanks_fscore_scene(n_gt=5000, n_est=5000, tau=0.01, seed=7)
    v = s["volume"]
    s["vol"] = F.make_volume(v["axis"], v["axis_min"], v["axis_max"], v["polygon"])
    s["ovol"] = (s["vol"]["axis"], s["vol"]["axis_min"], s["vol"]["axis_max"], s["vol"]["polygon"])
    s["oracle_register"] = O.register(s["est"], s["gt"], s["init"], s["ovol"], s["tau"])
    return s


def test_register_against_oracle(scene):
    s = scene
    T, rounds = F.register(dev(s["est"]), dev(s["gt"]), s["init"], s["vol"], s["tau"])
    wT, wrounds = s["oracle_register"]
    assert len(rounds) == len(wrounds) == 3
    err0 = np.abs(s["init"] - s["T_true"]).max()
    for r, w in zip(rounds, wrounds):
        print("round: iterations", r["iterations"], w["iterations"], "fitness", r["fitness"], w["fitness"], "rmse", r["inlier_rmse"], w["inlier_rmse"],
              "max |dT|", np.abs(r["transformation"] - w["transformation"]).max())
        assert r["iterations"] == w["iterations"] and 0 < r["iterations"] <= 20
        assert np.abs(r["transformation"] - w["transformation"]).max() <= 1e-9
        assert np.abs(r["transformation"] - s["T_true"]).max() < err0          # closer to the truth than the initial one, every round
    assert np.abs(T - wT).max() <= 1e-9
    assert np.abs(T - s["T_true"]).max() < 0.1 * err0


def check_evaluate(est, gt, T, vol, ovol, tau, **kw):
    got = F.evaluate(dev(est), dev(gt), T, vol, tau, **kw)
    want = O.evaluate(est, gt, T, ovol, tau, **kw)
    for k in ("precision", "recall", "n_est", "n_gt"):
        assert got[k] == want[k], k
    assert abs(got["fscore"] - want["fscore"]) <= 1e-15 * abs(want["fscore"])
    assert np.array_equal(got["hist_est"], want["hist_est"]) and np.array_equal(got["hist_gt"], want["hist_gt"])
    return got


def test_evaluate_against_oracle(scene):
    s = scene
    r = check_evaluate(s["est"], s["gt"], s["T_true"], s["vol"], s["ovol"], s["tau"])
    assert 0.8 < r["precision"] < 0.95 and 0.5 < r["recall"] < 0.9 and r["n_est"] < 5000 and r["n_gt"] < 5000
    assert r["curve_est"].shape == (499,) and r["curve_est"][-1] <= 1.0 and np.all(np.diff(r["curve_gt"]) >= 0)
    check_evaluate(s["est"], s["gt"], s["init"], s["vol"], s["ovol"], s["tau"])


BOX = np.array([[-10.0, -10.0], [10.0, -10.0], [10.0, 10.0], [-10.0, 10.0]])


def test_evaluate_known_answers():
    tau = 0.01
    g = np.arange(12) * 4.0 * tau
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    vol, ovol = F.make_volume(2, -10.0, 10.0, BOX), (2, -10.0, 10.0, BOX)
    r = check_evaluate(pts, pts, np.eye(4), vol, ovol, tau)
    assert r["precision"] == 1.0 and r["recall"] == 1.0 and r["fscore"] == 1.0 and r["n_est"] == len(pts)
    T = np.eye(4)
    T[0, 3] = 1.5 * tau
    r = check_evaluate(pts, pts, T, vol, ovol, tau, down_sample=False)
    assert r["precision"] == 0.0 and r["recall"] == 0.0 and r["fscore"] == 0.0
    r = check_evaluate(pts[: len(pts) // 2], pts, np.eye(4), vol, ovol, tau)
    assert r["precision"] == 1.0 and abs(r["recall"] - 0.5) < 1e-12
    empty = F.make_volume(2, 50.0, 60.0, BOX)
    r = F.evaluate(dev(pts), dev(pts), np.eye(4), empty, tau)
    assert r["precision"] == 0.0 and r["recall"] == 0.0 and r["fscore"] == 0.0 and r["n_est"] == 0 and r["n_gt"] == 0
    assert not r["hist_est"].any() and not r["hist_gt"].any()
    T[0, 3] = 100.0                                              # only the estimate leaves the volume
    r = F.evaluate(dev(pts), dev(pts), T, vol, tau)
    assert r["fscore"] == 0.0 and r["n_est"] == 0 and r["n_gt"] == len(pts)


def test_dist_hist_exact():
    rng = np.random.default_rng(8)
    tau, nbins = 0.003, 499
    w = tau / 100.0
    d = np.concatenate([rng.random(70001) * 0.02, np.full(500, 5 * tau), np.zeros(77), np.arange(499) * w, [tau, np.nextafter(tau, 0)]])
    counts, below = F.dist_hist(dev(d), tau, nbins, w)
    b = np.floor(d / w)
    want = np.bincount(b[(b >= 0) & (b < nbins)].astype(np.int64), minlength=nbins).astype(np.uint64)
    assert np.array_equal(counts, want) and below == int((d < tau).sum())
    assert F.dist_hist(torch.zeros(0, device=DEV, dtype=torch.float64), tau, nbins, w)[1] == 0


# ---- command line -----------------------------------------------------------------------------------------------------
def test_command_line_matches_evaluate_files(tmp_path):
    gt, ply = str(tmp_path / "gt"), str(tmp_path / "ply")
    synthetic.write_tanks_gt_tree(gt, ply, scenes=("Barn", "Truck"), n_gt=3000, n_est=3000)
    env = dict(os.environ, PYTHONPATH=REPO)
    p = subprocess.run([sys.executable, "-m", "rc_mvsnet_amd.tanks_fscore", "--plydir", ply, "--gtpath", gt, "--scenes", "Barn,Truck",
                        "--curves", str(tmp_path / "curves")], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 3 and lines[-1]["summary"] and lines[-1]["scenes"] == 2
    for line, scene in zip(lines, ("Barn", "Truck")):
        want = F.evaluate_files(ply, gt, scene, device=DEV)
        assert line == json.loads(json.dumps(want))
        assert line["scene"] == scene and line["tau"] == F.SCENE_TAU[scene] and len(line["icp"]) == 3
        assert 0.5 < line["fscore"] < 1.0
        assert np.load(tmp_path / "curves" / f"{scene}.precision.npy").shape == (499,)
    assert abs(lines[-1]["mean_fscore"] - (lines[0]["fscore"] + lines[1]["fscore"]) / 2) < 1e-15
