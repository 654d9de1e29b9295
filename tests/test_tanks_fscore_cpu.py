"""Host side of the Tanks and Temples F-score (rc_mvsnet_amd/tanks_fscore.py): the readers, the Umeyama fit, the trajectory
alignment, the command line, and the oracle's own known answers (tests/tanks_fscore_oracle.py)."""
import json

import numpy as np
import pytest

import tanks_fscore_oracle as O
from rc_mvsnet_amd import _lib, synthetic, tanks_fscore as F


def _sim(deg, scale, shift, axis=(0.2, -0.4, 0.9)):
    return synthetic._similarity(axis, deg, scale, shift)


# ---- readers ----------------------------------------------------------------------------------------------------------
def test_readers_on_a_written_tree(tmp_path):
    scenes = synthetic.write_tanks_gt_tree(str(tmp_path / "gt"), str(tmp_path / "ply"), scenes=("Barn",), n_gt=50, n_est=40, n_cams=5)
    p = F.scene_paths(str(tmp_path / "ply"), str(tmp_path / "gt"), "Barn")
    v = F.read_crop_json(p["crop"])
    s = scenes["Barn"]
    assert v["axis"] == 2 and v["axis_min"] == s["volume"]["axis_min"] and v["axis_max"] == s["volume"]["axis_max"]
    assert np.array_equal(v["polygon"], s["volume"]["polygon"][:, :2])
    assert np.array_equal(F.read_alignment(p["trans"]), s["init"])
    traj = F.read_trajectory_log(p["log"])
    assert traj.shape == (5, 4, 4) and traj.dtype == np.float64 and np.allclose(traj[:, 3], [0, 0, 0, 1])
    from rc_mvsnet_amd.dtu_io import read_ply_xyz
    assert np.array_equal(read_ply_xyz(p["gt"]), s["gt"]) and np.array_equal(read_ply_xyz(p["est"]), s["est"])


def test_crop_json_axes_and_malformed(tmp_path):
    good = {"axis_max": 2.0, "axis_min": -1.0, "bounding_polygon": [[0, 5, 0], [1, 6, 0], [0, 7, 1]], "orthogonal_axis": "Y"}
    path = tmp_path / "c.json"
    path.write_text(json.dumps(good))
    v = F.read_crop_json(str(path))
    assert v["axis"] == 1 and np.array_equal(v["polygon"], [[0, 0], [1, 0], [0, 1]])        # (x, z): the remaining axes in order
    for bad in ({k: good[k] for k in good if k != "axis_min"}, dict(good, orthogonal_axis="W"), dict(good, orthogonal_axis=1),
                dict(good, bounding_polygon=[[0, 0, 0], [1, 1, 1]]), dict(good, bounding_polygon=[[0, 0], [1, 1], [2, 2]]),
                dict(good, axis_max="high"), dict(good, bounding_polygon=[[0, 0, 0]] * (F.MAX_POLYGON + 1)), [1, 2]):
        path.write_text(json.dumps(bad))
        with pytest.raises(_lib.RcmvsError, match="c.json"):
            F.read_crop_json(str(path))
    path.write_text("{not json")
    with pytest.raises(_lib.RcmvsError, match="JSON"):
        F.read_crop_json(str(path))
    with pytest.raises(_lib.RcmvsError):
        F.read_crop_json(str(tmp_path / "missing.json"))


def test_trajectory_log_and_alignment_malformed(tmp_path):
    path = tmp_path / "t.log"
    rows = "1 0 0 0\n0 1 0 0\n0 0 1 0\n0 0 0 1\n"
    path.write_text("0 0 1\n" + rows + "\n1 1 1\n" + rows)
    assert F.read_trajectory_log(str(path)).shape == (2, 4, 4)
    for bad in ("0 0 1\n" + rows + "1 1 1\n", "0 0\n" + rows, "0 0 x\n" + rows, "0 0 1\n1 0 0\n0 1 0 0\n0 0 1 0\n0 0 0 1\n",
                "0 0 1\n1 0 0 nan\n0 1 0 0\n0 0 1 0\n0 0 0 1\n", ""):
        path.write_text(bad)
        with pytest.raises(_lib.RcmvsError, match="t.log"):
            F.read_trajectory_log(str(path))
    with pytest.raises(_lib.RcmvsError):
        F.read_trajectory_log(str(tmp_path / "missing.log"))
    tp = tmp_path / "a.txt"
    for bad in ("1 0 0\n0 1 0\n0 0 1\n", "1 0 0 0\n0 1 0 0\n0 0 1 0\n0 0 0 x\n", "1 0 0 0\n0 1 0 0\n0 0 1 0\n0 0 0 inf\n"):
        tp.write_text(bad)
        with pytest.raises(_lib.RcmvsError, match="a.txt"):
            F.read_alignment(str(tp))


# ---- alignment --------------------------------------------------------------------------------------------------------
def test_umeyama_recovers_a_similarity():
    rng = np.random.default_rng(0)
    src = rng.normal(size=(40, 3))
    for T in (_sim(37.0, 1.8, (0.3, -2.0, 1.0)), _sim(170.0, 0.4, (5.0, 0.0, -1.0))):
        dst = src @ T[:3, :3].T + T[:3, 3]
        assert np.abs(F.umeyama(src, dst) - T).max() <= 1e-12
    R = _sim(25.0, 1.0, (0.1, 0.2, 0.3))
    dst = src @ R[:3, :3].T + R[:3, 3]
    assert np.abs(F.umeyama(src, dst, with_scaling=False) - R).max() <= 1e-12


def test_umeyama_reflection_case():
    """a planar cloud: the cross-covariance has rank 2 and the sign of the third singular vectors is arbitrary, so the det < 0 fix
    decides between the similarity and its mirror image"""
    rng = np.random.default_rng(1)
    src = rng.normal(size=(30, 3))
    src[:, 2] = 0.0                                              # planar: the cross-covariance has rank 2
    T = _sim(50.0, 1.3, (1.0, 2.0, 3.0))
    dst = src @ T[:3, :3].T + T[:3, 3]
    got = F.umeyama(src, dst)
    assert np.linalg.det(got[:3, :3]) > 0 and np.abs(got - T).max() <= 1e-12
    full = rng.normal(size=(30, 3))                            # a true mirror image: the proper rotation is returned, not the reflection
    got = F.umeyama(full, full * np.array([1.0, 1.0, -1.0]))
    assert np.linalg.det(got[:3, :3]) > 0
    m = O.umeyama_from_moments(_moments(full, full * np.array([1.0, 1.0, -1.0])))
    assert np.abs(m - got).max() <= 1e-12
    with pytest.raises(_lib.RcmvsError):
        F.umeyama(src[:2], dst[:2])


def _moments(s, t):
    mom = np.zeros(18)
    mom[0] = len(s)
    mom[1] = ((s - t) ** 2).sum()
    mom[2:5], mom[5:8] = s.sum(0), t.sum(0)
    mom[8:17] = (s[:, :, None] * t[:, None, :]).sum(0).ravel()
    mom[17] = (s * s).sum()
    return mom


def test_umeyama_from_moments_matches_arrays():
    rng = np.random.default_rng(2)
    s = rng.normal(size=(200, 3)) + 2.0
    T = _sim(12.0, 1.05, (0.1, -0.1, 0.2))
    t = s @ T[:3, :3].T + T[:3, 3] + rng.normal(0, 0.01, s.shape)
    a, b = F.umeyama(s, t), F.umeyama_from_moments(_moments(s, t))
    assert np.abs(a - b).max() <= 1e-10
    assert np.abs(b - O.umeyama_from_moments(_moments(s, t))).max() <= 1e-14


def test_trajectory_alignment_identical_trajectories():
    rng = np.random.default_rng(3)
    traj = np.stack([_sim(rng.uniform(0, 180), 1.0, rng.uniform(-3, 3, 3), rng.normal(size=3)) for _ in range(20)])
    gt_trans = _sim(33.0, 2.5, (1.0, -4.0, 0.5))
    assert np.abs(F.trajectory_alignment(traj, traj, gt_trans) - gt_trans).max() <= 1e-10
    with pytest.raises(_lib.RcmvsError, match="1600"):
        F.trajectory_alignment(np.repeat(traj, 81, 0), np.repeat(traj, 81, 0), gt_trans)
    with pytest.raises(_lib.RcmvsError):
        F.trajectory_alignment(traj, traj[:10], gt_trans)


# ---- command line -----------------------------------------------------------------------------------------------------
def test_scene_tau():
    assert F.SCENE_TAU == {"Barn": 0.01, "Caterpillar": 0.005, "Church": 0.025, "Courthouse": 0.025, "Ignatius": 0.003,
                           "Meetingroom": 0.01, "Truck": 0.005}


def test_command_line_parsing(capsys):
    a = F.parse_args(["--plydir", "p", "--gtpath", "g"])
    assert a.scenes == list(F.SCENE_TAU) and a.gpus == 1 and not a.no_register and a.traj is None and a.curves is None
    a = F.parse_args(["--plydir", "p", "--gtpath", "g", "--scenes", "Barn, Truck", "--no-register", "--curves", "c", "--gpus", "2"])
    assert a.scenes == ["Barn", "Truck"] and a.no_register and a.curves == "c" and a.gpus == 2
    assert F.parse_args(["--plydir", "p", "--gtpath", "g", "--scenes", "Barn", "--traj", "x.log"]).traj == "x.log"
    for bad in (["--plydir", "p"], ["--plydir", "p", "--gtpath", "g", "--scenes", "Family"],
                ["--plydir", "p", "--gtpath", "g", "--traj", "x.log"], ["--plydir", "p", "--gtpath", "g", "--gpus", "0"]):
        with pytest.raises(SystemExit):
            F.parse_args(bad)
    capsys.readouterr()


def test_needs_a_gpu_or_says_so(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="GPU"):
        F.main(["--plydir", "p", "--gtpath", "g", "--scenes", "Barn"])
    with pytest.raises(_lib.RcmvsError, match="GPU"):
        F.crop(torch.zeros((4, 3)), F.make_volume(2, 0.0, 1.0, [[0, 0], [1, 0], [0, 1]]))


# ---- the oracle's own known answers -------------------------------------------------------------------------------------
BOX = (2, -10.0, 10.0, np.array([[-10.0, -10.0], [10.0, -10.0], [10.0, 10.0], [-10.0, 10.0]]))


def _grid_cloud(tau):
    g = np.arange(12) * 4.0 * tau                              # spacing 4 tau: every point alone in its tau / 2 voxel
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


def test_oracle_identical_clouds():
    pts = _grid_cloud(0.01)
    r = O.evaluate(pts, pts, np.eye(4), BOX, 0.01)
    assert r["precision"] == 1.0 and r["recall"] == 1.0 and r["fscore"] == 1.0 and r["n_est"] == r["n_gt"] == len(pts)
    assert r["hist_est"][0] == len(pts) and r["hist_est"][1:].sum() == 0


def test_oracle_shifted_cloud_scores_zero():
    tau = 0.01
    pts = _grid_cloud(tau)
    T = np.eye(4)
    T[0, 3] = 1.5 * tau
    r = O.evaluate(pts, pts, T, BOX, tau, down_sample=False)
    assert r["precision"] == 0.0 and r["recall"] == 0.0 and r["fscore"] == 0.0


def test_oracle_half_missing_estimate():
    pts = _grid_cloud(0.01)
    r = O.evaluate(pts[: len(pts) // 2], pts, np.eye(4), BOX, 0.01)
    assert r["precision"] == 1.0 and abs(r["recall"] - 0.5) < 1e-12 and abs(r["fscore"] - 2.0 / 3.0) < 1e-12


def test_oracle_voxel_and_crop_by_hand():
    pts = np.array([[0, 0, 0], [0.4, 0, 0], [0.6, 0, 0], [0.1, 0.1, 0.1], [-0.4, 0, 0]], dtype=np.float32)
    out = O.voxel_down_sample(pts, 1.0)                          # origin -0.9: voxels [-0.9, 0.1) and [0.1, 1.1) in x
    want = np.array([[(0.0 + np.float32(-0.4)) / 2, 0, 0], [(np.float64(np.float32(0.4)) + np.float32(0.6) + np.float32(0.1)) / 3] + [np.float32(0.1) / 3.0] * 2])
    assert np.array_equal(out, want.astype(np.float32))
    tri = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    q = np.array([[0.2, 0.2, 0.5], [0.8, 0.8, 0.5], [0.2, 0.2, 1.5], [0.2, 0.2, 1.0], [0.2, 0.2, 0.0]], dtype=np.float32)
    f, _ = O.crop(q, 2, 0.0, 1.0, tri)
    assert f.tolist() == [True, False, False, True, True]


def test_oracle_candidate_search_equals_brute_force():
    rng = np.random.default_rng(5)
    t = rng.random((3000, 3)).astype(np.float32)
    t = np.concatenate([t, t[:100]])
    q = np.concatenate([t[rng.integers(0, len(t), 500)].astype(np.float64), rng.random((1500, 3))])
    a, b = O.nearest(q, t, brute=True), O.nearest(q, t, brute=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
