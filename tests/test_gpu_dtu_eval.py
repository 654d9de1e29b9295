"""GPU: the DTU scorer (rc_mvsnet_amd/dtu_eval.py over csrc/pointcloud.hip) against the fp64 oracle of tests/dtu_oracle.py:
nearest distances on ragged clouds and corner cases, the reduction's kept mask bit for bit, DataInMask / StlAbovePlane at their
knife edges, a known answer, a synthetic scan, a DTU-sized scan against fp64 brute force, and the command line."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import dtu_oracle as O
from conftest import REPO
from rc_mvsnet_amd import _lib, dtu_eval, fusion, synthetic

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(REPO, "tests", "golden", "dtu_eval")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _nn_check(q, t, cap, bb=None):
    got = dtu_eval.nearest_distances(_t(q), _t(t), cap=cap, lattice=None if bb is None else (bb, 60.0)).cpu().numpy()
    want = O.nearest(q, t, cap, None if bb is None else O.lattice(bb))
    assert got.shape == want.shape
    err = np.abs(got - want)
    assert float(err.max(initial=0.0)) <= 1e-6, (float(err.max()), int(err.argmax()))
    return got


def test_nearest_ragged_clouds_against_brute_force():
    _lib.load()
    rng = np.random.default_rng(0)
    t = np.concatenate([rng.random((14000, 3)) * [200, 150, 80], rng.normal(50, 0.3, (1001, 3))])
    q = np.concatenate([rng.random((19000, 3)) * [220, 170, 100] - 10, rng.normal(50, 0.5, (600, 3)),
                        rng.random((400, 3)) * 900 - 450])          # some far outside the target's box
    bb = np.array([[-5.0, -5.0, -5.0], [170.0, 140.0, 70.0]])      # lattice ends at 175 / 175 / 115: some queries outside it
    _nn_check(q, t, 60.0)
    got = _nn_check(q, t, 20.0, bb)
    assert (got == 20.0).sum() > 400 and (got < 1.0).sum() > 300


def test_nearest_corner_cases():
    _lib.load()
    rng = np.random.default_rng(1)
    q = rng.random((3000, 3)) * 50
    _nn_check(q, np.array([[25.0, 25.0, 25.0]]), 60.0)                            # one target point
    _nn_check(q[:1], rng.random((5000, 3)) * 50, 60.0)                            # one query
    got = dtu_eval.nearest_distances(_t(q), torch.zeros((0, 3), device=DEV), cap=20.0)
    assert torch.equal(got.cpu(), torch.full((3000,), 20.0, dtype=torch.float64))        # empty target
    lat = np.mgrid[0:12, 0:12, 0:12].reshape(3, -1).T * 0.5                       # points on cell boundaries, exact duplicates
    _nn_check(np.concatenate([lat, lat + 0.25, lat[::7]]), np.concatenate([lat, lat[:100]]), 60.0)
    far = np.concatenate([rng.random((10000, 3)) * [1e5, 1.0, 1.0], [[0, 0, 0], [1e5, 1, 1]]])   # extent that forces the edge clamp
    g = dtu_eval.Grid(_t(far), h_min=1e-6)
    assert np.prod(g.dims) <= 8 * len(far) and g.h > 1.0
    _nn_check(rng.random((4000, 3)) * [1e5, 3.0, 3.0], far, 60.0)


def _invariants(pts, keep, order, dst):
    k = pts[keep]
    for s in range(0, len(k), 2048):
        d = np.sqrt(O._d2(k[s:s + 2048], k))
        d[np.arange(len(d)), s + np.arange(len(d))] = np.inf
        assert d.min() > dst
    rank = np.empty(len(pts), dtype=np.int64)
    rank[order] = np.arange(len(pts))
    rem = np.nonzero(~keep)[0]
    kidx = np.nonzero(keep)[0]
    for s in range(0, len(rem), 2048):
        r = rem[s:s + 2048]
        close = np.sqrt(O._d2(pts[r], pts[kidx])) <= dst
        earlier = rank[kidx][None, :] < rank[r][:, None]
        assert (close & earlier).any(axis=1).all()


@pytest.mark.parametrize("seed", [0, 1])
def test_reduction_bit_identical_to_sequential_greedy(seed):
    _lib.load()
    rng = np.random.default_rng(seed)
    pts = np.concatenate([rng.random((12000, 3)) * [20, 20, 5], rng.normal(8.0, 0.05, (3000, 3)),    # clusters denser than 0.2
                          np.repeat(rng.random((300, 3)) * 20, 5, axis=0)]).astype(np.float32)      # exact duplicates
    order = rng.permutation(len(pts))
    kept, reduced = dtu_eval.reduce_points(_t(pts), dst=0.2, order=torch.from_numpy(order))
    want = O.greedy_reduce(pts, order, 0.2)
    got = kept.cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(reduced.cpu().numpy(), pts[want])
    _invariants(pts, got, order, 0.2)
    assert 2 <= dtu_eval.last_reduce_rounds < 200


def test_reduction_default_order_is_the_seeded_permutation():
    _lib.load()
    pts = np.random.default_rng(2).random((5000, 3)).astype(np.float32) * 3
    k1, _ = dtu_eval.reduce_points(_t(pts), seed=5)
    k2, _ = dtu_eval.reduce_points(_t(pts), order=dtu_eval.permutation(len(pts), 5))
    assert torch.equal(k1, k2)
    assert np.array_equal(k1.cpu().numpy(), O.greedy_reduce(pts, dtu_eval.permutation(len(pts), 5).numpy(), 0.2))


def test_mask_and_plane_knife_edges():
    _lib.load()
    res, bb = 0.5, np.array([[10.0, -4.0, 2.0], [13.0, -1.0, 5.0]])
    rng = np.random.default_rng(3)
    mask = rng.random((7, 6, 5)) > 0.4
    mask[0, :, :] = mask[-1, :, :] = True
    k = np.arange(-1, 10) - 0.5                                   # v = k + 1.5: exact halves, both mask edges and beyond
    grid = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
    q = np.concatenate([bb[0] + grid * res, bb[0] + rng.random((5000, 3)) * 4.5 - 0.5]).astype(np.float32)
    d = torch.full((len(q),), 1.0, dtype=torch.float64, device=DEV)
    d[::3] = 25.0                                                 # above the outlier threshold
    flags, sel, st = dtu_eval.select_stats(_t(q), d, "mask", (bb[0], res), 20.0, obs_mask=torch.from_numpy(mask))
    want = O.data_in_mask(q, bb, res, mask)
    assert np.array_equal(flags.cpu().numpy(), want)
    assert want.sum() > 100 and (~want).sum() > 100
    assert st["n"] == int((want & (d.cpu().numpy() < 20)).sum()) == len(sel)
    P = np.array([0.0, 0.0, 1.0, -3.0])
    qp = np.concatenate([q, [[1.0, 1.0, 3.0], [2.0, 2.0, 3.0]]]).astype(np.float32)      # on the plane: not above
    zeros = torch.zeros(len(qp), dtype=torch.float64, device=DEV)
    flags, _, _ = dtu_eval.select_stats(_t(qp), zeros, "plane", P, 20.0)
    want = O.stl_above_plane(qp, P)
    assert np.array_equal(flags.cpu().numpy(), want) and not want[-1] and not want[-2]
    P = np.array([0.3, -0.7, 0.2, 1.1])
    flags, _, _ = dtu_eval.select_stats(_t(qp), zeros, "plane", P, 20.0)
    assert np.array_equal(flags.cpu().numpy(), O.stl_above_plane(qp, P))


def test_known_answer_shifted_lattice():
    """data = the stl lattice moved 0.5 mm along the plane's normal: accuracy = completeness = 0.5."""
    _lib.load()
    xy = np.stack(np.meshgrid(np.arange(120) * 0.3, np.arange(100) * 0.3, indexing="ij"), -1).reshape(-1, 2)
    stl = np.concatenate([xy, np.full((len(xy), 1), 10.0)], 1).astype(np.float32)
    data = stl + np.float32([0, 0, 0.5])
    bb = np.array([[-1.0, -1.0, 5.0], [40.0, 40.0, 15.0]])
    mask = np.ones((100, 100, 30), dtype=bool)
    r = dtu_eval.evaluate_scan(_t(data), _t(stl), torch.from_numpy(mask), bb, 0.5, np.array([0, 0, 1.0, -5.0]))
    assert abs(r["MeanData"] - 0.5) <= 1e-5 and abs(r["MeanStl"] - 0.5) <= 1e-5
    assert r["nData"] == len(data) and r["nStl"] == len(stl) and r["VarData"] <= 1e-12
    assert abs(dtu_eval.summarize([r])["overall"] - 0.5) <= 1e-5


def _compare(got, want):
    for k in ("nStl", "nData", "MedStl", "MedData"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("MeanStl", "MeanData", "VarStl", "VarData"):
        assert abs(got[k] - want[k]) <= 1e-9 * abs(want[k]), (k, got[k], want[k])


def test_evaluate_scan_against_oracle():
    _lib.load()
    s = synthetic.dtu_eval_scan(n_stl=15000, n_data=20000, extent=100.0, res=2.0, seed=4)
    got = dtu_eval.evaluate_scan(_t(s["data"]), _t(s["stl"]), torch.from_numpy(s["obs_mask"]), s["bb"], s["res"], s["plane"],
                                 seed=9, per_point=True)
    order = dtu_eval.permutation(len(s["data"]), 9).numpy()
    want = O.evaluate_scan(s["data"], s["stl"], s["obs_mask"], s["bb"], s["res"], s["plane"], order, cap=20.0)
    assert np.array_equal(got["DataInMask"].cpu().numpy(), want["DataInMask"])
    assert np.array_equal(got["StlAbovePlane"].cpu().numpy(), want["StlAbovePlane"])
    assert float(np.abs(got["Ddata"].cpu().numpy() - want["Ddata"]).max()) <= 1e-6
    assert float(np.abs(got["Dstl"].cpu().numpy() - want["Dstl"]).max()) <= 1e-6
    _compare(got, want)
    assert 0 < got["nData"] < len(got["Qdata"]) and 0 < got["nStl"] < len(s["stl"])


def _brute_min(q, t, cap, lo, hi):
    q = q.double()
    best = torch.full((len(q),), float("inf"), dtype=torch.float64, device=q.device)
    for s in range(0, len(t), 1 << 13):                          # fp64 brute force in chunks (cdist's direct mode has a grid limit)
        c = t[s:s + (1 << 13)].double()
        dx, dy, dz = (q[:, None, a] - c[None, :, a] for a in range(3))
        best = torch.minimum(best, ((dx * dx + dy * dy) + dz * dz).min(dim=1).values)
    out = torch.clamp(best.sqrt(), max=cap)
    lo, hi = torch.tensor(lo, device=q.device), torch.tensor(hi, device=q.device)
    inside = ((q >= lo) & (q < hi)).all(dim=1)
    return torch.where(inside, out, torch.full_like(out, cap))


def test_dtu_sized_scan_against_brute_force():
    _lib.load()
    s = synthetic.dtu_eval_scan(n_stl=2_500_000, n_data=3_000_000, extent=600.0, res=4.0, seed=6)
    data, stl = _t(s["data"]), _t(s["stl"])
    r = dtu_eval.evaluate_scan(data, stl, torch.from_numpy(s["obs_mask"]), s["bb"], s["res"], s["plane"], per_point=True)
    assert 100_000 < r["nData"] and 100_000 < r["nStl"] and 0.0 < r["MeanData"] < 20.0 and 0.0 < r["MeanStl"] < 20.0
    qdata = r["Qdata"]
    lo, hi = dtu_eval.lattice_bounds(s["bb"])
    g = torch.Generator().manual_seed(0)
    for src, dst, d in ((qdata, stl, r["Ddata"]), (stl, qdata, r["Dstl"])):
        idx = torch.randint(0, len(src), (4096,), generator=g).to(DEV)
        want = _brute_min(src[idx], dst, 20.0, lo, hi)
        assert float((d[idx] - want).abs().max()) <= 1e-6


def _fixture_scans():
    sys.path.insert(0, GOLDEN)
    try:
        import make_dtu_eval_fixtures as mk
    finally:
        sys.path.remove(GOLDEN)
    return mk.scans()


def test_cli_end_to_end_on_golden_layout(tmp_path):
    _lib.load()
    scans = _fixture_scans()
    gt = tmp_path / "MVS_Data"
    os.makedirs(gt / "Points" / "stl")
    os.makedirs(gt / "ObsMask")
    for name in os.listdir(GOLDEN):
        if name.endswith(".mat"):
            shutil.copy(os.path.join(GOLDEN, name), gt / "ObsMask" / name)
    plydir = tmp_path / "out"
    os.makedirs(plydir)
    for scan, s in scans.items():
        (plydir / f"scan{scan}.ply").write_bytes(fusion.ply_bytes(s["data"], np.zeros((len(s["data"]), 3), np.uint8)))
        (gt / "Points" / "stl" / f"stl{scan:03d}_total.ply").write_bytes(fusion.ply_bytes(s["stl"], np.zeros((len(s["stl"]), 3), np.uint8)))
    env = dict(os.environ, PYTHONPATH=REPO)
    p = subprocess.run([sys.executable, "-m", "rc_mvsnet_amd.dtu_eval", "--plydir", str(plydir), "--gtpath", str(gt),
                        "--scans", ",".join(str(k) for k in scans)], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == len(scans) + 1 and lines[-1]["summary"]
    for line in lines[:-1]:
        s = scans[line["scan"]]
        want = dtu_eval.evaluate_scan(_t(s["data"]), _t(s["stl"]), torch.from_numpy(s["obs_mask"]), s["bb"], s["res"], s["plane"])
        for k in dtu_eval.STAT_FIELDS:
            assert line[k] == want[k], k
    want = dtu_eval.summarize(lines[:-1])
    assert all(abs(lines[-1][k] - want[k]) <= 1e-12 for k in ("acc", "comp", "overall"))
