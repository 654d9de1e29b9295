"""The DTU scorer's kernels (csrc/pointcloud.hip) on the CPU emulation of tests/emu, driven through rc_mvsnet_amd/dtu_eval.py on
CPU tensors and checked against the fp64 oracle (tests/dtu_oracle.py): the kept mask of the reduction bit for bit, distances
within 1e-6, masks and statistics.  The emulation runs blocks one after another, so this also pins that no result depends on
the blocks' order."""
import numpy as np
import pytest
import torch

import dtu_oracle as O
from rc_mvsnet_amd import dtu_eval, fusion, synthetic


@pytest.fixture
def emu_dtu(emu, monkeypatch):
    monkeypatch.setattr(dtu_eval, "_chk", fusion._chk)          # the emu fixture routes fusion / ops; the scorer module too
    monkeypatch.setattr(dtu_eval, "_stream", fusion._stream)
    return emu


def _scan():
    return synthetic.dtu_eval_scan(n_stl=1500, n_data=2000, extent=30.0, res=1.5, seed=3)


def test_reduction_on_emulated_kernels(emu_dtu):
    rng = np.random.default_rng(0)
    pts = np.concatenate([rng.random((1500, 3)) * 4.0, rng.normal(2.0, 0.04, (400, 3)),
                          np.repeat(rng.random((25, 3)) * 4.0, 4, axis=0)]).astype(np.float32)
    order = rng.permutation(len(pts))
    kept, reduced = dtu_eval.reduce_points(torch.from_numpy(pts), dst=0.2, order=torch.from_numpy(order))
    want = O.greedy_reduce(pts, order, 0.2)
    assert np.array_equal(kept.numpy(), want)
    assert np.array_equal(reduced.numpy(), pts[want])
    assert dtu_eval.last_reduce_rounds >= 2


def test_nearest_on_emulated_kernels(emu_dtu):
    s = _scan()
    q, t = s["data"], s["stl"][:1200]
    for cap, lat in ((60.0, None), (20.0, s["bb"]), (1.0, None)):
        got = dtu_eval.nearest_distances(torch.from_numpy(q), torch.from_numpy(t), cap=cap, lattice=None if lat is None else (lat, 60.0))
        want = O.nearest(q, t, cap, None if lat is None else O.lattice(lat))
        assert got.dtype == torch.float64 and float(np.abs(got.numpy() - want).max()) <= 1e-6
    got = dtu_eval.nearest_distances(torch.from_numpy(q[:5]), torch.zeros((0, 3)), cap=20.0)
    assert torch.equal(got, torch.full((5,), 20.0, dtype=torch.float64))


def test_evaluate_scan_on_emulated_kernels(emu_dtu):
    s = _scan()
    order = dtu_eval.permutation(len(s["data"]), 0).numpy()
    got = dtu_eval.evaluate_scan(torch.from_numpy(s["data"]), torch.from_numpy(s["stl"]), torch.from_numpy(s["obs_mask"]), s["bb"], s["res"],
                                 s["plane"], per_point=True)
    want = O.evaluate_scan(s["data"], s["stl"], s["obs_mask"], s["bb"], s["res"], s["plane"], order, cap=20.0)
    assert np.array_equal(got["DataInMask"].numpy(), want["DataInMask"])
    assert np.array_equal(got["StlAbovePlane"].numpy(), want["StlAbovePlane"])
    assert float(np.abs(got["Ddata"].numpy() - want["Ddata"]).max()) <= 1e-6
    assert float(np.abs(got["Dstl"].numpy() - want["Dstl"]).max()) <= 1e-6
    assert 0 < got["nData"] < len(s["data"]) and 0 < got["nStl"] < len(s["stl"])
    for k in ("nStl", "nData", "MedStl", "MedData"):
        assert got[k] == want[k], k
    for k in ("MeanStl", "MeanData", "VarStl", "VarData"):
        assert abs(got[k] - want[k]) <= 1e-9 * abs(want[k]), k
