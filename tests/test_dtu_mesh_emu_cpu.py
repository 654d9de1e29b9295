"""MeshSupSamp's kernels (csrc/pointcloud.hip: pc_mesh_*) on the CPU emulation of tests/emu, driven through
rc_mvsnet_amd.dtu_eval.sample_mesh on CPU tensors: the points equal the literal oracle's (tests/mesh_oracle.py) rounded to fp32,
bit for bit, on small meshes with degenerate, tiny and large triangles; a bad index is refused."""
import numpy as np
import pytest
import torch

import dtu_oracle as O
import mesh_oracle as M
from rc_mvsnet_amd import _lib, dtu_eval, fusion, synthetic


@pytest.fixture
def emu_dtu(emu, monkeypatch):
    monkeypatch.setattr(dtu_eval, "_chk", fusion._chk)          # the emu fixture routes fusion / ops; the scorer module too
    monkeypatch.setattr(dtu_eval, "_stream", fusion._stream)
    return emu


def _mixed_mesh(seed, n_verts=60, n_faces=120):
    rng = np.random.default_rng(seed)
    v = (rng.random((n_verts, 3)) * 3.0 - 1.0).astype(np.float32)
    v[-4:] = [[0, 0, 0], [4.0, 0, 0], [0, 3.0, 0.5], [2.0, 0, 0]]            # a large triangle and a collinear one
    f = rng.integers(0, n_verts - 4, (n_faces, 3))
    f[::9, 1] = f[::9, 0]                                                       # repeated vertex
    extra = [[n_verts - 4, n_verts - 3, n_verts - 2], [n_verts - 4, n_verts - 1, n_verts - 3],
             [n_verts - 2, n_verts - 4, n_verts - 3]]
    return v, np.concatenate([f, extra]).astype(np.int32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("seed,dst", [(0, 0.2), (1, 0.1), (2, 0.35)])
def test_sampling_bit_identical_to_literal_oracle(emu_dtu, seed, dst):
    v, f = _mixed_mesh(seed)
    got = dtu_eval.sample_mesh(torch.from_numpy(v), torch.from_numpy(f), dst)
    want = M.literal(v, f, dst).astype(np.float32)
    assert got.shape == want.shape and len(want) > len(v) + 500
    assert np.array_equal(_bits(got.numpy()), _bits(want))
    again = dtu_eval.sample_mesh(torch.from_numpy(v), torch.from_numpy(f.astype(np.int64)), dst)
    assert np.array_equal(_bits(again.numpy()), _bits(want))


def test_sampling_edge_cases(emu_dtu):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.05, 0.05, 0]], dtype=np.float32)
    for faces, n in (([[0, 1, 2]], 10),                          # the right triangle of the CPU known answers
                     ([[0, 0, 1], [0, 3, 3], [0, 1, 3]], 0),     # repeated vertices, a sliver below dst
                     ([[0, 3, 1], [1, 2, 3], [0, 1, 2]], None)):
        got = dtu_eval.sample_mesh(torch.from_numpy(v), torch.tensor(faces, dtype=torch.int32), 0.2)
        want = M.literal(v, faces, 0.2)
        assert n is None or len(want) == 4 + n
        assert np.array_equal(_bits(got.numpy()), _bits(want))
    got = dtu_eval.sample_mesh(torch.from_numpy(v), torch.zeros((0, 3), dtype=torch.int32), 0.2)
    assert torch.equal(got, torch.from_numpy(v))


def test_out_of_range_index_is_refused(emu_dtu):
    v, f = _mixed_mesh(3)
    for bad in (len(v), -1):
        g = f.copy()
        g[5, 2] = bad
        with pytest.raises(_lib.RcmvsError, match="outside"):
            dtu_eval.sample_mesh(torch.from_numpy(v), torch.from_numpy(g), 0.2)
        with pytest.raises(_lib.RcmvsError, match="outside"):
            dtu_eval.sample_mesh(torch.from_numpy(v), torch.from_numpy(g.astype(np.int64)), 0.2)


def test_evaluate_mesh_on_emulated_kernels(emu_dtu):
    s = synthetic.dtu_eval_mesh(nx=14, ny=12, edge=0.45, n_stl=900, res=1.5, seed=4)
    cloud = M.vectorised(s["verts"], s["faces"], 0.2).astype(np.float32)
    order = dtu_eval.permutation(len(cloud), 0).numpy()
    got = dtu_eval.evaluate_mesh(torch.from_numpy(s["verts"]), torch.from_numpy(s["faces"]), torch.from_numpy(s["stl"]),
                                 torch.from_numpy(s["obs_mask"]), s["bb"], s["res"], s["plane"], per_point=True)
    want = O.evaluate_scan(cloud, s["stl"], s["obs_mask"], s["bb"], s["res"], s["plane"], order, cap=20.0)
    assert np.array_equal(got["DataInMask"].numpy(), want["DataInMask"])
    assert float(np.abs(got["Ddata"].numpy() - want["Ddata"]).max()) <= 1e-6
    assert float(np.abs(got["Dstl"].numpy() - want["Dstl"]).max()) <= 1e-6
    for k in ("nStl", "nData", "MedStl", "MedData"):
        assert got[k] == want[k], k
    for k in ("MeanStl", "MeanData", "VarStl", "VarData"):
        assert abs(got[k] - want[k]) <= 1e-9 * abs(want[k]), k
