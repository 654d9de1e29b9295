"""GPU: mesh evaluation (rc_mvsnet_amd/dtu_eval.py: sample_mesh / evaluate_mesh over csrc/pointcloud.hip's pc_mesh_* kernels)
against the oracles of tests/mesh_oracle.py and tests/dtu_oracle.py: super-sampling bit for bit on mixed meshes, a mesh without
faces, a known answer, a whole evaluation, the command line with its error clouds, and the 2^31 guard."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import dtu_oracle as O
import mesh_oracle as M
from conftest import REPO
from rc_mvsnet_amd import _lib, dtu_eval, synthetic

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _mixed_mesh():
    """about 10^4 faces: DTU-like small triangles, slivers, repeated-vertex and collinear ones, and last one large triangle with
    more than 10^5 samples at dst 0.2"""
    rng = np.random.default_rng(0)
    c = rng.random((8000, 3)) * [300.0, 250.0, 40.0]
    small = np.concatenate([c, c + rng.normal(0, 0.4, (8000, 3)), c + rng.normal(0, 0.4, (8000, 3))])
    fs = np.arange(24000).reshape(3, 8000).T.copy()
    fs[::13, 2] = fs[::13, 1]                                        # repeated vertex
    L, eps = rng.uniform(0.5, 5.0, 1500), rng.uniform(1e-3, 0.2, 1500)
    c = rng.random((1500, 3)) * 200.0
    sliver = np.concatenate([c, c + np.stack([L, 0 * L, 0 * L], 1), c + np.stack([L / 2, eps, 0 * L], 1)])
    fl = 24000 + np.arange(4500).reshape(3, 1500).T
    t = rng.uniform(0.2, 3.0, 500)
    c = rng.random((500, 3)) * 100.0
    line = np.concatenate([c, c + t[:, None], c + 2.5 * t[:, None]])                  # collinear
    fc = 28500 + np.arange(1500).reshape(3, 500).T
    big = np.array([[0, 0, 0], [120, 0, 0], [0, 110, 5.0]]) - 300.0
    v = np.concatenate([small, sliver, line, big])
    f = np.concatenate([fs, fl, fc, [[30000, 30001, 30002]]])
    return v.astype(np.float32), f.astype(np.int32)


def test_sampling_bit_identical_to_oracle_and_deterministic():
    _lib.load()
    v, f = _mixed_mesh()
    assert 9_000 <= len(f) <= 11_000
    want = M.vectorised(v, f, 0.2).astype(np.float32)
    big = M.literal(v, f[-1:], 0.2)
    assert len(big) - len(v) >= 100_000
    got = dtu_eval.sample_mesh(_t(v), _t(f, np.int32), 0.2)
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    again = dtu_eval.sample_mesh(_t(v), _t(f, np.int32), 0.2)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    for dst in (0.1, 0.5):
        got = dtu_eval.sample_mesh(_t(v), _t(f, np.int64), dst)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(M.vectorised(v, f, dst)))


def test_mesh_without_faces_is_its_vertices():
    _lib.load()
    s = synthetic.dtu_eval_scan(n_stl=3000, n_data=4000, extent=60.0, res=2.0, seed=2)
    data, stl = _t(s["data"]), _t(s["stl"])
    got = dtu_eval.sample_mesh(data, torch.zeros((0, 3), dtype=torch.int32, device=DEV))
    assert torch.equal(got, data)
    args = (stl, torch.from_numpy(s["obs_mask"]), s["bb"], s["res"], s["plane"])
    a = dtu_eval.evaluate_mesh(data, torch.zeros((0, 3), dtype=torch.int32, device=DEV), *args)
    b = dtu_eval.evaluate_scan(data, *args)
    assert set(a) == set(b) == set(dtu_eval.STAT_FIELDS)
    for k in dtu_eval.STAT_FIELDS:
        assert a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])), k


def test_known_answer_offset_square():
    """a 20 mm square of two triangles 1 mm above a 0.2 mm stl grid on its plane: every reduced sample is 1 mm above the plane
    and at most half a grid diagonal (0.1414 mm) from a grid point in it"""
    _lib.load()
    v = np.array([[0, 0, 1], [20, 0, 1], [20, 20, 1], [0, 20, 1]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    g = np.arange(101) * 0.2
    stl = np.stack(list(np.meshgrid(g, g, indexing="ij")) + [np.zeros((101, 101))], -1).reshape(-1, 3)
    bb = np.array([[-5.0, -5.0, -5.0], [25.0, 25.0, 5.0]])
    mask = np.ones((31, 31, 11), dtype=bool)
    plane = np.array([0.0, 0.0, 1.0, 0.5])                          # z > -0.5: every stl point counts
    r = dtu_eval.evaluate_mesh(_t(v), _t(f, np.int32), _t(stl), torch.from_numpy(mask), bb, 1.0, plane)
    assert r["nData"] > 1000 and r["nStl"] == len(stl)
    assert 1.0 <= r["MeanData"] <= np.sqrt(1 + 0.1414 ** 2) + 1e-9 and r["MedData"] <= 1.0101
    assert 1.0 <= r["MeanStl"] < 1.2


def test_evaluate_mesh_against_oracle():
    _lib.load()
    s = synthetic.dtu_eval_mesh(nx=40, ny=30, edge=0.45, n_stl=4000, res=1.5, seed=5)
    cloud = M.vectorised(s["verts"], s["faces"], 0.2).astype(np.float32)
    order = np.random.default_rng(1).permutation(len(cloud))
    got = dtu_eval.evaluate_mesh(_t(s["verts"]), _t(s["faces"], np.int32), _t(s["stl"]), torch.from_numpy(s["obs_mask"]), s["bb"],
                                 s["res"], s["plane"], order=torch.from_numpy(order), per_point=True)
    want = O.evaluate_scan(cloud, s["stl"], s["obs_mask"], s["bb"], s["res"], s["plane"], order, cap=20.0)
    assert np.array_equal(got["Qdata"].cpu().numpy(), cloud[want["keep"]])
    assert np.array_equal(got["DataInMask"].cpu().numpy(), want["DataInMask"])
    assert np.array_equal(got["StlAbovePlane"].cpu().numpy(), want["StlAbovePlane"])
    assert float(np.abs(got["Ddata"].cpu().numpy() - want["Ddata"]).max()) <= 1e-6
    assert float(np.abs(got["Dstl"].cpu().numpy() - want["Dstl"]).max()) <= 1e-6
    assert 0 < got["nData"] and 0 < got["nStl"] < len(s["stl"])
    for k in ("nStl", "nData", "MedStl", "MedData"):
        assert got[k] == want[k], k
    for k in ("MeanStl", "MeanData", "VarStl", "VarData"):
        assert abs(got[k] - want[k]) <= 1e-9 * abs(want[k]), k


def _mat_bytes(variables):
    """a level-5 MAT file of full double / logical arrays (what the ground truth's ObsMask*.mat and Plane*.mat hold)"""
    def el(typ, payload):
        return struct.pack("<II", typ, len(payload)) + payload + b"\0" * ((-len(payload)) % 8)

    out = b"MATLAB 5.0 MAT-file, written by a test".ljust(116) + b"\0" * 8 + struct.pack("<H", 0x0100) + b"IM"
    for name, a in variables.items():
        a = np.atleast_2d(a)
        logical = a.dtype == bool
        flags = struct.pack("<II", (9 | 0x200) if logical else 6, 0)             # mxUINT8_CLASS + logical, mxDOUBLE_CLASS
        data = np.asfortranarray(a.astype(np.uint8 if logical else np.float64)).tobytes(order="F")
        body = (el(6, flags) + el(5, struct.pack("<%di" % a.ndim, *a.shape)) + el(1, name.encode())
                + el(2 if logical else 9, data))
        out += el(14, body)
    return out


def _ply_mesh_bytes(verts, faces):
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(verts), len(faces))).encode()
    rec = np.empty(len(faces), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    rec["n"], rec["i"] = 3, faces
    return head + np.ascontiguousarray(verts, dtype="<f4").tobytes() + rec.tobytes()


def _read_coloured_ply(path):
    with open(path, "rb") as f:
        data = f.read()
    head, body = data.split(b"end_header\n", 1)
    n = int(head.split(b"element vertex ")[1].split(b"\n")[0])
    rec = np.frombuffer(body, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")], count=n)
    assert len(body) == rec.itemsize * n
    return np.stack([rec["x"], rec["y"], rec["z"]], 1), np.stack([rec["r"], rec["g"], rec["b"]], 1)


def test_cli_surfaces_end_to_end_with_error_clouds(tmp_path):
    _lib.load()
    scans = {3: synthetic.dtu_eval_mesh(nx=60, ny=40, edge=0.4, n_stl=6000, res=2.0, seed=3),
             7: synthetic.dtu_eval_mesh(nx=45, ny=50, edge=0.35, n_stl=5000, res=2.0, seed=7, offset=3.0)}
    gt = tmp_path / "MVS_Data"
    os.makedirs(gt / "Points" / "stl")
    os.makedirs(gt / "ObsMask")
    plydir = tmp_path / "meshes"
    os.makedirs(plydir)
    for scan, s in scans.items():
        (plydir / f"tola{scan:03d}_l3_surf_11_trim_8.ply").write_bytes(_ply_mesh_bytes(s["verts"], s["faces"]))
        head = f"ply\nformat binary_little_endian 1.0\nelement vertex {len(s['stl'])}\nproperty float x\nproperty float y\nproperty float z\nend_header\n"
        (gt / "Points" / "stl" / f"stl{scan:03d}_total.ply").write_bytes(head.encode() + s["stl"].astype("<f4").tobytes())
        (gt / "ObsMask" / f"ObsMask{scan}_10.mat").write_bytes(_mat_bytes({"ObsMask": s["obs_mask"], "BB": s["bb"], "Res": np.array([[s["res"]]])}))
        (gt / "ObsMask" / f"Plane{scan}.mat").write_bytes(_mat_bytes({"P": s["plane"].reshape(4, 1)}))
    clouds = tmp_path / "clouds"
    env = dict(os.environ, PYTHONPATH=REPO)
    p = subprocess.run([sys.executable, "-m", "rc_mvsnet_amd.dtu_eval", "--plydir", str(plydir), "--gtpath", str(gt), "--scans", "3,7",
                        "--surfaces", "--pattern", "tola{scan:03d}_l3_surf_11_trim_8.ply", "--error-clouds", str(clouds), "--method", "tola"],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 3 and lines[-1]["summary"] and [ln["scan"] for ln in lines[:2]] == [3, 7]
    for line in lines[:2]:
        assert set(line) == {"scan", *dtu_eval.STAT_FIELDS}
        s = scans[line["scan"]]
        want = dtu_eval.evaluate_mesh(_t(s["verts"]), _t(s["faces"], np.int32), _t(s["stl"]), torch.from_numpy(s["obs_mask"]), s["bb"],
                                      s["res"], s["plane"], per_point=True)
        for k in dtu_eval.STAT_FIELDS:
            assert line[k] == want[k], k
        xyz, rgb = _read_coloured_ply(clouds / f"tola2Stl_{line['scan']}.ply")
        assert len(xyz) == len(want["Qdata"]) and np.array_equal(xyz, want["Qdata"].cpu().numpy())
        assert np.array_equal(rgb, dtu_eval.error_colours(want["Ddata"], want["DataInMask"]).cpu().numpy())
        xyz, rgb = _read_coloured_ply(clouds / f"Stl2tola_{line['scan']}.ply")
        assert len(xyz) == len(s["stl"]) and np.array_equal(xyz, s["stl"])
        assert np.array_equal(rgb, dtu_eval.error_colours(want["Dstl"], want["StlAbovePlane"]).cpu().numpy())
    want = dtu_eval.summarize(lines[:2])
    assert all(abs(lines[-1][k] - want[k]) <= 1e-12 for k in ("acc", "comp", "overall"))
    d = torch.tensor([0.0, 5.0, 10.0, 12.5, 20.0], dtype=torch.float64, device=DEV)
    on = dtu_eval.error_colours(d, torch.ones(5, dtype=torch.bool, device=DEV))
    off = dtu_eval.error_colours(d, torch.zeros(5, dtype=torch.bool, device=DEV))
    assert on.is_cuda and on.cpu().tolist() == [[255, 255, 255], [255, 128, 128], [255, 0, 0], [255, 0, 0], [255, 0, 0]]
    assert off.cpu().tolist() == [[0, 0, 255], [0, 128, 128], [0, 255, 0], [0, 255, 0], [0, 255, 0]]


def test_more_than_2_31_points_is_refused_before_allocating():
    _lib.load()
    v = np.array([[0, 0, 0], [1000, 0, 0], [0, 1000, 0], [1000, 1000, 0], [0, 0, 1000]], dtype=np.float32)
    f = np.array([[0, 1, 2], [1, 3, 2], [0, 1, 4]], dtype=np.int32)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    for dst in (0.02, 1e-9):                # about 3.7e9 samples in 3 x 5e4 rows; rows alone past 2^31
        with pytest.raises(_lib.RcmvsError, match="2\\^31"):
            dtu_eval.sample_mesh(_t(v), _t(f, np.int32), dst)
    assert torch.cuda.max_memory_allocated() - base < 16 << 20
