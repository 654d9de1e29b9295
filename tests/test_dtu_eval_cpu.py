"""CPU: the DTU scorer's readers (PLY, MAT v5), the fp64 oracle's own semantics (tests/dtu_oracle.py) and the scorer's refusal
to run without a GPU."""
import io
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import dtu_oracle as O
from rc_mvsnet_amd import _lib, dtu_eval, dtu_io, fusion, synthetic


def _write(tmp_path, name, data):
    p = os.path.join(str(tmp_path), name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def _ply(fmt, xyz, extra_before=True, faces=0, vertex_first=True, xyz_type="float"):
    """a PLY with a colour property before x, a 'confidence' double after z, an optional element before the vertices and faces after"""
    n = len(xyz)
    end = {"binary_little_endian": "<", "binary_big_endian": ">"}.get(fmt)
    head = ["ply", f"format {fmt} 1.0", "comment made by a test"]
    pre = []
    if not vertex_first:
        head += ["element camera 2", "property float k", "property list uchar int ids"]
        pre = [(1.5, [1, 2, 3]), (2.5, [])]
    head += [f"element vertex {n}", "property uchar red", f"property {xyz_type} x", f"property {xyz_type} y", f"property {xyz_type} z",
             "property double confidence"]
    face_rows = [[0, 1, 2]] * faces
    if faces:
        head += [f"element face {faces}", "property list uchar int vertex_indices"]
    head += ["end_header"]
    out = io.BytesIO()
    out.write(("\n".join(head) + "\n").encode())
    npt = {"float": "f4", "double": "f8", "int": "i4"}[xyz_type]
    if fmt == "ascii":
        for k, ids in pre:
            out.write((f"{k} {len(ids)} " + " ".join(map(str, ids)) + "\n").encode())
        for i, p in enumerate(xyz):
            out.write(f"{i % 256} {repr(float(p[0]))} {repr(float(p[1]))} {repr(float(p[2]))} 0.5\n".encode())
        for r in face_rows:
            out.write(("3 " + " ".join(map(str, r)) + "\n").encode())
    else:
        for k, ids in pre:
            out.write(struct.pack(end + "fB", k, len(ids)) + struct.pack(end + "%di" % len(ids), *ids))
        rec = np.empty(n, dtype=[("red", "u1"), ("x", end + npt), ("y", end + npt), ("z", end + npt), ("confidence", end + "f8")])
        rec["red"] = np.arange(n) % 256
        for a, k in enumerate("xyz"):
            rec[k] = xyz[:, a]
        rec["confidence"] = 0.5
        out.write(rec.tobytes())
        for r in face_rows:
            out.write(struct.pack(end + "B3i", 3, *r))
    return out.getvalue()


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
@pytest.mark.parametrize("faces,vertex_first", [(0, True), (4, True), (3, False)])
def test_ply_reader_round_trips(tmp_path, fmt, faces, vertex_first):
    xyz = np.random.default_rng(0).normal(0, 100, (37, 3)).astype(np.float32)
    got = dtu_io.read_ply_xyz(_write(tmp_path, "a.ply", _ply(fmt, xyz, faces=faces, vertex_first=vertex_first)))
    assert got.dtype == np.float32 and got.shape == (37, 3)
    assert np.array_equal(got, xyz)


@pytest.mark.parametrize("xyz_type", ["double", "int"])
def test_ply_reader_other_scalar_types(tmp_path, xyz_type):
    xyz = np.random.default_rng(1).integers(-500, 500, (11, 3)).astype(np.float32)
    got = dtu_io.read_ply_xyz(_write(tmp_path, "b.ply", _ply("binary_big_endian", xyz, xyz_type=xyz_type)))
    assert np.array_equal(got, xyz)


def test_ply_reader_reads_ply_bytes_output(tmp_path):
    xyz = np.random.default_rng(2).normal(0, 50, (101, 3)).astype(np.float32)
    rgb = np.random.default_rng(3).integers(0, 255, (101, 3)).astype(np.uint8)
    assert np.array_equal(dtu_io.read_ply_xyz(_write(tmp_path, "c.ply", fusion.ply_bytes(xyz, rgb))), xyz)


def test_ply_reader_rejects_bad_files(tmp_path):
    with pytest.raises(dtu_io.FormatError):
        dtu_io.read_ply_xyz(_write(tmp_path, "d.ply", b"not a ply\n"))
    with pytest.raises(dtu_io.FormatError):
        dtu_io.read_ply_xyz(_write(tmp_path, "e.ply", b"ply\nformat ascii 1.0\nelement face 0\nend_header\n"))


@pytest.mark.parametrize("compress", [False, True])
def test_mat_reader_against_scipy(tmp_path, compress):
    sio = pytest.importorskip("scipy.io")
    rng = np.random.default_rng(4)
    vars_ = {"ObsMask": rng.random((7, 5, 3)) > 0.5, "BB": rng.normal(0, 100, (2, 3)), "Res": np.array([[0.25]]),
             "P": rng.normal(0, 1, (4, 1)), "I16": rng.integers(-3000, 3000, (3, 4)).astype(np.int16),
             "F32": rng.random((1, 6)).astype(np.float32), "U8": rng.integers(0, 255, (2, 2, 2)).astype(np.uint8),
             "name": "skipped text", "cell": np.array([[1.0, 2.0]], dtype=object)}
    p = os.path.join(str(tmp_path), "m.mat")
    sio.savemat(p, vars_, do_compression=compress)
    got = dtu_io.read_mat(p)
    want = sio.loadmat(p)
    for k in ("ObsMask", "BB", "Res", "P", "I16", "F32", "U8"):
        assert got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k].astype(bool) if k == "ObsMask" else want[k]), k
    assert got["ObsMask"].dtype == bool
    assert "name" not in got and "cell" not in got


def test_mat_reader_refuses_v73(tmp_path):
    head = b"MATLAB 7.3 MAT-file, Platform: GLNXA64, Created on: Mon Jan  1 00:00:00 2024 HDF5 schema 1.00 .".ljust(116) + b"\0" * 8 + b"\x00\x02IM"
    p = _write(tmp_path, "v73.mat", head + b"\0" * 384 + b"\x89HDF\r\n\x1a\n" + b"\0" * 64)
    with pytest.raises(dtu_io.FormatError, match="7.3"):
        dtu_io.read_mat(p)


def test_mat_reader_hand_written_small_elements(tmp_path):
    """A level-5 file written by hand: a compressed 4x1 double (P) and an uncompressed 1x1 double (Res) whose name and value
    use the small-element form."""
    def el(typ, payload):
        pad = (-len(payload)) % 8
        return struct.pack("<II", typ, len(payload)) + payload + b"\0" * pad

    def small(typ, payload):
        return struct.pack("<HH", typ, len(payload)) + payload.ljust(4, b"\0")

    def matrix(name, values, dims):
        body = el(6, struct.pack("<II", 6, 0)) + el(5, struct.pack("<%di" % len(dims), *dims)) + small(1, name.encode())
        raw = struct.pack("<%dd" % len(values), *values)
        body += el(9, raw)
        return el(14, body)

    hdr = b"MATLAB 5.0 MAT-file, written by a test".ljust(116) + b"\0" * 8 + struct.pack("<H", 0x0100) + b"IM"
    P = [0.1, -0.2, 0.3, 4.0]
    mp = matrix("P", P, [4, 1])
    data = hdr + struct.pack("<II", 15, len(zlib.compress(mp))) + zlib.compress(mp) + matrix("Res", [0.5], [1, 1])
    got = dtu_io.read_mat(_write(tmp_path, "h.mat", data))
    assert np.array_equal(got["P"].ravel(), P) and got["Res"].shape == (1, 1) and got["Res"][0, 0] == 0.5


def test_oracle_greedy_equals_matlab_chunked_loop():
    rng = np.random.default_rng(5)
    pts = np.concatenate([rng.random((300, 3)) * 3.0, rng.normal(1.0, 0.05, (100, 3)), np.repeat(rng.random((5, 3)), 4, axis=0)]).astype(np.float32)
    order = rng.permutation(len(pts))
    nbrs = O.neighbours(pts, 0.2)
    keep = O.greedy_reduce(pts, order, 0.2, nbrs)
    for chunk in (7, 100, len(pts) - 1):
        assert np.array_equal(O.matlab_chunked_reduce(pts, order, 0.2, chunk, nbrs), keep)
    k = pts[keep].astype(np.float64)
    d = np.sqrt(O._d2(k, k)) + np.eye(len(k)) * 1e9
    assert d.min() > 0.2                                         # kept points are pairwise farther than dst
    rank = np.empty(len(pts), dtype=int)
    rank[order] = np.arange(len(pts))
    for i in np.nonzero(~keep)[0]:                               # a removed point has an earlier kept one within dst
        assert any(keep[j] and rank[j] < rank[i] for j in nbrs[i])


def test_oracle_matlab_round_half_away():
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999999999999994, -0.49999999999999994, 2.4999999999999996, 3.0, -3.0])
    assert np.array_equal(O.matlab_round(x), [1, 2, 3, -1, -2, -3, 0, -0, 2, 3, -3])
    assert not np.array_equal(np.round(x[:6]), O.matlab_round(x[:6]))      # numpy rounds half to even


def test_oracle_statistics():
    n, mean, var, med = O.stats([4.0, 1.0, 3.0, 2.0])
    assert (n, mean, med) == (4, 2.5, 2.5) and abs(var - 5.0 / 3.0) < 1e-15
    assert float(torch.median(torch.tensor([4.0, 1.0, 3.0, 2.0], dtype=torch.float64))) == 2.0     # the lower middle: not MATLAB's
    assert O.stats([7.0])[1:] == (7.0, 0.0, 7.0)
    n, mean, var, med = O.stats([])
    assert n == 0 and np.isnan(mean) and np.isnan(var) and np.isnan(med)
    assert dtu_eval.summarize([{"MeanData": 1.0, "MeanStl": 2.0}, {"MeanData": 3.0, "MeanStl": 4.0}]) == {"acc": 2.0, "comp": 3.0, "overall": 2.5}


def test_oracle_lattice_and_nearest():
    lo, hi = O.lattice([[0, 0, 0], [119.0, 60.0, 10.0]])
    assert list(lo) == [0, 0, 0] and list(hi) == [120.0, 120.0, 60.0]
    q = np.array([[0, 0, 0], [1, 1, 1], [-1e-3, 0, 0], [5, 5, 120.0]], dtype=np.float32)
    d = O.nearest(q, np.array([[0, 0, 1]], dtype=np.float32), 60.0, (lo, hi))
    assert list(d) == [1.0, np.sqrt(2.0), 60.0, 60.0]
    assert list(O.nearest(q, np.zeros((0, 3), np.float32), 20.0)) == [20.0] * 4


def test_scorer_refuses_cpu_tensors():
    s = synthetic.dtu_eval_scan(n_stl=200, n_data=300, extent=40.0)
    data, stl = torch.from_numpy(s["data"]), torch.from_numpy(s["stl"])
    with pytest.raises(_lib.RcmvsError):
        dtu_eval.reduce_points(data)
    with pytest.raises(_lib.RcmvsError):
        dtu_eval.nearest_distances(data, stl)
    with pytest.raises(_lib.RcmvsError):
        dtu_eval.evaluate_scan(data, stl, torch.from_numpy(s["obs_mask"]), s["bb"], s["res"], s["plane"])


def test_cell_edge_bounds_the_grid():
    h, dims = dtu_eval.cell_edge([0, 0, 0], [600.0, 600.0, 600.0], 0.2, 1 << 24)
    assert np.prod(dims) <= 1 << 24 and 2.3 < h < 2.5
    h, dims = dtu_eval.cell_edge([0, 0, 0], [1e5, 0.0, 0.0], 0.2, 4096)
    assert np.prod(dims) <= 4096 and h >= 1e5 / 4096
    h, dims = dtu_eval.cell_edge([1, 1, 1], [1, 1, 1], 0.202, 64)
    assert h == 0.202 and dims == [1, 1, 1]


def test_golden_mat_fixtures_match_their_generator():
    """tests/golden/dtu_eval/*.mat (written by make_dtu_eval_fixtures.py through scipy) read back by the in-package reader."""
    import sys
    from conftest import REPO
    here = os.path.join(REPO, "tests", "golden", "dtu_eval")
    sys.path.insert(0, here)
    try:
        import make_dtu_eval_fixtures as mk
    finally:
        sys.path.remove(here)
    for k, s in mk.scans().items():
        m = dtu_io.read_mat(os.path.join(here, f"ObsMask{k}_10.mat"))
        assert m["ObsMask"].dtype == bool and np.array_equal(m["ObsMask"], s["obs_mask"])
        assert np.array_equal(m["BB"], s["bb"]) and float(m["Res"].ravel()[0]) == s["res"]
        assert np.array_equal(dtu_io.read_mat(os.path.join(here, f"Plane{k}.mat"))["P"].ravel(), s["plane"])
