"""CPU: the mesh side of the DTU scorer -- dtu_io.read_ply_mesh (round trips, refusals), MeshSupSamp's known answers and
degenerate triangles on the literal oracle (tests/mesh_oracle.py) and its vectorised twin, and the command line's --pattern /
--surfaces handling."""
import io
import json
import os
import struct

import numpy as np
import pytest
import torch

import mesh_oracle as M
from rc_mvsnet_amd import _lib, dtu_eval, dtu_io

_NP = {"char": "i1", "uchar": "u1", "short": "i2", "ushort": "u2", "int": "i4", "uint": "u4", "float": "f4", "double": "f8"}


def _mesh_ply(fmt, verts, faces, count_t="uchar", index_t="int", index_name="vertex_indices", face_name="face", extra_list=False,
              with_faces=True):
    """a mesh PLY: vertex x y z float + a uchar 'quality'; faces with a leading float 'area', the index list, and optionally
    a trailing list property 'texnumbers'"""
    end = {"binary_little_endian": "<", "binary_big_endian": ">"}.get(fmt)
    head = ["ply", f"format {fmt} 1.0", "comment a test mesh", f"element vertex {len(verts)}", "property float x", "property float y",
            "property float z", "property uchar quality"]
    if with_faces:
        head += [f"element {face_name} {len(faces)}", "property float area", f"property list {count_t} {index_t} {index_name}"]
        if extra_list:
            head += ["property list uchar float texnumbers"]
    head += ["end_header"]
    out = io.BytesIO()
    out.write(("\n".join(head) + "\n").encode())
    extra = [[0.25 * k for k in range(i % 4)] for i in range(len(faces))]
    if fmt == "ascii":
        for i, p in enumerate(verts):
            out.write(f"{repr(float(p[0]))} {repr(float(p[1]))} {repr(float(p[2]))} {i % 7}\n".encode())
        if with_faces:
            for i, f in enumerate(faces):
                row = f"1.5 {len(f)} " + " ".join(str(int(x)) for x in f)
                if extra_list:
                    row += f" {len(extra[i])} " + " ".join(repr(x) for x in extra[i])
                out.write((row + "\n").encode())
    else:
        for i, p in enumerate(verts):
            out.write(struct.pack(end + "fffB", *[float(x) for x in p], i % 7))
        if with_faces:
            for i, f in enumerate(faces):
                out.write(struct.pack(end + "f", 1.5))
                out.write(np.array([len(f)], dtype=end + _NP[count_t]).tobytes() + np.array(f, dtype=end + _NP[index_t]).tobytes())
                if extra_list:
                    out.write(struct.pack(end + "B%df" % len(extra[i]), len(extra[i]), *extra[i]))
    return out.getvalue()


def _write(tmp_path, data, name="m.ply"):
    p = os.path.join(str(tmp_path), name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def _mesh(seed=0, n=40, m=70):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 30, (n, 3)).astype(np.float32), rng.integers(0, n, (m, 3)).astype(np.int32)


FORMATS = ["ascii", "binary_little_endian", "binary_big_endian"]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("count_t,index_t", [("uchar", "int"), ("int", "uint")])
def test_read_ply_mesh_round_trips(tmp_path, fmt, count_t, index_t):
    v, f = _mesh()
    gv, gf = dtu_io.read_ply_mesh(_write(tmp_path, _mesh_ply(fmt, v, f, count_t=count_t, index_t=index_t)))
    assert gv.dtype == np.float32 and gf.dtype == np.int32 and gf.shape == (70, 3)
    assert np.array_equal(gv, v) and np.array_equal(gf, f)


@pytest.mark.parametrize("fmt", FORMATS)
def test_read_ply_mesh_names_extra_lists_and_no_faces(tmp_path, fmt):
    v, f = _mesh(1)
    for kw in ({"index_name": "vertex_index"}, {"index_name": "indices", "face_name": "Tri"}, {"extra_list": True},
               {"extra_list": True, "index_t": "ushort", "count_t": "int"}):
        gv, gf = dtu_io.read_ply_mesh(_write(tmp_path, _mesh_ply(fmt, v, f, **kw)))
        assert np.array_equal(gv, v) and np.array_equal(gf, f), kw
    gv, gf = dtu_io.read_ply_mesh(_write(tmp_path, _mesh_ply(fmt, v, f, with_faces=False)))
    assert np.array_equal(gv, v) and gf.shape == (0, 3) and gf.dtype == np.int32
    gv, gf = dtu_io.read_ply_mesh(_write(tmp_path, _mesh_ply(fmt, v, f[:0])))
    assert gf.shape == (0, 3)


@pytest.mark.parametrize("fmt", FORMATS)
def test_read_ply_mesh_refusals(tmp_path, fmt):
    v, f = _mesh(2)
    quads = [list(r) for r in f[:5]] + [[0, 1, 2, 3]] + [list(r) for r in f[5:]]
    with pytest.raises(dtu_io.FormatError, match="face 5 has 4 vertices"):
        dtu_io.read_ply_mesh(_write(tmp_path, _mesh_ply(fmt, v, quads)))
    with pytest.raises(dtu_io.FormatError, match="vertices"):
        dtu_io.read_ply_mesh(_write(tmp_path, _mesh_ply(fmt, v, quads, extra_list=True)))
    for bad in (len(v), -1):
        g = f.copy()
        g[3, 1] = bad
        with pytest.raises(dtu_io.FormatError, match="outside"):
            dtu_io.read_ply_mesh(_write(tmp_path, _mesh_ply(fmt, v, g)))
    w = v.copy()
    w[7, 2] = np.nan
    with pytest.raises(dtu_io.FormatError, match="non-finite"):
        dtu_io.read_ply_mesh(_write(tmp_path, _mesh_ply(fmt, w, f)))
    with pytest.raises(dtu_io.FormatError, match="index list"):
        dtu_io.read_ply_mesh(_write(tmp_path, _mesh_ply(fmt, v, f, index_name="corners")))


def test_read_ply_mesh_reads_xyz_of_the_same_file(tmp_path):
    v, f = _mesh(3)
    p = _write(tmp_path, _mesh_ply("binary_little_endian", v, f, extra_list=True))
    assert np.array_equal(dtu_io.read_ply_xyz(p), dtu_io.read_ply_mesh(p)[0])


RIGHT = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]


@pytest.mark.parametrize("tri,dst,n", [(RIGHT, 0.2, 10), (RIGHT, 0.25, 6), (RIGHT, 0.1, 45),
                                       ([[0, 0, 0], [2, 0, 0], [0, 1, 0]], 0.2, 25),
                                       ([[0, 0, 0], [1, 0, 0], [0.5, 0.8660254037844386, 0]], 0.2, 6)])
def test_known_sample_counts(tri, dst, n):
    v = np.array(tri, dtype=np.float32)
    pts = M.literal(v, [[0, 1, 2]], dst)
    assert len(pts) == 3 + n
    assert np.array_equal(pts[:3], v.astype(np.float64))
    assert np.array_equal(M.vectorised(v, [[0, 1, 2]], dst), pts)


def test_diagonal_pairs_round_to_one_and_are_dropped():
    # at dst 0.2 the right triangle has n1 = n2 = 5: k = 0.1, 0.3, ..., 0.9 and k1 + k2 = 1 is not kept
    assert (1.5 / 5.0) + (3.5 / 5.0) == 1.0 and (0.5 / 5.0) + (4.5 / 5.0) == 1.0
    pts = M.literal(np.array(RIGHT, dtype=np.float32), [[0, 1, 2]], 0.2)[3:]
    assert np.all(pts[:, 0] + pts[:, 1] < 1.0)
    assert [tuple(np.round(p[:2], 12)) for p in pts[:4]] == [(0.1, 0.1), (0.1, 0.3), (0.1, 0.5), (0.1, 0.7)]


def test_degenerate_triangles_give_nothing():
    v = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [0.1, 0, 0], [0, 0.1, 0]], dtype=np.float32)
    for f in ([0, 1, 2], [0, 0, 1], [1, 1, 1], [0, 3, 4]):           # collinear, repeated vertex, one point, smaller than dst
        assert len(M.literal(v, [f], 0.2)) == len(v), f
        assert len(M.vectorised(v, [f], 0.2)) == len(v), f


def test_vectorised_oracle_equals_literal_on_random_meshes():
    rng = np.random.default_rng(7)
    for k in range(3):
        v = (rng.random((80, 3)) * [4, 3, 1]).astype(np.float32)
        f = rng.integers(0, 80, (150, 3))
        f[::11, 2] = f[::11, 0]
        want = M.literal(v, f, 0.15 + 0.05 * k)
        assert len(want) > 80
        for chunk in (5, 1000, 1 << 22):
            assert np.array_equal(M.vectorised(v, f, 0.15 + 0.05 * k, chunk=chunk), want)


def test_sample_mesh_refuses_cpu_tensors():
    v, f = _mesh(4)
    with pytest.raises(_lib.RcmvsError):
        dtu_eval.sample_mesh(torch.from_numpy(v), torch.from_numpy(f))


def test_error_colours_rule():
    d = torch.tensor([0.0, 5.0, 10.0, 20.0, 2.5], dtype=torch.float64)
    on = dtu_eval.error_colours(d, torch.ones(5, dtype=torch.bool)).tolist()
    off = dtu_eval.error_colours(d, torch.zeros(5, dtype=torch.bool)).tolist()
    assert on[:4] == [[255, 255, 255], [255, 128, 128], [255, 0, 0], [255, 0, 0]]
    assert off[:4] == [[0, 0, 255], [0, 128, 128], [0, 255, 0], [0, 255, 0]]
    assert on[4] == [255, 191, 191] and off[4] == [0, 64, 191]          # alpha 0.25: floor(255 * 0.75 + 0.5) = 191


def test_cli_pattern_and_surfaces_reach_the_evaluation(monkeypatch, capsys):
    seen = []

    def fake(plydir, gtpath, scan, **kw):
        seen.append((scan, kw))
        return dict(scan=scan, **{k: 1.0 for k in dtu_eval.STAT_FIELDS})

    monkeypatch.setattr(dtu_eval, "evaluate_files", fake)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(_lib, "load", lambda: None)
    dtu_eval.main(["--plydir", "P", "--gtpath", "G", "--scans", "1,24"])
    assert [s for s, _ in seen] == [1, 24]
    for _, kw in seen:                      # the default keeps the points mode as it was
        assert kw["pattern"] == "scan{scan}.ply" and kw["surfaces"] is False and kw["error_clouds"] is None
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines()]
    assert [ln.get("scan") for ln in lines] == [1, 24, None] and lines[-1]["summary"]
    seen.clear()
    dtu_eval.main(["--plydir", "P", "--gtpath", "G", "--scans", "9", "--surfaces", "--pattern", "tola{scan:03d}_l3_surf_11_trim_8.ply",
                   "--error-clouds", "E", "--method", "tola"])
    (scan, kw), = seen
    assert scan == 9 and kw["surfaces"] is True and kw["error_clouds"] == "E" and kw["method"] == "tola"
    assert dtu_eval.scan_paths("P", "G", 9, kw["pattern"])["data"] == os.path.join("P", "tola009_l3_surf_11_trim_8.ply")
    assert dtu_eval.scan_paths("P", "G", 9)["data"] == os.path.join("P", "scan9.ply")
    with pytest.raises(SystemExit):
        dtu_eval.main(["--plydir", "P", "--gtpath", "G", "--scans", "9", "--pattern", "scan{n}.ply"])
