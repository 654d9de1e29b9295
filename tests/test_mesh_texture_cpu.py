"""Host logic of the mesh texturing that needs no kernel: the header's table, the oracle's own known answers, the PLY with texcoords
through every reader, the OBJ writer, the texture coordinates, the options, and host refusals with the argument named and nothing
written."""
import os

import numpy as np
import pytest
import torch

import mesh_texture_cases as MTC
import mesh_texture_oracle as O
from rc_mvsnet_amd import _lib, dtu_io, mesh_texture as MT, tsdf_mesh as TM


def test_the_header_declares_every_entry_point_with_a_timed_twin():
    assert any(p.endswith("mesh_texture.h") for p in _lib.EXT_HEADERS) and _lib.CONSTANTS["RCMVS_VERSION"] == 106
    names = sorted(k for k in _lib.EXT_SIGNATURES if k.startswith("rcmvs_mt_"))
    assert names == sorted("rcmvs_mt_" + n + t for n in ("vote", "layout", "fill", "shade") for t in ("", "_timed"))
    for name in names[::2]:
        plain, timed = _lib.EXT_SIGNATURES[name], _lib.EXT_SIGNATURES[name + "_timed"]
        assert timed[:len(plain) - 1] == plain[:-1] and len(timed) == len(plain) + 3        # phase, ev0, ev1 before the stream
    assert (MT.MIN_CLASS, MT.MAX_CLASS, MT.MAX_SHIFT, MT.MAX_ATLAS, MT.STATS, MT.TABLE) == (2, 10, 8, 16384, 24, 48)
    assert (O.MIN_CLASS, O.MAX_CLASS, O.MAX_SHIFT) == (MT.MIN_CLASS, MT.MAX_CLASS, MT.MAX_SHIFT) and O.STAT_NAMES == MT.STAT_NAMES


def test_morton_runs_from_aligned_bases_are_squares():
    assert [O.morton_xy(m) for m in range(8)] == [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (3, 0), (2, 1), (3, 1)]
    for k, base in ((2, 0), (2, 48), (3, 64), (5, 3 * 4 ** 5)):
        pts = {O.morton_xy(base + i) for i in range(4 ** k)}
        ox, oy = O.morton_xy(base)
        assert ox % 2 ** k == 0 and oy % 2 ** k == 0 and pts == {(ox + i, oy + j) for i in range(2 ** k) for j in range(2 ** k)}


def test_size_classes_at_their_thresholds():
    for shift in (0, 1, 8):
        for k in range(2, 11):
            side = (2 ** k - 3) * 256 * 2 ** shift
            assert O.size_class(side * side, shift) == (k, False)
            assert O.size_class(side * side + 1, shift) == ((k + 1, False) if k < 10 else (10, True))
    assert O.size_class(0, 0) == (2, False)


@pytest.mark.parametrize("seed", range(6))
def test_the_oracles_layout_on_random_classes(seed):
    rng = np.random.default_rng(seed)
    klass = rng.choice([0, 2, 2, 2, 3, 3, 4, 5, 6], size=int(rng.integers(0, 300))).tolist()
    order, table, texel = O.layout(klass)
    assert sorted(order) == list(range(len(klass)))
    keys = [(klass[f] == 0, -klass[f], f) for f in order]
    assert keys == sorted(keys)                                   # descending class, a class in face order, invalid last
    total = sum((table["classes"][k]["faces"] + 1) // 2 * 4 ** k for k in table["classes"])
    assert table["total"] == total and 4 ** table["m"] >= total and (table["m"] == 0 or 4 ** (table["m"] - 1) < total)
    for k, row in table["classes"].items():
        assert row["base"] % 4 ** k == 0 and row["faces"] == klass.count(k)
    owner = np.full((table["Sy"], table["S"]), -1, np.int32)
    for f, k in enumerate(klass):                                  # paint each face's half cell from its corners alone: no texel twice
        if k == 0:
            continue
        s = 1 << k
        (ax, ay), (bx, _), _ = texel[f].tolist()
        sign = 1 if bx > ax else -1
        for i in range(s):
            for j in range(s - 1 - i if sign > 0 else s - i):
                assert owner[ay + sign * j, ax + sign * i] == -1
                owner[ay + sign * j, ax + sign * i] = f
    stats = {"faces_seen": 0, "faces_unseen": len(klass) - klass.count(0), "faces_invalid": klass.count(0), "texels_image": 0,
             "texels_vertex": int((owner >= 0).sum()), "texels_fallback": 0, "faces_per_class": {k: klass.count(k) for k in range(2, 11)}}
    MTC.check_invariants(None, {"klass": np.array(klass, np.int32), "texel": texel, "owner": owner, "table": table, "stats": stats}, f"seed {seed}")


@pytest.mark.parametrize("name", ["one_face", "three_faces_missing_partner", "hidden_everywhere", "thresholds_shift_0", "width_1", "hostile_coordinates"])
def test_the_oracles_results_hold_the_known_answers(name):
    MTC.check_invariants(MTC.case(name), MTC.reference(name), name)
    if name in MTC.EXPECTED_VIEWS:
        assert MTC.reference(name)["views"] == MTC.EXPECTED_VIEWS[name]


def test_texcoords_put_texel_centres_in_the_unit_square_with_v_up():
    texel = np.array([[(0, 0), (13, 0), (0, 13)], [(15, 15), (2, 15), (15, 2)]], np.int32)
    uv = MT.texcoords(torch.from_numpy(texel), 16, 8)
    assert uv.dtype == np.float32 and uv.shape == (2, 3, 2)
    assert uv[0, 0].tolist() == [0.5 / 16, 1 - 0.5 / 8] and uv[0, 1].tolist() == [13.5 / 16, 1 - 0.5 / 8] and uv[1, 2].tolist() == [15.5 / 16, 1 - 2.5 / 8]
    # exact at the largest atlas: (x + 0.5) / 2^14 has 15 significant bits
    big = np.array([[(16383, 16383), (0, 1), (8191, 8192)]], np.int32)
    uv = MT.texcoords(big, 16384, 16384).astype(np.float64)
    assert np.array_equal(np.rint(uv[..., 0] * 16384 - 0.5), big[..., 0]) and np.array_equal(np.rint((1 - uv[..., 1]) * 16384 - 0.5), big[..., 1])
    assert np.array_equal(uv[..., 0] * 32768, 2.0 * big[..., 0] + 1)


def _mesh(nv=7, nf=9, seed=0):
    rng = np.random.default_rng(seed)
    verts = rng.standard_normal((nv, 3)).astype(np.float32)
    faces = np.stack([rng.permutation(nv)[:3] for _ in range(nf)]).astype(np.int32) if nf else np.zeros((0, 3), np.int32)
    return verts, faces, rng.integers(0, 256, (nv, 3), dtype=np.uint8), rng.random((nf, 3, 2), dtype=np.float32)


def test_ply_without_the_options_is_byte_for_byte_what_it_was():
    v, f, c, _ = _mesh()
    head = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n"
            f"property uchar green\nproperty uchar blue\nelement face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n").encode()
    body = b"".join(v[i].astype("<f4").tobytes() + c[i].tobytes() for i in range(len(v))) + b"".join(b"\x03" + f[i].astype("<i4").tobytes() for i in range(len(f)))
    assert TM.mesh_ply_bytes(v, f, c) == head + body == TM.mesh_ply_bytes(v, f, c, texcoords=None, texture_file=None)


@pytest.mark.parametrize("with_normals", [False, True])
def test_textured_ply_reads_back_in_every_bit(tmp_path, with_normals):
    v, f, c, uv = _mesh()
    uv = uv.copy()
    uv.view(np.uint32)[0, 0, 0] = 0x7FC01234                      # a NaN with a payload, a negative zero, a denormal: the bits are kept
    uv[0, 0, 1], uv[0, 1, 0] = -0.0, 1e-42
    normals = np.random.default_rng(1).standard_normal(v.shape).astype(np.float32) if with_normals else None
    data = TM.mesh_ply_bytes(v, f, c, normals=normals, texcoords=uv, texture_file="atlas_0.png")
    head = data[:data.index(b"end_header\n")].decode()
    assert "comment TextureFile atlas_0.png\n" in head and head.count("property list") == 2
    assert head.index("property list uchar int vertex_indices") < head.index("property list uchar float texcoord") and ("property float nx" in head) == with_normals
    path = tmp_path / "t.ply"
    path.write_bytes(data)
    rv, rf, rc, rn, ruv, name = dtu_io.read_ply_mesh_texture(str(path))
    assert name == "atlas_0.png" and np.array_equal(rv.view(np.uint32), v.view(np.uint32)) and np.array_equal(rf, f) and np.array_equal(rc, c)
    assert ruv.dtype == np.float32 and np.array_equal(ruv.view(np.uint32), uv.view(np.uint32))
    assert (rn is None) if not with_normals else np.array_equal(rn.view(np.uint32), normals.view(np.uint32))
    # the older readers go on reading vertices, faces, colours and normals of such a file
    for got in (dtu_io.read_ply_mesh(str(path)), dtu_io.read_ply_mesh_rgb(str(path)), dtu_io.read_ply_mesh_normals(str(path))):
        assert np.array_equal(got[0].view(np.uint32), v.view(np.uint32)) and np.array_equal(got[1], f) and got[1].dtype == np.int32
    assert np.array_equal(dtu_io.read_ply_mesh_rgb(str(path))[2], c)
    assert np.array_equal(dtu_io.read_ply_xyz(str(path)).view(np.uint32), v.view(np.uint32))


def test_textured_ply_of_an_empty_mesh_and_plain_files(tmp_path):
    e = tmp_path / "empty.ply"
    e.write_bytes(TM.mesh_ply_bytes(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), None, texcoords=np.zeros((0, 3, 2), np.float32), texture_file="e.png"))
    v, f, c, n, uv, name = dtu_io.read_ply_mesh_texture(str(e))
    assert v.shape == (0, 3) and f.shape == (0, 3) and uv.shape == (0, 3, 2) and name == "e.png"
    p = tmp_path / "plain.ply"
    mv, mf, mc, _ = _mesh()
    p.write_bytes(TM.mesh_ply_bytes(mv, mf, mc))
    v, f, c, n, uv, name = dtu_io.read_ply_mesh_texture(str(p))
    assert np.array_equal(f, mf) and uv is None and name is None and n is None


def test_faces_with_lists_of_varying_length_are_still_read(tmp_path):
    """a face element whose second list differs from face to face (no texcoords on some faces): the readers take the slow path"""
    v, f, c, uv = _mesh(nf=4)
    head = (f"ply\nformat binary_little_endian 1.0\ncomment TextureFile x.png\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
            f"element face {len(f)}\nproperty list uchar int vertex_indices\nproperty list uchar float texcoord\nend_header\n").encode()
    body = v.astype("<f4").tobytes()
    for i in range(len(f)):
        body += b"\x03" + f[i].astype("<i4").tobytes() + (b"\x06" + uv[i].astype("<f4").tobytes() if i % 2 == 0 else b"\x00")
    path = tmp_path / "ragged.ply"
    path.write_bytes(head + body)
    rv, rf = dtu_io.read_ply_mesh(str(path))
    assert np.array_equal(rf, f) and np.array_equal(rv, v)
    assert dtu_io.read_ply_mesh_texture(str(path))[4] is None
    # big-endian, texcoords first: the readers find the index list by its name
    head = head.replace(b"little", b"big").replace(b"property list uchar int vertex_indices\nproperty list uchar float texcoord\n",
                                                  b"property list uchar float texcoord\nproperty list uchar int vertex_indices\n")
    body = v.astype(">f4").tobytes() + b"".join(b"\x06" + uv[i].astype(">f4").tobytes() + b"\x03" + f[i].astype(">i4").tobytes() for i in range(len(f)))
    path.write_bytes(head + body)
    rv, rf = dtu_io.read_ply_mesh(str(path))
    got = dtu_io.read_ply_mesh_texture(str(path))
    assert np.array_equal(rf, f) and np.array_equal(rv, v) and np.array_equal(got[4].view(np.uint32), uv.view(np.uint32)) and got[5] == "x.png"


def test_quads_with_texcoords_are_refused_as_quads_without(tmp_path):
    v, f, c, uv = _mesh(nf=3)
    head = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
            f"element face {len(f)}\nproperty list uchar int vertex_indices\nproperty list uchar float texcoord\nend_header\n").encode()
    body = v.astype("<f4").tobytes() + b"".join(b"\x04" + np.append(f[i], 0).astype("<i4").tobytes() + b"\x08" + np.zeros(8, "<f4").tobytes() for i in range(len(f)))
    path = tmp_path / "quads.ply"
    path.write_bytes(head + body)
    with pytest.raises(dtu_io.FormatError, match="face 0 has 4 vertices"):
        dtu_io.read_ply_mesh(str(path))


def test_mesh_ply_bytes_refuses_bad_texcoords():
    v, f, c, uv = _mesh()
    for kw, pattern in (({"texcoords": uv[:-1], "texture_file": "a.png"}, r"texcoords must be \(9,3,2\) float32"),
                        ({"texcoords": uv.astype(np.float64), "texture_file": "a.png"}, "texcoords must be"),
                        ({"texcoords": uv.reshape(-1, 6), "texture_file": "a.png"}, "texcoords must be"),
                        ({"texcoords": uv}, "texture_file = None"), ({"texcoords": uv, "texture_file": "a b.png"}, "texture_file = 'a b.png'"),
                        ({"texcoords": uv, "texture_file": ""}, "texture_file = ''"), ({"texture_file": "a.png"}, "texture_file without texcoords")):
        with pytest.raises(_lib.RcmvsError, match=pattern):
            TM.mesh_ply_bytes(v, f, c, **kw)


def test_obj_writer_and_its_refusal(tmp_path):
    v, f, c, uv = _mesh()
    path = tmp_path / "deep" / "m.obj"
    MT.write_obj(str(path), torch.from_numpy(v), torch.from_numpy(f), uv, "m.png")
    MTC.check_obj(str(path), len(v), len(f), uv)
    rows = [line.split() for line in path.read_text().splitlines() if line.startswith("v ")]
    assert np.array_equal(np.array([[float(x) for x in r[1:]] for r in rows], np.float32), v)          # %.9g round-trips a float32
    with pytest.raises(_lib.RcmvsError, match="26 texture coordinates for 9 faces"):
        MT.write_obj(str(tmp_path / "bad" / "n.obj"), v, f, uv.reshape(-1, 2)[:-1], "n.png")
    assert not os.path.exists(tmp_path / "bad")


def test_options():
    assert MT.texture_options() is None and MT.texture_options(False, 4096) is None
    assert MT.texture_options(True) == {"max_size": 8192, "shift": 0} and MT.texture_options(True, 2048) == {"max_size": 2048, "shift": 0}
    for bad in (0, 16385, -1, 2.5, True):
        with pytest.raises(_lib.RcmvsError, match="max_size"):
            MT.texture_options(True, bad)
    assert TM._texture_argument(False, None) == {} and TM._texture_argument(True, 1024) == {"texture": {"max_size": 1024, "shift": 0}}


def test_host_refusals_name_the_argument_before_any_kernel_runs(tmp_path):
    """these are raised by the Python layer alone: no library is loaded for them"""
    s = MTC.case("one_face")
    tv, tf, tc = (torch.from_numpy(np.array(s[k])) for k in ("verts", "faces", "rgb"))
    img = torch.from_numpy(np.array(s["images"]))
    for kw, pattern in (({"max_size": 0}, "max_size = 0"), ({"shift": 9}, r"shift = 9 \(0 .. 8\)"), ({"chunk": 0}, "chunk = 0"), ({"near": -1.0}, "near = -1.0"),
                        ({"background": (1, 2)}, "background"), ({"max_size": "big"}, "max_size = 'big'")):
        with pytest.raises(_lib.RcmvsError, match=pattern):
            MT.texture(tv, tf, tc, img, s["cams"], **kw)
    with pytest.raises(_lib.RcmvsError, match="images must be"):
        MT.texture(tv, tf, tc, img.float(), s["cams"])
    with pytest.raises(_lib.RcmvsError, match="1 images of .* for 2 cameras"):
        MT.texture(tv, tf, tc, img, np.concatenate([s["cams"], s["cams"]]))
    plain = tmp_path / "plain.ply"
    plain.write_bytes(TM.mesh_ply_bytes(s["verts"], s["faces"], s["rgb"]))
    with pytest.raises(_lib.RcmvsError, match="no texcoords"):
        MT.read_textured(str(plain), "cpu")
