"""The host side of the COLMAP import (rc_mvsnet_amd/colmap_io.py, the file writers of colmap_import.py) and the oracle's known
answers (tests/colmap_oracle.py).  No GPU."""
import math
import os
import struct

import numpy as np
import pytest

import colmap_oracle as O
from rc_mvsnet_amd import colmap_import as CI, colmap_io, scan_io, synthetic
from rc_mvsnet_amd._lib import RcmvsError


@pytest.fixture(scope="module")
def model():
    return synthetic.colmap_model(n_images=5, n_points=120, hw=(48, 64), seed=1)


@pytest.fixture
def text_dir(model, tmp_path):
    synthetic.write_colmap_model(model, str(tmp_path))
    return tmp_path


def rewrite(path, fn):
    with open(path) as f:
        text = f.read()
    with open(path, "w") as f:
        f.write(fn(text))


# ---- readers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera_model", ["PINHOLE", "SIMPLE_PINHOLE"])
def test_text_and_binary_read_to_identical_arrays(tmp_path, camera_model):
    model = synthetic.colmap_model(n_images=5, n_points=120, hw=(48, 64), seed=1, camera_model=camera_model)
    synthetic.write_colmap_model(model, str(tmp_path / "txt"))
    synthetic.write_colmap_model(model, str(tmp_path / "bin"), binary=True)
    a, b = colmap_io.read_model(str(tmp_path / "txt")), colmap_io.read_model(str(tmp_path / "bin"))
    for k in a:
        if k == "files":
            continue
        if k == "names":
            assert a[k] == b[k]
        else:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    truth = model["truth"]
    assert a["image_ids"].tolist() == [10, 12, 14, 16, 18] and a["names"] == ["view_%03d.jpg" % k for k in range(5)]
    assert np.array_equal(a["point_ids"], 5 + 3 * np.arange(120))
    assert a["offsets"].dtype == np.int64 and a["ids"].dtype == np.int32
    assert np.array_equal(a["offsets"], truth["offsets"]) and np.array_equal(a["ids"], truth["ids"])      # ascending, the duplicate dropped
    assert np.array_equal(a["points"], truth["points"]) and np.array_equal(a["intrinsics"], truth["intrinsics"])
    assert np.abs(a["extrinsics"] - truth["extrinsics"]).max() < 1e-14 and np.abs(a["centres"] - truth["centres"]).max() < 1e-14
    assert a["sizes"].tolist() == [[64, 48]] * 5
    if camera_model == "SIMPLE_PINHOLE":
        assert (a["intrinsics"][:, 0, 0] == a["intrinsics"][:, 1, 1]).all()


def test_text_wins_over_binary(model, tmp_path):
    synthetic.write_colmap_model(model, str(tmp_path), binary=True)
    synthetic.write_colmap_model(model, str(tmp_path))
    os.truncate(str(tmp_path / "images.bin"), 40)
    assert colmap_io.read_model(str(tmp_path))["files"]["images"].endswith("images.txt")
    os.remove(str(tmp_path / "images.txt"))
    with pytest.raises(RcmvsError, match=r"images\.bin.*truncated"):
        colmap_io.read_model(str(tmp_path))


def test_image_without_points_has_an_empty_line(text_dir):
    def drop(text):
        lines = text.split("\n")
        first = next(i for i, ln in enumerate(lines) if not ln.startswith("#"))
        lines[first + 1] = ""
        return "\n".join(lines)
    rewrite(str(text_dir / "images.txt"), drop)
    M = colmap_io.read_model(str(text_dir))
    assert (np.diff(M["offsets"]) == 0).sum() == 1 and len(M["image_ids"]) == 5


TEXT_FAULTS = {
    "cameras.txt: malformed": ("cameras.txt", lambda t: t.replace(" PINHOLE 64 ", " PINHOLE sixty-four "), r"cameras\.txt: line 3"),
    "cameras.txt: parameter count": ("cameras.txt", lambda t: t.rstrip("\n").rsplit(" ", 1)[0] + "\n", r"cameras\.txt: line 3 \(camera 3\): PINHOLE takes 4"),
    "cameras.txt: non-finite": ("cameras.txt", lambda t: t.replace(" 32.0 ", " nan "), r"cameras\.txt: line 3 \(camera 3\): non-finite"),
    "images.txt: truncated": ("images.txt", lambda t: "\n".join(t.split("\n")[:4]) + "\n", r"images\.txt: line 4 \(image \d+\): the file is truncated"),
    "images.txt: malformed header": ("images.txt", lambda t: t.replace(" 3 view_", " three view_", 1), r"images\.txt: line 4: expected"),
    "images.txt: point triples": ("images.txt", lambda t: "\n".join(ln + " 1.5" if i == 4 else ln for i, ln in enumerate(t.split("\n"))),
                                  r"images\.txt: line 4 \(image \d+\): the 2-D points"),
    "images.txt: non-finite": ("images.txt", lambda t: "\n".join(" ".join(["inf" if j == 5 else w for j, w in enumerate(ln.split(" "))]) if i == 3 else ln
                                                               for i, ln in enumerate(t.split("\n"))), r"images\.txt: line 4 \(image \d+\): non-finite"),
    "images.txt: unknown camera": ("images.txt", lambda t: t.replace(" 3 view_", " 9 view_", 1), r"images\.txt: image \d+ \(view_00\d\.jpg\): unknown camera id 9"),
    "points3D.txt: malformed": ("points3D.txt", lambda t: "\n".join(ln.rsplit(" ", 1)[0] if i == 2 else ln for i, ln in enumerate(t.split("\n"))),
                                r"points3D\.txt: line 3: expected"),
    "points3D.txt: non-finite": ("points3D.txt", lambda t: "\n".join(" ".join(["nan" if j == 2 else w for j, w in enumerate(ln.split(" "))]) if i == 2 else ln
                                                                   for i, ln in enumerate(t.split("\n"))), r"points3D\.txt: line 3 \(point \d+\): non-finite"),
    "unknown point": ("points3D.txt", lambda t: "\n".join(ln for i, ln in enumerate(t.split("\n")) if i != 2),
                      r"images\.txt: image \d+ \(view_00\d\.jpg\): observation of unknown point \d+"),
}


@pytest.mark.parametrize("fault", list(TEXT_FAULTS))
def test_malformed_text_raises_with_the_file_named(text_dir, fault):
    name, fn, pattern = TEXT_FAULTS[fault]
    rewrite(str(text_dir / name), fn)
    with pytest.raises(RcmvsError, match=pattern):
        colmap_io.read_model(str(text_dir))


@pytest.mark.parametrize("name,cut,pattern", [("cameras.bin", 30, r"cameras\.bin: camera record 0: the file is truncated"),
                                              ("images.bin", 100, r"images\.bin: image record 0.*truncated"),
                                              ("points3D.bin", 6000, r"points3D\.bin: point record \d+.*truncated"),
                                              ("points3D.bin", 4, r"points3D\.bin: point count: the file is truncated")])
def test_truncated_binary_raises_with_the_file_named(model, tmp_path, name, cut, pattern):
    synthetic.write_colmap_model(model, str(tmp_path), binary=True)
    os.truncate(str(tmp_path / name), cut)
    with pytest.raises(RcmvsError, match=pattern):
        colmap_io.read_model(str(tmp_path))


def test_binary_faults_non_finite_trailing_bytes_unknown_camera(model, tmp_path):
    synthetic.write_colmap_model(model, str(tmp_path), binary=True)
    path = str(tmp_path / "points3D.bin")
    with open(path, "rb") as f:
        buf = bytearray(f.read())
    struct.pack_into("<d", buf, 8 + 8 + 8, float("nan"))                        # y of the first record
    with open(path, "wb") as f:
        f.write(buf)
    with pytest.raises(RcmvsError, match=r"points3D\.bin: point record 0 \(point \d+\): non-finite"):
        colmap_io.read_model(str(tmp_path))
    synthetic.write_colmap_model(model, str(tmp_path), binary=True)
    with open(str(tmp_path / "cameras.bin"), "ab") as f:
        f.write(b"\0\0")
    with pytest.raises(RcmvsError, match=r"cameras\.bin: 2 bytes after the last record"):
        colmap_io.read_model(str(tmp_path))
    other = dict(model, cameras=[dict(model["cameras"][0], id=4)])
    synthetic.write_colmap_model(other, str(tmp_path), binary=True)
    with pytest.raises(RcmvsError, match=r"images\.bin: image 10 \(view_000\.jpg\): unknown camera id 3"):
        colmap_io.read_model(str(tmp_path))


@pytest.mark.parametrize("binary", [False, True])
def test_opencv_camera_raises(model, tmp_path, binary):
    other = dict(model, cameras=[dict(model["cameras"][0], model="OPENCV", params=[70.0, 70.0, 32.0, 24.0, 0.1, 0.0, 0.0, 0.0])])
    synthetic.write_colmap_model(other, str(tmp_path), binary=binary)
    with pytest.raises(RcmvsError, match=r"cameras\.(txt|bin).*OPENCV.*undistorted first"):
        colmap_io.read_model(str(tmp_path))


def test_missing_file_is_named(tmp_path):
    with pytest.raises(RcmvsError, match="neither cameras.txt nor cameras.bin"):
        colmap_io.read_model(str(tmp_path))


# ---- known answers ----------------------------------------------------------------------------------------------------
def one_point_score(angle_deg, **kw):
    a = math.radians(angle_deg)
    centres = np.array([[2.0, 0.0, 0.0], [2.0 * math.cos(a), 2.0 * math.sin(a), 0.0]])
    points = np.zeros((1, 3))
    S, K = O.pair_scores(centres, points, np.array([0, 1, 2]), np.array([0, 0], dtype=np.int32), **kw)
    assert K[0, 1] == 1
    return S[0, 1]


def test_score_known_answers():
    assert abs(one_point_score(5.0) - 1.0) <= 1e-15
    assert abs(one_point_score(90.0) - math.exp(-85.0 ** 2 / 200.0)) <= 1e-15
    assert abs(one_point_score(3.0) - math.exp(-4.0 / 2.0)) <= 1e-13            # below theta0: sigma1
    assert abs(one_point_score(25.0, theta0=10.0, sigma1=2.0, sigma2=5.0) - math.exp(-225.0 / 50.0)) <= 1e-13
    centres, points = np.array([[2.0, 0.0, 0.0], [0.0, 2.0, 0.0]]), np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    S, K = O.pair_scores(centres, points, np.array([0, 1, 2]), np.array([0, 1], dtype=np.int32))      # disjoint lists
    assert S[0, 1] == 0 and K[0, 1] == 0 and (S == S.T).all() and (np.diag(S) == 0).all()
    on_centre = O.angle_deg(centres[0], centres[1], centres[:1])
    assert on_centre[0] == 0.0                                                  # atan2(0, 0)


def test_oracle_ordering_and_ties():
    S = np.array([[0.0, 2.0, 2.0, 0.0, 3.0], [2.0, 0.0, 0.0, 0.0, 0.0], [2.0, 0.0, 0.0, 0.0, 0.0], [0.0] * 5, [3.0, 0.0, 0.0, 0.0, 0.0]])
    lists, counts = O.top_views(S, 2)
    assert lists == [[4, 1], [0], [0], [], [0]] and counts.tolist() == [3, 1, 1, 0, 1]


def test_quaternion_and_centre_hand_case():
    s = math.sqrt(0.5)
    R = colmap_io.qvec_to_rotmat([s, 0.0, 0.0, s])                              # 90 degrees about z
    assert np.allclose(R, [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], atol=1e-15)
    assert np.allclose(R, O.quat_to_rotmat([s, 0.0, 0.0, s]), atol=1e-15)
    assert np.allclose(colmap_io.qvec_to_rotmat([2.0, 0.0, 0.0, 0.0]), np.eye(3))      # normalised
    C = colmap_io.camera_centre(R, [1.0, 2.0, 3.0])                             # -R^T t
    assert np.allclose(C, [-2.0, 1.0, -3.0], atol=1e-15)
    assert np.allclose(R @ C + [1.0, 2.0, 3.0], 0.0, atol=1e-15)
    rng = np.random.default_rng(0)
    for _ in range(5):
        q = rng.normal(size=4)
        R = colmap_io.qvec_to_rotmat(q)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-14) and abs(np.linalg.det(R) - 1.0) < 1e-14
        back = synthetic._rotmat_to_qvec(R)
        assert np.allclose(back, q / np.linalg.norm(q) * (1 if q[0] >= 0 else -1), atol=1e-14)
    cam = {"model": "SIMPLE_PINHOLE", "params": np.array([70.0, 31.5, 23.5])}
    assert colmap_io.intrinsic_matrix(cam).tolist() == [[70.0, 0.0, 31.5], [0.0, 70.0, 23.5], [0.0, 0.0, 1.0]]      # no half-pixel shift
    cam = {"model": "PINHOLE", "params": np.array([70.0, 71.0, 31.5, 23.5])}
    assert colmap_io.intrinsic_matrix(cam).tolist() == [[70.0, 0.0, 31.5], [0.0, 71.0, 23.5], [0.0, 0.0, 1.0]]


def test_ranks():
    for c in (2, 99, 100, 101, 257, 5000, 123457):
        assert CI.rank_pair(c) == (int(c * 0.01), int(c * 0.99)) == O.ranks(c)
    assert CI.rank_pair(2) == (0, 1) and CI.rank_pair(100) == (1, 99) and CI.rank_pair(5000) == (50, 4950)


# ---- writers ----------------------------------------------------------------------------------------------------------
def test_cam_and_pair_files_round_trip_through_scan_io(tmp_path):
    rng = np.random.default_rng(3)
    cam = np.zeros((2, 4, 4))
    cam[0] = synthetic._similarity(rng.normal(size=3), 33.0, 1.0, rng.normal(size=3))
    cam[1, :3, :3] = [[1234.5678, 0.0, 511.25], [0.0, 1233.4321, 383.75], [0.0, 0.0, 1.0]]
    dmin, dmax, max_d = 1.2345678901234, 9.87654321, 192
    cam[1, 3] = (dmin, (dmax - dmin) / (max_d - 1) / 1.0, max_d, dmax)
    path = str(tmp_path / "00000000_cam.txt")
    scan_io.write_cam(path, cam)
    K, E = scan_io.read_camera_parameters(path)
    assert np.array_equal(E, cam[0].astype(np.float32)) and np.array_equal(K, cam[1, :3, :3].astype(np.float32))
    K4, E4, d0, interval = scan_io.read_cam_file(path, 1.0, 192)
    assert d0 == dmin and np.array_equal(E4, E) and np.array_equal(K4[:2], K[:2] / 4.0)
    assert interval == (dmin + 192 * cam[1, 3, 1] - dmin) / 192
    with open(path) as f:
        tail = [float(v) for v in f.read().split("\n")[11].split()]
    assert tail == [dmin, cam[1, 3, 1], 192.0, dmax]
    pair = str(tmp_path / "pair.txt")
    lists = [(0, [(2, 3.25), (1, 0.1 + 0.2)]), (2, [(0, 3.25)])]                # image 1 has no partner: no entry
    CI.write_pair_file(pair, lists)
    assert scan_io.read_pair_file(pair) == [(0, [2, 1]), (2, [0])]
    with open(pair) as f:
        lines = f.read().split("\n")
    assert lines[0] == "2" and lines[2].split() == ["2", "2", "3.25", "1", repr(0.1 + 0.2)]


def test_image_copy_jpeg_bytes_png_conversion_and_size_check(tmp_path):
    from PIL import Image
    ys, xs = np.meshgrid(np.arange(24), np.arange(32), indexing="ij")
    img = np.stack([4 * xs + 60, 6 * ys + 40, 3 * xs + 3 * ys + 20], 2).astype(np.uint8)      # smooth: JPEG keeps it within a few levels
    Image.fromarray(img).save(str(tmp_path / "a.jpg"), quality=80)
    Image.fromarray(img).save(str(tmp_path / "b.png"))
    CI._copy_image(str(tmp_path / "a.jpg"), str(tmp_path / "0.jpg"), (32, 24))
    with open(str(tmp_path / "a.jpg"), "rb") as a, open(str(tmp_path / "0.jpg"), "rb") as b:
        assert a.read() == b.read()
    CI._copy_image(str(tmp_path / "b.png"), str(tmp_path / "1.jpg"), (32, 24))
    with Image.open(str(tmp_path / "1.jpg")) as im:
        assert im.format == "JPEG" and im.size == (32, 24)
        assert np.abs(np.asarray(im, dtype=np.int32) - img).mean() < 3           # quality 95 of a smooth image
    with pytest.raises(RcmvsError, match=r"a\.jpg: size 32 x 24 differs from its camera's 64 x 48"):
        CI._copy_image(str(tmp_path / "a.jpg"), str(tmp_path / "2.jpg"), (64, 48))
    with pytest.raises(RcmvsError, match=r"missing\.jpg"):
        CI._copy_image(str(tmp_path / "missing.jpg"), str(tmp_path / "3.jpg"), (32, 24))


def test_functions_have_no_cpu_fallback():
    import torch
    z = torch.zeros((2, 3), dtype=torch.float64)
    with pytest.raises(RcmvsError, match="GPU"):
        CI.pair_scores(z, z, torch.tensor([0, 1, 2]), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RcmvsError, match="ascending"):
        CI.pair_scores(z, z, torch.tensor([0, 2, 1]), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RcmvsError, match="RCMVS_VS_MAX_SRC"):
        CI.top_views(torch.zeros((3, 3), dtype=torch.float64), 33)
