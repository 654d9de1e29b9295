"""The host side of the undistorting COLMAP import: the oracle (tests/undistort_oracle.py) against an independent sampler, the
readers of rc_mvsnet_amd/colmap_io.py with ``distortion=True``, and the argument checks of colmap_import.py.  No GPU."""
import struct

import numpy as np
import pytest
import torch

import undistort_cases as C
import undistort_oracle as O
from rc_mvsnet_amd import colmap_import as CI, colmap_io, synthetic
from rc_mvsnet_amd._lib import RcmvsError

MODELS = ["SIMPLE_RADIAL", "RADIAL", "OPENCV", "FULL_OPENCV"]


# ---- the oracle -------------------------------------------------------------------------------------------------------
def forward_model(h, w, cam, dist, scale):
    """An independently written forward model (OpenCV's documented form, powers of r written out, no Horner scheme):
    -> the source position (u, v) of every output pixel centre, in COLMAP's convention (pixel centres at +0.5)"""
    fx, fy, cx, cy = cam
    k1, k2, p1, p2, k3, k4, k5, k6 = dist
    v, u = np.mgrid[0:h, 0:w].astype(np.float64) + 0.5
    x, y = (u - cx) / (scale * fx), (v - cy) / (scale * fy)
    r2 = x ** 2 + y ** 2
    r4, r6 = r2 ** 2, r2 ** 3
    radial = (1 + k1 * r2 + k2 * r4 + k3 * r6) / (1 + k4 * r2 + k5 * r4 + k6 * r6)
    xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x ** 2)
    yd = y * radial + p1 * (r2 + 2 * y ** 2) + 2 * p2 * x * y
    return fx * xd + cx, fy * yd + cy


@pytest.mark.parametrize("name", ["simple_radial_barrel", "radial_pincushion", "opencv_barrel", "opencv_pincushion", "full_opencv_barrel",
                                  "full_opencv_pincushion", "focal_scale_0.8", "focal_scale_1.3", "principal_point_off_centre",
                                  "principal_point_outside", "pincushion_blank_border"])
def test_oracle_against_an_independent_sampler(name):
    """Values before rounding within 1e-9 of scipy's linear interpolation at the independently computed positions, on the valid
    pixels whose position was not clamped: fp64 blends of values up to 255 with a handful of operations, and positions that
    agree to some 1e-13 pixels, so this is many orders above the rounding error; the blank masks agree away from the border."""
    from scipy.ndimage import map_coordinates
    h, w = 64, 96
    cam, dist, scale = C.PARAMS[name](h, w)
    img = C.image(h, w)
    out, blank, values, ok = O.undistort(img, cam, dist, scale, return_values=True)
    u, v = forward_model(h, w, cam, dist, scale)
    assert np.abs(np.stack(O.positions(h, w, *cam, scale * cam[0], scale * cam[1], dist)) - np.stack([u, v])).max() < 1e-9
    inside = (u >= 0) & (u < w) & (v >= 0) & (v < h)
    far = (np.abs(u) > 1e-6) & (np.abs(u - w) > 1e-6) & (np.abs(v) > 1e-6) & (np.abs(v - h) > 1e-6)
    assert np.array_equal(inside[far], ok[far]) and blank == int((~ok).sum())
    unclamped = ok & inside & (u - 0.5 >= 0) & (u - 0.5 <= w - 1) & (v - 0.5 >= 0) & (v - 0.5 <= h - 1)
    assert unclamped.sum() > 0.3 * h * w
    for c in range(3):
        ref = map_coordinates(img[..., c].astype(np.float64), [v - 0.5, u - 0.5], order=1, mode="nearest")
        assert np.abs(ref - values[..., c])[unclamped].max() <= 1e-9
    assert np.array_equal(out, np.floor(values + 0.5).astype(np.uint8)) and (out[~ok] == 0).all()


def test_oracle_known_answers():
    img = C.image(5, 7)
    out, blank = O.undistort(img, (6.0, 5.0, 3.2, 2.9), C.d8())
    assert np.array_equal(out, img) and blank == 0                                # identity
    # the footprint and the blend of two neighbours, rounded half up
    two = np.array([[[10, 20, 31], [11, 23, 40]]], dtype=np.uint8)
    us = np.array([[1.0, 1.25]])
    x0, x1, a = O.footprint(us, 2)
    assert x0.tolist() == [[0, 0]] and x1.tolist() == [[1, 1]] and a.tolist() == [[0.5, 0.75]]
    v = O.blend(two[0, 0].astype(float), two[0, 1].astype(float), two[0, 0].astype(float), two[0, 1].astype(float), 0.5, 0.3)
    assert (v + 0.5).astype(int).tolist() == [11, 22, 36]                        # 10.5 -> 11, 21.5 -> 22, 35.5 -> 36
    x0, x1, a = O.footprint(np.array([0.2, 1.9]), 2)                               # half a pixel at the border: the border pixel
    assert x0.tolist() == [0, 1] and x1.tolist() == [1, 1] and a.tolist() == [0.0, 0.0]
    nan, inf = float("nan"), float("inf")
    assert O.valid(np.array([nan, inf, -inf, 0.0, 2.0, 1.999]), np.array([0.5] * 6), 1, 2).tolist() == [False, False, False, True, False, True]


# ---- readers ----------------------------------------------------------------------------------------------------------
def model_of(camera_model, **kw):
    return synthetic.colmap_model(n_images=5, n_points=120, hw=(48, 64), seed=1, camera_model=camera_model, **kw)


@pytest.mark.parametrize("camera_model", MODELS)
def test_text_and_binary_read_to_identical_arrays_with_distortion(tmp_path, camera_model):
    model = model_of(camera_model)
    synthetic.write_colmap_model(model, str(tmp_path / "txt"))
    synthetic.write_colmap_model(model, str(tmp_path / "bin"), binary=True)
    a, b = colmap_io.read_model(str(tmp_path / "txt"), distortion=True), colmap_io.read_model(str(tmp_path / "bin"), distortion=True)
    assert set(a) == set(b) and {"distortion", "models"} <= set(a)
    for k in a:
        if k == "files":
            continue
        if k in ("names", "models"):
            assert a[k] == b[k]
        else:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    coeffs = synthetic.COLMAP_DISTORTION[camera_model]
    row = {"SIMPLE_RADIAL": coeffs + [0.0] * 7, "RADIAL": coeffs + [0.0] * 6, "OPENCV": coeffs + [0.0] * 4, "FULL_OPENCV": coeffs}[camera_model]
    assert a["distortion"].dtype == np.float64 and a["distortion"].shape == (5, 8) and a["distortion"].tolist() == [row] * 5
    assert a["models"] == [camera_model] * 5
    truth = model["truth"]
    assert np.array_equal(a["intrinsics"], truth["intrinsics"]) and a["sizes"].tolist() == [[64, 48]] * 5
    if camera_model in ("SIMPLE_RADIAL", "RADIAL"):
        assert (a["intrinsics"][:, 0, 0] == a["intrinsics"][:, 1, 1]).all()
    else:
        assert (a["intrinsics"][:, 0, 0] != a["intrinsics"][:, 1, 1]).all()


def test_full_opencv_parameter_order():
    cam = {"model": "FULL_OPENCV", "params": np.array([70.0, 71.0, 31.5, 23.5, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0])}
    assert colmap_io.distortion_row(cam).tolist() == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]      # k1 k2 p1 p2 k3 k4 k5 k6 as COLMAP lists them
    assert colmap_io.intrinsic_matrix(cam).tolist() == [[70.0, 0.0, 31.5], [0.0, 71.0, 23.5], [0.0, 0.0, 1.0]]
    cam = {"model": "RADIAL", "params": np.array([70.0, 31.5, 23.5, 0.1, 0.2])}
    assert colmap_io.distortion_row(cam).tolist() == [0.1, 0.2, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert colmap_io.intrinsic_matrix(cam).tolist() == [[70.0, 0.0, 31.5], [0.0, 70.0, 23.5], [0.0, 0.0, 1.0]]


def test_pinhole_models_read_with_distortion_as_zero_rows(tmp_path):
    synthetic.write_colmap_model(model_of("PINHOLE"), str(tmp_path))
    a, b = colmap_io.read_model(str(tmp_path)), colmap_io.read_model(str(tmp_path), distortion=True)
    assert "distortion" not in a and "models" not in a                             # the default result is unchanged
    assert not b["distortion"].any() and b["models"] == ["PINHOLE"] * 5
    assert all(np.array_equal(a[k], b[k]) for k in a if k not in ("files", "names"))


def rewrite(path, fn):
    with open(path) as f:
        text = f.read()
    with open(path, "w") as f:
        f.write(fn(text))


@pytest.mark.parametrize("camera_model,count", [("SIMPLE_RADIAL", 4), ("RADIAL", 5), ("OPENCV", 8), ("FULL_OPENCV", 12)])
def test_parameter_count_and_non_finite_faults_name_file_and_record(tmp_path, camera_model, count):
    model = model_of(camera_model)
    synthetic.write_colmap_model(model, str(tmp_path))
    path = str(tmp_path / "cameras.txt")
    rewrite(path, lambda t: t.rstrip("\n").rsplit(" ", 1)[0] + "\n")
    with pytest.raises(RcmvsError, match=r"cameras\.txt: line 3 \(camera 3\): %s takes %d parameters, found %d" % (camera_model, count, count - 1)):
        colmap_io.read_model(str(tmp_path), distortion=True)
    rewrite(path, lambda t: t.rstrip("\n") + " 0.5 0.25\n")
    with pytest.raises(RcmvsError, match=r"cameras\.txt: line 3 \(camera 3\): %s takes %d parameters, found %d" % (camera_model, count, count + 1)):
        colmap_io.read_model(str(tmp_path), distortion=True)
    synthetic.write_colmap_model(model, str(tmp_path))
    rewrite(path, lambda t: t.rstrip("\n").rsplit(" ", 1)[0] + " inf\n")
    with pytest.raises(RcmvsError, match=r"cameras\.txt: line 3 \(camera 3\): non-finite"):
        colmap_io.read_model(str(tmp_path), distortion=True)
    # binary: the count follows from the model id, so a short record is a truncated file; a NaN coefficient is named
    other = str(tmp_path / "bin")
    synthetic.write_colmap_model(model, other, binary=True)
    with open(other + "/cameras.bin", "rb") as f:
        buf = bytearray(f.read())
    assert len(buf) == 8 + 24 + 8 * count
    with open(other + "/cameras.bin", "wb") as f:
        f.write(buf[:-8])
    with pytest.raises(RcmvsError, match=r"cameras\.bin: camera record 0: the file is truncated"):
        colmap_io.read_model(other, distortion=True)
    struct.pack_into("<d", buf, len(buf) - 8, float("nan"))
    with open(other + "/cameras.bin", "wb") as f:
        f.write(buf)
    with pytest.raises(RcmvsError, match=r"cameras\.bin: camera record 0 \(camera 3\): non-finite"):
        colmap_io.read_model(other, distortion=True)


@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("distortion", [False, True])
def test_fisheye_is_refused_in_both_modes(tmp_path, binary, distortion):
    model = model_of("PINHOLE")
    other = dict(model, cameras=[dict(model["cameras"][0], model="OPENCV_FISHEYE", params=[70.0, 70.0, 32.0, 24.0, 0.1, 0.0, 0.0, 0.0])])
    synthetic.write_colmap_model(other, str(tmp_path), binary=binary)
    with pytest.raises(RcmvsError, match=r"cameras\.(txt|bin).*camera 3.*OPENCV_FISHEYE is not supported.*undistorted first"):
        colmap_io.read_model(str(tmp_path), distortion=distortion)


@pytest.mark.parametrize("name", ["FOV", "THIN_PRISM_FISHEYE", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE"])
def test_other_models_are_refused_with_distortion(tmp_path, name):
    with open(str(tmp_path / "cameras.txt"), "w") as f:
        f.write("1 %s 64 48 70.0 70.0 32.0 24.0 0.1\n" % name)
    with pytest.raises(RcmvsError, match=r"cameras\.txt: line 1 \(camera 1\): camera model %s is not supported" % name):
        colmap_io.read_cameras_text(str(tmp_path / "cameras.txt"), distortion=True)


@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("camera_model", MODELS)
def test_distorted_models_are_refused_without_the_keyword(tmp_path, camera_model, binary):
    synthetic.write_colmap_model(model_of(camera_model), str(tmp_path), binary=binary)
    with pytest.raises(RcmvsError, match=r"cameras\.(txt|bin).*%s.*undistorted first" % camera_model):
        colmap_io.read_model(str(tmp_path))
    with pytest.raises(RcmvsError, match=r"cameras\.(txt|bin).*%s.*undistorted first.*--undistort" % camera_model):
        colmap_io.read_model(str(tmp_path), distortion=False)
    with pytest.raises(RcmvsError, match=r"cameras\.(txt|bin).*%s.*undistorted first" % camera_model):
        CI.import_scene(str(tmp_path), "nowhere", str(tmp_path / "out"), device="cpu")      # raised by the reader, before any launch
    with pytest.raises(RcmvsError, match=r"cameras\.(txt|bin).*%s.*undistorted first" % camera_model):
        CI.import_scene(str(tmp_path), "nowhere", str(tmp_path / "out"), device="cpu", undistort=False)
    assert not (tmp_path / "out").exists()


def test_synthetic_models():
    with pytest.raises(ValueError, match="takes 4 distortion coefficients"):
        model_of("OPENCV", distortion=[0.1])
    with pytest.raises(ValueError, match="no distortion"):
        model_of("PINHOLE", distortion=[0.1])
    m = model_of("RADIAL", distortion=[0.25, -0.5])
    assert m["cameras"][0]["params"][3:] == [0.25, -0.5] and len(m["cameras"][0]["params"]) == 5
    a, b = model_of("PINHOLE"), model_of("OPENCV")                                 # the same scene and random stream behind every model
    assert a["cameras"][0]["params"] == b["cameras"][0]["params"][:4]
    assert [im["name"] for im in a["images"]] == [im["name"] for im in b["images"]] and np.array_equal(a["points"]["xyz"], b["points"]["xyz"])


# ---- colmap_import ----------------------------------------------------------------------------------------------------
def test_undistort_image_argument_errors_and_no_cpu_fallback():
    img = torch.zeros((4, 6, 3), dtype=torch.uint8)
    cam, dist = (5.0, 5.0, 3.0, 2.0), [0.0] * 8
    for bad in (torch.zeros((4, 6), dtype=torch.uint8), torch.zeros((4, 6, 4), dtype=torch.uint8), torch.zeros((0, 6, 3), dtype=torch.uint8),
                torch.zeros((3, 4, 6), dtype=torch.uint8)):
        with pytest.raises(RcmvsError, match=r"expected an \(H,W,3\) image"):
            CI.undistort_image(bad, cam, dist)
    with pytest.raises(RcmvsError, match="8 coefficients"):
        CI.undistort_image(img, cam, [0.0] * 4)
    with pytest.raises(RcmvsError, match="8 coefficients"):
        CI.undistort_image(img, cam[:3], dist)
    for c, d in (((0.0, 5.0, 3.0, 2.0), dist), ((5.0, -1.0, 3.0, 2.0), dist), ((5.0, 5.0, float("nan"), 2.0), dist),
                 (cam, [0.0] * 7 + [float("inf")]), (cam, [float("nan")] + [0.0] * 7)):
        with pytest.raises(RcmvsError, match="finite, focal lengths positive"):
            CI.undistort_image(img, c, d)
    for s in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RcmvsError, match="focal_scale"):
            CI.undistort_image(img, cam, dist, s)
    with pytest.raises(RcmvsError, match="GPU"):
        CI.undistort_image(img, cam, dist)                                        # a CPU tensor: there is no CPU fallback


def test_focal_scale_needs_undistort(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        CI.parse_args(["--model", "m", "--images", "i", "--out", "o", "--focal-scale", "0.9"])
    assert e.value.code == 2 and "--focal-scale needs --undistort" in capsys.readouterr().err
    args = CI.parse_args(["--model", "m", "--images", "i", "--out", "o"])
    assert args.undistort is False and args.focal_scale == 1.0
    args = CI.parse_args(["--model", "m", "--images", "i", "--out", "o", "--undistort", "--focal-scale", "0.9"])
    assert args.undistort is True and args.focal_scale == 0.9
    assert CI.parse_args(["--model", "m", "--images", "i", "--out", "o", "--undistort"]).focal_scale == 1.0
    with pytest.raises(RcmvsError, match="focal_scale 0.9.*undistort=True"):
        CI.import_scene(str(tmp_path), "nowhere", str(tmp_path / "out"), device="cpu", focal_scale=0.9)
    with pytest.raises(RcmvsError, match="focal_scale"):
        CI.import_scene(str(tmp_path), "nowhere", str(tmp_path / "out"), device="cpu", undistort=True, focal_scale=0.0)


def test_extension_header_declares_the_entry_point():
    from rc_mvsnet_amd import _lib
    import ctypes
    assert any(p.endswith("undistort.h") for p in _lib.EXT_HEADERS)
    sig = _lib.EXT_SIGNATURES["rcmvs_undistort_rgb8"]
    assert sig == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_double] * 6 + [ctypes.c_void_p] * 3
    assert "rcmvs_undistort_rgb8" not in _lib.SIGNATURES and _lib.CONSTANTS["RCMVS_VERSION"] == 106
