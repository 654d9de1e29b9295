"""The cases and checks of the undistortion kernel (csrc/undistort.hip through colmap_import.undistort_image), shared by
tests/test_gpu_undistort.py (device "cuda:0") and tests/test_undistort_emu_cpu.py (the CPU emulation, device "cpu"): the same
images and cameras, against tests/undistort_oracle.py.  Every check is exact: bytes equal in every byte, blank count equal, two
runs identical -- the kernel and the oracle do the same correctly rounded fp64 operations in the same order."""
import functools
import io
import os

import numpy as np
import torch

import undistort_oracle as O
from rc_mvsnet_amd import colmap_import as CI, colmap_io, scan_io, synthetic

# (33, 47): 1551 pixels, no multiple of the four pixels a thread owns; (64, 96): six blocks; (1, 7), (5, 1), (2, 2): one row, one
# column, fewer pixels than one thread's group
SIZES = ((2, 2), (1, 7), (5, 1), (33, 47), (64, 96))


def image(h, w):
    return np.random.default_rng(1000 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


def camera(h, w, cx=None, cy=None):
    """two focal lengths, the principal point a little off the centre and off the pixel grid"""
    return (1.2 * w, 1.212 * w, 0.5 * w + 0.3 if cx is None else cx, 0.5 * h - 0.2 if cy is None else cy)


def d8(k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0, k4=0.0, k5=0.0, k6=0.0):
    return (k1, k2, p1, p2, k3, k4, k5, k6)


def one_focal(h, w):
    c = camera(h, w)
    return (c[0], c[0], c[2], c[3])


OPENCV = d8(-0.15, 0.03, 0.004, -0.003)
# name -> (h, w) -> (camera, the 8 coefficients, focal_scale)
PARAMS = {
    "simple_radial_barrel": lambda h, w: (one_focal(h, w), d8(-0.12), 1.0),
    "simple_radial_pincushion": lambda h, w: (one_focal(h, w), d8(0.15), 1.0),
    "radial_barrel": lambda h, w: (one_focal(h, w), d8(-0.2, 0.05), 1.0),
    "radial_pincushion": lambda h, w: (one_focal(h, w), d8(0.1, 0.05), 1.0),
    "opencv_barrel": lambda h, w: (camera(h, w), OPENCV, 1.0),                                   # tangential terms (+, -)
    "opencv_pincushion": lambda h, w: (camera(h, w), d8(0.12, 0.02, -0.005, 0.006), 1.0),        # tangential terms (-, +)
    "full_opencv_barrel": lambda h, w: (camera(h, w), d8(-0.15, 0.03, 0.004, -0.003, 0.01, 0.02, -0.01, 0.005), 1.0),
    "full_opencv_pincushion": lambda h, w: (camera(h, w), d8(0.2, 0.04, -0.004, 0.003, -0.01, -0.05, 0.01, -0.002), 1.0),
    "focal_scale_0.8": lambda h, w: (camera(h, w), OPENCV, 0.8),
    "focal_scale_1.3": lambda h, w: (camera(h, w), OPENCV, 1.3),
    "principal_point_off_centre": lambda h, w: (camera(h, w, 0.3 * w, 0.7 * h), OPENCV, 1.0),
    "principal_point_outside": lambda h, w: (camera(h, w, -0.4 * w, 1.3 * h), OPENCV, 1.0),
    "pincushion_blank_border": lambda h, w: (camera(h, w), d8(3.0), 1.0),
    # fx = fy = 8 and the principal point on a pixel centre make x = i / 8, y = j / 8 and r2 = (i^2 + j^2) / 64 exact, so the
    # denominator 1 + r2 k4 is exactly 0 at the pixels with i^2 + j^2 = 1 and changes sign beyond: 1 / 0 = inf there ...
    "denominator_zero_inf": lambda h, w: ((8.0, 8.0, 0.5, 0.5), d8(k1=0.1, k4=-64.0), 1.0),
    # ... and 0 / 0 = NaN with the numerator vanishing at the same radius
    "denominator_zero_nan": lambda h, w: ((8.0, 8.0, 0.5, 0.5), d8(k1=-64.0, k4=-64.0), 1.0),
    # the axis pixel (x = y = 0 exactly) keeps its position; everything else lands some 1e26 pixels away
    "coefficients_1e30": lambda h, w: ((1.2 * w, 1.212 * w, w // 2 + 0.5, h // 2 + 0.5), d8(1e30, 1e30, 1e30, 1e30, 1e30), 1.0),
    # 2 p1 and 2 p2 overflow to inf and the radial polynomial does off the axis; inf * 0 = NaN on the axis' row and column, the axis
    # pixel included: every pixel is blank, through inf or through NaN
    "coefficients_overflow": lambda h, w: ((1.2 * w, 1.212 * w, w // 2 + 0.5, h // 2 + 0.5), d8(1.7e308, 1.7e308, 1.7e308, 1.7e308, 1.7e308), 1.0),
}


@functools.lru_cache(maxsize=None)
def reference(h, w, name):
    """the oracle's answer, computed once per case and shared: (out, blank, us, vs); the arrays are read-only"""
    cam, dist, scale = PARAMS[name](h, w)
    out, blank = O.undistort(image(h, w), cam, dist, scale)
    us, vs = O.positions(h, w, cam[0], cam[1], cam[2], cam[3], scale * cam[0], scale * cam[1], dist)
    for a in (out, us, vs):
        a.setflags(write=False)
    return out, blank, us, vs


def run(dev, img, cam, dist, scale=1.0):
    out, blank = CI.undistort_image(torch.from_numpy(img).to(dev), cam, dist, scale)
    assert out.dtype == torch.uint8 and tuple(out.shape) == img.shape and type(blank) is int
    return out.cpu().numpy(), blank


def check_case(dev, name, sizes=SIZES):
    for h, w in sizes:
        cam, dist, scale = PARAMS[name](h, w)
        img = image(h, w)
        want, want_blank, us, vs = reference(h, w, name)
        # what the case is there for, on the oracle alone
        if name == "pincushion_blank_border" and h * w > 7:
            assert 0.2 * h * w < want_blank < h * w
        if name.startswith("denominator_zero"):
            bad = ~np.isfinite(us) | ~np.isfinite(vs)
            assert bad.any() and (np.isnan(us).any() if name.endswith("nan") else (np.isinf(us) | np.isinf(vs)).any())
            assert (want[bad] == 0).all() and want_blank >= bad.sum()
        if name == "coefficients_1e30":
            assert want_blank == h * w - 1 and np.isfinite(us).all()
        if name == "coefficients_overflow":
            assert want_blank == h * w and np.isnan(us).any() and (h * w < 8 or np.isinf(us).any())
        got, blank = run(dev, img, cam, dist, scale)
        differ = int((got != want).sum())
        print(f"{name} {h}x{w}: {differ} bytes differ, blank {blank} (oracle {want_blank}) of {h * w}")
        assert differ == 0 and blank == want_blank
        again, blank2 = run(dev, img, cam, dist, scale)
        assert np.array_equal(again, got) and blank2 == blank                      # two runs: the same bytes


def check_identity(dev):
    """all coefficients zero, scale 1: the known answer is the input itself"""
    for h, w in SIZES:
        img = image(h, w)
        for cam in (camera(h, w), camera(h, w, -0.4 * w, 1.3 * h), (0.7 * w, 3.1 * w, 0.25 * w, 0.5 * h)):
            got, blank = run(dev, img, cam, d8(), 1.0)
            assert np.array_equal(got, img) and blank == 0, (h, w, cam)


def check_full_size(dev):
    """1080 x 1920 OPENCV: the flat-index arithmetic at real size (2025 blocks), a blank border included"""
    h, w = 1080, 1920
    img = np.random.default_rng(5).integers(0, 256, (h, w, 3), dtype=np.uint8)
    cam, dist = (1.1 * w, 1.09 * w, 0.5 * w - 7.3, 0.5 * h + 4.6), d8(0.09, 0.02, 0.001, -0.0015)
    want, want_blank = O.undistort(img, cam, dist, 1.0)
    assert 0 < want_blank < 0.2 * h * w
    got, blank = run(dev, img, cam, dist, 1.0)
    differ = int((got != want).sum())
    print(f"full size {h}x{w}: {differ} bytes differ, blank {blank} (oracle {want_blank})")
    assert differ == 0 and blank == want_blank


# ---- the import, end to end -------------------------------------------------------------------------------------------
K1 = -0.12


def two_camera_model():
    """four 32 x 64 images: three with SIMPLE_RADIAL camera 3 (k = K1), view_001 with camera 4, the same but k = 0"""
    model = synthetic.colmap_model(n_images=4, n_points=200, hw=(32, 64), seed=3, camera_model="SIMPLE_RADIAL", distortion=[K1])
    cam = model["cameras"][0]
    model["cameras"] = [cam, dict(cam, id=4, params=cam["params"][:3] + [0.0])]
    model["images"] = [dict(im, camera_id=4) if im["name"] == "view_001.jpg" else im for im in model["images"]]
    return model


def jpeg_bytes(rgb):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", quality=95)
    return buf.getvalue()


def check_end_to_end(dev, tmp_path, binary=False):
    from PIL import Image
    from rc_mvsnet_amd.mvs_dataset import MVSDataset
    model = two_camera_model()
    sparse, photos = str(tmp_path / "sparse"), str(tmp_path / "photos")
    synthetic.write_colmap_model(model, sparse, binary=binary)
    synthetic.write_colmap_images(model, photos)
    M = colmap_io.read_model(sparse, distortion=True)
    assert M["models"] == ["SIMPLE_RADIAL"] * 4 and M["distortion"][:, 0].tolist() == [K1, 0.0, K1, K1] and not M["distortion"][:, 1:].any()
    K = M["intrinsics"]
    plain = None
    for scale in (1.0, 0.9):
        out = str(tmp_path / ("test%g" % scale) / "scene")
        summary = CI.import_scene(sparse, photos, out, max_d=32, num_src=2, device=dev, undistort=True, focal_scale=scale)
        assert summary["images"] == 4 and summary["focal_scale"] == scale and summary["undistorted"] == (3 if scale == 1.0 else 4)
        fractions = []
        for k in range(4):
            Kw, _ = scan_io.read_camera_parameters(os.path.join(out, "cams", "%08d_cam.txt" % k))
            want_K = K[k].copy()
            want_K[0, 0], want_K[1, 1] = scale * K[k, 0, 0], scale * K[k, 1, 1]
            assert np.array_equal(Kw, want_K.astype(np.float32))                  # the scaled pinhole camera, no half-pixel shift
            src, dst = os.path.join(photos, M["names"][k]), os.path.join(out, "images", "%08d.jpg" % k)
            with open(src, "rb") as f:
                src_bytes = f.read()
            with open(dst, "rb") as f:
                dst_bytes = f.read()
            with Image.open(dst) as im:
                assert im.format == "JPEG" and im.size == (64, 32)
            if scale == 1.0 and k == 1:
                assert dst_bytes == src_bytes                                      # zero coefficients, scale 1: the copy route
                continue
            with Image.open(src) as im:
                rgb = np.array(im.convert("RGB"), dtype=np.uint8)
            want, blank = O.undistort(rgb, (K[k, 0, 0], K[k, 1, 1], K[k, 0, 2], K[k, 1, 2]), M["distortion"][k], scale)
            assert dst_bytes == jpeg_bytes(want) and dst_bytes != src_bytes
            fractions.append(blank / (32 * 64))
        assert summary["blank_fraction_max"] == max(fractions)
        if scale == 1.0:
            plain = summary
        else:                                                                      # a wider view of a barrel lens: blank corners
            assert summary["blank_fraction_max"] > 0
            assert {k: v for k, v in summary.items() if k not in ("scene", "undistorted", "focal_scale", "blank_fraction_max")} == \
                   {k: v for k, v in plain.items() if k not in ("scene", "undistorted", "focal_scale", "blank_fraction_max")}
        ds = MVSDataset(str(tmp_path / ("test%g" % scale)), ["scene"], mode="test", nviews=3, max_h=32, max_w=64, device=dev)
        assert len(ds) == summary["refs"] and tuple(ds[0]["imgs"].shape) == (3, 3, 32, 64)
    return plain
