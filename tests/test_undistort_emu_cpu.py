"""The undistortion kernel (csrc/undistort.hip) on the CPU emulation of tests/emu, driven through
rc_mvsnet_amd/colmap_import.py on CPU tensors: the cases of tests/test_gpu_undistort.py (tests/undistort_cases.py), bytes and
blank counts equal to tests/undistort_oracle.py.  The emulation runs blocks one after another, so this also pins that no result
depends on the blocks' order.  The C ABI's negative statuses are checked here too, on the emulated library."""
import ctypes

import numpy as np
import pytest
import torch

import undistort_cases as C
from rc_mvsnet_amd import _lib, colmap_import as CI, fusion


@pytest.fixture(autouse=True)
def emu_ci(emu, monkeypatch):
    _lib.bind(emu)                                               # the emu fixture binds the primary header's table; the extensions' too
    monkeypatch.setattr(CI, "_chk", fusion._chk)                 # routed by the emu fixture: CPU tensors, NULL stream
    monkeypatch.setattr(CI, "_stream", fusion._stream)
    return emu


@pytest.mark.parametrize("name", list(C.PARAMS))
def test_bytes_and_blank_count_on_emulated_kernel(name):
    C.check_case("cpu", name)


def test_identity_on_emulated_kernel():
    C.check_identity("cpu")


@pytest.mark.parametrize("binary", [False, True])
def test_import_scene_undistort_end_to_end_on_emulated_kernel(tmp_path, binary):
    C.check_end_to_end("cpu", tmp_path, binary)


def test_unaligned_destination_takes_the_byte_stores():
    h, w = 33, 47
    img = torch.from_numpy(C.image(h, w))
    cam, dist, _ = C.PARAMS["opencv_barrel"](h, w)
    want, want_blank, _, _ = C.reference(h, w, "opencv_barrel")
    buf = torch.zeros(h * w * 3 + 8, dtype=torch.uint8)
    base = next(o for o in range(1, 5) if (buf.data_ptr() + o) % 4 == 1)
    blank = torch.full((1,), -7, dtype=torch.int32)
    d = (ctypes.c_double * 8)(*dist)
    _lib.call("rcmvs_undistort_rgb8", ctypes.c_void_p(img.data_ptr()), ctypes.c_void_p(buf.data_ptr() + base), h, w, *cam, cam[0], cam[1], d,
              ctypes.c_void_p(blank.data_ptr()), ctypes.c_void_p(0))
    assert np.array_equal(buf[base:base + h * w * 3].numpy().reshape(h, w, 3), want) and int(blank) == want_blank
    assert not buf[:base].any() and not buf[base + h * w * 3:].any()             # nothing written around the image


def test_c_abi_refuses_bad_arguments():
    src, dst = torch.zeros((2, 3, 3), dtype=torch.uint8), torch.zeros((2, 3, 3), dtype=torch.uint8)
    blank = torch.zeros(1, dtype=torch.int32)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                   # noqa: E731
    good = dict(src=p(src), dst=p(dst), h=2, w=3, fx=4.0, fy=4.0, cx=1.5, cy=1.0, fxo=4.0, fyo=4.0, dist=[0.0] * 8, blank=p(blank))

    def call(**kw):
        a = dict(good, **kw)
        d = None if a["dist"] is None else (ctypes.c_double * 8)(*a["dist"])
        _lib.call("rcmvs_undistort_rgb8", a["src"], a["dst"], a["h"], a["w"], a["fx"], a["fy"], a["cx"], a["cy"], a["fxo"], a["fyo"], d, a["blank"],
                  ctypes.c_void_p(0))

    call()
    nan, inf = float("nan"), float("inf")
    for kw, pattern in (({"h": 0}, "bad dims"), ({"w": -1}, "bad dims"), ({"h": 1 << 15, "w": 1 << 15}, "bad dims"),
                        ({"h": 26755, "w": 26755}, "bad dims"),                   # 3 h w = 2^31 + 1427 (and h w below 2^31)
                        ({"src": None}, "null pointer"), ({"dst": None}, "null pointer"), ({"dist": None}, "null pointer"),
                        ({"blank": None}, "null pointer"), ({"dst": good["src"]}, "differ from src"),
                        ({"fx": 0.0}, "focal"), ({"fy": -1.0}, "focal"), ({"fxo": nan}, "focal"), ({"fyo": inf}, "focal"),
                        ({"cx": nan}, "principal point"), ({"cy": -inf}, "principal point"),
                        ({"dist": [0.0] * 5 + [nan, 0.0, 0.0]}, "coefficient 5"), ({"dist": [inf] + [0.0] * 7}, "coefficient 0")):
        with pytest.raises(_lib.RcmvsError, match=pattern):
            call(**kw)
    assert 3 * 26755 * 26755 >= 1 << 31 > 26755 * 26755
    assert not dst.any() and int(blank) == 0                                      # the refused calls wrote nothing
