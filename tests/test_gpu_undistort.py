"""Image undistortion on the GPU (rc_mvsnet_amd/colmap_import.py undistort_image, csrc/undistort.hip) against the fp64 oracle
(tests/undistort_oracle.py); the cases are tests/undistort_cases.py's, which the CPU emulation runs too.  Bytes equal in every byte
and the blank count equal (the kernel and the oracle do the same correctly rounded fp64 operations in one written order, and the
blank test is made on the fp64 position before any conversion), two runs identical; the identity camera returns its input."""
import json
import os

import pytest

import undistort_cases as C
from rc_mvsnet_amd import colmap_import as CI, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", list(C.PARAMS))
def test_bytes_and_blank_count_equal_the_oracle(name):
    C.check_case(DEV, name)


def test_identity_returns_the_input():
    C.check_identity(DEV)


def test_full_size_opencv_image():
    C.check_full_size(DEV)


def test_import_scene_undistort_end_to_end(tmp_path):
    C.check_end_to_end(DEV, tmp_path)


def test_command_line_undistorts_a_simple_radial_model(tmp_path, capsys):
    model = synthetic.colmap_model(n_images=4, n_points=200, hw=(32, 64), seed=3, camera_model="SIMPLE_RADIAL")
    synthetic.write_colmap_model(model, str(tmp_path / "sparse"), binary=True)
    synthetic.write_colmap_images(model, str(tmp_path / "photos"))
    out = str(tmp_path / "test" / "scene")
    argv = ["--model", str(tmp_path / "sparse"), "--images", str(tmp_path / "photos"), "--out", out, "--num-src", "2", "--max-d", "32"]
    with pytest.raises(CI._lib.RcmvsError, match=r"cameras\.bin.*SIMPLE_RADIAL.*undistorted first"):
        CI.main(argv)                                                             # refused as before without the option
    CI.main(argv + ["--undistort", "--focal-scale", "0.9"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["images"] == 4 and line["undistorted"] == 4 and line["focal_scale"] == 0.9 and 0 < line["blank_fraction_max"] < 0.5
    assert sorted(os.listdir(os.path.join(out, "images"))) == ["%08d.jpg" % k for k in range(4)]
