"""TSDF fusion and marching tetrahedra on the GPU (rc_mvsnet_amd/tsdf_mesh.py, csrc/tsdf_mesh.hip) against the fp64 oracle
(tests/tsdf_oracle.py); the cases are tests/tsdf_cases.py's, which the CPU emulation runs too.  Every plane of the integration
state, every vertex, colour and face equal to the oracle in every bit and in order, totals equal, two runs identical; the closed
spheres closed, consistently oriented, of Euler characteristic 2 with outward normals, on the kernel's own output.

Vertices lie within sqrt(3) h of the sphere they mesh: a vertex and the true crossing lie on the same grid edge, which is at most
a cube's diagonal long.  Measured maxima on the GPU (equal to the oracle's, as every bit is): 0.0854 h (sphere_12), 0.1068 h
(sphere_13_zero_corners), 0.0929 h (sphere_13x13x14)."""
import json
import os

import numpy as np
import pytest

import tsdf_cases as C
from rc_mvsnet_amd import _lib, dtu_io, synthetic, tsdf_mesh as TM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", C.INTEGRATE)
def test_integration_state_equals_the_oracle(name):
    C.check_integrate(DEV, name)


def test_chunking_does_not_change_a_bit():
    C.check_chunking(DEV)


@pytest.mark.parametrize("name", C.EXTRACT)
def test_extraction_equals_the_oracle(name):
    C.check_extract(DEV, name)


def test_scan_top_level_on_a_162_cube():
    C.check_scan_top_level(DEV)


def test_mesh_scan_end_to_end(tmp_path):
    C.check_end_to_end(DEV, tmp_path)


def test_command_line_prints_the_summary(tmp_path, capsys):
    pair_folder, out_folder = C.write_scan(tmp_path)
    ply = str(tmp_path / "mesh.ply")
    TM.main(["--pair-folder", pair_folder, "--scan-folder", out_folder, "--out-folder", out_folder, "--mesh", ply, "--resolution", "24",
             "--min-weight", "2"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    verts, faces = dtu_io.read_ply_mesh(ply)
    assert line["vertices"] == len(verts) > 0 and line["faces"] == len(faces) > 0 and line["min_weight"] == 2 and max(line["dims"]) in (30, 31)


def test_eval_driver_mesh_option(tmp_path):
    """eval_driver --filter --mesh on a synthetic scan folder writes <scan>_mesh.ply after the cloud; the cloud is the same to the
    byte as without --mesh, and --mesh without --filter is refused"""
    from rc_mvsnet_amd import eval_driver
    _lib.load()
    scan = synthetic.fusion_scan(V=4, H=128, W=160, seed=1, n_src=3)
    data = str(tmp_path / "data")
    synthetic.write_fusion_scan(scan, os.path.join(data, "scan7"), os.path.join(data, "scan7"))
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        f.write("scan7\n")
    clouds = []
    for out, extra in ((str(tmp_path / "plain"), []), (str(tmp_path / "meshed"), ["--mesh", "--mesh-resolution", "32"])):
        eval_driver.main(["--outdir", out, "--testpath", data, "--testlist", lst, "--num_view", "3", "--ndepths", "16,8,8", "--filter",
                          "--prob_thres", "0.0", "--num_consistency", "1", "--img_dist_thres", "4.0", "--depth_thres", "0.5"] + extra)
        with open(os.path.join(out, "scan7.ply"), "rb") as f:
            clouds.append(f.read())
    assert clouds[0] == clouds[1] and len(clouds[0]) > 1000
    assert not os.path.exists(str(tmp_path / "plain" / "scan7_mesh.ply"))
    verts, faces = dtu_io.read_ply_mesh(str(tmp_path / "meshed" / "scan7_mesh.ply"))
    assert len(verts) > 0 and len(faces) > 0 and faces.max() < len(verts) and np.isfinite(verts).all()
    with pytest.raises(SystemExit, match="--mesh"):
        eval_driver.main(["--outdir", str(tmp_path / "x"), "--mesh"])
