"""The block-sparse TSDF volume on the GPU (rc_mvsnet_amd/tsdf_mesh.py SparseTsdfVolume, csrc/tsdf_sparse.hip) against
tests/tsdf_sparse_oracle.py -- the dense fp64 oracle read through the block table -- and against the dense kernels themselves;
the cases are tests/tsdf_sparse_cases.py's, which the CPU emulation runs too.  Flags, skipped counts, ranks, planes, vertices,
colours and faces equal in every bit and in order, two runs identical; where a sparse mesh is compared with a dense one, equal
as multisets of vertex records and of faces written as vertex records."""
import json
import os

import numpy as np
import pytest

import tsdf_cases as C
import tsdf_sparse_cases as SC
from rc_mvsnet_amd import _lib, dtu_io, synthetic, tsdf_mesh as TM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", SC.MARK)
def test_marking_equals_the_oracle(name):
    SC.check_mark(DEV, name)


@pytest.mark.parametrize("name", list(SC.BUILD))
def test_build_equals_the_oracle(name):
    SC.check_build(DEV, name)


def test_calls_out_of_order_and_an_empty_block_set_are_refused():
    SC.check_call_order(DEV)


@pytest.mark.parametrize("name", C.INTEGRATE)
def test_integration_state_equals_the_oracle(name):
    SC.check_integrate(DEV, name)


def test_chunking_does_not_change_a_bit():
    SC.check_chunking(DEV)


@pytest.mark.parametrize("name", C.INTEGRATE)
def test_integration_state_equals_the_dense_kernel(name):
    SC.check_integrate_against_dense_kernel(DEV, name)


@pytest.mark.parametrize("name", SC.EXTRACT)
def test_extraction_equals_the_oracle(name):
    SC.check_extract(DEV, name)


def test_scan_top_level_on_9261_blocks():
    SC.check_scan_top_level(DEV)


@pytest.mark.parametrize("name", list(SC.SCENES))
def test_sparse_mesh_is_the_dense_mesh(name):
    SC.check_scene_on_the_kernels(DEV, name)


def test_mesh_scan_sparse_end_to_end(tmp_path):
    SC.check_end_to_end(DEV, tmp_path)


def test_mesh_scan_tanks_end_to_end(tmp_path):
    SC.check_tanks_end_to_end(DEV, tmp_path)


def test_command_line_sparse_prints_the_summary(tmp_path, capsys):
    pair_folder, out_folder = C.write_scan(tmp_path)
    ply = str(tmp_path / "mesh.ply")
    TM.main(["--pair-folder", pair_folder, "--scan-folder", out_folder, "--out-folder", out_folder, "--mesh", ply, "--resolution", "24", "--sparse"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    verts, faces = dtu_io.read_ply_mesh(ply)
    assert line["vertices"] == len(verts) > 0 and line["faces"] == len(faces) > 0 and line["skipped_pixels"] == 0
    assert line["dims"] == [8 * b for b in line["bdims"]] and max(line["dims"]) == 32 and line["allocated_voxels"] == 512 * line["active_blocks"] > 0


def test_eval_driver_mesh_sparse_option(tmp_path):
    """eval_driver --filter --mesh --mesh-sparse on a synthetic scan folder: the sparse volume's mesh next to an unchanged cloud"""
    from rc_mvsnet_amd import eval_driver
    _lib.load()
    scan = synthetic.fusion_scan(V=4, H=128, W=160, seed=1, n_src=3)
    data = str(tmp_path / "data")
    synthetic.write_fusion_scan(scan, os.path.join(data, "scan7"), os.path.join(data, "scan7"))
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        f.write("scan7\n")
    clouds = []
    for out, extra in ((str(tmp_path / "plain"), []), (str(tmp_path / "meshed"), ["--mesh", "--mesh-sparse", "--mesh-resolution", "64"])):
        eval_driver.main(["--outdir", out, "--testpath", data, "--testlist", lst, "--num_view", "3", "--ndepths", "16,8,8", "--filter",
                          "--prob_thres", "0.0", "--num_consistency", "1", "--img_dist_thres", "4.0", "--depth_thres", "0.5"] + extra)
        with open(os.path.join(out, "scan7.ply"), "rb") as f:
            clouds.append(f.read())
    assert clouds[0] == clouds[1] and len(clouds[0]) > 1000
    verts, faces = dtu_io.read_ply_mesh(str(tmp_path / "meshed" / "scan7_mesh.ply"))
    assert len(verts) > 0 and len(faces) > 0 and faces.max() < len(verts) and np.isfinite(verts).all()


def test_eval_driver_tanks_mesh(tmp_path):
    """eval_driver --dataset tanks --mesh writes <plydir>/<scene>_mesh.ply after the cloud, and the cloud is the same to the byte as
    without --mesh.  The depth maps come from a network with seeded random weights, so the scene's filter may keep no point; then
    the mesh is written empty (mesh_scan_tanks on depth maps that do reproject is test_mesh_scan_tanks_end_to_end)."""
    from rc_mvsnet_amd import eval_driver
    data = str(tmp_path / "tt")
    synthetic.write_tanks_tree(data, scenes=("Family",), V=7, hw=(64, 96), orig_hw=(75, 100), n_src=6)
    common = ["--dataset", "tanks", "--testpath", data, "--scenes", "Family", "--num_view", "7", "--max_w", "96", "--max_h", "64", "--ndepths", "16,8,8",
              "--io_threads", "2"]
    clouds = []
    for k, extra in enumerate(([], ["--mesh", "--mesh-resolution", "64", "--mesh-trunc-voxels", "2.0"])):
        out, ply = str(tmp_path / ("exp%d" % k)), str(tmp_path / ("ply%d" % k))
        eval_driver.main(common + ["--outdir", out, "--plydir", ply] + extra)
        with open(os.path.join(ply, "Family.ply"), "rb") as f:
            clouds.append(f.read())
    assert clouds[0] == clouds[1] and clouds[0].startswith(b"ply\n")
    assert not os.path.exists(str(tmp_path / "ply0" / "Family_mesh.ply"))
    verts, faces = dtu_io.read_ply_mesh(str(tmp_path / "ply1" / "Family_mesh.ply"))
    assert len(faces) == 0 or (faces.max() < len(verts) and np.isfinite(verts).all())
