"""The mesh normals (csrc/mesh_normals.hip through rc_mvsnet_amd/mesh_normals.py) on the GPU: the cases of tests/mesh_normals_cases.py,
every face normal, vertex normal, counter, normal-map float, smooth byte and colour byte equal to tests/mesh_normals_oracle.py in
every bit under both weights, two runs identical; the known answers (a planar grid, swapped faces, Max's weights on a jittered
sphere); the normal pass on the rasteriser's cases and on hostile face images; smooth against flat shading on a sphere; the PLY with
normals through mesh_scan, the readers, the command lines and dtu_eval --surfaces.  The log of a run with -s is
profiles/mesh_normals_pytest_gpu.txt."""
import numpy as np
import pytest
import torch

import mesh_normals_cases as MNC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name,weight", MNC.case_keys())
def test_vertex_and_face_normals_equal_the_oracle(name, weight):
    MNC.check_case(DEV, name, weight, twice=True)


def test_ascending_descending_and_shuffled_faces_of_one_strip():
    MNC.check_orders(DEV)


def test_swapped_faces_negate_every_normal_under_area():
    MNC.check_flip(DEV)


def test_a_real_extraction_before_and_after_decimation():
    MNC.check_extraction(DEV)


def test_refusals():
    MNC.check_refusals(DEV)


@pytest.mark.parametrize("name,W,H,cull", MNC.shade_keys())
def test_normal_pass_equals_the_oracle(name, W, H, cull):
    MNC.check_shade_case(DEV, name, W, H, cull)


def test_a_plane_facing_the_camera_and_vanishing_normals():
    MNC.check_plane(DEV)


def test_a_face_image_is_never_trusted_as_an_address():
    MNC.check_bad_face_image(DEV)


def test_interpolated_normals_are_nearer_the_sphere_than_flat_ones():
    MNC.check_smooth_beats_flat(DEV)


def test_mesh_scan_without_normals_is_what_it_was_and_the_ply_with_normals_round_trips(tmp_path):
    MNC.check_mesh_scan(DEV, tmp_path)


def test_dtu_eval_scores_a_ply_with_normals_as_the_one_without(tmp_path):
    """dtu_eval --surfaces reads a mesh through read_ply_mesh, which skips nx ny nz: every statistic is the same number.  GPU only:
    the evaluation's searches are slow under the emulation."""
    from rc_mvsnet_amd import dtu_eval, mesh_normals as MN, synthetic, tsdf_mesh as TM
    from test_gpu_dtu_mesh import _mat_bytes
    s = synthetic.dtu_eval_mesh(nx=30, ny=20, edge=0.4, n_stl=1500, res=2.0, seed=3)
    gt = tmp_path / "MVS_Data"
    (gt / "Points" / "stl").mkdir(parents=True)
    (gt / "ObsMask").mkdir()
    head = f"ply\nformat binary_little_endian 1.0\nelement vertex {len(s['stl'])}\nproperty float x\nproperty float y\nproperty float z\nend_header\n"
    (gt / "Points" / "stl" / "stl003_total.ply").write_bytes(head.encode() + s["stl"].astype("<f4").tobytes())
    (gt / "ObsMask" / "ObsMask3_10.mat").write_bytes(_mat_bytes({"ObsMask": s["obs_mask"], "BB": s["bb"], "Res": np.array([[s["res"]]])}))
    (gt / "ObsMask" / "Plane3.mat").write_bytes(_mat_bytes({"P": s["plane"].reshape(4, 1)}))
    v, f = np.ascontiguousarray(s["verts"], np.float32), np.ascontiguousarray(s["faces"], np.int32)
    normals, stats = MN.vertex_normals(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), "sphere")
    assert stats["vertices_with_normal"] == len(v)
    rows = []
    for name, kw in (("plain", {}), ("normals", {"normals": normals})):
        (tmp_path / name).mkdir()
        (tmp_path / name / "scan3.ply").write_bytes(TM.mesh_ply_bytes(v, f, None, **kw))
        rows.append(dtu_eval.evaluate_files(str(tmp_path / name), str(gt), 3, device=DEV, surfaces=True))
    print("dtu_eval --surfaces on a PLY with normals:", rows[1])
    assert repr(rows[0]) == repr(rows[1]) and rows[0]["scan"] == 3 and len(rows[0]) > 3
