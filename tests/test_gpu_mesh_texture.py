"""The mesh texturing (csrc/mesh_texture.hip through rc_mvsnet_amd/mesh_texture.py) on the GPU: the cases of tests/mesh_texture_cases.py,
every best, class, sorted index, table entry, texel coordinate, owner, atlas byte, counter and textured pixel equal to
tests/mesh_texture_oracle.py in every bit, two runs identical; the view choice; the class thresholds, shifts and max_size; the known
answers of the fill on the ramp plane; the round trips on the plane and on the decimated sphere; mesh_scan, the readers, the command
lines and dtu_eval --surfaces.  The log of a run with -s is profiles/mesh_texture_pytest_gpu.txt."""
import numpy as np
import pytest

import mesh_texture_cases as MTC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", MTC.case_keys())
def test_texture_equals_the_oracle(name):
    MTC.check_case(DEV, name, twice=True)


def test_chunks_of_views_and_single_votes_give_the_same_bits():
    MTC.check_chunks(DEV)


def test_max_size_raises_the_shift_and_refuses_with_the_needed_size():
    MTC.check_max_size(DEV)


def test_texels_of_a_plane_hold_the_ramp_at_their_own_position():
    MTC.check_ramp(DEV)


def test_textured_render_of_the_plane_reproduces_the_image():
    MTC.check_plane_round_trip(DEV)


def test_textured_sphere_is_nearer_its_images_than_vertex_colours():
    MTC.check_sphere(DEV)


def test_refusals():
    MTC.check_refusals(DEV)


def test_mesh_scan_without_texture_is_what_it_was_and_the_textured_ply_round_trips(tmp_path):
    MTC.check_mesh_scan(DEV, tmp_path)


def test_dtu_eval_scores_a_textured_ply_as_the_one_without(tmp_path):
    """dtu_eval --surfaces reads a mesh through read_ply_mesh, which skips the faces' texcoord lists: every statistic is the same number.
    GPU only: the evaluation's searches are slow under the emulation."""
    from rc_mvsnet_amd import dtu_eval, synthetic, tsdf_mesh as TM
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
    uv = np.random.default_rng(2).random((len(f), 3, 2), dtype=np.float32)
    rows = []
    for name, kw in (("plain", {}), ("textured", {"texcoords": uv, "texture_file": "scan3.png"})):
        (tmp_path / name).mkdir()
        (tmp_path / name / "scan3.ply").write_bytes(TM.mesh_ply_bytes(v, f, None, **kw))
        rows.append(dtu_eval.evaluate_files(str(tmp_path / name), str(gt), 3, device=DEV, surfaces=True))
    print("dtu_eval --surfaces on a textured PLY:", rows[1])
    assert repr(rows[0]) == repr(rows[1]) and rows[0]["scan"] == 3 and len(rows[0]) > 3
