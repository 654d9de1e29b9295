"""The mesh rasteriser (csrc/mesh_render.hip through rc_mvsnet_amd/mesh_render.py) on the GPU: the cases of tests/mesh_render_cases.py,
every key, depth, face number, colour byte, shade byte and counter equal to tests/mesh_render_oracle.py in every bit, two runs
identical; the comparison table's counts equal and its sum within 1e-12 relative; the known answers (a fronto-parallel quad at
depth exactly 2.0f on a hand-counted pixel set, a slanted plane within the snapping bound, flat and ramped colours) and the round
trip on the sphere scene of the sparse TSDF suite, whose bound is derived in mesh_render_cases.check_round_trip.  The test prints
the measured maximum of the round trip; the log of a run with -s is profiles/mesh_render_pytest_gpu.txt."""
import pytest

import mesh_render_cases as MRC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name,W,H,cull", MRC.case_keys())
def test_render_equals_the_oracle(name, W, H, cull):
    MRC.check_case(DEV, name, W, H, cull, twice=True)


def test_white_faces_and_background():
    MRC.check_without_colours_and_background(DEV)


def test_permuted_and_reversed_faces():
    MRC.check_permutation(DEV)


def test_views_in_one_call_and_one_by_one():
    MRC.check_views_one_by_one(DEV)


def test_a_list_longer_than_the_large_grid():
    MRC.check_large_path_alone(DEV)


def test_compare_counts_and_sum():
    MRC.check_compare(DEV)


def test_refusals():
    MRC.check_refusals(DEV)


def test_round_trip_on_the_sphere_scene():
    MRC.check_round_trip(DEV)


def test_mesh_scan_without_render_is_what_it_was_and_command_line_round_trip(tmp_path):
    MRC.check_command_line_round_trip(DEV, tmp_path)
