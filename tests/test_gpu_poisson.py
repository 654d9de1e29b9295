"""The Poisson reconstruction (csrc/poisson.hip through rc_mvsnet_amd/poisson_mesh.py) on the GPU: the cases of tests/poisson_cases.py,
every accumulator, plane, right-hand side, level after every cycle, residual, isovalue, field and mesh equal to
tests/poisson_oracle.py in every bit, two runs identical (the splats' atomics arrive in whatever order the hardware chooses); the
known answers (spheres, trimming, a plane patch, a uniform colour, two spheres and keep_largest); the refusals.  The log of a run
with -s is profiles/poisson_pytest_gpu.txt.

Figures, the oracle's (fp32 planes, fp64 arithmetic) and, equal in every bit, the kernels': the sphere's vertices lie within 0.2569 h
(16^3, 1 500 points) and 0.2665 h (24^3, 4 000 points) of it, bounds 1.5 x that; the residual falls by 0.100, 0.188, 0.201, 0.212
(16^3) and 0.107, 0.215, 0.223, 0.232 (24^3) over cycles 1 .. 4, bound 1.5 x the largest; the plane patch's vertices lie within
0.2348 h of the plane."""
import pytest

import poisson_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", C.PIPELINE_CASES)
def test_every_stage_equals_the_oracle_and_two_runs_agree(name):
    C.check_pipeline(DEV, name)


@pytest.mark.parametrize("r", [16, 24])
def test_a_sphere_is_closed_oriented_near_and_converges(r):
    C.check_sphere(DEV, r)


@pytest.mark.parametrize("r", [16, 24])
def test_trimming_keeps_a_full_sphere_closed_and_opens_a_capless_one(r):
    C.check_trim(DEV, r)


def test_a_plane_patch_stays_near_the_plane_and_keeps_its_colour():
    C.check_plane(DEV)


def test_keep_largest_leaves_one_of_two_spheres():
    C.check_keep_largest(DEV)


def test_the_fusion_drivers_cloud_writer_meshes_the_cleaned_cloud(tmp_path):
    C.check_write_cloud(DEV, tmp_path)


def test_refusals():
    C.check_refusals(DEV)
