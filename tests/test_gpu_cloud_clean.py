"""The point-cloud clean-up (csrc/cloud_knn.hip through rc_mvsnet_amd/cloud_clean.py) on the GPU: the cases of tests/cloud_clean_cases.py,
every neighbour index, squared distance, mean, count, flag, mu, sigma, bound, normal and counter equal to tests/cloud_clean_oracle.py
in every bit under a tiny, the default and a single grid cell, two runs identical; the known answers (a planar grid with far points,
a loop of equal means, a sphere seen from outside cameras); scipy's k-d tree and numpy's eigh as independent checks; the fusion
drivers with and without ``clean``.  The log of a run with -s is profiles/cloud_clean_pytest_gpu.txt."""
import pytest

import cloud_clean_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name,k", C.KNN_CASES)
def test_knn_equals_the_oracle_under_three_cell_edges(name, k):
    C.check_knn(DEV, name, k, twice=True)


def test_every_combination_of_outputs_and_the_counters():
    C.check_knn_outputs(DEV)


def test_non_finite_points_are_removed_and_counted():
    C.check_finite(DEV)


def test_a_kd_tree_gives_the_same_rows():
    C.check_kdtree(DEV)


@pytest.mark.parametrize("name,r,cap", C.RADIUS_CASES)
def test_radius_counts_equal_the_oracle(name, r, cap):
    C.check_radius(DEV, name, r, cap)


@pytest.mark.parametrize("name,k,ratio", C.STAT_CASES)
def test_statistical_rule_equals_the_oracle(name, k, ratio):
    C.check_stat(DEV, name, k, ratio)


@pytest.mark.parametrize("name,k,oriented", C.NORMAL_CASES)
def test_normals_and_counters_equal_the_oracle(name, k, oriented):
    C.check_normals(DEV, name, k, oriented)


def test_a_plane_with_centres_above_below_and_in_it():
    C.check_plane_orientation(DEV)


def test_a_sphere_seen_from_outside_cameras():
    C.check_sphere(DEV)


@pytest.mark.parametrize("name,k", [("u4097", 16), ("sphere", 12)])
def test_normals_against_numpy_eigh(name, k):
    C.check_eigh(DEV, name, k)


def test_refusals():
    C.check_refusals(DEV)


def test_clean_cloud_runs_its_steps_in_order():
    C.check_clean_cloud(DEV)


def test_filter_depth_with_and_without_clean(tmp_path):
    C.check_filter_depth(DEV, tmp_path)


def test_filter_depth_tanks_with_and_without_clean(tmp_path):
    C.check_filter_depth_tanks(DEV, tmp_path)
