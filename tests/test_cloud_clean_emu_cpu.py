"""The point-cloud clean-up kernels (csrc/cloud_knn.hip) on the CPU emulation of tests/emu, driven through rc_mvsnet_amd/cloud_clean.py on
CPU tensors: the checks of tests/test_gpu_cloud_clean.py (tests/cloud_clean_cases.py).  The emulation runs blocks one after another, so
a kernel that waited for another workgroup would never return here.  What it cannot show is the device compiler's arithmetic, which
the same functions check on the GPU."""
import os
import subprocess
import sys

import pytest

import cloud_clean_cases as C
from rc_mvsnet_amd import _lib


@pytest.fixture(autouse=True)
def emu_ck(emu):
    _lib.bind(emu)                                               # the emu fixture binds the primary header's table; the extensions' too
    return emu


@pytest.mark.parametrize("name,k", C.KNN_CASES)
def test_knn_on_emulated_kernels(name, k):
    C.check_knn("cpu", name, k, twice=name in ("lattice", "u2049", "dup40"))


def test_every_combination_of_outputs_on_emulated_kernels():
    C.check_knn_outputs("cpu")


def test_non_finite_points_on_emulated_kernels():
    C.check_finite("cpu")


def test_a_kd_tree_gives_the_same_rows_on_emulated_kernels():
    C.check_kdtree("cpu")


@pytest.mark.parametrize("name,r,cap", C.RADIUS_CASES)
def test_radius_counts_on_emulated_kernels(name, r, cap):
    C.check_radius("cpu", name, r, cap)


@pytest.mark.parametrize("name,k,ratio", C.STAT_CASES)
def test_statistical_rule_on_emulated_kernels(name, k, ratio):
    C.check_stat("cpu", name, k, ratio)


@pytest.mark.parametrize("name,k,oriented", C.NORMAL_CASES)
def test_normals_on_emulated_kernels(name, k, oriented):
    C.check_normals("cpu", name, k, oriented)


def test_a_plane_with_centres_on_emulated_kernels():
    C.check_plane_orientation("cpu")


def test_a_sphere_on_emulated_kernels():
    C.check_sphere("cpu")


@pytest.mark.parametrize("name,k", [("u4097", 16), ("sphere", 12)])
def test_normals_against_numpy_eigh_on_emulated_kernels(name, k):
    C.check_eigh("cpu", name, k)


def test_refusals_on_the_emulated_path():
    C.check_refusals("cpu")


def test_clean_cloud_on_emulated_kernels():
    C.check_clean_cloud("cpu")


def test_filter_depth_on_emulated_kernels(tmp_path):
    C.check_filter_depth("cpu", tmp_path)


def test_filter_depth_tanks_on_emulated_kernels(tmp_path):
    C.check_filter_depth_tanks("cpu", tmp_path)


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("order", ["1", "2"])
def test_other_thread_orders_give_the_same_bytes(order, tmp_path):
    """RCMVS_EMU_ORDER=1|2 schedules every block's threads in another order between synchronisation points: the grid's counting sort
    fills its cells in another order and the counters' atomic adds arrive in another order, and nothing may show.  Run in a child
    process (the order is read when the library is loaded)."""
    script = tmp_path / "run.py"
    script.write_text(
        "import sys\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np, torch, conftest\n"
        "import cloud_clean_cases as C\n"
        "from rc_mvsnet_amd import _lib, cloud_clean as CC\n"
        "lib = conftest.load_emu_lib()\n"
        "conftest.route_to_emulation(lib, setattr)\n"
        "_lib.bind(lib)\n"
        "for name, k in (('u2049', 20), ('lattice', 26), ('dup40', 8), ('clusters', 8), ('zeros', 8)):\n"
        "    t = C.dev_cloud(name, 'cpu')\n"
        "    r = CC.knn_device(t, k, want=('idx', 'd2', 'mean'))\n"
        "    sys.stdout.write(''.join(r[key].numpy().tobytes().hex() for key in ('idx', 'd2', 'mean')))\n"
        "    keep, stats = CC.statistical_from_means(r['mean'], 1.0)\n"
        "    n, c = CC.normals_from_neighbours(t, r['idx'])\n"
        "    keep2, counts = CC.radius_outliers(t, 0.1, 4)\n"
        "    sys.stdout.write(''.join(x.numpy().tobytes().hex() for x in (keep, stats, n, c, keep2, counts)))\n"
        % (REPO, os.path.join(REPO, "tests")))
    outs = []
    for o in ("0", order):
        env = dict(os.environ, RCMVS_EMU_ORDER=o)
        outs.append(subprocess.run([sys.executable, str(script)], env=env, check=True, capture_output=True, text=True).stdout)
    assert len(outs[0]) > 100000 and outs[0] == outs[1]
