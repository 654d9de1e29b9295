"""The Poisson reconstruction kernels (csrc/poisson.hip) on the CPU emulation of tests/emu, driven through rc_mvsnet_amd/poisson_mesh.py
on CPU tensors: the checks of tests/test_gpu_poisson.py (tests/poisson_cases.py).  The emulation runs blocks one after another, so a
kernel that waited for another workgroup would never return here.  What it cannot show is the device compiler's arithmetic and the
order in which the hardware's atomics arrive, which the same functions check on the GPU."""
import os
import subprocess
import sys

import pytest

import poisson_cases as C
from rc_mvsnet_amd import _lib


@pytest.fixture(autouse=True)
def emu_po(emu):
    _lib.bind(emu)                                               # the emu fixture binds the primary header's table; the extensions' too
    return emu


@pytest.mark.parametrize("name", C.PIPELINE_CASES)
def test_every_stage_equals_the_oracle_on_emulated_kernels(name):
    C.check_pipeline("cpu", name)


@pytest.mark.parametrize("r", [16, 24])
def test_a_sphere_on_emulated_kernels(r):
    C.check_sphere("cpu", r)


def test_trimming_a_sphere_on_emulated_kernels():
    C.check_trim("cpu", 16)


def test_a_plane_patch_and_its_colour_on_emulated_kernels():
    C.check_plane("cpu")


def test_keep_largest_on_emulated_kernels():
    C.check_keep_largest("cpu")


def test_the_fusion_drivers_cloud_writer_on_emulated_kernels(tmp_path):
    C.check_write_cloud("cpu", tmp_path)


def test_refusals_on_the_emulated_path():
    C.check_refusals("cpu")


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("order", ["1", "2"])
def test_other_thread_orders_give_the_same_bytes(order, tmp_path):
    """RCMVS_EMU_ORDER=1|2 schedules every block's threads in another order between synchronisation points: the splats' atomic adds
    arrive in another order, and nothing may show (the sums are integers).  Run in a child process (the order is read when the
    library is loaded)."""
    script = tmp_path / "run.py"
    script.write_text(
        "import sys\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np, torch, conftest\n"
        "import poisson_cases as C\n"
        "from rc_mvsnet_amd import _lib\n"
        "lib = conftest.load_emu_lib()\n"
        "conftest.route_to_emulation(lib, setattr)\n"
        "_lib.bind(lib)\n"
        "for name in ('contention', 'dup40', 'n4097', 'hazards', 'sphere16_rel'):\n"
        "    r = C.run('cpu', name, False)\n"
        "    arrays = [r[k] for k in ('acc', 'W', 'V', 'point', 'b', 'x', 'stats', 'dsum', 'wsum')] + [r['mesh']['verts'], r['mesh']['faces']]\n"
        "    sys.stdout.write(''.join(np.ascontiguousarray(a).tobytes().hex() for a in arrays) + repr(r['resid']) + repr(r['counters']))\n"
        % (REPO, os.path.join(REPO, "tests")))
    outs = []
    for o in ("0", order):
        env = dict(os.environ, RCMVS_EMU_ORDER=o)
        outs.append(subprocess.run([sys.executable, str(script)], env=env, check=True, capture_output=True, text=True).stdout)
    assert len(outs[0]) > 100000 and outs[0] == outs[1]
