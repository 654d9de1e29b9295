"""The depth-map fusion kernels (csrc/fusion.hip) on the CPU emulation of tests/emu, driven through rc_mvsnet_amd/fusion.py and the C
entry points on CPU tensors: the cases of tests/test_gpu_fusion.py (tests/fusion_cases.py), every mask, depth, point, colour byte, debug
output, compacted row and block offset equal to tests/fusion_oracle.py in every bit, at every pixel.  The emulation compiles the
kernels' own source with contraction off and runs blocks one after another; what it cannot show is the device compiler's arithmetic,
which tests/test_gpu_fusion.py checks with the same functions on the GPU."""
import os

import pytest

import fusion_cases as FC

FULL = os.environ.get("RCMVS_EMU_FULL", "0") == "1"


@pytest.fixture(autouse=True)
def emu_fusion(emu):
    return emu


def test_friendly_scan_on_emulated_kernels():
    FC.check_friendly("cpu")


@pytest.mark.parametrize("group", [g for g in FC.GROUPS if g != "friendly"])
def test_hostile_cases_on_emulated_kernels(group):
    FC.check_group("cpu", group)


@pytest.mark.parametrize("n", [pytest.param(n, marks=pytest.mark.skipif(n in FC.COMPACT_LARGEST and not FULL, reason="RCMVS_EMU_FULL=1")) for n in FC.COMPACT_SIZES])
def test_compaction_on_emulated_kernels(n):
    """Below 1000 blocks every mask, with rgb and without.  At the sizes round 1024 blocks (a second and more per call here) the random mask
    with rgb and the last-element mask without, which is what the one-block scan's chunks show in; RCMVS_EMU_FULL=1 runs them all, as
    the GPU does."""
    if n < 1000 * FC.BLOCK or FULL:
        FC.check_compaction("cpu", n)
    else:
        FC.check_compaction("cpu", n, masks=FC.QUICK_MASKS, both=False)


def test_refusals_on_the_emulated_path():
    FC.check_refusals("cpu")


def test_filter_depth_on_emulated_kernels(tmp_path):
    FC.check_filter_depth("cpu", tmp_path)


def test_filter_depth_tanks_on_emulated_kernels(tmp_path):
    FC.check_filter_depth_tanks("cpu", tmp_path)
