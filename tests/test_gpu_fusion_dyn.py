"""GPU: the dynamic depth-map fusion kernel (rc_mvsnet_amd/fusion.py over rcmvs_fuse_view_dyn) against the exact oracle
(tests/fusion_dyn_oracle.py) on the cases of tests/fusion_dyn_cases.py: every output and the whole `used` array in every bit, at every
pixel.  tests/test_fusion_dyn_emu_cpu.py runs the same functions on the CPU emulation."""
import pytest

import fusion_dyn_cases as DC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("group", list(DC.GROUPS))
def test_exact_cases(group):
    """the existing scans under the defaults, the graded scan, the knife edges, the level ranges, the suppression cases"""
    DC.check_group(DEV, group)


def test_exact_wrapper():
    DC.check_wrapper(DEV)


def test_exact_scan_in_order():
    DC.check_scan_in_order(DEV)


def test_known_answer():
    DC.check_known_answer(DEV)


def test_exact_large_view():
    DC.check_large_view(DEV)


def test_refusals_before_any_launch():
    DC.check_refusals(DEV)


def test_filter_depth_modes_are_the_exact_oracle(tmp_path):
    DC.check_filter_depth(DEV, tmp_path)


def test_filter_depth_tanks_modes_are_the_exact_oracle(tmp_path):
    DC.check_filter_depth_tanks(DEV, tmp_path)
