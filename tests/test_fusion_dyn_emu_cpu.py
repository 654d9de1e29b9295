"""The dynamic depth-map fusion kernel (csrc/fusion_dyn.hip) on the CPU emulation of tests/emu, driven through rc_mvsnet_amd/fusion.py and
the C entry point on CPU tensors: the cases of tests/test_gpu_fusion_dyn.py (tests/fusion_dyn_cases.py), every output and the whole
`used` array equal to tests/fusion_dyn_oracle.py in every bit, at every pixel.  What the emulation cannot show is the device compiler's
arithmetic, which tests/test_gpu_fusion_dyn.py checks with the same functions on the GPU."""
import pytest

import fusion_dyn_cases as DC


@pytest.fixture(autouse=True)
def emu_fusion(emu):
    return emu


@pytest.mark.parametrize("group", list(DC.GROUPS))
def test_cases_on_emulated_kernel(group):
    DC.check_group("cpu", group)


def test_wrapper_on_emulated_kernel():
    DC.check_wrapper("cpu")


def test_scan_in_order_on_emulated_kernel():
    DC.check_scan_in_order("cpu")


def test_known_answer_on_emulated_kernel():
    DC.check_known_answer("cpu")


def test_refusals_on_the_emulated_path():
    DC.check_refusals("cpu")


def test_filter_depth_on_emulated_kernel(tmp_path):
    DC.check_filter_depth("cpu", tmp_path)


def test_filter_depth_tanks_on_emulated_kernel(tmp_path):
    DC.check_filter_depth_tanks("cpu", tmp_path)
