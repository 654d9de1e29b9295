"""The COLMAP-import kernels (csrc/view_select.hip) on the CPU emulation of tests/emu, driven through
rc_mvsnet_amd/colmap_import.py on CPU tensors: the cases and bounds of tests/test_gpu_colmap_import.py (tests/colmap_cases.py).
The emulation runs blocks one after another, so this also pins that no result depends on the blocks' order."""
import pytest

import colmap_cases as C
from rc_mvsnet_amd import _lib, colmap_import as CI, fusion


@pytest.fixture(autouse=True)
def emu_ci(emu, monkeypatch):
    _lib.bind(emu)                                               # the emu fixture binds the primary header's table; the extensions' too
    monkeypatch.setattr(CI, "_chk", fusion._chk)                 # routed by the emu fixture: CPU tensors, NULL stream
    monkeypatch.setattr(CI, "_stream", fusion._stream)
    return emu


@pytest.mark.parametrize("name", ["n2", "n3_interleaved", "n3_ranges", "n9"])
def test_pair_scores_on_emulated_kernels(name):
    C.check_scores("cpu", name)


def test_top_views_order_on_emulated_kernels():
    C.check_ordering("cpu")


def test_top_views_ties_on_emulated_kernels():
    C.check_duplicates("cpu")


def test_depth_ranks_on_emulated_kernels():
    C.check_depth_ranks("cpu")


def test_import_scene_end_to_end_on_emulated_kernels(tmp_path):
    C.check_end_to_end("cpu", tmp_path)
