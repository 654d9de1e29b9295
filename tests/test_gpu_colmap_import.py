"""The COLMAP import on the GPU (rc_mvsnet_amd/colmap_import.py, csrc/view_select.hip) against the fp64 oracle
(tests/colmap_oracle.py); the cases and bounds are tests/colmap_cases.py's, which the CPU emulation runs too.  Scores within
1e-12 (1 + the number of common points): every term is at most 1 and carries a few ulp of fp64 atan2 and exp, the margin the
project gives its other fp64 sums; the table symmetric to the bit, two runs bit-identical; orderings and counts exactly; depth
order statistics bit for bit."""
import json
import os

import pytest

import colmap_cases as C
from rc_mvsnet_amd import colmap_import as CI, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", ["n2", "n3_interleaved", "n3_ranges", "n9"])
def test_pair_scores_vs_oracle(name):
    C.check_scores(DEV, name)


def test_top_views_order_equals_the_oracle():
    C.check_ordering(DEV)


def test_top_views_ties_zero_scores_and_counts():
    C.check_duplicates(DEV)


def test_depth_ranks_are_the_sorted_values():
    C.check_depth_ranks(DEV)


def test_import_scene_end_to_end(tmp_path):
    C.check_end_to_end(DEV, tmp_path)


def test_command_line_prints_the_summary(tmp_path, capsys):
    model = synthetic.colmap_model(n_images=4, n_points=200, hw=(32, 64), seed=3, ext="png")
    synthetic.write_colmap_model(model, str(tmp_path / "sparse"), binary=True)
    synthetic.write_colmap_images(model, str(tmp_path / "photos"))
    out = str(tmp_path / "test" / "scene")
    CI.main(["--model", str(tmp_path / "sparse"), "--images", str(tmp_path / "photos"), "--out", out, "--num-src", "2", "--max-d", "32"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["images"] == 4 and line["num_src"] == 2 and line["skipped_refs"] == [] and line["scene"] == out
    with open(os.path.join(out, "images", "00000000.jpg"), "rb") as f:          # a PNG source arrives as a JPEG
        assert f.read(3) == b"\xff\xd8\xff"
