"""The hole-filling kernels (csrc/mesh_holes.hip) on cuda:0 against tests/mesh_holes_oracle.py: the cases of
tests/mesh_holes_cases.py, every successor, flag, counter, position, colour and face equal in every bit, two runs identical."""
import json

import pytest

import mesh_holes_cases as MHC
from rc_mvsnet_amd import dtu_io, tsdf_mesh as TM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name,k", MHC.case_keys())
def test_fill_holes_and_boundary_equal_the_oracle_and_two_runs_are_identical(name, k):
    MHC.check_case(DEV, name, k, twice=True)


def test_refusals():
    MHC.check_refusals(DEV)


def test_clean_mesh_fills_between_compaction_and_smoothing():
    MHC.check_clean_composite(DEV)


def test_clean_mesh_without_the_option_is_what_it_was():
    MHC.check_off_is_today(DEV)


@pytest.mark.parametrize("sparse", [False, True])
def test_mesh_scan_with_hole_filling_end_to_end_and_its_command_line(tmp_path, capsys, sparse):
    pair_folder, out_folder, summary = MHC.check_end_to_end(DEV, tmp_path, sparse)
    capsys.readouterr()
    ply = str(tmp_path / "cli.ply")
    TM.main(["--pair-folder", pair_folder, "--scan-folder", out_folder, "--out-folder", out_folder, "--mesh", ply, "--resolution", "32", "--keep-largest", "1",
             "--fill-holes", "64", "--device", DEV] + (["--sparse"] if sparse else []))
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["clean"] == summary["clean"] and open(ply, "rb").read() == open(summary["mesh"], "rb").read()
    assert line["faces"] == len(dtu_io.read_ply_mesh(ply)[1])


def test_mesh_clean_command_line_round_trip(tmp_path):
    MHC.check_command_line_round_trip(DEV, tmp_path)
