"""The mesh clean-up pass on the GPU (rc_mvsnet_amd/mesh_clean.py, csrc/mesh_clean.hip) against tests/mesh_clean_oracle.py; the cases
are tests/mesh_clean_cases.py's, which the CPU emulation runs too.  Labels, flags, ranks, neighbours, multiplicities, positions,
colours, faces and every count equal in every bit and in order; two runs identical."""
import json

import numpy as np
import pytest
import torch

import mesh_clean_cases as MCC
import tsdf_cases as C
from rc_mvsnet_amd import _lib, dtu_io, mesh_clean as MC, tsdf_mesh as TM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", list(MCC.CASES))
def test_components_and_adjacency_equal_the_oracle(name):
    MCC.check_parts(DEV, name)


@pytest.mark.parametrize("name,k", MCC.case_keys())
def test_clean_mesh_equals_the_oracle_and_two_runs_are_identical(name, k):
    MCC.check_clean(DEV, name, k, twice=True)


def test_scan_reaches_its_third_level():
    MCC.check_scan_third_level(DEV)


def test_taubin_identities_and_pinning():
    MCC.check_smoothing_parts(DEV)


def test_real_extraction():
    MCC.check_extraction(DEV)


def test_mesh_scan_with_clean_options_end_to_end(tmp_path):
    MCC.check_end_to_end(DEV, tmp_path)


def test_cpu_tensors_are_refused():
    v, f = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    _lib.load()
    with pytest.raises(_lib.RcmvsError, match="GPU"):
        MC.clean_mesh(v, f)
    with pytest.raises(_lib.RcmvsError, match="one device"):
        MC.clean_mesh(v.to(DEV), f)


def test_command_lines_print_the_summary(tmp_path, capsys):
    """python -m rc_mvsnet_amd.mesh_clean on a written mesh, and tsdf_mesh's own --keep-largest / --smooth"""
    v, f, _ = MCC.case("tiles_4097")
    src, out = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    with open(src, "wb") as fh:
        fh.write(TM.mesh_ply_bytes(v, f))
    MC.main(["--in", src, "--out", out, "--keep-largest", "3", "--smooth", "1", "--no-pin-boundary", "--device", DEV])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    gv, gf = dtu_io.read_ply_mesh(out)
    wv, wf, _, wstats = MCC.O.clean_mesh(v, f, None, keep_largest=3, smooth_iterations=1, pin_boundary=False)
    assert {k: line[k] for k in wstats} == wstats and line["faces_out"] == 12 and MCC.same_bits(gv, wv) and np.array_equal(gf, wf)
    pair_folder, out_folder = C.write_scan(tmp_path)
    ply = str(tmp_path / "mesh.ply")
    TM.main(["--pair-folder", pair_folder, "--scan-folder", out_folder, "--out-folder", out_folder, "--mesh", ply, "--resolution", "24", "--keep-largest", "1",
             "--smooth", "1"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    gv, gf = dtu_io.read_ply_mesh(ply)
    assert line["clean"]["components_kept"] == 1 and line["clean"]["smooth_iterations"] == 1 and line["vertices"] == len(gv) and line["faces"] == len(gf) > 0
