"""Mesh decimation on the GPU (rc_mvsnet_amd/mesh_decimate.py, csrc/mesh_decimate.hip) against tests/mesh_decimate_oracle.py; the
cases are tests/mesh_decimate_cases.py's, which the CPU emulation runs too.  Cluster numbers, keys, flags, counters, quadrics,
positions, colours and faces equal in every bit and in order; two runs identical; the command lines."""
import json

import numpy as np
import pytest
import torch

import mesh_decimate_cases as MDC
import tsdf_cases as C
from rc_mvsnet_amd import _lib, dtu_io, mesh_decimate as MD, tsdf_mesh as TM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name,k", MDC.case_keys())
def test_decimate_and_its_parts_equal_the_oracle_and_two_runs_are_identical(name, k):
    MDC.check_case(DEV, name, k, twice=True)


def test_refusals():
    MDC.check_refusals(DEV)


def test_identity_when_every_vertex_is_alone():
    MDC.check_identity_when_every_vertex_is_alone(DEV)


def test_real_extraction():
    MDC.check_extraction(DEV)


def test_cpu_tensors_are_refused():
    v, f = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    _lib.load()
    with pytest.raises(_lib.RcmvsError, match="GPU"):
        MD.decimate(v, f, cell=1.0)
    with pytest.raises(_lib.RcmvsError, match="one device"):
        MD.decimate(v.to(DEV), f, cell=1.0)


def test_mesh_decimate_command_line_round_trip(tmp_path, capsys):
    """python -m rc_mvsnet_amd.mesh_decimate on a written coloured mesh: the bytes of mesh_ply_bytes of decimate()'s result"""
    v, f, rgb = MDC.case("two_sheets")
    src, out = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    with open(src, "wb") as fh:
        fh.write(TM.mesh_ply_bytes(v, f, rgb))
    for argv, kw in (([], {}), (["--placement", "mean", "--reg", "0.01", "--keep-unreferenced"], {"placement": "mean", "reg": 0.01, "drop_unreferenced": False})):
        MD.main(["--in", src, "--out", out, "--cell", "1.0", "--device", DEV] + argv)
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        gv, gf, gc, stats = MD.decimate(*MDC.to_dev(DEV, v, f, rgb), cell=1.0, **kw)
        assert open(out, "rb").read() == TM.mesh_ply_bytes(gv, gf, gc) and {k: line[k] for k in stats} == stats and line["faces_out"] == 32
        wv, wf, wc, wstats, _ = MDC.O.decimate(v, f, rgb, cell=1.0, **kw)
        rv, rf, rc = dtu_io.read_ply_mesh_rgb(out)
        assert MDC.same_bits(rv, wv) and np.array_equal(rf, wf) and np.array_equal(rc, wc) and stats == wstats


@pytest.mark.parametrize("sparse", [False, True])
def test_tsdf_mesh_with_decimation_end_to_end_and_its_command_line(tmp_path, capsys, sparse):
    pair_folder, out_folder, summary = MDC.check_end_to_end(DEV, tmp_path, sparse)
    capsys.readouterr()
    ply = str(tmp_path / "cli.ply")
    TM.main(["--pair-folder", pair_folder, "--scan-folder", out_folder, "--out-folder", out_folder, "--mesh", ply, "--resolution", "32", "--decimate-voxels", "2",
             "--device", DEV] + (["--sparse"] if sparse else []))
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    gv, gf = dtu_io.read_ply_mesh(ply)
    d = line["decimate"]
    assert d == summary["decimate"] and d["faces_out"] < d["faces_in"] and line["vertices"] == len(gv) == d["vertices_out"] and line["faces"] == len(gf) == d["faces_out"]
