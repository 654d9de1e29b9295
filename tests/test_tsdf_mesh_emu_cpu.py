"""The TSDF fusion and marching-tetrahedra kernels (csrc/tsdf_mesh.hip) on the CPU emulation of tests/emu, driven through
rc_mvsnet_amd/tsdf_mesh.py on CPU tensors: the cases of tests/test_gpu_tsdf_mesh.py (tests/tsdf_cases.py), every plane, vertex,
colour and face equal to tests/tsdf_oracle.py in every bit.  The emulation runs blocks one after another, so this also pins that
no result depends on the blocks' order.  The C ABI's refusals are checked here too, on the emulated library."""
import ctypes

import numpy as np
import pytest
import torch

import tsdf_cases as C
from rc_mvsnet_amd import _lib, dtu_eval, fusion, tsdf_mesh as TM


@pytest.fixture(autouse=True)
def emu_tm(emu, monkeypatch):
    _lib.bind(emu)                                               # the emu fixture binds the primary header's table; the extensions' too
    monkeypatch.setattr(dtu_eval, "_chk", fusion._chk)           # the mesh super-sampling of the end-to-end case
    monkeypatch.setattr(dtu_eval, "_stream", fusion._stream)
    return emu


@pytest.mark.parametrize("name", C.INTEGRATE)
def test_integration_state_on_emulated_kernel(name):
    C.check_integrate("cpu", name)


def test_chunking_does_not_change_a_bit_on_emulated_kernel():
    C.check_chunking("cpu")


@pytest.mark.parametrize("name", C.EXTRACT)
def test_extraction_on_emulated_kernels(name):
    C.check_extract("cpu", name)


def test_mesh_scan_end_to_end_on_emulated_kernels(tmp_path):
    C.check_end_to_end("cpu", tmp_path)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def test_c_abi_refuses_bad_arguments():
    """every refusal of csrc/tsdf_mesh.h, and nothing written by a refused call"""
    n, H, W, dims = 2, 6, 8, (3, 2, 2)
    vox = 12
    depth, rgb = torch.full((n, H, W), 2.0), torch.full((n, H, W, 3), 7, dtype=torch.uint8)
    planes = [torch.full((vox,), -5.0) for _ in range(5)]
    cam = list(C.cam_row(np.eye(3), (0.0, 0.0, 1.0), 4.0, 4.0, 3.5, 2.5))
    good = dict(depth=_p(depth), rgb=_p(rgb), n=n, H=H, W=W, cams=cam * n, trunc=1.0, grid=[0.0, 0.0, 0.0, 1.0], dims=list(dims),
                dsum=_p(planes[0]), wsum=_p(planes[1]), cr=_p(planes[2]), cg=_p(planes[3]), cb=_p(planes[4]))
    nan, inf = float("nan"), float("inf")

    def integrate(**kw):
        a = dict(good, **kw)
        cams = None if a["cams"] is None else (ctypes.c_double * len(a["cams"]))(*a["cams"])
        grid = None if a["grid"] is None else (ctypes.c_double * 4)(*a["grid"])
        d = None if a["dims"] is None else (ctypes.c_int * 3)(*a["dims"])
        _lib.call("rcmvs_tsdf_integrate", a["depth"], a["rgb"], a["n"], a["H"], a["W"], cams, a["trunc"], grid, d, a["dsum"], a["wsum"], a["cr"],
                  a["cg"], a["cb"], ctypes.c_void_p(0))

    def cams_with(view, k, value):
        c = cam * n
        c[16 * view + k] = value
        return c

    refusals = [({"depth": None}, "null pointer"), ({"cams": None}, "null pointer"), ({"grid": None}, "null pointer"), ({"dims": None}, "null pointer"),
                ({"dsum": None}, "null pointer"), ({"wsum": None}, "null pointer"), ({"cg": None}, "null pointer"),
                ({"dims": [0, 2, 2]}, "bad dims"), ({"dims": [3, -1, 2]}, "bad dims"), ({"dims": [1 << 14, 1 << 14, 2]}, "bad dims"),
                ({"dims": [1 << 16, 1 << 16, 1 << 16]}, "bad dims"),
                ({"H": 0}, "bad image size"), ({"W": -3}, "bad image size"), ({"H": 1 << 16, "W": 1 << 15}, "bad image size"),
                ({"n": 0}, "views"), ({"n": 17}, "views"),
                ({"grid": [0.0, 0.0, 0.0, 0.0]}, "voxel edge"), ({"grid": [0.0, 0.0, 0.0, -1.0]}, "voxel edge"), ({"grid": [0.0, 0.0, 0.0, inf]}, "grid value 3"),
                ({"grid": [0.0, nan, 0.0, 1.0]}, "grid value 1"), ({"grid": [-inf, 0.0, 0.0, 1.0]}, "grid value 0"),
                ({"trunc": 0.0}, "trunc"), ({"trunc": nan}, "trunc"), ({"trunc": inf}, "trunc"),
                ({"cams": cams_with(1, 12, 0.0)}, "camera 1 focal"), ({"cams": cams_with(0, 13, -4.0)}, "camera 0 focal"),
                ({"cams": cams_with(1, 12, inf)}, "camera 1 value 12"), ({"cams": cams_with(0, 4, nan)}, "camera 0 value 4"),
                ({"cams": cams_with(1, 11, -inf)}, "camera 1 value 11"), ({"cams": cams_with(0, 15, nan)}, "camera 0 value 15")]
    for kw, pattern in refusals:
        with pytest.raises(_lib.RcmvsError, match=pattern):
            integrate(**kw)
    assert all(bool((p == -5.0).all()) for p in planes)                          # the refused calls wrote nothing
    integrate(rgb=None)                                                          # rgb may be NULL, and so may the three colour planes
    integrate(cr=None, cg=None, cb=None)
    integrate()
    assert bool((planes[1] != -5.0).any())

    # count and emit
    dsum, wsum = torch.tensor([-1.0, 1.0] * 6), torch.ones(vox)
    mask, tri = torch.full((vox,), 99, dtype=torch.uint8), torch.full((vox,), 99, dtype=torch.uint8)
    work = torch.full((256 + 2,), -7, dtype=torch.int32)
    vs, ts = torch.full((vox + 1,), -7, dtype=torch.int32), torch.full((vox + 1,), -7, dtype=torch.int32)
    totals = torch.full((2,), -7, dtype=torch.int64)
    cgood = dict(dsum=_p(dsum), wsum=_p(wsum), dims=list(dims), mw=1, mask=_p(mask), tri=_p(tri), work=_p(work), vs=_p(vs), ts=_p(ts), totals=_p(totals))

    def count(**kw):
        a = dict(cgood, **kw)
        d = None if a["dims"] is None else (ctypes.c_int * 3)(*a["dims"])
        _lib.call("rcmvs_tsdf_mesh_count", a["dsum"], a["wsum"], d, a["mw"], a["mask"], a["tri"], a["work"], a["vs"], a["ts"], a["totals"], ctypes.c_void_p(0))

    for kw, pattern in [({k: None}, "null pointer") for k in ("dsum", "wsum", "dims", "mask", "tri", "work", "vs", "ts", "totals")] + \
                       [({"dims": [3, 0, 2]}, "bad dims"), ({"dims": [1 << 28, 2, 1]}, "bad dims"), ({"mw": 0}, "min_weight"), ({"mw": -2}, "min_weight")]:
        with pytest.raises(_lib.RcmvsError, match=pattern):
            count(**kw)
    assert bool((mask == 99).all() and (tri == 99).all() and (work == -7).all() and (vs == -7).all() and (ts == -7).all() and (totals == -7).all())
    count()
    nv, nf = (int(t) for t in totals)
    assert nv > 0 and nf > 0 and int(vs[-1]) == nv and int(ts[-1]) == nf

    verts, faces = torch.full((nv, 3), -5.0), torch.full((nf, 3), -7, dtype=torch.int32)
    vrgb = torch.full((nv, 3), 9, dtype=torch.uint8)
    csum = [torch.full((vox,), 100.0) for _ in range(3)]
    egood = dict(dsum=_p(dsum), wsum=_p(wsum), cr=_p(csum[0]), cg=_p(csum[1]), cb=_p(csum[2]), grid=[0.0, 0.0, 0.0, 1.0], dims=list(dims), mw=1,
                 mask=_p(mask), tri=_p(tri), vs=_p(vs), ts=_p(ts), nv=nv, nf=nf, verts=_p(verts), vrgb=_p(vrgb), faces=_p(faces))

    def emit(**kw):
        a = dict(egood, **kw)
        grid = None if a["grid"] is None else (ctypes.c_double * 4)(*a["grid"])
        d = None if a["dims"] is None else (ctypes.c_int * 3)(*a["dims"])
        _lib.call("rcmvs_tsdf_mesh_emit", a["dsum"], a["wsum"], a["cr"], a["cg"], a["cb"], grid, d, a["mw"], a["mask"], a["tri"], a["vs"], a["ts"],
                  a["nv"], a["nf"], a["verts"], a["vrgb"], a["faces"], ctypes.c_void_p(0))

    for kw, pattern in [({k: None}, "null pointer") for k in ("dsum", "wsum", "grid", "dims", "mask", "tri", "vs", "ts", "verts", "faces", "cr")] + \
                       [({"dims": [3, 2, 0]}, "bad dims"), ({"mw": 0}, "min_weight"), ({"grid": [0.0, 0.0, nan, 1.0]}, "grid value 2"),
                        ({"grid": [0.0, 0.0, 0.0, 0.0]}, "voxel edge"), ({"nv": -1}, "vertices"), ({"nf": 1 << 31}, "faces")]:
        with pytest.raises(_lib.RcmvsError, match=pattern):
            emit(**kw)
    assert bool((verts == -5.0).all() and (faces == -7).all() and (vrgb == 9).all())
    emit(vrgb=None, cr=None, cg=None, cb=None)
    assert bool((verts != -5.0).all() and (faces >= 0).all() and (faces < nv).all() and (vrgb == 9).all())
    emit()
    assert bool((vrgb == 100).all())


def test_emit_writes_nothing_beyond_the_totals_it_is_given():
    """nv, nf smaller than the scans say (a caller's mistake): the vertices and faces beyond them are dropped, not written"""
    dims, grid, dsum, wsum, csum, mw = C.planes_for("sphere_12")
    vol = C.load_volume("cpu", dims, grid, dsum, wsum, None)
    edge_mask, tri_count, vert_start, tri_start, (nv, nf) = vol.count(mw)
    verts, faces = torch.full((nv, 3), -5.0), torch.full((nf, 3), -7, dtype=torch.int32)
    g, d = vol._host()
    _lib.call("rcmvs_tsdf_mesh_emit", _p(vol.dsum), _p(vol.wsum), None, None, None, g, d, mw, _p(edge_mask), _p(tri_count), _p(vert_start),
              _p(tri_start), nv - 10, nf - 10, _p(verts), None, _p(faces), ctypes.c_void_p(0))
    want = C.extract_reference("sphere_12")
    assert C.same_bits(verts[:nv - 10].numpy(), want["verts"][:nv - 10]) and np.array_equal(faces[:nf - 10].numpy(), want["faces"][:nf - 10])
    assert bool((verts[nv - 10:] == -5.0).all() and (faces[nf - 10:] == -7).all())
