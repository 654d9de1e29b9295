"""The block-sparse TSDF kernels (csrc/tsdf_sparse.hip) on the CPU emulation of tests/emu, driven through rc_mvsnet_amd/tsdf_mesh.py
on CPU tensors: the cases of tests/test_gpu_tsdf_sparse.py (tests/tsdf_sparse_cases.py), every flag, rank, plane, vertex, colour
and face equal to tests/tsdf_sparse_oracle.py in every bit.  The emulation runs blocks one after another, so this also pins that
no result depends on the blocks' order.  The C ABI's refusals are checked here too, on the emulated library."""
import ctypes

import numpy as np
import pytest
import torch

import tsdf_cases as C
import tsdf_sparse_cases as SC
import tsdf_sparse_oracle as S
from rc_mvsnet_amd import _lib, dtu_eval, fusion, tsdf_mesh as TM


@pytest.fixture(autouse=True)
def emu_tm(emu, monkeypatch):
    _lib.bind(emu)                                               # the emu fixture binds the primary header's table; the extensions' too
    monkeypatch.setattr(dtu_eval, "_chk", fusion._chk)           # the mesh super-sampling of the end-to-end case
    monkeypatch.setattr(dtu_eval, "_stream", fusion._stream)
    return emu


@pytest.mark.parametrize("name", SC.MARK)
def test_marking_on_emulated_kernel(name):
    SC.check_mark("cpu", name)


@pytest.mark.parametrize("name", list(SC.BUILD))
def test_build_on_emulated_kernels(name):
    SC.check_build("cpu", name)


def test_calls_out_of_order_and_an_empty_block_set_are_refused():
    SC.check_call_order("cpu")


@pytest.mark.parametrize("name", C.INTEGRATE)
def test_integration_state_on_emulated_kernel(name):
    SC.check_integrate("cpu", name)


def test_chunking_does_not_change_a_bit_on_emulated_kernel():
    SC.check_chunking("cpu")


def test_integration_equals_the_dense_kernel_on_emulated_kernels():
    SC.check_integrate_against_dense_kernel("cpu", "views_3")


@pytest.mark.parametrize("name", SC.EXTRACT)
def test_extraction_on_emulated_kernels(name):
    SC.check_extract("cpu", name)


@pytest.mark.parametrize("name", ["5x4x4", "6x6x6_h_0.1"])
def test_sparse_mesh_is_the_dense_mesh_on_emulated_kernels(name):
    SC.check_scene_on_the_kernels("cpu", name)


def test_mesh_scan_sparse_end_to_end_on_emulated_kernels(tmp_path):
    SC.check_end_to_end("cpu", tmp_path)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _arr(kind, values):
    return None if values is None else (kind * len(values))(*values)


NULL = ctypes.c_void_p(0)


def test_c_abi_refuses_bad_arguments():
    """every refusal of csrc/tsdf_sparse.h, and nothing written by a refused call"""
    n, H, W, bdims = 2, 6, 8, (2, 1, 1)
    nan, inf = float("nan"), float("inf")
    depth, rgb = torch.full((n, H, W), 2.0), torch.full((n, H, W, 3), 7, dtype=torch.uint8)
    cam = list(C.cam_row(np.eye(3), (-4.0, -4.0, 1.0), 4.0, 4.0, 3.5, 2.5))

    def cams_with(view, k, value):
        c = cam * n
        c[16 * view + k] = value
        return c

    views = [({"depth": None}, "null pointer"), ({"cams": None}, "null pointer"), ({"grid": None}, "null pointer"), ({"bdims": None}, "null pointer"),
             ({"bdims": [0, 1, 1]}, "bad bdims"), ({"bdims": [2, -1, 1]}, "bad bdims"), ({"bdims": [1 << 14, 1 << 14, 2]}, "bad bdims"),
             ({"bdims": [1 << 16, 1 << 16, 1 << 16]}, "bad bdims"),
             ({"H": 0}, "bad image size"), ({"W": -3}, "bad image size"), ({"H": 1 << 16, "W": 1 << 15}, "bad image size"),
             ({"n": 0}, "views"), ({"n": 17}, "views"),
             ({"grid": [0.0, 0.0, 0.0, 0.0]}, "voxel edge"), ({"grid": [0.0, 0.0, 0.0, -1.0]}, "voxel edge"), ({"grid": [0.0, 0.0, 0.0, inf]}, "grid value 3"),
             ({"grid": [0.0, nan, 0.0, 1.0]}, "grid value 1"), ({"grid": [-inf, 0.0, 0.0, 1.0]}, "grid value 0"),
             ({"trunc": 0.0}, "trunc"), ({"trunc": nan}, "trunc"), ({"trunc": inf}, "trunc"),
             ({"cams": cams_with(1, 12, 0.0)}, "camera 1 focal"), ({"cams": cams_with(0, 13, -4.0)}, "camera 0 focal"),
             ({"cams": cams_with(1, 12, inf)}, "camera 1 value 12"), ({"cams": cams_with(0, 4, nan)}, "camera 0 value 4")]

    # mark
    flags, skipped = torch.full((2,), 9, dtype=torch.uint8), torch.full((1,), -7, dtype=torch.int64)
    mgood = dict(depth=_p(depth), n=n, H=H, W=W, cams=cam * n, trunc=1.0, grid=[0.0, 0.0, 0.0, 1.0], bdims=list(bdims), flags=_p(flags), skipped=_p(skipped))

    def mark(**kw):
        a = dict(mgood, **kw)
        _lib.call("rcmvs_tsdf_sp_mark", a["depth"], a["n"], a["H"], a["W"], _arr(ctypes.c_double, a["cams"]), a["trunc"], _arr(ctypes.c_double, a["grid"]),
                  _arr(ctypes.c_int, a["bdims"]), a["flags"], a["skipped"], NULL)

    for kw, pattern in views + [({"flags": None}, "null pointer"), ({"skipped": None}, "null pointer")]:
        with pytest.raises(_lib.RcmvsError, match=pattern):
            mark(**kw)
    assert bool((flags == 9).all()) and int(skipped) == -7                       # the refused calls wrote nothing
    flags.zero_()
    skipped.zero_()
    mark()
    assert flags.tolist() == [1, 1] and int(skipped) == 0                    # x from 1 - h to 7 + h: both blocks

    # build
    words, rank = torch.full((1,), -7, dtype=torch.int32), torch.full((2,), -7, dtype=torch.int32)
    active, work = torch.full((2,), -7, dtype=torch.int32), torch.full((1,), -7, dtype=torch.int32)
    bgood = dict(flags=_p(flags), bdims=list(bdims), words=_p(words), rank=_p(rank), active=_p(active), cap=2, work=_p(work))

    def build(**kw):
        a = dict(bgood, **kw)
        _lib.call("rcmvs_tsdf_sp_build", a["flags"], _arr(ctypes.c_int, a["bdims"]), a["words"], a["rank"], a["active"], a["cap"], a["work"], NULL)

    for kw, pattern in [({k: None}, "null pointer") for k in ("flags", "bdims", "words", "rank", "active", "work")] + \
                       [({"bdims": [2, 0, 1]}, "bad bdims"), ({"bdims": [1 << 27, 2, 1]}, "bad bdims"), ({"cap": 0}, "active_capacity")]:
        with pytest.raises(_lib.RcmvsError, match=pattern):
            build(**kw)
    assert bool((words == -7).all() and (rank == -7).all() and (active == -7).all() and (work == -7).all())
    flags.fill_(1)
    build(cap=1)                                                                 # only the first active_capacity entries are written
    assert words.tolist() == [3] and rank.tolist() == [0, 2] and active.tolist() == [0, -7]
    build()
    assert active.tolist() == [0, 1]

    # integrate
    vox = 1024
    planes = [torch.full((vox,), -5.0) for _ in range(5)]
    igood = dict(mgood, rgb=_p(rgb), active=_p(active), na=2, dsum=_p(planes[0]), wsum=_p(planes[1]), cr=_p(planes[2]), cg=_p(planes[3]), cb=_p(planes[4]))

    def integrate(**kw):
        a = dict(igood, **kw)
        _lib.call("rcmvs_tsdf_sp_integrate", a["depth"], a["rgb"], a["n"], a["H"], a["W"], _arr(ctypes.c_double, a["cams"]), a["trunc"],
                  _arr(ctypes.c_double, a["grid"]), _arr(ctypes.c_int, a["bdims"]), a["active"], a["na"], a["dsum"], a["wsum"], a["cr"], a["cg"], a["cb"], NULL)

    for kw, pattern in views + [({"active": None}, "null pointer"), ({"dsum": None}, "null pointer"), ({"wsum": None}, "null pointer"),
                                ({"cg": None}, "null pointer"), ({"na": 0}, "active blocks"), ({"na": 3}, "active blocks"), ({"na": -1}, "active blocks")]:
        with pytest.raises(_lib.RcmvsError, match=pattern):
            integrate(**kw)
    assert all(bool((p == -5.0).all()) for p in planes)
    integrate(rgb=None)
    integrate(cr=None, cg=None, cb=None)
    integrate()
    assert bool((planes[1] != -5.0).any())

    # count and emit
    dsum, wsum = torch.tensor([-1.0, 1.0] * (vox // 2)), torch.ones(vox)
    mask, tri = torch.full((vox,), 99, dtype=torch.uint8), torch.full((vox,), 99, dtype=torch.uint8)
    cwork = torch.full((1024 + 4,), -7, dtype=torch.int32)
    vs, ts = torch.full((vox + 1,), -7, dtype=torch.int32), torch.full((vox + 1,), -7, dtype=torch.int32)
    totals = torch.full((2,), -7, dtype=torch.int64)
    cgood = dict(dsum=_p(dsum), wsum=_p(wsum), bdims=list(bdims), words=_p(words), rank=_p(rank), active=_p(active), na=2, mw=1, mask=_p(mask), tri=_p(tri),
                 work=_p(cwork), vs=_p(vs), ts=_p(ts), totals=_p(totals))

    def count(**kw):
        a = dict(cgood, **kw)
        _lib.call("rcmvs_tsdf_sp_mesh_count", a["dsum"], a["wsum"], _arr(ctypes.c_int, a["bdims"]), a["words"], a["rank"], a["active"], a["na"], a["mw"],
                  a["mask"], a["tri"], a["work"], a["vs"], a["ts"], a["totals"], NULL)

    for kw, pattern in [({k: None}, "null pointer") for k in ("dsum", "wsum", "bdims", "words", "rank", "active", "mask", "tri", "work", "vs", "ts", "totals")] + \
                       [({"bdims": [2, 0, 1]}, "bad bdims"), ({"mw": 0}, "min_weight"), ({"mw": -2}, "min_weight"), ({"na": 0}, "active blocks"),
                        ({"na": 3}, "active blocks"), ({"na": (1 << 19) + 1, "bdims": [1 << 20, 1, 1]}, "active blocks"),
                        ({"work": ctypes.c_void_p(cwork.data_ptr() + 4)}, "8-byte aligned")]:
        with pytest.raises(_lib.RcmvsError, match=pattern):
            count(**kw)
    assert bool((mask == 99).all() and (tri == 99).all() and (cwork == -7).all() and (vs == -7).all() and (ts == -7).all() and (totals == -7).all())
    count()
    nv, nf = (int(t) for t in totals)
    assert nv > 0 and nf > 0 and int(vs[-1]) == nv and int(ts[-1]) == nf

    verts, faces = torch.full((nv, 3), -5.0), torch.full((nf, 3), -7, dtype=torch.int32)
    vrgb = torch.full((nv, 3), 9, dtype=torch.uint8)
    csum = [torch.full((vox,), 100.0) for _ in range(3)]
    egood = dict(cgood, cr=_p(csum[0]), cg=_p(csum[1]), cb=_p(csum[2]), grid=[0.0, 0.0, 0.0, 1.0], nv=nv, nf=nf, verts=_p(verts), vrgb=_p(vrgb), faces=_p(faces))

    def emit(**kw):
        a = dict(egood, **kw)
        _lib.call("rcmvs_tsdf_sp_mesh_emit", a["dsum"], a["wsum"], a["cr"], a["cg"], a["cb"], _arr(ctypes.c_double, a["grid"]), _arr(ctypes.c_int, a["bdims"]),
                  a["words"], a["rank"], a["active"], a["na"], a["mw"], a["mask"], a["tri"], a["vs"], a["ts"], a["nv"], a["nf"], a["verts"], a["vrgb"],
                  a["faces"], NULL)

    for kw, pattern in [({k: None}, "null pointer") for k in ("dsum", "wsum", "grid", "bdims", "words", "rank", "active", "mask", "tri", "vs", "ts", "verts",
                                                               "faces", "cr")] + \
                       [({"bdims": [2, 1, 0]}, "bad bdims"), ({"mw": 0}, "min_weight"), ({"grid": [0.0, 0.0, nan, 1.0]}, "grid value 2"),
                        ({"grid": [0.0, 0.0, 0.0, 0.0]}, "voxel edge"), ({"nv": -1}, "vertices"), ({"nf": 1 << 31}, "faces"), ({"na": 0}, "active blocks")]:
        with pytest.raises(_lib.RcmvsError, match=pattern):
            emit(**kw)
    assert bool((verts == -5.0).all() and (faces == -7).all() and (vrgb == 9).all())
    emit(vrgb=None, cr=None, cg=None, cb=None)
    assert bool((verts != -5.0).all() and (faces >= 0).all() and (faces < nv).all() and (vrgb == 9).all())
    emit()
    assert bool((vrgb == 100).all())


def test_a_block_number_outside_the_grid_is_ignored():
    """active[] is the caller's: an entry that is no block of the grid makes no kernel read or write anything for it"""
    bdims, grid = (2, 1, 1), (0.0, 0.0, 0.0, 1.0)
    vol = SC.chosen_volume("cpu", grid, bdims, [0, 1])
    vol.active[1] = 7
    depth, cams = torch.full((1, 6, 8), 4.0), C.cam_row(np.eye(3), (-4.0, -4.0, 1.0), 4.0, 4.0, 3.5, 2.5)[None]
    vol.integrate(depth, cams, None, trunc=2.0)
    assert bool((vol.wsum[:512] > 0).any()) and not bool(vol.wsum[512:].any())
    edge_mask, tri_count, vert_start, tri_start, (nv, nf) = vol.count(1)
    assert not bool(edge_mask[512:].any()) and not bool(tri_count[512:].any())
    verts, faces, _ = vol.extract(1)
    assert len(verts) == nv and len(faces) == nf
