"""The rasteriser's kernels (csrc/mesh_render.hip) on the CPU emulation of tests/emu, driven through rc_mvsnet_amd/mesh_render.py on
CPU tensors: the cases of tests/test_gpu_mesh_render.py (tests/mesh_render_cases.py), every key, depth, face number, colour byte,
shade byte and counter equal to tests/mesh_render_oracle.py in every bit.  The emulation runs blocks one after another, so a kernel
that waited for another workgroup would never return here.  The C ABI's refusals are checked here too, on the emulated library."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_render_cases as MRC
from rc_mvsnet_amd import _lib, dtu_eval, fusion, mesh_render as MR


@pytest.fixture(autouse=True)
def emu_mr(emu, monkeypatch):
    _lib.bind(emu)                                               # the emu fixture binds the primary header's table; the extensions' too
    monkeypatch.setattr(dtu_eval, "_chk", fusion._chk)
    monkeypatch.setattr(dtu_eval, "_stream", fusion._stream)
    return emu


@pytest.mark.parametrize("name,W,H,cull", MRC.case_keys())
def test_render_on_emulated_kernels(name, W, H, cull):
    MRC.check_case("cpu", name, W, H, cull, twice=(W, H) == (7, 5))


def test_white_faces_and_background_on_emulated_kernels():
    MRC.check_without_colours_and_background("cpu")


def test_permuted_and_reversed_faces_on_emulated_kernels():
    MRC.check_permutation("cpu")


def test_views_in_one_call_and_one_by_one_on_emulated_kernels():
    MRC.check_views_one_by_one("cpu")


def test_a_list_longer_than_the_large_grid_on_emulated_kernels():
    MRC.check_large_path_alone("cpu")


def test_compare_on_emulated_kernels():
    MRC.check_compare("cpu")


def test_refusals_on_the_emulated_path():
    MRC.check_refusals("cpu")


def test_round_trip_on_the_sphere_scene_on_emulated_kernels():
    MRC.check_round_trip("cpu")


def test_mesh_scan_without_render_is_what_it_was_and_command_line_round_trip_on_emulated_kernels(tmp_path):
    MRC.check_command_line_round_trip("cpu", tmp_path)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


NULL = ctypes.c_void_p(0)


def test_c_abi_refuses_bad_arguments():
    """every refusal of csrc/mesh_render.h with the argument named, and nothing written by a refused call"""
    v, f, c, cams = MRC.case("right_triangle")
    verts, faces, rgb = (torch.from_numpy(np.array(a)) for a in (v, f, c))
    nv, nf, n, H, W = 3, 1, 1, 5, 7
    cam = np.ascontiguousarray(cams, np.float64)
    fill = {torch.uint8: 99, torch.int32: -7, torch.int64: -7, torch.float32: -7.0, torch.float64: -7.0}
    mk = lambda count, dtype: torch.full((count,), fill[dtype], dtype=dtype)                 # noqa: E731
    untouched = lambda *ts: all(bool((t == fill[t.dtype]).all()) for t in ts)               # noqa: E731
    px = n * H * W
    proj, work, keys, depth, face, orgb, shade, stats, trace = (mk(3 * nv, torch.int64), mk(nf + 1, torch.int32), mk(px, torch.int64), mk(px, torch.float32),
                                                                mk(px, torch.int32), mk(3 * px, torch.uint8), mk(px, torch.uint8), mk(8 * n, torch.int64),
                                                                mk(MR.TRACE, torch.int64))
    good = dict(verts=_p(verts), rgb=_p(rgb), faces=_p(faces), nv=nv, nf=nf, n=n, H=H, W=W, cams=cam.ctypes.data_as(ctypes.c_void_p), near=0.5, cull=0, bg=0,
                proj=_p(proj), work=_p(work), keys=_p(keys), depth=_p(depth), face=_p(face), orgb=_p(orgb), shade=_p(shade), stats=_p(stats), trace=NULL)
    order = ("verts", "rgb", "faces", "nv", "nf", "n", "H", "W", "cams", "near", "cull", "bg", "proj", "work", "keys", "depth", "face", "orgb", "shade", "stats",
             "trace")
    render = lambda **a: _lib.call("rcmvs_mr_render", *[a[k] for k in order], NULL)                                     # noqa: E731
    timed = lambda **a: _lib.call("rcmvs_mr_render_timed", *[a[k] for k in order], a.get("phase", 0), NULL, NULL, NULL)  # noqa: E731

    def refused(call, base, bad):
        for kw, pattern in bad:
            with pytest.raises(_lib.RcmvsError, match=pattern):
                call(**dict(base, **kw))

    inf, nan = float("inf"), float("nan")
    refused(render, good, [({"H": 0}, "H = 0"), ({"W": 0}, "W = 0"), ({"H": MR.MAX_SIDE + 1}, "H = 16385"), ({"W": MR.MAX_SIDE + 1}, "W = 16385"),
                           ({"H": -1}, "H = -1"), ({"near": 0.0}, "near_z"), ({"near": -0.5}, "near_z"), ({"near": nan}, "near_z"), ({"near": inf}, "near_z"),
                           ({"n": 0}, "n = 0"), ({"n": -1}, "n = -1"), ({"verts": NULL, "nv": 0}, "rgb needs verts"), ({"cull": 2}, "cull"),
                           ({"bg": -1}, "background"), ({"bg": 1 << 24}, "background"), ({"nv": -1}, "vertices"), ({"nf": -1}, "faces"),
                           ({"depth": _p(face)}, "overlaps"), ({"shade": ctypes.c_void_p(orgb.data_ptr() + 5)}, "overlaps"), ({"keys": _p(proj)}, "overlaps"),
                           ({"stats": _p(keys)}, "overlaps"), ({"orgb": _p(rgb)}, "overlaps"), ({"work": _p(faces)}, "overlaps"), ({"trace": _p(stats)}, "overlaps"),
                           ({"keys": ctypes.c_void_p(keys.data_ptr() + 4)}, "8-byte aligned")] +
            [({k: NULL}, "null pointer") for k in ("verts", "faces", "cams", "proj", "work", "keys", "depth", "face", "orgb", "shade", "stats")])
    refused(timed, good, [({"phase": 5}, "phase"), ({"phase": -1}, "phase")])
    assert untouched(proj, work, keys, depth, face, orgb, shade, stats, trace)
    render(**dict(good, trace=_p(trace)))
    want = MRC.reference("right_triangle", W, H, "none")
    assert np.array_equal(keys.numpy().view(np.uint64).reshape(H, W), want["keys"][0]) and np.array_equal(face.numpy().reshape(H, W), want["face"][0])
    assert stats.tolist() == [1, 0, 0, 0, 0, 0, 10, 0] and work[0] == 0
    # 15 samples in the box, 10 inside and as many atomics on the untouched image; -7 + the count
    assert trace.tolist() == [-7 + 10, -7 + 10, -7, -7, -7, -7, -7 + 1, -7, -7, -7]
    render(**dict(good, rgb=NULL))                                 # white without vertex colours
    assert set(orgb.tolist()) == {0, 255}

    # compare
    r, d = MRC.compare_inputs(1, 3, 5)
    tr, td = torch.from_numpy(r), torch.from_numpy(d)
    th = (ctypes.c_double * 3)(0.001, 0.01, 0.05)
    partial, table = mk(1, torch.float64), mk(8, torch.int64)
    good = dict(r=_p(tr), d=_p(td), n=1, H=3, W=5, th=ctypes.cast(th, ctypes.c_void_p), nt=3, partial=_p(partial), table=_p(table))
    cmp_ = lambda **a: _lib.call("rcmvs_mr_compare", a["r"], a["d"], a["n"], a["H"], a["W"], a["th"], a["nt"], a["partial"], a["table"], NULL)      # noqa: E731
    bad_th = (ctypes.c_double * 3)(0.001, -0.01, 0.05)
    nan_th = (ctypes.c_double * 3)(nan, 0.01, 0.05)
    refused(cmp_, good, [({"H": 0}, "H = 0"), ({"W": MR.MAX_SIDE + 1}, "W = 16385"), ({"n": 0}, "n = 0"), ({"n": MR.CMP_MAX_VIEWS + 1}, "n = 65536"), ({"nt": 4}, "nt = 4"), ({"nt": -1}, "nt = -1"),
                         ({"th": ctypes.cast(bad_th, ctypes.c_void_p)}, r"thresholds\[1\]"), ({"th": ctypes.cast(nan_th, ctypes.c_void_p)}, r"thresholds\[0\]"),
                         ({"table": _p(tr)}, "overlaps"), ({"partial": _p(td)}, "overlaps")] +
            [({k: NULL}, "null pointer") for k in ("r", "d", "th", "partial", "table")])
    assert untouched(partial, table)
    cmp_(**good)
    row = MR.table_rows(table.reshape(1, 8), (0.001, 0.01, 0.05))
    MRC.assert_rows(row, MRC.O.compare(r, d, (0.001, 0.01, 0.05)), "abi")
    cmp_(**dict(good, nt=0, th=NULL))


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("order", ["1", "2"])
def test_other_thread_orders_give_the_same_bytes(order, tmp_path):
    """RCMVS_EMU_ORDER=1|2 schedules every block's threads in another order between synchronisation points: the atomic minima and
    the appends to the list of large faces arrive in another order, and must not show.  Run in a child process (the order is read
    when the library is loaded)."""
    script = tmp_path / "run.py"
    script.write_text(
        "import sys, os\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import torch, conftest\n"
        "import mesh_render_cases as MRC\n"
        "from rc_mvsnet_amd import _lib, mesh_render as MR\n"
        "lib = conftest.load_emu_lib()\n"
        "conftest.route_to_emulation(lib, setattr)\n"
        "_lib.bind(lib)\n"
        "for name in ('random_scene', 'coplanar_twins', 'sizes_of_boxes', 'fan64', 'three_views'):\n"
        "    out = MRC.run('cpu', name, 64, 48)\n"
        "    sys.stdout.write(''.join(out[k].numpy().tobytes().hex() for k in ('keys', 'depth', 'face', 'rgb', 'shade', 'stats')))\n"
        % (REPO, os.path.join(REPO, "tests")))
    outs = []
    for o in ("0", order):
        env = dict(os.environ, RCMVS_EMU_ORDER=o)
        outs.append(subprocess.run([sys.executable, str(script)], env=env, check=True, capture_output=True, text=True).stdout)
    assert len(outs[0]) > 100000 and outs[0] == outs[1]
