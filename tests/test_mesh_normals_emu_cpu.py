"""The mesh-normal kernels (csrc/mesh_normals.hip) on the CPU emulation of tests/emu, driven through rc_mvsnet_amd/mesh_normals.py on
CPU tensors: the cases of tests/test_gpu_mesh_normals.py (tests/mesh_normals_cases.py), every face normal, vertex normal, counter,
normal-map float, smooth byte and colour byte equal to tests/mesh_normals_oracle.py in every bit.  The emulation runs blocks one
after another, so a kernel that waited for another workgroup would never return here.  The C ABI's refusals are checked here too,
on the emulated library.  GPU only: the dtu_eval scoring of a PLY with normals (its searches are slow under the emulation)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_normals_cases as MNC
from rc_mvsnet_amd import _lib, dtu_eval, fusion, mesh_normals as MN


@pytest.fixture(autouse=True)
def emu_mn(emu, monkeypatch):
    _lib.bind(emu)                                               # the emu fixture binds the primary header's table; the extensions' too
    monkeypatch.setattr(dtu_eval, "_chk", fusion._chk)
    monkeypatch.setattr(dtu_eval, "_stream", fusion._stream)
    return emu


@pytest.mark.parametrize("name,weight", MNC.case_keys())
def test_vertex_and_face_normals_on_emulated_kernels(name, weight):
    MNC.check_case("cpu", name, weight, twice=name in ("fan_600", "hostile", "corners_2049"))


def test_face_orders_of_one_strip_on_emulated_kernels():
    MNC.check_orders("cpu")


def test_swapped_faces_on_emulated_kernels():
    MNC.check_flip("cpu")


def test_a_real_extraction_on_emulated_kernels():
    MNC.check_extraction("cpu")


def test_refusals_on_the_emulated_path():
    MNC.check_refusals("cpu")


@pytest.mark.parametrize("name,W,H,cull", MNC.shade_keys())
def test_normal_pass_on_emulated_kernels(name, W, H, cull):
    MNC.check_shade_case("cpu", name, W, H, cull)


def test_a_plane_and_vanishing_normals_on_emulated_kernels():
    MNC.check_plane("cpu")


def test_bad_face_images_on_emulated_kernels():
    MNC.check_bad_face_image("cpu")


def test_smooth_against_flat_on_emulated_kernels():
    MNC.check_smooth_beats_flat("cpu")


def test_mesh_scan_and_command_lines_on_emulated_kernels(tmp_path):
    MNC.check_mesh_scan("cpu", tmp_path)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


NULL = ctypes.c_void_p(0)


def test_c_abi_refuses_bad_arguments():
    """every refusal of csrc/mesh_normals.h with the argument named, and nothing written by a refused call"""
    v, f = MNC.case("one_face")
    verts, faces = torch.from_numpy(np.array(v)), torch.from_numpy(np.array(f))
    nv, nf, n = 3, 1, 3
    fill = {torch.uint8: 99, torch.int32: -7, torch.int64: -7, torch.float32: -7.0}
    mk = lambda count, dtype: torch.full((count,), fill[dtype], dtype=dtype)                 # noqa: E731
    untouched = lambda *ts: all(bool((t == fill[t.dtype]).all()) for t in ts)               # noqa: E731
    table = 256
    ka, ia, kb, ib, hist, start, seg, normals, stats, fnorm = (mk(n, torch.int32), mk(n, torch.int32), mk(n, torch.int32), mk(n, torch.int32), mk(table, torch.int32),
                                                               mk(table + 1, torch.int32), mk(2 * nv, torch.int32), mk(3 * nv, torch.float32), mk(MN.STATS, torch.int64),
                                                               mk(3 * nf, torch.float32))
    work = MN._scan_work(table, "cpu")

    def refused(call, base, bad):
        for kw, pattern in bad:
            with pytest.raises(_lib.RcmvsError, match=pattern):
                call(**dict(base, **kw))

    # vertex normals
    good = dict(verts=_p(verts), faces=_p(faces), nv=nv, nf=nf, weight=0, ka=_p(ka), ia=_p(ia), kb=_p(kb), ib=_p(ib), hist=_p(hist), start=_p(start), work=_p(work),
                seg=_p(seg), normals=_p(normals), stats=_p(stats))
    order = ("verts", "faces", "nv", "nf", "weight", "ka", "ia", "kb", "ib", "hist", "start", "work", "seg", "normals", "stats")
    vn = lambda **a: _lib.call("rcmvs_mn_vertex_normals", *[a[k] for k in order], NULL)                                            # noqa: E731
    vn_timed = lambda **a: _lib.call("rcmvs_mn_vertex_normals_timed", *[a[k] for k in order], a.get("phase", 0), NULL, NULL, NULL)  # noqa: E731
    refused(vn, good, [({"nv": -1}, "nv = -1"), ({"nf": -1}, "nf = -1"), ({"nf": (2 ** 31 - 256) // 3 + 1}, "nf = 715827798"), ({"weight": 2}, "weight = 2"),
                       ({"weight": -1}, "weight = -1"), ({"stats": NULL}, r"null pointer \(stats\)"), ({"work": NULL}, r"null pointer \(scan_work\)"),
                       ({"work": ctypes.c_void_p(work.data_ptr() + 4)}, "scan_work must be 8-byte aligned"),
                       ({"stats": ctypes.c_void_p(stats.data_ptr() + 4)}, "stats must be 8-byte aligned"),
                       ({"kb": _p(ka)}, "overlaps"), ({"ib": ctypes.c_void_p(ia.data_ptr() + 4)}, "overlaps"), ({"normals": _p(verts)}, "overlaps"),
                       ({"seg": _p(faces)}, "overlaps"), ({"start": _p(hist)}, "overlaps"), ({"stats": _p(seg)}, "overlaps")] +
            [({k: NULL}, "null pointer") for k in ("verts", "faces", "ka", "ia", "kb", "ib", "hist", "start", "seg", "normals")])
    refused(vn_timed, good, [({"phase": 3}, "phase = 3"), ({"phase": -1}, "phase = -1")])
    assert untouched(ka, ia, kb, ib, hist, start, seg, normals, stats)
    for weight, name in ((0, "area"), (1, "sphere")):
        vn(**dict(good, weight=weight))
        want, wstats = MNC.reference("one_face", name)
        assert np.array_equal(MNC.bits(normals.numpy().reshape(3, 3)), MNC.bits(want)) and stats.tolist() == [0, 0, 0, 0, 3, 0, 0, 0]
    vn(**dict(good, nv=0, nf=0, verts=NULL, faces=NULL, ka=NULL, ia=NULL, kb=NULL, ib=NULL, hist=NULL, start=NULL, seg=NULL, normals=NULL))     # empty arrays may be NULL
    assert stats.tolist() == [0] * 8

    # face normals
    good = dict(verts=_p(verts), faces=_p(faces), nv=nv, nf=nf, out=_p(fnorm))
    fnc = lambda **a: _lib.call("rcmvs_mn_face_normals", a["verts"], a["faces"], a["nv"], a["nf"], a["out"], NULL)                              # noqa: E731
    fn_timed = lambda **a: _lib.call("rcmvs_mn_face_normals_timed", a["verts"], a["faces"], a["nv"], a["nf"], a["out"], a["phase"], NULL, NULL, NULL)  # noqa: E731
    refused(fnc, good, [({"nv": -1}, "nv = -1"), ({"nf": -2}, "nf = -2"), ({"verts": NULL}, r"null pointer \(verts\)"), ({"faces": NULL}, r"null pointer \(faces\)"),
                        ({"out": NULL}, r"null pointer \(face_normals\)"), ({"out": _p(verts)}, "overlaps"), ({"out": _p(faces)}, "overlaps"),
                        ({"out": ctypes.c_void_p(fnorm.data_ptr() + 2)}, "4-byte aligned")])
    refused(fn_timed, good, [({"phase": 1}, "phase = 1")])
    assert untouched(fnorm)
    fnc(**good)
    assert np.array_equal(MNC.bits(fnorm.numpy().reshape(1, 3)), MNC.bits(MNC.reference_faces("one_face")))

    # the normal pass
    H, W = 3, 4
    cam = np.ascontiguousarray(MNC.MRC.PIX[None], np.float64)
    img = torch.zeros(H * W, dtype=torch.int32)
    vnorm = torch.from_numpy(np.array(MNC.reference("one_face", "area")[0]))
    nmap, smooth, nrgb = mk(3 * H * W, torch.float32), mk(H * W, torch.uint8), mk(3 * H * W, torch.uint8)
    good = dict(verts=_p(verts), faces=_p(faces), vnorm=_p(vnorm), nv=nv, nf=nf, n=1, H=H, W=W, cams=cam.ctypes.data_as(ctypes.c_void_p), near=0.5, img=_p(img), bg=0,
                nmap=_p(nmap), smooth=_p(smooth), nrgb=_p(nrgb))
    order = ("verts", "faces", "vnorm", "nv", "nf", "n", "H", "W", "cams", "near", "img", "bg", "nmap", "smooth", "nrgb")
    sh = lambda **a: _lib.call("rcmvs_mn_shade", *[a[k] for k in order], NULL)                                            # noqa: E731
    sh_timed = lambda **a: _lib.call("rcmvs_mn_shade_timed", *[a[k] for k in order], a["phase"], NULL, NULL, NULL)      # noqa: E731
    inf, nan = float("inf"), float("nan")
    refused(sh, good, [({"nv": -1}, "nv = -1"), ({"nf": -1}, "nf = -1"), ({"n": 0}, "n = 0"), ({"H": 0}, "H = 0"), ({"W": 16385}, "W = 16385"), ({"near": 0.0}, "near_z"),
                       ({"near": nan}, "near_z"), ({"near": inf}, "near_z"), ({"bg": -1}, "background"), ({"bg": 1 << 24}, "background"),
                       ({"nmap": _p(verts)}, "overlaps"), ({"smooth": ctypes.c_void_p(nrgb.data_ptr() + 5)}, "overlaps"), ({"nrgb": _p(img)}, "overlaps"),
                       ({"nmap": _p(vnorm)}, "overlaps"), ({"nmap": ctypes.c_void_p(nmap.data_ptr() + 2)}, "4-byte aligned")] +
            [({k: NULL}, "null pointer") for k in ("verts", "faces", "vnorm", "cams", "img", "nmap", "smooth", "nrgb")])
    refused(sh_timed, good, [({"phase": 2}, "phase = 2")])
    assert untouched(nmap, smooth, nrgb)
    sh(**good)
    want = MNC.O.shade(v, f, vnorm.numpy(), cam, img.numpy().reshape(1, H, W), 0.5)
    assert np.array_equal(MNC.bits(nmap.numpy().reshape(1, H, W, 3)), MNC.bits(want["normal"])) and np.array_equal(smooth.numpy().reshape(1, H, W), want["smooth"])
    assert np.array_equal(nrgb.numpy().reshape(1, H, W, 3), want["normal_rgb"])


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("order", ["1", "2"])
def test_other_thread_orders_give_the_same_bytes(order, tmp_path):
    """RCMVS_EMU_ORDER=1|2 schedules every block's threads in another order between synchronisation points: the counters' atomic
    adds arrive in another order, and nothing may show.  Run in a child process (the order is read when the library is loaded)."""
    script = tmp_path / "run.py"
    script.write_text(
        "import sys, os\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import torch, conftest\n"
        "import mesh_normals_cases as MNC\n"
        "from rc_mvsnet_amd import _lib, mesh_normals as MN\n"
        "lib = conftest.load_emu_lib()\n"
        "conftest.route_to_emulation(lib, setattr)\n"
        "_lib.bind(lib)\n"
        "for name in ('corners_2049', 'fan_600', 'hostile', 'degenerate', 'nv_300', 'uv_sphere'):\n"
        "    v, f = MNC.case(name)\n"
        "    tv, tf = torch.from_numpy(v.copy()), torch.from_numpy(f.copy())\n"
        "    for w in MNC.WEIGHTS:\n"
        "        n, s = MN.vertex_normals_device(tv, tf, w)\n"
        "        sys.stdout.write(n.numpy().tobytes().hex() + s.numpy().tobytes().hex())\n"
        "    sys.stdout.write(MN.face_normals(tv, tf).numpy().tobytes().hex())\n"
        "v, f, c, cams = MNC.MRC.case('fan64')\n"
        "face = torch.from_numpy(MNC.MRC.reference('fan64', 64, 48, 'none')['face'].copy())\n"
        "out = MN.shade(torch.from_numpy(v.copy()), torch.from_numpy(f.copy()), torch.from_numpy(MNC.shade_normals('fan64').copy()), cams, face, near=MNC.MRC.NEAR)\n"
        "sys.stdout.write(''.join(out[k].numpy().tobytes().hex() for k in ('normal', 'smooth', 'normal_rgb')))\n"
        % (REPO, os.path.join(REPO, "tests")))
    outs = []
    for o in ("0", order):
        env = dict(os.environ, RCMVS_EMU_ORDER=o)
        outs.append(subprocess.run([sys.executable, str(script)], env=env, check=True, capture_output=True, text=True).stdout)
    assert len(outs[0]) > 100000 and outs[0] == outs[1]
