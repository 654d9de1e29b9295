"""The mesh-texture kernels (csrc/mesh_texture.hip) on the CPU emulation of tests/emu, driven through rc_mvsnet_amd/mesh_texture.py on
CPU tensors: the cases of tests/test_gpu_mesh_texture.py (tests/mesh_texture_cases.py), every best, class, sorted index, table entry,
texel coordinate, owner, atlas byte, counter and textured pixel equal to tests/mesh_texture_oracle.py in every bit.  The emulation
runs blocks one after another, so a kernel that waited for another workgroup would never return here.  The C ABI's refusals are
checked here too, on the emulated library.  GPU only: the dtu_eval scoring of a textured PLY (its searches are slow under the
emulation)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_texture_cases as MTC
from rc_mvsnet_amd import _lib, dtu_eval, fusion, mesh_texture as MT


@pytest.fixture(autouse=True)
def emu_mt(emu, monkeypatch):
    _lib.bind(emu)                                               # the emu fixture binds the primary header's table; the extensions' too
    monkeypatch.setattr(dtu_eval, "_chk", fusion._chk)
    monkeypatch.setattr(dtu_eval, "_stream", fusion._stream)
    return emu


@pytest.mark.parametrize("name", MTC.case_keys())
def test_texture_on_emulated_kernels(name):
    MTC.check_case("cpu", name, twice=name in ("specks_2049", "hostile_coordinates", "hidden_then_open"))


def test_chunks_of_views_on_emulated_kernels():
    MTC.check_chunks("cpu")


def test_max_size_on_emulated_kernels():
    MTC.check_max_size("cpu")


def test_ramp_plane_on_emulated_kernels():
    MTC.check_ramp("cpu")


def test_plane_round_trip_on_emulated_kernels():
    MTC.check_plane_round_trip("cpu")


def test_sphere_on_emulated_kernels():
    MTC.check_sphere("cpu")


def test_refusals_on_the_emulated_path():
    MTC.check_refusals("cpu")


def test_mesh_scan_and_command_lines_on_emulated_kernels(tmp_path):
    MTC.check_mesh_scan("cpu", tmp_path)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


NULL = ctypes.c_void_p(0)


def test_c_abi_refuses_bad_arguments():
    """every refusal of csrc/mesh_texture.h with the argument named, and nothing written by a refused call"""
    s = MTC.case("three_faces_missing_partner")
    verts, faces, rgb = (torch.from_numpy(np.array(s[k])) for k in ("verts", "faces", "rgb"))
    images = torch.from_numpy(np.array(s["images"]))
    V, H, W = images.shape[:3]
    nv, nf = len(verts), len(faces)
    cams = np.ascontiguousarray(s["cams"], np.float64)
    cams_dev = torch.from_numpy(cams.copy())
    host_cams = cams.ctypes.data_as(ctypes.c_void_p)
    fill = {torch.uint8: 99, torch.int32: -7, torch.int64: -7}
    mk = lambda count, dtype: torch.full((count,), fill[dtype], dtype=dtype)                 # noqa: E731
    untouched = lambda *ts: all(bool((t == fill[t.dtype]).all()) for t in ts)               # noqa: E731
    inf, nan = float("inf"), float("nan")

    def refused(call, base, bad):
        for kw, pattern in bad:
            with pytest.raises(_lib.RcmvsError, match=pattern):
                call(**dict(base, **kw))

    sizes = [({"nv": -1}, "nv = -1"), ({"nf": -1}, "nf = -1"), ({"nf": 2 ** 30 - 255}, "nf = 1073741569"), ({"H": 0}, "H = 0"), ({"W": 16385}, "W = 16385"),
             ({"near": 0.0}, "near_z"), ({"near": nan}, "near_z"), ({"near": inf}, "near_z")]

    # vote
    face_image = torch.zeros(H * W, dtype=torch.int32)
    count, best = mk(nf, torch.int32), mk(nf, torch.int64)
    good = dict(verts=_p(verts), faces=_p(faces), nv=nv, nf=nf, n=1, H=H, W=W, cams=host_cams, near=0.5, img=_p(face_image), first=0, reset=1, count=_p(count),
                best=_p(best))
    order = ("verts", "faces", "nv", "nf", "n", "H", "W", "cams", "near", "img", "first", "reset", "count", "best")
    vote = lambda **a: _lib.call("rcmvs_mt_vote", *[a[k] for k in order], NULL)                                              # noqa: E731
    vote_timed = lambda **a: _lib.call("rcmvs_mt_vote_timed", *[a[k] for k in order], a["phase"], NULL, NULL, NULL)        # noqa: E731
    refused(vote, good, sizes + [({"n": 0}, "n = 0"), ({"first": -1}, "first_view = -1"), ({"first": 2 ** 31 - 1}, "first_view = 2147483647"),
                                 ({"best": ctypes.c_void_p(best.data_ptr() + 4)}, "best must be 8-byte aligned"), ({"count": _p(faces)}, "overlaps"),
                                 ({"best": _p(face_image)}, "overlaps"), ({"count": _p(best)}, "overlaps")] +
            [({k: NULL}, "null pointer") for k in ("verts", "faces", "cams", "img", "count", "best")])
    refused(vote_timed, good, [({"phase": 1}, "phase = 1")])
    assert untouched(count, best)
    vote(**good)
    want = MTC.O.vote(s["verts"], s["faces"], face_image.numpy().reshape(1, H, W), cams, 0.5)
    assert best.numpy().view(np.uint64).tolist() == want and want[0] == (H * W << 32 | 0xFFFFFFFF) and want[1:] == [0, 0]
    vote(**dict(good, nv=0, nf=0, verts=NULL, faces=NULL, count=NULL, best=NULL))                   # empty arrays may be NULL

    # layout
    cells = 256
    klass, ka, ia, kb, order_t, hist, start, texel = (mk(nf, torch.int32), mk(nf, torch.int32), mk(nf, torch.int32), mk(nf, torch.int32), mk(nf, torch.int32),
                                                      mk(cells, torch.int32), mk(cells + 1, torch.int32), mk(6 * nf, torch.int32))
    table, stats = mk(MT.TABLE, torch.int64), mk(MT.STATS, torch.int64)
    work = MT._scan_work(cells, "cpu")
    good = dict(verts=_p(verts), faces=_p(faces), nv=nv, nf=nf, V=V, H=H, W=W, cams=_p(cams_dev), near=0.5, best=_p(best), shift=0, klass=_p(klass), ka=_p(ka),
                ia=_p(ia), kb=_p(kb), order=_p(order_t), hist=_p(hist), start=_p(start), work=_p(work), table=_p(table), texel=_p(texel), stats=_p(stats))
    order = ("verts", "faces", "nv", "nf", "V", "H", "W", "cams", "near", "best", "shift", "klass", "ka", "ia", "kb", "order", "hist", "start", "work", "table",
             "texel", "stats")
    lay = lambda **a: _lib.call("rcmvs_mt_layout", *[a[k] for k in order], NULL)                                             # noqa: E731
    lay_timed = lambda **a: _lib.call("rcmvs_mt_layout_timed", *[a[k] for k in order], a["phase"], NULL, NULL, NULL)       # noqa: E731
    refused(lay, good, sizes + [({"V": 0}, "V = 0"), ({"shift": -1}, "shift = -1"), ({"shift": 9}, "shift = 9"), ({"work": NULL}, r"null pointer \(scan_work\)"),
                                ({"work": ctypes.c_void_p(work.data_ptr() + 4)}, "scan_work must be 8-byte aligned"),
                                ({"stats": ctypes.c_void_p(stats.data_ptr() + 4)}, "8-byte aligned"), ({"table": ctypes.c_void_p(table.data_ptr() + 4)}, "8-byte aligned"),
                                ({"kb": _p(ka)}, "overlaps"), ({"order": ctypes.c_void_p(ia.data_ptr() + 4)}, "overlaps"), ({"texel": _p(verts)}, "overlaps"),
                                ({"klass": _p(faces)}, "overlaps"), ({"start": _p(hist)}, "overlaps"), ({"table": _p(best)}, "overlaps"),
                                ({"stats": _p(cams_dev)}, "overlaps")] +
            [({k: NULL}, "null pointer") for k in ("verts", "faces", "cams", "best", "klass", "ka", "ia", "kb", "order", "hist", "start", "table", "texel", "stats")])
    refused(lay_timed, good, [({"phase": -1}, "phase = -1")])
    assert untouched(klass, ka, ia, kb, order_t, hist, start, texel, table, stats)
    lay(**good)
    # face 0 is seen by every sample; its hypotenuse of sqrt(32) pixels is beyond the 5 texels of class 3: class 4; the others are unseen
    ref = MTC.O.layout([4, 2, 2])
    assert klass.tolist() == [4, 2, 2] and order_t.tolist() == [0, 1, 2] and np.array_equal(texel.numpy().reshape(nf, 3, 2), ref[2])
    assert MT.table_dict(table) == ref[1] and MT.stats_dict(stats)["faces_seen"] == 1 and MT.stats_dict(stats)["faces_unseen"] == 2
    lay(**dict(good, nv=0, nf=0, verts=NULL, faces=NULL, best=NULL, klass=NULL, ka=NULL, ia=NULL, kb=NULL, order=NULL, hist=NULL, start=NULL, texel=NULL))
    assert MT.table_dict(table)["total"] == 0 and MT.table_dict(table)["S"] == 1 and MT.table_dict(table)["Sy"] == 1 and stats.tolist() == [0] * MT.STATS
    lay(**good)

    # fill
    S, Sy = 32, 16                                               # one cell of 16 x 16 and one of 4 x 4: 272 texels, 4^5 >= 272, and twice that fits
    assert (ref[1]["S"], ref[1]["Sy"]) == (S, Sy)
    atlas, owner = mk(S * Sy * 3, torch.uint8), mk(S * Sy, torch.int32)
    stats_before = stats.clone()
    good = dict(verts=_p(verts), rgb=_p(rgb), faces=_p(faces), nv=nv, nf=nf, V=V, H=H, W=W, cams=_p(cams_dev), near=0.5, images=_p(images), best=_p(best),
                order=_p(order_t), table=_p(table), S=S, Sy=Sy, bg=0, atlas=_p(atlas), owner=_p(owner), stats=_p(stats))
    order = ("verts", "rgb", "faces", "nv", "nf", "V", "H", "W", "cams", "near", "images", "best", "order", "table", "S", "Sy", "bg", "atlas", "owner", "stats")
    fil = lambda **a: _lib.call("rcmvs_mt_fill", *[a[k] for k in order], NULL)                                               # noqa: E731
    fil_timed = lambda **a: _lib.call("rcmvs_mt_fill_timed", *[a[k] for k in order], a["phase"], NULL, NULL, NULL)         # noqa: E731
    refused(fil, good, sizes + [({"V": 0}, "V = 0"), ({"S": 0}, "S = 0"), ({"S": 6}, "S = 6"), ({"S": 32768, "Sy": 32768}, "S = 32768"), ({"Sy": 2}, "Sy = 2"),
                                ({"S": 1, "Sy": 0}, "Sy = 0"), ({"bg": -1}, "background"), ({"bg": 1 << 24}, "background"), ({"atlas": _p(images)}, "overlaps"),
                                ({"owner": _p(order_t)}, "overlaps"), ({"stats": _p(table)}, "overlaps"), ({"atlas": _p(rgb)}, "overlaps")] +
            [({k: NULL}, "null pointer") for k in ("verts", "faces", "cams", "images", "best", "order", "table", "atlas", "owner", "stats")])
    refused(fil_timed, good, [({"phase": 2}, "phase = 2")])
    assert untouched(atlas, owner) and torch.equal(stats, stats_before)
    fil(**good)
    views = [0, -1, -1]
    want_atlas, want_owner, counts = MTC.O.fill(s["verts"], s["faces"], s["rgb"], s["images"], cams, 0.5, views, ref[0], ref[1], ref[2])
    assert np.array_equal(atlas.numpy().reshape(Sy, S, 3), want_atlas) and np.array_equal(owner.numpy().reshape(Sy, S), want_owner)
    assert {k: MT.stats_dict(stats)[k] for k in counts} == counts and counts["texels_image"] == 16 * 15 // 2 and counts["texels_vertex"] == 6 + 10
    fil(**dict(good, rgb=NULL))                                                                      # no vertex colours: white
    assert (atlas.numpy().reshape(Sy, S, 3)[want_owner >= 1] == 255).all()
    other_atlas, other_owner = mk(16 * 16 * 3, torch.uint8), mk(256, torch.int32)
    fil(**dict(good, S=16, Sy=16, bg=5 | 6 << 8 | 7 << 16, atlas=_p(other_atlas), owner=_p(other_owner)))       # a size the table does not state: background
    assert (other_owner == -1).all() and other_atlas.reshape(-1, 3).unique(dim=0).tolist() == [[5, 6, 7]]
    fil(**good)

    # shade
    out = mk(3 * H * W, torch.uint8)
    good = dict(verts=_p(verts), faces=_p(faces), nv=nv, nf=nf, n=1, H=H, W=W, cams=host_cams, near=0.5, img=_p(face_image), texel=_p(texel), atlas=_p(atlas), S=S,
                Sy=Sy, bg=0, out=_p(out))
    order = ("verts", "faces", "nv", "nf", "n", "H", "W", "cams", "near", "img", "texel", "atlas", "S", "Sy", "bg", "out")
    sh = lambda **a: _lib.call("rcmvs_mt_shade", *[a[k] for k in order], NULL)                                               # noqa: E731
    sh_timed = lambda **a: _lib.call("rcmvs_mt_shade_timed", *[a[k] for k in order], a["phase"], NULL, NULL, NULL)         # noqa: E731
    refused(sh, good, sizes + [({"n": 0}, "n = 0"), ({"S": 3}, "S = 3"), ({"Sy": 8}, "Sy = 8"), ({"Sy": 64}, "Sy = 64"), ({"bg": -1}, "background"), ({"out": _p(atlas)}, "overlaps"),
                               ({"out": _p(face_image)}, "overlaps"), ({"out": _p(texel)}, "overlaps")] +
            [({k: NULL}, "null pointer") for k in ("verts", "faces", "cams", "img", "texel", "atlas", "out")])
    refused(sh_timed, good, [({"phase": 1}, "phase = 1")])
    assert untouched(out)
    sh(**good)
    want = MTC.O.shade(s["verts"], s["faces"], cams, face_image.numpy().reshape(1, H, W), ref[2], want_atlas, 0.5)
    assert np.array_equal(out.numpy().reshape(1, H, W, 3), want)


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("order", ["1", "2"])
def test_other_thread_orders_give_the_same_bytes(order, tmp_path):
    """RCMVS_EMU_ORDER=1|2 schedules every block's threads in another order between synchronisation points: the votes' and the counters'
    atomic adds arrive in another order, and nothing may show.  Run in a child process (the order is read when the library is loaded)."""
    script = tmp_path / "run.py"
    script.write_text(
        "import sys, os\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import torch, conftest\n"
        "import mesh_texture_cases as MTC\n"
        "from rc_mvsnet_amd import _lib\n"
        "lib = conftest.load_emu_lib()\n"
        "conftest.route_to_emulation(lib, setattr)\n"
        "_lib.bind(lib)\n"
        "for name in ('specks_2049', 'hostile_coordinates', 'hidden_everywhere', 'thresholds_shift_1', 'bad_face_image', 'ramp_plane'):\n"
        "    tex = MTC.run('cpu', MTC.case(name))[1]\n"
        "    sys.stdout.write(''.join(tex[k].numpy().tobytes().hex() for k in ('best', 'klass', 'order', 'texel', 'owner', 'atlas')))\n"
        "    sys.stdout.write(repr(tex['stats']) + repr(tex['table']))\n"
        % (REPO, os.path.join(REPO, "tests")))
    outs = []
    for o in ("0", order):
        env = dict(os.environ, RCMVS_EMU_ORDER=o)
        outs.append(subprocess.run([sys.executable, str(script)], env=env, check=True, capture_output=True, text=True).stdout)
    assert len(outs[0]) > 100000 and outs[0] == outs[1]
