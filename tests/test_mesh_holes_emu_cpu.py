"""The hole-filling kernels (csrc/mesh_holes.hip) on the CPU emulation of tests/emu, driven through rc_mvsnet_amd/mesh_holes.py on
CPU tensors: the cases of tests/test_gpu_mesh_holes.py (tests/mesh_holes_cases.py), every successor, flag, counter, position,
colour and face equal to tests/mesh_holes_oracle.py in every bit.  The emulation runs blocks one after another, so a kernel that
waited for another workgroup would never return here.  The C ABI's refusals are checked here too, on the emulated library."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import mesh_holes_cases as MHC
from rc_mvsnet_amd import _lib, dtu_eval, fusion, mesh_holes as MH


@pytest.fixture(autouse=True)
def emu_mh(emu, monkeypatch):
    _lib.bind(emu)                                               # the emu fixture binds the primary header's table; the extensions' too
    monkeypatch.setattr(dtu_eval, "_chk", fusion._chk)
    monkeypatch.setattr(dtu_eval, "_stream", fusion._stream)
    return emu


@pytest.mark.parametrize("name,k", MHC.case_keys())
def test_fill_holes_and_boundary_on_emulated_kernels(name, k):
    MHC.check_case("cpu", name, k)


def test_refusals_on_the_emulated_path():
    MHC.check_refusals("cpu")


def test_clean_mesh_fills_between_compaction_and_smoothing_on_emulated_kernels():
    MHC.check_clean_composite("cpu")


def test_clean_mesh_without_the_option_is_what_it_was_on_emulated_kernels():
    MHC.check_off_is_today("cpu")


@pytest.mark.parametrize("sparse", [False, True])
def test_mesh_scan_with_hole_filling_end_to_end_on_emulated_kernels(tmp_path, sparse):
    MHC.check_end_to_end("cpu", tmp_path, sparse)


def test_mesh_clean_command_line_round_trip_on_emulated_kernels(tmp_path):
    MHC.check_command_line_round_trip("cpu", tmp_path)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


NULL = ctypes.c_void_p(0)


def test_c_abi_refuses_bad_arguments():
    """every refusal of csrc/mesh_holes.h, and nothing written by a refused call"""
    nv, nf = 4, 2
    verts = torch.tensor([[0, 0, 0], [2, 0, 0], [0, 2, 0], [2, 2, 1]], dtype=torch.float32)
    rgb = torch.tensor([[0, 10, 255], [1, 20, 255], [2, 30, 255], [2, 41, 254]], dtype=torch.uint8)
    faces = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32)
    i32 = lambda n: torch.full((n,), -7, dtype=torch.int32)                  # noqa: E731
    u8 = lambda n: torch.full((n,), 99, dtype=torch.uint8)                   # noqa: E731
    i64 = lambda n: torch.full((n,), -7, dtype=torch.int64)                  # noqa: E731
    untouched = lambda *ts: all(bool((t == (99 if t.dtype == torch.uint8 else -7)).all()) for t in ts)      # noqa: E731

    def refused(call, good, bad):
        for kw, pattern in bad:
            with pytest.raises(_lib.RcmvsError, match=pattern):
                call(**dict(good, **kw))

    def nulls(*keys):
        return [({k: NULL}, "null pointer") for k in keys]

    from rc_mvsnet_amd import mesh_clean as MC
    adj = MC.adjacency(nv, faces)

    # boundary
    oc, ic, succ, pred, flags, counts = i32(nv), i32(nv), i32(nv), i32(nv), u8(nv), i64(2)
    good = dict(faces=_p(faces), nv=nv, nf=nf, rs=_p(adj["row_start"]), rl=_p(adj["row_len"]), nbr=_p(adj["nbr"]), mult=_p(adj["mult"]), entries=6 * nf,
                oc=_p(oc), ic=_p(ic), succ=_p(succ), pred=_p(pred), flags=_p(flags), counts=_p(counts))
    bnd = lambda **a: _lib.call("rcmvs_mh_boundary", a["faces"], a["nv"], a["nf"], a["rs"], a["rl"], a["nbr"], a["mult"], a["entries"], a["oc"], a["ic"],      # noqa: E731
                                a["succ"], a["pred"], a["flags"], a["counts"], NULL)
    refused(bnd, good, nulls("faces", "rs", "rl", "nbr", "mult", "oc", "ic", "succ", "pred", "flags", "counts") +
            [({"nv": -1}, "vertices"), ({"nf": -1}, "faces"), ({"entries": -1}, "entries"), ({"entries": 2 ** 31}, "entries")])
    assert untouched(oc, ic, succ, pred, flags, counts)
    bnd(**good)
    assert succ.tolist() == [1, 3, 0, 2] and pred.tolist() == [2, 0, 3, 1] and flags.tolist() == [MH.SIMPLE] * 4 and counts.tolist() == [4, 0]
    assert oc.tolist() == [1] * 4 and ic.tolist() == [1] * 4
    bnd(**dict(good, entries=5))                                   # the segments of vertices 2 and 3 do not lie inside nbr: no half-edge leaves them
    assert oc.tolist() == [1, 1, 0, 0] and ic.tolist() == [0, 1, 0, 1] and flags.tolist() == [MH.COMPLEX, MH.SIMPLE, MH.NONE, MH.COMPLEX]
    assert succ.tolist() == [-1, 3, -1, -1] and pred.tolist() == [-1, 0, -1, -1] and counts.tolist() == [2, 2]
    bnd(**good)

    # leaders
    ll, vc, fc, vr, fr, work, totals = i32(nv), u8(nv), i32(nv), i32(nv + 1), i32(nv + 1), i32(MH.SCAN_WORK + 2), i64(5)
    good = dict(succ=_p(succ), pred=_p(pred), nv=nv, me=4, ll=_p(ll), vc=_p(vc), fc=_p(fc), vr=_p(vr), fr=_p(fr), work=_p(work), totals=_p(totals))
    led = lambda **a: _lib.call("rcmvs_mh_leaders", a["succ"], a["pred"], a["nv"], a["me"], a["ll"], a["vc"], a["fc"], a["vr"], a["fr"], a["work"],      # noqa: E731
                                a["totals"], NULL)
    refused(led, good, nulls("succ", "pred", "ll", "vc", "fc", "vr", "fr", "work", "totals") +
            [({"me": m}, "max_edges") for m in (2, 0, -1, MH.MAX_EDGES + 1)] + [({"nv": -1}, "vertices"),
                                                                               ({"work": ctypes.c_void_p(work.data_ptr() + 4)}, "8-byte aligned")])
    assert untouched(ll, vc, fc, vr, fr, work, totals)
    led(**dict(good, me=3))
    assert ll.tolist() == [0] * 4 and vr.tolist() == [0] * 5 and fr.tolist() == [0] * 5 and totals.tolist() == [0] * 5
    led(**dict(good, me=MH.MAX_EDGES))
    assert ll.tolist() == [4, 0, 0, 0] and vc.tolist() == [1, 0, 0, 0] and fc.tolist() == [4, 0, 0, 0]
    assert vr.tolist() == [0, 1, 1, 1, 1] and fr.tolist() == [0, 4, 4, 4, 4] and totals.tolist() == [1, 4, 1, 0, 4]

    # emit
    ov, oc_, of = torch.full((nv + 1, 3), -7.0), u8(3 * (nv + 1)), i32(3 * (nf + 4))
    good = dict(verts=_p(verts), rgb=_p(rgb), faces=_p(faces), nv=nv, nf=nf, succ=_p(succ), ll=_p(ll), vr=_p(vr), fr=_p(fr), nvo=nv + 1, nfo=nf + 4,
                ov=_p(ov), oc=_p(oc_), of=_p(of))
    emi = lambda **a: _lib.call("rcmvs_mh_emit", a["verts"], a["rgb"], a["faces"], a["nv"], a["nf"], a["succ"], a["ll"], a["vr"], a["fr"], a["nvo"],      # noqa: E731
                                a["nfo"], a["ov"], a["oc"], a["of"], NULL)
    refused(emi, good, nulls("verts", "rgb", "faces", "succ", "ll", "vr", "fr", "ov", "of") +
            [({"nv": -1}, "vertices"), ({"nf": -1}, "faces"), ({"nvo": nv - 1}, "vertices"), ({"nfo": nf - 1}, "faces"), ({"ov": _p(verts)}, "overlaps"),
             ({"of": _p(faces)}, "overlaps"), ({"oc": _p(rgb)}, "overlaps")])
    assert bool((ov == -7.0).all()) and untouched(oc_, of)
    emi(**dict(good, rgb=NULL, oc=NULL))
    assert untouched(oc_) and ov[:nv].tolist() == verts.tolist() and ov[nv].tolist() == [1.0, 1.0, 0.25]
    assert of.reshape(-1, 3).tolist() == faces.tolist() + [[1, 0, 4], [3, 1, 4], [2, 3, 4], [0, 2, 4]]
    emi(**good)
    assert oc_.reshape(-1, 3).tolist() == rgb.tolist() + [[1, 25, 255]]          # 5 / 4 rounds to 1, 101 / 4 to 25, 1019 / 4 to 255
    of.fill_(-7), ov.fill_(-7.0)
    emi(**dict(good, nvo=nv, nfo=nf + 3))                         # ranks outside the output are not written
    assert of.reshape(-1, 3)[:nf].tolist() == faces.tolist() and untouched(of[3 * nf:]) and bool((ov[nv] == -7.0).all())


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("order", ["1", "2"])
def test_other_thread_orders_give_the_same_bytes(order, tmp_path):
    """RCMVS_EMU_ORDER=1|2 schedules every block's threads in another order between synchronisation points: the plain stores of
    succ and pred that meet at a complex vertex land in another order, and must not show.  The cases with complex vertices and
    two with several loops.  Run in a child process (the order is read when the library is loaded)."""
    script = tmp_path / "run.py"
    script.write_text(
        "import sys, os\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import torch, conftest\n"
        "import mesh_holes_cases as MHC\n"
        "from rc_mvsnet_amd import _lib, mesh_holes as MH\n"
        "lib = conftest.load_emu_lib()\n"
        "conftest.route_to_emulation(lib, setattr)\n"
        "_lib.bind(lib)\n"
        "for name in ('holes_share_vertex', 'nonmanifold_3', 'flipped_patch', 'sphere_caps_2.5', 'grid_holes'):\n"
        "    tv, tf, tc = MHC.to_dev('cpu', *MHC.case(name))\n"
        "    b = MH.boundary(int(tv.shape[0]), tf)\n"
        "    v, f, c, stats = MH.fill_holes(tv, tf, tc, max_edges=64)\n"
        "    sys.stdout.write(b['succ'].numpy().tobytes().hex() + b['pred'].numpy().tobytes().hex() + v.numpy().tobytes().hex() + f.numpy().tobytes().hex() +\n"
        "                     c.numpy().tobytes().hex() + repr(sorted(stats.items())))\n"
        % (REPO, os.path.join(REPO, "tests")))
    outs = []
    for o in ("0", order):
        env = dict(os.environ, RCMVS_EMU_ORDER=o)
        outs.append(subprocess.run([sys.executable, str(script)], env=env, check=True, capture_output=True, text=True).stdout)
    assert "('complex_vertices', 2)" in outs[0] and "('loops_filled', 4)" in outs[0] and len(outs[0]) > 10000 and outs[0] == outs[1]
