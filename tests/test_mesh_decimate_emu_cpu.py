"""The mesh decimation kernels (csrc/mesh_decimate.hip) on the CPU emulation of tests/emu, driven through
rc_mvsnet_amd/mesh_decimate.py on CPU tensors: the cases of tests/test_gpu_mesh_decimate.py (tests/mesh_decimate_cases.py), every
cluster number, key, flag, counter, quadric, position, colour and face equal to tests/mesh_decimate_oracle.py in every bit.  The
emulation runs blocks one after another, so a kernel that waited for another workgroup would never return here.  The C ABI's
refusals are checked here too, on the emulated library."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import mesh_decimate_cases as MDC
from rc_mvsnet_amd import _lib, dtu_eval, fusion, mesh_decimate as MD


@pytest.fixture(autouse=True)
def emu_md(emu, monkeypatch):
    _lib.bind(emu)                                               # the emu fixture binds the primary header's table; the extensions' too
    monkeypatch.setattr(dtu_eval, "_chk", fusion._chk)
    monkeypatch.setattr(dtu_eval, "_stream", fusion._stream)
    return emu


@pytest.mark.parametrize("name,k", MDC.case_keys())
def test_decimate_and_its_parts_on_emulated_kernels(name, k):
    MDC.check_case("cpu", name, k)


def test_refusals_on_the_emulated_path():
    MDC.check_refusals("cpu")


def test_identity_when_every_vertex_is_alone_on_emulated_kernels():
    MDC.check_identity_when_every_vertex_is_alone("cpu")


def test_real_extraction_on_emulated_kernels():
    MDC.check_extraction("cpu")


@pytest.mark.parametrize("sparse", [False, True])
def test_mesh_scan_with_decimation_end_to_end_on_emulated_kernels(tmp_path, sparse):
    MDC.check_end_to_end("cpu", tmp_path, sparse)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


NULL = ctypes.c_void_p(0)


def test_c_abi_refuses_bad_arguments():
    """every refusal of csrc/mesh_decimate.h, and nothing written by a refused call"""
    nan, inf = float("nan"), float("inf")
    nv, nf, m = 4, 2, 3
    verts = torch.tensor([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0.25, 0, 0]], dtype=torch.float32)
    rgb = torch.arange(12, dtype=torch.uint8).reshape(4, 3)
    faces = torch.tensor([[0, 1, 2], [3, 1, 2]], dtype=torch.int32)
    i32 = lambda n: torch.full((n,), -7, dtype=torch.int32)                  # noqa: E731
    u8 = lambda n: torch.full((n,), 99, dtype=torch.uint8)                   # noqa: E731
    i64 = lambda n: torch.full((n,), -7, dtype=torch.int64)                  # noqa: E731
    f64 = lambda n: torch.full((n,), -7.0, dtype=torch.float64)              # noqa: E731
    untouched = lambda *ts: all(bool((t == (99 if t.dtype == torch.uint8 else -7)).all()) for t in ts)      # noqa: E731
    host = lambda arr: ctypes.cast(arr, ctypes.c_void_p)                      # noqa: E731

    def refused(call, good, bad):
        for kw, pattern in bad:
            with pytest.raises(_lib.RcmvsError, match=pattern):
                call(**dict(good, **kw))

    def nulls(*keys):
        return [({k: NULL}, "null pointer") for k in keys]

    # bounds
    bnd = i32(8)
    good = dict(verts=_p(verts), nv=nv, bounds=_p(bnd))
    refused(lambda **a: _lib.call("rcmvs_md_bounds", a["verts"], a["nv"], a["bounds"], NULL), good, nulls("verts", "bounds") + [({"nv": -1}, "vertices")])
    assert untouched(bnd)
    lo, hi, finite = MD.bounds(verts)
    assert lo.tolist() == [0, 0, 0] and hi.tolist() == [2, 2, 0] and finite == 4

    # lattice (host only)
    box, lat, g = (ctypes.c_float * 6)(0, 0, 0, 2, 2, 0), (ctypes.c_double * 4)(-7, -7, -7, -7), (ctypes.c_longlong * 3)(-7, -7, -7)
    good = dict(box=host(box), cell=1.0, lat=host(lat), g=host(g))
    far = (ctypes.c_float * 6)(0, 0, 0, 1, 1, 2 ** 21)
    refused(lambda **a: _lib.call("rcmvs_md_lattice", a["box"], a["cell"], a["lat"], a["g"]), good,
            nulls("box", "lat", "g") + [({"cell": c}, "cell") for c in (0.0, -1.0, nan, inf)] +
            [({"box": host((ctypes.c_float * 6)(0, 0, 0, 2, nan, 0))}, "axis y"), ({"box": host((ctypes.c_float * 6)(3, 0, 0, 2, 2, 0))}, "axis x"),
             ({"box": host((ctypes.c_float * 6)(0, 0, -inf, 2, 2, 0))}, "axis z"), ({"box": host(far)}, "2097153 cells on axis z"),
             ({"cell": 1e-30}, "cells on axis x")])
    assert list(lat) == [-7] * 4 and list(g) == [-7] * 3
    _lib.call("rcmvs_md_lattice", host(box), 1.0, host(lat), host(g))
    assert list(lat) == [-0.5, -0.5, -0.5, 1.0] and list(g) == [3, 3, 1]

    # cluster
    ka, kb, ia, ib, hist, hstart, work = i64(nv), i64(nv), i32(nv), i32(nv), i32(256), i32(257), i32(MD.SCAN_WORK + 2)
    head, hrank, cl, order, start, ckey, totals = u8(nv), i32(nv + 1), i32(nv), i32(nv), i32(nv + 1), i64(nv), i64(2)
    good = dict(verts=_p(verts), nv=nv, lat=host(lat), g=host(g), ka=_p(ka), ia=_p(ia), kb=_p(kb), ib=_p(ib), hist=_p(hist), hstart=_p(hstart), work=_p(work),
                head=_p(head), hrank=_p(hrank), cl=_p(cl), order=_p(order), start=_p(start), ckey=_p(ckey), totals=_p(totals))
    clu = lambda **a: _lib.call("rcmvs_md_cluster", a["verts"], a["nv"], a["lat"], a["g"], a["ka"], a["ia"], a["kb"], a["ib"], a["hist"], a["hstart"],      # noqa: E731
                                a["work"], a["head"], a["hrank"], a["cl"], a["order"], a["start"], a["ckey"], a["totals"], NULL)
    bad_lattice = [({"lat": host((ctypes.c_double * 4)(0, 0, 0, c))}, "cell") for c in (0.0, -2.0, nan, inf)] + \
        [({"lat": host((ctypes.c_double * 4)(0, nan, 0, 1))}, "origin"), ({"g": host((ctypes.c_longlong * 3)(3, 0, 1))}, "0 cells on axis y"),
         ({"g": host((ctypes.c_longlong * 3)(2 ** 21 + 1, 3, 1))}, "2097153 cells on axis x"), ({"g": host((ctypes.c_longlong * 3)(3, 3, -1))}, "axis z")]
    refused(clu, good, nulls("verts", "lat", "g", "ka", "ia", "kb", "ib", "hist", "hstart", "work", "head", "hrank", "cl", "order", "start", "ckey", "totals") +
            bad_lattice + [({"nv": -1}, "vertices"), ({"work": ctypes.c_void_p(work.data_ptr() + 4)}, "8-byte aligned")])
    assert untouched(ka, kb, ia, ib, hist, hstart, work, head, hrank, cl, order, start, ckey, totals)
    clu(**good)
    assert cl.tolist() == [0, 1, 2, 0] and order.tolist() == [0, 3, 1, 2] and start.tolist() == [0, 2, 3, 4, -7] and ckey.tolist() == [0, 2, 6, -7]
    assert totals.tolist() == [3, 4]

    # faces
    cface, fclass, table, counts = i32(3 * nf), u8(nf), i32(4), i64(4)
    good = dict(faces=_p(faces), nv=nv, nf=nf, cl=_p(cl), cface=_p(cface), fclass=_p(fclass), table=_p(table), cap=4, counts=_p(counts))
    cla = lambda **a: _lib.call("rcmvs_md_classify_faces", a["faces"], a["nv"], a["nf"], a["cl"], a["cface"], a["fclass"], a["table"], a["cap"],      # noqa: E731
                                a["counts"], NULL)
    refused(cla, good, nulls("faces", "cl", "cface", "fclass", "table", "counts") +
            [({"cap": c}, "table_capacity") for c in (2, 3, 6, 0, -4, 2 ** 33)] + [({"nv": -1}, "vertices"), ({"nf": -1}, "faces"), ({"nf": 2 ** 30}, "faces")])
    assert untouched(cface, fclass, table, counts)
    cla(**good)
    assert cface.tolist() == [0, 1, 2, 0, 1, 2] and fclass.tolist() == [MD.FACE_KEPT, MD.FACE_DUPLICATE] and counts.tolist() == [0, 0, 0, 1]

    # quadrics
    n = 3 * nf
    cka, ckb, cia, cib, seg, quad = i32(n), i32(n), i32(n), i32(n), i32(2 * m), f64(9 * m)
    hist.fill_(-7), hstart.fill_(-7), work.fill_(-7)
    good = dict(verts=_p(verts), faces=_p(faces), nv=nv, nf=nf, cl=_p(cl), ckey=_p(ckey), m=m, lat=host(lat), g=host(g), cka=_p(cka), cia=_p(cia), ckb=_p(ckb),
                cib=_p(cib), hist=_p(hist), hstart=_p(hstart), work=_p(work), seg=_p(seg), quad=_p(quad))
    qua = lambda **a: _lib.call("rcmvs_md_quadrics", a["verts"], a["faces"], a["nv"], a["nf"], a["cl"], a["ckey"], a["m"], a["lat"], a["g"], a["cka"],      # noqa: E731
                                a["cia"], a["ckb"], a["cib"], a["hist"], a["hstart"], a["work"], a["seg"], a["quad"], NULL)
    refused(qua, good, nulls("verts", "faces", "cl", "ckey", "lat", "g", "cka", "cia", "ckb", "cib", "hist", "hstart", "work", "seg", "quad") + bad_lattice +
            [({"m": 0}, "clusters"), ({"m": nv + 1}, "clusters"), ({"nv": -1}, "vertices"), ({"nf": -1}, "faces"),
             ({"work": ctypes.c_void_p(work.data_ptr() + 4)}, "8-byte aligned")])
    assert untouched(cka, ckb, cia, cib, hist, hstart, work, seg, quad)
    qua(**good)
    # cluster 0 (centre 0 0 0) holds the first corners of both faces: normals (0, 0, 4) and (0, 0, 3.5) through z = 0
    assert quad.reshape(m, 9)[0].tolist() == [0, 0, 0, 0, 0, 16 + 12.25, 0, 0, 0] and quad.reshape(m, 9)[1].tolist() == [0, 0, 0, 0, 0, 28.25, 0, 0, 0]

    # place
    ov, oc, via, pc = torch.full((m, 3), -7.0), u8(3 * m), u8(m), i64(3)
    good = dict(verts=_p(verts), rgb=_p(rgb), nv=nv, order=_p(order), start=_p(start), ckey=_p(ckey), m=m, lat=host(lat), g=host(g), quad=_p(quad), how=0,
                reg=1e-3, ov=_p(ov), oc=_p(oc), via=_p(via), pc=_p(pc))
    pla = lambda **a: _lib.call("rcmvs_md_place", a["verts"], a["rgb"], a["nv"], a["order"], a["start"], a["ckey"], a["m"], a["lat"], a["g"], a["quad"],      # noqa: E731
                                a["how"], a["reg"], a["ov"], a["oc"], a["via"], a["pc"], NULL)
    refused(pla, good, nulls("verts", "rgb", "order", "start", "ckey", "lat", "g", "quad", "ov", "via", "pc") + bad_lattice +
            [({"how": 2}, "placement"), ({"how": -1}, "placement"), ({"reg": -1e-9}, "reg"), ({"reg": nan}, "reg"), ({"reg": inf}, "reg"), ({"m": -1}, "clusters"),
             ({"m": nv + 1}, "clusters"), ({"nv": -1}, "vertices")])
    assert bool((ov == -7.0).all()) and untouched(oc, via, pc)
    pla(**dict(good, rgb=NULL, oc=NULL))
    assert untouched(oc) and via.tolist() == [MD.VIA_QUADRIC] * 3 and pc.tolist() == [0, 0, 0]
    assert ov[1:].tolist() == [[2, 0, 0], [0, 2, 0]] and ov[0].tolist() == [0.125, 0, 0]          # a plane alone: the minimiser is the members' mean
    pla(**dict(good, how=1, quad=NULL))
    assert via.tolist() == [MD.VIA_MEAN] * 3 and ov[0].tolist() == [0.125, 0, 0] and oc.tolist() == [5, 6, 7, 3, 4, 5, 6, 7, 8]

    # select
    fk, vk, fr, vr, tot = u8(nf), u8(m), i32(nf + 1), i32(m + 1), i64(2)
    work.fill_(-7)
    good = dict(cface=_p(cface), fclass=_p(fclass), m=m, nf=nf, drop=1, fk=_p(fk), vk=_p(vk), fr=_p(fr), vr=_p(vr), work=_p(work), tot=_p(tot))
    sel = lambda **a: _lib.call("rcmvs_md_select", a["cface"], a["fclass"], a["m"], a["nf"], a["drop"], a["fk"], a["vk"], a["fr"], a["vr"], a["work"],      # noqa: E731
                                a["tot"], NULL)
    refused(sel, good, nulls("cface", "fclass", "fk", "vk", "fr", "vr", "work", "tot") +
            [({"m": -1}, "vertices"), ({"nf": -1}, "faces"), ({"work": ctypes.c_void_p(work.data_ptr() + 4)}, "8-byte aligned")])
    assert untouched(fk, vk, fr, vr, work, tot)
    sel(**good)
    assert fk.tolist() == [1, 0] and vk.tolist() == [1, 1, 1] and fr.tolist() == [0, 1, 1] and vr.tolist() == [0, 1, 2, 3] and tot.tolist() == [1, 3]


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("order", ["1", "2"])
def test_other_thread_orders_give_the_same_bytes(order, tmp_path):
    """RCMVS_EMU_ORDER=1|2 schedules every block's threads in another order between synchronisation points: a missing barrier in the
    sort, or a duplicate table whose outcome depended on the order of its insertions, would change the mesh.  The cases with
    duplicate faces, the long segment and a two-pass shuffled strip, both placements.  Run in a child process (the order is read
    when the library is loaded)."""
    script = tmp_path / "run.py"
    script.write_text(
        "import sys, os\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import torch, conftest\n"
        "import mesh_decimate_cases as MDC\n"
        "from rc_mvsnet_amd import _lib, mesh_decimate as MD\n"
        "lib = conftest.load_emu_lib()\n"
        "conftest.route_to_emulation(lib, setattr)\n"
        "_lib.bind(lib)\n"
        "for name in ('two_sheets', 'duplicates', 'patch_600_in_one_cell', 'strip_2049_shuffled'):\n"
        "    for placement in ('quadric', 'mean'):\n"
        "        v, f, c, stats = MD.decimate(*MDC.to_dev('cpu', *MDC.case(name)), placement=placement, **MDC.CASES[name][1][0])\n"
        "        sys.stdout.write(v.numpy().tobytes().hex() + f.numpy().tobytes().hex() + c.numpy().tobytes().hex() + repr(sorted(stats.items())))\n"
        % (REPO, os.path.join(REPO, "tests")))
    outs = []
    for o in ("0", order):
        env = dict(os.environ, RCMVS_EMU_ORDER=o)
        outs.append(subprocess.run([sys.executable, str(script)], env=env, check=True, capture_output=True, text=True).stdout)
    assert "('duplicate_faces', 32)" in outs[0] and len(outs[0]) > 10000 and outs[0] == outs[1]
