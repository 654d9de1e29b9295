"""The mesh simplification kernels (csrc/mesh_simplify.hip) on the CPU emulation of tests/emu, driven through
rc_mvsnet_amd/mesh_simplify.py on CPU tensors: the cases of tests/test_gpu_mesh_simplify.py (tests/mesh_simplify_cases.py), every flag,
key, counter, quadric, position, colour sum and face equal to tests/mesh_simplify_oracle.py in every bit after every round.  The
emulation runs blocks one after another, so a kernel that waited for another workgroup would never return here.  The C ABI's
refusals are checked here too, on the emulated library."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import mesh_simplify_cases as MSC
from rc_mvsnet_amd import _lib, dtu_eval, fusion, mesh_simplify as MS


@pytest.fixture(autouse=True)
def emu_ms(emu, monkeypatch):
    _lib.bind(emu)                                               # the emu fixture binds the primary header's table; the extensions' too
    monkeypatch.setattr(dtu_eval, "_chk", fusion._chk)
    monkeypatch.setattr(dtu_eval, "_stream", fusion._stream)
    return emu


@pytest.mark.parametrize("name,k", [key for key in MSC.case_keys() if key[0] not in ("plane_17", "cube_9", "plane_9", "cube_5")])
def test_every_round_and_the_result_on_emulated_kernels(name, k):
    MSC.check_case("cpu", name, k)


def test_plane_known_answer_on_emulated_kernels():
    """the 9 x 9 plane: the 17 x 17 one takes 127 rounds of one or two collapses, a minute here, and runs on the device"""
    MSC.check_plane("cpu", 9)


def test_cube_known_answer_on_emulated_kernels():
    """the cube of 5 x 5 sides: the one of 9 x 9 sides takes 256 rounds, minutes here, and runs on the device"""
    MSC.check_cube("cpu", 5)


def test_untouched_vertices_are_copies_on_emulated_kernels():
    MSC.check_untouched_vertices("cpu")


def test_refusals_on_the_emulated_path():
    MSC.check_refusals("cpu")


def test_real_extraction_on_emulated_kernels():
    MSC.check_extraction("cpu")


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


NULL = ctypes.c_void_p(0)


def test_c_abi_refuses_bad_arguments():
    """every refusal of csrc/mesh_simplify.h, and nothing written by a refused call"""
    nan, inf = float("nan"), float("inf")
    v, f, rgb = MSC.case("octahedron")
    nv, nf = len(v), len(f)
    verts, faces, colours = torch.from_numpy(v.copy()), torch.from_numpy(f.copy()), torch.from_numpy(rgb.copy())
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

    frame = (ctypes.c_double * 4)(0.0, 0.0, 0.25, 2.5)
    bad_frame = [({"frame": host((ctypes.c_double * 4)(0, nan, 0, 1))}, "centre"), ({"frame": host((ctypes.c_double * 4)(0, 0, inf, 1))}, "centre")] + \
        [({"frame": host((ctypes.c_double * 4)(0, 0, 0, s))}, "side") for s in (0.0, -1.0, nan, inf)]
    bad_sizes = [({"nv": -1}, "vertices"), ({"nf": -1}, "faces"), ({"nf": 2 ** 29}, "faces")]
    n, e = 3 * nf, 6 * nf
    ka, ia, kb, ib, hist, hstart, work, seg = i32(n), i32(n), i32(n), i32(n), i32(256), i32(257), i32(MS.C["RCMVS_MS_SCAN_WORK"] + 2), i32(2 * nv)
    quad, members, csum, live, stats = f64(10 * nv), i32(nv), i64(3 * nv), i64(1), i64(4)
    misaligned = ({"work": ctypes.c_void_p(work.data_ptr() + 4)}, "8-byte aligned")

    # init
    good = dict(verts=_p(verts), faces=_p(faces), rgb=_p(colours), nv=nv, nf=nf, frame=host(frame), ka=_p(ka), ia=_p(ia), kb=_p(kb), ib=_p(ib), hist=_p(hist),
                hstart=_p(hstart), work=_p(work), seg=_p(seg), quad=_p(quad), members=_p(members), csum=_p(csum), live=_p(live), stats=_p(stats))
    ini = lambda **a: _lib.call("rcmvs_ms_init", a["verts"], a["faces"], a["rgb"], a["nv"], a["nf"], a["frame"], a["ka"], a["ia"], a["kb"], a["ib"], a["hist"],      # noqa: E731
                                a["hstart"], a["work"], a["seg"], a["quad"], a["members"], a["csum"], a["live"], a["stats"], NULL)
    refused(ini, good, nulls("verts", "faces", "rgb", "frame", "ka", "ia", "kb", "ib", "hist", "hstart", "work", "seg", "quad", "members", "csum", "live", "stats") +
            bad_frame + bad_sizes + [misaligned])
    assert untouched(ka, ia, kb, ib, hist, hstart, work, seg, quad, members, csum, live, stats)
    ini(**good)
    assert live.tolist() == [8] and stats.tolist() == [0, 0, 8, 0] and members.tolist() == [1] * nv and csum.reshape(nv, 3).tolist() == rgb.tolist()
    want = MSC.O.begin(v, f, rgb)
    assert MSC.same_bits64(quad.reshape(nv, 10).numpy(), want["quad"])
    ini(**dict(good, rgb=NULL, csum=NULL))                       # no colours

    # round
    fout, rs, rl, nbr, mult, onb, cur, heavy, adj = i32(n), i32(nv + 1), i32(nv), i32(e), i32(e), u8(nv), i32(nv), i32(e // 49 + 1), i64(6)
    locked, edge, key, b1, b2, sel, rank, app, remap, counts = u8(nv), u8(e), i64(e), i64(nv), i64(nv), u8(e), i32(e + 1), u8(e), i32(nv), i64(16)
    for t in (ka, ia, kb, ib, hist, hstart, work, seg):
        t.fill_(-7)
    before = [t.clone() for t in (verts, quad, members, csum, live)]
    good = dict(verts=_p(verts), fin=_p(faces), fout=_p(fout), nv=nv, nf=nf, frame=host(frame), quad=_p(quad), members=_p(members), csum=_p(csum), target=0,
                err=inf, rs=_p(rs), rl=_p(rl), nbr=_p(nbr), mult=_p(mult), onb=_p(onb), cur=_p(cur), heavy=_p(heavy), cap=int(heavy.numel()), adj=_p(adj), ka=_p(ka),
                ia=_p(ia), kb=_p(kb), ib=_p(ib), hist=_p(hist), hstart=_p(hstart), work=_p(work), seg=_p(seg), locked=_p(locked), edge=_p(edge), key=_p(key),
                b1=_p(b1), b2=_p(b2), sel=_p(sel), rank=_p(rank), app=_p(app), remap=_p(remap), live=_p(live), counts=_p(counts))
    rnd = lambda **a: _lib.call("rcmvs_ms_round", a["verts"], a["fin"], a["fout"], a["nv"], a["nf"], a["frame"], a["quad"], a["members"], a["csum"], a["target"],      # noqa: E731
                                a["err"], a["rs"], a["rl"], a["nbr"], a["mult"], a["onb"], a["cur"], a["heavy"], a["cap"], a["adj"], a["ka"], a["ia"], a["kb"],
                                a["ib"], a["hist"], a["hstart"], a["work"], a["seg"], a["locked"], a["edge"], a["key"], a["b1"], a["b2"], a["sel"], a["rank"],
                                a["app"], a["remap"], a["live"], a["counts"], NULL)
    refused(rnd, good, nulls("verts", "fin", "fout", "frame", "quad", "members", "rs", "rl", "nbr", "mult", "onb", "cur", "heavy", "adj", "ka", "ia", "kb", "ib", "hist",
                             "hstart", "work", "seg", "locked", "edge", "key", "b1", "b2", "sel", "rank", "app", "remap", "live", "counts") +
            bad_frame + bad_sizes + [misaligned, ({"target": -1}, "target_faces"), ({"err": -1e-9}, "max_error"), ({"err": nan}, "max_error"),
                                     ({"cap": 0}, "heavy_capacity"), ({"fout": _p(faces)}, "overlaps")])
    assert untouched(fout, rs, rl, nbr, mult, onb, cur, heavy, adj, ka, ia, kb, ib, hist, hstart, work, seg, locked, edge, key, b1, b2, sel, rank, app, remap, counts)
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip((verts, quad, members, csum, live), before))
    rnd(**good)
    assert counts[MS.COUNT["applied"]] == 1 and live.tolist() == [6] and counts[MS.COUNT["live_before"]] == 8 and int(sel.sum()) == 1 and int((members == 0).sum()) == 1

    # finish
    fk, vk, fr, vr, orgb, tot = u8(nf), u8(nv), i32(nf + 1), i32(nv + 1), u8(3 * nv), i64(2)
    work.fill_(-7)
    good = dict(faces=_p(fout), nv=nv, nf=nf, members=_p(members), csum=_p(csum), drop=1, fk=_p(fk), vk=_p(vk), fr=_p(fr), vr=_p(vr), work=_p(work), orgb=_p(orgb),
                tot=_p(tot))
    fin = lambda **a: _lib.call("rcmvs_ms_finish", a["faces"], a["nv"], a["nf"], a["members"], a["csum"], a["drop"], a["fk"], a["vk"], a["fr"], a["vr"], a["work"],      # noqa: E731
                                a["orgb"], a["tot"], NULL)
    refused(fin, good, nulls("faces", "members", "csum", "fk", "vk", "fr", "vr", "work", "orgb", "tot") + bad_sizes + [misaligned])
    assert untouched(fk, vk, fr, vr, work, orgb, tot)
    fin(**good)
    assert tot.tolist() == [6, 5] and int(fk.sum()) == 6 and int(vk.sum()) == 5


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("order", ["1", "2"])
def test_other_thread_orders_give_the_same_bytes(order, tmp_path):
    """RCMVS_EMU_ORDER=1|2 schedules every block's threads in another order between synchronisation points: a missing barrier in a
    block reduction, or a key that two lanes wrote, would change the mesh.  Run in a child process (the order is read when the
    library is loaded)."""
    script = tmp_path / "run.py"
    script.write_text(
        "import sys, os\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import torch, conftest\n"
        "import mesh_simplify_cases as MSC\n"
        "from rc_mvsnet_amd import _lib, mesh_simplify as MS\n"
        "lib = conftest.load_emu_lib()\n"
        "conftest.route_to_emulation(lib, setattr)\n"
        "_lib.bind(lib)\n"
        "for name in ('sphere', 'fan_50', 'duplicates_and_fin', 'sheet_257'):\n"
        "    v, f, c, stats = MS.simplify(*MSC.to_dev('cpu', *MSC.case(name)), **MSC.CASES[name][1][0])\n"
        "    sys.stdout.write(v.numpy().tobytes().hex() + f.numpy().tobytes().hex() + c.numpy().tobytes().hex() + repr(sorted(stats.items())))\n"
        % (REPO, os.path.join(REPO, "tests")))
    outs = []
    for o in ("0", order):
        env = dict(os.environ, RCMVS_EMU_ORDER=o)
        outs.append(subprocess.run([sys.executable, str(script)], env=env, check=True, capture_output=True, text=True).stdout)
    assert "('faces_out', 264)" in outs[0] and len(outs[0]) > 10000 and outs[0] == outs[1]


@pytest.mark.parametrize("sparse", [False, True])
def test_mesh_scan_with_simplification_end_to_end_on_emulated_kernels(tmp_path, sparse):
    MSC.check_end_to_end("cpu", tmp_path, sparse)
