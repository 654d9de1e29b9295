"""The mesh clean-up kernels (csrc/mesh_clean.hip) on the CPU emulation of tests/emu, driven through rc_mvsnet_amd/mesh_clean.py on
CPU tensors: the cases of tests/test_gpu_mesh_clean.py (tests/mesh_clean_cases.py), every label, flag, rank, neighbour, position,
colour and face equal to tests/mesh_clean_oracle.py in every bit.  The emulation runs blocks one after another, so a kernel that
waited for another workgroup would never return here.  The C ABI's refusals are checked here too, on the emulated library."""
import ctypes

import pytest
import torch

import mesh_clean_cases as MCC
from rc_mvsnet_amd import _lib, dtu_eval, fusion, mesh_clean as MC


@pytest.fixture(autouse=True)
def emu_mc(emu, monkeypatch):
    _lib.bind(emu)                                               # the emu fixture binds the primary header's table; the extensions' too
    monkeypatch.setattr(dtu_eval, "_chk", fusion._chk)
    monkeypatch.setattr(dtu_eval, "_stream", fusion._stream)
    return emu


@pytest.mark.parametrize("name", list(MCC.CASES))
def test_components_and_adjacency_on_emulated_kernels(name):
    MCC.check_parts("cpu", name)


@pytest.mark.parametrize("name,k", MCC.case_keys())
def test_clean_mesh_on_emulated_kernels(name, k):
    MCC.check_clean("cpu", name, k)


def test_taubin_identities_and_pinning_on_emulated_kernel():
    MCC.check_smoothing_parts("cpu")


def test_real_extraction_on_emulated_kernels():
    MCC.check_extraction("cpu")


def test_mesh_scan_with_clean_options_end_to_end_on_emulated_kernels(tmp_path):
    MCC.check_end_to_end("cpu", tmp_path)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


NULL = ctypes.c_void_p(0)


def test_c_abi_refuses_bad_arguments():
    """every refusal of csrc/mesh_clean.h, and nothing written by a refused call"""
    nan, inf = float("nan"), float("inf")
    nv, nf = 4, 2
    faces = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32)
    i32 = lambda n: torch.full((n,), -7, dtype=torch.int32)                  # noqa: E731
    u8 = lambda n: torch.full((n,), 99, dtype=torch.uint8)                   # noqa: E731
    i64 = lambda n: torch.full((n,), -7, dtype=torch.int64)                  # noqa: E731
    untouched = lambda *ts: all(bool((t == (99 if t.dtype == torch.uint8 else -7)).all()) for t in ts)      # noqa: E731

    def refused(call, good, bad):
        for kw, pattern in bad:
            with pytest.raises(_lib.RcmvsError, match=pattern):
                call(**dict(good, **kw))

    # components
    label, ok, cf, counts = i32(nv), u8(nf), i32(nv), i64(4)
    good = dict(faces=_p(faces), nv=nv, nf=nf, label=_p(label), ok=_p(ok), cf=_p(cf), counts=_p(counts))
    comp = lambda **a: _lib.call("rcmvs_mc_components", a["faces"], a["nv"], a["nf"], a["label"], a["ok"], a["cf"], a["counts"], NULL)      # noqa: E731
    refused(comp, good, [({k: NULL}, "null pointer") for k in ("faces", "label", "ok", "cf", "counts")] + [({"nv": -1}, "vertices"), ({"nf": -2}, "faces")])
    assert untouched(label, ok, cf, counts)
    comp(**good)
    assert label.tolist() == [0, 0, 0, 0] and ok.tolist() == [1, 1] and cf.tolist() == [2, 0, 0, 0] and counts.tolist() == [0, 0, 0, 0]

    # component table
    flags, rank, work, table, totals = u8(nv), i32(nv + 1), i32(MC.SCAN_WORK + 2), i32(2), i64(2)
    good = dict(label=_p(label), cf=_p(cf), nv=nv, flags=_p(flags), rank=_p(rank), work=_p(work), table=_p(table), cap=1, totals=_p(totals))
    tab = lambda **a: _lib.call("rcmvs_mc_component_table", a["label"], a["cf"], a["nv"], a["flags"], a["rank"], a["work"], a["table"], a["cap"],      # noqa: E731
                                a["totals"], NULL)
    refused(tab, good, [({k: NULL}, "null pointer") for k in ("label", "cf", "flags", "rank", "work", "totals")] +
            [({"table": NULL}, "capacity"), ({"cap": -1}, "capacity"), ({"nv": -1}, "vertices"), ({"work": ctypes.c_void_p(work.data_ptr() + 4)}, "8-byte aligned")])
    assert untouched(flags, rank, work, table, totals)
    tab(**good)
    assert table.tolist() == [0, 2] and totals.tolist() == [1, 2] and rank.tolist() == [0, 1, 1, 1, 1]
    tab(**dict(good, table=NULL, cap=0))

    # select
    fk, vk, fr, vr, tot3 = u8(nf), u8(nv), i32(nf + 1), i32(nv + 1), i64(3)
    work.fill_(-7)
    good = dict(faces=_p(faces), ok=_p(ok), label=_p(label), cf=_p(cf), nv=nv, nf=nf, minf=0, frac=0.0, most=2, kl=0, kf=0, klab=0, drop=1, fk=_p(fk), vk=_p(vk),
                fr=_p(fr), vr=_p(vr), work=_p(work), totals=_p(tot3))
    sel = lambda **a: _lib.call("rcmvs_mc_select", a["faces"], a["ok"], a["label"], a["cf"], a["nv"], a["nf"], a["minf"], a["frac"], a["most"], a["kl"],      # noqa: E731
                                a["kf"], a["klab"], a["drop"], a["fk"], a["vk"], a["fr"], a["vr"], a["work"], a["totals"], NULL)
    refused(sel, good, [({k: NULL}, "null pointer") for k in ("faces", "ok", "label", "cf", "fk", "vk", "fr", "vr", "work", "totals")] +
            [({"minf": -1}, "min_faces"), ({"kl": -1}, "keep_largest"), ({"frac": nan}, "min_fraction"), ({"frac": inf}, "min_fraction"), ({"nf": -1}, "faces")])
    assert untouched(fk, vk, fr, vr, work, tot3)
    sel(**good)
    assert fk.tolist() == [1, 1] and vk.tolist() == [1, 1, 1, 1] and fr.tolist() == [0, 1, 2] and vr.tolist() == [0, 1, 2, 3, 4] and tot3.tolist() == [2, 4, 1]

    # gather
    verts, rgb = torch.arange(12, dtype=torch.float32).reshape(4, 3), torch.arange(12, dtype=torch.uint8).reshape(4, 3)
    ov, oc, of = torch.full((4, 3), -7.0), u8(12), i32(6)
    good = dict(verts=_p(verts), rgb=_p(rgb), faces=_p(faces), fk=_p(fk), fr=_p(fr), vk=_p(vk), vr=_p(vr), nv=nv, nf=nf, nvo=4, nfo=2, ov=_p(ov), oc=_p(oc), of=_p(of))
    gat = lambda **a: _lib.call("rcmvs_mc_gather", a["verts"], a["rgb"], a["faces"], a["fk"], a["fr"], a["vk"], a["vr"], a["nv"], a["nf"], a["nvo"], a["nfo"],      # noqa: E731
                                a["ov"], a["oc"], a["of"], NULL)
    refused(gat, good, [({k: NULL}, "null pointer") for k in ("verts", "rgb", "faces", "fk", "fr", "vk", "vr", "ov", "of")] +
            [({"nvo": 5}, "vertices"), ({"nfo": 3}, "faces out"), ({"nvo": -1}, "vertices"), ({"nv": -1}, "vertices")])
    assert untouched(ov, oc, of)
    gat(**dict(good, rgb=NULL, oc=NULL))
    assert torch.equal(ov, verts) and of.tolist() == faces.reshape(-1).tolist() and untouched(oc)
    gat(**good)
    assert oc.tolist() == list(range(12))

    # adjacency
    rs, rl, nbr, mult, ob, cur, heavy, stats = i32(nv + 1), i32(nv), i32(6 * nf), i32(6 * nf), u8(nv), i32(nv), i32(1), i64(6)
    work.fill_(-7)
    good = dict(faces=_p(faces), nv=nv, nf=nf, rs=_p(rs), rl=_p(rl), nbr=_p(nbr), mult=_p(mult), ob=_p(ob), cur=_p(cur), heavy=_p(heavy), hcap=1, work=_p(work),
                stats=_p(stats))
    adj = lambda **a: _lib.call("rcmvs_mc_adjacency", a["faces"], a["nv"], a["nf"], a["rs"], a["rl"], a["nbr"], a["mult"], a["ob"], a["cur"], a["heavy"],      # noqa: E731
                                a["hcap"], a["work"], a["stats"], NULL)
    refused(adj, good, [({k: NULL}, "null pointer") for k in ("faces", "rs", "rl", "nbr", "mult", "ob", "cur", "heavy", "work", "stats")] +
            [({"hcap": 0}, "heavy_capacity"), ({"nf": (1 << 31) // 6 + 1}, "entries"), ({"nv": -1}, "vertices")])
    assert untouched(rs, rl, nbr, mult, ob, cur, heavy, work, stats)
    adj(**good)
    assert rs.tolist() == [0, 2, 6, 10, 12] and rl.tolist() == [2, 3, 3, 2] and nbr.tolist() == [1, 2, 0, 2, 3, -1, 0, 1, 3, -1, 1, 2]
    assert mult.tolist() == [1, 1, 1, 2, 1, 0, 1, 2, 1, 0, 1, 1] and ob.tolist() == [1, 1, 1, 1] and stats.tolist() == [5, 4, 0, 4, 0, 12]

    # a Taubin step
    dst = torch.full((4, 3), -7.0)
    good = dict(src=_p(verts), dst=_p(dst), nv=nv, rs=_p(rs), rl=_p(rl), nbr=_p(nbr), n=12, pin=NULL, f=0.5)
    step = lambda **a: _lib.call("rcmvs_mc_taubin_step", a["src"], a["dst"], a["nv"], a["rs"], a["rl"], a["nbr"], a["n"], a["pin"], a["f"], NULL)      # noqa: E731
    refused(step, good, [({k: NULL}, "null pointer") for k in ("src", "dst", "rs", "rl", "nbr")] +
            [({"f": nan}, "factor"), ({"f": -inf}, "factor"), ({"n": -1}, "entries"), ({"nv": -1}, "vertices"), ({"dst": _p(verts)}, "overlap"),
             ({"dst": ctypes.c_void_p(verts.data_ptr() + 12)}, "overlap")])
    assert bool((dst == -7.0).all())
    step(**dict(good, pin=_p(ob)))
    assert torch.equal(dst, verts)                                               # every vertex is on the boundary: pinned
    step(**good)
    assert dst[0].tolist() == [(0 + 0.5 * ((3 + 6) / 2 - 0)), (1 + 0.5 * ((4 + 7) / 2 - 1)), (2 + 0.5 * ((5 + 8) / 2 - 2))]
    # a neighbour list that does not belong to this mesh moves nothing and reads nothing outside src
    bad = nbr.clone()
    bad[8], bad[10] = 4, 2 ** 31 - 1
    step(**dict(good, nbr=_p(bad)))
    assert torch.equal(dst[2:], verts[2:]) and not torch.equal(dst[:2], verts[:2])
    step(**dict(good, n=11))
    assert torch.equal(dst[3], verts[3]) and not torch.equal(dst[:3], verts[:3])


def test_module_refuses_bad_arguments_on_the_emulated_path():
    v, f = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    for kw, pattern in (({"min_faces": -1}, "min_faces"), ({"keep_largest": -2}, "keep_largest"), ({"smooth_iterations": -1}, "smooth_iterations"),
                        ({"min_fraction": float("nan")}, "min_fraction"), ({"lam": float("inf")}, "lam"), ({"mu": float("nan")}, "mu")):
        with pytest.raises(_lib.RcmvsError, match=pattern):
            MC.clean_mesh(v, f, **kw)
