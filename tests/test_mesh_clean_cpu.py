"""tests/mesh_clean_oracle.py itself, on answers that can be checked by hand, and the parts of rc_mvsnet_amd/mesh_clean.py that need
no kernel: the argument refusals and the default-off plumbing.  The kernels inherit every property below through bit equality with
this oracle (tests/test_mesh_clean_emu_cpu.py, tests/test_gpu_mesh_clean.py)."""
import inspect

import numpy as np
import pytest
import torch

import mesh_clean_cases as MCC
import mesh_clean_oracle as O
from rc_mvsnet_amd import _lib, mesh_clean as MC, tsdf_mesh as TM

TET = [(0, 1, 2), (0, 3, 1), (1, 3, 2), (2, 3, 0)]


def test_known_answers():
    v = np.eye(4, 3, dtype=np.float32)
    s = O.clean_mesh(v, TET)[3]
    assert (s["components_in"], s["euler_characteristic"], s["boundary_edges"], s["edges"], s["nonmanifold_edges"]) == (1, 2, 0, 6, 0)
    s = O.clean_mesh(v[:3], [(0, 1, 2)])[3]
    assert (s["components_in"], s["boundary_edges"], s["edges"], s["euler_characteristic"]) == (1, 3, 3, 1)
    s = O.clean_mesh(np.zeros((5, 3), np.float32), [(0, 1, 2), (0, 1, 3), (1, 0, 4)])[3]
    assert (s["nonmanifold_edges"], s["boundary_edges"], s["edges"]) == (1, 6, 7)
    a = O.adjacency(5, [(0, 1, 2), (0, 1, 3), (1, 0, 4)])
    assert a["nbr"][:4].tolist() == [1, 2, 3, 4] and a["mult"][:4].tolist() == [3, 1, 1, 1] and a["row_len"].tolist() == [4, 4, 2, 2, 2]
    assert a["row_start"].tolist() == [0, 6, 12, 14, 16, 18] and a["nbr"][4:6].tolist() == [-1, -1] and a["on_boundary"].tolist() == [1] * 5


def test_every_case_says_what_it_is_there_for():
    for name, want in MCC.KNOWN.items():
        got = MCC.reference(name, 0)[3]
        assert {k: got[k] for k in want} == want, name


def test_vertex_connectivity_and_labels():
    label, ok, faces_c, invalid = O.components(7, [(4, 5, 6), (6, 2, 3), (1, 1, 0), (0, 1, 9)])
    assert label.tolist() == [0, 1, 2, 2, 2, 2, 2] and ok.tolist() == [1, 1, 0, 0] and invalid == 2
    assert faces_c.tolist() == [0, 0, 2, 0, 0, 0, 0]                        # both faces' first indices carry the label 2


def test_selection_rules():
    table = np.array([[0, 5], [3, 9], [7, 5], [9, 1], [12, 9]], np.int32)
    assert O.kept_labels(table) == {0, 3, 7, 9, 12}
    assert O.kept_labels(table, min_faces=5) == {0, 3, 7, 12}
    assert O.kept_labels(table, min_fraction=0.56) == {3, 12} and O.kept_labels(table, min_fraction=5 / 9) == {0, 3, 7, 12}
    assert O.kept_labels(table, keep_largest=1) == {3} and O.kept_labels(table, keep_largest=3) == {3, 12, 0}     # ties: the smaller label
    assert O.kept_labels(table, keep_largest=9) == {0, 3, 7, 9, 12} and O.kept_labels(table, keep_largest=4, min_faces=6) == {3, 12}


def test_compaction_is_stable_and_rewrites_indices():
    v = np.arange(24, dtype=np.float32).reshape(8, 3)
    rgb = np.arange(24, dtype=np.uint8).reshape(8, 3)
    f = [(6, 5, 7), (1, 1, 2), (2, 1, 7)]
    ov, of, oc, info = O.compact(v, f, rgb)
    assert of.tolist() == [[3, 2, 4], [1, 0, 4]] and np.array_equal(ov, v[[1, 2, 5, 6, 7]]) and np.array_equal(oc, rgb[[1, 2, 5, 6, 7]])
    ov, of, oc, info = O.compact(v, f, rgb, drop_unreferenced=False)
    assert of.tolist() == [[6, 5, 7], [2, 1, 7]] and np.array_equal(ov, v) and info["vertices_out"] == 8


def test_zero_iterations_and_zero_factors_are_identities():
    v, f, _ = MCC.case("hostile_positions")
    adj = O.adjacency(len(v), f)
    assert MCC.same_bits(O.taubin(v, adj, 0), v)
    v, f, _ = MCC.case("grid_patch")
    adj = O.adjacency(len(v), f)
    for pin in (True, False):                                                # finite, non-zero positions: p + 0 * (m - p) = p in every bit
        assert MCC.same_bits(O.taubin(v, adj, 4, 0.0, 0.0, pin), v)


def test_pinned_boundary_vertices_do_not_move():
    v, f, _ = MCC.case("grid_patch")
    adj = O.adjacency(len(v), f)
    out = O.taubin(v, adj, 5)
    rim = adj["on_boundary"] != 0
    assert rim.sum() == 72 and MCC.same_bits(out[rim], v[rim]) and (MCC.bits(out[~rim]) != MCC.bits(v[~rim])).any(1).all()
    free = O.taubin(v, adj, 5, pin_boundary=False)
    assert (MCC.bits(free[rim]) != MCC.bits(v[rim])).any()


def test_relabelling_the_vertices_keeps_the_partition():
    v, f, _ = MCC.case("tiles_verts_tile")
    nv = len(v)
    perm = np.random.default_rng(5).permutation(nv)                          # old number -> new number
    label, _, faces_c, _ = O.components(nv, f)
    label2, _, faces_c2, _ = O.components(nv, perm[f])
    # the same partition: two vertices share a label before exactly when their images share one after
    pairs = {(int(a), int(b)) for a, b in zip(label, label2[perm])}
    assert len(pairs) == len(set(label.tolist())) == len(set(label2.tolist()))
    assert sorted(faces_c[faces_c > 0].tolist()) == sorted(faces_c2[faces_c2 > 0].tolist())
    assert (label2 <= np.arange(nv)).all() and (label2[label2] == label2).all()


def test_smoothing_reduces_radial_noise_on_a_sphere():
    n = 24
    theta, phi = np.meshgrid(np.linspace(0.15, np.pi - 0.15, n), np.linspace(0, 2 * np.pi, 2 * n, endpoint=False), indexing="ij")
    unit = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], -1).reshape(-1, 3)
    idx = np.arange(n * 2 * n).reshape(n, 2 * n)
    a, b = idx[:-1], np.roll(idx, -1, 1)[:-1]
    c, d = idx[1:], np.roll(idx, -1, 1)[1:]
    faces = np.concatenate([np.stack([a.ravel(), b.ravel(), c.ravel()], 1), np.stack([b.ravel(), d.ravel(), c.ravel()], 1)])
    radius = 1.0 + 0.02 * np.random.default_rng(9).standard_normal(len(unit))
    v = (unit * radius[:, None]).astype(np.float32)
    adj = O.adjacency(len(v), faces)
    out = O.taubin(v, adj, 10)
    inner = adj["on_boundary"] == 0
    rms = lambda p: float(np.sqrt(np.mean((np.linalg.norm(p[inner].astype(np.float64), axis=1) - 1.0) ** 2)))      # noqa: E731
    print(f"radial rms before {rms(v):.5f}, after 10 iterations {rms(out):.5f}")
    assert rms(out) < 0.5 * rms(v)


def test_argument_refusals():
    v, f = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    rgb = torch.zeros((3, 3), dtype=torch.uint8)
    bad = [((v.double(), f), {}, "verts"), ((v.reshape(9), f), {}, "verts"), ((v, f.long()), {}, "faces"), ((v, f.reshape(3, 1)), {}, "faces"),
           ((v, f, rgb.float()), {}, "rgb"), ((v, f, rgb[:2]), {}, "rgb"), ((v.numpy(), f), {}, "verts"),
           ((v, f), {"min_faces": -1}, "min_faces"), ((v, f), {"min_faces": 1.5}, "min_faces"), ((v, f), {"keep_largest": -1}, "keep_largest"),
           ((v, f), {"smooth_iterations": -3}, "smooth_iterations"), ((v, f), {"min_fraction": float("nan")}, "min_fraction"),
           ((v, f), {"min_fraction": float("inf")}, "min_fraction"), ((v, f), {"lam": float("nan")}, "lam"), ((v, f), {"mu": -float("inf")}, "mu"),
           ((v, f), {"mu": "much"}, "mu")]
    for args, kw, pattern in bad:
        with pytest.raises(_lib.RcmvsError, match=pattern):
            MC.clean_mesh(*args, **kw)
    with pytest.raises(_lib.RcmvsError, match="GPU"):                        # a CPU tensor outside the emulation
        MC.clean_mesh(v, f)
    with pytest.raises(_lib.RcmvsError, match="GPU"):
        MC.components(v, f)
    with pytest.raises(_lib.RcmvsError, match="GPU"):
        MC.adjacency(3, f)
    with pytest.raises(_lib.RcmvsError, match="verts_n"):
        MC.adjacency(-1, f)
    with pytest.raises(_lib.RcmvsError, match="iterations"):
        MC.taubin(v, {"verts_n": 3}, -1)


def test_the_clean_pass_is_off_by_default():
    """with none of the four options mesh_scan hands no clean-up to _mesh_views, so its summary has no "clean" key"""
    assert MC.clean_options() is None and MC.clean_options(0, 0.0, 0, 0) is None
    assert MC.clean_options(keep_largest=1) == {"min_faces": 0, "min_fraction": 0.0, "keep_largest": 1, "smooth_iterations": 0}
    for fn in (TM.mesh_scan, TM.mesh_scan_tanks):
        p = inspect.signature(fn).parameters
        assert [p[k].default for k in ("min_faces", "min_fraction", "keep_largest", "smooth")] == [0, 0.0, 0, 0]
    assert inspect.signature(TM._mesh_views).parameters["clean"].default is None
    seen = {}

    def views_only(views, meshfilename, *args):
        seen["clean"] = args[-1]
        return {"mesh": meshfilename}

    import unittest.mock as mock
    with mock.patch.object(TM, "filtered_views", lambda *a, **k: {}), mock.patch.object(TM, "_mesh_views", views_only):
        assert "clean" not in TM.mesh_scan("p", "s", "o", "m.ply", 0.8, 3, 0.5, 0.01) and seen["clean"] is None
        TM.mesh_scan("p", "s", "o", "m.ply", 0.8, 3, 0.5, 0.01, smooth=2)
        assert seen["clean"]["smooth_iterations"] == 2


def test_header_is_an_extension_header():
    assert any(p.endswith("mesh_clean.h") for p in _lib.EXT_HEADERS)
    names = {"components", "component_table", "select", "gather", "adjacency", "taubin_step"}
    for n in names:
        plain, timed = _lib.EXT_SIGNATURES["rcmvs_mc_" + n], _lib.EXT_SIGNATURES["rcmvs_mc_" + n + "_timed"]
        assert timed[:len(plain) - 1] == plain[:-1] and len(timed) == len(plain) + 2
    assert _lib.CONSTANTS["RCMVS_VERSION"] == 106 and MC.SORT_LIMIT % 2 == 0
