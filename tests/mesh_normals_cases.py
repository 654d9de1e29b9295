"""The cases and checks of the mesh normals (csrc/mesh_normals.hip through rc_mvsnet_amd/mesh_normals.py), shared by
tests/test_gpu_mesh_normals.py (device "cuda:0") and tests/test_mesh_normals_emu_cpu.py (the CPU emulation, device "cpu"), against
tests/mesh_normals_oracle.py.  Every comparison with the oracle is bit equality: face normals, vertex normals and normal-map floats
as their 32-bit patterns, smooth bytes, colour bytes and counters.  The tolerances of the known answers are derived next to their
asserts."""
import functools
import json
import os

import numpy as np
import torch

import mesh_clean_cases as MCC
import mesh_normals_oracle as O
import mesh_render_cases as MRC
import tsdf_cases as C
from mesh_clean_cases import INT_MAX, INT_MIN, bits, host, to_dev
from rc_mvsnet_amd import _lib, data_io, dtu_io, mesh_decimate as MD, mesh_normals as MN, mesh_render as MR, tsdf_mesh as TM

WEIGHTS = ("area", "sphere")
F32_MAX = float(np.finfo(np.float32).max)


def _mesh(verts, faces):
    return np.ascontiguousarray(verts, np.float32).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)


def _positions(nv, seed):
    return np.random.default_rng(seed).standard_normal((nv, 3)).astype(np.float32)


# ---- builders: each -> (verts (nv,3) fp32, faces (nf,3) int32) -----------------------------------------------------------------------
def strip(n, order="shuffled", nv=None, seed=0):
    """n triangles (p, p + 1, p + 2) along a strip; nv: the strip's n + 2 vertices take random distinct numbers below nv, so the
    rest is unreferenced and the keys use all the bits nv needs.  order: the faces ascending, descending or shuffled."""
    rng = np.random.default_rng(seed + n)
    number = np.arange(n + 2) if nv is None else np.sort(rng.choice(nv, n + 2, replace=False))
    if nv is not None:
        number[-1] = nv - 1                                          # the largest key below the sentinel is used
    faces = np.stack([number[:-2], number[1:-1], number[2:]], 1)
    faces[1::2] = faces[1::2][:, [0, 2, 1]]                          # a strip alternates: keep every face's normal on one side
    if order == "descending":
        faces = faces[::-1]
    elif order == "shuffled":
        faces = faces[rng.permutation(n)]
    return _mesh(_positions(n + 2 if nv is None else nv, seed + 1), faces)


def fan(n):
    """n triangles round vertex 0 on a cone: n corners at one vertex"""
    ang = 2 * np.pi * np.arange(n + 1) / (n + 1)
    rim = np.stack([np.cos(ang), np.sin(ang), -0.3 + 0.05 * np.cos(5 * ang)], 1)
    verts = np.concatenate([[[0.0, 0.0, 0.0]], rim])
    faces = np.stack([np.zeros(n, np.int64), 1 + np.arange(n), 2 + np.arange(n)], 1)
    return _mesh(verts, faces)


def specks(n):
    return _mesh(_positions(3 * n, n), np.arange(3 * n).reshape(n, 3))


def grid(m, z=0.0, step=1.0):
    """(m + 1)^2 vertices in the plane z, 2 m^2 faces whose normal (b - a) x (c - a) is +z"""
    idx = np.arange((m + 1) * (m + 1)).reshape(m + 1, m + 1)
    y, x = np.mgrid[0:m + 1, 0:m + 1]
    verts = np.stack([x.ravel() * step, y.ravel() * step, np.full(x.size, z)], 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    faces = np.stack([np.stack([a, b, c], 1), np.stack([b, d, c], 1)], 1).reshape(-1, 3)
    return _mesh(verts, faces)


def invalid_and_repeated():
    v, f = grid(3)
    nv = len(v)
    bad = [(-1, 1, 2), (0, nv, 2), (0, 1, INT_MAX), (INT_MIN, 1, 2), (1, 1, 2), (3, 2, 3), (4, 4, 4), (nv - 1, nv, nv + 1)]
    return _mesh(v + _positions(nv, 3) * 0.1, np.concatenate([f[:5], bad, f[5:]]))


def hostile():
    """a 6 x 6 grid with one vertex each NaN, +inf, -inf (their neighbours keep faces of finite vertices), then separate triangles
    of the largest finite values, 1e30 and denormals"""
    v, f = grid(6)
    v = v + _positions(len(v), 5) * 0.1
    v[8, 1], v[17, 0], v[30, 2] = np.nan, np.inf, -np.inf
    big, tiny = F32_MAX, 1.401298464324817e-45
    extra = [(big, -big, big), (-big, big, -big), (big, big, -big),            # differences of 2^129, products of 2^258
             (1e30, 0, 0), (0, 1e30, 0), (0, 0, -1e30),
             (tiny, 0, 0), (0, 3 * tiny, 0), (0, 0, 5 * tiny),                 # F components of 2^-298 and below, squares underflow
             (big, 0, 0), (0, tiny, 0), (0, 0, 1.0),
             (1e-20, 2e-20, 0), (3e-20, 0, 1e-20), (0, 1e-20, 5e-20)]
    n = len(v)
    faces = np.concatenate([f, n + np.arange(len(extra)).reshape(-1, 3)])
    return _mesh(np.concatenate([v, np.asarray(extra, np.float32)]), faces)


def degenerate():
    """a zero-area face of three collinear points, a face with a zero-length edge between two vertex numbers, each sharing vertices
    with a proper face"""
    verts = [(0, 0, 0), (1, 1, 1), (2, 2, 2), (0, 1, 0),            # 0 1 2 collinear; (0, 1, 3) proper
             (5, 0, 0), (5, 0, 0), (6, 1, 0), (5, 2, 1)]            # 4 and 5 coincide; (4, 6, 7) proper
    return _mesh(verts, [(0, 1, 2), (0, 1, 3), (4, 5, 6), (4, 6, 7), (2, 2, 3)])


def opposite_twins():
    """two coincident faces of opposite orientation: their three vertices cancel; a third vertex set keeps a normal"""
    v = _positions(6, 9)
    return _mesh(v, [(0, 1, 2), (0, 2, 1), (3, 4, 5)])


def signed_zeros():
    verts = [(-0.0, 0.0, -0.0), (1.0, -0.0, 0.0), (0.0, 1.0, -0.0), (-0.0, -0.0, 1.0), (0.0, 0.0, 0.0)]
    return _mesh(verts, [(0, 1, 2), (0, 2, 3), (0, 3, 1), (4, 2, 1), (1, 2, 3)])


SPHERE_SEED, SPHERE_RINGS, SPHERE_SEGMENTS, SPHERE_RADIUS, SPHERE_CENTRE = 20, 7, 9, 2.5, (0.5, -0.25, 0.75)


def uv_sphere(rings=SPHERE_RINGS, segments=SPHERE_SEGMENTS, radius=SPHERE_RADIUS, centre=SPHERE_CENTRE, jitter=0.35, seed=SPHERE_SEED):
    """rings x segments vertices and two poles ON the sphere (fp64, rounded to fp32), their angles jittered by a fraction of the
    spacing (numpy's default_rng(seed).uniform); faces oriented outwards.  7 x 9: 65 vertices, 126 faces."""
    rng = np.random.default_rng(seed)
    theta = (np.arange(1, rings + 1)[:, None] + jitter * rng.uniform(-1, 1, (rings, segments))) * np.pi / (rings + 1)
    phi = (np.arange(segments)[None, :] + jitter * rng.uniform(-1, 1, (rings, segments))) * 2 * np.pi / segments
    unit = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], -1).reshape(-1, 3)
    unit = np.concatenate([[[0.0, 0.0, 1.0]], unit, [[0.0, 0.0, -1.0]]])
    verts = np.asarray(centre) + radius * unit
    idx = 1 + np.arange(rings * segments).reshape(rings, segments)
    nxt = np.roll(idx, -1, 1)
    south = 1 + rings * segments
    faces = [np.stack([np.zeros(segments, np.int64), idx[0], nxt[0]], 1), np.stack([np.full(segments, south), nxt[-1], idx[-1]], 1)]
    for r in range(rings - 1):
        faces += [np.stack([idx[r], idx[r + 1], nxt[r + 1]], 1), np.stack([idx[r], nxt[r + 1], nxt[r]], 1)]
    return _mesh(verts, np.concatenate(faces))


CORNER_COUNTS = (255, 258, 2046, 2049, 4095, 4098)                   # 3 nf round the radix block (256) and the scan tile (2048), and twice the tile
PASSES = {"nv_200": (200, 1), "nv_300": (300, 2), "nv_70000": (70000, 3)}

CASES = {
    "nv_0_nf_0": lambda: _mesh(np.zeros((0, 3)), np.zeros((0, 3))),
    "nv_0_with_faces": lambda: _mesh(np.zeros((0, 3)), [(0, 1, 2), (0, 0, 0)]),
    "nf_0": lambda: _mesh(_positions(5, 0), np.zeros((0, 3))),
    "one_face": lambda: _mesh([(0, 0, 0), (2, 0, 0.5), (0.25, 3, 0)], [(0, 1, 2)]),
    "strip_ascending": lambda: strip(40, "ascending", seed=4),
    "strip_descending": lambda: strip(40, "descending", seed=4),
    "strip_shuffled": lambda: strip(40, "shuffled", seed=4),
    "fan_48": lambda: fan(48),
    "fan_50": lambda: fan(50),
    "fan_600": lambda: fan(600),
    "specks_4097": lambda: specks(4097),
    "invalid_and_repeated": invalid_and_repeated,
    "hostile": hostile,
    "degenerate": degenerate,
    "opposite_twins": opposite_twins,
    "signed_zeros": signed_zeros,
    "grid_plane": lambda: grid(5),
    "uv_sphere": uv_sphere,
}
for _n in CORNER_COUNTS:
    CASES[f"corners_{_n}"] = functools.partial(strip, _n // 3, "shuffled")
for _name, (_nv, _) in PASSES.items():
    CASES[_name] = functools.partial(strip, 50, "shuffled", _nv)


@functools.lru_cache(maxsize=None)
def case(name):
    out = CASES[name]()
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, weight):
    v, f = case(name)
    n, stats = O.vertex_normals(v, f, weight)
    n.setflags(write=False)
    return n, stats


@functools.lru_cache(maxsize=None)
def reference_faces(name):
    n = O.face_normals(*case(name))
    n.setflags(write=False)
    return n


def case_keys():
    return [(name, w) for name in CASES for w in WEIGHTS]


def radix_passes(nv):
    return max(1, (int(nv).bit_length() + 7) // 8)


def sine_to(normals, directions):
    """the sine of the angle between rows of two (n,3) arrays, fp64"""
    a, b = np.asarray(normals, np.float64), np.asarray(directions, np.float64)
    return np.linalg.norm(np.cross(a, b), axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


def check_known(name, weight):
    """the hand answers, on the oracle alone"""
    v, f = case(name)
    n, st = reference(name, weight)
    fn = reference_faces(name)
    nv, nf = len(v), len(f)
    assert st["vertices_with_normal"] + st["vertices_unreferenced"] + st["vertices_cancelled"] == nv, st
    assert st["faces_invalid"] + st["faces_nonfinite"] <= nf and (weight == "sphere" or st["corners_skipped"] == 0)
    assert np.isfinite(n).all() and np.isfinite(fn).all(), name          # whatever the input holds
    length = np.linalg.norm(n.astype(np.float64), axis=1)
    assert (np.abs(length[length > 0] - 1.0) < 1e-6).all()
    if name in ("nv_0_nf_0", "nv_0_with_faces", "nf_0"):
        assert st["vertices_unreferenced"] == nv and st["faces_invalid"] == (2 if name == "nv_0_with_faces" else 0) and not n.any()
    if name == "one_face":
        assert st["vertices_with_normal"] == 3 and np.array_equal(bits(n), bits(np.repeat(fn, 3, 0)))       # one face: its own normal, whatever the weight
    if name.startswith("corners_"):
        assert 3 * nf == int(name.split("_")[1]) and st["vertices_with_normal"] == nv
    if name in PASSES:
        assert nv == PASSES[name][0] and radix_passes(nv) == PASSES[name][1] and st["vertices_unreferenced"] == nv - 52 and int(f.max()) == nv - 1
    if name.startswith("fan_"):
        assert int((f == 0).sum()) == int(name.split("_")[1]) and n[0, 2] > 0.9
    if name == "specks_4097":
        assert st["vertices_with_normal"] == 3 * 4097 and np.array_equal(bits(n), bits(np.repeat(fn, 3, 0)))
    if name == "invalid_and_repeated":
        assert st["faces_invalid"] == 8 and st["vertices_with_normal"] == nv
    if name == "hostile":
        # Six faces meet at each of the three non-finite vertices and are skipped; their neighbours keep faces of finite vertices.  The
        # five separate faces all have normals: the largest finite values give products of 2^258 and squared lengths of 2^518, the
        # denormals an F of 2^-298 whose squared length, 2^-596, is far above the smallest fp64.
        assert st["faces_nonfinite"] == 6 + 6 + 6 and st["faces_invalid"] == 0 and st["faces_degenerate"] == 0, st
        for bad in (8, 17, 30):
            neighbours = sorted(set(f[(f == bad).any(1)].ravel().tolist()) - {bad})
            assert len(neighbours) == 6 and (length[neighbours] > 0).all() and length[bad] == 0
        assert (length[49:] > 0).all() and fn[-5:].any(1).all() and st["vertices_unreferenced"] == 3 and st["vertices_cancelled"] == 0, (length[49:], st)
    if name == "degenerate":
        assert st["faces_degenerate"] == 2 and st["faces_invalid"] == 1 and not fn[0].any() and not fn[2].any() and fn[1].any() and fn[3].any()
        assert st["corners_skipped"] == (2 if weight == "sphere" else 0), st     # the two corners at the ends of the zero-length edge
        # vertex 2 has the collinear face alone: a zero sum, cancelled; vertex 5 the zero-length-edge face alone: under SPHERE its corner
        # is skipped and it is unreferenced, under AREA its sum is zero
        assert not n[2].any() and not n[5].any() and n[0].any() and n[4].any()
        assert (st["vertices_cancelled"], st["vertices_unreferenced"]) == ((1, 1) if weight == "sphere" else (2, 0)), st
    if name == "opposite_twins":
        assert st["vertices_cancelled"] == 3 and not n[:3].any() and st["vertices_with_normal"] == 3 and fn[0].any()
        assert (fn[0] == -fn[1]).all()
    if name == "grid_plane":
        # every F is (0, 0, k) and every C / (l1 l2) is (0, 0, c): the sums are exact multiples along z and sqrt(fl(x x)) == x
        assert (n == np.array([0.0, 0.0, 1.0], np.float32)).all() and (fn == np.array([0.0, 0.0, 1.0], np.float32)).all()
    if name.startswith("strip_"):
        pass                                                             # the orders are compared with one another in check_orders
    if name == "uv_sphere":
        assert (nv, nf) == (65, 126)
        radial = v.astype(np.float64) - np.asarray(SPHERE_CENTRE)
        s = sine_to(n, radial)
        print(f"uv sphere {weight}: largest sine of the angle to the radius {s.max():.3g}")
        if weight == "sphere":
            # Max's weights are exact for vertices on a sphere.  The vertices are rounded to fp32: each moves by at most 2^-24 of its
            # largest coordinate (below 4: 2.4e-7) against edges of 1.2 and more, a tilt of some 2e-7 in the worst case; the fp64
            # arithmetic adds 1e-15 and the rounding of N to fp32 6e-8.
            assert s.max() < 1e-6, s.max()
        else:
            assert s.max() > 0.1, s.max()                                # the area-weighted mean follows the jittered faces


def assert_vertex_normals(got, stats, name, weight, what=None):
    want, wstats = reference(name, weight)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    g = host(got)
    if not np.array_equal(bits(g), bits(want)):
        at = np.argwhere(bits(g) != bits(want))[:5]
        print(what or (name, weight), "normals differ at", at.tolist(), "got", [g[tuple(i)] for i in at], "want", [want[tuple(i)] for i in at])
    assert np.array_equal(bits(g), bits(want)), what or (name, weight)
    assert stats == wstats, (what or (name, weight), stats, wstats)


def check_case(dev, name, weight, twice=True):
    check_known(name, weight)
    v, f = case(name)
    tv, tf, _ = to_dev(dev, v, f, None)
    got, stats = MN.vertex_normals(tv, tf, weight)
    print(f"{name} {weight}: {stats}")
    assert_vertex_normals(got, stats, name, weight)
    if weight == "area":
        fn = MN.face_normals(tv, tf)
        assert fn.dtype == torch.float32 and np.array_equal(bits(host(fn)), bits(reference_faces(name))), name
    if twice:
        again, raw = MN.vertex_normals_device(tv, tf, weight)
        assert torch.equal(got.view(torch.int32), again.view(torch.int32)) and MN.stats_dict(raw, weight) == stats and int(raw[len(MN.STAT_NAMES):].sum()) == 0


def check_orders(dev):
    """one strip with its faces ascending, descending and shuffled: each order equals its own oracle (check_case); the orders agree
    with one another to the rounding of a sum of at most three terms"""
    ref = {o: reference(f"strip_{o}", "sphere")[0].astype(np.float64) for o in ("ascending", "descending", "shuffled")}
    for o in ("descending", "shuffled"):
        assert np.abs(ref[o] - ref["ascending"]).max() < 1e-6
    for o in ref:
        for w in WEIGHTS:
            check_case(dev, f"strip_{o}", w, twice=False)


def check_flip(dev):
    """b and c swapped in every face: every face and vertex normal negated under AREA (==, so that zeros of either sign match)"""
    for name in ("strip_shuffled", "fan_50", "uv_sphere", "hostile", "degenerate"):
        v, f = case(name)
        tv, tf, _ = to_dev(dev, v, f, None)
        tg = tf[:, [0, 2, 1]].contiguous()
        a, b = MN.vertex_normals(tv, tf, "area"), MN.vertex_normals(tv, tg, "area")
        assert bool((a[0] == -b[0]).all()) and {k: x for k, x in a[1].items()} == {k: x for k, x in b[1].items()}, name
        assert bool((MN.face_normals(tv, tf) == -MN.face_normals(tv, tg)).all()), name
        assert np.array_equal(bits(host(b[0])), bits(O.vertex_normals(v, f[:, [0, 2, 1]], "area")[0]))


def check_extraction(dev):
    """the two spheres and the speck of mesh_clean_cases, as extracted and after decimate at 2 voxels: equal to the oracle in every
    bit under both weights, every vertex with a normal, and the normals point away from the centre of the sphere whose surface is
    nearest (the extraction is oriented from the inside to the outside)"""
    verts, faces, rgb = MCC.scene_volume(dev).extract(1)
    meshes = {"extracted": (verts, faces), "decimated": MD.decimate(verts, faces, rgb, cell=2.0)[:2]}
    for what, (mv, mf) in meshes.items():
        v, f = host(mv), host(mf)
        for w in WEIGHTS:
            want, wstats = O.vertex_normals(v, f, w)
            got, stats = MN.vertex_normals(mv, mf, w)
            print(f"extraction {what} {w}: {len(f)} faces, {stats}")
            assert np.array_equal(bits(host(got)), bits(want)) and stats == wstats, (what, w)
            assert stats["faces_invalid"] == stats["faces_nonfinite"] == stats["vertices_unreferenced"] == 0
            centres = np.array([c for c, _ in MCC.SCENE_SPHERES])
            radii = np.array([r for _, r in MCC.SCENE_SPHERES])
            near = centres[np.argmin(np.abs(np.linalg.norm(v[:, None, :].astype(np.float64) - centres[None], axis=2) - radii[None]), axis=1)]
            outward = (want.astype(np.float64) * (v - near)).sum(1)
            if what == "extracted":
                assert stats["vertices_with_normal"] == len(v) and (outward > 0).all(), (what, w, float(outward.min()))
            else:
                assert (outward > 0).mean() > 0.95
        assert np.array_equal(bits(host(MN.face_normals(mv, mf))), bits(O.face_normals(v, f)))


def check_refusals(dev):
    v, f = case("one_face")
    tv, tf, _ = to_dev(dev, v, f, None)
    n = torch.zeros((3, 3), dtype=torch.float32).to(dev)
    img = torch.zeros((1, 2, 2), dtype=torch.int32).to(dev)
    for bad, pattern in ((lambda: MN.vertex_normals(tv, tf, "angle"), "weight"), (lambda: MN.vertex_normals(tv, tf.long(), "area"), "faces"),
                         (lambda: MN.vertex_normals(tv.double(), tf), "verts"), (lambda: MN.face_normals(tv[:, :2], tf), "verts"),
                         (lambda: MN.shade(tv, tf, n[:2], MRC.PIX[None], img), "normals"), (lambda: MN.shade(tv, tf, n, MRC.PIX[None], img.long()), "face_image"),
                         (lambda: MN.shade(tv, tf, n, np.zeros((2, 16)), img), "cameras"), (lambda: MN.shade(tv, tf, n, MRC.PIX[None], img, near=0.0), "near"),
                         (lambda: MN.shade(tv, tf, n, MRC.PIX[None], img, near=float("nan")), "near"),
                         (lambda: MN.shade(tv, tf, n, MRC.PIX[None], img, background=(0, 0, 256)), "background"),
                         (lambda: MN.normals_options("angle"), "weight")):
        try:
            bad()
        except _lib.RcmvsError as e:
            assert pattern in str(e), (pattern, str(e))
        else:
            raise AssertionError(f"a bad argument was accepted ({pattern})")
    assert MN.normals_options(None) is None and MN.normals_options("sphere") == {"weight": "sphere"}


# ---- the normal pass ----------------------------------------------------------------------------------------------------------------
SHADE_CASES = ("right_triangle", "shared_edge_00", "shared_edge_01", "fan64", "coplanar_twins", "three_views")
SHADE_SIZES = ((1, 1), (7, 5), (64, 48))


def shade_keys():
    return [(name, W, H, cull) for name in SHADE_CASES for (W, H) in SHADE_SIZES for cull in ("none", "back")]


@functools.lru_cache(maxsize=None)
def shade_normals(name):
    """the SPHERE normals of a render case's mesh (the oracle's), read-only"""
    v, f, c, cams = MRC.case(name)
    n = O.vertex_normals(v, f, "sphere")[0]
    n.setflags(write=False)
    return n


def assert_shade(got, want, what):
    assert got["normal"].dtype == torch.float32 and got["smooth"].dtype == torch.uint8 and got["normal_rgb"].dtype == torch.uint8
    assert np.array_equal(bits(host(got["normal"])), bits(want["normal"])), what
    assert np.array_equal(host(got["smooth"]), want["smooth"]), what
    assert np.array_equal(host(got["normal_rgb"]), want["normal_rgb"]), what


def check_shade_case(dev, name, W, H, cull, background=(7, 8, 9)):
    """the render's own face image (equal to the render oracle's: tests/test_gpu_mesh_render.py) through the normal pass"""
    v, f, c, cams = MRC.case(name)
    face = MRC.reference(name, W, H, cull)["face"]
    n = shade_normals(name)
    want = O.shade(v, f, n, cams, face, MRC.NEAR, background)
    tv, tf, _ = to_dev(dev, v, f, None)
    tn, timg = torch.from_numpy(np.array(n)).to(dev), torch.from_numpy(np.array(face)).to(dev)
    got = MN.shade(tv, tf, tn, cams, timg, near=MRC.NEAR, background=background)
    assert_shade(got, want, (name, W, H, cull))
    covered = face >= 0
    assert (want["normal_rgb"][~covered] == background).all() and not want["normal"][~covered].any() and not want["smooth"][~covered].any()
    if name == "three_views" and (W, H) == (64, 48):
        # a closed surface with outward normals seen from outside: the interpolated normals face the camera
        assert covered.sum() > 900 and (want["normal"][covered][:, 2] < 0).all() and (want["normal_rgb"][covered][:, 2] >= 128).all()
        ln = np.linalg.norm(want["normal"][covered].astype(np.float64), axis=1)
        assert np.abs(ln - 1).max() < 1e-6
        for k in range(len(cams)):                                       # three views in one call against three calls
            one = MN.shade(tv, tf, tn, cams[k:k + 1], timg[k:k + 1].contiguous(), near=MRC.NEAR, background=background)
            for key in got:
                assert torch.equal(got[key][k:k + 1], one[key]), (k, key)
        through = MR.render(tv, tf, None, cams, H, W, near=MRC.NEAR, cull=cull, background=background, normals=tn)
        assert np.array_equal(host(through["face"]), face)
        assert_shade(through, want, "through render")


def check_plane(dev):
    """the plane z = 2 in the identity camera with normals (0, 0, -1): normal map exactly (0, 0, -1), smooth 255, colour (128, 128, 255)"""
    v, f, c, cams = MRC.quad_grid(shuffle=False)
    n = np.zeros_like(v)
    n[:, 2] = -1.0
    tv, tf, _ = to_dev(dev, v, f, None)
    tn = torch.from_numpy(n).to(dev)
    out = MR.render(tv, tf, None, cams, 48, 64, near=MRC.NEAR, normals=tn)
    covered = host(out["face"]) >= 0
    assert covered.sum() == 27 * 27
    assert (host(out["normal"])[covered] == np.array([0.0, 0.0, -1.0], np.float32)).all() and (host(out["smooth"])[covered] == 255).all()
    assert (host(out["normal_rgb"])[covered] == (128, 128, 255)).all() and (host(out["normal_rgb"])[~covered] == 0).all()
    assert_shade(out, O.shade(v, f, n, cams, host(out["face"]), MRC.NEAR), "plane")
    # vertex normals that vanish or cancel in the interpolation: a zero normal, smooth 0, grey
    zero = MN.shade(tv, tf, torch.zeros_like(tn), cams, out["face"], near=MRC.NEAR, background=(1, 2, 3))
    assert (host(zero["normal_rgb"])[covered] == 128).all() and (host(zero["normal_rgb"])[~covered] == (1, 2, 3)).all()
    assert not host(zero["normal"]).any() and not host(zero["smooth"]).any()
    assert_shade(zero, O.shade(v, f, np.zeros_like(n), cams, host(out["face"]), MRC.NEAR, (1, 2, 3)), "zero normals")


def check_bad_face_image(dev):
    """a face image that holds -1, nf, INT_MAX, INT_MIN, the number of an invalid face, of a face behind the camera and of a face of
    no area in the image: background pixels, no fault; the proper face's number anywhere in the image is shaded by extrapolation"""
    v, f, c, cams = MRC.case("hostile")
    nf = len(f)
    invalid = next(i for i, t in enumerate(f.tolist()) if not O.RO.face_valid(*t, len(v)))
    img = np.array([[[-1, nf, INT_MAX, INT_MIN], [invalid, 2, 3, 0], [nf - 1, nf + 1, -2, 5]]], np.int32)
    n = O.vertex_normals(v, f, "area")[0]
    want = O.shade(v, f, n, cams[:1], img, MRC.NEAR, (9, 8, 7))
    tv, tf, _ = to_dev(dev, v, f, None)
    got = MN.shade(tv, tf, torch.from_numpy(n).to(dev), cams[:1], torch.from_numpy(img).to(dev), near=MRC.NEAR, background=(9, 8, 7))
    assert_shade(got, want, "bad face image")
    assert (want["normal_rgb"][0, 0] == (9, 8, 7)).all() and (want["normal_rgb"][0, 1, 0] == (9, 8, 7)).all() and not want["normal"][0, 0].any()
    assert (want["normal_rgb"][0, 1, 3] != (9, 8, 7)).any()             # face 0 (z = near exactly) is usable
    # no mesh at all under an image that names faces
    e = MN.shade(torch.zeros((0, 3)).to(dev), torch.zeros((0, 3), dtype=torch.int32).to(dev), torch.zeros((0, 3)).to(dev), cams[:1], torch.from_numpy(img).to(dev),
                 near=MRC.NEAR, background=(9, 8, 7))
    assert (host(e["normal_rgb"]) == (9, 8, 7)).all() and not host(e["normal"]).any()


def check_smooth_beats_flat(dev):
    """A 16 x 24 UV sphere (unjittered, radius 1 at z = 3) with SPHERE normals rendered at 64 x 48.  On the pixels at least 2 px
    inside the silhouette the mean angle between the interpolated normal and the sphere's normal at the pixel's ray is smaller than
    the mean angle between the flat face normal and that normal."""
    centre = np.array([0.1, -0.05, 3.0])
    v, f = uv_sphere(16, 24, 1.0, tuple(centre), jitter=0.0)
    cam = C.cam_row(np.eye(3), (0.0, 0.0, 0.0), 40.0, 40.0, 31.5, 23.5)[None]
    tv, tf, _ = to_dev(dev, v, f, None)
    normals, stats = MN.vertex_normals(tv, tf, "sphere")
    assert stats["vertices_with_normal"] == len(v)
    out = MR.render(tv, tf, None, cam, 48, 64, near=0.5, cull="back", normals=normals)
    face, interp = host(out["face"])[0], host(out["normal"])[0].astype(np.float64)
    covered = face >= 0
    inside = np.zeros_like(covered)
    inside[2:-2, 2:-2] = True
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            inside[2:-2, 2:-2] &= covered[2 + dy:covered.shape[0] - 2 + dy, 2 + dx:covered.shape[1] - 2 + dx]
    assert inside.sum() > 300
    ys, xs = np.nonzero(inside)
    ray = np.stack([(xs - 31.5) / 40.0, (ys - 23.5) / 40.0, np.ones(len(xs))], 1)
    A, B, Cq = (ray * ray).sum(1), -2 * (ray @ centre), centre @ centre - 1.0
    disc = B * B - 4 * A * Cq
    assert (disc > 0).all()                                              # the mesh is inscribed: a ray that meets it meets the sphere
    t = (-B - np.sqrt(disc)) / (2 * A)
    truth = ray * t[:, None] - centre
    flat = host(MN.face_normals(tv, tf)).astype(np.float64)[face[ys, xs]]
    angle = lambda a: np.degrees(np.arcsin(np.clip(sine_to(a, truth), 0, 1)))          # noqa: E731
    smooth_mean, flat_mean = float(angle(interp[ys, xs]).mean()), float(angle(flat).mean())
    print(f"sphere 16 x 24 at 64 x 48, {int(inside.sum())} pixels: mean angle to the analytic normal {smooth_mean:.3f} deg interpolated, {flat_mean:.3f} deg flat")
    assert smooth_mean < flat_mean
    assert ((interp[ys, xs] * truth).sum(1) > 0).all()


# ---- PLY, hooks and command lines ---------------------------------------------------------------------------------------------------
def check_mesh_scan(dev, tmp_path):
    """mesh_scan without normals: PLY bytes and summary keys as the TSDF suite's oracle fixes them (what the parent commit gives);
    with normals="sphere": the same keys plus "normals", the same mesh with nx ny nz equal to the oracle's normals in every bit, read
    back by read_ply_mesh_normals, and by read_ply_mesh / read_ply_mesh_rgb as it was; with render_dir too, the two more PNGs per view;
    then the command line of mesh_normals on the plain PLY writes the same bytes."""
    from PIL import Image
    pair_folder, out_folder = C.write_scan(tmp_path)
    plain_ply, ply, cli_ply, rdir = (str(tmp_path / "out" / n) for n in ("plain.ply", "normals.ply", "cli.ply", "render"))
    kw = dict(resolution=32, device=dev)
    plain = TM.mesh_scan(pair_folder, out_folder, out_folder, plain_ply, C.PROB, C.NCONS, C.DIST, C.DEPTH, **kw)
    assert list(plain) == ["mesh", "origin", "dims", "voxel", "trunc", "min_weight", "views", "vertices", "faces", "unreferenced_vertices", "observed_voxels"]
    views = TM.filtered_views(pair_folder, out_folder, out_folder, C.PROB, C.NCONS, C.DIST, C.DEPTH, device=dev)
    want, _ = C.oracle_mesh_of(views, plain)
    with open(plain_ply, "rb") as fh:
        plain_bytes = fh.read()
    assert plain_bytes == TM.mesh_ply_bytes(want["verts"], want["faces"], want["rgb"]) and b"property float nx" not in plain_bytes
    summary = TM.mesh_scan(pair_folder, out_folder, out_folder, ply, C.PROB, C.NCONS, C.DIST, C.DEPTH, normals="sphere", render_dir=rdir, **kw)
    assert list(summary) == list(plain) + ["normals", "render"]
    assert {k: v for k, v in summary.items() if k not in ("mesh", "normals", "render")} == {k: v for k, v in plain.items() if k != "mesh"}
    wn, wstats = O.vertex_normals(want["verts"], want["faces"], "sphere")
    assert summary["normals"] == wstats and wstats["vertices_with_normal"] > 0
    v, f, c, n = dtu_io.read_ply_mesh_normals(ply)
    assert np.array_equal(bits(v), bits(want["verts"])) and np.array_equal(f, want["faces"]) and np.array_equal(c, want["rgb"]) and np.array_equal(bits(n), bits(wn))
    v2, f2, c2 = dtu_io.read_ply_mesh_rgb(ply)
    v3, f3 = dtu_io.read_ply_mesh(ply)
    assert np.array_equal(bits(v2), bits(v)) and np.array_equal(f2, f) and np.array_equal(c2, c) and np.array_equal(bits(v3), bits(v)) and np.array_equal(f3, f)
    with open(ply, "rb") as fh:
        assert fh.read() == TM.mesh_ply_bytes(want["verts"], want["faces"], want["rgb"], normals=wn)
    V, H, W = views["depth"].shape
    assert len(os.listdir(os.path.join(rdir, "render"))) == 4 * V
    tv, tf, tc = to_dev(dev, want["verts"], want["faces"], want["rgb"])
    out = MR.render(tv, tf, tc, views["cams"], H, W, normals=torch.from_numpy(wn).to(dev))
    for kind, key, mode in (("smooth", "smooth", "L"), ("normal", "normal_rgb", "RGB")):
        with Image.open(os.path.join(rdir, "render", f"00000002_{kind}.png")) as im:
            assert im.size == (W, H) and im.mode == mode and np.array_equal(np.asarray(im), host(out[key][2]))
    assert (host(out["face"]) >= 0).sum() > 0
    # the command line on the plain PLY
    total = MN.main(["--in", plain_ply, "--out", cli_ply, "--weight", "sphere", "--device", dev])
    with open(ply, "rb") as a, open(cli_ply, "rb") as b:
        assert a.read() == b.read()
    assert {k: total[k] for k in wstats} == wstats and total["vertices"] == len(v) and total["faces"] == len(f) and json.dumps(total)
    # mesh_render's command line with --normals
    dst = str(tmp_path / "cli_render")
    MR.main(["--mesh", plain_ply, "--pair-folder", pair_folder, "--scan-folder", out_folder, "--out", dst, "--size", str(H), str(W), "--normals", "sphere",
             "--device", dev])
    with Image.open(os.path.join(dst, "render", "00000002_normal.png")) as im:
        assert np.array_equal(np.asarray(im), host(out["normal_rgb"][2]))
    # the block-sparse volume takes the same way through _mesh_views
    sn = str(tmp_path / "out" / "sparse_normals.ply")
    b = TM.mesh_scan(pair_folder, out_folder, out_folder, sn, C.PROB, C.NCONS, C.DIST, C.DEPTH, sparse=True, normals="area", **kw)
    assert list(b)[-1] == "normals" and "active_blocks" in b and b["normals"]["weight"] == "area"
    vb, fb, cb, nb = dtu_io.read_ply_mesh_normals(sn)
    wb, wbstats = O.vertex_normals(vb, fb, "area")
    assert len(fb) == b["faces"] > 0 and np.array_equal(bits(nb), bits(wb)) and b["normals"] == wbstats
