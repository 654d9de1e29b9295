"""The cases and checks of the mesh texturing (csrc/mesh_texture.hip through rc_mvsnet_amd/mesh_texture.py), shared by
tests/test_gpu_mesh_texture.py (device "cuda:0") and tests/test_mesh_texture_emu_cpu.py (the CPU emulation, device "cpu"), against
tests/mesh_texture_oracle.py.  Every comparison with the oracle is equality in every bit: best, classes, the sorted order, the table,
texel coordinates, owners, atlas bytes, counters and textured pixels.  The bounds of the known answers are derived next to their
asserts.

Most meshes are built in the image as tests/mesh_render_cases.py builds them: with the camera PIX (R = I, t = 0, fx = fy = 1,
cx = cy = 0) a vertex (u z, v z, z) with z a power of two lands on pixel position (u, v) exactly.  Images are at most 64 x 48 and
atlases at most 256 x 256, but for the one case whose face must be longer than the largest class's 1021 texels."""
import functools
import json
import os
from fractions import Fraction

import numpy as np
import torch

import mesh_render_cases as MRC
import mesh_texture_oracle as O
import tsdf_cases as C
from mesh_clean_cases import INT_MAX, INT_MIN, host, to_dev
from rc_mvsnet_amd import _lib, dtu_io, mesh_decimate as MD, mesh_render as MR, mesh_texture as MT, tsdf_mesh as TM

NEAR = MRC.NEAR
PIX = MRC.PIX


def ramp(H, W):
    """three integer ramps, each linear in (u, v) and within a byte up to 64 x 48: 2u + v, u + 2v, 255 - (u + v)"""
    v, u = np.mgrid[0:H, 0:W]
    return np.stack([2 * u + v, u + 2 * v, 255 - (u + v)], -1).astype(np.uint8)


RAMP = (lambda u, v: 2 * u + v, lambda u, v: u + 2 * v, lambda u, v: 255 - (u + v))


def noise(V, H, W, seed=0):
    return np.random.default_rng(seed + 101).integers(0, 256, (V, H, W, 3), dtype=np.uint8)


def scene(uvz, faces, H, W, cams=None, images=None, seed=0, **kw):
    v, f, c = MRC.pix_mesh(uvz, faces, seed)
    cams = PIX[None] if cams is None else np.asarray(cams, np.float64).reshape(-1, 16)
    return dict({"verts": v, "faces": f, "rgb": c, "cams": cams, "images": noise(len(cams), H, W, seed) if images is None else images}, **kw)


# ---- builders ----------------------------------------------------------------------------------------------------------------------
def empty():
    return {"verts": np.zeros((0, 3), np.float32), "faces": np.zeros((0, 3), np.int32), "rgb": np.zeros((0, 3), np.uint8), "cams": PIX[None], "images": noise(1, 5, 7)}


def no_vertices():
    return dict(empty(), faces=np.array([(0, 1, 2), (0, 0, 0)], np.int32))


def one_face():
    return scene([(1, 1, 2), (5, 1, 2), (1, 5, 2)], [(0, 1, 2)], 8, 8)


def few_faces(n):
    """n right triangles of one class side by side"""
    uvz, faces = [], []
    for k in range(n):
        uvz += [(1 + 5 * k, 1, 2), (5 + 5 * k, 1, 2), (1 + 5 * k, 5, 2)]
        faces.append((3 * k, 3 * k + 1, 3 * k + 2))
    return scene(uvz, faces, 8, 5 * n + 3, rgb_none=(n == 2))


def specks(n):
    """n small triangles over 64 x 48, most below a pixel (seen only when they hold a pixel centre), every 8th of 1.5 pixels and every
    32nd of 7: three classes, seen and unseen faces, and face counts round the radix block and the scan tile"""
    rng = np.random.default_rng(n)
    size = np.where(np.arange(n) % 32 == 0, 7.0, np.where(np.arange(n) % 8 == 1, 1.5, 0.6))
    at = np.stack([rng.uniform(0.5, 62.0 - size), rng.uniform(0.5, 46.0 - size)], 1)
    uvz, z = [], 2.0
    for k in range(n):
        x, y, s = at[k, 0], at[k, 1], size[k]
        uvz += [(x, y, z), (x + s, y + 0.2 * s, z), (x + 0.3 * s, y + s, z)]
    return scene(uvz, np.arange(3 * n).reshape(n, 3), 48, 64, seed=n)


def invalid_indices():
    s = few_faces(3)
    nv = len(s["verts"])
    bad = [(-1, 1, 2), (0, nv, 2), (0, 1, INT_MAX), (INT_MIN, 1, 2), (1, 1, 2), (3, 2, 3), (4, 4, 4), (nv - 1, nv, nv + 1)]
    s["faces"] = np.concatenate([s["faces"][:1], np.asarray(bad, np.int32), s["faces"][1:]])
    return s


def hostile_coordinates():
    """the rasteriser's hostile vertices (NaN, +-inf, 1e30, behind the camera, 2^17 pixels away, invalid indices) under its three
    cameras, and faces of denormal and 1e30 coordinates; a few proper faces among them"""
    v, f, c, cams = MRC.case("hostile")
    tiny = 1.401298464324817e-45
    extra = np.asarray([(tiny, 0, 0), (0, 3 * tiny, 0), (0, 0, 5 * tiny), (1e30, 0, 1e30), (0, 1e30, 1e30), (1e30, 1e30, 1e30)], np.float32)
    n = len(v)
    faces = np.concatenate([f, [(n, n + 1, n + 2), (n + 3, n + 4, n + 5)]]).astype(np.int32)
    rgb = np.concatenate([c, np.full((6, 3), 77, np.uint8)])
    return {"verts": np.concatenate([v, extra]), "faces": faces, "rgb": rgb, "cams": cams, "images": noise(len(cams), 20, 24, 3)}


def image_1x1():
    """H = W = 1: only a face whose vertices all snap to the one sample is eligible, and it has no area; the face image names it"""
    s = scene([(0, 0, 2), (0.001, 0, 4), (0, 0.001, 1), (-3, -3, 2), (5, -3, 2), (-3, 5, 2)], [(0, 1, 2), (3, 4, 5)], 1, 1)
    s["face_images"] = np.zeros((1, 1, 1), np.int32)
    return s


def width_1():
    """W = 1: a face on the column u = 0 is eligible; handed a face image that names it, its texels sample an image one pixel wide"""
    s = scene([(0, 0, 2), (0, 2, 4), (0, 4, 1), (-3, -3, 2), (5, -3, 2), (-3, 9, 2)], [(0, 1, 2), (3, 4, 5)], 5, 1)
    s["face_images"] = np.array([0, 0, 1, -1, 0], np.int32).reshape(1, 5, 1)
    return s


def bad_face_image():
    s = few_faces(3)
    H, W = s["images"].shape[1:3]
    img = np.random.default_rng(8).integers(-2, 5, (1, H, W)).astype(np.int32)
    img[0, 0, :4] = (-1, 3, INT_MAX, INT_MIN)
    s["face_images"] = img
    return s


def rot_y(t):
    return np.array([[np.cos(t), 0.0, np.sin(t)], [0.0, 1.0, 0.0], [-np.sin(t), 0.0, np.cos(t)]])


def world_quad(half, z, first=0):
    v = [(-half, -half, z), (half, -half, z), (half, half, z), (-half, half, z)]
    return v, [(first, first + 1, first + 2), (first, first + 2, first + 3)]


def world_scene(verts, faces, cams, H, W, seed=0, rgb=None):
    verts = np.asarray(verts, np.float32)
    rgb = np.random.default_rng(seed + 11).integers(0, 256, (len(verts), 3), dtype=np.uint8) if rgb is None else np.asarray(rgb, np.uint8)
    cams = np.stack(cams)
    return {"verts": verts, "faces": np.asarray(faces, np.int32), "rgb": rgb, "cams": cams, "images": noise(len(cams), H, W, seed)}


def frontal_and_oblique():
    """a quad at z = 4; view 1 looks at it head on, view 0 from 60 degrees at the same distance: about half the samples"""
    v, f = world_quad(1.0, 4.0)
    R = rot_y(np.pi / 3)
    t = np.array([0.0, 0.0, 4.0]) - R @ np.array([0.0, 0.0, 4.0])
    return world_scene(v, f, [C.cam_row(R, t, 20.0, 20.0, 20.0, 20.0), C.cam_row(np.eye(3), (0, 0, 0), 20.0, 20.0, 20.0, 20.0)], 40, 40)


def equal_counts():
    v, f = world_quad(1.0, 4.0)
    cam = C.cam_row(np.eye(3), (0, 0, 0), 20.0, 20.0, 20.0, 20.0)
    return world_scene(v, f, [cam, cam, cam], 40, 40)


def outside_by(steps):
    """view 0 sees most of the face, but its corner a lies `steps` lattice steps left of the sample rectangle; view 1 sees it at half
    the size, inside"""
    s = scene([(0, 0, 2), (40, 0, 2), (0, 30, 2)], [(0, 1, 2)], 48, 64, cams=[MRC.pix_cam(-steps / 256.0, 0.0), C.cam_row(np.eye(3), (0, 0, 0), 0.5, 0.5, 1.0, 1.0)])
    return s


def hidden_then_open():
    """faces 0, 1: a quad at z = 2; faces 2, 3: a larger quad at z = 4 that view 0 sees only behind the first; view 1 looks from the
    other side, where the larger quad is in front"""
    v0, f0 = world_quad(2.0, 2.0)
    v1, f1 = world_quad(3.0, 4.0, 4)
    back = C.cam_row(np.diag([-1.0, 1.0, -1.0]), (0.0, 0.0, 6.0), 8.0, 8.0, 32.0, 24.0)
    return world_scene(v0 + v1, f0 + f1, [C.cam_row(np.eye(3), (0, 0, 0), 8.0, 8.0, 32.0, 24.0), back], 48, 64)


def hidden_everywhere():
    """faces 2, 3 lie between two quads that hide them from both views: unseen, their texels are their vertex colours"""
    v0, f0 = world_quad(3.0, 2.0)
    v1, f1 = world_quad(1.0, 3.0, 4)
    v2, f2 = world_quad(3.0, 4.0, 8)
    s = hidden_then_open()
    rgb = np.random.default_rng(4).integers(0, 256, (12, 3), dtype=np.uint8)
    rgb[4:8] = (10, 200, 30)
    return world_scene(v0 + v1 + v2, f0 + f1 + f2, list(s["cams"]), 48, 64, rgb=rgb)


def three_views():
    v, f, c, cams = MRC.case("three_views")
    return {"verts": v, "faces": f, "rgb": c, "cams": cams, "images": noise(3, 48, 64, 7), "cull": "back"}


THRESHOLD_EDGES = (1, 1 + 1 / 256, 5, 5 + 1 / 256, 10, 10 + 1 / 256, 13, 13 + 1 / 256, 29, 29 + 1 / 256)
# a class's legs are 2^k - 3 texels: 1, 5, 13, 29, 61 pixels at shift 0, twice that at shift 1, 256 pixels and more at shift 8
THRESHOLD_CLASSES = {0: (2, 3, 3, 4, 4, 4, 4, 5, 5, 6), 1: (2, 2, 3, 3, 3, 4, 4, 4, 5, 5), 8: (2,) * 10}


def thresholds(shift=0, max_size=MT.DEFAULT_MAX_SIZE):
    """faces whose longest edge, horizontal from a pixel centre, is exactly the legs of a class long, and one lattice step longer"""
    uvz, faces = [], []
    for k, e in enumerate(THRESHOLD_EDGES):
        y = 1 + 3 * k
        uvz += [(1, y, 2), (1 + e, y, 2), (1 + e / 2, y + min(e / 2, 2.0), 2)]
        faces.append((3 * k, 3 * k + 1, 3 * k + 2))
    return scene(uvz, faces, 48, 64, shift=shift, max_size=max_size)


def capped():
    """an edge of 1022 pixels: longer than the legs of the largest class"""
    return scene([(0, 0, 2), (1022, 0, 2), (0, 1, 2)], [(0, 1, 2)], 2, 1024)


PLANE_AT, PLANE_STEP, PLANE_N = (4, 3), (6, 5), 4


def ramp_plane():
    """4 x 4 quads of 6 x 5 pixels on the plane z = 2, corners on pixel centres, well inside a 64 x 48 image that holds the ramps"""
    n = PLANE_N + 1
    uvz = [(PLANE_AT[0] + PLANE_STEP[0] * i, PLANE_AT[1] + PLANE_STEP[1] * j, 2) for j in range(n) for i in range(n)]
    idx = np.arange(n * n).reshape(n, n)
    a, b, c_, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    faces = np.stack([np.stack([a, b, c_], 1), np.stack([b, d, c_], 1)], 1).reshape(-1, 3)
    return scene(uvz, faces, 48, 64, images=ramp(48, 64)[None])


CASES = {
    "nv_0_nf_0": empty,
    "nv_0_with_faces": no_vertices,
    "one_face": one_face,
    "two_faces_one_cell": lambda: few_faces(2),
    "three_faces_missing_partner": lambda: few_faces(3),
    "specks_255": lambda: specks(255),
    "specks_256": lambda: specks(256),
    "specks_257": lambda: specks(257),
    "specks_2047": lambda: specks(2047),
    "specks_2048": lambda: specks(2048),
    "specks_2049": lambda: specks(2049),
    "specks_4097": lambda: specks(4097),
    "invalid_indices": invalid_indices,
    "hostile_coordinates": hostile_coordinates,
    "image_1x1": image_1x1,
    "width_1": width_1,
    "bad_face_image": bad_face_image,
    "frontal_and_oblique": frontal_and_oblique,
    "equal_counts": equal_counts,
    "outside_by_0": lambda: outside_by(0),
    "outside_by_1": lambda: outside_by(1),
    "hidden_then_open": hidden_then_open,
    "hidden_everywhere": hidden_everywhere,
    "three_views": three_views,
    "thresholds_shift_0": lambda: thresholds(0),
    "thresholds_shift_1": lambda: thresholds(1),
    "thresholds_shift_8": lambda: thresholds(8),
    "capped": capped,
    "ramp_plane": ramp_plane,
}
EXPECTED_VIEWS = {"frontal_and_oblique": [1, 1], "equal_counts": [0, 0], "outside_by_0": [0], "outside_by_1": [1], "hidden_then_open": [0, 0, 1, 1],
                  "hidden_everywhere": [0, 0, -1, -1, 1, 1]}


@functools.lru_cache(maxsize=None)
def case(name):
    s = CASES[name]()
    if s.pop("rgb_none", False):
        s["rgb"] = None
    for a in s.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return s


def options(s):
    return {k: s[k] for k in ("shift", "max_size", "cull") if k in s}


@functools.lru_cache(maxsize=None)
def reference(name):
    s = case(name)
    r = O.texture(s["verts"], s["faces"], s["rgb"], s["images"], s["cams"], NEAR, face_images=s.get("face_images"), **options(s))
    r["tex_rgb"] = O.shade(s["verts"], s["faces"], s["cams"], r["face_images"], r["texel"], r["atlas"], NEAR)
    return r


def run(dev, s, **kw):
    tv, tf, tc = to_dev(dev, s["verts"], s["faces"], s["rgb"])
    fi = None if s.get("face_images") is None else torch.from_numpy(np.array(s["face_images"])).to(dev)
    tex = MT.texture(tv, tf, tc, torch.from_numpy(np.array(s["images"])).to(dev), s["cams"], near=NEAR, face_images=fi, **dict(options(s), **kw))
    return (tv, tf, tc), tex


def assert_equal(tex, want, what):
    """a texture() result against the oracle's, every output in every bit"""
    assert tex["best"].dtype == torch.int64 and tex["atlas"].dtype == torch.uint8 and tex["owner"].dtype == torch.int32 and tex["texel"].dtype == torch.int32
    assert np.array_equal(host(tex["best"]).view(np.uint64), want["best"]), what
    assert np.array_equal(host(tex["klass"]), want["klass"]), what
    assert np.array_equal(host(tex["order"]), want["order"]), what
    assert tex["table"] == want["table"], (what, tex["table"], want["table"])
    assert tex["shift"] == want["shift"] and tex["size"] == (want["table"]["Sy"], want["table"]["S"]), what
    assert np.array_equal(host(tex["texel"]), want["texel"]), what
    assert np.array_equal(host(tex["owner"]), want["owner"]), what
    if not np.array_equal(host(tex["atlas"]), want["atlas"]):
        at = np.argwhere(host(tex["atlas"]) != want["atlas"])[:5]
        print(what, "atlas differs at", at.tolist(), [int(host(tex["atlas"])[tuple(i)]) for i in at], [int(want["atlas"][tuple(i)]) for i in at])
    assert np.array_equal(host(tex["atlas"]), want["atlas"]), what
    assert tex["stats"] == want["stats"], (what, tex["stats"], want["stats"])
    assert tex["uv"].dtype == np.float32 and np.array_equal(tex["uv"].view(np.uint32), want["uv"].view(np.uint32)), what


def check_invariants(s, r, what):
    """the known answers of every case, on a result (the kernels' or the oracle's): cells inside the atlas and aligned to their side, no
    two faces in one half cell, each valid face the owner of exactly s (s - 1) / 2 or s (s + 1) / 2 texels and of no other, the
    half-height atlas exactly when the total allows it, the counters adding up"""
    klass, texel, owner, table = np.asarray(r["klass"]), np.asarray(r["texel"]), np.asarray(r["owner"]), r["table"]
    S, Sy, total = table["S"], table["Sy"], table["total"]
    assert owner.shape == (Sy, S) and S & (S - 1) == 0 and S * S >= total and (S == 1 or (S // 2) ** 2 < total)
    assert (Sy == S // 2) == (S >= 2 and 2 * total <= S * S) and Sy in (S, S // 2)
    counts = np.bincount(owner[owner >= 0].ravel(), minlength=len(klass)) if len(klass) else np.zeros(0, np.int64)
    taken = set()
    for f, k in enumerate(klass.tolist()):
        if k == 0:
            assert counts[f] == 0 and not texel[f].any(), (what, f)
            continue
        s_, L = 1 << k, (1 << k) - 3
        (ax, ay), (bx, by), (cx, cy) = texel[f].tolist()
        half = 0 if bx > ax else 1
        ox, oy = (ax, ay) if half == 0 else (ax - s_ + 1, ay - s_ + 1)
        assert MT.MIN_CLASS <= k <= MT.MAX_CLASS and abs(bx - ax) == L and by == ay and cx == ax and abs(cy - ay) == L, (what, f)
        assert ox % s_ == 0 and oy % s_ == 0 and 0 <= ox <= S - s_ and 0 <= oy <= Sy - s_, (what, f, ox, oy, s_)
        assert (ox, oy, half) not in taken, (what, f)
        taken.add((ox, oy, half))
        assert counts[f] == (s_ * (s_ - 1) // 2 if half == 0 else s_ * (s_ + 1) // 2), (what, f, counts[f])
        assert (owner[oy:oy + s_, ox:ox + s_] == f).sum() == counts[f], (what, f)
    st = r["stats"]
    assert st["faces_seen"] + st["faces_unseen"] + st["faces_invalid"] == len(klass) and st["faces_invalid"] == int((klass == 0).sum())
    assert sum(st["faces_per_class"].values()) == st["faces_seen"] + st["faces_unseen"]
    assert st["texels_image"] + st["texels_vertex"] + st["texels_fallback"] == int((owner >= 0).sum())


def check_case(dev, name, twice=False):
    s, want = case(name), reference(name)
    check_invariants(s, want, name + " (oracle)")
    mesh, tex = run(dev, s)
    assert_equal(tex, want, name)
    check_invariants(s, dict(tex, klass=host(tex["klass"]), texel=host(tex["texel"]), owner=host(tex["owner"])), name)
    fi = torch.from_numpy(np.array(want["face_images"])).to(dev)
    shaded = MT.shade(mesh[0], mesh[1], s["cams"], fi, tex["texel"], tex["atlas"], near=NEAR)
    assert shaded.dtype == torch.uint8 and np.array_equal(host(shaded), want["tex_rgb"]), name
    if "face_images" not in s:
        out = MR.render(*mesh, s["cams"], *s["images"].shape[1:3], near=NEAR, cull=s.get("cull", "none"), texture=(tex["atlas"], tex["texel"]))
        assert np.array_equal(host(out["face"]), want["face_images"]) and np.array_equal(host(out["tex_rgb"]), want["tex_rgb"]), name
    if name in EXPECTED_VIEWS:
        assert want["views"] == EXPECTED_VIEWS[name], (name, want["views"])
    if name.startswith("thresholds_shift_"):
        assert tuple(want["klass"].tolist()) == THRESHOLD_CLASSES[s["shift"]] and want["stats"]["faces_seen"] == 10 and want["stats"]["faces_capped"] == 0
    if name == "capped":
        assert want["klass"].tolist() == [10] and want["stats"]["faces_capped"] == 1 and want["stats"]["faces_seen"] == 1 and want["table"]["S"] == 1024
    if name == "hidden_everywhere":
        own = want["owner"]
        assert (want["atlas"][(own == 2) | (own == 3)] == (10, 200, 30)).all() and want["stats"]["texels_vertex"] == int(((own == 2) | (own == 3)).sum())
    if name.startswith("specks_"):
        assert want["stats"]["faces_seen"] > 0 and want["stats"]["faces_unseen"] > 0 and sum(1 for n in want["stats"]["faces_per_class"].values() if n) >= 3
        assert want["table"]["S"] <= 256
    if name in ("image_1x1", "width_1"):
        assert want["views"][0] == 0 and want["stats"]["texels_image"] > 0
    if name == "hostile_coordinates":
        # (0, nv, 2) of the rasteriser's case is valid here, where six vertices follow; some texels of seen faces do not project and fall back
        assert want["stats"]["faces_invalid"] == 4 and want["stats"]["faces_seen"] > 0 and want["stats"]["faces_unseen"] > 10 and want["stats"]["texels_fallback"] > 0
    if twice:
        again = run(dev, s)[1]
        for k in ("best", "klass", "order", "texel", "owner", "atlas"):
            assert torch.equal(tex[k], again[k]), (name, k)
        assert again["stats"] == tex["stats"] and again["table"] == tex["table"]


def case_keys():
    return list(CASES)


# ---- view choice: chunks ------------------------------------------------------------------------------------------------------------
def check_chunks(dev):
    """three views in one call against chunks of two and of one, and against three calls of vote with one view each: the same bits"""
    s = case("three_views")
    mesh, whole = run(dev, s, chunk=3)
    assert len(set(v for v in reference("three_views")["views"] if v >= 0)) == 3
    for chunk in (1, 2):
        part = run(dev, s, chunk=chunk)[1]
        for k in ("best", "klass", "order", "texel", "owner", "atlas"):
            assert torch.equal(whole[k], part[k]), (chunk, k)
    H, W = s["images"].shape[1:3]
    best = None
    for v in range(3):
        face = MR.render(*mesh, s["cams"][v:v + 1], H, W, near=NEAR, cull="back")["face"]
        best = MT.vote(mesh[0], mesh[1], face, s["cams"][v:v + 1], NEAR, first_view=v, best=best)
    assert torch.equal(best, whole["best"])


# ---- max_size -----------------------------------------------------------------------------------------------------------------------
def check_max_size(dev):
    """an atlas that just fits max_size keeps its shift; one texel less and the shift rises until it fits; a mesh that does not fit at
    shift 8 is refused with the size it needs"""
    s = case("thresholds_shift_0")
    S0 = reference("thresholds_shift_0")["table"]["S"]
    assert S0 >= 8
    for max_size, raised in ((S0, False), (S0 - 1, True), (S0 // 2, True)):
        want = O.texture(s["verts"], s["faces"], s["rgb"], s["images"], s["cams"], NEAR, max_size=max_size)
        tex = run(dev, s, max_size=max_size)[1]
        assert_equal(tex, want, f"max_size {max_size}")
        assert (tex["shift"] > 0) == raised and tex["table"]["S"] <= max_size
    three = case("three_faces_missing_partner")
    try:
        run(dev, three, max_size=2)
    except _lib.RcmvsError as e:
        # three faces of the smallest class: two cells of 4 x 4, 32 texels; 4^3 >= 32 gives S = 8, and 2 x 32 <= 64 half the height
        assert "8 x 4" in str(e) and "shift 8" in str(e) and "max_size = 2" in str(e), str(e)
    else:
        raise AssertionError("an atlas beyond max_size at shift 8 was accepted")
    try:
        O.texture(three["verts"], three["faces"], three["rgb"], three["images"], three["cams"], NEAR, max_size=2)
    except O.Refused as e:
        assert e.args[0] == (8, 4)
    else:
        raise AssertionError("the oracle accepted an atlas beyond max_size at shift 8")


# ---- fill: known answers ------------------------------------------------------------------------------------------------------------
def check_ramp(dev):
    """The ramp plane: the map from a face's texels to the image is affine (a fronto-parallel plane under a pinhole camera), and
    bilinear interpolation of a linear ramp is that ramp.  So texel (i', j') of a face must hold the ramp at its own image position
    p = wa A + wb B + wc C (the corners' pixel positions, the weights exact rationals of denominator L), clamped to the image,
    rounded: floor(r + 1/2) with r = ramp(p) a rational of denominator at most 2 L <= 26.

    Bound: the kernel's value differs from r by fp64 rounding only, below 1e-10 (a dozen operations on numbers below 2^8, each within
    2^-53 relative).  r + 1/2 is an integer or at least 1 / (2 L) > 0.03 from one, so the byte is exactly floor(r + 1/2), zero levels
    off, except at an exact tie (r + 1/2 an integer), where rounding may fall either way: at most one level, downwards.  A gutter
    texel (i' + j' = L + 1, wa = -1 / L) holds the ramp extrapolated one texel beyond the hypotenuse."""
    s = case("ramp_plane")
    tex = run(dev, s)[1]
    assert_equal(tex, reference("ramp_plane"), "ramp_plane")
    atlas, owner, texel, klass = host(tex["atlas"]), host(tex["owner"]), host(tex["texel"]), host(tex["klass"])
    H, W = s["images"].shape[1:3]
    pix = [(Fraction(float(p[0] / p[2])), Fraction(float(p[1] / p[2]))) for p in s["verts"].astype(np.float64)]
    checked = ties = gutters = worst = 0
    for f, (a, b, c) in enumerate(s["faces"].tolist()):
        k = int(klass[f])
        assert k == 4                                              # the longest edge is sqrt(61) pixels: beyond 5, within 13
        L = (1 << k) - 3
        (ax, ay), (bx, _), _ = texel[f].tolist()
        sign = 1 if bx > ax else -1
        ys, xs = np.nonzero(owner == f)
        for y, x in zip(ys.tolist(), xs.tolist()):
            ip, jp = sign * (x - ax), sign * (y - ay)
            assert 0 <= ip and 0 <= jp and ip + jp <= L + 1 + (sign < 0)
            wb, wc = Fraction(ip, L), Fraction(jp, L)
            wa = 1 - wb - wc
            u = min(max(wa * pix[a][0] + wb * pix[b][0] + wc * pix[c][0], 0), W - 1)
            v = min(max(wa * pix[a][1] + wb * pix[b][1] + wc * pix[c][1], 0), H - 1)
            for ch in range(3):
                r = RAMP[ch](u, v) + Fraction(1, 2)
                want = r.numerator // r.denominator
                got = int(atlas[y, x, ch])
                tie = r.denominator == 1
                assert got == want or (tie and got == want - 1), (f, x, y, ch, got, want, tie)
                ties += tie
                worst = max(worst, abs(got - want))
            checked += 1
            gutters += wa < 0
    print(f"ramp plane: {checked} texels, {gutters} in a gutter, {ties} exact ties, largest difference {worst} level(s)")
    assert checked == int((owner >= 0).sum()) and gutters >= 32 * 14 and tex["stats"]["texels_image"] == checked


def check_plane_round_trip(dev):
    """The ramp plane rendered with its texture into the view it was textured from, against that view's image, on covered pixels.

    Bound: a covered pixel's texel position is the affine image of the pixel (one plane, one camera), so the four texels round it
    hold the ramp at four positions whose bilinear mean is the pixel's own ramp value; a tap beyond the face's texels has weight
    exactly zero (positions stay within 0 <= x, 0 <= y, x + y <= L, and the gutter diagonal covers x + y = L + 1).  Each texel is
    within 1/2 level of its ramp value (the first rounding), so their mean is within 1/2 of the image's integer, and the second
    rounding adds at most 1/2: the difference of the two integers is at most 1 level."""
    s = case("ramp_plane")
    mesh, tex = run(dev, s)
    H, W = s["images"].shape[1:3]
    out = MR.render(*mesh, s["cams"], H, W, near=NEAR, texture=(tex["atlas"], tex["texel"]))
    face, got = host(out["face"])[0], host(out["tex_rgb"])[0].astype(np.int64)
    covered = face >= 0
    assert covered.sum() == PLANE_N * PLANE_STEP[0] * PLANE_N * PLANE_STEP[1]
    diff = np.abs(got - s["images"][0].astype(np.int64))[covered]
    print(f"plane round trip: {int(covered.sum())} pixels, largest difference {int(diff.max())}, mean {float(diff.mean()):.4f} levels")
    assert diff.max() <= 1
    assert (got[~covered] == 0).all()


# ---- the sphere ---------------------------------------------------------------------------------------------------------------------
SPHERE_VIEWS, SPHERE_H, SPHERE_W, SPHERE_F, SPHERE_DIST, SPHERE_VOXEL, SPHERE_GRID, SPHERE_PERIOD = 4, 48, 64, 60.0, 3.2, 0.08, 30, 0.25


def pattern(d):
    """a colour per direction (unit vectors, (..., 3)): three sines of period SPHERE_PERIOD along the axes"""
    return np.clip(np.floor(127.5 + 127.5 * np.sin(2.0 * np.pi / SPHERE_PERIOD * d) + 0.5), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def sphere_scene():
    """a unit sphere at the origin seen from four sides: exact depth maps, and images that carry `pattern` of the surface direction"""
    cams, depths, images = [], [], []
    for k in range(SPHERE_VIEWS):
        az, el = 2.0 * np.pi * k / SPHERE_VIEWS + 0.3, 0.35
        centre = SPHERE_DIST * np.array([np.cos(el) * np.sin(az), -np.sin(el), -np.cos(el) * np.cos(az)])
        fwd = -centre / np.linalg.norm(centre)
        right = np.cross(fwd, [0.0, -1.0, 0.0])
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        R = np.stack([right, down, fwd])
        cams.append(C.cam_row(R, -R @ centre, SPHERE_F, SPHERE_F, (SPHERE_W - 1) / 2.0, (SPHERE_H - 1) / 2.0))
        jj, ii = np.mgrid[0:SPHERE_H, 0:SPHERE_W]
        ray = np.stack([(ii - cams[-1][14]) / SPHERE_F, (jj - cams[-1][15]) / SPHERE_F, np.ones((SPHERE_H, SPHERE_W))], -1)
        oc = -(R @ centre)                                         # the sphere's centre in the camera frame
        A, B, Cq = (ray * ray).sum(-1), -2.0 * (ray * oc).sum(-1), (oc * oc).sum() - 1.0
        disc = B * B - 4 * A * Cq
        z = np.where(disc > 0, (-B - np.sqrt(np.maximum(disc, 0))) / (2 * A), 0.0)
        world = (ray * z[..., None] - oc) @ R                      # R^T (p - oc): on the unit sphere where z > 0
        depths.append(z.astype(np.float32))
        images.append(np.where(z[..., None] > 0, pattern(world), 0).astype(np.uint8))
    return np.stack(cams), np.stack(depths), np.stack(images)


def check_sphere(dev):
    """An extracted, decimated sphere whose images carry a pattern finer than the vertex spacing (period 0.25 against cells of 0.32):
    over the covered pixels of the view each face was textured from, the textured render must be nearer the source image than the
    vertex-colour render (mean absolute difference).  The same pair over the other views' pixels is printed, not asserted."""
    cams, depths, images = sphere_scene()
    h, n = SPHERE_VOXEL, SPHERE_GRID
    vol = TM.TsdfVolume([-0.5 * n * h] * 3, h, [n, n, n], dev)
    vol.integrate(torch.from_numpy(depths).to(dev), cams, torch.from_numpy(images).to(dev), trunc=3.0 * h)
    verts, faces, rgb = vol.extract(1)
    verts, faces, rgb = MD.decimate(verts, faces, rgb, cell=4.0 * h)[:3]
    nf = int(faces.shape[0])
    assert 100 < nf < 4000
    tex = MT.texture(verts, faces, rgb, torch.from_numpy(images).to(dev), cams, near=NEAR, cull="back")
    assert tex["stats"]["faces_seen"] > 0.8 * nf and tex["table"]["S"] <= 512
    out = MR.render(verts, faces, rgb, cams, SPHERE_H, SPHERE_W, near=NEAR, cull="back", texture=(tex["atlas"], tex["texel"]))
    face, textured, coloured = host(out["face"]), host(out["tex_rgb"]).astype(np.float64), host(out["rgb"]).astype(np.float64)
    best = host(tex["best"]).view(np.uint64)
    view_of = np.where(best != 0, 0xFFFFFFFF - (best & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    covered = (face >= 0) & (depths > 0)
    chosen_here = np.zeros_like(covered)
    for v in range(SPHERE_VIEWS):
        chosen_here[v] = covered[v] & (view_of[np.where(covered[v], face[v], 0)] == v)
    src = images.astype(np.float64)
    figures = {}
    for what, sel in (("own", chosen_here), ("other", covered & ~chosen_here)):
        figures[what] = (int(sel.sum()), float(np.abs(textured - src)[sel].mean()), float(np.abs(coloured - src)[sel].mean()))
        print(f"sphere, {nf} faces, atlas {tex['size']}: pixels of the view a face was {'textured from' if what == 'own' else 'not textured from'}: "
              f"{figures[what][0]}, mean |textured - image| = {figures[what][1]:.2f}, mean |vertex colours - image| = {figures[what][2]:.2f} levels")
    assert figures["own"][0] > 1000 and figures["own"][1] < figures["own"][2]


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def check_refusals(dev):
    s = case("three_faces_missing_partner")
    tv, tf, tc = to_dev(dev, s["verts"], s["faces"], s["rgb"])
    img = torch.from_numpy(np.array(s["images"])).to(dev)
    good = dict(verts=tv, faces=tf, rgb=tc, images=img, cams=s["cams"], near=NEAR)
    bad = [({"max_size": 0}, "max_size = 0"), ({"max_size": 16385}, "max_size = 16385"), ({"shift": 9}, "shift = 9"), ({"shift": -1}, "shift = -1"),
           ({"chunk": 0}, "chunk = 0"), ({"near": 0.0}, "near = 0"), ({"near": float("nan")}, "near"), ({"images": img[0]}, "images must be"),
           ({"images": img.to(torch.int32)}, "images must be"), ({"cams": s["cams"][:0]}, "no views"), ({"cams": np.concatenate([s["cams"]] * 2)}, "2 cameras"),
           ({"rgb": tc[:-1]}, "rgb must be"), ({"faces": tf.to(torch.int64)}, "faces must be"), ({"background": (0, 0, 256)}, "background"),
           ({"cull": "front"}, "cull = 'front'"), ({"face_images": torch.zeros((1, 2, 2), dtype=torch.int32, device=dev)}, "face_images must be")]
    for kw, pattern_ in bad:
        a = dict(good, **kw)
        try:
            MT.texture(a.pop("verts"), a.pop("faces"), a.pop("rgb"), a.pop("images"), a.pop("cams"), **a)
        except _lib.RcmvsError as e:
            assert pattern_ in str(e), (kw, str(e))
        else:
            raise AssertionError(f"accepted {list(kw)}")
    tex = MT.texture(tv, tf, tc, img, s["cams"], near=NEAR)
    face = torch.zeros((1,) + tuple(img.shape[1:3]), dtype=torch.int32, device=dev)
    for call, pattern_ in ((lambda: MT.shade(tv, tf, s["cams"], face, tex["texel"][:-1], tex["atlas"]), "texel must be"),
                           (lambda: MT.shade(tv, tf, s["cams"], face, tex["texel"], tex["atlas"][..., 0]), "atlas must be"),
                           (lambda: MT.shade(tv, tf, s["cams"], face.to(torch.int64), tex["texel"], tex["atlas"]), "face_image must be"),
                           (lambda: MT.vote(tv, tf, face, s["cams"], NEAR, best=torch.zeros(1, dtype=torch.int64, device=dev)), "best must be"),
                           (lambda: MT.vote(tv, tf, face, s["cams"], NEAR, first_view=-1), "first_view")):
        try:
            call()
        except _lib.RcmvsError as e:
            assert pattern_ in str(e), str(e)
        else:
            raise AssertionError("a bad argument was accepted")


# ---- wiring -------------------------------------------------------------------------------------------------------------------------
def check_mesh_scan(dev, tmp_path):
    """mesh_scan without the option: PLY bytes and summary keys as the TSDF suite's oracle fixes them (what the parent commit gives), no
    PNG written; with texture=True: the same keys plus "texture", the same mesh with texcoords equal to the oracle's in every bit and
    the atlas PNG equal to the oracle's atlas, read back by read_ply_mesh_texture and by the older readers as it was; with render_dir
    the textured views; then the command lines."""
    from PIL import Image
    pair_folder, out_folder = C.write_scan(tmp_path)
    plain_ply, ply, rdir = (str(tmp_path / "out" / n) for n in ("plain.ply", "textured.ply", "render"))
    kw = dict(resolution=32, device=dev)
    plain = TM.mesh_scan(pair_folder, out_folder, out_folder, plain_ply, C.PROB, C.NCONS, C.DIST, C.DEPTH, **kw)
    assert list(plain) == ["mesh", "origin", "dims", "voxel", "trunc", "min_weight", "views", "vertices", "faces", "unreferenced_vertices", "observed_voxels"]
    views = TM.filtered_views(pair_folder, out_folder, out_folder, C.PROB, C.NCONS, C.DIST, C.DEPTH, device=dev)
    want, _ = C.oracle_mesh_of(views, plain)
    with open(plain_ply, "rb") as fh:
        plain_bytes = fh.read()
    assert plain_bytes == TM.mesh_ply_bytes(want["verts"], want["faces"], want["rgb"]) and b"texcoord" not in plain_bytes and b"TextureFile" not in plain_bytes
    assert not os.path.exists(str(tmp_path / "out" / "plain.png"))
    summary = TM.mesh_scan(pair_folder, out_folder, out_folder, ply, C.PROB, C.NCONS, C.DIST, C.DEPTH, texture=True, texture_size=4096, render_dir=rdir, **kw)
    assert list(summary) == list(plain) + ["texture", "render"]
    assert {k: v for k, v in summary.items() if k not in ("mesh", "texture", "render")} == {k: v for k, v in plain.items() if k != "mesh"}
    images = host(views["rgb"])
    ref = O.texture(want["verts"], want["faces"], want["rgb"], images, views["cams"], MT.DEFAULT_NEAR, max_size=4096)
    assert {k: summary["texture"][k] for k in O.STAT_NAMES} == {k: ref["stats"][k] for k in O.STAT_NAMES} and ref["stats"]["faces_seen"] > 0
    assert summary["texture"]["atlas"] == [ref["table"]["Sy"], ref["table"]["S"]] and summary["texture"]["shift"] == ref["shift"]
    assert summary["render"]["textured_views"] == len(images) and json.dumps(summary)
    v, f, c, n, uv, name = dtu_io.read_ply_mesh_texture(ply)
    assert name == "textured.ply"[:-4] + ".png" and n is None
    assert np.array_equal(v.view(np.uint32), want["verts"].view(np.uint32)) and np.array_equal(f, want["faces"]) and np.array_equal(c, want["rgb"])
    assert uv.dtype == np.float32 and np.array_equal(uv.view(np.uint32), ref["uv"].view(np.uint32))
    with open(ply, "rb") as fh:
        assert fh.read() == TM.mesh_ply_bytes(want["verts"], want["faces"], want["rgb"], texcoords=ref["uv"], texture_file=name)
    v2, f2, c2 = dtu_io.read_ply_mesh_rgb(ply)
    v3, f3 = dtu_io.read_ply_mesh(ply)
    assert np.array_equal(v2.view(np.uint32), v.view(np.uint32)) and np.array_equal(f2, f) and np.array_equal(c2, c) and np.array_equal(v3, v) and np.array_equal(f3, f)
    with Image.open(os.path.join(os.path.dirname(ply), name)) as im:
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), ref["atlas"])
    V, H, W = views["depth"].shape
    assert len(os.listdir(os.path.join(rdir, "render"))) == 3 * V
    tv, tf, tc, atlas, texel = MT.read_textured(ply, dev)
    assert np.array_equal(host(texel), ref["texel"]) and np.array_equal(host(atlas), ref["atlas"])
    out = MR.render(tv, tf, tc, views["cams"], H, W, texture=(atlas, texel))
    with Image.open(os.path.join(rdir, "render", "00000002_tex.png")) as im:
        assert im.size == (W, H) and im.mode == "RGB" and np.array_equal(np.asarray(im), host(out["tex_rgb"][2]))
    assert (host(out["face"]) >= 0).sum() > 0
    # with normals too: both in one PLY, every reader
    both = str(tmp_path / "out" / "both.ply")
    b = TM.mesh_scan(pair_folder, out_folder, out_folder, both, C.PROB, C.NCONS, C.DIST, C.DEPTH, texture=True, normals="area", **kw)
    assert list(b) == list(plain) + ["normals", "texture"]
    vb, fb, cb, nb, uvb, nameb = dtu_io.read_ply_mesh_texture(both)
    assert nb is not None and nb.shape == vb.shape and nameb == "both.png" and np.array_equal(fb, f)
    assert uvb.shape == (len(f), 3, 2) and float(uvb.min()) > 0.0 and float(uvb.max()) < 1.0
    # mesh_render's command line on the textured PLY
    dst = str(tmp_path / "cli_render")
    MR.main(["--mesh", ply, "--pair-folder", pair_folder, "--scan-folder", out_folder, "--out", dst, "--size", str(H), str(W), "--texture", "--device", dev])
    with Image.open(os.path.join(dst, "render", "00000002_tex.png")) as im:
        assert np.array_equal(np.asarray(im), host(out["tex_rgb"][2]))
    # mesh_texture's command line on the plain PLY, with an OBJ
    cli = str(tmp_path / "cli" / "scan.ply")
    total = MT.main(["--mesh", plain_ply, "--pair-folder", pair_folder, "--scan-folder", out_folder, "--out", cli, "--size", str(H), str(W), "--texture-obj",
                     "--render", str(tmp_path / "cli" / "views"), "--device", dev])
    assert json.dumps(total) and total["faces"] == len(f) and total["faces_seen"] > 0 and sorted(os.listdir(tmp_path / "cli")) == \
        ["scan.mtl", "scan.obj", "scan.ply", "scan.png", "views"]
    vc, fc, _, _, uvc, namec = dtu_io.read_ply_mesh_texture(cli)
    assert namec == "scan.png" and np.array_equal(fc, f) and uvc.shape == (len(f), 3, 2)
    check_obj(str(tmp_path / "cli" / "scan.obj"), len(v), len(f), uvc)
    assert len(os.listdir(tmp_path / "cli" / "views" / "render")) == 3 * V
    return ply, plain_ply


def check_obj(path, nv, nf, uv):
    """the OBJ's v, vt and f records: 3 nf texture coordinates equal to uv as printed, every index in range, the .mtl names the PNG"""
    rows = [line.split() for line in open(path).read().splitlines()]
    vs, vts, fs = ([r for r in rows if r[0] == k] for k in ("v", "vt", "f"))
    assert len(vs) == nv and len(vts) == 3 * nf and len(fs) == nf
    got = np.array([[float(x) for x in r[1:]] for r in vts], np.float32).reshape(nf, 3, 2)
    assert np.array_equal(got, uv)
    for i, r in enumerate(fs):
        pairs = [tuple(int(x) for x in p.split("/")) for p in r[1:]]
        assert len(pairs) == 3 and all(1 <= a <= nv for a, _ in pairs) and [t for _, t in pairs] == [3 * i + 1, 3 * i + 2, 3 * i + 3]
    stem = os.path.splitext(path)[0]
    assert rows[0] == ["mtllib", os.path.basename(stem) + ".mtl"] and f"map_Kd {os.path.basename(stem)}.png" in open(stem + ".mtl").read()
