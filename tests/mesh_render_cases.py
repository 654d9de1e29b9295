"""The cases and checks of the mesh rasteriser (csrc/mesh_render.hip through rc_mvsnet_amd/mesh_render.py), shared by
tests/test_gpu_mesh_render.py (device "cuda:0") and tests/test_mesh_render_emu_cpu.py (the CPU emulation, device "cpu"), against
tests/mesh_render_oracle.py.  Every comparison with the oracle is bit equality: keys, depths (as their 32-bit patterns), face
numbers, colour bytes, shade bytes and counters; the comparison table's counts are equal and its sum is within 1e-12 relative.
The tolerances of the known answers are derived next to their asserts.

Most meshes are built in the image: with the camera PIX (R = I, t = 0, fx = fy = 1, cx = cy = 0) a vertex (u z, v z, z) with z a
power of two lands on pixel position (u, v) exactly."""
import functools
import json
import os

import numpy as np
import torch

import mesh_clean_cases as MCC
import mesh_render_oracle as O
import tsdf_cases as C
import tsdf_sparse_cases as SC
from mesh_clean_cases import INT_MAX, INT_MIN, host, to_dev
from rc_mvsnet_amd import _lib, data_io, dtu_io, mesh_clean as MC, mesh_decimate as MD, mesh_holes as MH, mesh_render as MR, tsdf_mesh as TM

SIZES = ((1, 1), (2, 2), (7, 5), (64, 48))                           # (W, H)
PIX = C.cam_row(np.eye(3), (0.0, 0.0, 0.0), 1.0, 1.0, 0.0, 0.0)
NEAR = 0.5


def pix_cam(cx=0.0, cy=0.0):
    return C.cam_row(np.eye(3), (0.0, 0.0, 0.0), 1.0, 1.0, cx, cy)


def pix_mesh(uvz, faces, seed=0):
    """uvz: rows (u, v, z) -> verts (u z, v z, z) fp32, faces int32, random colours"""
    uvz = np.asarray(uvz, np.float64).reshape(-1, 3)
    verts = np.stack([uvz[:, 0] * uvz[:, 2], uvz[:, 1] * uvz[:, 2], uvz[:, 2]], 1).astype(np.float32)
    rgb = np.random.default_rng(seed + 11).integers(0, 256, (len(verts), 3), dtype=np.uint8)
    return verts, np.asarray(faces, np.int32).reshape(-1, 3), rgb


def flip(faces, which):
    faces = np.array(faces, np.int32)
    for f in which:
        faces[f] = faces[f, ::-1]
    return faces


# ---- builders: each -> (verts, faces, rgb, cams (n, 16)) ---------------------------------------------------------------------------
def right_triangle():
    """(1,1), (5,1), (1,5): vertices, the top edge, the left edge and the hypotenuse x + y = 6 all pass through pixel centres"""
    return pix_mesh([(1, 1, 2), (5, 1, 2), (1, 5, 2)], [(0, 1, 2)]) + (PIX[None],)


def between_samples():
    return pix_mesh([(2.25, 2.25, 2), (2.75, 2.25, 2), (2.25, 2.75, 2), (0.25, 0.5, 2), (0.75, 0.5, 2), (0.5, 0.75, 2)], [(0, 1, 2), (5, 4, 3)]) + (PIX[None],)


def shared_edge(flip_first, flip_second):
    """the square [1, 4] x [1, 4] split along the diagonal (1,1) - (4,4), which passes through the centres (2,2) and (3,3)"""
    v, f, c = pix_mesh([(1, 1, 2), (4, 1, 2), (4, 4, 2), (1, 4, 2)], [(0, 1, 2), (0, 2, 3)])
    return v, flip(f, [i for i, on in enumerate((flip_first, flip_second)) if on]), c, PIX[None]


def fan64():
    """64 faces round the pixel centre (3, 2), rim at radius 200: the fan covers every image of SIZES, and its axis-parallel and
    diagonal spokes pass through pixel centres; every second face is reversed"""
    ang = 2 * np.pi * np.arange(64) / 64
    rim = [(3 + 200 * np.cos(a), 2 + 200 * np.sin(a), 2) for a in ang]
    faces = [(0, 1 + k, 1 + (k + 1) % 64) for k in range(64)]
    v, f, c = pix_mesh([(3, 2, 2)] + rim, faces)
    return v, flip(f, range(0, 64, 2)), c, PIX[None]


GRID_N, GRID_STEP, GRID_AT = 9, 3, (2, 1)


def quad_grid(z=2.0, shuffle=True):
    """9 x 9 quads of 3 x 3 pixels, corners on pixel centres from (2, 1): the union is [2, 29) x [1, 28) under the top-left rule"""
    n = GRID_N + 1
    uvz = [(GRID_AT[0] + GRID_STEP * i, GRID_AT[1] + GRID_STEP * j, z) for j in range(n) for i in range(n)]
    idx = np.arange(n * n).reshape(n, n)
    a, b, c_, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    faces = np.stack([np.stack([a, b, c_], 1), np.stack([b, d, c_], 1)], 1).reshape(-1, 3)
    if shuffle:
        rng = np.random.default_rng(3)
        faces = faces[rng.permutation(len(faces))]
        faces = flip(faces, np.nonzero(rng.random(len(faces)) < 0.5)[0])
    v, f, c = pix_mesh(uvz, faces)
    return v, f, c, PIX[None]


def grid_count(W, H):
    x = max(0, min(W, GRID_AT[0] + GRID_STEP * GRID_N) - GRID_AT[0])
    y = max(0, min(H, GRID_AT[1] + GRID_STEP * GRID_N) - GRID_AT[1])
    return x * y


def degenerate():
    """faces whose vertices differ in fp32 and fall on one lattice point or one lattice line, then one proper face in both orientations"""
    uvz = [(1, 1, 2), (2, 2, 2), (3, 3.0001, 2),                        # collinear on the lattice: 0.0001 px is 0.0256 of a lattice step
           (4.0001, 1.0001, 2), (4.0002, 1.0001, 2), (4.0001, 1.0002, 2),  # one lattice point
           (1, 2, 2), (5, 2, 2), (1, 4, 2)]
    return pix_mesh(uvz, [(0, 1, 2), (2, 1, 0), (3, 4, 5), (6, 7, 8), (8, 7, 6)]) + (PIX[None],)


def hostile():
    """one face per hostile vertex, its other two vertices good; near = 0.5.  The faces with u = +-2^16 are usable in the first view
    (cx = 0) and clipped in the views whose cx moves u to the next fp64 beyond (the spacing of fp64 at 2^16 is 2^-36)."""
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    bad = [(1.0, 1.0, 0.5), (1.0, 1.0, below), (1.0, 1.0, 0.0), (1.0, 1.0, -1.0), (np.nan, 1.0, 2.0), (1.0, 1.0, np.nan), (1.0, np.inf, 2.0), (1.0, 1.0, np.inf),
           (1.0, 1.0, -np.inf), (1.0, 1.0, 1e30), (1e30, 1.0, 2.0), (65536.0 * 2, 1.0, 2.0), (-65536.0 * 2, 1.0, 2.0), (1.0, 65536.0 * 2, 2.0),
           (1.0, -65536.0 * 2, 2.0)]
    verts, faces = [], []
    for k, p in enumerate(bad):
        verts += [p, (14.0, 2.0 + (2 * k) % 7, 2.0), (2.0, 12.0, 2.0)]
        faces.append((3 * k, 3 * k + 1, 3 * k + 2))
    nv = len(verts)
    faces += [(-1, 1, 2), (0, nv, 2), (0, 1, INT_MAX), (INT_MIN, 1, 2), (1, 1, 2), (1, 2, 4)]
    verts = np.asarray(verts, np.float32)
    rgb = np.random.default_rng(5).integers(0, 256, (nv, 3), dtype=np.uint8)
    eps = 2.0 ** -36
    return verts, np.asarray(faces, np.int32), rgb, np.stack([pix_cam(), pix_cam(eps, eps), pix_cam(-eps, -eps)])


def sizes_of_boxes():
    """a face far larger than any image, boxes of exactly SMALL_SIDE pixels and one more in x and in y, a sliver across 64 x 48"""
    s = MR.SMALL_SIDE
    uvz = [(-1000, -1000, 4), (3000, -1000, 2), (-1000, 3000, 8),
           (1, 1, 2), (s, 1, 2), (1, 3, 2), (1, 5, 2), (s + 1, 5, 2), (1, 7, 2),
           (12, 1, 1), (14, 1, 1), (12, s, 1), (16, 1, 1), (18, 1, 1), (16, s + 1, 1),
           (-5, 0.3, 1), (70, 47.6, 1), (70, 47.9, 1)]
    return pix_mesh(uvz, [(0, 1, 2), (3, 4, 5), (6, 7, 8), (9, 10, 11), (12, 13, 14), (15, 16, 17)]) + (PIX[None],)


def coplanar_twins():
    """faces 1 and 3 are the same triangle under other vertex numbers (3 reversed), in front of face 0 and behind face 2's plane"""
    uvz = [(0, 0, 4), (40, 0, 4), (0, 40, 4), (1, 1, 2), (9, 1, 2), (1, 9, 2), (1, 1, 2), (9, 1, 2), (1, 9, 2), (2, 2, 1), (4, 2, 1), (2, 4, 1)]
    return pix_mesh(uvz, [(0, 1, 2), (3, 4, 5), (9, 10, 11), (8, 7, 6)]) + (PIX[None],)


def interpenetrating():
    uvz = [(1, 1, 1), (30, 2, 4), (3, 30, 4), (30, 30, 1), (2, 3, 4), (28, 1, 4)]
    return pix_mesh(uvz, [(0, 1, 2), (3, 4, 5)]) + (PIX[None],)


def random_scene(n=40, seed=9):
    rng = np.random.default_rng(seed)
    uvz = np.concatenate([rng.uniform(-8, 72, (3 * n, 1)), rng.uniform(-8, 56, (3 * n, 1)), rng.uniform(1.0, 9.0, (3 * n, 1))], 1)
    uvz[: 3 * (n // 2)] = uvz[: 3 * (n // 2)] * [0.15, 0.15, 1.0] + [20.0, 15.0, 0.0]     # half of the faces small
    return pix_mesh(uvz, np.arange(3 * n).reshape(n, 3), seed) + (PIX[None],)


def three_views():
    """an extracted sphere (marching tetrahedra, outward normals) seen by three cameras of different pose and intrinsics whose
    entries are not representable in fp32"""
    r = C.extract_reference("sphere_13x13x14")
    cams = []
    for k, (ax, ay) in enumerate(((0.1, -0.2), (-0.3, 0.4), (0.05, 3.0))):
        R = C.rot(ax, ay)
        Cw = np.array([6.3, 6.6, 7.1]) - (14.0 + k) * R[2] + 0.1 * k
        cams.append(C.cam_row(R, -R @ Cw, 50.1 + k, 49.3 - k, 31.7 - k, 23.9 + 0.7 * k))
    return np.array(r["verts"]), np.array(r["faces"]), np.array(r["rgb"]), np.stack(cams)


def below_fp32():
    """a left edge at u = 3 + 1/512, the rounding boundary of the lattice: with cx = 0 it snaps to 769 and the column x = 3 lies
    outside; with cx = -1e-13, far below fp32's spacing, it snaps to 768 and the column lies on a left edge, inside"""
    u = 3.0 + 1.0 / 512
    return pix_mesh([(u, 1, 2), (6, 1, 2), (u, 4, 2)], [(0, 1, 2)]) + (np.stack([pix_cam(), pix_cam(-1e-13, 0.0)]),)


def slanted_plane():
    """one face far larger than the image on the plane through three fp32 points, depth 2 .. 6 across 64 pixels"""
    return pix_mesh([(-20, -30, 1.25), (150, -10, 9.5), (-10, 160, 3.5)], [(0, 1, 2)]) + (PIX[None],)


def flat_colour():
    v, f, c, cams = random_scene(30, 4)
    c = np.empty_like(c)
    c[:] = (17, 200, 93)
    return v, f, c, cams


def colour_ramp():
    """colours 0 / 0 / 255: the bytes rise monotonically towards the third vertex (60, 24); depths differ, so the ramp is not linear"""
    v, f, c = pix_mesh([(-2, -2, 1), (-2, 50, 4), (60, 24, 2)], [(0, 1, 2)])
    c = np.array([[0, 0, 0], [0, 0, 0], [255, 255, 255]], np.uint8)
    return v, f, c, PIX[None]


CASES = {
    "nv_0_nf_0": lambda: (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint8), PIX[None]),
    "nv_0_with_faces": lambda: (np.zeros((0, 3), np.float32), np.array([(0, 1, 2), (0, 0, 0)], np.int32), np.zeros((0, 3), np.uint8), PIX[None]),
    "nf_0": lambda: pix_mesh([(1, 1, 2), (2, 1, 2), (1, 2, 2)], np.zeros((0, 3))) + (PIX[None],),
    "right_triangle": right_triangle,
    "between_samples": between_samples,
    "shared_edge_00": lambda: shared_edge(False, False),
    "shared_edge_01": lambda: shared_edge(False, True),
    "shared_edge_10": lambda: shared_edge(True, False),
    "shared_edge_11": lambda: shared_edge(True, True),
    "fan64": fan64,
    "quad_grid": quad_grid,
    "degenerate": degenerate,
    "hostile": hostile,
    "sizes_of_boxes": sizes_of_boxes,
    "coplanar_twins": coplanar_twins,
    "interpenetrating": interpenetrating,
    "random_scene": random_scene,
    "three_views": three_views,
    "below_fp32": below_fp32,
    "slanted_plane": slanted_plane,
    "flat_colour": flat_colour,
    "colour_ramp": colour_ramp,
}


@functools.lru_cache(maxsize=None)
def case(name):
    out = CASES[name]()
    for a in out:
        a.setflags(write=False)
    return out


def sizes(name):
    """every case runs at every size of SIZES"""
    return SIZES


def case_keys():
    return [(name, W, H, cull) for name in CASES for (W, H) in sizes(name) for cull in ("none", "back")]


@functools.lru_cache(maxsize=None)
def reference(name, W, H, cull, background=(0, 0, 0), with_rgb=True):
    v, f, c, cams = case(name)
    r = O.render(v, f, c if with_rgb else None, cams, H, W, NEAR, cull, background)
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(dev, name, W, H, cull="none", background=(0, 0, 0), with_rgb=True, cams=None):
    v, f, c, case_cams = case(name)
    tv, tf, tc = to_dev(dev, v, f, c if with_rgb else None)
    return MR.render(tv, tf, tc, case_cams if cams is None else cams, H, W, near=NEAR, cull=cull, background=background)


def assert_equal(got, want, what):
    """a render() result against the oracle's, every output in every bit"""
    assert got["depth"].dtype == torch.float32 and got["face"].dtype == torch.int32 and got["rgb"].dtype == torch.uint8 and got["shade"].dtype == torch.uint8
    keys = host(got["keys"]).view(np.uint64)
    if not np.array_equal(keys, want["keys"]):
        at = np.argwhere(keys != want["keys"])[:5]
        print(what, "keys differ at", at.tolist(), "got", [hex(int(keys[tuple(i)])) for i in at], "want", [hex(int(want["keys"][tuple(i)])) for i in at])
    assert np.array_equal(keys, want["keys"]), what
    assert np.array_equal(bits(host(got["depth"])), bits(want["depth"])), what
    assert np.array_equal(host(got["face"]), want["face"]), what
    assert np.array_equal(host(got["rgb"]), want["rgb"]), what
    assert np.array_equal(host(got["shade"]), want["shade"]), what
    assert MR.stats_rows(got) == want["stats"], (what, MR.stats_rows(got), want["stats"])
    assert bool((got["stats"][:, len(MR.STAT_NAMES):] == 0).all())


def single_coverage(name, W, H):
    """per pixel, the number of faces of the case that cover it when each is rendered alone (the oracle)"""
    v, f, c, cams = case(name)
    count = np.zeros((H, W), np.int64)
    for k in range(len(f)):
        count += O.render(v, f[k:k + 1], None, cams[:1], H, W, NEAR)["face"][0] >= 0
    return count


def check_known(name, W, H, cull):
    """the hand answers, on the oracle alone"""
    want = reference(name, W, H, cull)
    st = want["stats"][0]
    v, f, c, cams = case(name)
    assert sum(s for k, s in st.items() if k.startswith("faces_") and k != "faces_large") == len(f), (name, st)
    assert st["pixels_covered"] == int((want["face"][0] >= 0).sum()) == int((want["depth"][0] > 0).sum())
    covered = want["face"][0] >= 0
    if name in ("nv_0_nf_0", "nv_0_with_faces", "nf_0", "between_samples"):
        assert not (want["face"] >= 0).any() and (want["depth"] == 0).all() and (want["shade"] == 0).all() and (want["rgb"] == 0).all()
        assert st["faces_invalid"] == (2 if name == "nv_0_with_faces" else 0)
        if name == "between_samples":
            assert st["faces_drawn"] == (2 if cull == "none" else 1) and st["faces_large"] == 0
    if name == "right_triangle":
        # x >= 1 (the left edge owns its samples), y >= 1 (the top edge does), x + y < 6 (the hypotenuse is neither): 4 + 3 + 2 + 1 pixels
        inside = {(x, y) for y in range(1, 5) for x in range(1, 6 - y) if x < W and y < H}
        assert {(int(x), int(y)) for y, x in np.argwhere(covered)} == (inside if cull == "none" else set()), name
        if (W, H) == (7, 5) and cull == "none":
            assert covered.sum() == 10 and (bits(want["depth"][0][covered]) == bits(np.float32(2.0))).all()
    if name.startswith("shared_edge"):
        flipped = [name[-2] == "1", name[-1] == "1"]                  # as built the faces have area2 > 0: a flipped one faces the camera
        union = np.zeros((H, W), bool)
        union[1:4, 1:4] = True
        if cull == "none":
            assert np.array_equal(covered, union), name
            assert np.array_equal(single_coverage(name, W, H), union.astype(np.int64)), name      # each pixel of the union exactly once
        else:
            assert st["faces_culled"] == 2 - sum(flipped) and st["faces_drawn"] == sum(flipped)
    if name == "fan64" and cull == "none":
        assert covered.all() and (single_coverage(name, W, H) == 1).all() and st["faces_drawn"] == 64
    if name == "fan64" and cull == "back":
        assert st["faces_culled"] == 32 and st["faces_drawn"] == 32
    if name == "quad_grid" and cull == "none":
        assert st["pixels_covered"] == grid_count(W, H) and st["faces_drawn"] == 2 * GRID_N * GRID_N, (name, st)
        assert (bits(want["depth"][0][covered]) == bits(np.float32(2.0))).all()                   # iz = 0.5: every product and sum is exact
        assert (want["shade"][0][covered] == 255).all()
        if (W, H) == (64, 48):
            assert st["pixels_covered"] == 27 * 27 and (single_coverage(name, W, H)[covered] == 1).all()
    if name == "degenerate":
        assert st["faces_degenerate"] == 3
        assert (st["faces_drawn"], st["faces_culled"]) == ((2, 0) if cull == "none" else (1, 1))
    if name == "hostile":
        # view 0: z = 0.5 (= near), 1e30 and the four +-2^16 are usable; z below near, 0, -1, NaN, +-inf and x = 1e30 are not
        s0, s1, s2 = want["stats"]
        assert s0["faces_invalid"] == s1["faces_invalid"] == 5 and s0["faces_clipped"] == 9, s0
        assert s0["faces_drawn"] + s0["faces_culled"] == 7
        assert s1["faces_clipped"] == s2["faces_clipped"] == 11, (s1, s2)                      # u = 2^16 + 2^-36 and v likewise are beyond the guard
    if name == "sizes_of_boxes" and (W, H) == (64, 48) and cull == "none":
        assert st["faces_large"] == 4 and st["faces_drawn"] == 6, st                            # the giant, the two of SMALL_SIDE + 1, the sliver
        assert covered.all()
    if name == "coplanar_twins" and (W, H) == (64, 48):
        if cull == "none":
            assert set(np.unique(want["face"][0])) == {-1, 0, 1, 2} and (want["face"][0][3:6, 3:6] != 3).all()     # of the twins the smaller number
        else:
            assert set(np.unique(want["face"][0])) == {-1, 3} and st["faces_culled"] == 3       # alone, the reversed twin shows
    if name == "interpenetrating" and (W, H) == (64, 48) and cull == "none":
        assert set(np.unique(want["face"][0])) == {-1, 0, 1}
    if name == "below_fp32" and cull == "none" and W > 3 and H > 3:
        f0, f1 = want["face"]
        assert (f0[1:4, 3] == -1).all() and (f1[1:3, 3] == 0).all() and not np.array_equal(want["keys"][0], want["keys"][1])
    if name == "flat_colour":
        assert (want["rgb"][0][covered] == (17, 200, 93)).all() and (want["rgb"][0][~covered] == 0).all() and (covered.sum() > 500 or W < 64)
    if name == "colour_ramp" and (W, H) == (64, 48) and cull == "none":
        row = want["rgb"][0][24, :, 0].astype(int)
        assert covered[24, :60].all() and (np.diff(row[:60]) >= 0).all() and row[0] < 20 and row[59] > 240 and len(set(row[:60])) > 40
        assert (want["rgb"][0][..., 0] == want["rgb"][0][..., 2]).all()
    if name == "slanted_plane" and cull == "none":
        check_slanted_plane(want, W, H)
    if name == "three_views":
        # the extracted sphere is closed with outward normals: the faces a camera outside sees have area2 < 0, so culling the back
        # faces changes no pixel, and about half of the faces are culled
        other = reference(name, W, H, "none" if cull == "back" else "back")
        for key in ("keys", "depth", "face", "rgb", "shade"):
            assert np.array_equal(other[key], want[key]), key
        for s in reference(name, W, H, "back")["stats"]:
            assert 0.35 * len(f) < s["faces_culled"] < 0.65 * len(f) and (s["pixels_covered"] > 300 or (W, H) != (64, 48))


def check_slanted_plane(want, W, H):
    """The rendered depth of a face on a plane against the ray-plane depth.

    Bound.  On the plane, g = 1 / z is linear in the pixel position P: g(P) = n . (P, 1) / d with the plane n . p = d through the
    three fp32 vertices and fx = fy = 1, cx = cy = 0; its gradient per pixel is G = (n_x, n_y) / d.  The rasteriser interpolates the
    vertices' 1 / z with barycentric weights l_i of the SNAPPED positions Q_i, so it returns g(P + sum l_i (P_i - Q_i)): a convex
    combination (inside, l_i >= 0) of the snapping moves, each at most sqrt(2) / 512 px (half a lattice step per axis).  Hence
    |g~ - g| <= |G| sqrt(2) / 512 and |z~ - z| = |g - g~| z z~ <= |G| (sqrt(2) / 512) z z~.  The result is rounded once to fp32,
    2^-24 z~, and the fp64 evaluation of either side is below 1e-12 z."""
    v = case("slanted_plane")[0].astype(np.float64)
    n = np.cross(v[1] - v[0], v[2] - v[0])
    d = n @ v[0]
    py, px = np.mgrid[0:H, 0:W].astype(np.float64)
    z = d / (n[0] * px + n[1] * py + n[2])
    got = want["depth"][0].astype(np.float64)
    assert (want["face"][0] == 0).all()
    bound = np.hypot(n[0], n[1]) / abs(d) * (np.sqrt(2.0) / 512) * z * got + 2.0 ** -24 * got + 1e-12 * z
    err = np.abs(got - z)
    print(f"slanted plane {W}x{H}: max |depth - ray-plane| = {err.max():.3g}, bound there {bound.ravel()[err.argmax()]:.3g}, depth {z.min():.3g} .. {z.max():.3g}")
    assert (err <= bound).all()


def check_case(dev, name, W, H, cull, twice=False):
    check_known(name, W, H, cull)
    want = reference(name, W, H, cull)
    got = run(dev, name, W, H, cull)
    print(f"{name} {W}x{H} cull={cull}: {MR.stats_rows(got)}")
    assert_equal(got, want, (name, W, H, cull))
    if twice:
        again = run(dev, name, W, H, cull)
        for key in got:
            assert torch.equal(got[key], again[key]), (name, key)


def check_without_colours_and_background(dev):
    for name, (W, H) in (("random_scene", (64, 48)), ("quad_grid", (7, 5))):
        want = reference(name, W, H, "none", (1, 2, 250), False)
        got = run(dev, name, W, H, "none", (1, 2, 250), False)
        assert_equal(got, want, name)
        covered = want["face"][0] >= 0
        assert (want["rgb"][0][covered] == 255).all() and (want["rgb"][0][~covered] == (1, 2, 250)).all() and (~covered).any()


def check_permutation(dev):
    """the random scene with its faces in another order and every second one reversed: depth, colour and shade are equal and the face
    numbers map through the permutation (no two faces of the scene give a pixel the same depth bits)"""
    v, f, c, cams = case("random_scene")
    perm = np.random.default_rng(1).permutation(len(f))
    g = flip(f[perm], range(0, len(f), 2))
    a = run(dev, "random_scene", 64, 48)
    tv, tf, tc = to_dev(dev, v, g, c)
    b = MR.render(tv, tf, tc, cams, 48, 64, near=NEAR)
    fa, fb = host(a["face"]), host(b["face"])
    assert (fa >= 0).sum() > 500 and len(np.unique(fa)) > 10
    assert torch.equal(a["depth"].view(torch.int32), b["depth"].view(torch.int32)) and torch.equal(a["rgb"], b["rgb"]) and torch.equal(a["shade"], b["shade"])
    assert np.array_equal(fa >= 0, fb >= 0) and np.array_equal(perm[fb[fb >= 0]], fa[fa >= 0])


def check_views_one_by_one(dev):
    """three views in one call against three calls"""
    for name in ("three_views", "hostile"):
        W, H = sizes(name)[-1]
        cams = case(name)[3]
        whole = run(dev, name, W, H)
        for k in range(len(cams)):
            one = run(dev, name, W, H, cams=cams[k:k + 1])
            for key in whole:
                assert torch.equal(whole[key][k:k + 1], one[key]), (name, k, key)


def check_large_path_alone(dev):
    """a list longer than the large kernel's grid: 1500 faces of 9 x 9 pixels over one another at rising depth, the nearest first
    in number and last in the list as often as not"""
    rng = np.random.default_rng(2)
    n = 1500
    uvz = []
    for k in range(n):
        z = 1.0 + rng.random()
        x, y = rng.integers(0, 50), rng.integers(0, 35)
        uvz += [(x, y, z), (x + 9, y, z), (x, y + 9, z)]
    v, f, c = pix_mesh(uvz, np.arange(3 * n).reshape(n, 3))
    want = O.render(v, f, c, PIX[None], 48, 64, NEAR)
    assert want["stats"][0]["faces_large"] == n
    tv, tf, tc = to_dev(dev, v, f, c)
    assert_equal(MR.render(tv, tf, tc, PIX[None], 48, 64, near=NEAR), want, "large list")


# ---- compare --------------------------------------------------------------------------------------------------------------------
def compare_inputs(V=2, H=67, W=131, seed=0):
    """more than one tile of 4096 pixels and no multiple of it; holes of every kind in both maps, differences at the thresholds"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(1.0, 9.0, (V, H, W)).astype(np.float32)
    r = (d.astype(np.float64) * (1.0 + rng.choice([0.0, 0.0005, 0.001, 0.01, 0.02, -0.01, 0.3], (V, H, W)))).astype(np.float32)
    for a, s in ((d, 1), (r, 2)):
        m = np.random.default_rng(seed + s).random((V, H, W))
        a[m < 0.1] = 0.0
        a[(m >= 0.1) & (m < 0.13)] = -1.0
        a[(m >= 0.13) & (m < 0.16)] = np.nan
        a[(m >= 0.16) & (m < 0.18)] = np.inf
    return r, d


def assert_rows(got, want, what):
    for g, w in zip(got, want):
        assert {k: g[k] for k in ("both", "only_mesh", "only_map", "within")} == {k: w[k] for k in ("both", "only_mesh", "only_map", "within")}, (what, g, w)
        assert abs(g["sum_abs"] - w["sum_abs"]) <= 1e-12 * abs(w["sum_abs"]), (what, g["sum_abs"], w["sum_abs"])
        assert (g["mean_abs"] is None) == (w["mean_abs"] is None)
    assert len(got) == len(want)


def check_compare(dev):
    for shape, th in (((2, 67, 131), (0.001, 0.01, 0.05)), ((1, 1, 1), (0.0,)), ((3, 5, 7), ()), ((1, 64, 64), (0.0, 1.0))):
        r, d = compare_inputs(*shape)
        want = O.compare(r, d, th)
        tr, td = torch.from_numpy(r).to(dev), torch.from_numpy(d).to(dev)
        got = MR.compare(tr, td, th)
        print(f"compare {shape} {th}: {got[0]}")
        assert_rows(got, want, shape)
        t1, t2 = MR.compare_table(tr, td, th), MR.compare_table(tr, td, th)
        assert torch.equal(t1, t2)                                     # two runs identical, the fp64 sum's bits included
        if shape[0] == 2:
            assert want[0]["both"] > 4096 and want[0]["only_mesh"] > 0 and want[0]["only_map"] > 0 and 0 < want[0]["within"][0] < want[0]["within"][1] < want[0]["both"]
    same = MR.compare(td, td, (0.0,))
    assert same[0]["sum_abs"] == 0.0 and same[0]["within"] == [same[0]["both"]] and same[0]["only_mesh"] == same[0]["only_map"] == 0


def check_refusals(dev):
    """bad arguments of the module, on the device's path, and of the oracle"""
    v, f, c, cams = case("right_triangle")
    tv, tf, tc = to_dev(dev, v, f, c)
    good = dict(cams=cams, H=5, W=7, near=NEAR, cull="none", background=(0, 0, 0))
    for kw, pattern in (({"H": 0}, "H"), ({"W": 0}, "W"), ({"H": MR.MAX_SIDE + 1}, "H"), ({"W": MR.MAX_SIDE + 1}, "W"), ({"H": 5.0}, "H"), ({"near": 0.0}, "near"),
                        ({"near": -1.0}, "near"), ({"near": float("nan")}, "near"), ({"near": float("inf")}, "near"), ({"cams": np.zeros((0, 16))}, "views"),
                        ({"cull": "front"}, "cull"), ({"background": (0, 0, 256)}, "background"), ({"background": (0, 0)}, "background")):
        a = dict(good, **kw)
        try:
            MR.render(tv, tf, tc, a["cams"], a["H"], a["W"], near=a["near"], cull=a["cull"], background=a["background"])
        except _lib.RcmvsError as e:
            assert pattern in str(e), (kw, str(e))
        else:
            raise AssertionError(f"{kw} was accepted")
        if set(kw) & {"H", "W", "near", "cams"} and kw != {"H": 5.0}:
            try:
                O.render(v, f, c, a["cams"], a["H"], a["W"], a["near"], a["cull"])
            except O.Refused:
                pass
            else:
                raise AssertionError(f"the oracle accepted {kw}")
    for bad in (lambda: MR.render(tv, tf, tc[:2], cams, 5, 7), lambda: MR.render(tv, tf.long(), tc, cams, 5, 7), lambda: MR.compare(tv, tv, (0.1,)),
                lambda: MR.compare(torch.zeros((1, 2, 2)).to(dev), torch.zeros((1, 2, 3)).to(dev)), lambda: MR.compare(torch.zeros((1, 2, 2)).to(dev),
                torch.zeros((1, 2, 2)).to(dev), (0.1, 0.2, 0.3, 0.4)), lambda: MR.compare(torch.zeros((1, 2, 2)).to(dev), torch.zeros((1, 2, 2)).to(dev), (-0.1,))):
        try:
            bad()
        except _lib.RcmvsError:
            pass
        else:
            raise AssertionError("a bad argument was accepted")


# ---- the round trip on the sphere scene --------------------------------------------------------------------------------------------
SCENE = "5x4x4"


def sphere_truth(name=SCENE):
    """the scene's exact sphere per view: depth along z (0 off the sphere), the incidence cosine between the ray and the normal, and
    the cosine between the ray and the camera's axis"""
    depth, cams, rgb, trunc, grid, bdims = SC.scene(name)
    h = grid[3]
    dims = np.array(SC.S.dims_of(bdims), np.float64)
    centre = np.array(grid[:3]) + 0.5 * dims * h
    radius = 0.3 * dims.min() * h
    n, H, W = depth.shape
    zs, cosines, axes = [], [], []
    for c in cams:
        R, t = c[:9].reshape(3, 3), c[9:12]
        jj, ii = np.mgrid[0:H, 0:W]
        ray = np.stack([(ii - c[14]) / c[12], (jj - c[15]) / c[13], np.ones((H, W))], -1)
        oc = -(R @ centre + t)
        A, B, Cq = (ray * ray).sum(-1), 2 * (ray * oc).sum(-1), (oc * oc).sum() - radius ** 2
        disc = B * B - 4 * A * Cq
        z = np.where(disc > 0, (-B - np.sqrt(np.maximum(disc, 0))) / (2 * A), 0.0)
        p = ray * z[..., None]
        normal = (p + oc) / radius
        unit = ray / np.linalg.norm(ray, axis=-1, keepdims=True)
        zs.append(z)
        cosines.append(np.where(z > 0, -(normal * unit).sum(-1), 0.0))
        axes.append(1.0 / np.linalg.norm(ray, axis=-1))
    return np.stack(zs), np.stack(cosines), np.stack(axes), h, radius


def check_round_trip(dev, record=None):
    """Extract the sphere scene's mesh, render it into the scene's cameras and compare with the scene's depth maps, as extracted
    and after clean_mesh(smooth), fill_holes and decimate.

    Bound on |r - d| at a pixel whose ray meets the sphere (radius R) at an incidence cosine c >= 0.5, for the mesh as extracted,
    evaluated per pixel with that pixel's own c.  It has the form the extraction's vertex bound gives, a normal offset divided by c
    plus the sag of a chord of one voxel; the terms beyond sqrt(3) h are there because this scene's depth maps are the sphere's
    depth plus noise.  Let N be the largest |noise| of the input maps (measured on the inputs, from the exact sphere; the noise's
    sigma is 0.3 h, its maximum some 0.95 h) and ca the smallest cosine between a ray to the sphere and its camera's axis.
    (1) Where the fused field changes sign.  A view's term at a point p is its map's depth minus zc: the depth gap between p and
    the sphere along that view's ray, plus that pixel's noise.  At a normal offset t outside the sphere the gap is t times
    (cosine to the axis) / (incidence cosine) >= t ca; so beyond t = N / ca every observing view's term is positive (clamping
    keeps the sign), and beyond -N / ca every term is negative: the mean changes sign only within N / ca of the sphere.
    (2) The extraction puts a vertex on a grid edge whose ends have opposite signs, at most a cube's diagonal sqrt(3) h from
    either: a vertex lies within sqrt(3) h + N / ca of the sphere.  (3) Snapping moves a vertex by at most sqrt(2) / 512 px in the
    image, s = (sqrt(2) / 512) z_max / f in space.  So the rendered vertices lie within e = sqrt(3) h + N / ca + s of the sphere,
    normal to it, and a ray of incidence cosine c meets such an offset e / c further along, in distance and so in depth.
    (4) A face spans at most one voxel, a chord of at most sqrt(3) h: its sag below its vertices is at most 3 h^2 / (8 (R - e)).
    (5) The result is rounded once to fp32, 2^-24 r.  (6) d itself is the sphere's depth within N; this is the one place the
    noise of d enters.  So |r - d| <= (sqrt(3) h + N / ca + s) / c + 3 h^2 / (8 (R - e)) + N + 2^-24 r: 3.7 h at the disc's
    centre, 6.4 h at c = 0.5.  e / c is the first-order displacement, smaller than the exact one through a shell of that
    thickness, and the nearest-pixel lookup of the fusion is not counted: both would only loosen the bound.  The render culls
    back faces: through a hole of the front a ray would otherwise see the inside of the far half, a sphere's diameter away.  After
    smoothing, hole filling and decimation no bound is claimed: only the table is recorded."""
    depth, cams, rgb, trunc, grid, bdims = SC.scene(SCENE)
    z, cosine, axis, h, radius = sphere_truth()
    n, H, W = depth.shape
    on = depth > 0
    assert np.array_equal(on, z > 0)
    noise = float(np.abs(depth.astype(np.float64) - z)[on].max())
    snap = np.sqrt(2.0) / 512 * float(z.max()) / float(cams[:, 12:14].min())
    e = np.sqrt(3.0) * h + noise / float(axis[on].min()) + snap
    with np.errstate(divide="ignore"):
        bound = e / cosine + 3.0 * h * h / (8.0 * (radius - e)) + noise          # per pixel; + 2^-24 r where it is compared
    d, c = torch.from_numpy(np.array(depth)).to(dev), torch.from_numpy(rgb).to(dev)
    vol = TM.TsdfVolume(grid[:3], grid[3], SC.S.dims_of(bdims), dev)
    vol.integrate(d, cams, c, trunc=trunc)
    verts, faces, col = vol.extract(1)
    lines = []
    meshes = {"extracted": (verts, faces, col)}
    meshes["smoothed"] = MC.clean_mesh(verts, faces, col, keep_largest=1, smooth_iterations=3)[:3]
    meshes["filled"] = MH.fill_holes(*meshes["smoothed"], max_edges=64)[:3]
    meshes["decimated"] = MD.decimate(*meshes["filled"], cell=2.0 * h)[:3]
    for what, (mv, mf, mc) in meshes.items():
        out = MR.render(mv, mf, mc, cams, H, W, near=1e-3, cull="back")
        rows = MR.compare(out["depth"], d, (0.01, 0.05))
        total = MR.sum_rows(rows, (0.01, 0.05))
        assert_rows(rows, O.compare(host(out["depth"]), depth, (0.01, 0.05)), what)
        assert total["both"] > 0 and all(np.isfinite(v) for v in (total["sum_abs"], total["mean_abs"])) and total["both"] + total["only_map"] == int(on.sum())
        r = host(out["depth"]).astype(np.float64)
        sel = (cosine >= 0.5) & (r > 0) & on
        err, limit = np.abs(r - depth)[sel], (bound + 2.0 ** -24 * r)[sel]
        worst, at = float(err.max()), int((err / limit).argmax())
        lines.append(f"round trip {what}: {int(mf.shape[0])} faces, table {json.dumps(total)}, max |r - d| at cosine >= 0.5 = {worst:.4f}, "
                     f"largest |r - d| / bound = {float((err / limit).max()):.3f} (there {err[at]:.4f} against {limit[at]:.4f} at cosine {cosine[sel][at]:.3f}; "
                     f"h = {h}, noise max {noise:.4f}, bound {float(limit.min()):.4f} .. {float(limit.max()):.4f})")
        print(lines[-1])
        if what == "extracted":
            # Rays at cosine >= 0.5 cover sin^2(60 deg) = 3/4 of the sphere's disc.  The fusion of three noisy views leaves holes
            # (noise of sigma 0.3 h, at most 0.95 h, against a truncation of 1.5 h), so no coverage is claimed beyond most of those rays meeting the mesh.
            steep = int(((cosine >= 0.5) & on).sum())
            assert sel.sum() > 0.75 * steep and steep > 0.6 * on.sum()
            assert (err <= limit).all(), (worst, float((err / limit).max()))
    if record:
        os.makedirs(os.path.dirname(record), exist_ok=True)
        with open(record, "w") as fh:
            fh.write("\n".join(lines) + "\n")


# ---- hooks and command line --------------------------------------------------------------------------------------------------------
def check_off_is_today(dev, tmp_path):
    """mesh_scan without render_dir: PLY bytes and summary keys as the oracle of the TSDF suite fixes them (tsdf_cases.check_end_to_end
    demands those bytes of the parent commit too), no folder written; with it the same PLY bytes, the same keys plus "render", whose
    table equals compare() of a render of the written mesh into the filtered views"""
    pair_folder, out_folder = C.write_scan(tmp_path)
    plain_ply, ply, rdir = (str(tmp_path / "out" / n) for n in ("plain.ply", "rendered.ply", "render"))
    kw = dict(resolution=32, device=dev)
    plain = TM.mesh_scan(pair_folder, out_folder, out_folder, plain_ply, C.PROB, C.NCONS, C.DIST, C.DEPTH, **kw)
    assert list(plain) == ["mesh", "origin", "dims", "voxel", "trunc", "min_weight", "views", "vertices", "faces", "unreferenced_vertices", "observed_voxels"]
    assert not os.path.exists(rdir)
    views = TM.filtered_views(pair_folder, out_folder, out_folder, C.PROB, C.NCONS, C.DIST, C.DEPTH, device=dev)
    want, _ = C.oracle_mesh_of(views, plain)
    with open(plain_ply, "rb") as fh:
        plain_bytes = fh.read()
    assert plain_bytes == TM.mesh_ply_bytes(want["verts"], want["faces"], want["rgb"])
    summary = TM.mesh_scan(pair_folder, out_folder, out_folder, ply, C.PROB, C.NCONS, C.DIST, C.DEPTH, render_dir=rdir, **kw)
    with open(ply, "rb") as fh:
        assert fh.read() == plain_bytes
    assert list(summary) == list(plain) + ["render"] and {k: v for k, v in summary.items() if k not in ("mesh", "render")} == \
        {k: v for k, v in plain.items() if k != "mesh"}
    tv, tf, tc = to_dev(dev, want["verts"], want["faces"], want["rgb"])
    V, H, W = views["depth"].shape
    out = MR.render(tv, tf, tc, views["cams"], H, W)
    total = MR.sum_rows(MR.compare(out["depth"], views["depth"]), MR.DEFAULT_THRESHOLDS)
    print("render hook:", summary["render"])
    assert {k: v for k, v in summary["render"].items() if k != "stats"} == total and total["both"] > 0 and summary["render"]["stats"]["pixels_covered"] > 0
    assert views["ids"] == list(range(V)) and sorted(os.listdir(os.path.join(rdir, "depth_mesh"))) == ["{:0>8}.pfm".format(v) for v in views["ids"]]
    assert len(os.listdir(os.path.join(rdir, "render"))) == 2 * V
    back = data_io.read_pfm(os.path.join(rdir, "depth_mesh", "00000002.pfm"))[0]
    assert np.array_equal(bits(back), bits(host(out["depth"][2])))
    # the block-sparse volume: the same bytes and keys with and without the option
    sparse_plain, sparse_ply, sdir = (str(tmp_path / "out" / n) for n in ("sparse_plain.ply", "sparse_rendered.ply", "sparse_render"))
    a = TM.mesh_scan(pair_folder, out_folder, out_folder, sparse_plain, C.PROB, C.NCONS, C.DIST, C.DEPTH, sparse=True, **kw)
    b = TM.mesh_scan(pair_folder, out_folder, out_folder, sparse_ply, C.PROB, C.NCONS, C.DIST, C.DEPTH, sparse=True, render_dir=sdir, **kw)
    with open(sparse_plain, "rb") as fa, open(sparse_ply, "rb") as fb:
        assert fa.read() == fb.read()
    assert "render" not in a and list(b) == list(a) + ["render"] and {k: v for k, v in b.items() if k not in ("mesh", "render")} == \
        {k: v for k, v in a.items() if k != "mesh"}
    assert b["render"]["both"] > 0 and b["render"]["views"] == V and b["render"]["stats"]["faces_drawn"] > 0
    return pair_folder, out_folder, plain_ply


def check_command_line_round_trip(dev, tmp_path):
    """python -m rc_mvsnet_amd.mesh_render on a tiny folder: the PFMs read back equal to render(), the PNGs exist with the right size,
    the JSON totals equal compare()"""
    from PIL import Image
    pair_folder, out_folder, ply = check_off_is_today(dev, tmp_path)
    dst = str(tmp_path / "cli")
    total = MR.main(["--mesh", ply, "--pair-folder", pair_folder, "--scan-folder", out_folder, "--out", dst, "--depth-folder", out_folder, "--cull", "back",
                     "--device", dev])
    v, f, c = dtu_io.read_ply_mesh_rgb(ply)
    from rc_mvsnet_amd import scan_io
    names = ["{:0>8}".format(k) for k in range(5)]
    cams = np.stack([TM.camera_row(*scan_io.read_camera_parameters(os.path.join(out_folder, f"cams/{n}_cam.txt"))) for n in names])
    maps = np.stack([data_io.read_pfm(os.path.join(out_folder, f"depth_est/{n}.pfm"))[0] for n in names]).astype(np.float32)
    H, W = maps.shape[1:]
    out = MR.render(*to_dev(dev, v.astype(np.float32), f.astype(np.int32), c.astype(np.uint8)), cams, H, W, cull="back")
    want = MR.sum_rows(MR.compare(out["depth"], torch.from_numpy(maps).to(dev)), MR.DEFAULT_THRESHOLDS)
    assert {k: total[k] for k in want} == want and want["both"] > 0 and total["stats"]["faces_culled"] > 0
    for k, n in enumerate(names):
        assert np.array_equal(bits(data_io.read_pfm(os.path.join(dst, "depth_mesh", n + ".pfm"))[0]), bits(host(out["depth"][k])))
        for kind, mode in (("shade", "L"), ("rgb", "RGB")):
            with Image.open(os.path.join(dst, "render", f"{n}_{kind}.png")) as im:
                assert im.size == (W, H) and im.mode == mode
                assert np.array_equal(np.asarray(im), host(out[kind][k]))
    nopng = str(tmp_path / "cli2")
    MR.main(["--mesh", ply, "--pair-folder", pair_folder, "--scan-folder", out_folder, "--out", nopng, "--size", "9", "11", "--no-png", "--device", dev])
    assert not os.path.exists(os.path.join(nopng, "render")) and data_io.read_pfm(os.path.join(nopng, "depth_mesh", names[0] + ".pfm"))[0].shape == (9, 11)
