"""The cases and checks of the TSDF fusion and marching-tetrahedra kernels (csrc/tsdf_mesh.hip through rc_mvsnet_amd/tsdf_mesh.py),
shared by tests/test_gpu_tsdf_mesh.py (device "cuda:0") and tests/test_tsdf_mesh_emu_cpu.py (the CPU emulation, device "cpu"),
against tests/tsdf_oracle.py.  Every comparison with the oracle is exact: planes, vertices, colours and faces equal in every bit
and in order, totals equal, two runs identical -- the kernels and the oracle do the same correctly rounded fp64 operations in
one written order, and every index is an integer computation."""
import functools
import os

import numpy as np
import torch

import tsdf_oracle as O
from rc_mvsnet_amd import dtu_eval, dtu_io, synthetic, tsdf_mesh as TM

DIMS = (9, 7, 5)                     # 315 voxels: two blocks of the integrate kernel, no multiple of anything
H, W = 6, 8
PROB, NCONS, DIST, DEPTH = 0.8, 3, 0.5, 0.01


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- integration ------------------------------------------------------------------------------------------------------------
def rot(ax, ay):
    cx, sx, cy, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
    return np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])


def cam_row(R, t, fx, fy, cx, cy):
    return np.concatenate([np.asarray(R, np.float64).ravel(), np.asarray(t, np.float64), [fx, fy, cx, cy]])


def random_views(n, seed, scale=1.0, origin=(0.0, 0.0, 0.0)):
    """n cameras some 6 voxels in front of the grid looking along +z with small rotations; the depth maps put a noisy surface
    through the middle of the grid, so a part of the voxels is behind it, a part in front and a part beyond the images"""
    rng = np.random.default_rng(seed)
    centre = np.asarray(origin) + scale * np.array([4.5, 3.5, 2.5])
    cams, depth = [], []
    for _ in range(n):
        R = rot(*(0.08 * rng.standard_normal(2)))
        C = centre + scale * np.array([0.6 * rng.standard_normal(), 0.6 * rng.standard_normal(), -8.5 + 0.3 * rng.standard_normal()])
        cams.append(cam_row(R, -R @ C, 8.0 + rng.random(), 8.0 + rng.random(), 3.5 + 0.3 * rng.standard_normal(), 2.5 + 0.3 * rng.standard_normal()))
        depth.append(scale * (8.5 + 0.8 * rng.standard_normal((H, W))))
    rgb = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    return np.stack(depth).astype(np.float32), np.stack(cams), rgb


def exact_camera(tz=7.5):
    """R = I, t = (-0.5, -0.5, tz), f = 8, c = -0.5 on the unit grid at the origin: xc = i, yc = j and zc = k + 0.5 + tz exactly,
    so where zc = 8 the position is u + 0.5 = i, v + 0.5 = j without rounding"""
    return cam_row(np.eye(3), (-0.5, -0.5, tz), 8.0, 8.0, -0.5, -0.5)


def _views(name):
    grid, trunc = (0.0, 0.0, 0.0, 1.0), 1.5
    if name.startswith("views_"):
        depth, cams, rgb = random_views(int(name[6:]), 10 + int(name[6:]))
    elif name == "no_rgb":
        depth, cams, rgb = random_views(3, 20)
        rgb = None
    elif name == "behind_and_zc_zero":          # a camera inside the grid: zc = k - 2 is negative, exactly 0 (k = 2) and positive
        depth, cams, rgb = random_views(2, 21)
        cams[1] = cam_row(np.eye(3), (-4.5, -3.5, -2.5), 2.0, 2.0, 3.5, 2.5)
        depth[1] = 1.25
    elif name == "image_border":                # u + 0.5 == 0 (inside) and == W (outside) at k = 0, v + 0.5 == H at j = 6
        depth, cams, rgb = random_views(2, 22)
        cams[0] = exact_camera()
        depth[0] = 8.25
    elif name == "bad_depths":
        depth, cams, rgb = random_views(3, 23)
        for v in range(3):
            depth[v].ravel()[[1 + v, 9 + v, 17 + v, 25 + v, 33 + v]] = [0.0, -8.5, np.nan, np.inf, -np.inf]
    elif name == "sdf_at_trunc":                # depth 9, zc = 8 .. 12, trunc 1: sdf = +trunc, 0, -trunc, then beyond
        depth, cams, rgb = random_views(1, 24)
        cams[0], trunc = exact_camera(), 1.0
        depth[0] = 9.0
    elif name == "h_0.1":
        grid, trunc = (0.3, -0.2, 0.1, 0.1), 0.15
        depth, cams, rgb = random_views(3, 25, scale=0.1, origin=grid[:3])
        cams[:, 12:14] = 8.0 + np.arange(6).reshape(3, 2) / 7.0
    elif name == "camera_1e30":                 # zc = 1e30: the pixel is the principal point, sdf = -1e30; xc = 1e30: u is 1e30
        depth, cams, rgb = random_views(3, 26)
        cams[0] = cam_row(np.eye(3), (0.0, 0.0, 1e30), 8.0, 8.0, 3.5, 2.5)
        cams[2] = cam_row(np.eye(3), (1e30, -3.5, 6.0), 8.0, 8.0, 3.5, 2.5)
    else:
        raise KeyError(name)
    return depth, cams, rgb, trunc, grid


INTEGRATE = ("views_1", "views_3", "views_16", "views_17", "no_rgb", "behind_and_zc_zero", "image_border", "bad_depths", "sdf_at_trunc",
             "h_0.1", "camera_1e30")


def planes_of(state):
    return [state["dsum"], state["wsum"]] + list(state["csum"])


@functools.lru_cache(maxsize=None)
def integrate_reference(name):
    depth, cams, rgb, trunc, grid = _views(name)
    state = O.integrate(O.new_state(DIMS), depth, cams, rgb, trunc, grid, DIMS)
    planes = planes_of(state)
    for p in planes:
        p.setflags(write=False)
    return planes


def run_integrate(dev, name, splits=None):
    depth, cams, rgb, trunc, grid = _views(name)
    vol = TM.TsdfVolume(grid[:3], grid[3], DIMS, dev)
    d = torch.from_numpy(depth).to(dev)
    c = None if rgb is None else torch.from_numpy(rgb).to(dev)
    lo = 0
    for n in splits or [len(depth)]:
        vol.integrate(d[lo:lo + n], cams[lo:lo + n], None if c is None else c[lo:lo + n], trunc=trunc)
        lo += n
    assert lo == len(depth)
    return [p.cpu().numpy() for p in [vol.dsum, vol.wsum] + vol.csum]


def check_integrate(dev, name):
    want = integrate_reference(name)
    dsum, wsum = want[0].reshape(DIMS[::-1]), want[1].reshape(DIMS[::-1])              # indexed [k, j, i]
    # what the case is there for, on the oracle alone
    assert 0 < (wsum > 0).sum() < wsum.size or name == "sdf_at_trunc"
    if name == "no_rgb":
        assert not any(p.any() for p in want[2:])
    elif name not in ("sdf_at_trunc",):
        assert want[2].any()
    if name == "image_border":
        one = integrate_reference_single("image_border", 0)
        assert one[0, :6, 0].all() and not one[0, :, 8].any() and not one[0, 6, :].any() and one[0, :6, :8].all()
    if name == "sdf_at_trunc":
        assert (dsum[0, :6, :8] == 1).all() and (dsum[1, :6, :8] == 0).all() and (wsum[1, :6, :8] == 1).all()
        k2 = wsum[2] == 1
        assert k2.any() and (dsum[2][k2] == -1).all() and not wsum[3:].any()
    if name == "behind_and_zc_zero":
        one = integrate_reference_single(name, 1)
        assert not one[:3].any() and one[3:].any()
    if name == "camera_1e30":
        assert not integrate_reference_single(name, 0).any() and not integrate_reference_single(name, 2).any()
    got = run_integrate(dev, name)
    differ = [int((bits(g) != bits(w)).sum()) for g, w in zip(got, want)]
    print(f"{name}: values that differ per plane {differ}, observed voxels {int((want[1] > 0).sum())} of {want[1].size}")
    assert differ == [0] * 5
    again = run_integrate(dev, name)
    assert all(same_bits(a, g) for a, g in zip(again, got))                            # two runs: the same bits


def integrate_reference_single(name, view):
    """wsum [k, j, i] of one view of a case alone"""
    depth, cams, rgb, trunc, grid = _views(name)
    s = O.integrate(O.new_state(DIMS), depth[view:view + 1], cams[view:view + 1], None, trunc, grid, DIMS)
    return s["wsum"].reshape(DIMS[::-1])


def check_chunking(dev):
    whole = run_integrate(dev, "views_17")
    for splits in ([9, 8], [1, 16]):
        parts = run_integrate(dev, "views_17", splits)
        assert all(same_bits(a, b) for a, b in zip(parts, whole)), splits
    assert all(same_bits(a, b) for a, b in zip(whole, integrate_reference("views_17")))


# ---- extraction -------------------------------------------------------------------------------------------------------------
def voxel_centres(dims, grid):
    """(gz, gy, gx, 3) world positions, computed as the kernels do"""
    gx, gy, gz = dims
    ox, oy, oz, h = grid
    x = ox + (np.arange(gx, dtype=np.float64) + 0.5) * h
    y = oy + (np.arange(gy, dtype=np.float64) + 0.5) * h
    z = oz + (np.arange(gz, dtype=np.float64) + 0.5) * h
    return np.stack(np.broadcast_arrays(x[None, None, :], y[None, :, None], z[:, None, None]), -1)


def sphere_field(dims, grid, centre, radius):
    return np.linalg.norm(voxel_centres(dims, grid) - np.asarray(centre, np.float64), axis=-1) - radius


UNIT = (0.0, 0.0, 0.0, 1.0)
TENTH = (-0.35, 0.2, 1.0, 0.1)                                   # an edge that is not representable, an origin off the lattice
SPHERES = {                                                       # name -> (dims, grid, centre, radius): closed surfaces
    "sphere_12": ((12, 12, 12), TENTH, (-0.35 + 0.57, 0.2 + 0.62, 1.0 + 0.64), 0.43),
    "sphere_13_zero_corners": ((13, 13, 13), UNIT, (6.5, 6.5, 6.5), 3.0),
    "sphere_13x13x14": ((13, 13, 14), UNIT, (6.3, 6.6, 7.1), 4.0),
}


def _field(name):
    """-> dims, grid, field [k, j, i] fp64, weights [k, j, i] fp32, min_weight"""
    if name in SPHERES:
        dims, grid, c, r = SPHERES[name]
        f = sphere_field(dims, grid, c, r)
        w = np.ones(f.shape, np.float32) if name == "sphere_13_zero_corners" else (1 + (np.arange(f.size) % 3)).reshape(f.shape).astype(np.float32)
        return dims, grid, f, w, 1
    if name == "plane_through_centres":                          # exactly 0 on the voxel centres i = 4: outside, zero-area triangles
        dims = DIMS
        f = voxel_centres(dims, UNIT)[..., 0] - 4.5
        return dims, UNIT, f, np.ones(f.shape, np.float32), 1
    if name == "negative_zero_is_outside":                       # the same plane from the other side: the centres i = 4 hold -0.0
        dims = DIMS
        f = -(voxel_centres(dims, UNIT)[..., 0] - 4.5)
        return dims, UNIT, f, np.full(f.shape, 2.0, np.float32), 1
    if name == "two_sheets":
        dims = (8, 7, 12)
        f = np.abs(voxel_centres(dims, UNIT)[..., 2] - 6.2) - 2.1
        return dims, UNIT, f, np.full(f.shape, 2.0, np.float32), 1
    if name in ("hole", "min_weight_1", "min_weight_2"):
        dims, grid, c, r = SPHERES["sphere_12"]
        f = sphere_field(dims, grid, c, r)
        w = np.ones(f.shape, np.float32)
        if name == "hole":
            w[4:8, 5:7, :] = 0.0                                  # a tunnel of unobserved voxels through the sphere
            return dims, grid, f, w, 1
        w[:, :, 6:] = 2.0                                         # at min_weight 2 half of the volume is unobserved
        return dims, grid, f, w, int(name[-1])
    if name.startswith("side_of_1"):
        dims = {"x": (1, 9, 9), "y": (9, 1, 9), "z": (9, 9, 1)}[name[-1]]
        f = sphere_field(dims, UNIT, (0.4 * dims[0], 0.45 * dims[1], 0.5 * dims[2]), 3.0)
        return dims, UNIT, f, np.ones(f.shape, np.float32), 1
    if name in ("all_outside", "all_inside"):
        f = np.full(DIMS[::-1], 0.25 if name == "all_outside" else -0.25)
        return DIMS, UNIT, f, np.full(f.shape, 3.0, np.float32), 1
    raise KeyError(name)


EXTRACT = tuple(SPHERES) + ("plane_through_centres", "negative_zero_is_outside", "two_sheets", "hole", "min_weight_1", "min_weight_2", "side_of_1_x", "side_of_1_y",
                            "side_of_1_z", "all_outside", "all_inside")


def planes_for(name):
    """the planes a case loads: dsum = fp32(field * weight), wsum = weight, colour sums = an integer colour * weight"""
    dims, grid, f, w, min_weight = _field(name)
    rng = np.random.default_rng(len(name) + f.size)
    dsum = (f * w.astype(np.float64)).astype(np.float32).ravel()
    csum = [(rng.integers(0, 256, f.size).astype(np.float32) * w.ravel()) for _ in range(3)]
    return dims, grid, dsum, w.ravel().copy(), csum, min_weight


@functools.lru_cache(maxsize=None)
def extract_reference(name):
    dims, grid, dsum, wsum, csum, min_weight = planes_for(name)
    r = O.extract(dsum, wsum, csum, grid, dims, min_weight)
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


def load_volume(dev, dims, grid, dsum, wsum, csum):
    vol = TM.TsdfVolume(grid[:3], grid[3], dims, dev, colour=csum is not None)
    vol.dsum.copy_(torch.from_numpy(dsum))
    vol.wsum.copy_(torch.from_numpy(wsum))
    for c in range(3 if csum is not None else 0):
        vol.csum[c].copy_(torch.from_numpy(csum[c]))
    return vol


def compare_mesh(got, want, what):
    verts, faces, rgb = got
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    print(f"{what}: {len(v)} vertices (oracle {len(want['verts'])}), {len(f)} faces (oracle {len(want['faces'])})")
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32 and v.shape == want["verts"].shape and f.shape == want["faces"].shape
    assert same_bits(v, want["verts"]) and np.array_equal(f, want["faces"])
    if want["rgb"] is not None:
        assert rgb.dtype == torch.uint8 and np.array_equal(rgb.cpu().numpy(), want["rgb"])
    return v, f


def check_extract(dev, name):
    """vertices, colours and faces equal to the oracle in every bit and in order, the count kernel's arrays and totals equal, two
    runs identical; on the spheres every vertex within sqrt(3) h of the sphere (vertex and true crossing lie on the same grid
    edge, whose length is at most sqrt(3) h) -- measured maxima on the kernel's output: 0.0854 h, 0.1068 h and 0.0929 h -- and the surface closed, consistently
    oriented (every directed edge once, its reverse once), of Euler characteristic 2, every non-degenerate normal outward."""
    dims, grid, dsum, wsum, csum, min_weight = planes_for(name)
    want = extract_reference(name)
    nv, nf = len(want["verts"]), len(want["faces"])
    # what the case is there for, on the oracle alone
    if name.startswith("side_of_1") or name.startswith("all_"):
        assert nf == 0 and (name.startswith("side") or nv == 0)
    else:
        assert nf > 0
    if name == "sphere_13_zero_corners":
        assert int((dsum == 0).sum()) == 30
    if name == "plane_through_centres":
        assert (np.asarray(want["verts"])[:, 0] == 4.5).all()
    if name == "negative_zero_is_outside":
        assert int(np.signbit(dsum[dsum == 0]).sum()) == 35 and (np.asarray(want["verts"])[:, 0] == 4.5).all()
    if name == "sphere_13x13x14":
        assert dims[0] * dims[1] * dims[2] > TM.SCAN_TILE
    if name == "hole":
        assert nf < len(extract_reference("min_weight_1")["faces"])
    if name == "min_weight_2":
        assert 0 < nf < len(extract_reference("min_weight_1")["faces"])
    vol = load_volume(dev, dims, grid, dsum, wsum, csum)
    edge_mask, tri_count, vert_start, tri_start, totals = vol.count(min_weight)
    assert totals == (nv, nf)
    assert np.array_equal(edge_mask.cpu().numpy(), want["edge_mask"]) and np.array_equal(tri_count.cpu().numpy(), want["tri_count"])
    assert np.array_equal(vert_start.cpu().numpy(), want["vert_start"]) and np.array_equal(tri_start.cpu().numpy(), want["tri_start"])
    got = vol.extract(min_weight)
    v, f = compare_mesh(got, want, name)
    again = vol.extract(min_weight)
    assert all(torch.equal(a, b) for a, b in zip(again, got))
    if name in SPHERES:
        _, _, centre, radius = SPHERES[name]
        off = np.abs(np.linalg.norm(v.astype(np.float64) - np.asarray(centre), axis=1) - radius).max() / grid[3]
        ok, euler = O.closed_and_oriented(f)
        outward, inward, degenerate = O.normals_outward(v, f, centre)
        print(f"{name}: max distance to the sphere {off:.4f} h, closed {ok}, Euler {euler}, normals {outward} out / {inward} in / {degenerate} degenerate")
        assert off <= np.sqrt(3.0)
        assert ok and euler == 2 and inward == 0 and outward + degenerate == len(f)
        assert (degenerate > 0) == (name == "sphere_13_zero_corners")
    # without colour planes: the same vertices and faces, no colours
    plain = load_volume(dev, dims, grid, dsum, wsum, None).extract(min_weight)
    assert plain[2] is None and torch.equal(plain[0], got[0]) and torch.equal(plain[1], got[1])


def check_scan_top_level(dev):
    """162^3 = 4 251 528 voxels: 2 076 tiles of 2 048, so the middle level of the scan has two blocks and the top level two entries"""
    dims, grid = (162, 162, 162), (-1.0, 0.5, 2.0, 0.025)
    assert dims[0] ** 3 > TM.SCAN_TILE ** 2
    centre, radius = (-1.0 + 81.3 * 0.025, 0.5 + 80.6 * 0.025, 2.0 + 81.1 * 0.025), 70.2 * 0.025
    f = sphere_field(dims, grid, centre, radius)
    dsum, wsum = f.astype(np.float32).ravel(), np.ones(f.size, np.float32)
    want = O.extract(dsum, wsum, None, grid, dims, 1, sparse=True)
    vol = load_volume(dev, dims, grid, dsum, wsum, None)
    edge_mask, tri_count, vert_start, tri_start, totals = vol.count(1)
    assert totals == (len(want["verts"]), len(want["faces"])) and totals[1] > 100000
    vs, ts = vert_start.cpu().numpy(), tri_start.cpu().numpy()
    assert vs[-1] == want["vert_start"][-1] == totals[0] and ts[-1] == want["tri_start"][-1] == totals[1]
    assert np.array_equal(vs, want["vert_start"]) and np.array_equal(ts, want["tri_start"])
    v, fc = compare_mesh(vol.extract(1), want, "162^3 sphere")
    ok, euler = O.closed_and_oriented(fc)
    assert ok and euler == 2


# ---- end to end -------------------------------------------------------------------------------------------------------------
def write_scan(tmp_path, name="scan1"):
    s = synthetic.fusion_scan(V=5, H=48, W=64)
    pair_folder, out_folder = str(tmp_path / "data" / name), str(tmp_path / "out" / name)
    synthetic.write_fusion_scan(s, pair_folder, out_folder)
    return pair_folder, out_folder


def oracle_mesh_of(views, summary):
    """the oracle's mesh of the filtered depth maps mesh_scan integrated, in the grid its summary reports"""
    grid = list(summary["origin"]) + [summary["voxel"]]
    state = O.integrate(O.new_state(summary["dims"]), views["depth"].cpu().numpy(), views["cams"], views["rgb"].cpu().numpy(), summary["trunc"], grid,
                        summary["dims"])
    r = O.extract(state["dsum"], state["wsum"], state["csum"], grid, summary["dims"], summary["min_weight"])
    return r, state


def check_end_to_end(dev, tmp_path):
    pair_folder, out_folder = write_scan(tmp_path)
    ply = str(tmp_path / "out" / "scan1_mesh.ply")
    summary = TM.mesh_scan(pair_folder, out_folder, out_folder, ply, PROB, NCONS, DIST, DEPTH, resolution=48, device=dev)
    views = TM.filtered_views(pair_folder, out_folder, out_folder, PROB, NCONS, DIST, DEPTH, device=dev)
    want, state = oracle_mesh_of(views, summary)
    verts, faces = dtu_io.read_ply_mesh(ply)
    print("end to end:", {k: v for k, v in summary.items() if k != "mesh"})
    assert max(summary["dims"]) in (54, 55) and summary["views"] == 5 and summary["faces"] > 1000      # 48 voxels + 2 x 3 of padding
    assert same_bits(verts, want["verts"]) and np.array_equal(faces, want["faces"])
    assert summary["vertices"] == len(verts) and summary["faces"] == len(faces)
    assert summary["unreferenced_vertices"] == len(verts) - len(np.unique(faces))
    assert summary["observed_voxels"] == want["observed"]
    with open(ply, "rb") as f:
        assert f.read() == TM.mesh_ply_bytes(want["verts"], want["faces"], want["rgb"])            # the colours too
    # the existing mesh super-sampling accepts it
    cloud = dtu_eval.sample_mesh(torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev), 0.5 * summary["voxel"])
    assert cloud.shape[0] > len(verts) and bool(torch.isfinite(cloud).all())
    return summary, verts, faces
