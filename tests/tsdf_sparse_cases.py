"""The cases and checks of the block-sparse TSDF volume (csrc/tsdf_sparse.hip through rc_mvsnet_amd/tsdf_mesh.py), shared by
tests/test_gpu_tsdf_sparse.py (device "cuda:0") and tests/test_tsdf_sparse_emu_cpu.py (the CPU emulation, device "cpu"), against
tests/tsdf_sparse_oracle.py, which is tests/tsdf_oracle.py read through the block table.  Every comparison is exact: flags,
ranks, planes, vertices, colours and faces equal in every bit and in order, two runs identical; where a sparse mesh is compared
with a dense one only the order is free (multisets of vertex records and of faces written as vertex records)."""
import functools

import numpy as np
import torch

import tsdf_cases as C
import tsdf_oracle as O
import tsdf_sparse_oracle as S
from rc_mvsnet_amd import _lib, dtu_eval, dtu_io, synthetic, tsdf_mesh as TM

GUARD, SENTINEL = 256, 0xAB


def block_numbers(bdims, blocks):
    return np.array(sorted(X + bdims[0] * (Y + bdims[1] * Z) for X, Y, Z in blocks), np.int32)


# ---- marking ----------------------------------------------------------------------------------------------------------------
MARK_BDIMS = (5, 4, 4)                                             # 40 x 32 x 32 voxels, 80 blocks: three mask words
LOOK_X = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])        # camera z = world x, camera x = world y, camera y = world z


def looking_z(centre, dist, f, H, W, scale=1.0, tilt=(0.0, 0.0)):
    """a camera `dist` in front of `centre` (world units) looking along +z, the principal point in the middle of the image"""
    R = C.rot(*tilt)
    Cw = np.asarray(centre, np.float64) + scale * np.array([0.0, 0.0, -dist])
    return C.cam_row(R, -R @ Cw, f, f, (W - 1) / 2.0, (H - 1) / 2.0)


def _mark_case(name):
    """-> depth (n,H,W) fp32, cams (n,16), trunc, grid, and per view what the oracle's ranges must show (checked in check_mark)"""
    grid, trunc, rng = (0.0, 0.0, 0.0, 1.0), 2.0, np.random.default_rng(sum(name.encode()))
    centre = np.array([20.0, 16.0, 16.0])
    if name == "random_3_views":                                   # footprint 46 / 40 = 1.15 h; the images reach beyond the grid in x and y
        H, W = 40, 48
        cams = np.stack([looking_z(centre + rng.standard_normal(3), 46.0, 40.0, H, W, tilt=0.1 * rng.standard_normal(2)) for _ in range(3)])
        depth = 46.0 + 1.5 * rng.standard_normal((3, H, W))
    elif name == "bad_depths":
        H, W = 6, 8
        cams = looking_z(centre, 46.0, 9.0, H, W)[None]
        depth = 46.0 + rng.standard_normal((1, H, W))
        depth[0].ravel()[[1, 9, 17, 25, 33]] = [0.0, -46.0, np.nan, np.inf, -np.inf]
    elif name == "z0_clamped":                                     # a camera inside the grid, depth below trunc: the slab starts at the camera
        H, W = 6, 8
        cams = C.cam_row(np.eye(3), -centre, 9.0, 9.0, 3.5, 2.5)[None]
        depth = np.full((1, H, W), 1.25)
    elif name == "camera_1e30":                                    # the pixel of the principal point reaches from -1e30 / 2 f to 1e30 / 2 f: skipped, counted
        H, W = 6, 8
        far = float(np.float32(1e30))
        cams = np.stack([looking_z(centre, 46.0, 9.0, H, W), C.cam_row(np.eye(3), (0.0, 0.0, far), 8.0, 8.0, 3.0, 2.0)])
        depth = np.stack([46.0 + rng.standard_normal((H, W)), np.full((H, W), far)])
    elif name == "focal_1e-308":                                   # (a - cx) / fx overflows: not finite, skipped and counted
        H, W = 6, 8
        cams = np.stack([looking_z(centre, 46.0, 9.0, H, W), looking_z(centre, 46.0, 1e-308, H, W)])
        depth = 46.0 + rng.standard_normal((2, H, W))
    elif name == "outside":                                        # the surface lies 30 in front of the grid: nothing marked, nothing counted
        H, W = 6, 8
        cams = looking_z(centre, 46.0, 9.0, H, W)[None]
        depth = np.full((1, H, W), 12.0)
    elif name == "grid_faces":                                     # the surface on the lower z face (left half) and on the upper one
        H, W = 12, 16
        cams = looking_z(centre, 46.0, 12.0, H, W)[None]
        depth = np.full((1, H, W), 30.25)
        depth[0, :, W // 2:] = 61.75
    elif name in ("span_4", "span_5"):                             # looking along +x from x = -30: the slab is 50 -+ trunc -+ h in world x
        H, W = 6, 8
        Cw = np.array([-30.0, 16.0, 16.0])
        cams = C.cam_row(LOOK_X, -LOOK_X @ Cw, 40.0, 40.0, 3.5, 2.5)[None]
        depth = np.full((1, H, W), 50.0)
        trunc = 11.0 if name == "span_4" else 14.5                 # x from 8 to 32: blocks 1..4; from 4.5 to 35.5: blocks 0..4
    elif name == "h_0.1":
        H, W = 24, 32
        grid, trunc = (0.3, -0.2, 0.1, 0.1), 0.15
        c = np.array(grid[:3]) + 0.1 * centre
        cams = np.stack([looking_z(c + 0.1 * rng.standard_normal(3), 46.0, 36.0, H, W, scale=0.1, tilt=0.1 * rng.standard_normal(2)) for _ in range(2)])
        depth = 0.1 * (46.0 + 1.5 * rng.standard_normal((2, H, W)))
    else:
        raise KeyError(name)
    return depth.astype(np.float32), cams, trunc, grid


MARK = ("random_3_views", "bad_depths", "z0_clamped", "camera_1e30", "focal_1e-308", "outside", "grid_faces", "span_4", "span_5", "h_0.1")


@functools.lru_cache(maxsize=None)
def mark_reference(name):
    depth, cams, trunc, grid = _mark_case(name)
    flags, skipped = S.mark(depth, cams, trunc, grid, MARK_BDIMS)
    flags.setflags(write=False)
    return flags, skipped


def guarded_flags(vol):
    """vol.flags becomes a window of a larger tensor filled with a sentinel -> that tensor"""
    big = torch.full((GUARD + vol.blocks + GUARD,), SENTINEL, dtype=torch.uint8, device=vol.device)
    big[GUARD:GUARD + vol.blocks] = 0
    vol.flags = big[GUARD:GUARD + vol.blocks]
    return big


def check_mark(dev, name):
    depth, cams, trunc, grid = _mark_case(name)
    want, skipped = mark_reference(name)
    # what the case is there for, on the oracle alone
    r = [S.mark_ranges(depth[v], cams[v], trunc, grid, MARK_BDIMS) for v in range(len(depth))]
    usable = [x["ok"] & x["finite"] & x["inside"] & ~x["long"] for x in r]
    H, W = depth.shape[1:]
    if name == "random_3_views":
        assert 0 < want.sum() < want.size and skipped == 0 and any((x["ok"] & x["finite"] & ~x["inside"]).any() for x in r)
    if name == "bad_depths":
        assert int((~r[0]["ok"]).sum()) == 5 and skipped == 0 and usable[0].sum() == H * W - 5
    if name == "z0_clamped":
        assert (r[0]["z0"] == 0).all() and usable[0].all() and want.sum() > 0
    if name == "camera_1e30":
        assert int((r[1]["ok"] & r[1]["finite"] & r[1]["inside"] & r[1]["long"]).sum()) == 1 == skipped and not usable[1].any() and not r[1]["inside"].sum() > 1
        assert np.array_equal(want, S.mark(depth[:1], cams[:1], trunc, grid, MARK_BDIMS)[0])
    if name == "focal_1e-308":
        assert not r[1]["finite"].any() and skipped == H * W and usable[0].all()
    if name == "outside":
        assert r[0]["ok"].all() and r[0]["finite"].all() and not r[0]["inside"].any() and skipped == 0 and not want.any()
    if name == "grid_faces":
        fl, fh = r[0]["fl"][..., 2], r[0]["fh"][..., 2]
        assert ((fl < 0) & (fh >= 0) & usable[0]).any() and ((fh > MARK_BDIMS[2] - 1) & (fl <= MARK_BDIMS[2] - 1) & usable[0]).any() and skipped == 0
    if name == "span_4":
        assert (r[0]["cl"][..., 0] == 1).all() and (r[0]["ch"][..., 0] == 4).all() and usable[0].all() and skipped == 0
    if name == "span_5":
        assert (r[0]["cl"][..., 0] == 0).all() and (r[0]["ch"][..., 0] == 4).all() and r[0]["long"].all() and skipped == H * W and not want.any()
    if name == "h_0.1":
        assert 0 < want.sum() < want.size and skipped == 0
    runs = []
    for _ in range(2):
        vol = TM.SparseTsdfVolume(grid[:3], grid[3], MARK_BDIMS, dev)
        big = guarded_flags(vol)
        d = torch.from_numpy(depth).to(dev)
        vol.mark(d[:1], cams[:1], trunc)                            # repeated calls accumulate
        if len(depth) > 1:
            vol.mark(d[1:], cams[1:], trunc)
        got, guard = vol.flags.cpu().numpy(), big.cpu().numpy()
        assert (guard[:GUARD] == SENTINEL).all() and (guard[GUARD + vol.blocks:] == SENTINEL).all()      # nothing written outside the flags
        runs.append((got, int(vol._skipped.cpu()[0])))
    print(f"{name}: {int(want.sum())} of {want.size} blocks marked, {skipped} pixels skipped; kernel {int(runs[0][0].sum())}, {runs[0][1]}")
    assert np.array_equal(runs[0][0], want) and runs[0][1] == skipped
    assert np.array_equal(runs[1][0], runs[0][0]) and runs[1][1] == runs[0][1]


# ---- build ------------------------------------------------------------------------------------------------------------------
BUILD = {"all_80": (MARK_BDIMS, range(80)), "one": (MARK_BDIMS, [37]), "word_boundary": (MARK_BDIMS, [31, 32]), "last_block": (MARK_BDIMS, [0, 63, 64, 79]),
         "33x1x1": ((33, 1, 1), [0, 5, 31, 32]), "33x1x1_all": ((33, 1, 1), range(33))}


def check_build(dev, name):
    bdims, blocks = BUILD[name]
    flags = np.zeros(bdims[0] * bdims[1] * bdims[2], np.uint8)
    flags[list(blocks)] = 1
    mask_words, word_rank, active = S.build(flags)
    assert len(mask_words) == (3 if bdims == MARK_BDIMS else 2)
    vol = TM.SparseTsdfVolume((0.0, 0.0, 0.0), 1.0, bdims, dev, colour=False)
    vol.flags.copy_(torch.from_numpy(flags))
    assert vol.build() == len(active) == vol.n_active and vol.skipped == 0
    got = vol.active.cpu().numpy()
    assert np.array_equal(got, np.nonzero(flags)[0]) and (np.diff(got) > 0).all() and np.array_equal(got, active)
    assert np.array_equal(vol.mask_words.cpu().numpy().view(np.uint32), mask_words)
    assert np.array_equal(vol.word_rank.cpu().numpy().view(np.uint32), word_rank)
    assert vol.dsum.shape == (512 * len(active),) and vol.csum is None and not bool(vol.dsum.any())


def check_call_order(dev):
    vol = TM.SparseTsdfVolume((0.0, 0.0, 0.0), 1.0, MARK_BDIMS, dev)
    depth, cams, trunc, grid = _mark_case("bad_depths")
    d = torch.from_numpy(depth).to(dev)
    for call in (lambda: vol.integrate(d, cams, None, trunc=trunc), lambda: vol.count(), lambda: vol.extract()):
        try:
            call()
        except _lib.RcmvsError as e:
            assert "build() first" in str(e)
        else:
            raise AssertionError("accepted before build()")
    try:
        vol.build()                                                  # no block flagged
    except _lib.RcmvsError as e:
        assert "0 active blocks" in str(e)
    else:
        raise AssertionError("an empty block set was accepted")
    vol.mark(d, cams, trunc)
    assert vol.build() > 0
    for call in (lambda: vol.mark(d, cams, trunc), vol.build):
        try:
            call()
        except _lib.RcmvsError as e:
            assert "fixed by build()" in str(e)
        else:
            raise AssertionError("accepted after build()")


# ---- integration: the dense suite's views on a grid of whole blocks -------------------------------------------------------
# tsdf_cases' grid is 9 x 7 x 5 voxels of h; here the same box (and half a voxel more on the lower sides, a little more on the
# upper ones) is 40 x 32 x 24 voxels of h / 4, so every camera, depth map and truncation distance of the dense suite is used as it is.
INT_BDIMS = (5, 4, 3)
INT_ACTIVE = block_numbers(INT_BDIMS, [(0, 1, 1), (4, 2, 1), (2, 0, 1), (2, 3, 1), (1, 1, 0), (3, 2, 2),      # one at each face of the grid
                                        (4, 0, 0),                                                              # alone (and in a corner)
                                        (1, 1, 1), (2, 1, 1), (1, 2, 1), (2, 2, 1), (1, 1, 2), (2, 1, 2), (1, 2, 2), (2, 2, 2)])   # a full 2 x 2 x 2


def sparse_views(name):
    depth, cams, rgb, trunc, grid = C._views(name)
    h = grid[3]
    return depth, cams, rgb, trunc, (grid[0] - 0.5 * h, grid[1] - 0.5 * h, grid[2] - 0.5 * h, h / 4.0)


@functools.lru_cache(maxsize=None)
def integrate_reference(name):
    depth, cams, rgb, trunc, grid = sparse_views(name)
    planes, _ = S.integrate(INT_BDIMS, INT_ACTIVE, depth, cams, rgb, trunc, grid)
    for p in planes:
        p.setflags(write=False)
    return planes


def chosen_volume(dev, grid, bdims, active, colour=True):
    vol = TM.SparseTsdfVolume(grid[:3], grid[3], bdims, dev, colour=colour)
    vol.flags[torch.from_numpy(np.asarray(active, np.int64)).to(dev)] = 1
    assert vol.build() == len(active)
    return vol


def run_integrate(dev, name, splits=None):
    depth, cams, rgb, trunc, grid = sparse_views(name)
    vol = chosen_volume(dev, grid, INT_BDIMS, INT_ACTIVE)
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
    w = want[1].reshape(len(INT_ACTIVE), 512)
    # what the case is there for, on the oracle alone: seen and unseen voxels, and every kind of block takes part
    assert 0 < (w > 0).sum() < w.size
    if name not in ("sdf_at_trunc", "behind_and_zc_zero"):
        assert ((w > 0).any(1)).sum() >= 12
    assert bool(want[2].any()) == (name != "no_rgb")
    got = run_integrate(dev, name)
    differ = [int((C.bits(g) != C.bits(x)).sum()) for g, x in zip(got, want)]
    print(f"{name}: values that differ per plane {differ}, observed voxels {int((want[1] > 0).sum())} of {want[1].size}")
    assert differ == [0] * 5
    again = run_integrate(dev, name)
    assert all(C.same_bits(a, g) for a, g in zip(again, got))


def check_chunking(dev):
    whole = run_integrate(dev, "views_17")
    for splits in ([9, 8], [1, 16]):
        parts = run_integrate(dev, "views_17", splits)
        assert all(C.same_bits(a, b) for a, b in zip(parts, whole)), splits
    assert all(C.same_bits(a, b) for a, b in zip(whole, integrate_reference("views_17")))


def check_integrate_against_dense_kernel(dev, name):
    """dense kernel against sparse kernel, no oracle in between: every active block's planes are TsdfVolume's planes of the same voxels"""
    depth, cams, rgb, trunc, grid = sparse_views(name)
    dense = TM.TsdfVolume(grid[:3], grid[3], S.dims_of(INT_BDIMS), dev)
    dense.integrate(torch.from_numpy(depth).to(dev), cams, None if rgb is None else torch.from_numpy(rgb).to(dev), trunc=trunc)
    vox = torch.from_numpy(S.voxel_of_alloc(INT_BDIMS, INT_ACTIVE)).to(dev)
    got = run_integrate(dev, name)
    for g, p in zip(got, [dense.dsum, dense.wsum] + dense.csum):
        assert C.same_bits(g, p[vox].cpu().numpy())
    assert bool((dense.wsum[vox] > 0).any())


# ---- extraction from loaded planes ------------------------------------------------------------------------------------------
EIGHT = [(X, Y, Z) for Z in (0, 1) for Y in (0, 1) for X in (0, 1)]
ALL_222 = block_numbers((2, 2, 2), EIGHT)


def _field(name):
    """-> bdims, grid, active block numbers, field [k, j, i] fp64 over the grid of 8 * bdims, weights fp32, min_weight, centre or None"""
    if name in ("sphere_on_the_corner_of_8", "sphere_7_of_8", "min_weight_1", "min_weight_2"):
        bdims, grid = (3, 3, 3), C.TENTH                             # the eight blocks meet at voxel index 8 = world o + 0.8
        centre = (grid[0] + 0.8, grid[1] + 0.8, grid[2] + 0.8)
        active = block_numbers(bdims, EIGHT if name != "sphere_7_of_8" else [b for b in EIGHT if b != (1, 1, 1)])
        f = C.sphere_field(S.dims_of(bdims), grid, centre, 0.53)
        w = (1 + (np.arange(f.size) % 3)).reshape(f.shape).astype(np.float32)
        if name.startswith("min_weight"):
            w = np.ones(f.shape, np.float32)
            w[:, :, 8:] = 2.0
        return bdims, grid, active, f, w, int(name[-1]) if name.startswith("min_weight") else 1, centre
    if name == "sphere_cut_by_upper_faces":
        bdims = (2, 2, 2)
        f = C.sphere_field(S.dims_of(bdims), C.UNIT, (12.3, 11.6, 12.1), 6.2)
        return bdims, C.UNIT, ALL_222, f, np.ones(f.shape, np.float32), 1, None
    if name == "plane_on_a_block_face":                              # exactly 0 on the centres i = 8, the first voxels of the blocks X = 1
        bdims = (2, 2, 2)
        f = C.voxel_centres(S.dims_of(bdims), C.UNIT)[..., 0] - 8.5
        return bdims, C.UNIT, ALL_222, f, np.ones(f.shape, np.float32), 1, None
    if name in ("all_outside", "all_inside"):
        bdims = (2, 2, 2)
        f = np.full(S.dims_of(bdims)[::-1], 0.25 if name == "all_outside" else -0.25)
        return bdims, C.UNIT, ALL_222, f, np.full(f.shape, 3.0, np.float32), 1, None
    raise KeyError(name)


EXTRACT = ("sphere_on_the_corner_of_8", "sphere_7_of_8", "sphere_cut_by_upper_faces", "plane_on_a_block_face", "min_weight_1", "min_weight_2",
           "all_outside", "all_inside")


def planes_for(name):
    """-> bdims, grid, active, planes in allocated order [dsum, wsum, r, g, b], min_weight, centre"""
    bdims, grid, active, f, w, min_weight, centre = _field(name)
    rng = np.random.default_rng(len(name) + f.size)
    dsum = (f * w.astype(np.float64)).astype(np.float32).ravel()
    csum = [(rng.integers(0, 256, f.size).astype(np.float32) * w.ravel()) for _ in range(3)]
    vox = S.voxel_of_alloc(bdims, active)
    return bdims, grid, active, [dsum[vox], w.ravel()[vox]] + [c[vox] for c in csum], min_weight, centre


@functools.lru_cache(maxsize=None)
def extract_reference(name):
    bdims, grid, active, planes, min_weight, _ = planes_for(name)
    r = S.extract(S.scatter(planes, bdims, active), grid, bdims, active, min_weight)
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


def load_volume(dev, bdims, grid, active, planes, colour=True):
    vol = chosen_volume(dev, grid, bdims, active, colour)
    vol.dsum.copy_(torch.from_numpy(planes[0]))
    vol.wsum.copy_(torch.from_numpy(planes[1]))
    for c in range(3 if colour else 0):
        vol.csum[c].copy_(torch.from_numpy(planes[2 + c]))
    return vol


def check_extract(dev, name):
    bdims, grid, active, planes, min_weight, centre = planes_for(name)
    want = extract_reference(name)
    nv, nf = len(want["verts"]), len(want["faces"])
    # what the case is there for, on the oracle alone
    if name.startswith("all_"):
        assert nv == 0 and nf == 0
    else:
        assert nf > 0
    if name == "sphere_on_the_corner_of_8":                         # every one of the eight blocks owns faces, and faces use vertices of other blocks
        owners = (np.searchsorted(want["vert_start"], want["faces"], side="right") - 1) // 512
        cubes = (np.searchsorted(want["tri_start"], np.arange(nf), side="right") - 1) // 512
        assert len(np.unique(cubes)) == 8 and (owners != cubes[:, None]).any()
    if name == "sphere_7_of_8":
        full = extract_reference("sphere_on_the_corner_of_8")
        assert 0 < nf < len(full["faces"]) and not O.closed_and_oriented(want["faces"])[0]
    if name == "sphere_cut_by_upper_faces":
        assert not O.closed_and_oriented(want["faces"])[0]
    if name == "plane_on_a_block_face":
        assert (np.asarray(want["verts"])[:, 0] == 8.5).all() and O.normals_outward(want["verts"], want["faces"], (0, 8, 8))[2] > 0
    if name == "min_weight_2":
        assert 0 < nf < len(extract_reference("min_weight_1")["faces"])
    vol = load_volume(dev, bdims, grid, active, planes)
    edge_mask, tri_count, vert_start, tri_start, totals = vol.count(min_weight)
    assert totals == (nv, nf)
    assert np.array_equal(edge_mask.cpu().numpy(), want["edge_mask"]) and np.array_equal(tri_count.cpu().numpy(), want["tri_count"])
    assert np.array_equal(vert_start.cpu().numpy(), want["vert_start"]) and np.array_equal(tri_start.cpu().numpy(), want["tri_start"])
    got = vol.extract(min_weight)
    v, f = C.compare_mesh(got, want, name)
    again = vol.extract(min_weight)
    assert all(torch.equal(a, b) for a, b in zip(again, got))
    if name == "sphere_on_the_corner_of_8":
        ok, euler = O.closed_and_oriented(f)
        outward, inward, degenerate = O.normals_outward(v, f, centre)
        print(f"{name}: closed {ok}, Euler {euler}, normals {outward} out / {inward} in / {degenerate} degenerate")
        assert ok and euler == 2 and inward == 0 and outward + degenerate == len(f)
    plain = load_volume(dev, bdims, grid, active, planes, colour=False).extract(min_weight)       # without colour planes
    assert plain[2] is None and torch.equal(plain[0], got[0]) and torch.equal(plain[1], got[1])


def check_scan_top_level(dev):
    """21^3 = 9 261 active blocks: five tiles of 2 048 block sums, so the top level of the scan has five entries"""
    bdims, grid = (21, 21, 21), (-1.0, 0.5, 2.0, 0.025)
    active = np.arange(21 ** 3, dtype=np.int32)
    assert len(active) > 8192
    centre, radius = (-1.0 + 84.3 * 0.025, 0.5 + 83.6 * 0.025, 2.0 + 84.1 * 0.025), 72.2 * 0.025
    f = C.sphere_field(S.dims_of(bdims), grid, centre, radius)
    vox = S.voxel_of_alloc(bdims, active)
    planes = [f.astype(np.float32).ravel()[vox], np.ones(f.size, np.float32)]
    want = S.extract(S.scatter(planes, bdims, active, colour=False), grid, bdims, active, 1)
    vol = load_volume(dev, bdims, grid, active, planes, colour=False)
    edge_mask, tri_count, vert_start, tri_start, totals = vol.count(1)
    assert totals == (len(want["verts"]), len(want["faces"])) and totals[1] > 100000
    assert np.array_equal(vert_start.cpu().numpy(), want["vert_start"]) and np.array_equal(tri_start.cpu().numpy(), want["tri_start"])
    v, fc = C.compare_mesh(vol.extract(1), want, "21^3 blocks")
    ok, euler = O.closed_and_oriented(fc)
    assert ok and euler == 2


# ---- the theorem: with no skipped pixel the sparse mesh is the dense mesh ----------------------------------------------------
SCENES = {                                                           # name -> bdims, grid, cameras, trunc in voxels
    "5x4x4": ((5, 4, 4), (0.0, 0.0, 0.0, 1.0), 3, 1.5),
    "6x6x6_h_0.1": ((6, 6, 6), (0.3, -0.2, 0.1, 0.1), 4, 2.0),
    "8x8x8": ((8, 8, 8), (0.0, 0.0, 0.0, 1.0), 5, 3.0),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    """A noisy sphere in the middle of the grid seen by cameras on a ring round it, the pixel footprint about h at the surface
    -> depth (n,H,W) fp32 (0 off the sphere), cams, rgb, trunc, grid, bdims"""
    bdims, grid, n, trunc_voxels = SCENES[name]
    h = grid[3]
    rng = np.random.default_rng(len(name) + n)
    dims = np.array(S.dims_of(bdims), np.float64)
    centre = np.array(grid[:3]) + 0.5 * dims * h
    radius = 0.3 * dims.min() * h
    dist = 4.0 * radius
    f = 3.0 * radius / h                                             # footprint at the surface: (dist - radius) / f = h
    H = W = int(2 * (1.2 * radius / dist) * f) | 1
    cams, depth = [], []
    for v in range(n):
        a = 2 * np.pi * v / n + 0.3
        R = C.rot(0.2 * np.sin(a), a)
        Cw = centre - dist * R[2]                                    # the camera looks along its z axis, the third row of R
        cams.append(C.cam_row(R, -R @ Cw, f, f, (W - 1) / 2.0 + 0.2, (H - 1) / 2.0 - 0.3))
        jj, ii = np.mgrid[0:H, 0:W]
        ray = np.stack([(ii - cams[-1][14]) / f, (jj - cams[-1][15]) / f, np.ones((H, W))], -1)
        oc = R @ (Cw - centre)                                       # the centre of the sphere is at -oc in the camera frame
        A, B, Cq = (ray * ray).sum(-1), 2 * (ray * oc).sum(-1), (oc * oc).sum() - radius ** 2
        disc = B * B - 4 * A * Cq
        z = np.where(disc > 0, (-B - np.sqrt(np.maximum(disc, 0))) / (2 * A), 0.0)
        depth.append(np.where(z > 0, z + 0.3 * h * rng.standard_normal((H, W)), 0.0))
    rgb = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    depth = np.stack(depth).astype(np.float32)
    depth.setflags(write=False)
    return depth, np.stack(cams), rgb, trunc_voxels * h, grid, bdims


@functools.lru_cache(maxsize=None)
def scene_reference(name):
    """-> (flags, skipped, dense oracle's mesh (verts, faces, rgb), dense observed count)"""
    depth, cams, rgb, trunc, grid, bdims = scene(name)
    flags, skipped = S.mark(depth, cams, trunc, grid, bdims)
    dims = S.dims_of(bdims)
    state = O.integrate(O.new_state(dims), depth, cams, rgb, trunc, grid, dims)
    r = O.extract(state["dsum"], state["wsum"], state["csum"], grid, dims, 1, sparse=True)
    return flags, skipped, (r["verts"], r["faces"], r["rgb"]), r["observed"], state


def check_scene_on_the_oracles(name):
    depth, cams, rgb, trunc, grid, bdims = scene(name)
    flags, skipped, dense, observed, state = scene_reference(name)
    active = S.build(flags)[2]
    _, kept = S.restrict(state, bdims, active)
    sp = S.extract(kept, grid, bdims, active, 1)
    print(f"{name}: {len(active)} of {flags.size} blocks active, {skipped} skipped, observed dense {observed} sparse {sp['observed']}, "
          f"{len(dense[0])} vertex records, {len(dense[1])} faces")
    assert skipped == 0 and 0 < len(active) < flags.size and sp["observed"] <= observed and len(dense[1]) > 1000
    assert S.same_mesh_as_multisets((sp["verts"], sp["faces"], sp["rgb"]), dense)
    return sp


def check_scene_on_the_kernels(dev, name):
    depth, cams, rgb, trunc, grid, bdims = scene(name)
    flags, skipped, dense, _, _ = scene_reference(name)
    d, c = torch.from_numpy(np.array(depth)).to(dev), torch.from_numpy(rgb).to(dev)
    vol = TM.SparseTsdfVolume(grid[:3], grid[3], bdims, dev)
    vol.mark(d, cams, trunc)
    assert vol.build() == int(flags.sum()) and vol.skipped == 0 == skipped
    assert np.array_equal(vol.flags.cpu().numpy(), flags)
    vol.integrate(d, cams, c, trunc=trunc)
    got = [t.cpu().numpy() for t in vol.extract(1)]
    full = TM.TsdfVolume(grid[:3], grid[3], S.dims_of(bdims), dev)
    full.integrate(d, cams, c, trunc=trunc)
    want = [t.cpu().numpy() for t in full.extract(1)]
    print(f"{name}: {vol.n_active} of {vol.blocks} blocks, {len(got[0])} vertices, {len(got[1])} faces (dense kernel {len(want[0])}, {len(want[1])})")
    assert S.same_mesh_as_multisets((got[0], got[1], got[2]), (want[0], want[1], want[2]))
    assert S.same_mesh_as_multisets((got[0], got[1], got[2]), dense)


# ---- end to end -------------------------------------------------------------------------------------------------------------
def oracle_sparse_mesh_of(views, summary):
    """the sparse oracle's mesh of the filtered depth maps, in the grid the summary reports"""
    grid = list(summary["origin"]) + [summary["voxel"]]
    depth, rgb = views["depth"].cpu().numpy(), views["rgb"].cpu().numpy()
    flags, skipped = S.mark(depth, views["cams"], summary["trunc"], grid, summary["bdims"])
    active = S.build(flags)[2]
    _, kept = S.integrate(summary["bdims"], active, depth, views["cams"], rgb, summary["trunc"], grid)
    return S.extract(kept, grid, summary["bdims"], active, summary["min_weight"]), active, skipped


def check_summary(summary, want, active, skipped):
    assert summary["skipped_pixels"] == skipped == 0 and summary["active_blocks"] == len(active) and summary["allocated_voxels"] == 512 * len(active)
    assert summary["dims"] == S.dims_of(summary["bdims"]) and summary["vertices"] == len(want["verts"]) and summary["faces"] == len(want["faces"]) > 1000
    assert summary["observed_voxels"] == want["observed"]
    assert 0 < summary["active_blocks"] < summary["bdims"][0] * summary["bdims"][1] * summary["bdims"][2]


def check_end_to_end(dev, tmp_path):
    pair_folder, out_folder = C.write_scan(tmp_path)
    args = (PROB, NCONS, DIST, DEPTH) = (C.PROB, C.NCONS, C.DIST, C.DEPTH)
    views = TM.filtered_views(pair_folder, out_folder, out_folder, *args, device=dev)
    voxel = TM.plan_grid(views["lo"], views["hi"], resolution=48)[1]                     # the dense run's voxel
    ply = str(tmp_path / "out" / "scan1_sparse.ply")
    summary = TM.mesh_scan(pair_folder, out_folder, out_folder, ply, *args, voxel=voxel, device=dev, sparse=True)
    want, active, skipped = oracle_sparse_mesh_of(views, summary)
    print("end to end:", {k: v for k, v in summary.items() if k != "mesh"})
    check_summary(summary, want, active, skipped)
    with open(ply, "rb") as f:
        assert f.read() == TM.mesh_ply_bytes(want["verts"], want["faces"], want["rgb"])
    # the dense path on the same origin and dims: the same mesh in another order
    lo = np.array(summary["origin"])
    hi = lo + (np.array(summary["dims"]) - 0.5) * voxel                                  # ceil((hi - lo) / voxel) = dims whatever the rounding
    dense_ply = str(tmp_path / "out" / "scan1_dense.ply")
    dense = TM.mesh_scan(pair_folder, out_folder, out_folder, dense_ply, *args, voxel=voxel, bounds=list(lo) + list(hi), device=dev)
    assert dense["dims"] == summary["dims"] and dense["origin"] == summary["origin"] and dense["trunc"] == summary["trunc"]
    assert S.same_mesh_as_multisets(read_coloured_mesh(ply), read_coloured_mesh(dense_ply))
    verts, faces = dtu_io.read_ply_mesh(ply)
    cloud = dtu_eval.sample_mesh(torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev), 0.5 * summary["voxel"])
    assert cloud.shape[0] > len(verts) and bool(torch.isfinite(cloud).all())
    return summary


def read_coloured_mesh(path):
    """(verts, faces, rgb) of a PLY that mesh_ply_bytes wrote"""
    data = open(path, "rb").read()
    at = data.index(b"end_header\n") + 11
    verts, faces = dtu_io.read_ply_mesh(path)
    rgb = np.frombuffer(data, np.uint8, 15 * len(verts), at).reshape(-1, 15)[:, 12:]
    return verts, faces, rgb


TANKS = dict(pix=0.75, dth=0.01, photo=0.8, wh=(96, 64), orig_wh=(100, 75), ncons=3)


def check_tanks_end_to_end(dev, tmp_path):
    s = synthetic.tanks_fusion_scan(V=5, hw=(64, 96), orig_hw=(75, 100))
    scan_folder, out_folder = str(tmp_path / "tt" / "Horse"), str(tmp_path / "exp" / "Horse")
    synthetic.write_tanks_fusion_scan(s, scan_folder, out_folder)
    t = TANKS
    args = (t["pix"], t["dth"], t["photo"], t["wh"], t["orig_wh"], t["ncons"])
    ply = str(tmp_path / "ply" / "Horse_mesh.ply")
    summary = TM.mesh_scan_tanks(scan_folder, out_folder, ply, *args, 5, "Horse", device=dev, resolution=64)
    views = TM.filtered_views_tanks(scan_folder, out_folder, *args, device=dev)
    want, active, skipped = oracle_sparse_mesh_of(views, summary)
    print("tanks:", {k: v for k, v in summary.items() if k != "mesh"})
    check_summary(summary, want, active, skipped)
    with open(ply, "rb") as f:
        assert f.read() == TM.mesh_ply_bytes(want["verts"], want["faces"], want["rgb"])
