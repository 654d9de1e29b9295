"""TSDF fusion and marching tetrahedra, oracle and host code only (no kernel runs here): the header's 16-case table against the
parity rule, the oracle's own topology and chunk invariance, the PLY writer against dtu_io.read_ply_mesh, the grid planning, and
the geometric quality of the mesh of the synthetic fusion scan."""
import os
import re

import numpy as np
import pytest

import tsdf_cases as C
import tsdf_oracle as O
from oracle import fusion as OF
from rc_mvsnet_amd import _lib, dtu_io, synthetic, tsdf_mesh as TM

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rc_mvsnet_amd", "csrc", "tsdf_mesh_math.h")


def test_header_tables_equal_the_parity_rule():
    text = re.sub(r"//[^\n]*", "", open(HEADER).read())
    T = re.search(r"T\[6\]\[4\]\s*=\s*\{(.*?)\};", text, re.S).group(1)
    assert tuple(tuple(int(x) for x in row.split(",")) for row in re.findall(r"\{([^{}]*)\}", T)) == O.TETS
    S = re.search(r"S\[6\]\s*=\s*\{([^{}]*)\};", text).group(1)
    assert tuple(int(x) for x in S.split(",")) == O.tet_signs()
    body = re.search(r"C\[16\]\s*=\s*\{(.*?)\n\s*\};", text, re.S).group(1)
    rows = re.findall(r"\{\s*(\d+)\s*,\s*\{([^{}]*)\}\s*\}", body)
    assert len(rows) == 16
    want = O.case_table()
    for m, (n, edges) in enumerate(rows):
        e = [int(x) for x in edges.split(",")]
        got = [[(e[3 * k + c] >> 2, e[3 * k + c] & 3) for c in range(3)] for k in range(int(n))]
        assert got == [[tuple(edge) for edge in tri] for tri in want[m]], m
        assert len(e) == 6 and not any(e[3 * int(n):])
    # the rule's own consistency: complementary cases are the same triangles turned round
    for m in range(1, 15):
        assert {e for t in want[m] for e in t} == {e for t in want[15 - m] for e in t}
        assert len(want[m]) == (2 if bin(m).count("1") == 2 else 1)
    assert _lib.CONSTANTS["RCMVS_TSDF_MAX_VOXELS"] == 1 << 28 and _lib.CONSTANTS["RCMVS_TSDF_MAX_VIEWS"] == O.MAX_VIEWS
    assert _lib.CONSTANTS["RCMVS_VERSION"] == 106
    for name in ("integrate", "mesh_count", "mesh_emit"):
        assert "rcmvs_tsdf_" + name in _lib.EXT_SIGNATURES and "rcmvs_tsdf_" + name + "_timed" in _lib.EXT_SIGNATURES


@pytest.mark.parametrize("name", list(C.SPHERES))
def test_oracle_spheres_are_closed_and_oriented(name):
    dims, grid, centre, radius = C.SPHERES[name]
    r = C.extract_reference(name)
    ok, euler = O.closed_and_oriented(r["faces"])
    outward, inward, degenerate = O.normals_outward(r["verts"], r["faces"], centre)
    off = np.abs(np.linalg.norm(r["verts"].astype(np.float64) - np.asarray(centre), axis=1) - radius).max() / grid[3]
    assert ok and euler == 2 and inward == 0 and outward + degenerate == len(r["faces"])
    assert off <= np.sqrt(3.0)
    # the sparse walk over the cubes with mixed signs gives the same mesh
    _, _, dsum, wsum, csum, mw = C.planes_for(name)
    s = O.extract(dsum, wsum, csum, grid, dims, mw, sparse=True)
    assert all(np.array_equal(s[k], r[k]) for k in ("verts", "faces", "rgb", "tri_start", "vert_start"))


def test_oracle_integration_is_chunk_invariant():
    depth, cams, rgb, trunc, grid = C._views("views_17")
    whole = C.integrate_reference("views_17")
    for splits in ([9, 8], [1, 16], [1] * 17):
        state, lo = O.new_state(C.DIMS), 0
        for n in splits:
            O.integrate(state, depth[lo:lo + n], cams[lo:lo + n], rgb[lo:lo + n], trunc, grid, C.DIMS)
            lo += n
        assert all(C.same_bits(a, b) for a, b in zip(C.planes_of(state), whole))


def test_ply_round_trip(tmp_path):
    r = C.extract_reference("sphere_12")
    for rgb in (r["rgb"], None):
        path = str(tmp_path / "m.ply")
        data = TM.mesh_ply_bytes(r["verts"], r["faces"], rgb)
        with open(path, "wb") as f:
            f.write(data)
        verts, faces = dtu_io.read_ply_mesh(path)
        assert C.same_bits(verts, r["verts"]) and np.array_equal(faces, r["faces"]) and faces.dtype == np.int32
        head = data[:data.index(b"end_header\n")].decode("ascii").split("\n")
        assert head[:2] == ["ply", "format binary_little_endian 1.0"] and "property list uchar int vertex_indices" in head
        assert [h.split()[-1] for h in head if h.startswith("property") and "list" not in h] == ["x", "y", "z", "red", "green", "blue"]
        assert len(data) == data.index(b"end_header\n") + 11 + 15 * len(verts) + 13 * len(faces)
        colours = np.frombuffer(data, np.uint8, 15 * len(verts), data.index(b"end_header\n") + 11).reshape(-1, 15)[:, 12:]
        assert np.array_equal(colours, r["rgb"]) if rgb is not None else (colours == 255).all()
    empty = str(tmp_path / "empty.ply")
    with open(empty, "wb") as f:
        f.write(TM.mesh_ply_bytes(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), None))
    verts, faces = dtu_io.read_ply_mesh(empty)
    assert verts.shape == (0, 3) and faces.shape == (0, 3)


def test_plan_grid():
    origin, voxel, dims, trunc = TM.plan_grid([0.0, 1.0, 2.0], [48.0, 25.0, 14.0], resolution=48)
    assert voxel == 1.0 and trunc == 3.0 and origin == [-3.0, -2.0, -1.0] and dims == [54, 30, 18]
    origin, voxel, dims, trunc = TM.plan_grid([0.0, 1.0, 2.0], [48.0, 25.0, 14.0], voxel=0.5, trunc_voxels=2.0, pad=False)
    assert origin == [0.0, 1.0, 2.0] and dims == [96, 48, 24] and trunc == 1.0
    for bad in (dict(lo=[0, 0, 0], hi=[1, 1, float("nan")]), dict(lo=[0, 0, 0], hi=[1, -1, 1]), dict(lo=[0, 0, 0], hi=[0, 0, 0]),
                dict(lo=[0, 0, 0], hi=[1, 1, 1], voxel=0.0), dict(lo=[0, 0, 0], hi=[1, 1, 1], voxel=1e-4)):
        with pytest.raises(_lib.RcmvsError):
            TM.plan_grid(**bad)
    with pytest.raises(_lib.RcmvsError, match="dims"):
        TM.TsdfVolume((0, 0, 0), 1.0, (1 << 10, 1 << 10, 1 << 9), "cpu")


def test_geometric_quality_of_the_synthetic_scan_mesh():
    """The scan of synthetic.fusion_scan(V=5, H=48, W=64) filtered by the fusion oracle, integrated and meshed by the TSDF oracle
    at resolution 48 (the grid mesh_scan plans): the median |z - synthetic._surface(x, y)| over the vertices, the depth noise being
    0.25 and the voxel 6.125.  Measured: 0.2382 (5 897 vertices, 10 086 faces, 54 x 43 x 20 voxels).  The bound is twice that: the seeded input is
    deterministic, so the margin covers libm differences only.  The GPU's mesh equals the oracle's in every bit
    (tests/test_gpu_tsdf_mesh.py), so the check is not repeated there."""
    s = synthetic.fusion_scan(V=5, H=48, W=64)
    depth, rgb, cams, pts = [], [], [], []
    for ref, srcs in s["pairs"]:
        r = OF.fuse_view(s["depth"][ref], s["conf"][ref], s["img"][ref].astype(np.float32) / 255.0, s["K"][ref], s["E"][ref],
                         [s["depth"][v] for v in srcs], [s["K"][v] for v in srcs], [s["E"][v] for v in srcs], C.PROB, C.NCONS, C.DIST, C.DEPTH)
        depth.append(np.where(r["final"], r["depth_avg"], 0.0).astype(np.float32))
        rgb.append(s["img"][ref])
        cams.append(TM.camera_row(s["K"][ref], s["E"][ref]))
        pts.append(r["xyz"].astype(np.float64))
    pts = np.concatenate(pts)
    origin, voxel, dims, trunc = TM.plan_grid(pts.min(0), pts.max(0), resolution=48)
    grid = origin + [voxel]
    state = O.integrate(O.new_state(dims), np.stack(depth), np.stack(cams), np.stack(rgb), trunc, grid, dims)
    r = O.extract(state["dsum"], state["wsum"], state["csum"], grid, dims, 1)
    v = r["verts"].astype(np.float64)
    err = float(np.median(np.abs(v[:, 2] - synthetic._surface(v[:, 0], v[:, 1]))))
    print(f"median |z - surface| = {err:.4f}, voxel {voxel:.3f}, {len(v)} vertices, {len(r['faces'])} faces, dims {dims}")
    assert len(r["faces"]) > 1000 and max(dims) in (54, 55)
    assert err < 2 * 0.2382
