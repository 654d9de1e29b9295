"""Mesh simplification on the GPU (rc_mvsnet_amd/mesh_simplify.py, csrc/mesh_simplify.hip) against tests/mesh_simplify_oracle.py; the
cases are tests/mesh_simplify_cases.py's, which the CPU emulation runs too.  After every round the 1-ring, flags, keys, remap,
positions, quadrics, members, colour sums and the live count equal the oracle's in every bit; so do the final mesh and the stats;
two runs are identical; the known answers of the plane and the cube; the comparison with clustering; the command lines."""
import json
import os

import numpy as np
import pytest
import torch

import mesh_simplify_cases as MSC
from rc_mvsnet_amd import _lib, dtu_io, mesh_decimate as MD, mesh_simplify as MS, tsdf_mesh as TM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,k", [key for key in MSC.case_keys() if key[0] not in ("plane_17", "cube_9", "plane_9", "cube_5")])
def test_every_round_and_the_result_equal_the_oracle_and_two_runs_are_identical(name, k):
    MSC.check_case(DEV, name, k, twice=True)


@pytest.mark.parametrize("n", [9, 17])
def test_plane_known_answer(n):
    MSC.check_plane(DEV, n)


@pytest.mark.parametrize("n", [5, 9])
def test_cube_known_answer_and_clustering_misses_the_corners(n):
    MSC.check_cube(DEV, n)


def test_untouched_vertices_are_copies():
    MSC.check_untouched_vertices(DEV)


def test_refusals():
    MSC.check_refusals(DEV)


def test_cpu_tensors_are_refused():
    v, f = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    _lib.load()
    with pytest.raises(_lib.RcmvsError, match="GPU"):
        MS.simplify(v, f, ratio=0.5)
    with pytest.raises(_lib.RcmvsError, match="one device"):
        MS.simplify(v.to(DEV), f, ratio=0.5)


def _closest_on_triangle(p, a, b, c):
    """the point of the triangle a b c nearest to p (Ericson, Real-Time Collision Detection, 5.1.5)"""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = ab @ ap, ac @ ap
    if d1 <= 0 and d2 <= 0:
        return a
    bp = p - b
    d3, d4 = ab @ bp, ac @ bp
    if d3 >= 0 and d4 <= d3:
        return b
    vc = d1 * d4 - d3 * d2
    if vc <= 0 and d1 >= 0 and d3 <= 0:
        return a + ab * (d1 / (d1 - d3))
    cp = p - c
    d5, d6 = ab @ cp, ac @ cp
    if d6 >= 0 and d5 <= d6:
        return c
    vb = d5 * d2 - d1 * d6
    if vb <= 0 and d2 >= 0 and d6 <= 0:
        return a + ac * (d2 / (d2 - d6))
    va = d3 * d6 - d5 * d4
    if va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0:
        return b + (c - b) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))
    return a + ab * (vb / (va + vb + vc)) + ac * (vc / (va + vb + vc))


def _sphere_error(v, f, centre, radius):
    """-> (surface, vertices): the largest distance from a point of the mesh to the analytic sphere (the one-sided Hausdorff distance:
    | |p - centre| - radius | is largest at a vertex, or at the point of a face nearest to the centre, where the chord's sagitta is),
    and the same over the vertices alone"""
    p, centre = v.astype(np.float64), np.asarray(centre, np.float64)
    at_vertices = float(np.abs(np.linalg.norm(p - centre, axis=1) - radius).max())
    nearest = min(float(np.linalg.norm(_closest_on_triangle(centre, p[a], p[b], p[c]) - centre)) for a, b, c in f.tolist())
    return max(at_vertices, abs(nearest - radius)), at_vertices


def test_real_extraction_and_collapse_is_closer_to_the_sphere_than_clustering():
    """The extracted spheres and the speck at ratio 0.5 and 0.1 equal the oracle.  Then, on the large sphere alone (the clean-up's
    largest component): clustering at 2 and at 3 voxels (the cells of the clustering's own extraction test), and the collapse down to
    the face count each of them reached, so the two are compared at an equal budget (the collapse may end one face lower).  The
    collapse's largest distance to the analytic sphere must be the smaller one: two measured values, written to the profile with those
    of the cube before they are compared.  The distance is the SURFACE's (vertices and the faces' nearest points: with a few hundred
    faces the chords' sagitta is the larger part, and a quadric places its vertices outside the sphere to halve it); the vertices' own
    figure is written next to it."""
    from rc_mvsnet_amd import mesh_clean as MC
    MSC.check_extraction(DEV)
    verts, faces, rgb, _ = MC.clean_mesh(*MSC.MCC.scene_volume(DEV).extract(1), keep_largest=1)
    centre, radius = MSC.MCC.SCENE_SPHERES[0]
    err = lambda v, f: _sphere_error(MSC.host(v), MSC.host(f), centre, radius)      # noqa: E731
    lines = ["the large sphere as extracted: %d faces, max distance to the analytic sphere: surface %.6f, vertices %.6f" % ((int(faces.shape[0]),) + err(verts, faces))]
    results = []
    for voxels in (2.0, 3.0):
        cv, cf, _, cstats = MD.decimate(verts, faces, rgb, cell=voxels)
        sv, sf, _, stats = MS.simplify(verts, faces, rgb, target_faces=cstats["faces_out"])
        assert stats["stop"] == "target" and cstats["faces_out"] - 1 <= stats["faces_out"] <= cstats["faces_out"] < stats["faces_in"], (voxels, stats, cstats)
        collapse, cluster = err(sv, sf), err(cv, cf)
        lines.append(f"large sphere, clustering cell {voxels} voxels: {cstats['faces_out']} faces, max distance to the sphere: surface {cluster[0]:.6f}, vertices "
                     f"{cluster[1]:.6f}; collapse to {stats['faces_out']} faces in {stats['rounds']} rounds (collapses per round {stats['collapses']}): "
                     f"surface {collapse[0]:.6f}, vertices {collapse[1]:.6f}")
        print(lines[-1])
        results.append((collapse[0], cluster[0], lines[-1]))
    lines.append(MSC.check_cube(DEV, 9))
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "mesh_simplify_pytest_gpu.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    for collapse, cluster, line in results:                       # after the figures are on file
        assert collapse < cluster, line


def test_mesh_simplify_command_line_round_trip(tmp_path, capsys):
    """python -m rc_mvsnet_amd.mesh_simplify on a written coloured mesh: the bytes of mesh_ply_bytes of simplify()'s result, and the
    JSON line is its stats"""
    v, f, rgb = MSC.case("sphere")
    src, out = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    with open(src, "wb") as fh:
        fh.write(TM.mesh_ply_bytes(v, f, rgb))
    for argv, kw in ((["--ratio", "0.5"], {"ratio": 0.5}),
                     (["--faces", "100", "--max-error", "1e-3", "--max-rounds", "5", "--keep-unreferenced"], {"target_faces": 100, "max_error": 1e-3, "max_rounds": 5, "drop_unreferenced": False})):
        MS.main(["--in", src, "--out", out, "--device", DEV] + argv)
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        gv, gf, gc, stats = MS.simplify(*MSC.to_dev(DEV, v, f, rgb), **kw)
        assert open(out, "rb").read() == TM.mesh_ply_bytes(gv, gf, gc) and {k: line[k] for k in stats} == stats and line["in"] == src and line["out"] == out
        wv, wf, wc, wstats, _ = MSC.O.simplify(v, f, rgb, **kw)
        rv, rf, rc = dtu_io.read_ply_mesh_rgb(out)
        assert MSC.same_bits(rv, wv) and np.array_equal(rf, wf) and np.array_equal(rc, wc) and stats == wstats


@pytest.mark.parametrize("sparse", [False, True])
def test_tsdf_mesh_with_simplification_end_to_end_and_its_command_line(tmp_path, capsys, sparse):
    pair_folder, out_folder, summary = MSC.check_end_to_end(DEV, tmp_path, sparse)
    capsys.readouterr()
    ply = str(tmp_path / "cli.ply")
    TM.main(["--pair-folder", pair_folder, "--scan-folder", out_folder, "--out-folder", out_folder, "--mesh", ply, "--resolution", "32", "--simplify-ratio", "0.5",
             "--device", DEV] + (["--sparse"] if sparse else []))
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    gv, gf = dtu_io.read_ply_mesh(ply)
    s = line["simplify"]
    assert s == summary["simplify"] and s["faces_out"] < s["faces_in"] and line["vertices"] == len(gv) == s["vertices_out"] and line["faces"] == len(gf) == s["faces_out"]
