"""The mesh normals (rc_mvsnet_amd/mesh_normals.py, csrc/mesh_normals.hip) on the mesh of the dense TSDF bench's synthetic scene
(tools/tsdf_mesh_bench.py: 512 x 512 x 384 voxels, some 1.27 M vertices / 2.53 M faces), built the way tools/mesh_render_bench.py
builds it, and the normal pass over --views of the bench's own 1184 x 1600 cameras: ms per phase from the kernels' own timestamps,
one JSON line.

The scene is synthetic and its size is ASSUMED (a DTU-like scan, not measured from one).  Reported per phase, each as the median of
--reps after a warm-up, from the start / stop timestamps of the launches themselves (the *_timed entry points), next to the time its
bytes would take at 8 TB/s if every array it must touch crossed HBM once (nv vertices, nf faces, n = 3 nf corners, P radix passes,
p = H W pixels per view, c covered pixels):
    face_normals    faces read (12 nf), positions read once (12 nv), normals written (12 nf)
    incidence       faces and positions read (12 nf + 12 nv), the pairs written (8 n), per pass the keys read twice, the corner numbers
                    once and the pairs written (20 n P), the sorted keys read (4 n), the segments zeroed and written (16 nv); the
                    histograms and their scans are in no floor
    accumulate      segments (8 nv), corner numbers (4 n), faces (12 nf), positions (12 nv) read, normals written (12 nv); the gather
                    of three positions per corner is in no floor: the ratio to the floor is what it costs
    shade           per view the face image read (4 p), normal map, smooth and colour written (16 p), per covered pixel its face,
                    three positions and three normals (84 c)
Also ``oracle``: tests/mesh_normals_oracle.py (numpy, one corner after another, one process) on the faces near a 64 x 48 crop of the
first view, its times, and whether the GPU's normals of that sub-mesh and its normal pass over the crop equal it in every bit.

    python tools/mesh_normals_bench.py [--reps 5] [--views 2] [--no-cpu-baseline] [--out profiles/mesh_normals_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from rc_mvsnet_amd import _lib, mesh_normals as MN, mesh_render as MR, tsdf_mesh as TM        # noqa: E402
from tools.mesh_clean_bench import phase        # noqa: E402
from tools.mesh_render_bench import CROP, timed        # noqa: E402
from tools.tsdf_mesh_bench import DIMS, H, ORIGIN, TRUNC_VOXELS, VOXEL, W, scene        # noqa: E402

WHAT = "see the docstring of tools/mesh_normals_bench.py"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--views", type=int, default=2)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    _lib.load()
    dev = "cuda:0"
    depth, rgb_views, cams = scene(dev)
    vol = TM.TsdfVolume(ORIGIN, VOXEL, DIMS, dev)
    vol.integrate(depth, cams, rgb_views, trunc=TRUNC_VOXELS * VOXEL)
    verts, faces, rgb = vol.extract(1)
    del vol, rgb_views, depth
    nv, nf, V, p = int(verts.shape[0]), int(faces.shape[0]), args.views, H * W
    n, passes = 3 * nf, max(1, (nv.bit_length() + 7) // 8)
    cams = cams[:V]

    normals, stats = {}, {}
    for w in ("area", "sphere"):
        normals[w], stats[w] = MN.vertex_normals(verts, faces, w)
        again = MN.vertex_normals_device(verts, faces, w)[0]
        assert torch.equal(normals[w].view(torch.int32), again.view(torch.int32)), "two runs differ"
    out = MR.render(verts, faces, rgb, cams, H, W, cull="back")
    covered = int((out["face"] >= 0).sum())
    shaded = MN.shade(verts, faces, normals["sphere"], cams, out["face"])
    ms = {"face_normals": timed(lambda e0, e1: MN.face_normals(verts, faces, _timed=("all", e0, e1)), args.reps),
          "incidence": timed(lambda e0, e1: MN.vertex_normals_device(verts, faces, "area", _timed=("incidence", e0, e1)), args.reps),
          "accumulate_area": timed(lambda e0, e1: MN.vertex_normals_device(verts, faces, "area", _timed=("accumulate", e0, e1)), args.reps),
          "accumulate_sphere": timed(lambda e0, e1: MN.vertex_normals_device(verts, faces, "sphere", _timed=("accumulate", e0, e1)), args.reps),
          "all_area": timed(lambda e0, e1: MN.vertex_normals_device(verts, faces, "area", _timed=("all", e0, e1)), args.reps),
          "all_sphere": timed(lambda e0, e1: MN.vertex_normals_device(verts, faces, "sphere", _timed=("all", e0, e1)), args.reps),
          "shade": timed(lambda e0, e1: MN.shade(verts, faces, normals["sphere"], cams, out["face"], _timed=("all", e0, e1)), args.reps)}
    walls = []
    for _ in range(args.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        MN.vertex_normals_device(verts, faces, "sphere")
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    accumulate_bytes = 8 * nv + 4 * n + 12 * nf + 24 * nv
    line = {"workload": "mesh_normals", "sizes": "assumed, synthetic scene (not measured from a scan)", "vertices": nv, "faces": nf, "corners": n,
            "radix_passes": passes, "views": V, "H": H, "W": W, "incidence_route": "stable radix sort of the (vertex, corner) pairs, segments from the sorted keys",
            "timing": "the kernels' own start / stop timestamps, median of %d launches" % args.reps,
            "face_normals": phase(ms["face_normals"], 24 * nf + 12 * nv, WHAT),
            "incidence": phase(ms["incidence"], 12 * nf + 12 * nv + 8 * n + 20 * n * passes + 4 * n + 16 * nv, WHAT),
            "accumulate_area": phase(ms["accumulate_area"], accumulate_bytes, WHAT), "accumulate_sphere": phase(ms["accumulate_sphere"], accumulate_bytes, WHAT),
            "vertex_normals_area": {"ms": ms["all_area"][0], "ms_min": ms["all_area"][1], "what": "first launch's start to last launch's stop"},
            "vertex_normals_sphere": {"ms": ms["all_sphere"][0], "ms_min": ms["all_sphere"][1], "what": "first launch's start to last launch's stop"},
            "shade": phase(ms["shade"], 20 * p * V + 84 * covered, WHAT),
            "vertex_normals_wall_ms": {"median": round(float(np.median(walls[1:])), 2), "min": round(min(walls[1:]), 2),
                                       "what": "vertex_normals_device(sphere) end to end with its allocations, host clock"},
            "stats": stats, "pixels_covered": covered,
            "mean_smooth_shade_of_covered_pixels": round(float(shaded["smooth"][out["face"] >= 0].float().mean()), 2)}
    if args.no_cpu_baseline:
        line["oracle"] = "not measured"
    else:
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import mesh_normals_oracle as O
        ch, cw, y0, x0 = CROP
        cam = np.array(cams[0])
        cam[14] -= x0
        cam[15] -= y0
        # the faces that can touch the crop, as tools/mesh_render_bench.py selects them, with their vertices renumbered (bench set-up, torch on the device)
        R, t = torch.from_numpy(cam[:9].reshape(3, 3)).to(dev), torch.from_numpy(cam[9:12]).to(dev)
        pc = verts.double() @ R.T + t
        u, v = cam[12] * pc[:, 0] / pc[:, 2] + cam[14], cam[13] * pc[:, 1] / pc[:, 2] + cam[15]
        near_crop = (u > -4) & (u < cw + 4) & (v > -4) & (v < ch + 4)
        sub = faces[near_crop[faces.long()].all(1)]
        used, inverse = torch.unique(sub.long(), return_inverse=True)
        sv, sf = verts[used].contiguous(), inverse.to(torch.int32).reshape(-1, 3).contiguous()
        hv, hf = sv.cpu().numpy(), sf.cpu().numpy()
        oracle = {"what": "tests/mesh_normals_oracle.py (numpy, one corner after another, one process) on the %d faces / %d vertices near a %d x %d crop of "
                          "view 0, same host" % (len(hf), len(hv), cw, ch)}
        same = True
        for w in ("area", "sphere"):
            got, gstats = MN.vertex_normals(sv, sf, w)
            t0 = time.perf_counter()
            want, wstats = O.vertex_normals(hv, hf, w)
            oracle["vertex_normals_%s_ms" % w] = round((time.perf_counter() - t0) * 1e3, 1)
            same = same and np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)) and gstats == wstats
        crop = MR.render(sv, sf, None, cam[None], ch, cw, cull="back", normals=got)
        face = crop["face"].cpu().numpy()
        t0 = time.perf_counter()
        wshade = O.shade(hv, hf, want, cam[None], face, MR.DEFAULT_NEAR)
        oracle["shade_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        same = (same and np.array_equal(crop["normal"].cpu().numpy().view(np.uint32), wshade["normal"].view(np.uint32)) and
                np.array_equal(crop["smooth"].cpu().numpy(), wshade["smooth"]) and np.array_equal(crop["normal_rgb"].cpu().numpy(), wshade["normal_rgb"]))
        assert same, "the GPU's sub-mesh differs from the oracle's"
        oracle.update(gpu_equal_in_every_bit=bool(same), pixels_covered=int((face >= 0).sum()))
        line["oracle"] = oracle
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
