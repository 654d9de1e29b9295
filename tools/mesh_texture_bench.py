"""The mesh texturing (rc_mvsnet_amd/mesh_texture.py, csrc/mesh_texture.hip) on the mesh of the dense TSDF bench's synthetic scene
(tools/tsdf_mesh_bench.py: 512 x 512 x 384 voxels, some 1.27 M vertices / 2.53 M faces), built the way tools/mesh_render_bench.py
builds it, as extracted and after decimation at --voxels voxels, textured from --views of the bench's own 1184 x 1600 cameras and
images: ms per phase from the kernels' own timestamps, one JSON line.

The scene is synthetic and its size is ASSUMED (a DTU-like scan, not measured from one); its images are noise.  Reported per mesh and
phase, each as the median of --reps after a warm-up, from the start / stop timestamps of the launches themselves (the *_timed entry
points), next to the time its bytes would take at 8 TB/s if every array it must touch crossed HBM once (nv vertices, nf faces, V
views of p = H W pixels, c covered pixels, T = S Sy texels of the atlas):
    vote            per view the face image read (4 p), the counts zeroed, added to and read (12 nf), faces and positions read
                    (12 nf + 12 nv), best read and written (16 nf); the atomic adds themselves are in no floor
    layout          classes: faces, positions and best read (20 nf + 12 nv), class, key and index written (12 nf); one radix pass: the
                    keys read twice, the indices once, the pairs written (20 nf); corners: keys and order read (8 nf), texel
                    coordinates written (24 nf); the histogram, its scan and the table are in no floor
    fill            atlas and owner written (7 T), the images read once (3 p V), per face its indices, positions, best and order
                    (24 nf + 12 nv); the four taps per texel are in no floor: the ratio to the floor is what they cost.  Next to it the
                    same fill with every face taken as unseen (no projection, no image read; the images leave its floor): what of the
                    fill is finding the texel's face and writing the atlas
    shade           per view the face image read (4 p) and the pixels written (3 p), per covered pixel its face, three positions and
                    six texel coordinates (72 c), the atlas read once (3 T)
The render that gives the vote its face images is mesh_render's and is timed by tools/mesh_render_bench.py, not here.
Also ``oracle``: tests/mesh_texture_oracle.py (numpy, one process) on the faces near a 64 x 48 crop of the first view, textured from
that crop alone: its times per phase, and whether the GPU's result on that sub-mesh equals it in every bit.

    python tools/mesh_texture_bench.py [--reps 5] [--views 2] [--voxels 2] [--no-cpu-baseline] [--out profiles/mesh_texture_bench.json]
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
from rc_mvsnet_amd import _lib, mesh_decimate as MD, mesh_render as MR, mesh_texture as MT, tsdf_mesh as TM        # noqa: E402
from tools.mesh_clean_bench import phase        # noqa: E402
from tools.mesh_render_bench import CROP, timed        # noqa: E402
from tools.tsdf_mesh_bench import DIMS, H, ORIGIN, TRUNC_VOXELS, VOXEL, W, scene        # noqa: E402

WHAT = "see the docstring of tools/mesh_texture_bench.py"


def measure(verts, faces, rgb, images, cams, reps):
    """one mesh -> its part of the JSON line"""
    nv, nf, V, p = int(verts.shape[0]), int(faces.shape[0]), len(cams), H * W
    tex = MT.texture(verts, faces, rgb, images, cams, cull="back")
    again = MT.texture(verts, faces, rgb, images, cams, cull="back", chunk=1)
    assert all(torch.equal(tex[k], again[k]) for k in ("best", "klass", "order", "texel", "owner", "atlas")), "two runs differ"
    Sy, S = tex["size"]
    T = S * Sy
    out = MR.render(verts, faces, rgb, cams, H, W, cull="back")
    covered = int((out["face"] >= 0).sum())
    cams_dev = torch.from_numpy(cams.copy()).to(verts.device)
    lay = MT.layout(verts, faces, tex["best"], cams_dev, H, W, shift=tex["shift"])
    ms = {"vote": timed(lambda e0, e1: MT.vote(verts, faces, out["face"], cams, _timed=(e0, e1)), reps),
          "layout": timed(lambda e0, e1: MT.layout(verts, faces, tex["best"], cams_dev, H, W, shift=tex["shift"], _timed=(e0, e1)), reps),
          "fill": timed(lambda e0, e1: MT.fill(verts, faces, rgb, images, tex["best"], lay, S, Sy, _timed=(e0, e1)), reps),
          "shade": timed(lambda e0, e1: MT.shade(verts, faces, cams, out["face"], tex["texel"], tex["atlas"], _timed=(e0, e1)), reps)}
    # the same layout filled with every face taken as unseen: the texel's class, cell and face are found and the atlas is written, but no
    # face is projected and no image is read -- what of the fill is the atlas's own traffic and what the projection and the taps
    unseen = torch.zeros_like(tex["best"])
    ms["fill_unseen"] = timed(lambda e0, e1: MT.fill(verts, faces, rgb, images, unseen, lay, S, Sy, _timed=(e0, e1)), reps)
    MT.fill(verts, faces, rgb, images, tex["best"], lay, S, Sy)                     # the counters of lay["stats"] as they were
    walls = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        MT.texture(verts, faces, rgb, images, cams, cull="back")
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    return {"vertices": nv, "faces": nf, "atlas": [Sy, S], "shift": tex["shift"], "texels_used": tex["table"]["total"], "pixels_covered": covered,
            "vote": phase(ms["vote"], V * (4 * p + 40 * nf + 12 * nv), WHAT),
            "layout": phase(ms["layout"], 84 * nf + 12 * nv, WHAT),
            "fill": phase(ms["fill"], 7 * T + 3 * p * V + 24 * nf + 12 * nv, WHAT),
            "fill_with_every_face_unseen": phase(ms["fill_unseen"], 7 * T + 24 * nf + 12 * nv, WHAT),
            "shade": phase(ms["shade"], 7 * p * V + 72 * covered + 3 * T, WHAT),
            "texture_wall_ms": {"median": round(float(np.median(walls[1:])), 2), "min": round(min(walls[1:]), 2),
                                "what": "texture() end to end with its renders, allocations and the host's read of the table, host clock"},
            "stats": tex["stats"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--views", type=int, default=2)
    ap.add_argument("--voxels", type=float, default=2.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    _lib.load()
    dev = "cuda:0"
    depth, rgb_views, cams = scene(dev)
    vol = TM.TsdfVolume(ORIGIN, VOXEL, DIMS, dev)
    vol.integrate(depth, cams, rgb_views, trunc=TRUNC_VOXELS * VOXEL)
    verts, faces, rgb = vol.extract(1)
    del vol, depth
    V = args.views
    cams, images = np.ascontiguousarray(cams[:V]), rgb_views[:V].contiguous()
    del rgb_views
    dv, df, dc = MD.decimate(verts, faces, rgb, cell=args.voxels * VOXEL)[:3]
    line = {"workload": "mesh_texture", "sizes": "assumed, synthetic scene (not measured from a scan); the images are noise", "views": V, "H": H, "W": W, "cull": "back",
            "timing": "the kernels' own start / stop timestamps, median of %d launches" % args.reps,
            "decimated_%g_voxels" % args.voxels: measure(dv, df, dc, images, cams, args.reps), "undecimated": measure(verts, faces, rgb, images, cams, args.reps)}
    if args.no_cpu_baseline:
        line["oracle"] = "not measured"
    else:
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import mesh_texture_oracle as O
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
        sv, sf, sc = verts[used].contiguous(), inverse.to(torch.int32).reshape(-1, 3).contiguous(), rgb[used].contiguous()
        crop = images[:1, y0:y0 + ch, x0:x0 + cw].contiguous()
        got = MT.texture(sv, sf, sc, crop, cam[None], cull="back")
        face = MR.render(sv, sf, sc, cam[None], ch, cw, cull="back")["face"]
        shaded = MT.shade(sv, sf, cam[None], face, got["texel"], got["atlas"])
        hv, hf, hc, himg, hface = (x.cpu().numpy() for x in (sv, sf, sc, crop, face))
        near = MT.DEFAULT_NEAR
        t0 = time.perf_counter()
        best = O.vote(hv, hf, hface, cam[None], near)
        t1 = time.perf_counter()
        views, Ps = O.chosen(hv, hf, best, cam[None], ch, cw, near)
        klass, capped = O.classes(hf, views, Ps, got["shift"])
        order, table, texel = O.layout(klass)
        t2 = time.perf_counter()
        atlas, owner, counts = O.fill(hv, hf, hc, himg, cam[None], near, views, order, table, texel)
        t3 = time.perf_counter()
        wshade = O.shade(hv, hf, cam[None], hface, texel, atlas, near)
        t4 = time.perf_counter()
        same = (np.array_equal(got["best"].cpu().numpy().view(np.uint64), np.array(best, np.uint64)) and np.array_equal(got["klass"].cpu().numpy(), klass) and
                np.array_equal(got["order"].cpu().numpy(), order) and got["table"] == table and np.array_equal(got["texel"].cpu().numpy(), texel) and
                np.array_equal(got["owner"].cpu().numpy(), owner) and np.array_equal(got["atlas"].cpu().numpy(), atlas) and
                np.array_equal(shaded.cpu().numpy(), wshade) and all(got["stats"][k] == n for k, n in counts.items()))
        assert same, "the GPU's sub-mesh differs from the oracle's"
        line["oracle"] = {"what": "tests/mesh_texture_oracle.py (numpy, one process) on the %d faces / %d vertices near a %d x %d crop of view 0, textured from that "
                                  "crop, same host; the oracle's vote is given the GPU render's face image" % (len(hf), len(hv), cw, ch),
                          "vote_ms": round((t1 - t0) * 1e3, 1), "layout_ms": round((t2 - t1) * 1e3, 1), "fill_ms": round((t3 - t2) * 1e3, 1),
                          "shade_ms": round((t4 - t3) * 1e3, 1), "atlas": [table["Sy"], table["S"]], "gpu_equal_in_every_bit": bool(same)}
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
