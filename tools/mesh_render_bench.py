"""The mesh rasteriser (rc_mvsnet_amd/mesh_render.py, csrc/mesh_render.hip) on the mesh of the dense TSDF bench's synthetic scene
(tools/tsdf_mesh_bench.py: 512 x 512 x 384 voxels, some 1.27 M vertices / 2.53 M faces) rendered into --views of the bench's own
1184 x 1600 cameras: ms per phase of one view from the kernels' own timestamps, one JSON line.

The scene is synthetic and its size is ASSUMED (a DTU-like scan, not measured from one).  Reported per phase, each as the median of
--reps after a warm-up, from the start / stop timestamps of the launches themselves (rcmvs_mr_render_timed with the phase named,
which brackets that phase of the call's last view; rcmvs_mr_compare_timed), next to the time its bytes would take at 8 TB/s if
every array it must touch crossed HBM once (nv vertices, nf faces, p = H W pixels, c covered pixels):
    project     positions read (12 nv), one record per vertex written (24 nv)
    small       the keys cleared (8 p), faces read (12 nf), the records read once (24 nv); the gathers of three records per face
                and the key traffic of the samples are in no floor: the ratio to the floor is what they cost
    large       the list and its faces' records; with no face on the large path the floor is the list's count alone, reported as 0
    resolve     keys read (8 p), depth, face, colour, shade written (12 p), per covered pixel its face, three positions and three
                colours (57 c)
    compare     the two depth maps read (8 p per view)
Also: the histogram of the faces' clamped bounding boxes by their longer side, the share of faces on the large path, the samples
inside a face against the atomics issued (what the early reject saved; both depend on the schedule), and ``oracle``:
tests/mesh_render_oracle.py (numpy, one face after another, one process) on a 64 x 48 crop of the first view with the faces that
can touch it, its time, and whether the GPU's render of the same crop equals it in every bit.

    python tools/mesh_render_bench.py [--reps 5] [--views 2] [--no-cpu-baseline] [--out profiles/mesh_render_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from rc_mvsnet_amd import _lib, mesh_render as MR, tsdf_mesh as TM        # noqa: E402
from tools.mesh_clean_bench import phase        # noqa: E402
from tools.tsdf_mesh_bench import DIMS, H, ORIGIN, TRUNC_VOXELS, VOXEL, W, scene, timed_events        # noqa: E402

WHAT = "see the docstring of tools/mesh_render_bench.py"
CROP = (48, 64, 560, 760)                                          # H, W, first row, first column of the oracle's crop


def timed(launch, reps):
    """launch(ev0, ev1) -> (median, min) ms of the bracketed launches over reps, after one warm-up"""
    runs = []
    for _ in range(reps + 1):
        ev = timed_events()
        launch(ctypes.c_void_p(ev[0].cuda_event), ctypes.c_void_p(ev[1].cuda_event))
        runs.append(ev)
    torch.cuda.synchronize()
    t = [a.elapsed_time(b) for a, b in runs[1:]]
    return round(float(np.median(t)), 4), round(min(t), 4)


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
    del vol, rgb_views
    nv, nf, V, p = int(verts.shape[0]), int(faces.shape[0]), args.views, H * W
    cams, depth = cams[:V], depth[:V].contiguous()

    trace = torch.zeros(MR.TRACE, device=dev, dtype=torch.int64)
    out = MR.render(verts, faces, rgb, cams, H, W, cull="back", trace=trace)
    stats = MR.stats_rows(out)
    again = MR.render(verts, faces, rgb, cams, H, W, cull="back")
    assert all(torch.equal(out[k], again[k]) for k in out), "two runs differ"
    tr = dict(zip(MR.TRACE_NAMES, (int(x) for x in trace.cpu())))
    ms = {name: timed(lambda e0, e1, name=name: MR.render(verts, faces, rgb, cams, H, W, cull="back", _timed=(name, e0, e1)), args.reps)
          for name in ("project", "small", "large", "resolve", "all")}
    th = MR.DEFAULT_THRESHOLDS
    c_ms = timed(lambda e0, e1: MR.compare_table(out["depth"], depth, th, _timed=(e0, e1)), args.reps)
    table = MR.sum_rows(MR.compare(out["depth"], depth, th), th)
    walls = []
    for _ in range(args.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        MR.render(verts, faces, rgb, cams, H, W, cull="back")
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    c = stats[-1]["pixels_covered"]
    drawn = sum(s["faces_drawn"] for s in stats)
    line = {"workload": "mesh_render", "sizes": "assumed, synthetic scene (not measured from a scan)", "vertices": nv, "faces": nf, "views": V, "H": H, "W": W,
            "cull": "back", "timing": "the kernels' own start / stop timestamps, median of %d launches; the phases are those of one view (the call's last)" % args.reps,
            "project": phase(ms["project"], 36 * nv, WHAT), "raster_small": phase(ms["small"], 8 * p + 12 * nf + 24 * nv, WHAT),
            "raster_large": {"ms": ms["large"][0], "ms_min": ms["large"][1], "floor_ms": 0.0, "floor_what": WHAT},
            "resolve": phase(ms["resolve"], 20 * p + 57 * c, WHAT), "compare": phase(c_ms, 8 * p * V, WHAT),
            "all_views": {"ms": ms["all"][0], "ms_min": ms["all"][1], "what": "first launch's start to last launch's stop of the %d views" % V},
            "render_wall_ms": {"median": round(float(np.median(walls[1:])), 2), "min": round(min(walls[1:]), 2),
                               "what": "render() of the %d views end to end with its allocations, host clock" % V},
            "stats": stats, "box_histogram": {k: v for k, v in tr.items() if k.startswith("box_")},
            "share_on_large_path": sum(s["faces_large"] for s in stats) / max(drawn, 1),
            "early_reject": {"samples_inside": tr["samples_inside"], "atomics_issued": tr["atomics_issued"],
                             "share_of_atomics_saved": 1.0 - tr["atomics_issued"] / max(tr["samples_inside"], 1), "what": "over the %d views, one run; depends on the schedule" % V},
            "compare_with_the_fused_depth_maps": table}
    if args.no_cpu_baseline:
        line["oracle"] = "not measured"
    else:
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import mesh_render_oracle as O
        ch, cw, y0, x0 = CROP
        cam = np.array(cams[0])
        cam[14] -= x0
        cam[15] -= y0
        # the faces that can touch the crop: all three vertices within 4 pixels of it (bench set-up, torch on the device)
        R, t = torch.from_numpy(cam[:9].reshape(3, 3)).to(dev), torch.from_numpy(cam[9:12]).to(dev)
        pc = verts.double() @ R.T + t
        u, v = cam[12] * pc[:, 0] / pc[:, 2] + cam[14], cam[13] * pc[:, 1] / pc[:, 2] + cam[15]
        near_crop = (u > -4) & (u < cw + 4) & (v > -4) & (v < ch + 4)
        keep = near_crop[faces.long()].all(1)
        sub = faces[keep].contiguous()
        got = MR.render(verts, sub, rgb, cam[None], ch, cw, cull="back")
        hv, hf, hc = verts.cpu().numpy(), sub.cpu().numpy(), rgb.cpu().numpy()
        t0 = time.perf_counter()
        want = O.render(hv, hf, hc, cam[None], ch, cw, MR.DEFAULT_NEAR, "back")
        t1 = time.perf_counter()
        same = (np.array_equal(got["keys"].cpu().numpy().view(np.uint64), want["keys"]) and np.array_equal(got["rgb"].cpu().numpy(), want["rgb"]) and
                np.array_equal(got["shade"].cpu().numpy(), want["shade"]) and MR.stats_rows(got) == want["stats"] and
                np.array_equal(got["depth"].cpu().numpy().view(np.uint32), want["depth"].view(np.uint32)))
        assert same, "the GPU's crop differs from the oracle's"
        whole = out["depth"][0, y0:y0 + ch, x0:x0 + cw]
        line["oracle"] = {"what": "tests/mesh_render_oracle.py (numpy, one face after another, one process) on a %d x %d crop of view 0 with the %d faces near it, "
                                  "same host" % (cw, ch, len(hf)), "render_ms": round((t1 - t0) * 1e3, 1), "gpu_crop_equal_in_every_bit": bool(same),
                          "crop_depth_equals_the_whole_render": bool(torch.equal(whole.view(torch.int32), got["depth"][0].view(torch.int32))),
                          "pixels_covered": want["stats"][0]["pixels_covered"]}
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
