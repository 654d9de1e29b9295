"""COLMAP import (rc_mvsnet_amd/colmap_import.py) on a synthetic sparse model: ms per phase on the HIP path, one JSON line.

The sizes (300 images, 1 M points, a mean track length of about 6) are ASSUMED, not measured from a COLMAP reconstruction.  The
three phases (pair scores, top views, depth ranks) are timed with device events around each call, median of --reps after a
warm-up.  The yardstick is the numpy oracle (tests/colmap_oracle.py) on the same model and the same host, timed once; the results
of both are compared.  ``--rocprof DIR`` also runs the three phases once in a child process under ``rocprofv3 --kernel-trace --stats``.

The undistortion phase (``undistort_image``'s launch, csrc/undistort.hip) runs on OPENCV images of 1080 x 1920 and 3000 x 4000 (both
ASSUMED sizes): the kernel alone from its own start / stop timestamps (rcmvs_undistort_rgb8_timed), median of --reps launches
after a warm-up; against the numpy oracle (tests/undistort_oracle.py) on the same host, whose bytes and
blank count are compared, and against the bytes-moved floor: 3 H W bytes read plus 3 H W written at 8 TB/s.  ``host_codec_ms`` is
what the import spends around the launch on the same host: PIL decoding a quality-95 JPEG of that size (a smooth image with mild
noise) and encoding the result, median of 3.

    python tools/colmap_import_bench.py [--reps 5] [--phases all|import|undistort] [--rocprof DIR] [--no-cpu-baseline]
                                        [--out profiles/colmap_import_bench.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from rc_mvsnet_amd import _lib, colmap_import as CI, synthetic        # noqa: E402

N_IMAGES, N_POINTS, TRACK, NUM_SRC = 300, 1_000_000, 6.0, 10


def event_ms(fn, reps):
    """-> (result, median ms between two device events around fn)"""
    out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return out, round(float(np.median(times)), 4)


UNDISTORT_SIZES, HBM_BYTES_PER_S = ((1080, 1920), (3000, 4000)), 8e12


def host_codec_ms(h, w):
    """-> (decode ms, encode ms) of a quality-95 JPEG of a smooth h x w image with mild noise, PIL, median of 3"""
    import io
    from PIL import Image
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    rgb = np.stack([128 + 100 * np.sin(xs / 97.0), 128 + 100 * np.cos(ys / 61.0), 128 + 90 * np.sin((xs + ys) / 143.0)], 2)
    rgb = np.clip(rgb + np.random.default_rng(0).normal(0.0, 4.0, rgb.shape), 0, 255).astype(np.uint8)
    dec, enc = [], []
    for _ in range(3):
        buf = io.BytesIO()
        t0 = time.perf_counter()
        Image.fromarray(rgb).save(buf, format="JPEG", quality=95)
        t1 = time.perf_counter()
        with Image.open(io.BytesIO(buf.getvalue())) as im:
            np.array(im.convert("RGB"), dtype=np.uint8)
        t2 = time.perf_counter()
        enc.append((t1 - t0) * 1e3)
        dec.append((t2 - t1) * 1e3)
    return round(float(np.median(dec)), 1), round(float(np.median(enc)), 1)


def undistort_phase(reps, cpu_baseline, dev="cuda:0"):
    """-> the "undistort" entry of the JSON line: one dict per image size"""
    from rc_mvsnet_amd.ops import _chk, _stream
    rows = []
    for h, w in UNDISTORT_SIZES:
        img = np.random.default_rng(5).integers(0, 256, (h, w, 3), dtype=np.uint8)
        cam, dist = (1.1 * w, 1.09 * w, 0.5 * w - 7.3, 0.5 * h + 4.6), (0.09, 0.02, 0.001, -0.0015, 0.0, 0.0, 0.0, 0.0)
        src = torch.from_numpy(img).to(dev)
        out, blank = torch.empty_like(src), torch.empty(1, device=dev, dtype=torch.int32)
        d8 = (ctypes.c_double * 8)(*dist)

        events = []
        for i in range(reps + 1):                                                 # the first launch is the warm-up
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
            ev[1].record()                                                        # a torch event owns its hipEvent_t after a first record
            _lib.call("rcmvs_undistort_rgb8_timed", _chk(src, "src", torch.uint8), _chk(out, "out", torch.uint8), h, w, *cam, cam[0], cam[1], d8,
                      _chk(blank, "blank", torch.int32), ctypes.c_void_p(ev[0].cuda_event), ctypes.c_void_p(ev[1].cuda_event), _stream())
            events.append(ev)
        torch.cuda.synchronize()
        own = [1e3 * a.elapsed_time(b) for a, b in events[1:]]
        us, floor_us = float(np.median(own)), 2 * 3 * h * w / HBM_BYTES_PER_S * 1e6
        row = {"h": h, "w": w, "model": "OPENCV", "kernel_us": round(us, 3), "kernel_us_min": round(min(own), 3), "floor_us": round(floor_us, 3),
               "floor_what": "3 H W bytes read + 3 H W bytes written at 8 TB/s", "times_floor": round(us / floor_us, 2),
               "blank_fraction": int(blank.item()) / (h * w)}
        dec, enc = host_codec_ms(h, w)
        row["host_codec_ms"] = {"jpeg_decode": dec, "jpeg_encode_q95": enc, "kernel_share": round(us * 1e-3 / (dec + enc + us * 1e-3), 5)}
        got, got_blank = CI.undistort_image(src, cam, dist)
        row["two_runs_identical"] = bool(torch.equal(got, out)) and got_blank == int(blank.item())
        if cpu_baseline:
            import undistort_oracle as UO
            t0 = time.perf_counter()
            want, want_blank = UO.undistort(img, cam, dist)
            row["oracle_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            row["bytes_equal_oracle"] = bool(np.array_equal(got.cpu().numpy(), want))
            row["blank_equal_oracle"] = got_blank == want_blank
        else:
            row["oracle_ms"] = "not measured"
        rows.append(row)
    return {"sizes": "assumed", "timing": "the kernel's own start / stop timestamps, median of %d launches" % reps, "images": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--phases", choices=("all", "import", "undistort"), default="all", help="import: pair scores, top views, depth ranks; "
                    "undistort: the undistortion launch on two image sizes")
    ap.add_argument("--rocprof", default=None, help="directory: the three phases once in a child process under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--one-pass", action="store_true", help="(the profiled child) the three phases once, no timing")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    _lib.load()
    dev = "cuda:0"
    sys.path.insert(0, os.path.join(REPO, "tests"))
    if args.phases == "undistort":
        text = json.dumps({"workload": "colmap_import", "undistort": undistort_phase(args.reps, not args.no_cpu_baseline, dev)})
        print(text, flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    # every camera of the ring sees the whole box, so the frustum alone would give tracks of 300: observations are kept with the
    # probability that leaves about TRACK of them per point
    probe = synthetic.colmap_arrays(N_IMAGES, 20_000, hw=(1080, 1920), seed=0, arc_deg=300.0, keep=1.0)
    frac = len(probe["ids"]) / (N_IMAGES * 20_000)
    A = synthetic.colmap_arrays(N_IMAGES, N_POINTS, hw=(1080, 1920), seed=0, arc_deg=300.0, keep=TRACK / (N_IMAGES * frac))
    counts = np.diff(A["offsets"])
    ranks = np.array([CI.rank_pair(int(c)) for c in counts], dtype=np.int32)
    zrows = np.ascontiguousarray(A["extrinsics"][:, 2, :])
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         (("centres", A["centres"]), ("points", A["points"]), ("offsets", A["offsets"]), ("ids", A["ids"]), ("zrows", zrows), ("ranks", ranks))}

    def scores():
        return CI.pair_scores(t["centres"], t["points"], t["offsets"], t["ids"])

    def depth():
        return CI.depth_ranges(t["points"], t["zrows"], t["offsets"], t["ids"], t["ranks"])

    if args.one_pass:
        CI.top_views(scores(), NUM_SRC)
        depth()
        torch.cuda.synchronize()
        return
    line = {"workload": "colmap_import", "sizes": "assumed, not taken from a COLMAP reconstruction", "images": N_IMAGES, "points": N_POINTS,
            "observations": int(len(A["ids"])), "mean_track": round(len(A["ids"]) / N_POINTS, 3), "num_src": NUM_SRC,
            "timing": "device events around each call, median of %d" % args.reps}
    S, line["pair_scores_ms"] = event_ms(scores, args.reps)
    (ids, _, cnt), line["top_views_ms"] = event_ms(lambda: CI.top_views(S, NUM_SRC), args.reps)
    dr, line["depth_ranks_ms"] = event_ms(depth, args.reps)
    line["gpu_total_ms"] = round(line["pair_scores_ms"] + line["top_views_ms"] + line["depth_ranks_ms"], 4)
    line["two_runs_bit_identical"] = bool(torch.equal(S.view(torch.int64), scores().view(torch.int64)))
    if args.rocprof:
        os.makedirs(args.rocprof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.abspath(args.rocprof), "-o", "colmap_import",
               "--", sys.executable, os.path.abspath(__file__), "--one-pass"]
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=900)
        if p.returncode == 0:
            from tools.dtu_eval_bench import kernel_stats
            line["kernels"] = kernel_stats(args.rocprof)
        else:
            line["kernels"] = f"rocprofv3 exit {p.returncode}"
    if args.no_cpu_baseline:
        line["cpu_baseline"] = "not measured"
    else:
        import colmap_oracle as O
        t0 = time.perf_counter()
        want, common = O.pair_scores(A["centres"], A["points"], A["offsets"], A["ids"])
        t1 = time.perf_counter()
        lists, wcnt = O.top_views(want, NUM_SRC)
        t2 = time.perf_counter()
        wdr = O.depth_ranks(A["points"], zrows, A["offsets"], A["ids"], ranks)
        t3 = time.perf_counter()
        got = S.cpu().numpy()
        same_lists = [[j for j in row if j >= 0] for row in ids.cpu().numpy().tolist()] == lists
        line["cpu_baseline"] = {"what": "tests/colmap_oracle.py (numpy, one process) on the same model, same host",
                                "pair_scores_ms": round((t1 - t0) * 1e3, 1), "top_views_ms": round((t2 - t1) * 1e3, 1),
                                "depth_ranks_ms": round((t3 - t2) * 1e3, 1), "total_ms": round((t3 - t0) * 1e3, 1)}
        line["vs_oracle"] = {"max_score_error_over_bound": float((np.abs(got - want) / (1e-12 * (1 + common))).max()),
                             "top_lists_equal": bool(same_lists), "counts_equal": bool(np.array_equal(cnt.cpu().numpy(), wcnt)),
                             "depth_ranks_bit_identical": bool(np.array_equal(dr.cpu().numpy().view(np.int64), wdr.view(np.int64)))}
    if args.phases == "all":
        line["undistort"] = undistort_phase(args.reps, not args.no_cpu_baseline, dev)
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
