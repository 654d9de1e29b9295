"""The dynamic fusion launch (rcmvs_fuse_view_dyn, duplicate suppression off and on) against the fixed one (rcmvs_fuse_view, the
yardstick) at the DTU evaluation shape (1184 x 1600, 4 source views) and a Tanks-and-Temples-sized one (1056 x 1920, 10 source views):
each launch between two events on its stream, the three alternating in the same process after a warm-up, the median of 5, next to
its floor of compulsory bytes at 8 TB/s.  Also the points and claimed pixels of a whole scan under the four mode combinations, and
the numpy oracle's time for one view of a 64 x 48 crop.  Writes profiles/fusion_dynamic_bench.json (or --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rc_mvsnet_amd import _lib, fusion, synthetic        # noqa: E402

PROB, NCONS, DIST, DEPTH = 0.8, 3, 0.5, 0.01
HBM_BYTES_PER_S = 8e12
REPEATS = 5


def load(s, dev):
    depth_all = torch.from_numpy(s["depth"]).to(dev)
    jobs = []
    for ref, srcs in s["pairs"]:
        mats = torch.from_numpy(fusion.fusion_matrices(s["K"][ref], s["E"][ref], [s["K"][i] for i in srcs], [s["E"][i] for i in srcs])).to(dev)
        jobs.append((ref, srcs, torch.from_numpy(s["conf"][ref]).to(dev), torch.from_numpy(s["img"][ref].astype(np.float32) / 255.0).to(dev), mats))
    return depth_all, jobs


def floors(H, W, N, kept):
    """compulsory bytes of one launch: the reference and the N source depth maps once, confidence, image; masks, depth_avg, xyz, rgb.
    The dynamic launch writes one more mask plane and the level plane; with suppression it reads one `used` byte per pixel and
    stores at most N bytes per kept pixel."""
    px = H * W
    fixed = px * ((N + 1) * 4 + 4 + 12) + px * (3 + 4 + 12 + 3)
    dyn = fixed + px * 2
    return {"reference": fixed, "dynamic": dyn, "dynamic_dedup": dyn + px + N * kept}


def time_launches(depth_all, jobs):
    ref, srcs, conf, img, mats = jobs[0]
    used = torch.zeros(depth_all.shape, device=depth_all.device, dtype=torch.uint8)
    calls = {"reference": lambda: fusion.fuse_view(depth_all, ref, srcs, conf, img, mats, PROB, NCONS, DIST, DEPTH),
             "dynamic": lambda: fusion.fuse_view_dynamic(depth_all, ref, srcs, conf, img, mats, PROB),
             "dynamic_dedup": lambda: fusion.fuse_view_dynamic(depth_all, ref, srcs, conf, img, mats, PROB, used=used)}
    for call in calls.values():                                          # warm-up: code objects loaded, the allocator's blocks in place
        call()
        call()
    torch.cuda.synchronize()
    busy = torch.empty(1 << 30, device=depth_all.device, dtype=torch.uint8)
    ms = {k: [] for k in calls}
    for _ in range(REPEATS):
        for k, call in calls.items():
            used.zero_()
            busy.zero_()                                                 # keeps the device busy while the host queues what follows, so that the
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)      # events bracket the kernel and not the wrapper's Python
            a.record()
            r = call()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    kept = int(r["masks"][2].sum())
    return ms, kept


def scan_modes(depth_all, jobs):
    """points and claimed pixels of the whole scan, reference views in pair order, under the four combinations"""
    out = {}
    for method in fusion.METHODS:
        for dedup in (False, True):
            used = torch.zeros(depth_all.shape, device=depth_all.device, dtype=torch.uint8) if dedup else None
            points = claimed = 0
            for ref, srcs, conf, img, mats in jobs:
                if method == "reference" and not dedup:
                    r = fusion.fuse_view(depth_all, ref, srcs, conf, img, mats, PROB, NCONS, DIST, DEPTH)
                else:
                    r, _ = fusion._fuse_dyn(depth_all, ref, srcs, conf, img, mats, PROB, method, None, (NCONS, DIST, DEPTH), used)
                    claimed += int(r["masks"][3].sum())
                points += int(r["masks"][2].sum())
            out[method + ("+dedup" if dedup else "")] = {"points": points, "claimed": claimed}
    return out


def oracle_time():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fusion_dyn_oracle as DO
    s = synthetic.fusion_scan(V=5, H=48, W=64, seed=0, n_src=4)
    ref, srcs = s["pairs"][0]
    mats = fusion.fusion_matrices(s["K"][ref], s["E"][ref], [s["K"][i] for i in srcs], [s["E"][i] for i in srcs])
    used = np.zeros(s["depth"].shape, np.uint8)
    best = float("inf")
    for _ in range(3):
        t = time.perf_counter()
        DO.fuse_view_dyn_exact(s["depth"], ref, srcs, s["conf"][ref], s["img"][ref].astype(np.float32) / np.float32(255.0), mats, PROB, 2, 4, 0.25, 1.0 / 1300.0, used)
        best = min(best, time.perf_counter() - t)
    return best * 1e3


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fusion_dynamic_bench.json"))
    args = ap.parse_args(argv)
    _lib.load()
    dev = "cuda:0"
    result = {"device": torch.cuda.get_device_name(0), "repeats": REPEATS, "hbm_bytes_per_s": HBM_BYTES_PER_S, "timing": "one launch between two events on its "
              "stream, queued behind a 1 GiB fill so that the events bracket the kernel and not the wrapper's Python; reference / dynamic / dynamic+dedup "
              "alternate in one process after a warm-up; median of the repeats; the caches are cold for all three", "shapes": {}}
    for name, (V, H, W, n_src) in (("dtu_1184x1600_4src", (5, 1184, 1600, 4)), ("tanks_1056x1920_10src", (11, 1056, 1920, 10))):
        s = synthetic.fusion_scan(V=V, H=H, W=W, seed=0, n_src=n_src)
        depth_all, jobs = load(s, dev)
        ms, kept = time_launches(depth_all, jobs)
        fl = floors(H, W, n_src, kept)
        entry = {}
        for k in ms:
            med = float(np.median(ms[k]))
            entry[k] = {"ms_median": med, "ms_all": [float(x) for x in ms[k]], "spread_ms": float(max(ms[k]) - min(ms[k])), "bytes_floor": int(fl[k]),
                        "floor_ms": fl[k] / HBM_BYTES_PER_S * 1e3, "times_floor": med / (fl[k] / HBM_BYTES_PER_S * 1e3)}
        for k in ("dynamic", "dynamic_dedup"):
            entry[k]["ratio_to_reference"] = entry[k]["ms_median"] / entry["reference"]["ms_median"]
            entry[k]["ratio_of_floors"] = fl[k] / fl["reference"]
            budget = entry["reference"]["ms_median"] * entry[k]["ratio_of_floors"] + entry["reference"]["spread_ms"] + entry[k]["spread_ms"]
            entry[k]["within_scaled_reference"] = bool(entry[k]["ms_median"] <= budget)
        entry["whole_scan"] = scan_modes(depth_all, jobs)
        result["shapes"][name] = entry
        print(name, json.dumps(entry), flush=True)
        del depth_all, jobs
    result["oracle_ms_64x48_view"] = oracle_time()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
