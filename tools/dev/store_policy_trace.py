"""Per-family durations and boundary gaps of the bench scene from a rocprofv3 --kernel-trace CSV.

usage: python tools/dev/store_policy_trace.py <tag>=<kernel_trace.csv> [<tag>=<csv> ...] [--scenes 60]

A scene is the run of dispatches from one FeatureNet stem launch to the next.  The last `--scenes` complete scenes of each trace are
used.  Per kernel family the table gives, per scene, the sum of the dispatch durations and the sum of the gaps that FOLLOW its dispatches
(end of the dispatch to the start of the next one of the same scene): the write-back of a kernel's dirty lines is paid between its end
and its successor's start.  The gap after a scene's last dispatch (the host's turn) is left out.
"""
import csv
import re
import sys
from collections import defaultdict

FAMILIES = (("stem", r"conv2d_stem"), ("pair", r"conv2d_pair"), ("tile", r"conv2d_tile"), ("fpn", r"fpn_"), ("conv2d", r"conv2d_lds|conv1x1"),
            ("K1", r"warp_variance"), ("z8", r"conv3d_z8"), ("zs2", r"conv3d_zs2"), ("deep", r"conv3d_deep"), ("x3", r"conv3d_x3"),
            ("prob", r"prob_pair|conv11_prob"), ("head", r"softmax|depth_head|regress"), ("planes", r"plane|homography"))


def family(name):
    for fam, pat in FAMILIES:
        if re.search(pat, name):
            return fam
    return "other"


def load(path):
    with open(path, newline="") as f:
        rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f)]
    rows.sort(key=lambda r: r[1])
    return rows


def scenes_of(rows, count):
    starts = [i for i, r in enumerate(rows) if "conv2d_stem_kernel" in r[0]]
    if len(starts) < count + 1:
        raise SystemExit(f"only {len(starts)} scenes in the trace")
    starts = starts[-(count + 1):]
    return [rows[a:b] for a, b in zip(starts[:-1], starts[1:])]


def table(rows, count):
    dur, gap, launches = defaultdict(float), defaultdict(float), defaultdict(int)
    span = 0.0
    scenes = scenes_of(rows, count)
    for sc in scenes:
        span += (sc[-1][2] - sc[0][1]) / 1e3
        for i, (name, t0, t1) in enumerate(sc):
            fam = family(name)
            dur[fam] += (t1 - t0) / 1e3
            launches[fam] += 1
            if i + 1 < len(sc):
                gap[fam] += (sc[i + 1][1] - t1) / 1e3
    n = len(scenes)
    return {f: (launches[f] / n, dur[f] / n, gap[f] / n) for f in dur}, span / n


def main(argv):
    count = 60
    if "--scenes" in argv:
        i = argv.index("--scenes")
        count = int(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
    tabs = []
    for arg in argv:
        tag, path = arg.split("=", 1)
        tabs.append((tag,) + table(load(path), count))
    fams = [f for f, _ in FAMILIES] + ["other"]
    print(f"us per scene, mean of the last {count} scenes: launches, sum of durations, sum of the gaps after the family's dispatches")
    print("family   " + "".join(f"| {tag:>10s}: n    dur    gap " for tag, _, _ in tabs))
    for f in fams:
        if not any(f in t for _, t, _ in tabs):
            continue
        line = f"{f:8s} "
        for _, t, _ in tabs:
            n, d, g = t.get(f, (0, 0.0, 0.0))
            line += f"| {'':10s} {n:4.1f} {d:7.1f} {g:6.1f} "
        print(line)
    line = "total    "
    for _, t, span in tabs:
        line += f"| {'':10s} {sum(v[0] for v in t.values()):4.0f} {sum(v[1] for v in t.values()):7.1f} {sum(v[2] for v in t.values()):6.1f} "
    print(line)
    print("first start to last end of a scene: " + "  ".join(f"{tag} {span:.1f}" for tag, _, span in tabs))


if __name__ == "__main__":
    main(sys.argv[1:])
