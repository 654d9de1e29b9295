#!/usr/bin/env python
"""Generate tests/golden/tanks_eval.npz by IMPORTING THE REFERENCE: ``write_depth_img_2`` of eval_rcmvsnet_tanks.py (imported the
way make_golden.import_reference_eval does: cv2 / plyfile stubbed, matplotlib is installed so the function runs as shipped) is
called on seeded depth maps and the PNG it writes is read back.  ``vmin`` / ``vmax`` are the two numbers that function forms
(``depth.min()`` and ``np.percentile(depth, 95)``), recorded from the same numpy.  Nothing of the reference is copied -- the file
holds seeds, depth maps, images, scalars and version strings only.

Small cases are stored in full (map + image):
  ramp      64 x 96    smooth ramp + noise
  outliers  120 x 160  the synthetic surface with 3 % far outliers
  r33x47, r1x7, r5x1   ragged sizes
  constant  8 x 8      vmin == vmax
  ties      40 x 50    12 % of the pixels equal the 95th-percentile value exactly (ties across the selected rank)
  int21     3 x 7      (n - 1) * 0.95 is an integer (19)
  frac42    6 x 7      (n - 1) * 0.95 is not (38.95)
  narrow    48 x 64    2 000 +- 0.01: the rounding of vmax - vmin and of the division shows
  narrow2   48 x 64    a narrow range at 1 000.37 whose ends are not multiples of the fp32 spacing's power of two
  nan       16 x 20    one NaN
  one       1 x 1
  wide      48 x 64    0.3 .. 1 854.77 (within a factor of two of vmin, d - vmin and vmax - vmin are exact in any precision;
                       here they round), seeded with values at which an fp64 Normalize picks another table entry than the fp32
                       one -- the case that pins the fp32 form
The full-size case (1056 x 1920, ``synthetic.depth_vis_map(1056, 1920, seed)``) stores the seed, vmin, vmax, every 16th row and
column of the image and the CRC-32 of the whole image, as validation.npz does for its items.

    python tests/golden/make_golden_tanks_eval.py        (the reference checkout where make_golden.py expects it)
"""
import os
import sys
import tempfile
import zlib

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from rc_mvsnet_amd import synthetic  # noqa: E402

FULL = dict(H=1056, W=1920, seed=11)


def cases():
    rng = np.random.default_rng(7)
    out = {}
    ys, xs = np.meshgrid(np.arange(64.0), np.arange(96.0), indexing="ij")
    out["ramp"] = (400.0 + 3.0 * xs + 1.5 * ys + 0.5 * rng.standard_normal((64, 96))).astype(np.float32)
    out["outliers"] = synthetic.depth_vis_map(120, 160, seed=3)
    out["r33x47"] = synthetic.depth_vis_map(33, 47, seed=4)
    out["r1x7"] = synthetic.depth_vis_map(1, 7, seed=5, outliers=0.0)
    out["r5x1"] = synthetic.depth_vis_map(5, 1, seed=6, outliers=0.0)
    out["constant"] = np.full((8, 8), 731.25, dtype=np.float32)
    t = (500.0 + 200.0 * rng.random((40, 50))).astype(np.float32)
    order = np.argsort(t.ravel())
    t.ravel()[order[1780:2020]] = t.ravel()[order[1900]]            # ranks 1780 .. 2019 of 2000 hold one value; the 95 % rank is 1899.05
    out["ties"] = t
    out["int21"] = synthetic.depth_vis_map(3, 7, seed=8, outliers=0.0)
    out["frac42"] = synthetic.depth_vis_map(6, 7, seed=9, outliers=0.0)
    out["narrow"] = (2000.0 + 0.01 * (2.0 * rng.random((48, 64)) - 1.0)).astype(np.float32)
    out["narrow2"] = (1000.37 + 0.003 * rng.random((48, 64))).astype(np.float32)
    n = synthetic.depth_vis_map(16, 20, seed=10)
    n[5, 7] = np.nan
    out["nan"] = n
    out["one"] = np.full((1, 1), 3.5, dtype=np.float32)
    out["wide"] = wide_case(rng)
    return out


def wide_case(rng):
    """vmin = 0.3, vmax = 1 854.77 by construction (a plateau of 300 equal values across the 95 % rank), and among the rest every
    value of 4 M seeded draws at which Normalize in fp64 lands on another table entry than in fp32 (a few dozen), padded with draws."""
    vmin, vmax = np.float32(0.3), np.float32(1854.77)
    cand = rng.uniform(float(vmin), float(vmax), 4_000_000).astype(np.float32)
    i32 = np.trunc((cand - vmin) / np.float32(vmax - vmin) * np.float32(256))
    i64 = np.trunc(((cand.astype(np.float64) - np.float64(vmin)) / (np.float64(vmax) - np.float64(vmin))).astype(np.float32) * np.float32(256))
    tell = cand[i32 != i64][:400]
    assert len(tell) >= 8, len(tell)
    n = 48 * 64
    vals = np.concatenate([[vmin], tell, np.full(300, vmax, np.float32)])
    vals = np.concatenate([vals, cand[:n - len(vals)]]).astype(np.float32)
    rng.shuffle(vals)
    assert np.sort(vals)[int(0.95 * (n - 1))] == vmax == np.sort(vals)[int(0.95 * (n - 1)) + 1]
    return vals.reshape(48, 64)


def reference_image(mod, depth, folder, name):
    path = os.path.join(folder, "depth_est", name + ".pfm.png")
    mod.write_depth_img_2(path, depth)
    img = np.array(Image.open(path))
    assert img.dtype == np.uint8 and img.shape == depth.shape + (3,), (img.dtype, img.shape)
    return img


def main():
    import matplotlib
    import make_golden
    mod, _ = make_golden.import_reference_eval("eval_rcmvsnet_tanks")
    arrays = {"numpy_version": np.array(np.__version__), "matplotlib_version": np.array(matplotlib.__version__),
              "percentile": np.array(95.0)}
    all_cases = cases()
    arrays["cases"] = np.array(sorted(all_cases))
    with tempfile.TemporaryDirectory() as d:
        for name, depth in all_cases.items():
            arrays["case:%s:depth" % name] = depth
            outcome = "image"
            try:
                with np.errstate(all="ignore"):
                    arrays["case:%s:image" % name] = reference_image(mod, depth, d, name)
                    arrays["case:%s:vminmax" % name] = np.array([depth.min(), np.percentile(depth, 95)], dtype=np.float32)
            except Exception as e:                                   # noqa: BLE001 -- what the reference does with this map is the record
                outcome = "raises:" + type(e).__name__
            arrays["case:%s:outcome" % name] = np.array(outcome)
            print(name, depth.shape, outcome, arrays.get("case:%s:vminmax" % name))
        depth = synthetic.depth_vis_map(FULL["H"], FULL["W"], FULL["seed"])
        img = reference_image(mod, depth, d, "full")
        arrays["full:dims"] = np.array([FULL["H"], FULL["W"], FULL["seed"]])
        arrays["full:vminmax"] = np.array([depth.min(), np.percentile(depth, 95)], dtype=np.float32)
        arrays["full:image"] = img[::16, ::16]
        arrays["full:crc"] = np.array(zlib.crc32(np.ascontiguousarray(img).tobytes()), dtype=np.int64)
        arrays["full:depth_crc"] = np.array(zlib.crc32(np.ascontiguousarray(depth).tobytes()), dtype=np.int64)
        print("full", img.shape, arrays["full:vminmax"], int(arrays["full:crc"]))
    path = os.path.join(HERE, "tanks_eval.npz")
    np.savez_compressed(path, **arrays)
    print("tanks_eval.npz  %.1f KiB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
