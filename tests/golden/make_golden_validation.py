#!/usr/bin/env python
"""Generate tests/golden/validation.npz by IMPORTING THE REFERENCE (environment variable REFERENCE_ROOT = its checkout): the
validation loader datasets/dtu_yao.py ``MVSDataset(..., "test", 5)`` on the folder ``synthetic.write_dtu_train_folder``
writes, and utils.Thres_metrics / AbsDepthError_metrics / models.modules.cas_mvsnet_loss on seeded (estimate, ground truth,
mask) triples.  Nothing of the reference is copied -- the file holds recorded items and scalars only.

Shims, as in make_golden_train_dataset.py (cv2 and torchvision are not installed where this runs): ``cv2.resize`` = nearest
neighbour with OpenCV's rule (source index floor(dst * src_size / dst_size)); empty torchvision modules.

Stored: two items -- proj_matrices and depth_values in full; imgs as every 16th row and column, depth / mask stages as every
8th, each with the CRC-32 of the full array's bytes, which pins the rest.  Four metric cases -- the triples in full and the
12 scalars test_sample_depth forms from them (fp32, as the reference computes them):
  mixed   errors on both sides of 1 mm and in every band
  exact   errors of exactly 0, 1, 2, 4 and 8 mm (gt = est -+ T with est a multiple of 0.5: the fp32 subtraction is exact,
          asserted here), which the inclusive band ends and the strict thresholds treat differently
  empty   no error in [2, 8]: two empty bands
  odd     stage sizes that are not multiples of 4
every mask holds the values 0, 0.5, 0.500001 and 1.

    REFERENCE_ROOT=<RC-MVSNet checkout> python tests/golden/make_golden_validation.py
"""
import importlib
import os
import sys
import tempfile
import types
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from rc_mvsnet_amd import synthetic  # noqa: E402

FOLDER = dict(scans=["scan1", "scan2"], n_views=5, seed=0)      # the folder of the training-loader golden
NVIEWS = 5
DLOSSW = [0.5, 1.0, 2.0]
SCALAR_KEYS = ("loss", "depth_loss", "abs_depth_error", "thres2mm_error", "thres4mm_error", "thres8mm_error",
               "thres2mm_accu", "thres4mm_accu", "thres8mm_accu", "thres2mm_abserror", "thres4mm_abserror", "thres8mm_abserror")
MASK_VALUES = np.array([0.0, 0.5, 0.500001, 1.0, 1.0, 1.0], dtype=np.float32)


def nearest_resize(img, dsize=None, fx=None, fy=None, interpolation=0):
    h, w = img.shape[:2]
    ow, oh = dsize if dsize is not None else (int(round(w * fx)), int(round(h * fy)))
    ys = np.minimum(np.floor(np.arange(oh) * (h / oh)).astype(np.int64), h - 1)
    xs = np.minimum(np.floor(np.arange(ow) * (w / ow)).astype(np.int64), w - 1)
    return np.ascontiguousarray(img[ys][:, xs])


def import_reference():
    if "REFERENCE_ROOT" not in os.environ:
        raise SystemExit("set REFERENCE_ROOT to a checkout of the reference (RC-MVSNet)")
    cv2 = types.ModuleType("cv2")
    cv2.INTER_NEAREST, cv2.COLORMAP_JET = 0, 2
    cv2.resize = nearest_resize
    sys.modules["cv2"] = cv2
    for n in ("torchvision", "torchvision.transforms", "torchvision.utils"):
        sys.modules.setdefault(n, types.ModuleType(n))
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    sys.modules["torchvision"].utils = sys.modules["torchvision.utils"]
    sys.path.insert(0, os.environ["REFERENCE_ROOT"])
    return (importlib.import_module("datasets.dtu_yao"), importlib.import_module("utils"), importlib.import_module("models.modules"))


def metric_cases():
    """name -> [(est, gt, mask)] x 3 stages, fp32 (h, w) arrays"""
    rng = np.random.default_rng(2024)

    def stage(shape, err):
        est = (600.0 + 100.0 * rng.random(shape)).astype(np.float32)
        gt = (est + err(shape)).astype(np.float32)
        mask = MASK_VALUES[rng.integers(0, len(MASK_VALUES), shape)]
        mask.ravel()[:4] = MASK_VALUES[:4]
        return est, gt, mask

    def mixed(shape):
        return rng.choice([0.3, 1.5, 3.0, 6.0, 12.0], shape) * rng.standard_normal(shape)

    def empty(shape):
        return np.where(rng.random(shape) < 0.5, 1.9 * (2.0 * rng.random(shape) - 1.0), 8.5 + 10.0 * rng.random(shape))

    cases = {"mixed": [stage(s, mixed) for s in ((8, 10), (16, 20), (32, 40))],
             "empty": [stage(s, empty) for s in ((8, 10), (16, 20), (32, 40))],
             "odd": [stage(s, mixed) for s in ((7, 9), (13, 19), (27, 37))]}
    exact = []
    for shape in ((8, 10), (16, 20), (32, 40)):
        est = (600.0 + 0.5 * rng.integers(0, 200, shape)).astype(np.float32)
        step = rng.choice([0.0, 1.0, 2.0, 4.0, 8.0, 0.5, 3.0, 5.0, 9.0], shape).astype(np.float32) * rng.choice([-1.0, 1.0], shape).astype(np.float32)
        gt = (est + step).astype(np.float32)
        assert np.array_equal(est - gt, -step) and (est - gt).dtype == np.float32          # the fp32 subtraction is exact
        mask = MASK_VALUES[rng.integers(0, len(MASK_VALUES), shape)]
        mask.ravel()[:4] = MASK_VALUES[:4]
        exact.append((est, gt, mask))
    e = np.abs(exact[2][0] - exact[2][1])[exact[2][2] > 0.5]
    assert all((e == t).any() for t in (0.0, 1.0, 2.0, 4.0, 8.0))
    cases["exact"] = exact
    e = np.abs(cases["empty"][2][0] - cases["empty"][2][1])
    assert not ((e >= 2.0) & (e <= 8.0)).any()
    return cases


def reference_scalars(utils, modules, triples):
    """the scalar_outputs of test_sample_depth (train_rcmvsnet.py:468-487) on CPU tensors"""
    t = [[torch.from_numpy(a)[None] for a in tr] for tr in triples]
    outputs = {"stage%d" % (k + 1): {"depth": t[k][0]} for k in range(3)}
    depth_gt_ms = {"stage%d" % (k + 1): t[k][1] for k in range(3)}
    mask_ms = {"stage%d" % (k + 1): t[k][2] for k in range(3)}
    loss, depth_loss = modules.cas_mvsnet_loss(outputs, depth_gt_ms, mask_ms, dlossw=DLOSSW)
    est, gt, mask = t[2]
    m = mask > 0.5
    s = {"loss": loss, "depth_loss": depth_loss, "abs_depth_error": utils.AbsDepthError_metrics(est, gt, m)}
    for thres, band in ((2, [0, 2.0]), (4, [2.0, 4.0]), (8, [4.0, 8.0])):
        s["thres%dmm_error" % thres] = utils.Thres_metrics(est, gt, m, thres)
        s["thres%dmm_accu" % thres] = 1 - utils.Thres_metrics(est, gt, m, thres)
        s["thres%dmm_abserror" % thres] = utils.AbsDepthError_metrics(est, gt, m, band)
    return np.array([float(s[k]) for k in SCALAR_KEYS], dtype=np.float32)


def main():
    dtu_yao, utils, modules = import_reference()
    arrays = {"nviews": np.array(NVIEWS), "n_views_folder": np.array(FOLDER["n_views"]), "seed": np.array(FOLDER["seed"]),
              "scans": np.array(FOLDER["scans"]), "dlossw": np.array(DLOSSW), "scalar_keys": np.array(SCALAR_KEYS)}
    cases = metric_cases()
    arrays["cases"] = np.array(sorted(cases))
    for name, triples in cases.items():
        for k, (est, gt, mask) in enumerate(triples):
            arrays["case:%s:est%d" % (name, k + 1)], arrays["case:%s:gt%d" % (name, k + 1)] = est, gt
            arrays["case:%s:mask%d" % (name, k + 1)] = mask
        arrays["case:%s:scalars" % name] = reference_scalars(utils, modules, triples)
    with tempfile.TemporaryDirectory() as d:
        lst = synthetic.write_dtu_train_folder(d, **FOLDER)
        ds = dtu_yao.MVSDataset(d, lst, "test", NVIEWS, 192, 1.06)
        arrays["len"] = np.array(len(ds))
        items = (0, len(ds) - 1)
        arrays["items"] = np.array(items)
        for idx in items:
            item = ds[idx]
            tag = "%d:" % idx
            dense = {"imgs": (item["imgs"], 16)}
            for k in ("depth", "mask"):
                for s, v in item[k].items():
                    dense[k + ":" + s] = (v, 8)
            for k, (v, step) in dense.items():
                arrays[tag + k] = v[..., ::step, ::step]
                arrays[tag + k + ":crc"] = np.array([zlib.crc32(np.ascontiguousarray(v).tobytes())] + list(v.shape), dtype=np.int64)
                arrays[tag + k + ":dtype"] = np.array(str(v.dtype))
            for s, v in item["proj_matrices"].items():
                arrays[tag + "proj_matrices:" + s] = v
            arrays[tag + "depth_values"] = np.asarray(item["depth_values"])
    path = os.path.join(HERE, "validation.npz")
    np.savez_compressed(path, **arrays)
    print("validation.npz  %.1f KiB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
