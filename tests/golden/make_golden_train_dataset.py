#!/usr/bin/env python
"""Generate tests/golden/train_dataset.npz by IMPORTING THE REFERENCE's training loader (datasets/dtu_train.py ``MVSDataset``)
and running it on the folder ``synthetic.write_dtu_train_folder`` writes.  Needs the reference tree (environment variable
REFERENCE_ROOT = its checkout); nothing of it is copied -- the file holds recorded items only.

Shims, in the style of make_golden.py (cv2 and torchvision are not installed where this runs):
* ``cv2.resize`` = nearest neighbour with OpenCV's rule (source index floor(dst * src_size / dst_size)); ``cv2.imread`` /
  ``cv2.cvtColor`` through Pillow.
* ``torchvision.transforms``: Compose; ToTensor / Normalize = the torch ops of tests/train_dataset_oracle.py; ``ColorJitter``
  draws its parameters in torchvision's ranges (rounded to fp32, which is what the kernels take), RECORDS them and calls the
  oracle's Pillow calls.  The reference's own ``RandomGamma`` is replaced by a twin that records the gamma it draws.
* numpy >= 1.24 refuses ``np.stack`` of the ragged (matrix, [near, far]) pairs of build_proj_mats; the loader module sees a
  numpy whose ``stack`` builds the object array older numpy versions made of them.

Stored: every non-image key of two items; the recorded parameters; for imgs / imgs_aug / center_imgs every 16th row and
column.  The depth-like keys (depths_h, depth, mask: 9 MB per item in full) are stored as every 8th row and column plus the
CRC-32 of the full array's bytes, which pins the rest.

    REFERENCE_ROOT=<RC-MVSNet checkout> python tests/golden/make_golden_train_dataset.py
"""
import importlib
import os
import sys
import tempfile
import types
import zlib

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import train_dataset_oracle as O  # noqa: E402
from rc_mvsnet_amd import synthetic  # noqa: E402

FOLDER = dict(scans=["scan1", "scan2"], n_views=5, seed=0)      # what tests/test_train_dataset_cpu.py writes again
NVIEWS = 4
RECORD = []                                                     # one dict per transform_aug call, in call order


def nearest_resize(img, dsize=None, fx=None, fy=None, interpolation=0):
    h, w = img.shape[:2]
    ow, oh = dsize if dsize is not None else (int(round(w * fx)), int(round(h * fy)))
    ys = np.minimum(np.floor(np.arange(oh) * (h / oh)).astype(np.int64), h - 1)
    xs = np.minimum(np.floor(np.arange(ow) * (w / ow)).astype(np.int64), w - 1)
    return np.ascontiguousarray(img[ys][:, xs])


class ColorJitter:
    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0):
        self.ranges = ((max(0.0, 1 - brightness), 1 + brightness), (max(0.0, 1 - contrast), 1 + contrast),
                       (max(0.0, 1 - saturation), 1 + saturation), (-hue, hue))
        self.rng = np.random.default_rng(1234)

    def __call__(self, img):
        order = self.rng.permutation(4)
        factors = np.array([self.rng.uniform(lo, hi) for lo, hi in self.ranges]).astype(np.float32)
        RECORD.append({"order": order.astype(np.int32), "factors": factors})
        return Image.fromarray(O.color_jitter(np.array(img.convert("RGB"), dtype=np.uint8), order, factors))


class RandomGamma:
    def __init__(self, min_gamma=0.7, max_gamma=1.5, clip_image=False):
        self.lo, self.hi, self.clip = min_gamma, max_gamma, clip_image

    def __call__(self, img):
        gamma = np.random.uniform(self.lo, self.hi)
        RECORD[-1]["gamma"] = gamma
        out = torch.pow(img, gamma)
        if self.clip:
            out.clamp_(0.0, 1.0)
        return out


class Compose:
    def __init__(self, ts):
        self.ts = ts

    def __call__(self, x):
        for t in self.ts:
            x = t(x)
        return x


class Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, t):
        return O.normalize(t, self.mean, self.std)


class RaggedNumpy:
    """numpy, except that stack() of ragged rows gives the object array numpy < 1.24 gave"""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def stack(arrays, *a, **k):
        try:
            return np.stack(arrays, *a, **k)
        except ValueError:
            out = np.empty((len(arrays), len(arrays[0])), dtype=object)
            for i, row in enumerate(arrays):
                for j, x in enumerate(row):
                    out[i, j] = x
            return out


def import_reference_loader():
    cv2 = types.ModuleType("cv2")
    cv2.INTER_NEAREST, cv2.COLOR_BGR2RGB = 0, 4
    cv2.resize = nearest_resize
    cv2.imread = lambda name: np.array(Image.open(name).convert("RGB"), dtype=np.uint8)[..., ::-1]
    cv2.cvtColor = lambda img, code: np.ascontiguousarray(img[..., ::-1])
    sys.modules["cv2"] = cv2
    tv, tr = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tr.Compose, tr.Normalize, tr.ColorJitter = Compose, Normalize, ColorJitter
    tr.ToTensor = lambda: (lambda img: O.to_tensor(np.array(img, dtype=np.uint8)))
    tv.transforms = tr
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr
    if "REFERENCE_ROOT" not in os.environ:
        raise SystemExit("set REFERENCE_ROOT to a checkout of the reference (RC-MVSNet)")
    sys.path.insert(0, os.environ["REFERENCE_ROOT"])
    mod = importlib.import_module("datasets.dtu_train")
    mod.RandomGamma = RandomGamma
    mod.np = RaggedNumpy()
    return mod


def main():
    mod = import_reference_loader()
    np.random.seed(4321)
    arrays = {"nviews": np.array(NVIEWS), "n_views_folder": np.array(FOLDER["n_views"]), "seed": np.array(FOLDER["seed"]),
              "scans": np.array(FOLDER["scans"])}
    with tempfile.TemporaryDirectory() as d:
        lst = synthetic.write_dtu_train_folder(d, **FOLDER)
        ds = mod.MVSDataset(d, lst, "train", NVIEWS, 192, 1.06)
        arrays["len"] = np.array(len(ds))
        items = (0, len(ds) - 1)
        arrays["items"] = np.array(items)
        for idx in items:
            del RECORD[:]
            item = ds[idx]
            assert len(RECORD) == NVIEWS
            tag = "%d:" % idx
            arrays[tag + "aug_order"] = np.stack([r["order"] for r in RECORD])
            arrays[tag + "aug_factors"] = np.stack([r["factors"] for r in RECORD])
            arrays[tag + "aug_gamma"] = np.array([r["gamma"] for r in RECORD], dtype=np.float64)
            for k in ("imgs", "imgs_aug", "center_imgs"):
                full = np.stack([np.asarray(t) for t in item[k]])
                arrays[tag + k] = full[:, :, ::16, ::16]
            dense = {"depths_h": item["depths_h"]}
            for k in ("depth", "mask"):
                for s, v in item[k].items():
                    dense[k + ":" + s] = v
            for k, v in dense.items():
                arrays[tag + k] = v[..., ::8, ::8]
                arrays[tag + k + ":crc"] = np.array([zlib.crc32(np.ascontiguousarray(v).tobytes())] + list(v.shape), dtype=np.int64)
                arrays[tag + k + ":dtype"] = np.array(str(v.dtype))
            for s, v in item["proj_matrices"].items():
                arrays[tag + "proj_matrices:" + s] = v
            for k in ("depth_values", "w2cs", "c2ws", "near_fars", "proj_mats", "intrinsics", "view_ids", "light_id", "affine_mat",
                      "affine_mat_inv", "c2ws_all"):
                arrays[tag + k] = np.asarray(item[k])
            arrays[tag + "scan"] = np.array(item["scan"])
    path = os.path.join(HERE, "train_dataset.npz")
    np.savez_compressed(path, **arrays)
    print("train_dataset.npz  %.1f KiB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
