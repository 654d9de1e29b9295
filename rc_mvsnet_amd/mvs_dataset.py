"""Evaluation loaders for MVSNet-style scan folders: the test-mode ``MVSDataset`` of
datasets/dtu_test.py:11-229 and the Tanks-and-Temples one of datasets/tanks.py:11-186 (``TanksDataset`` here), with the
per-image work moved to the GPU.

Same constructor arguments, item order and item dict (``imgs`` (V,3,h,w), ``proj_matrices`` {stage1..3: (V,2,4,4)},
``depth_values`` (ndepths,), ``filename``) as the reference, so the loop of ``eval_rcmvsnet_dtu.py:174-197`` consumes the
items unchanged -- with ``DataLoader(num_workers=0)`` or the ``prefetch()`` iterator below: ``__getitem__`` launches HIP
kernels, so a forked loader worker (the reference's ``num_workers=1``) cannot run it ("Cannot re-initialize CUDA in forked
subprocess").  The
host parses the text files and decodes the JPEG; ``/255``, the ``cv2.resize`` of ``scale_mvs_input`` / the common-size resize,
``ToTensor`` and ``Normalize`` are one kernel per image (``rcmvs_prepare_image``) on the uploaded bytes -- that work costs the
reference's single loader worker ~10x the network's time per item.  ``imgs`` is therefore a CUDA tensor; everything else is
numpy like the reference's.  No CPU fallback: ``device`` must be a GPU.

``DTUTrainDataset`` is the training counterpart (datasets/dtu_train.py, ``--dataset dtu_train``): the host decodes every PNG
once and parses cameras / depth maps; ``imgs``, ``center_imgs`` and the colour-augmented ``imgs_aug`` of all views come from
two launches of csrc/train_aug.hip (``prepare_train_images``).  DESIGN.md section 4, "Training loader".

``DTUValDataset`` is the validation loader over the same folders (datasets/dtu_yao.py in mode "test", what the reference's
training script validates on): 5 views, images only divided by 255, the ground-truth depth and mask pyramids of the reference
view.  ``validation.validate`` consumes it.  DESIGN.md section 4, "Validation".
"""
import ctypes
import os

import numpy as np
import torch
from PIL import Image

from . import _lib, scan_io
from .data_io import read_pfm
from .ops import _chk, _stream

MEAN = (0.485, 0.456, 0.406)      # transforms.Normalize of datasets/dtu_test.py:78-81
STD = (0.229, 0.224, 0.225)


def scaled_size(h, w, max_h, max_w, base=32):
    """Target (new_h, new_w) of scale_mvs_input (datasets/dtu_test.py:127-137): fit inside (max_h, max_w), then round both
    sides down to a multiple of ``base``.  Floats, as the reference computes them."""
    if h > max_h or w > max_w:
        scale = 1.0 * max_h / h
        if scale * w > max_w:
            scale = 1.0 * max_w / w
        return scale * h // base * base, scale * w // base * base
    return 1.0 * h // base * base, 1.0 * w // base * base


def prepare_image(img_u8, out_hw, device, mean=MEAN, std=STD):
    """Decoded image (H,W,3) uint8 numpy -> (3,h,w) fp32 CUDA tensor, resized and normalised on the device
    (mean 0 / std 1 gives the plain resized image in [0,1])."""
    if img_u8.dtype != np.uint8 or img_u8.ndim != 3 or img_u8.shape[2] != 3:
        raise _lib.RcmvsError(f"prepare_image: expected an (H,W,3) uint8 image, got {img_u8.dtype} {img_u8.shape}")
    H, W = img_u8.shape[:2]
    h, w = int(out_hw[0]), int(out_hw[1])
    src = torch.from_numpy(np.ascontiguousarray(img_u8)).to(device, non_blocking=True)
    out = torch.empty((3, h, w), device=device, dtype=torch.float32)
    mean, std = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    _lib.call("rcmvs_prepare_image", _chk(src, "src", torch.uint8), _chk(out, "out"), H, W, h, w,
              ctypes.cast(mean, ctypes.c_void_p), ctypes.cast(std, ctypes.c_void_p), _stream())
    return out


class MVSDataset(torch.utils.data.Dataset):
    def __init__(self, datapath, listfile, mode, nviews, ndepths=192, interval_scale=1.06, device="cuda:0", **kwargs):
        super().__init__()
        assert mode == "test"
        self.datapath, self.listfile, self.mode, self.nviews, self.ndepths = datapath, listfile, mode, nviews, ndepths
        self.max_h, self.max_w = kwargs["max_h"], kwargs["max_w"]
        if kwargs.get("fix_res", False):
            raise ValueError("fix_res=True (one resolution latched for the whole list, datasets/dtu_test.py:201-205) is not provided: "
                             "every item is scaled by its own size, the reference's default")
        self.fix_res = False
        self.device = torch.device(device)
        self.interval_scale = {scan: (interval_scale if isinstance(interval_scale, float) else interval_scale[scan]) for scan in listfile}
        self.metas = self.build_list()

    def build_list(self):
        """[(scan, ref_view, src_views, scan)]; short source lists are padded with their first entry (dtu_test.py:28-57)."""
        metas = []
        for scan in self.listfile:
            for ref, srcs in scan_io.read_pair_file(os.path.join(self.datapath, "{}/pair.txt".format(scan))):
                if len(srcs) < self.nviews:
                    srcs = srcs + [srcs[0]] * (self.nviews - len(srcs))
                metas.append((scan, ref, srcs, scan))
        return metas

    def __len__(self):
        return len(self.metas)

    def load_host(self, idx):
        """Everything of item ``idx`` that needs no GPU: file parsing, JPEG decoding, target size, scaled intrinsics, depth values.
        Thread-safe (``prefetch`` runs it on worker threads; PIL releases the GIL while decoding)."""
        scan, ref_view, src_views, scene = self.metas[idx]
        view_ids = [ref_view] + src_views[:self.nviews - 1]
        raws, projs, depth_values, size = [], [], None, None
        for i, vid in enumerate(view_ids):
            name = os.path.join(self.datapath, "{}/images_post/{:0>8}.jpg".format(scan, vid))
            if not os.path.exists(name):
                name = os.path.join(self.datapath, "{}/images/{:0>8}.jpg".format(scan, vid))
            K, E, depth_min, depth_interval = scan_io.read_cam_file(
                os.path.join(self.datapath, "{}/cams/{:0>8}_cam.txt".format(scan, vid)), self.interval_scale[scene], self.ndepths)
            raw = np.array(Image.open(name), dtype=np.uint8)
            h0, w0 = raw.shape[:2]
            new_h, new_w = scaled_size(h0, w0, self.max_h, self.max_w)
            K[0, :] *= 1.0 * new_w / w0
            K[1, :] *= 1.0 * new_h / h0
            c_h, c_w = int(new_h), int(new_w)
            if i == 0:
                size = (c_h, c_w)
            elif (c_h, c_w) != size:
                # dtu_test.py:171-189 has a "resize to the standard size" branch, but it measures the already channels-first
                # tensor ((3, h) instead of (h, w)) and would hand that tensor to cv2.resize: views of one item must agree
                raise _lib.RcmvsError(f"view {vid} of {scan}: size {(c_h, c_w)} differs from the reference view's {size}")
            raws.append(raw)
            p = np.zeros((2, 4, 4), dtype=np.float32)
            p[0, :4, :4] = E
            p[1, :3, :3] = K
            projs.append(p)
            if i == 0:
                depth_values = np.arange(depth_min, depth_interval * (self.ndepths - 0.5) + depth_min, depth_interval, dtype=np.float32)
        return {"raw": raws, "size": size, "proj": np.stack(projs), "depth_values": depth_values,
                "filename": scan + "/{}/" + "{:0>8}".format(view_ids[0]) + "{}"}

    def to_device(self, host):
        return _finish_item(host, self.device)

    def __getitem__(self, idx):
        return self.to_device(self.load_host(idx))


def _finish_item(host, device):
    """The device half of an item: one rcmvs_prepare_image launch per view, then the three-stage projection matrices."""
    imgs = [prepare_image(raw, host["size"], device) for raw in host["raw"]]
    proj = host["proj"]
    stages = {"stage1": proj}
    for key, mul in (("stage2", 2), ("stage3", 4)):
        q = proj.copy()
        q[:, 1, :2, :] = proj[:, 1, :2, :] * mul
        stages[key] = q
    return {"imgs": torch.stack(imgs), "proj_matrices": stages, "depth_values": host["depth_values"], "filename": host["filename"]}


def prefetch(dataset, indices=None, workers=4, depth=8):
    """Items of ``dataset`` in order, with the host half (``load_host``: parsing + JPEG decoding, ~15 ms per 1200x1600 image, i.e.
    several times the network's time per item) of up to ``depth`` items running ahead on ``workers`` threads -- the reference's
    DataLoader(num_workers=1) serialises it with the GPU.  The device half runs on the calling thread / current stream."""
    from concurrent.futures import ThreadPoolExecutor
    idx = list(range(len(dataset))) if indices is None else list(indices)
    with ThreadPoolExecutor(max_workers=max(1, workers)) as pool:
        pending = []
        nxt = 0
        while nxt < len(idx) or pending:
            while nxt < len(idx) and len(pending) < max(1, depth):
                pending.append(pool.submit(dataset.load_host, idx[nxt]))
                nxt += 1
            host = pending.pop(0).result()                          # re-raises a worker's exception here, in order
            yield dataset.to_device(host)


class AsyncWriter:
    """Runs output writers (PFM / camera / JPEG files) on background threads so that disk I/O overlaps the next item's network
    pass; ``close()`` (or leaving the ``with`` block) waits for all of them and re-raises the first failure."""

    def __init__(self, workers=2):
        from concurrent.futures import ThreadPoolExecutor
        self.pool = ThreadPoolExecutor(max_workers=max(1, workers))
        self.jobs = []

    def submit(self, fn, *args, **kwargs):
        self.jobs.append(self.pool.submit(fn, *args, **kwargs))

    def close(self):
        jobs, self.jobs = self.jobs, []
        err = None
        for j in jobs:
            try:
                j.result()
            except Exception as e:                                  # noqa: BLE001 -- keep draining, report the first
                err = err or e
        self.pool.shutdown(wait=True)
        if err is not None:
            raise err

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:
            self.pool.shutdown(wait=True)
        return False


TANKS_SCANS = {     # scan -> (width, height) of the original images (datasets/tanks.py:24-48)
    "intermediate": {"Family": (1920, 1080), "Francis": (1920, 1080), "Horse": (1920, 1080), "Lighthouse": (2048, 1080),
                     "M60": (2048, 1080), "Panther": (2048, 1080), "Playground": (1920, 1080), "Train": (1920, 1080)},
    "advanced": {"Auditorium": (1920, 1080), "Ballroom": (1920, 1080), "Courtroom": (1920, 1080), "Museum": (1920, 1080),
                 "Palace": (1920, 1080), "Temple": (1920, 1080)},
}


class TanksDataset(torch.utils.data.Dataset):
    """datasets/tanks.py ``MVSDataset``: <datapath>/<split>/<scan>/{pair.txt, cams_1/, images/}; every image is resized to
    ``img_wh`` (no rounding to multiples of 32), the camera file's last line is ``depth_min depth_max`` and the ``ndepths``
    planes span exactly that range.  ``scans`` restricts the split's scan list (the reference always walks all of them)."""

    def __init__(self, datapath, split="intermediate", nviews=3, img_wh=(1920, 1056), ndepths=192, device="cuda:0", scans=None):
        super().__init__()
        self.datapath, self.split, self.nviews, self.img_wh, self.ndepths = datapath, split, nviews, img_wh, ndepths
        self.device = torch.device(device)
        self.image_sizes = dict(TANKS_SCANS[split])
        self.scans = list(self.image_sizes) if scans is None else list(scans)
        self.metas = []
        for scan in self.scans:
            for ref, srcs in scan_io.read_pair_file(os.path.join(datapath, split, scan, "pair.txt")):
                self.metas.append((scan, ref, srcs, scan))

    def __len__(self):
        return len(self.metas)

    @staticmethod
    def read_cam_file(filename):
        """-> intrinsics (first two rows / 4), extrinsics, depth_min, depth_max (datasets/tanks.py:66-80)."""
        lines = scan_io._cam_lines(filename)
        K, E = scan_io._matrix(lines[7:10], 3, 3), scan_io._matrix(lines[1:5], 4, 4)
        K[:2, :] /= 4.0
        tail = lines[11].split()
        return K, E, float(tail[0]), float(tail[1])

    def load_host(self, idx):
        scan, ref_view, src_views, _ = self.metas[idx]
        view_ids = [ref_view] + src_views[:self.nviews - 1]
        new_w, new_h = self.img_wh
        raws, projs, depth_values = [], [], None
        for i, vid in enumerate(view_ids):
            folder = os.path.join(self.datapath, self.split, scan)
            K, E, depth_min, depth_max = self.read_cam_file(os.path.join(folder, "cams_1/{:08d}_cam.txt".format(vid)))
            raw = np.array(Image.open(os.path.join(folder, "images/{:08d}.jpg".format(vid))), dtype=np.uint8)
            h0, w0 = raw.shape[:2]
            K[0, :] *= 1.0 * new_w / w0
            K[1, :] *= 1.0 * new_h / h0
            raws.append(raw)
            p = np.zeros((2, 4, 4), dtype=np.float32)
            p[0, :4, :4] = E
            p[1, :3, :3] = K
            projs.append(p)
            if i == 0:
                interval = (depth_max - depth_min) / (self.ndepths - 1)
                depth_values = np.arange(depth_min, interval * (self.ndepths - 0.5) + depth_min, interval, dtype=np.float32)
        return {"raw": raws, "size": (int(new_h), int(new_w)), "proj": np.stack(projs), "depth_values": depth_values,
                "filename": scan + "/{}/" + "{:0>8}".format(view_ids[0]) + "{}"}

    def to_device(self, host):
        return _finish_item(host, self.device)

    def __getitem__(self, idx):
        return self.to_device(self.load_host(idx))


# ---------------------------------------------------------------------------------------------------------------------
# training loader (datasets/dtu_train.py)
# ---------------------------------------------------------------------------------------------------------------------
JITTER_RANGES = ((0.0, 2.0), (0.0, 2.0), (0.5, 1.5), (-0.5, 0.5))   # ColorJitter(brightness=1, contrast=1, saturation=0.5, hue=0.5)
GAMMA_RANGE = (0.5, 2.0)                                            # RandomGamma(min_gamma=0.5, max_gamma=2.0, clip_image=True)
TRAIN_HW = (512, 640)                                               # prepare_img's crop (dtu_train.py:164-178)
TRAIN_RAW_HW = (1200, 1600)                                         # the depth / mask maps of Depths_raw


def tone_table(gamma=None, mean=MEAN, std=STD):
    """(3,256) fp32: what ToTensor [+ RandomGamma(gamma, clip_image=True)] + Normalize make of each byte value, computed with
    the torch CPU ops the reference applies to the whole image (datasets/utils.py:52-57), so the kernel's values are torch's."""
    t = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    if gamma is not None:
        t = torch.pow(t, float(gamma))
        t.clamp_(0.0, 1.0)
    t = t.view(1, 256).repeat(3, 1)
    return t.sub_(torch.as_tensor(mean, dtype=torch.float32).view(3, 1)).div_(torch.as_tensor(std, dtype=torch.float32).view(3, 1))


def draw_aug(generator, nviews):
    """Per-view augmentation parameters from ``generator``: ``order`` (V,4) int32 permutations of (brightness, contrast,
    saturation, hue), ``factors`` (V,4) fp32 in JITTER_RANGES, ``gamma`` (V,) fp64 in GAMMA_RANGE."""
    order = np.stack([torch.randperm(4, generator=generator).numpy() for _ in range(nviews)]).astype(np.int32)
    u = torch.rand((nviews, 5), generator=generator, dtype=torch.float64).numpy()
    lo = np.array([r[0] for r in JITTER_RANGES] + [GAMMA_RANGE[0]])
    hi = np.array([r[1] for r in JITTER_RANGES] + [GAMMA_RANGE[1]])
    v = lo + u * (hi - lo)
    factors = np.clip(v[:, :4].astype(np.float32), lo[:4].astype(np.float32), hi[:4].astype(np.float32))   # fp32 rounding stays inside
    return {"order": order, "factors": factors, "gamma": v[:, 4].copy()}


def prepare_train_images(raw_u8, aug, device, return_u8=False):
    """Decoded views (V,H,W,3) uint8 numpy + ``aug`` (see draw_aug) -> {"imgs", "center_imgs", "imgs_aug"}: (V,3,H,W) fp32
    tensors on ``device`` (rcmvs_train_image_stats + rcmvs_train_image_apply); ``return_u8`` adds "jitter_u8" (V,H,W,3), the
    bytes ColorJitter produced (equal to Pillow's)."""
    raw_u8 = np.asarray(raw_u8)
    if raw_u8.dtype != np.uint8 or raw_u8.ndim != 4 or raw_u8.shape[3] != 3:
        raise _lib.RcmvsError(f"prepare_train_images: expected (V,H,W,3) uint8 views, got {raw_u8.dtype} {raw_u8.shape}")
    V, H, W = raw_u8.shape[:3]
    order = np.ascontiguousarray(aug["order"], dtype=np.int32)
    factors = np.ascontiguousarray(aug["factors"], dtype=np.float32)
    gamma = np.asarray(aug["gamma"], dtype=np.float64)
    if order.shape != (V, 4) or factors.shape != (V, 4) or gamma.shape != (V,):
        raise _lib.RcmvsError(f"prepare_train_images: parameters of {V} views expected, got order {order.shape}, factors {factors.shape}, "
                              f"gamma {gamma.shape}")
    if not (np.isfinite(gamma).all() and (gamma > 0).all()):
        raise _lib.RcmvsError(f"prepare_train_images: gamma must be finite and > 0, got {gamma}")
    params = np.ascontiguousarray(np.concatenate([factors.view(np.int32), order], axis=1))            # (V,8) words: ta::ViewParams
    src = torch.from_numpy(np.ascontiguousarray(raw_u8)).to(device, non_blocking=True)
    params_dev = torch.from_numpy(params).to(device, non_blocking=True)
    lut_seg = tone_table().to(device, non_blocking=True)
    lut_aug = torch.stack([tone_table(g) for g in gamma]).to(device, non_blocking=True)
    sums = torch.empty((V, 8), device=device, dtype=torch.int64)
    out = {k: torch.empty((V, 3, H, W), device=device, dtype=torch.float32) for k in ("imgs", "center_imgs", "imgs_aug")}
    u8 = torch.empty((V, H, W, 3), device=device, dtype=torch.uint8) if return_u8 else None
    host = ctypes.c_void_p(params.ctypes.data)
    _lib.call("rcmvs_train_image_stats", _chk(src, "src", torch.uint8), V, H, W, host, _chk(params_dev, "params", torch.int32),
              _chk(sums, "sums", torch.int64), _stream())
    _lib.call("rcmvs_train_image_apply", _chk(src, "src", torch.uint8), V, H, W, host, _chk(params_dev, "params", torch.int32),
              _chk(sums, "sums", torch.int64), _chk(lut_seg, "lut_seg"), _chk(lut_aug, "lut_aug"),
              _chk(out["imgs"], "imgs"), _chk(out["center_imgs"], "center_imgs"), _chk(out["imgs_aug"], "imgs_aug"),
              ctypes.c_void_p(0) if u8 is None else _chk(u8, "u8_out", torch.uint8), _stream())
    if return_u8:
        out["jitter_u8"] = u8
    out["sums"] = sums
    return out


def _half_crop(raw, what):
    """prepare_img / read_depth_all (dtu_train.py:164-178,195-205): cv2.resize(INTER_NEAREST) to exactly half the size picks
    source index 2 * dst, then the centre crop to 512 x 640 -- strided slicing.  Only the raw size the reference's hard-coded
    crop ([44:556, 80:720] of the halved map) is written for is accepted."""
    if raw.shape != TRAIN_RAW_HW:
        raise _lib.RcmvsError(f"{what}: raw size {raw.shape} is not {TRAIN_RAW_HW}, the only one the reference's crop handles")
    return np.ascontiguousarray(raw[88:1112:2, 160:1440:2])


def _pyramid(full):
    return {"stage1": np.ascontiguousarray(full[::4, ::4]), "stage2": np.ascontiguousarray(full[::2, ::2]), "stage3": full}


class DTUTrainDataset(torch.utils.data.Dataset):
    """datasets/dtu_train.py ``MVSDataset`` (the training set of Yao Yao's preprocessed DTU):

        <datapath>/Cameras/pair.txt, Cameras/train/<view:08d>_cam.txt
        <datapath>/Rectified/<scan>_train/rect_<view+1:03d>_<light>_r5000.png            (512 x 640)
        <datapath>/Depths_raw/<scan>/depth_map_<view:04d>.pfm, depth_visual_<view:04d>.png  (1200 x 1600)

    One item per scan x viewpoint x light (7).  Same keys and shapes as the reference's item; ``imgs``, ``imgs_aug`` and
    ``center_imgs`` are CUDA tensors, the rest numpy.  The augmentation's random draws come from a generator seeded from
    (seed, epoch, idx) -- ``set_epoch`` -- and travel with the host half as ``host["aug"]``."""

    def __init__(self, datapath, listfile, mode, nviews, ndepths=192, interval_scale=1.06, random_view=False, device="cuda:0", seed=0):
        super().__init__()
        if mode not in ("train", "val"):
            raise ValueError(f"DTUTrainDataset: mode {mode!r} is not 'train' or 'val' (evaluation folders: MVSDataset)")
        self.datapath, self.listfile, self.mode, self.nviews, self.ndepths = datapath, listfile, mode, nviews, ndepths
        self.interval_scale, self.random_view, self.device, self.seed, self.epoch = interval_scale, random_view, torch.device(device), seed, 0
        self.metas = self.build_list()
        self.build_proj_mats()

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def build_list(self):
        with open(self.listfile) as f:
            scans = [line.rstrip() for line in f.readlines()]
        pairs = []
        with open(os.path.join(self.datapath, "Cameras/pair.txt")) as f:
            for _ in range(int(f.readline())):
                ref = int(f.readline().rstrip())
                pairs.append((ref, [int(x) for x in f.readline().rstrip().split()[1::2]]))
        metas = [(scan, light, ref, srcs) for scan in scans for ref, srcs in pairs for light in range(7)]
        self.id_list = np.unique(np.concatenate([[ref] + srcs for ref, srcs in pairs]).astype(np.int64)) if scans else np.zeros(0, np.int64)
        self.remap = np.zeros(int(self.id_list.max()) + 1 if len(self.id_list) else 0, dtype=int)
        self.remap[self.id_list] = np.arange(len(self.id_list))
        return metas

    def read_cam_file(self, filename):
        """-> intrinsics, extrinsics (fp32), depth_min, depth_interval * interval_scale, [depth_min, depth_max] (dtu_train.py:113-125)"""
        lines = scan_io._cam_lines(filename)
        tail = lines[11].split()
        depth_min, depth_interval = float(tail[0]), float(tail[1]) * self.interval_scale
        return (scan_io._matrix(lines[7:10], 3, 3), scan_io._matrix(lines[1:5], 4, 4), depth_min, depth_interval,
                [depth_min, depth_min + depth_interval * self.ndepths])

    def build_proj_mats(self):
        """Per camera of the pair file: the full-resolution intrinsics, the 4x4 projection at quarter resolution (float64, from
        an fp32 product, as dtu_train.py:31-54 forms it), near / far, world-to-camera and its inverse."""
        self.proj_mats, self.near_fars, intr, w2c, c2w = [], [], [], [], []
        for vid in self.id_list:
            K, E, _, _, near_far = self.read_cam_file(os.path.join(self.datapath, f"Cameras/train/{vid:08d}_cam.txt"))
            K[:2] *= 4
            intr.append(K.copy())
            K[:2] = K[:2] / 4
            P = np.eye(4)
            P[:3, :4] = K @ E[:3, :4]
            self.proj_mats.append(P)
            self.near_fars.append(near_far)
            w2c.append(E)
            c2w.append(np.linalg.inv(E))
        self.intrinsics_nerf, self.world2cams, self.cam2worlds = np.stack(intr), np.stack(w2c), np.stack(c2w)

    def __len__(self):
        return len(self.metas)

    def generator(self, idx):
        """The item's own random stream: a function of (seed, epoch, idx) only, not of the thread or order that loads it."""
        mix = ((int(self.seed) * 0x9E3779B1 + int(self.epoch)) * 0x85EBCA6B + int(idx)) & 0x7FFFFFFFFFFFFFFF
        return torch.Generator().manual_seed(mix)

    def load_host(self, idx):
        """Everything of item ``idx`` that needs no GPU: PNG / PFM decoding (every file once), camera parsing, the depth and mask
        pyramids, the renderer's matrices, and the augmentation draws.  Thread-safe (``prefetch`` runs it on worker threads)."""
        scan, light_idx, ref_view, src_views = self.metas[idx]
        g = self.generator(idx)
        if self.random_view:
            pick = torch.randperm(len(src_views), generator=g)[:self.nviews - 1]
            view_ids = [ref_view] + [src_views[int(i)] for i in pick]
        else:
            view_ids = [ref_view] + src_views[:self.nviews - 1]
        raws, proj_matrices, depths_h, proj_mats, affine, affine_inv, intr, w2cs, c2ws, near_fars = [], [], [], [], [], [], [], [], [], []
        for i, vid in enumerate(view_ids):
            img_name = os.path.join(self.datapath, "Rectified/{}_train/rect_{:0>3}_{}_r5000.png".format(scan, vid + 1, light_idx))
            mask_name = os.path.join(self.datapath, "Depths_raw/{}/depth_visual_{:0>4}.png".format(scan, vid))
            depth_name = os.path.join(self.datapath, "Depths_raw/{}/depth_map_{:0>4}.pfm".format(scan, vid))
            raw = np.array(Image.open(img_name).convert("RGB"), dtype=np.uint8)
            if raws and raw.shape != raws[0].shape:
                raise _lib.RcmvsError(f"view {vid} of {scan}: size {raw.shape[:2]} differs from the reference view's {raws[0].shape[:2]}")
            raws.append(raw)
            k = self.remap[vid]
            P = self.proj_mats[k]
            intr.append(self.intrinsics_nerf[k])
            w2cs.append(self.world2cams[k])
            c2ws.append(self.cam2worlds[k])
            near_fars.append(self.near_fars[k])
            affine.append(P)
            affine_inv.append(np.linalg.inv(P))
            if i == 0:
                ref_inv = np.linalg.inv(P)
                proj_mats.append(np.eye(4))
            else:
                proj_mats.append(P @ ref_inv)
            depth_full = None
            if os.path.exists(depth_name):
                depth_full = _half_crop(read_pfm(depth_name)[0], depth_name)
                depths_h.append(depth_full)
            else:
                depths_h.append(np.zeros((1, 1)))                   # dtu_train.py:303-308
            K, E, depth_min, depth_interval, _ = self.read_cam_file(os.path.join(self.datapath, "Cameras/train/{:0>8}_cam.txt".format(vid)))
            p = np.zeros((2, 4, 4), dtype=np.float32)
            p[0, :4, :4] = E
            p[1, :3, :3] = K
            proj_matrices.append(p)
            if i == 0:
                if depth_full is None:
                    raise _lib.RcmvsError(f"{depth_name}: the reference view's depth map is missing")
                visual = np.array(Image.open(mask_name), dtype=np.float32)
                mask = _pyramid(_half_crop((visual > 10).astype(np.float32), mask_name))
                depth = _pyramid(depth_full)
                depth_values = np.arange(depth_min, depth_interval * self.ndepths + depth_min, depth_interval, dtype=np.float32)
        view_ids_all = [ref_view] + list(src_views)
        return {"raw": np.stack(raws), "aug": draw_aug(g, len(view_ids)), "proj": np.stack(proj_matrices), "depth": depth, "mask": mask,
                "depth_values": depth_values, "depths_h": np.stack(depths_h).astype(np.float32), "w2cs": np.stack(w2cs).astype(np.float32),
                "c2ws": np.stack(c2ws).astype(np.float32), "near_fars": np.stack(near_fars).astype(np.float32),
                "proj_mats": np.stack(proj_mats)[:, :3].astype(np.float32), "intrinsics": np.stack(intr).astype(np.float32),
                "view_ids": np.array(view_ids), "light_id": np.array(light_idx), "affine_mat": np.stack(affine),
                "affine_mat_inv": np.stack(affine_inv), "scan": scan, "c2ws_all": self.cam2worlds[self.remap[view_ids_all]].astype(np.float32)}

    def to_device(self, host):
        """The device half: two launches for all views' three image tensors, then the three-stage projection matrices."""
        item = {k: v for k, v in host.items() if k not in ("raw", "aug", "proj")}
        out = prepare_train_images(host["raw"], host["aug"], self.device)
        item.update(imgs=out["imgs"], imgs_aug=out["imgs_aug"], center_imgs=out["center_imgs"])
        proj = host["proj"]
        stages = {"stage1": proj}
        for key, mul in (("stage2", 2), ("stage3", 4)):
            q = proj.copy()
            q[:, 1, :2, :] = proj[:, 1, :2, :] * mul
            stages[key] = q
        item["proj_matrices"] = stages
        return item

    def __getitem__(self, idx):
        return self.to_device(self.load_host(idx))

    def render_batch(self, item):
        """The dict train_step hands to Rendering_Consistency_Net (train_rcmvsnet.py:279-285): batch dimension added, on the device."""
        dev = item["imgs"].device
        batch = {k: torch.from_numpy(np.ascontiguousarray(item[k]))[None].to(dev) for k in ("w2cs", "c2ws", "intrinsics", "near_fars", "depths_h", "proj_mats")}
        batch["imgs"] = item["imgs"][None]
        return batch


# ---------------------------------------------------------------------------------------------------------------------
# validation loader (datasets/dtu_yao.py)
# ---------------------------------------------------------------------------------------------------------------------
_STAGES = ("stage1", "stage2", "stage3")


def _staging(array, device):
    """numpy -> host tensor an upload starts from: page-locked for a GPU, so that ``.to(device, non_blocking=True)`` is
    enqueued behind the running kernels instead of making the host wait for them (what a pageable copy does)."""
    t = torch.from_numpy(np.ascontiguousarray(array))
    return t.pin_memory() if device.type == "cuda" else t


class DTUValDataset(torch.utils.data.Dataset):
    """datasets/dtu_yao.py ``MVSDataset`` as train_rcmvsnet.py:518-519 builds it (mode "test", 5 views): the folder layout of
    ``DTUTrainDataset``, one item per scan x viewpoint x light, views ``[ref] + src[:nviews-1]``, no augmentation and no
    ImageNet normalisation.  Item = the reference's: ``imgs`` (V,3,H,W) = bytes / 255 in fp32 (a CUDA tensor, one
    rcmvs_prepare_image launch per view on the uploaded bytes), ``proj_matrices`` {stage1..3: (V,2,4,4)}, ``depth`` / ``mask``
    {stage1..3} of the reference view's Depths_raw files, ``depth_values``; all numpy but ``imgs``.  ``depth_dev`` / ``mask_dev``
    are the same pyramids as (1,h,w) tensors on the device, ``proj_dev`` / ``depth_values_dev`` the batched (1,...) device copies
    of the matrices and depth values: everything the forward and ``validation.depth_metrics`` read, uploaded with the item."""

    def __init__(self, datapath, listfile, mode="test", nviews=5, ndepths=192, interval_scale=1.06, device="cuda:0"):
        super().__init__()
        if mode not in ("train", "val", "test"):
            raise ValueError(f"DTUValDataset: mode {mode!r} is not 'train', 'val' or 'test'")
        self.datapath, self.listfile, self.mode, self.nviews, self.ndepths = datapath, listfile, mode, nviews, ndepths
        self.interval_scale, self.device = interval_scale, torch.device(device)
        self.metas = self.build_list()

    def build_list(self):
        with open(self.listfile) as f:
            scans = [line.rstrip() for line in f.readlines()]
        pairs = []
        with open(os.path.join(self.datapath, "Cameras/pair.txt")) as f:
            for _ in range(int(f.readline())):
                ref = int(f.readline().rstrip())
                pairs.append((ref, [int(x) for x in f.readline().rstrip().split()[1::2]]))
        return [(scan, light, ref, srcs) for scan in scans for ref, srcs in pairs for light in range(7)]

    def __len__(self):
        return len(self.metas)

    def read_cam_file(self, filename):
        """-> intrinsics, extrinsics (fp32), depth_min, depth_interval * interval_scale (dtu_yao.py:53-64)"""
        lines = scan_io._cam_lines(filename)
        tail = lines[11].split()
        return scan_io._matrix(lines[7:10], 3, 3), scan_io._matrix(lines[1:5], 4, 4), float(tail[0]), float(tail[1]) * self.interval_scale

    def load_host(self, idx):
        """Everything of item ``idx`` that needs no GPU: PNG / PFM decoding, camera parsing, the depth and mask pyramids.
        Thread-safe (``prefetch`` runs it on worker threads)."""
        scan, light_idx, ref_view, src_views = self.metas[idx]
        view_ids = [ref_view] + src_views[:self.nviews - 1]
        raws, projs = [], []
        for i, vid in enumerate(view_ids):
            img_name = os.path.join(self.datapath, "Rectified/{}_train/rect_{:0>3}_{}_r5000.png".format(scan, vid + 1, light_idx))
            raw = np.array(Image.open(img_name), dtype=np.uint8)
            if raw.ndim != 3 or raw.shape[2] != 3:
                raise _lib.RcmvsError(f"{img_name}: expected an RGB image, got shape {raw.shape}")
            if raws and raw.shape != raws[0].shape:
                raise _lib.RcmvsError(f"view {vid} of {scan}: size {raw.shape[:2]} differs from the reference view's {raws[0].shape[:2]}")
            raws.append(raw)
            K, E, depth_min, depth_interval = self.read_cam_file(os.path.join(self.datapath, "Cameras/train/{:0>8}_cam.txt".format(vid)))
            p = np.zeros((2, 4, 4), dtype=np.float32)
            p[0, :4, :4] = E
            p[1, :3, :3] = K
            projs.append(p)
            if i == 0:
                mask_name = os.path.join(self.datapath, "Depths_raw/{}/depth_visual_{:0>4}.png".format(scan, vid))
                depth_name = os.path.join(self.datapath, "Depths_raw/{}/depth_map_{:0>4}.pfm".format(scan, vid))
                visual = np.array(Image.open(mask_name), dtype=np.float32)
                mask = _pyramid(_half_crop((visual > 10).astype(np.float32), mask_name))
                depth = _pyramid(_half_crop(np.array(read_pfm(depth_name)[0], dtype=np.float32), depth_name))
                depth_values = np.arange(depth_min, depth_interval * self.ndepths + depth_min, depth_interval, dtype=np.float32)
        proj = np.stack(projs)
        stages = {"stage1": proj}
        for key, mul in (("stage2", 2), ("stage3", 4)):
            q = proj.copy()
            q[:, 1, :2, :] = proj[:, 1, :2, :] * mul
            stages[key] = q
        # one staging buffer for the bytes and one for every fp32 array the GPU reads: two uploads per item
        small = np.concatenate([depth[k].ravel() for k in _STAGES] + [mask[k].ravel() for k in _STAGES] +
                               [stages[k].ravel() for k in _STAGES] + [depth_values])
        return {"raw": _staging(np.stack(raws), self.device), "f32": _staging(small, self.device), "proj_matrices": stages, "depth": depth,
                "mask": mask, "depth_values": depth_values, "scan": scan, "view_ids": np.array(view_ids), "light_id": np.array(light_idx)}

    def to_device(self, host):
        """The device half: two uploads, one rcmvs_prepare_image launch per view (equal sizes, mean 0, std 1: float(b) / 255.0f),
        then views of the fp32 upload."""
        item = {k: v for k, v in host.items() if k not in ("raw", "f32")}
        src = host["raw"].to(self.device, non_blocking=True)
        V, H, W = src.shape[:3]
        imgs = torch.empty((V, 3, H, W), device=self.device, dtype=torch.float32)
        zero, one = (ctypes.c_float * 3)(0.0, 0.0, 0.0), (ctypes.c_float * 3)(1.0, 1.0, 1.0)
        for v in range(V):
            _lib.call("rcmvs_prepare_image", _chk(src[v], "src", torch.uint8), _chk(imgs[v], "imgs"), H, W, H, W,
                      ctypes.cast(zero, ctypes.c_void_p), ctypes.cast(one, ctypes.c_void_p), _stream())
        item["imgs"] = imgs
        f32 = host["f32"].to(self.device, non_blocking=True)
        at = 0
        for key, shapes in (("depth_dev", [(1,) + host["depth"][k].shape for k in _STAGES]), ("mask_dev", [(1,) + host["mask"][k].shape for k in _STAGES]),
                            ("proj_dev", [(1,) + host["proj_matrices"][k].shape for k in _STAGES])):
            item[key] = {}
            for k, shape in zip(_STAGES, shapes):
                n = int(np.prod(shape))
                item[key][k] = f32[at:at + n].view(shape)
                at += n
        item["depth_values_dev"] = f32[at:].view(1, -1)
        return item

    def __getitem__(self, idx):
        return self.to_device(self.load_host(idx))
