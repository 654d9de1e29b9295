"""Training loader, image preparation, without a GPU: the per-pixel arithmetic of csrc/train_aug_math.h (g++ loop harness)
against Pillow itself -- both HSV conversions on all 2^24 inputs, each enhancer, full ColorJitter in all 24 orders -- and the
kernels of csrc/train_aug.hip on the CPU emulation against the oracle (tests/train_dataset_oracle.py)."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance

import train_dataset_oracle as O
from rc_mvsnet_amd import _lib, mvs_dataset

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ta") / "ta_harness.so")
    subprocess.run(["g++", "-O2", "-w", "-ffp-contract=off", "-shared", "-fPIC", "-o", out,
                    os.path.join(HERE, "harness", "train_aug_harness.cpp")], check=True)
    return ctypes.CDLL(out)


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _params(order, factors):
    return np.ascontiguousarray(np.concatenate([np.asarray(factors, np.float32).view(np.int32), np.asarray(order, np.int32)]))


def harness_jitter(h, img, order, factors):
    out = np.empty_like(img)
    par = _params(order, factors)
    rc = h.h_jitter(_p(img), _p(out), ctypes.c_longlong(img.shape[0] * img.shape[1]), _p(par))
    assert rc == 0, rc
    return out


def _cube():
    a = np.arange(256, dtype=np.uint8)
    return np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(4096, 4096, 3)


def test_rgb_to_hsv_equals_pillow_on_all_inputs(harness):
    got = np.empty((1 << 24, 3), np.uint8)
    harness.h_rgb2hsv_cube(_p(got))
    want = np.array(Image.fromarray(_cube(), "RGB").convert("HSV")).reshape(-1, 3)
    assert int((got != want).any(1).sum()) == 0


def test_hsv_to_rgb_equals_pillow_on_all_inputs(harness):
    got = np.empty((1 << 24, 3), np.uint8)
    harness.h_hsv2rgb_cube(_p(got))
    want = np.array(Image.fromarray(_cube(), "HSV").convert("RGB")).reshape(-1, 3)
    assert int((got != want).any(1).sum()) == 0


def _inside(lo, hi):
    return [lo, hi, float(np.nextafter(np.float32(lo), np.float32(hi))), float(np.nextafter(np.float32(hi), np.float32(lo)))]


@pytest.mark.parametrize("op,enhancer,factors", [
    (O.BRIGHTNESS, ImageEnhance.Brightness, [0.0, 1.0, 2.0] + _inside(0.0, 2.0) + [0.37, 1.61]),
    (O.CONTRAST, ImageEnhance.Contrast, [0.0, 1.0, 2.0] + _inside(0.0, 2.0) + [0.37, 1.61]),
    (O.SATURATION, ImageEnhance.Color, [0.0, 1.0, 2.0] + _inside(0.5, 1.5) + [0.83, 1.27]),
])
def test_each_enhancer_equals_pillow(harness, op, enhancer, factors):
    img = np.random.default_rng(op).integers(0, 256, (96, 128, 3), dtype=np.uint8)
    # the operation under test first; the others as identities would still round (the hue round trip is lossy), so compare
    # against the oracle's chain with the same neutral parameters
    order = [op] + [k for k in range(4) if k != op]
    for f in factors:
        fac = np.array([1.0, 1.0, 1.0, 0.0], np.float32)
        fac[op] = f
        assert np.array_equal(np.array(enhancer(Image.fromarray(img)).enhance(float(fac[op]))), O.color_jitter(img, [op], fac)), f
        assert np.array_equal(harness_jitter(harness, img, order, fac), O.color_jitter(img, order, fac)), f


def test_hue_shift_equals_pillow(harness):
    img = np.random.default_rng(7).integers(0, 256, (96, 128, 3), dtype=np.uint8)
    for f in [0.0, 0.5, -0.5] + _inside(-0.5, 0.5)[2:] + [0.25, -0.25, 0.0039, -0.0039, 0.004, -0.1234]:
        fac = np.array([1.0, 1.0, 1.0, f], np.float32)
        assert np.array_equal(harness_jitter(harness, img, [3, 0, 1, 2], fac), O.color_jitter(img, [3, 0, 1, 2], fac)), f


def test_color_jitter_equals_pillow_in_all_orders(harness):
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (128, 160, 3), dtype=np.uint8)
    img[:16] = img[:16] // 8                                      # a dark band and a flat patch
    img[100:, 100:] = 77
    for order in itertools.permutations(range(4)):
        fac = np.array([rng.uniform(0, 2), rng.uniform(0, 2), rng.uniform(0.5, 1.5), rng.uniform(-0.5, 0.5)], np.float32)
        assert np.array_equal(harness_jitter(harness, img, order, fac), O.color_jitter(img, order, fac)), (order, fac)


def test_bad_parameters_are_refused_by_the_shared_check(harness):
    img = np.zeros((2, 2, 3), np.uint8)
    out = np.empty_like(img)
    for order, fac in (([0, 1, 2, 2], [1, 1, 1, 0]), ([0, 1, 2, 4], [1, 1, 1, 0]), ([0, 1, 2, 3], [-0.1, 1, 1, 0]),
                       ([0, 1, 2, 3], [1, np.inf, 1, 0]), ([0, 1, 2, 3], [1, 1, np.nan, 0]), ([0, 1, 2, 3], [1, 1, 1, 0.51]),
                       ([0, 1, 2, 3], [1, 1, 1, np.nan])):
        par = _params(order, fac)
        assert harness.h_jitter(_p(img), _p(out), ctypes.c_longlong(4), _p(par)) != 0, (order, fac)


def test_center_image_arithmetic(harness):
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (60, 81, 3), dtype=np.uint8)
    img[..., 2] = 9                                               # a constant channel: variance 0 -> zeros, not NaN
    got = np.empty((3, 60 * 81), np.float32)
    harness.h_center(_p(img), _p(got), ctypes.c_longlong(60 * 81))
    want = O.center_image(img)
    assert float(np.abs(got.reshape(3, 60, 81) - want).max()) <= 1e-6 * max(1.0, float(np.abs(want).max()))
    assert np.array_equal(got[2], np.zeros(60 * 81, np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# the kernels on the emulation
# ---------------------------------------------------------------------------------------------------------------------
def _views(V, H, W, seed):
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, (V, H, W, 3), dtype=np.uint8)
    raw[-1, :, :, 1] = 200                                        # a constant channel in the last view
    return raw


def _aug(V, seed, first_orders=((1, 0, 2, 3), (0, 2, 3, 1))):
    aug = mvs_dataset.draw_aug(torch.Generator().manual_seed(seed), V)
    for v, o in enumerate(first_orders[:V]):                      # contrast first / contrast last are always among the cases
        aug["order"][v] = o
    return aug


def check_against_oracle(raw, aug, out, atol):
    """shared with tests/test_gpu_train_dataset.py: bytes bit-identical, imgs / imgs_aug within atol, center_imgs rel 1e-6"""
    from conftest import rel_err
    for v in range(len(raw)):
        want_u8 = O.color_jitter(raw[v], aug["order"][v], aug["factors"][v])
        assert np.array_equal(out["jitter_u8"][v].cpu().numpy(), want_u8), v
        assert np.allclose(out["imgs"][v].cpu().numpy(), O.images_seg(raw[v]), rtol=0, atol=atol), v
        want_aug = O.images_aug(raw[v], aug["order"][v], aug["factors"][v], aug["gamma"][v])
        assert np.allclose(out["imgs_aug"][v].cpu().numpy(), want_aug, rtol=0, atol=atol), v
        assert rel_err(out["center_imgs"][v].cpu(), O.center_image(raw[v])) <= 1e-6, v
        sums = out["sums"][v].cpu().numpy()
        x = raw[v].reshape(-1, 3).astype(np.int64)
        assert np.array_equal(sums[:3], x.sum(0)) and np.array_equal(sums[3:6], (x * x).sum(0))


@pytest.mark.parametrize("V,H,W", [(3, 37, 53), (2, 32, 40)])
def test_kernels_on_emulation_match_oracle(emu, V, H, W):
    raw, aug = _views(V, H, W, 1), _aug(V, 5)
    out = mvs_dataset.prepare_train_images(raw, aug, "cpu", return_u8=True)
    check_against_oracle(raw, aug, out, atol=1e-6)
    assert torch.equal(out["center_imgs"][-1, 1], torch.zeros(H, W))


def test_kernel_entry_points_refuse_bad_input(emu):
    raw, aug = _views(2, 8, 8, 0), _aug(2, 0)
    for key, value in (("order", np.array([[0, 1, 2, 2], [0, 1, 2, 3]])), ("factors", np.array([[1, 1, 1, 0.6], [1, 1, 1, 0]])),
                       ("factors", np.array([[1, -1, 1, 0], [1, 1, 1, 0]])), ("factors", np.array([[1, 1, np.inf, 0], [1, 1, 1, 0]])),
                       ("gamma", np.array([1.0, -1.0])), ("gamma", np.array([1.0]))):
        bad = dict(aug)
        bad[key] = value
        with pytest.raises(_lib.RcmvsError):
            mvs_dataset.prepare_train_images(raw, bad, "cpu")
    with pytest.raises(_lib.RcmvsError):
        mvs_dataset.prepare_train_images(raw[..., :2], aug, "cpu")
    lib = emu
    z = ctypes.c_void_p(0)
    assert lib.rcmvs_train_image_stats(z, 1, 8, 8, z, z, z, z) != 0
    par = _params([0, 1, 2, 3], [1, 1, 1, 0])
    buf = np.zeros(64, np.int64)
    assert lib.rcmvs_train_image_stats(_p(buf), 0, 8, 8, _p(par), _p(par), _p(buf), z) != 0          # V outside 1..65535
    assert lib.rcmvs_train_image_stats(_p(buf), 1, 1 << 15, 1 << 14, _p(par), _p(par), _p(buf), z) != 0   # H W >= 2^29
    assert b"2^29" in lib.rcmvs_last_error_string() or b"size" in lib.rcmvs_last_error_string()


def test_prepare_fails_loudly_without_a_gpu():
    with pytest.raises(_lib.RcmvsError):
        mvs_dataset.prepare_train_images(_views(1, 8, 8, 0), _aug(1, 0), "cpu")
