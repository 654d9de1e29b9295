"""Test oracle of the training loader's image preparation (test infrastructure): what datasets/dtu_train.py of the reference
computes per image, with Pillow itself standing for torchvision's PIL backend.

* ``color_jitter``  -- transforms.ColorJitter's uint8 stage for given parameters: the PIL calls torchvision's
  functional_pil makes (ImageEnhance.Brightness / Contrast / Color, and for the hue the HSV round trip with a uint8 shift of
  the H channel), in the drawn order.  torchvision is not installed where this project is developed, so the call sequence is
  a restatement of its published source; everything below the calls is Pillow's own arithmetic.
* ``tone_table`` / ``images_aug`` / ``images_seg`` -- ToTensor, RandomGamma (torch.pow + clamp_) and Normalize with the torch
  CPU ops the reference applies.
* ``center_image`` -- dtu_train.py:156-161 in fp64 (the reference computes it in fp32 numpy).
"""
import numpy as np
import torch
from PIL import Image, ImageEnhance

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3


def adjust_hue(img, hue_factor):
    """torchvision.transforms.functional_pil.adjust_hue: the round trip is made for a zero shift too."""
    if not -0.5 <= hue_factor <= 0.5:
        raise ValueError("hue_factor is not in [-0.5, 0.5]")
    h, s, v = img.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    shift = int(hue_factor * 255) % 256                      # np.uint8(hue_factor * 255): truncation, then wrap-around
    np_h = (np_h.astype(np.int32) + shift).astype(np.uint8)
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


def color_jitter(img_u8, order, factors):
    """img_u8 (H,W,3) uint8; order: permutation of (0,1,2,3); factors: (brightness, contrast, saturation, hue) -> (H,W,3) uint8"""
    img = Image.fromarray(np.ascontiguousarray(img_u8), "RGB")
    for op in order:
        f = float(factors[op])
        if op == BRIGHTNESS:
            img = ImageEnhance.Brightness(img).enhance(f)
        elif op == CONTRAST:
            img = ImageEnhance.Contrast(img).enhance(f)
        elif op == SATURATION:
            img = ImageEnhance.Color(img).enhance(f)
        else:
            img = adjust_hue(img, f)
    return np.array(img, dtype=np.uint8)


def to_tensor(img_u8):
    """transforms.ToTensor on a PIL RGB image: (3,H,W) fp32 = byte / 255"""
    return torch.from_numpy(np.ascontiguousarray(img_u8)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


def normalize(t, mean=MEAN, std=STD):
    m = torch.as_tensor(mean, dtype=torch.float32).view(-1, 1, 1)
    s = torch.as_tensor(std, dtype=torch.float32).view(-1, 1, 1)
    return (t - m) / s


def images_seg(img_u8):
    """transform_seg: ToTensor + Normalize -> (3,H,W) fp32 numpy"""
    return normalize(to_tensor(img_u8)).numpy()


def images_aug(img_u8, order, factors, gamma):
    """transform_aug: ColorJitter, ToTensor, RandomGamma(clip_image=True), Normalize -> (3,H,W) fp32 numpy"""
    t = torch.pow(to_tensor(color_jitter(img_u8, order, factors)), float(gamma))
    t.clamp_(0.0, 1.0)
    return normalize(t).numpy()


def center_image(img_u8):
    """(H,W,3) uint8 -> (3,H,W) fp64"""
    x = img_u8.astype(np.float64)
    var = np.var(x, axis=(0, 1), keepdims=True)
    mean = np.mean(x, axis=(0, 1), keepdims=True)
    return ((x - mean) / (np.sqrt(var) + 0.00000001)).transpose(2, 0, 1)


def center_image_reference(img_u8):
    """the reference's own fp32 numpy form (what the golden holds)"""
    img = img_u8.astype(np.float32)
    var = np.var(img, axis=(0, 1), keepdims=True)
    mean = np.mean(img, axis=(0, 1), keepdims=True)
    return ((img - mean) / (np.sqrt(var) + 0.00000001)).transpose(2, 0, 1)


def nearest_half_crop(raw, out_hw=(512, 640)):
    """prepare_img / read_depth_all: cv2.resize(INTER_NEAREST) by exactly 1/2 (source index 2 * dst), then the centre crop."""
    ds = raw[::2, ::2][:raw.shape[0] // 2, :raw.shape[1] // 2]
    h, w = ds.shape
    sh, sw = (h - out_hw[0]) // 2, (w - out_hw[1]) // 2
    return ds[sh:sh + out_hw[0], sw:sw + out_hw[1]]
