"""Hostile cases and plain fp64 references for the self-supervised loss kernels (csrc/unsup_loss.hip) and the forward kernels of the
rendering tail (csrc/render.hip: gu_sample, point_feats, composite), shared by tests/test_gpu_losses.py and tests/test_gpu_render.py
(device "cuda:0"), by their re-run on the kernel emulation (tests/test_emu_gpu_suite_cpu.py) and by tests/test_unsup_loss_cpu.py,
which shows on the CPU that every exclusion cap holds for the references alone.  Nothing here calls the code under test."""
import functools

import numpy as np
import torch

from oracle import unsup_loss as O
from rc_mvsnet_amd import synthetic

KNIFE = 1e-3               # px: an fp64 position closer than this to an integer may floor() differently in fp32 (coordinates of the
#                            fp32 and the fp64 composition differ by ~1e-4 px)
CAP = 0.01                 # share of pixels a test may exclude as knife edges
D0 = float(2 ** 21)        # the depth of the hand-built tables: a power of two that absorbs the 1e-10 of the denominator in fp64 too
#                            (the spacing just below 2^21 is 2^-32 > 2e-10, so +-2^21 + 1e-10 rounds back), which makes
#                            p / (pz + 1e-10) the same exact quotient in both precisions


def dyadic(n):
    """n - 1 is a power of two: the normalise / un-normalise round trip x / (n-1) * 2 - 1, (x + 1) * (n-1) / 2 is then exact."""
    return n >= 2 and ((n - 1) & (n - 2)) == 0


# ---------------------------------------------------------------------------------------------------------------------
# inverse warp: plain fp64 restatement of losses/homography.py:41-59,104-200 on a coefficient table
# ---------------------------------------------------------------------------------------------------------------------
def warp_positions(coef, depth):
    """coef (B,12) = {M row-major, t}, depth (B,H,W) fp64 -> absolute x, y (after the reference's round trip) and pz, all (B,H,W)."""
    c = coef.double()
    B, H, W = depth.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    row = lambda i: c[:, 3 * i, None, None] * xs + c[:, 3 * i + 1, None, None] * ys + c[:, 3 * i + 2, None, None]   # noqa: E731
    px, py, pz = (row(i) * depth + c[:, 9 + i, None, None] for i in range(3))
    x, y = px / (pz + 1e-10), py / (pz + 1e-10)
    x = ((x / (W - 1) * 2.0 - 1.0) + 1.0) * (W - 1.0) / 2.0
    y = ((y / (H - 1) * 2.0 - 1.0) + 1.0) * (H - 1.0) / 2.0
    return x, y, pz


WILD = 1e6                 # px: beyond this a (masked) sample is the cancellation of bilinear weights of 1e6 and more: rounding noise


def bilinear(img, x, y, pin=None):
    """img (B,H,W,C) fp64, x, y (B,H,W) -> sampled (B,H,W,C), mask (B,H,W), wild (B,H,W): weights against the CLAMPED corners, mask
    x0 >= 0 && x1 <= W-1 && y0 >= 0 && y0 <= H-1 before clamping.  Non-finite depth is out of scope: the rule itself yields NaN there.
    Samples farther than WILD px from the image are always masked, but their values still enter the SSIM windows.  They are the
    difference of weights of 1e6 and more on one and the same clamped tap, so fp64 and fp32 disagree about them (8192 against
    0 to 3 in the "huge" tables): with `pin` (B,H,W,C), the kernel's documented fp32 evaluation (warp_sample_fp32), those samples
    are taken from it, as constants."""
    B, H, W, C = img.shape
    x0, y0 = torch.floor(x.detach()).clamp(-1e9, 1e9), torch.floor(y.detach()).clamp(-1e9, 1e9)
    mask = ((x0 >= 0) & (x0 + 1 <= W - 1) & (y0 >= 0) & (y0 <= H - 1)).double()
    x0c, x1c = x0.clamp(0, W - 1), (x0 + 1).clamp(0, W - 1)
    y0c, y1c = y0.clamp(0, H - 1), (y0 + 1).clamp(0, H - 1)
    flat = img.reshape(B, H * W, C)
    tap = lambda yy, xx: torch.gather(flat, 1, (yy * W + xx).long().reshape(B, H * W, 1).expand(-1, -1, C)).reshape(B, H, W, C)   # noqa: E731
    fx, fy = (x1c - x).unsqueeze(-1), (y1c - y).unsqueeze(-1)
    out = fx * fy * tap(y0c, x0c) + fx * (1 - fy) * tap(y1c, x0c) + (1 - fx) * fy * tap(y0c, x1c) + (1 - fx) * (1 - fy) * tap(y1c, x1c)
    wild = (x.detach().abs() > WILD) | (y.detach().abs() > WILD)
    if pin is not None:
        assert not bool((wild & (mask > 0)).any())
        out = torch.where(wild.unsqueeze(-1), pin.double(), out)
    return out, mask, wild


def warp_sample_fp32(img, coef, depth):
    """The evaluation csrc/unsup_loss_math.h documents for a sample (inv_warp_taps, tap_value), operation by operation in fp32 and
    without contraction: img (B,H,W,C), coef (B,12), depth (B,H,W) -> (B,H,W,C) fp32.  Used only to pin the wild samples of
    `bilinear`; everything decidable is compared with fp64."""
    img, c, d = img.float(), coef.float(), depth.float()
    B, H, W, C = img.shape
    yf, xf = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    row = lambda i: c[:, 3 * i, None, None] * xf + c[:, 3 * i + 1, None, None] * yf + c[:, 3 * i + 2, None, None]   # noqa: E731
    px, py, pz = (row(i) * d + c[:, 9 + i, None, None] for i in range(3))
    den = pz + 1e-10
    x, y = (px / den) / float(W - 1) * 2.0 - 1.0, (py / den) / float(H - 1) * 2.0 - 1.0
    x, y = (x + 1.0) * (W - 1.0) / 2.0, (y + 1.0) * (H - 1.0) / 2.0
    x0, y0 = torch.floor(x.clamp(-1e9, 1e9)).long(), torch.floor(y.clamp(-1e9, 1e9)).long()
    x0c, x1c, y0c, y1c = x0.clamp(0, W - 1), (x0 + 1).clamp(0, W - 1), y0.clamp(0, H - 1), (y0 + 1).clamp(0, H - 1)
    fx, fy = (x1c.float() - x).unsqueeze(-1), (y1c.float() - y).unsqueeze(-1)
    flat = img.reshape(B, H * W, C)
    tap = lambda yy, xx: torch.gather(flat, 1, (yy * W + xx).reshape(B, H * W, 1).expand(-1, -1, C)).reshape(B, H, W, C)   # noqa: E731
    wa, wb, wc, wd = fx * fy, fx * (1.0 - fy), (1.0 - fx) * fy, (1.0 - fx) * (1.0 - fy)
    return wa * tap(y0c, x0c) + wb * tap(y1c, x0c) + wc * tap(y0c, x1c) + wd * tap(y1c, x1c)


def near_integer(p, n, exact=None):
    """positions whose floor() an fp32 evaluation may decide differently: within KNIFE of an integer, on or beside the image (from
    1.5 px outside on the pixel is masked whatever the rounding), and not known to be exact in both precisions."""
    k = ((p - p.round()).abs() < KNIFE) & (p > -1.5) & (p < n + 0.5)
    return k if exact is None else k & ~exact


def exact_axis(p, n):
    """A position on a dyadic axis that is a dyadic rational of at most 20 fractional bits below 10 px: in the hand-built tables it is
    an exact product / quotient of small dyadic numbers, the same in fp32 and fp64, and the round trip keeps it (<= 24 bits)."""
    q = p * 2.0 ** 20
    return (q == q.round()) & (p.abs() < 10.0) & dyadic(n)


WARP_SHAPES = ((5, 9), (9, 20), (2, 2))
WARP_KINDS = ("shift", "frac", "behind", "zero", "huge")


def _table(m0, m1, m2=(0.0, 0.0, 1.0), t=(0.0, 0.0, 0.0)):
    return [*m0, *m1, *m2, *t]


@functools.lru_cache(maxsize=None)
def hostile_warp_case(H, W, kind):
    """Two batch items with different tables: -> img (2,H,W,3), depth (2,H,W), coef (2,12), all fp32.  m0 = x + (slope) y and
    m1 = y + (slope) x make the shift differ per row / column; the translation sits in t (times the depth D0), so positions are
    x + shift exactly.  On an axis where n - 1 is no power of two the round trip is inexact: shifts get +0.375 there so that no
    position is near an integer.
      shift  : integer shifts -> positions -1, 0, n-2, n-1, n on both axes
      frac   : -1 + 2^-20 ; -0.5 and n - 0.5
      behind : a block of negative depth (pz < 0, position x - shift) ; a table with m2 = -1 (pz < 0 everywhere)
      zero   : m2 = x - W//2 (or y - H//2), t2 = 0: one column (row) has pz == 0 exactly, with px == 0 on it in item 1
      huge   : a block of depth 2^-20 with t = +-4096: finite positions beyond +-1e9"""
    g = torch.Generator().manual_seed(H * 100 + W + len(kind))
    img = torch.randn(2, H, W, 3, generator=g)
    depth = torch.full((2, H, W), D0)
    fx, fy = (0.0 if dyadic(W) else 0.375), (0.0 if dyadic(H) else 0.375)
    e = 2.0 ** -20
    if kind == "shift":
        tabs = [_table((1, 2, 0), (1, 1, 0), t=((-1 + fx) * D0, (-1 + fy) * D0, 0)), _table((1, 1, 0), (2, 1, 0), t=((-1 + fx) * D0, (-1 + fy) * D0, 0))]
    elif kind == "frac":
        tabs = [_table((1, 0, 0), (0, 1, 0), t=((-1 + e + fx) * D0, (-1 + e + fy) * D0, 0)), _table((1, 1, 0), (1, 1, 0), t=((-0.5 + fx) * D0, (-0.5 + fy) * D0, 0))]
    elif kind == "behind":
        tabs = [_table((1, 1, 0), (0, 1, 0), t=((-1 + fx) * D0, fy * D0, 0)), _table((-1, -1, 0), (-1, -1, 0), (0, 0, -1), t=((-0.5 + fx) * D0, (-0.5 + fy) * D0, 0))]
        depth[0, : max(H // 2, 1)] = -D0
    elif kind == "zero":                                      # item 1 (dyadic W): px == py == pz == 0 at the centre pixel, 0 / 1e-10 = position (0, 0)
        tabs = [_table((1, 1, 0.375), (0, 1, fy), (1, 0, -(W // 2))), _table((1, 0, -(W // 2) + fx), (0, 1, -(H // 2)), (0, 1, -(H // 2)))]
    else:
        tabs = [_table((1, 0, 0), (0, 1, 0), t=(4096.0, -4096.0, 0)), _table((1, 0, 0), (0, 1, 0), t=(-4096.0, 4096.0, 0))]
        depth[:, :, W // 2:] = 2.0 ** -20
    return img, depth, torch.tensor(tabs, dtype=torch.float32)


def hostile_warp_reference(H, W, kind):
    """-> warped (2,H,W,3), mask (2,H,W), excluded (2,H,W) bool of the fp64 rule on hostile_warp_case."""
    img, depth, coef = hostile_warp_case(H, W, kind)
    x, y, _ = warp_positions(coef, depth.double())
    warped, mask, _ = bilinear(img.double(), x, y)
    excluded = near_integer(x, W, exact_axis(x, W)) | near_integer(y, H, exact_axis(y, H))
    return warped, mask, excluded


# ---------------------------------------------------------------------------------------------------------------------
# one stage of UnSupLoss (losses/unsup_loss.py:14-94) in fp64, term by term
# ---------------------------------------------------------------------------------------------------------------------
# the hand-built tables of hostile_warp_case at 5 x 9 as the two source views of one stage; the depth map is the first kind's
HOSTILE_LOSS = {"hostile": ("shift", "frac"), "hostile_behind": ("behind", "shift"), "hostile_zero": ("zero", "frac"),
                "hostile_huge": ("huge", "shift")}
KEEP_KNIFE = {"2x1x24x32": 3, "3x2x13x37": 3}                # cases that keep a few genuine knife-edge pixels (under the CAP)
UNSUP_SHAPES = ((1, 1, 3, 3), (2, 1, 24, 32), (2, 2, 7, 9), (1, 5, 24, 32), (1, 8, 11, 13), (3, 2, 13, 37))
UNSUP_CASES = tuple(f"{B}x{Vs}x{H}x{W}{tail}" for (B, Vs, H, W) in UNSUP_SHAPES for tail in ("", "_blind")) + tuple(HOSTILE_LOSS)


def relative_coefs(ref_cam, src_cams):
    """{M, t} of p = M (x,y,1)^T d + t composed in fp64 (homography.py:9-56; the projection keeps the REFERENCE view's K):
    ref_cam (B,2,4,4), src_cams (B,Vs,2,4,4) -> (Vs,B,12) fp64."""
    ref, src = ref_cam.double().unsqueeze(1), src_cams.double()
    K = ref[:, :, 1, :3, :3]
    R = src[:, :, 0, :3, :3] @ ref[:, :, 0, :3, :3].transpose(-1, -2)
    t = src[:, :, 0, :3, 3:4] - R @ ref[:, :, 0, :3, 3:4]
    return torch.cat(((K @ R @ torch.linalg.inv(K)).flatten(-2), (K @ t).flatten(-2)), -1).transpose(0, 1).contiguous()


def _knife_map(coef, depth):
    B, H, W = depth.shape
    k = torch.zeros(B, H, W, dtype=torch.bool)
    for v in range(coef.shape[0]):
        x, y, _ = warp_positions(coef[v], depth.double())
        k |= near_integer(x, W, exact_axis(x, W)) | near_integer(y, H, exact_axis(y, H))
    return k


@functools.lru_cache(maxsize=None)
def unsup_case(name):
    """-> dict(ref (B,H,W,3), srcs (Vs,B,H,W,3), depth (B,H,W), cams or None, coef64 (Vs,B,12), blind).  Synthetic images and stage-3
    cameras, the source cameras shifted differently per batch item (so that the items' tables differ); "_blind": the last source
    camera is translated away and sees nothing.  Depths whose source position falls within 2 KNIFE of an integer are redrawn, so
    that (almost) every pixel is decidable; the cases of KEEP_KNIFE keep up to three genuine knife-edge pixels, which the tests
    exclude under the CAP and which widen their scalar bounds.  HOSTILE_LOSS: the two source views are hand-built tables of
    hostile_warp_case at 5 x 9 -- exact positions on and beside every border, pz < 0 (negative depth and m2 = -1), a column with
    pz == 0 exactly, positions beyond +-1e9 (in both views of "hostile_huge": the depth block of 2^-20 sends the "shift" table
    out as well)."""
    if name in HOSTILE_LOSS:
        H, W = 5, 9
        parts = [hostile_warp_case(H, W, k) for k in HOSTILE_LOSS[name]]
        srcs = torch.stack([p[0] for p in parts])
        g = torch.Generator().manual_seed(17)
        ref = srcs[0].roll(1, 2) + 0.1 * torch.randn(2, H, W, 3, generator=g)
        return {"ref": ref.contiguous(), "srcs": srcs.contiguous(), "depth": parts[0][1].clone(), "cams": None,
                "coef64": torch.stack([p[2] for p in parts]).double(), "blind": False}
    shape, _, tail = name.partition("_")
    B, Vs, H, W = (int(s) for s in shape.split("x"))
    imgs = synthetic.images(B, Vs + 1, H, W, 3)
    cams = synthetic.proj_matrices(B, Vs + 1, H, W)["stage3"].clone()
    for b in range(B):
        cams[b, 1:, 0, :3, 3] += b * torch.tensor([4.0, -3.0, 2.0])
    if tail == "blind":
        cams[:, Vs, 0, :3, 3] += torch.tensor([5.0e4, 0.0, 0.0])
    coef64 = relative_coefs(cams[:, 0], cams[:, 1:])
    g = torch.Generator().manual_seed(7)
    depth = 600.0 + 60.0 * torch.rand(B, H, W, generator=g)
    flat_pair = H >= 7                                        # one exactly flat pair: the sign(0) convention of the smoothness gradient
    kept = None
    for _ in range(40):
        if flat_pair:
            depth[0, 2, 3] = depth[0, 2, 2]
        if kept is None:                                      # the first few knife-edge pixels of the first draw stay as they are
            first = _knife_map(coef64, depth).reshape(-1).nonzero().reshape(-1)[: KEEP_KNIFE.get(name, 0)]
            kept = torch.zeros(B * H * W, dtype=torch.bool)
            kept[first] = True
            kept = kept.reshape(B, H, W)
        x_bad = torch.zeros(B, H, W, dtype=torch.bool)
        for v in range(Vs):
            x, y, _ = warp_positions(coef64[v], depth.double())
            x_bad |= ((x - x.round()).abs() < 2 * KNIFE) | ((y - y.round()).abs() < 2 * KNIFE)
        x_bad &= ~kept
        if not bool(x_bad.any()):
            break
        if flat_pair:
            x_bad[0, 2, 2] |= x_bad[0, 2, 3]
        depth = torch.where(x_bad, 600.0 + 60.0 * torch.rand(B, H, W, generator=g), depth)
    ref = imgs[:, 0].permute(0, 2, 3, 1).contiguous()
    srcs = imgs[:, 1:].permute(1, 0, 3, 4, 2).contiguous()
    return {"ref": ref, "srcs": srcs, "depth": depth.contiguous(), "cams": cams, "coef64": coef64, "blind": tail == "blind"}


def dilate3(m):
    return torch.nn.functional.max_pool2d(m.float().unsqueeze(1), 3, 1, 1).squeeze(1) > 0


@functools.lru_cache(maxsize=None)
def unsup_reference(name):
    """fp64: the three terms, the per-view scalar losses, the winner map, d term / d depth for each term, and what a test needs to
    decide which pixels are comparable: knife (position within KNIFE of an integer in some view), pz_bad (|pz| below 1e-6 of its
    range in some view: the position is p / 1e-10), wild (a masked sample beyond WILD px in some view, pinned -- see `bilinear` --
    and constant, so its own gradient is not comparable), flat, tie.  Computed once per case; callers must not modify it."""
    c = unsup_case(name)
    ref, srcs, coef = c["ref"].double(), c["srcs"].double(), c["coef64"]
    Vs, B, H, W, _ = srcs.shape
    depth = c["depth"].double().requires_grad_(True)
    L, masks, ssim, flip_cost, pz_bad, ssim_max = [], [], 0.0, [], torch.zeros(B, H, W, dtype=torch.bool), 0.0
    wild = torch.zeros(B, H, W, dtype=torch.bool)
    for v in range(Vs):
        x, y, pz = warp_positions(coef[v], depth)
        warped, mask, w = bilinear(srcs[v], x, y, pin=warp_sample_fp32(c["srcs"][v], coef[v], c["depth"]))
        wild |= w
        L.append(O.reconstr_loss(warped, ref, mask.unsqueeze(-1)))
        masks.append(mask)
        if v < 2:
            s = O.ssim(ref, warped, mask.unsqueeze(-1))
            ssim = ssim + s.mean()
            ssim_max = max(ssim_max, float(torch.clamp((1 - _ssim_raw(ref, warped)) / 2, 0, 1).max()))
        # a mask flip at one pixel moves a - b there from 0 to e = warped - ref (or back): the photometric sum by <= sum_c |e_c|, the
        # two x- and the two y-differences that hold the pixel by as much each (smooth-L1 is 1-Lipschitz)
        E = float((warped - ref).detach().abs().sum(-1).max())
        n, nx, ny = B * H * W * 3.0, B * H * (W - 1) * 3.0, B * (H - 1) * W * 3.0
        flip_cost.append(0.5 * E * (1.0 / n + 2.0 / nx + 2.0 / ny))
        pz_bad |= pz.detach().abs() < 1e-6 * float(pz.detach().abs().max())
    L, masks = torch.stack(L), torch.stack(masks)
    vol = L.reshape(Vs, 1, 1, 1) + 1e4 * (1.0 - masks)
    best, winner = vol.min(0)
    winner = torch.where(best < 1e4, winner, torch.full_like(winner, -1))
    reconstr = (best * (best < 1e4)).sum() / (B * H * W)
    smooth = O.depth_smoothness(depth.unsqueeze(-1), ref)
    grads = [torch.autograd.grad(t, depth, retain_graph=True, allow_unused=True)[0] for t in (reconstr, ssim, smooth)]
    grads = [torch.zeros_like(depth) if gd is None else gd for gd in grads]
    Ld = L.detach()
    # two views whose scalar losses tie to fp32 accuracy: where both are valid the winner is not decidable
    tie = torch.zeros(B, H, W, dtype=torch.bool)
    for a in range(Vs):
        for b in range(a + 1, Vs):
            if abs(float(Ld[a] - Ld[b])) <= 1e-5 * max(float(Ld[a]), float(Ld[b]), 1e-30):
                tie |= (masks[a] > 0) & (masks[b] > 0)
    d = depth.detach()
    flat = torch.zeros(B, H, W, dtype=torch.bool)
    fx, fy = d[:, :, 1:] == d[:, :, :-1], d[:, 1:] == d[:, :-1]
    flat[:, :, 1:] |= fx
    flat[:, :, :-1] |= fx
    flat[:, 1:] |= fy
    flat[:, :-1] |= fy
    return {"reconstr": float(reconstr.detach()), "ssim": float(ssim.detach()) if Vs else 0.0, "smooth": float(smooth.detach()), "L": Ld, "masks": masks.detach(), "winner": winner,
            "grads": grads, "knife": _knife_map(coef, c["depth"]), "tie": tie, "flat": flat, "pz_bad": pz_bad, "wild": wild, "flip_cost": flip_cost,
            "ssim_max": ssim_max}


def _ssim_raw(x, y):
    pool = lambda t: torch.nn.functional.avg_pool2d(t.permute(0, 3, 1, 2), 3, 1)   # noqa: E731
    mx, my = pool(x), pool(y)
    n = (2 * mx * my + O.SSIM_C1) * (2 * (pool(x * y) - mx * my) + O.SSIM_C2)
    d = (mx ** 2 + my ** 2 + O.SSIM_C1) * ((pool(x * x) - mx ** 2) + (pool(y * y) - my ** 2) + O.SSIM_C2)
    return (n / d).detach()


# ---------------------------------------------------------------------------------------------------------------------
# masked smooth-L1
# ---------------------------------------------------------------------------------------------------------------------
SL1_SIZES = (1, 255, 257, 524288 + 257)
SL1_MASKS = ("random", "ones", "zeros", "threshold")


def sl1_case(n, mask_kind):
    """pred, target, mask (n,) fp32.  Values are multiples of 2^-6 below 8, so pred - target, 0.5 z^2 and |z| - 0.5 are exact in fp32
    and the only rounding left in the forward is the addition of a thread's partial sum; the differences include exactly +-1 and
    +-(1 +- 2^-6)."""
    g = torch.Generator().manual_seed(n % 1000 + len(mask_kind))
    target = torch.randint(-256, 256, (n,), generator=g).float() / 64.0
    z = torch.randint(-192, 193, (n,), generator=g).float() / 64.0
    edge = torch.tensor([1.0, -1.0, 1.0 - 2.0 ** -6, 1.0 + 2.0 ** -6, -1.0 + 2.0 ** -6, -1.0 - 2.0 ** -6, 0.0])
    z[: min(n, 7)] = edge[torch.arange(min(n, 7))] if n >= 7 else edge[:n]
    if n > 7:
        z[-7:] = edge
    pred = target + z
    if mask_kind == "random":
        mask = (torch.rand(n, generator=g) < 0.6).float()
        mask[0] = 1.0
    elif mask_kind == "ones":
        mask = torch.ones(n)
    elif mask_kind == "zeros":
        mask = torch.zeros(n)
    else:                                                     # > 0.5 selects: exactly 0.5 does not, its successor does
        vals = torch.tensor([0.5, float(np.nextafter(np.float32(0.5), np.float32(1.0))), 0.49])
        mask = vals[torch.arange(n) % 3] if n > 1 else vals[1:2].clone()
    return pred.contiguous(), target.contiguous(), mask.contiguous()


def sl1_reference(pred, target, mask):
    """-> sum, count, d mean / d pred in fp64 (F.smooth_l1_loss(pred[m], target[m]); zero gradient outside the selection)."""
    p = pred.double().requires_grad_(True)
    m = mask > 0.5
    z = p[m] - target.double()[m]
    a = z.abs()
    per = torch.where(a < 1.0, 0.5 * a * a, a - 0.5)
    total, count = per.sum(), int(m.sum())
    grad = torch.zeros_like(p) if count == 0 else torch.autograd.grad(total / count, p)[0]
    return float(total), count, grad


# ---------------------------------------------------------------------------------------------------------------------
# Gaussian-uniform sampler
# ---------------------------------------------------------------------------------------------------------------------
GU_S = (2, 3, 64, 65, 127, 129, 1000, 4096)
GU_N = (2, 6)


@functools.lru_cache(maxsize=None)
def gu_case(N, S, H=5, W=7):
    """pix holds the image corners; the Gaussian rays' eps have exact duplicates; with N = 6 the pseudo depth of ray 1 equals `near`
    (sigma == 0: all its samples are equal); u holds 0 and the largest float below 1."""
    from oracle import render as orr
    batch = synthetic.render_batch(3, H, W, 0)
    g = torch.Generator().manual_seed(N * 10000 + S)
    imgs = orr.unpreprocess(batch["imgs"])
    w2c, c2w, K, nf = batch["w2cs"][0, 0], batch["c2ws"][0, 0], batch["intrinsics"][0, 0], batch["near_fars"][0, 0]
    corners = [(0, 0), (W - 1, H - 1), (W - 1, 0), (0, H - 1), (3, 2), (2, 4)]
    pix = torch.tensor(corners[:N] if N <= 6 else corners + [(1, 1)] * (N - 6)).t().contiguous()
    pseudo = 500.0 + 300.0 * torch.rand(H, W, generator=g)
    if N >= 4:
        pseudo[pix[1, 1], pix[0, 1]] = nf[0]
    eps = torch.randn(N, S, generator=g)
    eps[:, S // 2] = eps[:, 0]                                # ties
    if S >= 8:
        eps[:, 5] = eps[:, 0]
        eps[:, S - 1] = eps[:, 3]
    u = torch.rand(N // 2, S, generator=g)
    u[:, 0] = 0.0
    u[:, -1] = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    cam = torch.cat((K.reshape(-1), c2w.reshape(-1), w2c.reshape(-1), K.reshape(-1), nf))
    return {"pseudo": pseudo, "img0": imgs[0, 0].contiguous(), "pix": pix, "eps": eps, "u": u, "cam": cam, "w2c": w2c, "c2w": c2w,
            "K": K, "near": nf[0], "far": nf[1]}


def gu_reference(c):
    """oracle.render.gaussian_uniform_samples / build_rays restated in fp64 (the oracle's own scalar-times-tensor products stay in
    fp32): z and the strata of the uniform rays, the unsorted Gaussian draws in fp32 (same operation order as the kernel, which
    compiles with contraction off), directions and the exact gathers."""
    pix, eps, u = c["pix"], c["eps"], c["u"]
    N, S = eps.shape
    near, far = c["near"], c["far"]
    mu = c["pseudo"][pix[1], pix[0]]
    sigma = torch.min(torch.abs(far - mu), torch.abs(mu - near)) / 3
    gauss32 = mu.unsqueeze(1) + sigma.unsqueeze(1) * eps
    t = torch.linspace(0.0, 1.0, steps=S).double().reshape(1, S)          # the fp32 linspace of the reference, then fp64
    lin = near.double() * (1.0 - t) + far.double() * t
    mids = 0.5 * (lin[:, 1:] + lin[:, :-1])
    lo, hi = torch.cat([lin[:, :1], mids], -1), torch.cat([mids, lin[:, -1:]], -1)
    z64 = torch.sort(mu.double().unsqueeze(1) + sigma.double().unsqueeze(1) * eps.double(), dim=1).values
    z64[N // 2:] = lo + (hi - lo) * u.double()
    K, c2w = c["K"].double(), c["c2w"].double()
    d = torch.stack([(pix[0].double() - K[0, 2]) / K[0, 0], (pix[1].double() - K[1, 2]) / K[1, 1], torch.ones(N, dtype=torch.float64)], -1)
    dirs = d @ c2w[:3, :3].t()
    return {"gauss32": gauss32, "z64": z64, "lo": lo, "hi": hi, "dirs": dirs, "origin": c2w[:3, 3], "rdepth": mu,
            "target": c["img0"][:, pix[1], pix[0]].t().contiguous()}


def gu_points(c, r, z):
    """pts and ndc in fp64 of the sampler's own z (N,S) (so the comparison is of the projection alone)."""
    from oracle import render as orr
    H, W = c["pseudo"].shape
    pts = r["origin"].reshape(1, 1, 3) + z.double().unsqueeze(-1) * r["dirs"].unsqueeze(1)
    inv = torch.tensor([W - 1, H - 1], dtype=torch.float64)
    return pts, orr.ndc_coordinate(c["w2c"].double(), c["K"].double(), pts, inv, c["near"].double(), c["far"].double())


# ---------------------------------------------------------------------------------------------------------------------
# point features: the image part (render_utils.py:247-279): border-padded bilinear RGB and the strict in-bounds mask
# ---------------------------------------------------------------------------------------------------------------------
PF_H, PF_W = 5, 9                                             # W - 1 = 8, H - 1 = 4: g = q / (n - 1) * 2 - 1 is exact for dyadic q


@functools.lru_cache(maxsize=None)
def point_image_case(M):
    """imgs (3,3,H,W), poses (3,25) = [w2c | K], pts (M,3).  Pose 0 is the identity with K = [[8,0,4],[0,4,2],[0,0,1]]: a point
    (X, Y, 1) projects to (8 X + 4, 4 Y + 2), so X = +-0.5 / Y = +-0.5 sit exactly on g = +-1 in both precisions.  Poses 1 and 2
    are small rigid motions.  Rows cycle through: in front of every camera; exactly on g = +-1 of pose 0; behind the cameras
    (Z < 0); Z == 0 (qz == 0 in pose 0: +-inf or, with X == 0 or Y == 0, NaN)."""
    g = torch.Generator().manual_seed(M)
    imgs = torch.rand(3, 3, PF_H, PF_W, generator=g)
    K0 = torch.tensor([[8.0, 0.0, 4.0], [0.0, 4.0, 2.0], [0.0, 0.0, 1.0]])
    poses = [torch.cat((torch.eye(4).reshape(16), K0.reshape(9)))]
    for i, (ang, t) in enumerate(((0.11, (0.2, -0.1, 0.3)), (-0.07, (-0.3, 0.15, 0.1)))):
        c, s = float(np.cos(ang)), float(np.sin(ang))
        w2c = torch.eye(4)
        w2c[:3, :3] = torch.tensor([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
        w2c[:3, 3] = torch.tensor(t)
        Ki = torch.tensor([[7.3 + i, 0.0, 4.2], [0.0, 3.9, 1.8 + 0.3 * i], [0.0, 0.0, 1.0]])
        poses.append(torch.cat((w2c.reshape(16), Ki.reshape(9))))
    pts = torch.empty(M, 3)
    pts[:, 0] = -0.9 + 1.8 * torch.rand(M, generator=g)
    pts[:, 1] = -0.9 + 1.8 * torch.rand(M, generator=g)
    pts[:, 2] = 1.0 + 2.0 * torch.rand(M, generator=g)
    on_edge = torch.tensor([[0.5, 0.25, 1.0], [-0.5, 0.25, 1.0], [0.25, 0.5, 1.0], [0.25, -0.5, 1.0], [0.5, 0.5, 1.0], [-0.5, -0.5, 1.0],
                            [1.0, 0.125, 2.0], [-1.0, -1.0, 2.0], [0.5 - 2.0 ** -10, 0.0, 1.0], [0.5 + 2.0 ** -10, 0.0, 1.0]])
    zero = torch.tensor([[0.3, 0.2, 0.0], [-0.3, -0.2, 0.0], [0.0, 0.0, 0.0], [0.0, 0.4, 0.0], [-0.7, 0.0, 0.0]])
    idx = torch.arange(M)
    kind = idx % 4 if M > 1 else torch.ones(1, dtype=torch.long)
    sel = kind == 1
    pts[sel] = on_edge[(idx[sel] // 4) % len(on_edge)]
    sel = kind == 2
    pts[sel, 2] = -pts[sel, 2]
    sel = kind == 3
    pts[sel] = zero[(idx[sel] // 4) % len(zero)]
    return imgs.contiguous(), torch.stack(poses).contiguous(), pts.contiguous()


def point_image_reference(imgs, poses, pts, nimg):
    """-> rgb (M,nimg,3), mask (M,nimg), margin (M,nimg) = distance of |g| from 1 (the mask is decidable in fp32 where it is exactly 0
    -- the dyadic rows -- or well above the coordinate rounding), all fp64.  grid_sample's border padding clips the pixel coordinate;
    ATen's clip sends NaN to 0."""
    M = pts.shape[0]
    H, W = imgs.shape[-2:]
    rgb, mask, margin = torch.zeros(M, nimg, 3, dtype=torch.float64), torch.zeros(M, nimg, dtype=torch.float64), torch.zeros(M, nimg, dtype=torch.float64)
    for i in range(nimg):
        w2c, K = poses[i, :16].double().reshape(4, 4), poses[i, 16:].double().reshape(3, 3)
        q = (pts.double() @ w2c[:3, :3].t() + w2c[:3, 3]) @ K.t()
        gx, gy = (q[:, 0] / q[:, 2] + 0.0) / (W - 1) * 2.0 - 1.0, (q[:, 1] / q[:, 2] + 0.0) / (H - 1) * 2.0 - 1.0
        mask[:, i] = ((gx > -1.0) & (gx < 1.0) & (gy > -1.0) & (gy < 1.0)).double()
        margin[:, i] = torch.minimum((gx.abs() - 1.0).abs(), (gy.abs() - 1.0).abs()).nan_to_num(nan=1.0)
        ix, iy = ((gx + 1.0) / 2.0 * (W - 1)).clamp(0, W - 1).nan_to_num(nan=0.0), ((gy + 1.0) / 2.0 * (H - 1)).clamp(0, H - 1).nan_to_num(nan=0.0)
        x0, y0 = ix.floor(), iy.floor()
        img = imgs[i].double()
        for dy in (0, 1):
            for dx in (0, 1):
                xx, yy = x0 + dx, y0 + dy
                w = ((ix - x0) if dx else (x0 + 1 - ix)) * ((iy - y0) if dy else (y0 + 1 - iy))
                ok = (xx <= W - 1) & (yy <= H - 1)
                val = img[:, yy.clamp(0, H - 1).long(), xx.clamp(0, W - 1).long()].t()
                rgb[:, i] += val * torch.where(ok, w, torch.zeros_like(w)).unsqueeze(-1)
    return rgb, mask, margin
