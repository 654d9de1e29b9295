"""GPU: the self-supervised losses on the HIP path (rc_mvsnet_amd/losses.py over rcmvs_unsup_loss_fwd/_bwd,
rcmvs_inverse_warp, rcmvs_masked_sl1_*) against the reference's golden values (tests/golden/unsup_loss.npz, produced by
importing losses/unsup_loss.py, losses/aug_loss.py, losses/homography.py) and against the oracle's autograd."""
import os

import numpy as np
import pytest
import torch

import loss_render_cases as LR
from oracle import unsup_loss as O
from rc_mvsnet_amd import _lib, losses, synthetic

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "unsup_loss.npz"))
STAGES = ("stage1", "stage2", "stage3")
DLOSSW = [0.5, 1.0, 2.0]
DEV = "cuda:0"


def case(tag):
    B, V, H, W, seed = [int(x) for x in GOLD[tag + ":dims"]]
    return B, V, H, W, synthetic.images(B, V, H, W, seed), synthetic.proj_matrices(B, V, H, W)


def grad_check(got, want, med=1e-5, frac=5e-3):
    err = (got.cpu() - want).abs()
    scale = float(want.abs().max())
    assert float(err.median()) <= med * scale, (float(err.median()), scale)
    assert float((err > 1e-3 * scale).float().mean()) <= frac            # knife-edge floor() decisions only


@pytest.mark.parametrize("tag", ["a", "b"])
def test_unsup_loss_multi_stage_matches_reference(tag):
    _lib.load()
    B, V, H, W, imgs, cams = case(tag)
    inputs = {k: {"depth": torch.tensor(GOLD[f"{tag}:depth:{k}"]).to(DEV).requires_grad_(True)} for k in STAGES}
    total, scalars = losses.UnsupLossMultiStage()(inputs, imgs.to(DEV), {k: v.to(DEV) for k, v in cams.items()}, dlossw=DLOSSW)
    total.backward()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    assert abs(float(total) - float(GOLD[tag + ":total"])) <= 2e-5 * abs(float(GOLD[tag + ":total"]))
    for k, v in scalars.items():
        want = float(GOLD[f"{tag}:{k}"])
        assert abs(float(v) - want) <= 2e-5 * abs(want), (k, float(v), want)
    for k in STAGES:
        grad_check(inputs[k]["depth"].grad, torch.tensor(GOLD[f"{tag}:grad:{k}"]))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_inverse_warping_matches_reference(tag):
    _lib.load()
    B, V, H, W, imgs, cams = case(tag)
    src = losses.stage_image(imgs[:, 1].to(DEV), 1)
    cam = cams["stage2"].to(DEV)
    warped, mask = losses.inverse_warping(src, cam[:, 0], cam[:, 1], torch.tensor(GOLD[f"{tag}:depth:stage2"]).to(DEV))
    want_w, want_m = torch.tensor(GOLD[tag + ":warped2"]), torch.tensor(GOLD[tag + ":mask2"])
    assert mask.shape == want_m.shape and warped.shape == want_w.shape
    same = mask.cpu() == want_m
    assert float((~same).float().mean()) <= 2e-3
    assert float(((warped.cpu() - want_w) * same).abs().max()) < 2e-3


@pytest.mark.parametrize("tag", ["a", "b"])
def test_aug_loss_and_sl1_match_reference(tag):
    _lib.load()
    B, V, H, W, imgs, cams = case(tag)
    inputs = {k: {"depth": torch.tensor(GOLD[f"{tag}:depth:{k}"]).to(DEV).requires_grad_(True)} for k in STAGES}
    fmask = torch.ones(B, 3, H, W)
    fmask[:, :, H // 4:H // 2, W // 8:W // 2] = 0.0
    total, scalars = losses.AugLossMultiStage()(inputs, torch.tensor(GOLD[tag + ":aug:pseudo"]).to(DEV), None, fmask.to(DEV), dlossw=DLOSSW)
    total.backward()
    assert abs(float(total) - float(GOLD[tag + ":aug:total"])) <= 1e-5 * abs(float(GOLD[tag + ":aug:total"]))
    for k, v in scalars.items():
        assert abs(float(v) - float(GOLD[f"{tag}:aug:{k}"])) <= 1e-5 * abs(float(GOLD[f"{tag}:aug:{k}"])), k
    for k in STAGES:
        assert torch.allclose(inputs[k]["depth"].grad.cpu(), torch.tensor(GOLD[f"{tag}:aug:grad:{k}"]), rtol=1e-4, atol=1e-9), k
    # SL1Loss (losses/sl1loss.py): default mask depth_gt > 0, factor 1/2
    g = torch.Generator().manual_seed(3)
    pred = (3.0 * torch.randn(1024, generator=g)).requires_grad_(True)
    gt = 3.0 * torch.randn(1024, generator=g)
    want = torch.nn.functional.smooth_l1_loss(pred[gt > 0], gt[gt > 0]) * 0.5
    want.backward()
    p2 = pred.detach().to(DEV).requires_grad_(True)
    got = losses.SL1Loss()(p2, gt.to(DEV))
    got.backward()
    assert abs(float(got) - float(want)) <= 1e-6 * abs(float(want))
    assert torch.allclose(p2.grad.cpu(), pred.grad, rtol=1e-5, atol=1e-9)


def test_unsup_loss_full_size_against_oracle():
    """BASELINE config 3 shape (4 views, 512x640, batch 1), stage 3: the three terms and the depth gradient against the
    oracle's autograd on the CPU."""
    _lib.load()
    B, V, H, W = 1, 4, 512, 640
    imgs, cams = synthetic.images(B, V, H, W, 5), synthetic.proj_matrices(B, V, H, W)["stage3"]
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    depth = (620.0 + 110.0 * torch.sin(4.0 * xx) * torch.cos(3.0 * yy) + torch.randn(H, W, generator=torch.Generator().manual_seed(6))).unsqueeze(0)
    d_cpu = depth.clone().requires_grad_(True)
    r = O.unsup_loss(imgs, cams, d_cpu, 2)
    r["loss"].backward()
    d_gpu = depth.to(DEV).requires_grad_(True)
    mod = losses.UnSupLoss()
    loss = mod(imgs.to(DEV), cams.to(DEV), d_gpu, 2)
    loss.backward()
    for name, got in (("reconstr", mod.reconstr_loss), ("ssim", mod.ssim_loss), ("smooth", mod.smooth_loss), ("loss", loss)):
        assert abs(float(got) - float(r[name])) <= 2e-5 * abs(float(r[name])), (name, float(got), float(r[name]))
    grad_check(d_gpu.grad, d_cpu.grad)


def test_unsup_loss_argument_checks():
    _lib.load()
    imgs, cams = synthetic.images(1, 3, 32, 40, 0).to(DEV), synthetic.proj_matrices(1, 3, 32, 40)["stage3"].to(DEV)
    depth = torch.full((1, 32, 40), 600.0, device=DEV)
    with pytest.raises(_lib.RcmvsError):
        losses.UnSupLoss()(imgs, cams, depth.double(), 2)                        # fp32 only
    with pytest.raises(_lib.RcmvsError):
        losses.UnSupLoss()(imgs[:, :, :, :2], cams, depth[:, :2], 2)             # SSIM needs 3 rows
    with pytest.raises(_lib.RcmvsError):
        losses.UnSupLoss()(imgs.repeat(1, 4, 1, 1, 1)[:, :10], cams.repeat(1, 4, 1, 1, 1)[:, :10], depth, 2)   # 9 source views
    # a loss that does not depend on depth leaves a zero gradient, not garbage
    d = depth.clone().requires_grad_(True)
    m = losses.UnSupLoss()
    m(imgs, cams, d, 2)
    (0.0 * m.reconstr_loss + 0.0 * m.ssim_loss + 0.0 * m.smooth_loss).backward()
    assert float(d.grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------
# hostile inputs against plain fp64 references (tests/loss_render_cases.py); re-run on the kernel emulation by test_emu_gpu_suite_cpu.py
# ------------------------------------------------------------------------------------------------
U24 = 2.0 ** -24


def dev(t):
    return t.to(DEV).contiguous()


@pytest.mark.parametrize("kind", LR.WARP_KINDS)
@pytest.mark.parametrize("H,W", LR.WARP_SHAPES)
def test_inverse_warp_hostile_geometry_vs_fp64(H, W, kind):
    """rcmvs_inverse_warp on hand-built {M, t} tables (LR.hostile_warp_case: two batch items with different tables): positions exactly
    on -1, 0, n-2, n-1, n, at -1 + 2^-20, -0.5 and n - 0.5 on every axis whose n - 1 is a power of two (both axes of 5 x 9 and 2 x 2, the
    rows of 9 x 20; the columns of 9 x 20 get generic fractional shifts, since the round trip is inexact there), pz < 0, pz == 0 exactly, positions beyond +-1e9 (the `big` clamp).  The mask
    equals the fp64 rule on every pixel that is not within 1e-3 px of an integer -- the dyadic placements are exact in both precisions
    and are NOT excluded --, at most 1 % may be excluded, `warped` is within 2e-3 where unmasked, and every output is finite.
    Non-finite depth is out of scope: the reference rule itself yields NaN there."""
    _lib.load()
    img, depth, coef = LR.hostile_warp_case(H, W, kind)
    want_w, want_m, excluded = LR.hostile_warp_reference(H, W, kind)
    assert float(excluded.double().mean()) <= LR.CAP
    warped = torch.full((2, H, W, 3), float("nan"), device=DEV)
    mask = torch.full((2, H, W), float("nan"), device=DEV)
    img_d, depth_d, coef_d = dev(img), dev(depth), dev(coef)                   # named: the pointers must outlive the call
    _lib.call("rcmvs_inverse_warp", losses._chk(img_d, "img"), losses._chk(depth_d, "depth"), losses._chk(coef_d, "coef"),
              losses._chk(warped, "warped"), losses._chk(mask, "mask"), 2, H, W, losses._stream())
    warped, mask = warped.cpu().double(), mask.cpu().double()
    assert bool(torch.isfinite(warped).all()) and bool(torch.isfinite(mask).all())
    assert torch.equal(mask[~excluded], want_m[~excluded]), (mask, want_m)
    keep = (~excluded & (want_m > 0)).unsqueeze(-1)
    assert int(keep.sum()) > 0
    err = float(((warped - want_w) * keep).abs().max())
    print(f"inverse warp {H}x{W} {kind}: max err {err:.3e} on {int(keep.sum())} valid pixels")
    assert err < 2e-3


def _stage_buffers(Vs, B, H, W):
    """every output of the two calls, filled with what a stale buffer might hold"""
    f = lambda shape, dtype, v: torch.full(shape, v, device=DEV, dtype=dtype)   # noqa: E731
    return {"warped": f((Vs, B, H, W, 3), torch.float32, 7.0), "masks": f((Vs, B, H, W), torch.float32, 7.0),
            "sums": f((4 * Vs + 2,), torch.float64, 1e30), "counts": f((Vs,), torch.int32, 12345), "out": f((4 + Vs,), torch.float32, 7.0),
            "ws": f((B, H - 2, W - 2, 9), torch.float32, 7.0), "kbuf": f((4 * Vs + 2,), torch.float32, 7.0)}


def _stage_fwd(ref, srcs, depth, coef, buf):
    """rcmvs_unsup_loss_fwd as losses.UnsupStageLossFn calls it, on caller-owned buffers (the product API keeps counts, the
    per-view losses and kbuf to itself)."""
    Vs, B, H, W, _ = srcs.shape
    c = losses._chk
    _lib.call("rcmvs_unsup_loss_fwd", c(ref, "ref"), c(srcs, "srcs"), c(depth, "depth"), c(coef, "coef"), c(buf["warped"], "warped"),
              c(buf["masks"], "masks"), c(buf["sums"], "sums", torch.float64), c(buf["counts"], "counts", torch.int32), c(buf["out"], "out"),
              B, Vs, H, W, losses._stream())
    return buf["out"].cpu().double(), buf["counts"].cpu()


def _stage_bwd(ref, srcs, depth, coef, buf, gout):
    Vs, B, H, W, _ = srcs.shape
    c = losses._chk
    g = torch.tensor(gout, dtype=torch.float32, device=DEV)
    gdepth = torch.full_like(depth, 7.0)
    _lib.call("rcmvs_unsup_loss_bwd", c(ref, "ref"), c(srcs, "srcs"), c(depth, "depth"), c(coef, "coef"), c(buf["warped"], "warped"),
              c(buf["masks"], "masks"), c(buf["counts"], "counts", torch.int32), c(g, "gout"), c(buf["ws"], "ws"), c(buf["kbuf"], "kbuf"),
              c(gdepth, "gdepth"), B, Vs, H, W, losses._stream())
    return gdepth.cpu().double()


# fp32 floor of the per-term gradients against the fp64 reference, measured on the MI355X and on the kernel emulation (same figures):
# the largest per-entry error over all cases is 5.8e-6 of the term's max |grad| (reconstruction), 7.4e-6 (SSIM), 1.3e-7 (smoothness)
# -- below the bound, which therefore stays at the 1e-4 asked for
_GRAD_TOL = 1e-4


@pytest.mark.parametrize("name", LR.UNSUP_CASES)
def test_unsup_loss_terms_one_by_one_vs_fp64(name):
    """One stage of the loss on the device, each term on its own, against LR.unsup_reference (fp64 positions, fp64 oracle terms, fp64
    autograd of ONE term): out[0..2], the per-view losses out[4 + v], counts against the winner map, d term / d depth for gout =
    (1,0,0), (0,1,0), (0,0,1) with the term's own max |grad| as scale and no share of pixels that may be anything, their sum against
    the combined call, and a repeat on the same (stale) buffers.  Shapes whose pixel count is no multiple of 256, one to eight source
    views, different tables per batch item, a source view that sees nothing ("_blind": count 0), and the hand-built tables as source views
    (LR.HOSTILE_LOSS): exact positions on and beside every border, pz < 0, pz == 0 exactly, positions beyond 1e9.  Samples beyond
    1e6 px are masked but enter SSIM windows; they are fp32 rounding noise (LR.bilinear), pinned in the reference to the documented
    fp32 evaluation, and their own gradient entries are excluded with the 3 x 3 neighbourhood of the pz ~ 0 pixels.  Knife-edge pixels (fp64 position within 1e-3 px of an integer; at most 1 %) widen the scalar bounds by
    what their mask flips can move and are excluded, with their 3 x 3 neighbourhood, from the reconstruction / SSIM gradients; pixels
    with an exactly flat neighbour are excluded from the smoothness gradient (the sign(0) convention)."""
    _lib.load()
    c, R = LR.unsup_case(name), LR.unsup_reference(name)
    Vs, B, H, W, _ = c["srcs"].shape
    n = B * H * W
    coef = c["coef64"].float() if c["cams"] is None else losses.inverse_warp_coefs(c["cams"][:, 0], c["cams"][:, 1:])
    ref, srcs, depth, coef = dev(c["ref"]), dev(c["srcs"]), dev(c["depth"]), dev(coef)
    buf = _stage_buffers(Vs, B, H, W)
    out, counts = _stage_fwd(ref, srcs, depth, coef, buf)
    knife = R["knife"]
    k = int(knife.sum())
    assert k <= LR.CAP * n, (k, n)
    # ---- scalars: 2e-5 relative, widened by k mask flips (LR.unsup_reference: flip_cost per view, the largest SSIM window value)
    Lmax = float(R["L"].max())
    wide_L = [k * fc for fc in R["flip_cost"]]
    wide = {"reconstr": sum(w * float((R["winner"] == v).sum()) / n for v, w in enumerate(wide_L)) + k * Lmax / n,
            "ssim": min(Vs, 2) * k * R["ssim_max"] / (B * (H - 2) * (W - 2)), "smooth": 0.0}
    for i, key in enumerate(("reconstr", "ssim", "smooth")):
        print(f"{name} {key}: got {float(out[i]):.9e} want {R[key]:.9e} widening {wide[key]:.2e}")
        assert abs(float(out[i]) - R[key]) <= 2e-5 * abs(R[key]) + wide[key], (key, float(out[i]), R[key])
    assert abs(float(out[3]) - (12 * R["reconstr"] + 6 * R["ssim"] + 0.18 * R["smooth"])) <= 2e-5 * float(out[3]) + 12 * wide["reconstr"] + 6 * wide["ssim"]
    for v in range(Vs):
        assert abs(float(out[4 + v]) - float(R["L"][v])) <= 2e-5 * float(R["L"][v]) + wide_L[v], (v, float(out[4 + v]), float(R["L"][v]))
    # ---- counts: exact up to the undecidable pixels
    slack = int((knife | R["tie"]).sum())
    for v in range(Vs):
        want = int(((R["winner"] == v) & ~(knife | R["tie"])).sum())
        assert want <= int(counts[v]) <= want + slack, (v, int(counts[v]), want, slack)
    assert int(counts.sum()) <= n
    if c["blind"]:
        assert int(counts[Vs - 1]) == 0 and float(buf["masks"][Vs - 1].abs().max()) == 0.0
    # ---- one-hot backward
    near = LR.dilate3(knife | R["pz_bad"]) | R["wild"]
    assert int((~near).sum()) >= n // 4
    grads = []
    for i, key in enumerate(("reconstr", "ssim", "smooth")):
        got = _stage_bwd(ref, srcs, depth, coef, buf, [float(j == i) for j in range(3)])
        grads.append(got)
        want = R["grads"][i]
        keep = ~(R["flat"] if key == "smooth" else near)
        if not bool(keep.any()):                                          # the constant depth of the hand-built tables: flat everywhere
            continue
        scale = float((want.abs() * keep).max())
        err = float(((got - want).abs()[keep]).max())
        assert bool(torch.isfinite(got[keep]).all())
        print(f"{name} d {key}: scale {scale:.3e} max err {err:.3e} ({err / max(scale, 1e-300):.2e} of scale), {int((~keep).sum())} excluded")
        assert err <= _GRAD_TOL * scale, (key, err, scale)
    # ---- linearity.  Scaling gout by a power of two scales every kbuf factor exactly, so the gradient scales bit for bit, per entry.
    # Additivity: the k factors and their products round ~8 times per path and the SSIM path sums 27 products.  Within one entry the
    # signed terms (five smooth-L1 slopes, four smoothness slopes, three channels) cancel, so the rounding is relative to the terms,
    # not to the entry's own result: 64 u of the largest summed magnitude bounds it; an entry's own magnitude does not
    w = (12.0, 6.0, 0.18)
    for i, f in enumerate((2.0, 4.0, 0.5)):
        scaled = _stage_bwd(ref, srcs, depth, coef, buf, [f * float(j == i) for j in range(3)])
        ok = torch.isfinite(grads[i])
        assert torch.equal(scaled[ok], f * grads[i][ok]), i
    both = _stage_bwd(ref, srcs, depth, coef, buf, list(w))
    kb = buf["kbuf"].clone()
    fin = torch.isfinite(both) & ~near
    mag = sum(abs(wi) * gi.abs() for wi, gi in zip(w, grads))
    assert float(((both - sum(wi * gi for wi, gi in zip(w, grads))).abs()[fin] - 64 * U24 * mag[fin].max()).max()) <= 0.0
    # ---- again on the same buffers, now stale with the first call's sums and counts
    out2, counts2 = _stage_fwd(ref, srcs, depth, coef, buf)
    assert torch.equal(counts2, counts)
    assert float((out2 - out).abs().max()) <= 2.0 ** -23 * float(out.abs().max())      # fp64 atomics in another order: the last fp32 bit at most
    both2 = _stage_bwd(ref, srcs, depth, coef, buf, list(w))
    assert torch.equal(buf["kbuf"], kb) and torch.equal(both2[fin], both[fin])


@pytest.mark.parametrize("mask_kind", LR.SL1_MASKS)
@pytest.mark.parametrize("n", LR.SL1_SIZES)
def test_masked_smooth_l1_vs_fp64(n, mask_kind):
    """rcmvs_masked_sl1_fwd / _bwd: one element, one block +- 1, and 524288 + 257, the first size whose grid-stride loop (2048 blocks
    of 256) runs twice; random, full and EMPTY masks and mask values at the > 0.5 threshold; pred - target exactly +-1 and either
    side.  The inputs are dyadic (LR.sl1_case), so the per-element terms are exact in fp32: the count is exact, and the sum is within
    the fp32 rounding of a thread's partial sum, n_per_thread 2^-24 relative.  The gradient, entrywise against fp64 autograd, carries
    the two roundings of k = gout / count and k * clamp(z): 2^-22 relative.  Empty mask: the loss is NaN as F.smooth_l1_loss of an
    empty selection, the gradient is zero and finite."""
    if DEV == "cpu" and n > 4096 and os.environ.get("RCMVS_EMU_FULL", "0") != "1":
        pytest.skip("half a million elements on the kernel emulation: RCMVS_EMU_FULL=1 (always run on the GPU)")
    _lib.load()
    pred, target, mask = LR.sl1_case(n, mask_kind)
    want_sum, want_count, want_grad = LR.sl1_reference(pred, target, mask)
    p, t, m = dev(pred).requires_grad_(True), dev(target), dev(mask)
    sums = torch.full((2,), 1e30, device=DEV, dtype=torch.float64)
    _lib.call("rcmvs_masked_sl1_fwd", losses._chk(p.detach(), "pred"), losses._chk(t, "target"), losses._chk(m, "mask"),
              losses._chk(sums, "sums", torch.float64), n, losses._stream())
    per_thread = -(-n // (min(-(-n // 256), 2048) * 256))
    assert float(sums[1]) == want_count
    assert abs(float(sums[0]) - want_sum) <= per_thread * U24 * want_sum, (float(sums[0]), want_sum)
    loss = losses.masked_smooth_l1(p, t, m)
    (3.0 * loss).backward()
    got = p.grad.cpu().double()
    assert bool(torch.isfinite(got).all())
    if want_count == 0:
        assert bool(torch.isnan(loss)) and float(got.abs().max()) == 0.0
        return
    assert abs(float(loss) - want_sum / want_count) <= (per_thread + 1) * U24 * want_sum / want_count
    assert float(((got - 3.0 * want_grad).abs() - 2.0 ** -22 * (3.0 * want_grad).abs()).max()) <= 0.0
    assert float(got[mask <= 0.5].abs().max() if bool((mask <= 0.5).any()) else 0.0) == 0.0
