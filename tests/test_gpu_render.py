"""GPU parity tests of the rendering-consistency branch: every HIP
kernel against the CPU oracle (oracle/render.py, oracle/conv3d.py) and against the fixtures captured
from the reference's Rendering_Consistency_Net.forward with injected random draws."""
import os
import types

import pytest
import torch

import loss_render_cases as LR
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def gpu(t):
    return t.to(DEV).contiguous()


@pytest.fixture(scope="module")
def hip():
    from rc_mvsnet_amd import _lib, ops
    _lib.load()
    return ops


def _args(S):
    return types.SimpleNamespace(multires=10, i_embed=0, pts_dim=3, dir_dim=3, netdepth=6, netwidth=128, net_type="v0",
                                 netchunk=1024, ckpt=None, N_samples=S, N_importance=0, perturb=1.0, use_viewdirs=True,
                                 white_bkgd=False, raw_noise_std=0.0, pad=0, img_downscale=1.0, use_color_volume=False,
                                 multires_views=4)


def _net(S):
    from rc_mvsnet_amd import synthetic
    from rc_mvsnet_amd.render_consist_net import Rendering_Consistency_Net
    m = Rendering_Consistency_Net(_args(S))
    m.load_state_dict(synthetic.render_state_dict(1), strict=True)
    return m.to(DEV).eval()


def test_resize_planes(hip):
    from oracle import conv3d as oc
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 41, 6, 8, 12, generator=g)
    ref = oc.resize_depth_align_corners(x, 128)
    y = hip.resize_planes(gpu(x), 128, pad_channels_to=44).cpu()
    assert y.shape == (1, 128, 8, 12, 44)
    assert float(y[..., 41:].abs().max()) == 0.0
    assert rel_err(y[..., :41].permute(0, 4, 1, 2, 3), ref) < 1e-6


def test_neural_volume_vs_golden(hip):
    g = load_golden("render")
    m = _net(16)
    with torch.no_grad():
        vol = m.MVSNet.forward_cl(gpu(g["vfw"]))               # (1,128,h,w,8)
        vol_nc = m.MVSNet(gpu(g["vfw"]))                        # reference layout through the module API
    v = vol.cpu().permute(0, 4, 1, 2, 3)
    assert rel_err(v[:, :, ::8], g["volume"]) < 5e-5
    assert torch.equal(vol_nc.cpu(), v.reshape(1, -1, *v.shape[2:]))


def _rays_case(S, seed=5, H=64, W=96, V=4):
    from rc_mvsnet_amd import synthetic
    from oracle import render as orr
    batch = synthetic.render_batch(V, H, W, 0)
    pix, eps, u = synthetic.render_randoms(H, W, 1024, S, seed)
    g = torch.Generator().manual_seed(seed)
    pseudo = 500.0 + 300.0 * torch.rand(H, W, generator=g)
    pseudo[:4] = 426.0
    imgs = orr.unpreprocess(batch["imgs"])
    w2cs, c2ws, intr, nf = batch["w2cs"][0], batch["c2ws"][0], batch["intrinsics"][0], batch["near_fars"][0]
    rays = orr.build_rays(imgs, pseudo, w2cs, c2ws, intr, nf, pix, eps, u)
    cam = torch.cat((intr[0].reshape(-1), c2ws[0].reshape(-1), w2cs[0].reshape(-1), intr[0].reshape(-1), nf[0]))
    return batch, imgs, pseudo, w2cs, c2ws, intr, nf, pix, eps, u, rays, cam


@pytest.mark.parametrize("S", [16, 128, 20])
def test_gu_sampler_vs_oracle(hip, S):
    batch, imgs, pseudo, w2cs, c2ws, intr, nf, pix, eps, u, rays, cam = _rays_case(S)
    z, pts, ndc, dirs, rdepth, target = hip.gu_sample(gpu(pseudo), gpu(imgs[0, 0]), gpu(pix.to(torch.int32)), gpu(eps), gpu(u), gpu(cam))
    assert torch.equal(rdepth.cpu(), rays["rays_depth"])
    assert torch.equal(target.cpu(), rays["target_s"])
    assert float((z.cpu() - rays["depth_candidates"]).abs().max()) < 2e-4          # mm of ~600: <= 3 ulp
    zc = z.cpu()
    assert bool((zc[:512, 1:] >= zc[:512, :-1]).all())                               # Gaussian half is sorted
    assert rel_err(dirs.cpu(), rays["rays_dir"]) < 1e-6
    assert rel_err(pts.cpu(), rays["rays_pts"]) < 1e-6
    assert float((ndc.cpu() - rays["rays_ndc"]).abs().max()) < 2e-6


def test_point_feats_vs_oracle(hip):
    from oracle import render as orr
    S = 16
    batch, imgs, pseudo, w2cs, c2ws, intr, nf, pix, eps, u, rays, cam = _rays_case(S)
    g = torch.Generator().manual_seed(3)
    vol = torch.randn(1, 8, 24, 16, 24, generator=g)
    # push some points outside the volume / images to exercise zeros / border padding and the mask
    rays["rays_ndc"][:8] = rays["rays_ndc"][:8] * 3.0 - 1.0
    rays["rays_pts"][8:16] = rays["rays_pts"][8:16] * 4.0
    ref = orr.point_features(vol, imgs[:, -3:], w2cs, intr, rays["rays_pts"], rays["rays_ndc"])
    poses = torch.cat((w2cs[:3].reshape(3, 16), intr[:3].reshape(3, 9)), dim=1)
    feat = hip.point_feats(gpu(vol[0].permute(1, 2, 3, 0)), gpu(imgs[0, -3:]), gpu(poses), gpu(rays["rays_pts"]), gpu(rays["rays_ndc"]), ldf=32)
    out = feat.cpu()[:, :20].reshape(1024, S, 20)
    assert rel_err(out[..., :8], ref[..., :8]) < 1e-5
    assert rel_err(out[..., 8:], ref[..., 8:]) < 1e-5
    assert torch.equal(out[..., 11], ref[..., 11]) and torch.equal(out[..., 19], ref[..., 19])   # masks


def test_nerf_mlp_vs_oracle(hip):
    """(the oracle MLP itself is pinned to the reference's RenderNet by tests/golden/nerf_mlp.npz on the CPU)"""
    from oracle import render as orr
    from rc_mvsnet_amd import synthetic
    sd = synthetic.render_state_dict(1)
    m = _net(16)
    gen = torch.Generator().manual_seed(11)
    N, S = 64, 16
    ndc = torch.rand(N, S, 3, generator=gen)
    feat20 = torch.randn(N * S, 20, generator=gen) * 0.5
    dirs = torch.randn(N, 3, generator=gen)
    w2c = synthetic.render_batch(4, 64, 96, 0)["w2cs"][0, 0]
    ang = (dirs / torch.norm(dirs, dim=-1, keepdim=True)) @ w2c[:3, :3].t()
    ref = orr.nerf_mlp(orr.embed(ndc).reshape(N * S, -1), feat20, ang[:, None].expand(-1, S, -1).reshape(N * S, 3), sd).reshape(N, S, 4)
    feat = torch.zeros(N * S, 32)
    feat[:, :20] = feat20
    feat[:, 20:] = 7.0                                                             # padding must be cleared by the kernel
    raw = hip.nerf_mlp(gpu(ndc), gpu(feat), gpu(dirs), gpu(w2c), m.network_fn.hip_blob()).cpu()
    print(f"MLP max err {float((raw - ref).abs().max()):.3e}")
    assert rel_err(raw, ref) < 5e-5


def test_rendernet_forward_on_its_own_vs_reference_golden(hip):
    """RenderNet.forward / Renderer_ours.forward / forward_alpha called directly (models/render_models.py:175-220,538-565) on rows that are
    already [embedded point | point feature | view direction]: against the reference's own `network_fn` on the same weights
    (tests/golden/nerf_mlp.npz), batch shape kept; the module explains itself on a foreign configuration, with gradients, off the device."""
    from rc_mvsnet_amd import synthetic
    from rc_mvsnet_amd.render_consist_net import RenderNet, Renderer_ours
    g = load_golden("nerf_mlp")
    net = RenderNet(D=6, W=128, input_ch_pts=63, input_ch_views=3, input_ch_feat=20, skips=[4], net_type="v0")
    net.load_state_dict({k[len("network_fn."):]: v for k, v in synthetic.render_state_dict(1).items() if k.startswith("network_fn.")}, strict=True)
    net = net.to(DEV).eval()
    x = gpu(g["x"])
    with torch.no_grad():
        out = net(x)
        alpha = net.forward_alpha(x[..., :83])
        out2 = net.nerf(x.reshape(-1, 86))
    assert out.shape == (64, 16, 4) and alpha.shape == (64, 16, 1)
    assert rel_err(out.cpu(), g["out"]) < 5e-5
    assert torch.equal(alpha[..., 0], out[..., 3]) and torch.equal(out2.reshape(64, 16, 4), out)
    with pytest.raises(Exception, match="no_grad|train|GPU"):
        net(x)                                                           # eval mode with autograd on
    with torch.no_grad():
        with pytest.raises(Exception, match="86"):
            net(x[..., :80])
        with pytest.raises(Exception, match="create_nerf_mvs"):
            Renderer_ours(D=8, W=256, use_viewdirs=True).to(DEV).eval()(x)


def test_composite_vs_oracle(hip):
    from oracle import render as orr
    gen = torch.Generator().manual_seed(2)
    for (N, S) in ((1024, 128), (64, 16), (10, 37)):
        raw = torch.rand(N, S, 4, generator=gen)
        raw[..., 3] = torch.relu(torch.randn(N, S, generator=gen)) * 0.3
        z = torch.sort(425 + 500 * torch.rand(N, S, generator=gen), dim=1).values
        ref = orr.composite(raw, z)
        rgb, depth, weights, alpha = hip.composite(gpu(raw), gpu(z))
        assert rel_err(alpha.cpu(), ref["alpha"]) < 1e-6
        assert rel_err(weights.cpu(), ref["weights"]) < 2e-6
        assert rel_err(rgb.cpu(), ref["rgb_map"]) < 1e-5
        assert float((depth.cpu() - ref["depth_map"]).abs().max()) < 2e-3
        assert float(weights.sum(1).max()) <= 1.0 + 1e-5


def test_render_forward_vs_reference_golden(hip):
    """Full Rendering_Consistency_Net.forward on the HIP path with the reference's captured draws."""
    from rc_mvsnet_amd import synthetic
    g = load_golden("render")
    H, W, V = int(g["H"]), int(g["W"]), int(g["V"])
    m = _net(16)
    batch = {k: gpu(v) for k, v in synthetic.render_batch(V, H, W, 0).items()}
    with torch.no_grad():
        rgb, feat, wts, dpred, alpha, _, rdepth, target = m(gpu(g["vfw"]), gpu(g["pseudo"]), batch,
                                                             randoms=(gpu(g["pix"]), gpu(g["eps"]), gpu(g["u"])))
    assert torch.equal(rdepth.cpu(), g["rays_depth"])
    assert rel_err(target.cpu(), g["target"]) < 1e-6
    # Rays through border pixels re-project onto |grid| == 1 exactly, where the strict in-bounds mask
    # (render_utils.py:273) is decided by the last ulp: compare those rays' masks statistically and
    # keep them out of the downstream comparisons.
    px, py = g["pix"][0], g["pix"][1]
    interior = (px > 0) & (px < W - 1) & (py > 0) & (py < H - 1)
    f, gf = feat.cpu()[::4], g["feat"]
    mask_cols = [11, 15, 19]
    other = [c for c in range(20) if c not in mask_cols]
    assert rel_err(f[..., other], gf[..., other]) < 2e-4
    assert float((f[..., mask_cols] != gf[..., mask_cols]).float().mean()) < 0.01
    assert torch.equal(f[interior[::4]][..., mask_cols], gf[interior[::4]][..., mask_cols])
    assert rel_err(alpha.cpu()[interior], g["alpha"][interior]) < 5e-4
    assert rel_err(wts.cpu()[interior], g["weights"][interior]) < 5e-4
    assert rel_err(rgb.cpu()[interior], g["rgb"][interior]) < 5e-4
    dd = (dpred.cpu() - g["depth"]).abs()[interior]
    print(f"render depth max err {float(dd.max()):.3e} mm over {int(interior.sum())} interior rays")
    assert float(dd.max()) / 500.0 < 5e-4


@pytest.mark.parametrize("ci,co,stride", [(41, 8, 1), (8, 16, 2), (16, 16, 1)])
def test_conv_bn_relu3d_block_on_its_own(hip, ci, co, stride):
    """ConvBnReLU3D (models/render_models.py:675-686: conv + norm, no ReLU) called as a module of its own -- what `CostReg` runs through
    its plan -- against the same layer in PyTorch-CPU fp64."""
    from rc_mvsnet_amd.render_consist_net import ConvBnReLU3D
    torch.manual_seed(ci + co)
    m = ConvBnReLU3D(ci, co, stride=stride)
    with torch.no_grad():
        m.bn.running_mean.normal_(0, 0.1); m.bn.running_var.uniform_(0.5, 1.5); m.bn.weight.uniform_(0.5, 1.5); m.bn.bias.normal_(0, 0.1)
    x = torch.randn(1, ci, 8, 16, 24)
    with torch.no_grad():
        want = torch.nn.functional.batch_norm(torch.nn.functional.conv3d(x.double(), m.conv.weight.double(), stride=stride, padding=1),
                                              m.bn.running_mean.double(), m.bn.running_var.double(), m.bn.weight.double(), m.bn.bias.double(),
                                              False, 0.0, m.bn.eps)
        got = m.to(DEV).eval()(gpu(x))
        again = m(gpu(x))
    assert tuple(got.shape) == tuple(want.shape) and torch.equal(got, again)
    assert rel_err(got.cpu().double(), want) < 2e-5


def test_render_forward_five_view_extension_vs_reference_golden(hip):
    """The flagged extension `args.num_views = 5` (BASELINE configs[2] as worded): the volume network takes the 44-channel warped volume
    feature of a five-view CascadeMVSNet pass; the renderer behind it is the reference's (last three images, first three poses of the batch).  Golden: the reference's own module with
    that one constructor argument changed (tests/golden/make_golden.py: render_v5_fixture), five-view batch, injected draws."""
    from rc_mvsnet_amd import synthetic
    from rc_mvsnet_amd.render_consist_net import Rendering_Consistency_Net
    g = load_golden("render_v5")
    H, W, V = int(g["H"]), int(g["W"]), int(g["V"])
    assert V == 5
    a = _args(16)
    a.num_views = 5
    m = Rendering_Consistency_Net(a)
    assert m.MVSNet.cost_reg_2.conv0.conv.weight.shape[1] == 44
    m.load_state_dict(synthetic.render_state_dict(1, vol_src=4), strict=True)
    m = m.to(DEV).eval()
    batch = {k: gpu(v) for k, v in synthetic.render_batch(V, H, W, 0).items()}
    pix, eps, u = synthetic.render_randoms(H, W, 1024, 16, int(g["seed"]))
    with torch.no_grad():
        vol = m.MVSNet(gpu(g["vfw"]))
        rgb, feat, wts, dpred, alpha, _, rdepth, target = m(gpu(g["vfw"]), gpu(g["pseudo"]), batch, randoms=(gpu(pix), gpu(eps), gpu(u)))
    assert rel_err(vol.cpu()[:, :, ::8], g["volume"]) < 5e-5
    assert torch.equal(rdepth.cpu(), g["rays_depth"]) and rel_err(target.cpu(), g["target"]) < 1e-6
    interior = (pix[0] > 0) & (pix[0] < W - 1) & (pix[1] > 0) & (pix[1] < H - 1)
    other = [c for c in range(20) if c not in (11, 15, 19)]
    assert rel_err(feat.cpu()[::4][..., other], g["feat"][..., other]) < 2e-4
    for got, key in ((alpha, "alpha"), (wts, "weights"), (rgb, "rgb")):
        assert rel_err(got.cpu()[interior], g[key][interior]) < 5e-4, key
    assert float((dpred.cpu() - g["depth"]).abs()[interior].max()) / 500.0 < 5e-4
    with pytest.raises(NotImplementedError):
        b = _args(16)
        b.num_views = 3
        Rendering_Consistency_Net(b)


def test_render_forward_full_size_properties(hip):
    """BASELINE config-3 shape (V=4, 512x640, 1024 rays x 128 samples): runs, finite, invariants hold."""
    from rc_mvsnet_amd import synthetic
    m = _net(128)
    H, W, V = 512, 640, 4
    batch = {k: gpu(v) for k, v in synthetic.render_batch(V, H, W, 0).items()}
    gen = torch.Generator().manual_seed(0)
    vfw = gpu(0.5 * torch.randn(1, 41, 48, H // 4, W // 4, generator=gen))
    pseudo = gpu(500.0 + 300.0 * torch.rand(1, H, W, generator=gen))
    with torch.no_grad():
        rgb, feat, wts, dpred, alpha, _, rdepth, target = m(vfw, pseudo, batch)
    for t in (rgb, feat, wts, dpred, alpha):
        assert torch.isfinite(t).all()
    assert rgb.shape == (1024, 3) and feat.shape == (1024, 128, 20) and wts.shape == (1024, 128)
    assert float(wts.sum(1).max()) <= 1.0 + 1e-4
    assert float(alpha.min()) >= 0.0 and float(alpha.max()) <= 1.0
    assert float(rgb.min()) >= 0.0 and float(rgb.max()) <= 1.0 + 1e-4


# ------------------------------------------------------------------------------------------------
# backward kernels of the rendering tail, each against fp64 autograd of the operation it differentiates (same fp32 inputs)
# ------------------------------------------------------------------------------------------------
def _per_ray_err(got, ref, floor=None):
    """max over rays of max |got - ref| / (that ray's largest |ref|, at least `floor` (N,) and 1e-6: rays whose whole gradient is
    below 1e-6 with O(1) inputs and cotangents -- samples behind a saturated one, a lone saturated sample -- are measured against 1e-6)."""
    n = ref.shape[0]
    d = (got.double() - ref).abs().reshape(n, -1).max(1).values
    s = ref.abs().reshape(n, -1).max(1).values.clamp_min(1e-6)
    if floor is not None:
        s = torch.maximum(s, floor.double())
    return float((d / s).max())


def _composite_raw(N, S, regime, gen):
    raw = torch.rand(N, S, 4, generator=gen)
    if regime == "zero":                                   # alpha = 0 everywhere, T = 1
        raw[..., 3] = 0.0
    elif regime == "saturated":                            # alpha == 1.0f mid-ray: T drops to the 1e-10 floor (then 1e-20) behind it
        raw[..., 3] = 0.05 * torch.rand(N, S, generator=gen)
        raw[:, S // 2, 3] = 50.0
        if S > 3:
            raw[:, S // 2 + 1, 3] = 60.0
    else:                                                  # mixed: empty, soft and saturated samples on every ray
        raw[..., 3] = torch.relu(torch.randn(N, S, generator=gen)) * 0.5
        raw[..., 3] = torch.where(torch.rand(N, S, generator=gen) < 0.02, torch.full((N, S), 40.0), raw[..., 3])
    z = torch.sort(425 + 500 * torch.rand(N, S, generator=gen), dim=1).values
    return raw, z


def _composite_grads_fp64(raw, z, cot):
    """d/d raw of sum(out_k * cot_k) over the oracle's fp64 compositing; cot = (g_rgb, g_depth, g_w, g_alpha), entries may be None."""
    from oracle import render as orr
    r = raw.detach().double().requires_grad_(True)
    ref = orr.composite(r, z.double())
    loss = r.new_zeros(())
    for key, g in zip(("rgb_map", "depth_map", "weights", "alpha"), cot):
        if g is not None:
            loss = loss + (ref[key] * g.double()).sum()
    loss.backward()
    return r.grad


# fp32 recurrences over S samples (T products, the reverse Q sum): the error grows with S (measured ~1e-6 at S = 1000)
_COMPOSITE_TOL = 2e-5


@pytest.mark.parametrize("N,S", [(1, 1), (63, 2), (65, 64), (70, 128), (5, 200), (3, 1000)])
@pytest.mark.parametrize("regime", ["zero", "saturated", "mixed"])
def test_composite_backward_vs_fp64_autograd(hip, N, S, regime):
    """rcmvs_composite_bwd (one thread per ray, forward T pass + division-free reverse recurrence) through CompositeFn with all four
    cotangents, and called directly with ONE cotangent and null pointers for the other three (autograd always materialises zeros,
    so only a direct call reaches the null branches): against fp64 autograd of oracle.render.composite, per ray."""
    from rc_mvsnet_amd import _lib, train_ops
    gen = torch.Generator().manual_seed(N * 7 + S)
    raw, z = _composite_raw(N, S, regime, gen)
    cot = (torch.randn(N, 3, generator=gen), torch.randn(N, generator=gen) / 1000.0, torch.randn(N, S, generator=gen),
           torch.randn(N, S, generator=gen))
    # G_i - Q_i of the reverse recurrence cancels fp32 terms of size |g_depth| z (z = 425 ... 925) however close the samples are:
    # that size is the yardstick of a ray as well
    floor = cot[1].abs() * z.max(1).values
    ref = _composite_grads_fp64(raw, z, cot)
    rg = gpu(raw.clone()).requires_grad_(True)
    outs = train_ops.CompositeFn.apply(rg, gpu(z))
    sum((o * gpu(g)).sum() for o, g in zip(outs, cot)).backward()
    err = _per_ray_err(rg.grad.cpu(), ref, floor)
    assert err < _COMPOSITE_TOL, ("all four", err)
    for k in range(4):
        one = tuple(g if i == k else None for i, g in enumerate(cot))
        ref_k = _composite_grads_fp64(raw, z, one)
        r, zz = gpu(raw), gpu(z)
        gs = [None if g is None else gpu(g) for g in one]
        graw = torch.full_like(r, 7.0)                                  # every element must be written
        _lib.check(_lib.load().rcmvs_composite_bwd(train_ops._chk(r, "raw"), train_ops._chk(zz, "z"), *(train_ops._opt(g, "g") for g in gs),
                                                   train_ops._chk(graw, "grad_raw"), N, S, train_ops._stream()), "composite_bwd")
        err = _per_ray_err(graw.cpu(), ref_k, floor if k == 1 else None)
        assert err < _COMPOSITE_TOL, (("g_rgb", "g_depth", "g_w", "g_alpha")[k], err)


def _grid_sample_fp64(vol_cl, ndc, gfeat8=None):
    """trilinear grid_sample (zeros padding, align_corners=True) of the channels-last (Dv,hv,wv,8) volume at ndc*2-1 in fp64:
    -> (values (M,8), d/d volume (Dv,hv,wv,8) of sum(values * gfeat8))."""
    import torch.nn.functional as F
    v = vol_cl.detach().double().permute(3, 0, 1, 2).unsqueeze(0).requires_grad_(True)          # (1,8,Dv,hv,wv)
    grid = (ndc.double() * 2.0 - 1.0).reshape(1, 1, 1, -1, 3)                          # x -> wv, y -> hv, z -> Dv
    out = F.grid_sample(v, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, :, 0, 0].t()   # (M,8)
    if gfeat8 is None:
        return out.detach(), None
    (out * gfeat8.double()).sum().backward()
    return out.detach(), v.grad[0].permute(1, 2, 3, 0)


def _lattice_points(Dv, hv, wv, gen):
    """points exactly on lattice nodes (ndc = k/(n-1), the far faces at 1.0), on lattice edges (two coordinates on nodes) and faces."""
    node = lambda n: torch.arange(n, dtype=torch.float32) / max(n - 1, 1)
    gz, gy, gx = torch.meshgrid(node(Dv), node(hv), node(wv), indexing="ij")
    nodes = torch.stack((gx, gy, gz), -1).reshape(-1, 3)
    edges = nodes[torch.randint(0, nodes.shape[0], (300,), generator=gen)].clone()
    axis = torch.randint(0, 3, (300,), generator=gen)
    edges[torch.arange(300), axis] = torch.rand(300, generator=gen)
    face = torch.rand(200, 3, generator=gen)
    face[:100, 0] = 1.0
    face[100:, 2] = 1.0
    return torch.cat((nodes, edges, face, torch.ones(1, 3), torch.zeros(1, 3)))


@pytest.mark.parametrize("case", ["spread", "lattice", "Dv1", "hv1", "wv1", "collide"])
def test_point_feats_backward_vs_fp64_grid_sample(hip, case):
    """rcmvs_point_feats_bwd (trilinear scatter with hardware fp32 atomics) through PointFeatsFn, and its forward columns 0-7, against
    fp64 F.grid_sample: points inside and outside the volume, exactly on nodes / edges / far faces, degenerate one-voxel-thick volumes,
    M not a multiple of 256, and thousands of points colliding in a 2x2x2 volume.  Gradient columns >= 8 (image taps, masks, padding)
    carry large values that must not reach the volume."""
    from rc_mvsnet_amd import train_ops
    gen = torch.Generator().manual_seed(len(case))
    dims = {"spread": (7, 9, 13), "lattice": (5, 6, 7), "Dv1": (1, 9, 13), "hv1": (7, 1, 13), "wv1": (7, 9, 1), "collide": (2, 2, 2)}[case]
    Dv, hv, wv = dims
    if case == "lattice":
        ndc = _lattice_points(Dv, hv, wv, gen)
    elif case == "collide":
        ndc = torch.cat((torch.rand(5000, 3, generator=gen), -0.2 + 1.4 * torch.rand(123, 3, generator=gen)))
    else:
        ndc = -0.2 + 1.4 * torch.rand(1000, 3, generator=gen)
    M = ndc.shape[0]
    assert M % 256
    ldf = 16
    vol = torch.randn(Dv, hv, wv, 8, generator=gen)
    gfeat = torch.randn(M, ldf, generator=gen)
    gfeat[:, 8:] *= 1e3
    imgs = torch.rand(1, 3, 4, 5, generator=gen)
    poses = torch.cat((torch.eye(4).reshape(16), torch.eye(3).reshape(9))).reshape(1, 25)
    pts = torch.rand(M, 1, 3, generator=gen) + torch.tensor([0.0, 0.0, 1.0])
    want, gref = _grid_sample_fp64(vol, ndc, gfeat[:, :8])
    vg = gpu(vol.clone()).requires_grad_(True)
    feat = train_ops.PointFeatsFn.apply(vg, gpu(imgs), gpu(poses), gpu(pts), gpu(ndc.reshape(M, 1, 3)), ldf)
    (feat * gpu(gfeat)).sum().backward()
    got = vg.grad.cpu().double()
    # forward: fp32 coordinates move each trilinear weight by <= ~4 ulp x (n - 1) (n <= 13 voxels per axis): < 1e-5 of the values
    assert float((feat.detach().cpu()[:, :8].double() - want).abs().max()) < 1e-5 * float(want.abs().max())
    if case != "collide":
        assert float((got - gref).abs().max()) < 1e-5 * float(gref.abs().max())
    else:
        # every point of the unit cube adds to all 8 voxels: n = M fp32 additions per (voxel, channel), in whatever order the atomics
        # land.  Bound: (n + 3) u sum|g w| (summation + the products g * ((wx wy) wz)) + 4 u sum|g| (the fp32 coordinate moves each
        # weight by <= 4 u here, n - 1 = 1), u = 2^-24
        u = 2.0 ** -24
        _, gabs = _grid_sample_fp64(vol, ndc, gfeat[:, :8].abs())
        bound = (M + 3) * u * gabs + 4 * u * gfeat[:, :8].abs().double().sum(0)
        excess = float(((got - gref).abs() - bound).max())
        assert excess <= 0.0, excess


@pytest.mark.parametrize("C,Cp", [(41, 44), (60, 60)])
@pytest.mark.parametrize("D,Do", [(48, 128), (12, 128), (127, 128), (128, 127), (9, 9), (20, 7), (1, 9), (1, 1), (5, 1)])
def test_resize_planes_forward_backward_vs_fp64(hip, C, Cp, D, Do):
    """ResizePlanesFn: forward (rcmvs_resize_planes_fwd) and its exact adjoint (rcmvs_resize_planes_bwd: klo/khi window of the output
    planes that read input plane j) against fp64 F.interpolate(trilinear, align_corners=True, size=[Do,h,w]) and its autograd: batch
    2, h*w = 279 (above 256, not a multiple), padding columns of the cotangent nonzero (they must not leak).  Do = 1 is accepted and
    matches torch (align_corners with one output sample reads plane 0)."""
    import torch.nn.functional as F
    from rc_mvsnet_amd import train_ops
    gen = torch.Generator().manual_seed(D * 131 + Do + C)
    B, h, w = 2, 9, 31
    x = torch.randn(B, C, D, h, w, generator=gen)
    G = torch.randn(B, Do, h, w, Cp, generator=gen)
    xr = x.double().requires_grad_(True)
    ref = F.interpolate(xr, size=[Do, h, w], mode="trilinear", align_corners=True)
    (ref * G[..., :C].double().permute(0, 4, 1, 2, 3)).sum().backward()
    xg = gpu(x.clone()).requires_grad_(True)
    y = train_ops.ResizePlanesFn.apply(xg, Do, Cp)
    assert tuple(y.shape) == (B, Do, h, w, Cp)
    (y * gpu(G)).sum().backward()
    yc = y.detach().cpu()
    if Cp > C:
        assert float(yc[..., C:].abs().max()) == 0.0
    # the fp32 source coordinate scale * k is off by <= 2u (D - 1) (u = 2^-24), and so are the lerp weights: forward within
    # 4u D max|x|; an input plane gathers n <= 2 ceil((Do - 1) / (D - 1)) + 2 weighted cotangents (n = Do when D = 1), each weight
    # off by as much, plus n roundings of the sum: backward within n (2D + n) u max|G|
    u = 2.0 ** -24
    assert float((yc[..., :C].permute(0, 4, 1, 2, 3).double() - ref.detach()).abs().max()) <= 4 * u * D * float(x.abs().max())
    n = Do if D == 1 else 2 * -(-(Do - 1) // (D - 1)) + 2
    gx = xg.grad.cpu().double()
    assert float((gx - xr.grad).abs().max()) <= n * (2 * D + n) * u * float(G[..., :C].abs().max())


# ------------------------------------------------------------------------------------------------
# forward kernels on hostile inputs against plain fp64 references (tests/loss_render_cases.py)
# ------------------------------------------------------------------------------------------------
def _emu_slow(flag):
    if DEV == "cpu" and flag and os.environ.get("RCMVS_EMU_FULL", "0") != "1":
        pytest.skip("slow on the kernel emulation: RCMVS_EMU_FULL=1 (always run on the GPU)")


@pytest.mark.parametrize("N", LR.GU_N)
@pytest.mark.parametrize("S", LR.GU_S)
def test_gu_sampler_sizes_ties_and_zero_sigma(hip, S, N):
    """rcmvs_gu_sample_fwd at S = 2, 3, below / at / above the power-of-two padding (64, 65, 127, 129, 1000), S > GU_THREADS up to the
    4096 limit, two and six rays of a 5 x 7 image with the corners among the pixels, exact duplicates in eps, and (N = 6) one Gaussian
    ray whose pseudo depth equals `near`: sigma == 0.  Gaussian rays: non-decreasing, and the multiset of z is, bit for bit, that of
    mu + sigma * eps evaluated in fp32 in the kernel's operation order (it compiles with contraction off) -- nothing lost, duplicated
    or replaced by the +inf padding.  Uniform rays: within the existing z tolerance of the fp64 samples, inside their strata (one ulp
    of `far`, 2^-14, for the fp32 evaluation of lo + (hi - lo) u).  pts / ndc / dirs / rays_depth / target as in
    test_gu_sampler_vs_oracle, pts and ndc against the fp64 projection of the sampler's own z."""
    _emu_slow(S > 1000)
    c = LR.gu_case(N, S)
    r = LR.gu_reference(c)
    z, pts, ndc, dirs, rdepth, target = (t.cpu() for t in hip.gu_sample(gpu(c["pseudo"]), gpu(c["img0"]), gpu(c["pix"].to(torch.int32)),
                                                                        gpu(c["eps"]), gpu(c["u"]), gpu(c["cam"])))
    half = N // 2
    assert torch.equal(rdepth, r["rdepth"]) and torch.equal(target, r["target"])
    assert bool(torch.isfinite(z).all())
    assert bool((z[:half, 1:] >= z[:half, :-1]).all())
    assert torch.equal(torch.sort(z[:half], dim=1).values, torch.sort(r["gauss32"][:half], dim=1).values)
    if N >= 4:
        assert bool((z[1] == c["near"]).all())                                                   # sigma == 0
    assert float((z.double() - r["z64"]).abs().max()) < 2e-4
    zu = z[half:].double()
    assert bool((zu >= r["lo"] - 2.0 ** -14).all()) and bool((zu <= r["hi"] + 2.0 ** -14).all())
    want_pts, want_ndc = LR.gu_points(c, r, z)
    assert rel_err(dirs, r["dirs"]) < 1e-6
    assert rel_err(pts, want_pts) < 1e-6
    assert float((ndc.double() - want_ndc).abs().max()) < 2e-6


def test_gu_sampler_refusals(hip):
    from rc_mvsnet_amd import _lib
    c = LR.gu_case(2, 3)
    args = lambda N, S: (gpu(c["pseudo"]), gpu(c["img0"]), gpu(torch.zeros(2, N, dtype=torch.int32)), gpu(torch.zeros(N, S)),   # noqa: E731
                         gpu(torch.zeros(max(N // 2, 1), S)), gpu(c["cam"]))
    for N, S in ((3, 4), (2, 1), (2, 4097)):
        with pytest.raises(_lib.RcmvsError):
            hip.gu_sample(*args(N, S))


def _point_feats_raw(hip, vol, imgs, poses, pts, ndc, nimg, ldf, sentinel):
    """rcmvs_point_feats_fwd into a caller-owned, pre-filled feature matrix (ops.point_feats allocates its own)."""
    from rc_mvsnet_amd import _lib
    M = pts.shape[0]
    feat = torch.full((M, ldf), sentinel, device=DEV)
    Dv, hv, wv, _ = vol.shape
    H, W = imgs.shape[-2:]
    c = hip._chk
    vol, imgs, poses, pts, ndc = (gpu(t) for t in (vol, imgs, poses, pts, ndc))           # named: the pointers must outlive the call
    _lib.call("rcmvs_point_feats_fwd", c(vol, "volume"), c(imgs, "imgs"), c(poses, "poses"), c(pts, "pts"), c(ndc, "ndc"),
              c(feat, "feat"), M, Dv, hv, wv, nimg, H, W, ldf, hip._stream())
    return feat.cpu()


@pytest.mark.parametrize("case", ["spread", "lattice", "Dv1", "hv1", "wv1", "collide"])
def test_point_feats_forward_volume_vs_fp64_grid_sample(hip, case):
    """Columns 0-7 of rcmvs_point_feats_fwd on the volumes of test_point_feats_backward_vs_fp64_grid_sample (an axis of size 1, points
    on nodes / edges / far faces, M no multiple of 256) against fp64 F.grid_sample, no point excluded.  Bound: the fp32 coordinate
    moves each axis weight by <= 4 u (n - 1), the eight products wx wy wz by <= 2 (dx + dy + dz) in sum, plus the roundings of the
    products and of the eight additions: (24 (n - 1) + 16) u max|vol|, u = 2^-24, n the longest axis.  Rows far outside the volume
    on every axis (1e9, +-1e30; on an axis of size 1 every finite coordinate is node 0, as in grid_sample) and rows with a NaN or an
    infinite coordinate give exactly zero: zeros padding, and no tap of a NaN coordinate passes the bounds test."""
    gen = torch.Generator().manual_seed(len(case))
    Dv, hv, wv = {"spread": (7, 9, 13), "lattice": (5, 6, 7), "Dv1": (1, 9, 13), "hv1": (7, 1, 13), "wv1": (7, 9, 1), "collide": (2, 2, 2)}[case]
    if case == "lattice":
        ndc = _lattice_points(Dv, hv, wv, gen)
    else:
        ndc = -0.2 + 1.4 * torch.rand(1000 if case != "collide" else 5123, 3, generator=gen)
    wild = torch.tensor([[1e9, 1e9, 1e9], [-1e30, -1e30, -1e30], [1e30, -1e30, 1e9], [float("nan"), 0.5, 0.5], [0.5, 0.5, float("nan")],
                         [float("nan")] * 3, [0.5, float("inf"), 0.5]])
    M0 = ndc.shape[0]
    ndc = torch.cat((ndc, wild))
    M = ndc.shape[0]
    assert M % 256
    vol = torch.randn(Dv, hv, wv, 8, generator=gen)
    want, _ = _grid_sample_fp64(vol, ndc[:M0])
    imgs, poses, _ = LR.point_image_case(1)
    feat = _point_feats_raw(hip, vol, imgs, poses, torch.ones(M, 3), ndc, 0, 8, 7.0)
    assert float(feat[M0:].abs().max()) == 0.0
    u = 2.0 ** -24
    err = float((feat[:M0].double() - want).abs().max())
    bound = (24 * (max(Dv, hv, wv) - 1) + 16) * u * float(vol.abs().max())
    print(f"point feats volume {case}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("nimg", [0, 1, 3])
@pytest.mark.parametrize("M", [1, 255, 257])
def test_point_feats_forward_images_vs_fp64(hip, M, nimg):
    """The image columns of rcmvs_point_feats_fwd (LR.point_image_case: 5 x 9 images, an identity pose with dyadic K and two small
    rigid motions): points in front of every camera, behind them, with qz == 0 (+-inf, and NaN -> 0 as ATen's clip does) and
    projections exactly on g = +-1, where the strict mask is decidable in both precisions.  Masks exact (the generic rows are shown
    to keep |g| at least 1e-4 from 1), border-padded RGB at the existing 1e-5, ldf = 40 with every unused column left alone."""
    imgs, poses, pts = LR.point_image_case(M)
    rgb, mask, margin = LR.point_image_reference(imgs, poses, pts, nimg)
    assert bool(((margin == 0.0) | (margin > 1e-4)).all())
    vol = torch.randn(3, 4, 5, 8, generator=torch.Generator().manual_seed(1))
    ndc = torch.rand(M, 3, generator=torch.Generator().manual_seed(2))
    feat = _point_feats_raw(hip, vol, imgs, poses, pts, ndc, nimg, 40, -77.0)
    assert bool((feat[:, 8 + 4 * nimg:] == -77.0).all())
    assert bool(torch.isfinite(feat).all())
    want_vol, _ = _grid_sample_fp64(vol, ndc)
    assert float((feat[:, :8].double() - want_vol).abs().max()) < 1e-5 * float(want_vol.abs().max())
    for i in range(nimg):
        assert torch.equal(feat[:, 11 + 4 * i].double(), mask[:, i]), i
        assert rel_err(feat[:, 8 + 4 * i:11 + 4 * i], rgb[:, i]) < 1e-5, i
    if nimg and M > 1:
        assert 0.0 < float(mask.mean()) < 1.0


@pytest.mark.parametrize("N,S", [(1, 1), (63, 2), (65, 64), (70, 128), (5, 200), (3, 1000)])
@pytest.mark.parametrize("regime", ["zero", "saturated", "mixed"])
def test_composite_forward_regimes_vs_fp64(hip, N, S, regime):
    """rcmvs_composite_fwd in the regimes of its backward test (alpha == 0 everywhere; alpha == 1.0f mid-ray, T at the 1e-10 floor behind
    it; both mixed) and at its sizes: S < 64 (lanes that own no sample), S = 200, 1000 (no multiple of ceil(S / 64)).  Against the fp64
    oracle; the yardstick is the same composition with fp32 ATen ops on the CPU (exp, exclusive cumprod): the kernel's error may be
    twice the yardstick's plus one fp32 ulp of the value range (1 for alpha / weights / rgb, 1024 for the depth of z < 925).  Measured
    on the MI355X, worst case (saturated, S = 64 and 128): weights err 1.6e-7 against a yardstick of 1.0e-7 to 1.2e-7."""
    from oracle import render as orr
    gen = torch.Generator().manual_seed(N * 7 + S)
    raw, z = _composite_raw(N, S, regime, gen)
    ref = orr.composite(raw.double(), z.double())
    yard = orr.composite(raw, z)
    rgb, depth, weights, alpha = (t.cpu() for t in hip.composite(gpu(raw), gpu(z)))
    for name, got, key, ulp in (("alpha", alpha, "alpha", 2.0 ** -23), ("weights", weights, "weights", 2.0 ** -23), ("rgb", rgb, "rgb_map", 2.0 ** -23),
                                ("depth", depth, "depth_map", 2.0 ** -13)):
        assert bool(torch.isfinite(got).all()), name
        e_k = float((got.double() - ref[key]).abs().max())
        e_y = float((yard[key].double() - ref[key]).abs().max())
        print(f"composite {regime} N={N} S={S} {name}: kernel {e_k:.3e} yardstick {e_y:.3e}")
        assert e_k <= 2.0 * e_y + ulp, (name, e_k, e_y)
    assert float(weights.double().sum(1).max()) <= 1.0 + S * 2.0 ** -23
    if regime == "saturated":
        assert float(alpha[:, S // 2].min()) == 1.0
