"""Layer-output stores through buffer descriptors with a cache policy (csrc/common.h, out_store16).

Every converted entry point runs at the smallest shapes whose tiles are partial in every axis, with its output placed inside a NaN-filled
buffer: no NaN may be left inside, the guards on both sides stay untouched (the descriptor's span and the masked lanes' out-of-range
offsets are what keeps a store inside), and the values equal the comparator the parity tests use for that layer at that test's tolerance.
The entry points allocate their outputs with torch.empty / torch.empty_like: `guarded` swaps those for an allocator that carves every
float32 device tensor out of such a buffer, so the C ABI is handed a pointer into it.

Then two chains of the inference scene run back to back with no synchronisation between their launches and must equal, bit for bit, the
same chains with a device synchronisation after every launch; and the launchers refuse spans of 2^31 bytes before any launch."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 2048                      # floats on each side: 8 KiB, a multiple of 16 bytes


@pytest.fixture(scope="module")
def hip():
    from rc_mvsnet_amd import _lib, ops
    _lib.load()
    assert torch.cuda.is_available()
    return ops


def gpu(t):
    return t.to(DEV).contiguous()


@contextlib.contextmanager
def guarded():
    """Inside: every float32 tensor that torch.empty / torch.empty_like creates on the GPU lies between two NaN guards.  Yields the list of
    (whole buffer, view) pairs."""
    made = []
    real_empty, real_like = torch.empty, torch.empty_like

    def empty(*size, **kw):
        dev = torch.device(kw.get("device", "cpu"))
        if dev.type != "cuda" or kw.get("dtype", torch.float32) != torch.float32:
            return real_empty(*size, **kw)
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
        n = int(np.prod(shape)) if shape else 1
        whole = torch.full((n + 2 * GUARD,), float("nan"), device=dev, dtype=torch.float32)
        view = whole[GUARD:GUARD + n].view(shape)
        made.append((whole, view))
        return view

    def empty_like(t, **kw):
        return empty(tuple(t.shape), device=t.device, dtype=kw.get("dtype", t.dtype))

    torch.empty, torch.empty_like = empty, empty_like
    try:
        yield made
    finally:
        torch.empty, torch.empty_like = real_empty, real_like


def contained(made, out):
    """`out` is one of the guarded tensors: fully written, and nothing written outside it."""
    torch.cuda.synchronize()
    hits = [(w, v) for w, v in made if v.data_ptr() == out.data_ptr() and v.numel() == out.numel()]
    assert len(hits) == 1, "the entry point's output was not allocated through torch.empty"
    whole, view = hits[0]
    assert not bool(torch.isnan(view).any()), "output elements left unwritten"
    assert bool(torch.isnan(whole[:GUARD]).all()) and bool(torch.isnan(whole[GUARD + view.numel():]).all()), "a store outside the output"
    for w, v in made:             # (no other buffer of the call was overrun either)
        assert bool(torch.isnan(w[:GUARD]).all()) and bool(torch.isnan(w[GUARD + v.numel():]).all())


# ------------------------------------------------------------------------------------------ 3-D convolutions
# every kernel family of the cost regularisation: z-marching (conv3d_z8), stride 2 (conv3d_zs2), split (conv3d_x3: transposed 16 -> 8), deep tiles (conv3d_deep)
@pytest.mark.parametrize("Ci,Co,kind", [(8, 8, "s1"), (16, 8, "s1"), (32, 8, "s1"), (16, 16, "s1"), (32, 32, "s1"), (64, 64, "s1"),
                                        (8, 16, "s2"), (16, 32, "s2"), (32, 64, "s2"), (16, 8, "t2"), (32, 16, "t2"), (64, 32, "t2")])
@pytest.mark.parametrize("pair", [True, False])
def test_conv3d_outputs_stay_inside(hip, Ci, Co, kind, pair):
    """Batch 2 (the deep kernels' per-batch descriptor base), residual + ReLU epilogue; pair: the fp16-pair form the scene runs, else the exact
    three-piece form (conv3d_x3's epilogues).  Comparator and tolerance of test_conv3d_x3h_vs_fp64: fp64, next to the fp32 FMA-chain kernels."""
    B, (D, H, W) = 2, ((5, 11, 37) if kind == "s2" else (3, 9, 35))
    g = torch.Generator().manual_seed(Ci * 7 + Co)
    x = torch.randn(B, Ci, D, H, W, generator=g) * torch.exp(torch.randn(B, Ci, D, H, W, generator=g))
    scale, shift = 0.5 + torch.rand(Co, generator=g), 0.1 * torch.randn(Co, generator=g)
    if kind == "t2":
        w = torch.randn(Ci, Co, 3, 3, 3, generator=g) / (Ci * 27 / 8) ** 0.5
        ref = torch.nn.functional.conv_transpose3d(x.double(), w.double(), padding=1, stride=2, output_padding=1)
        wp = hip.pack_conv3d_weight(gpu(w), transposed=True)
        run = lambda *a, **k: hip.deconv3d(*a, **k)
    else:
        st = 2 if kind == "s2" else 1
        w = torch.randn(Co, Ci, 3, 3, 3, generator=g) / (Ci * 27) ** 0.5
        ref = torch.nn.functional.conv3d(x.double(), w.double(), padding=1, stride=st)
        wp = hip.pack_conv3d_weight(gpu(w))
        run = lambda *a, **k: hip.conv3d(*a, stride=st, **k)
    res = torch.randn(ref.shape, generator=g)
    mag = float(ref.abs().max())
    ref = torch.relu(ref * scale.double().view(1, -1, 1, 1, 1) + shift.double().view(1, -1, 1, 1, 1)) + res.double()
    xcl, rcl = gpu(x.permute(0, 2, 3, 4, 1)), gpu(res.permute(0, 2, 3, 4, 1))
    kw = {"x_absmax": hip.absmax(xcl)} if pair else {}
    with guarded() as made:
        y = run(xcl, wp, gpu(scale), gpu(shift), rcl, relu=True, **kw)
        contained(made, y)
    try:
        hip.force_direct_conv(64)
        y32 = run(xcl, wp, gpu(scale), gpu(shift), rcl, relu=True)
    finally:
        hip.force_direct_conv(0)
    back = lambda t: t.cpu().permute(0, 4, 1, 2, 3).double()
    e, e32 = float((back(y) - ref).abs().max()), float((back(y32) - ref).abs().max())
    print(f"conv3d {Ci}->{Co} {kind} pair={pair}: max error vs fp64 / max {e / mag:.2e} (fp32 FMA chain {e32 / mag:.2e})")
    assert e <= 2.0 * e32 + 1e-7 * mag and e < 3e-6 * mag, (e, e32, mag)


# ------------------------------------------------------------------------------------------ 2-D maps: 3 views of 13 x 35
N2, H2, W2 = 3, 13, 35


def _bn(c, g):
    return 0.5 + torch.rand(c, generator=g), 0.2 * torch.randn(c, generator=g)


def test_conv2d_stem_output_stays_inside(hip):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N2, 3, H2, W2, generator=g)
    wa, wb = torch.randn(8, 3, 3, 3, generator=g) / 5.0, torch.randn(8, 8, 3, 3, generator=g) / 8.0
    (sa, ha), (sb, hb) = _bn(8, g), _bn(8, g)
    f = torch.nn.functional
    mid = torch.relu(f.conv2d(x.double(), wa.double(), padding=1) * sa.double().view(1, -1, 1, 1) + ha.double().view(1, -1, 1, 1))
    ref = torch.relu(f.conv2d(mid, wb.double(), padding=1) * sb.double().view(1, -1, 1, 1) + hb.double().view(1, -1, 1, 1))
    pa, img = hip.pack_conv2d_weight(gpu(wa), pad_in_to=4), hip.pack_conv2d_stem(gpu(wb))
    with guarded() as made:
        y = hip.conv2d_stem(gpu(x), pa, gpu(sa), gpu(ha), img, gpu(sb), gpu(hb))
        contained(made, y)
    assert float((y.cpu().permute(0, 3, 1, 2).double() - ref).abs().max()) < 2e-6 * float(ref.abs().max())      # (test_conv2d_stem_vs_fp64)


def test_conv2d_pair_output_stays_inside(hip):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(N2, 16, H2, W2, generator=g)
    wa, wb = (torch.randn(16, 16, 3, 3, generator=g) / 12.0 for _ in range(2))
    (sa, ha), (sb, hb) = _bn(16, g), _bn(16, g)
    f = torch.nn.functional
    mid = torch.relu(f.conv2d(x.double(), wa.double(), padding=1) * sa.double().view(1, -1, 1, 1) + ha.double().view(1, -1, 1, 1))
    ref = torch.relu(f.conv2d(mid, wb.double(), padding=1) * sb.double().view(1, -1, 1, 1) + hb.double().view(1, -1, 1, 1))
    img = hip.pack_conv2d_pair(gpu(wa), gpu(wb))
    with guarded() as made:
        y = hip.conv2d_pair(gpu(x.permute(0, 2, 3, 1)), img, gpu(sa), gpu(ha), gpu(sb), gpu(hb))
        contained(made, y)
    assert float((y.cpu().permute(0, 3, 1, 2).double() - ref).abs().max()) < 2e-6 * float(ref.abs().max())      # (test_conv2d_pair_vs_fp64)


@pytest.mark.parametrize("form", ["16", "s2d", "32"])
def test_conv2d_tile_output_stays_inside(hip, form):
    from rc_mvsnet_amd.casmvsnet import FeatureNet
    g = torch.Generator().manual_seed(3)
    f = torch.nn.functional
    if form == "s2d":
        x = torch.randn(N2, 8, 2 * H2, 2 * W2, generator=g)
        w5 = torch.randn(16, 8, 5, 5, generator=g) / (8 * 25) ** 0.5
        sc, sh = _bn(16, g)
        ref = torch.relu(f.conv2d(x.double(), w5.double(), stride=2, padding=2) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1))
        args, kw = (hip.pack_conv2d_tile(gpu(FeatureNet._w5s2(w5))), gpu(sc), gpu(sh)), {"relu": True, "s2d": True}
    else:
        co = int(form)
        x = torch.randn(N2, 32, H2, W2, generator=g)
        w = torch.randn(co, 32, 3, 3, generator=g) / (32 * 9) ** 0.5
        sc, sh = _bn(co, g)
        ref = torch.relu(f.conv2d(x.double(), w.double(), padding=1) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1))
        args, kw = (hip.pack_conv2d_tile(gpu(w)), gpu(sc), gpu(sh)), {"relu": True}
    xcl = gpu(x.permute(0, 2, 3, 1))
    with guarded() as made:
        y = hip.conv2d_tile(xcl, *args, **kw)
        contained(made, y)
    assert float((y.cpu().permute(0, 3, 1, 2).double() - ref).abs().max()) < 2e-6 * float(ref.abs().max())      # (test_conv2d_tile_vs_fp64)


@pytest.mark.parametrize("Ci,Co,K,stride", [(8, 8, 3, 1), (8, 16, 5, 2), (16, 16, 3, 1), (32, 8, 3, 1)])
def test_conv2d_output_stays_inside(hip, Ci, Co, K, stride):
    """The planar tile kernel (conv2d_lds_kernel), one pixel and two pixels per thread; comparator of test_conv2d_vs_torch_cpu."""
    from conftest import rel_err
    g = torch.Generator().manual_seed(Ci + Co)
    x = torch.randn(N2, Ci, H2, W2, generator=g)
    w = torch.randn(Co, Ci, K, K, generator=g) / (Ci * K * K) ** 0.5
    sc, sh = _bn(Co, g)
    ref = torch.relu(torch.nn.functional.conv2d(x, w, None, stride, K // 2) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    wp = hip.pack_conv2d_weight(gpu(w))
    with guarded() as made:
        y = hip.conv2d(gpu(x.permute(0, 2, 3, 1)), wp, gpu(sc), gpu(sh), stride=stride, relu=True)
        contained(made, y)
    assert rel_err(y.cpu().permute(0, 3, 1, 2), ref) < 2e-5


# the 1x1 kernels.  The up-add merge needs even maps: 14 x 34 there (still a partial last block and a partial last n-tile: 3 * 14 * 34 = 1428
# pixels = 5 blocks of 256 + 148 = 89 n-tiles of 16 + 4).  209 x 210: 131 670 pixels, the first size on the LDS-transposed store path
# (>= 131 072 pixels), its last block partial.
@pytest.mark.parametrize("Ci,H,W,up,mfma", [(16, 13, 35, False, False), (16, 14, 34, True, False), (32, 13, 35, False, True), (16, 14, 34, True, True),
                                            (8, 13, 35, False, False), (16, 209, 210, False, False)])
def test_conv1x1_output_stays_inside(hip, Ci, H, W, up, mfma):
    g = torch.Generator().manual_seed(Ci + H)
    x = torch.randn(N2, H, W, Ci, generator=g)
    w = torch.randn(32, Ci, 1, 1, generator=g) / Ci ** 0.5
    sc, sh = 0.5 + torch.rand(32, generator=g), 0.1 * torch.randn(32, generator=g)
    ua = torch.randn(N2, H // 2, W // 2, 32, generator=g) if up else None
    want = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), w.double()).permute(0, 2, 3, 1) * sc.double() + sh.double()
    if up:
        want = want + ua.double().repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    want = want.clamp_min(0)
    wp = hip.pack_conv2d_weight(gpu(w))
    with guarded() as made:
        y = hip.conv1x1(gpu(x), wp, gpu(sc), gpu(sh), up_add=gpu(ua) if up else None, relu=True, mfma=mfma)
        contained(made, y)
    assert float((y.cpu().double() - want).abs().max()) < 3e-6 * float(want.abs().max())         # (test_conv1x1_matrix_core_form)


def test_fpn_out_folded_output_stays_inside(hip):
    """The folded last FPN level on the matrix cores needs even maps: 14 x 34 (partial tiles in both axes); comparator of
    test_fpn_out_folded_matches_the_unfused_path."""
    H, W = 14, 34
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(N2, H, W, 8, generator=g)
    up = torch.randn(N2, H // 2, W // 2, 32, generator=g)
    w_in, b_in = 0.3 * torch.randn(32, 8, 1, 1, generator=g), 0.5 * torch.randn(32, generator=g)
    w_out = 0.1 * torch.randn(8, 32, 3, 3, generator=g)
    F = torch.nn.functional
    intra = F.interpolate(up.permute(0, 3, 1, 2).double(), scale_factor=2, mode="nearest") + F.conv2d(lat.permute(0, 3, 1, 2).double(), w_in.double(), b_in.double())
    want = F.conv2d(intra, w_out.double(), padding=1).permute(0, 2, 3, 1)
    img = hip.pack_fpn_folded_mfma(hip.pack_fpn_folded(gpu(w_in), gpu(b_in), gpu(w_out)))
    with guarded() as made:
        y = hip.fpn_out_folded(gpu(lat), gpu(up), img)
        contained(made, y)
    assert float((y.cpu().double() - want).abs().max()) < 2e-6 * float(want.abs().max())


@pytest.mark.parametrize("shape", [(3, 8, 13, 35), (2, 32, 3, 9, 35), (1, 64, 5, 7)])
def test_layout_output_stays_inside(hip, shape):
    x = torch.randn(*shape)
    with guarded() as made:
        cl = hip.to_channels_last(gpu(x))
        contained(made, cl)
    assert torch.equal(cl.cpu(), x.permute(0, *range(2, len(shape)), 1).contiguous())


# ------------------------------------------------------------------------------------------ K1
# 3 views at 9 x 35, D = 5, B = 2 (per-batch and per-plane descriptor bases; D = 5: the last plane chunk is partial).  C = 8 per-pixel planes: the
# plane-pipelined form; uniform planes: the window form; C = 16 / 32 per-pixel planes: the two-phase kernel; V = 4, variant 0: its run-time-view form.
@pytest.mark.parametrize("V,C,uniform,variant", [(3, 8, False, None), (3, 32, True, None), (3, 16, True, None), (3, 16, False, None), (3, 32, False, None),
                                                 (4, 8, False, 0), (4, 8, False, None)])
def test_warp_variance_output_stays_inside(hip, V, C, uniform, variant):
    from oracle import warp
    from test_gpu_parity import _k1_case
    B, D, h, w = 2, 5, 9, 35
    feats, pm, planes = _k1_case(B, V, C, D, h, w, 3)
    if uniform:
        planes = planes[:, :1, :1].expand(B, h, w, 2).contiguous()
    k = torch.arange(D, dtype=torch.float32).reshape(1, D, 1, 1)
    samples = planes[..., 0].unsqueeze(1) + k * planes[..., 1].unsqueeze(1)
    rots, transs = zip(*[warp.compose_homography(pm[:, v], pm[:, 0]) for v in range(1, V)])
    rot, trans = torch.stack([r.reshape(B, 9) for r in rots], dim=1), torch.stack(transs, dim=1)
    ref = warp.variance_volume(feats, pm, samples)
    f_cl = gpu(torch.stack([f.permute(0, 2, 3, 1) for f in feats], dim=1))
    with guarded() as made:
        var = hip.warp_variance(f_cl, gpu(rot), gpu(trans), gpu(planes), D, uniform_planes=uniform, variant=variant)
        contained(made, var)
    diff = (var.cpu().permute(0, 4, 1, 2, 3) - ref).abs()
    assert float(diff.max()) < 1e-5 * max(1.0, float(ref.abs().max()))          # (test_warp_variance_vs_oracle)


# ------------------------------------------------------------------------------------------ back-to-back launches
def _chains():
    from rc_mvsnet_amd import ops, synthetic
    from rc_mvsnet_amd.casmvsnet import CostRegNet, FeatureNet
    reg = CostRegNet(8, 8)
    reg.load_state_dict({k[3:]: v for k, v in synthetic.cost_reg_state_dict(np.random.RandomState(3), "cr", 8).items()}, strict=True)
    reg = reg.to(DEV).eval()
    fnet = FeatureNet(base_channels=8, num_stage=3, arch_mode="fpn")
    fnet.load_state_dict({k[len("feature."):]: v for k, v in synthetic.cascade_state_dict(0).items() if k.startswith("feature.")}, strict=True)
    fnet = fnet.to(DEV).eval()
    g = torch.Generator().manual_seed(11)
    vol = gpu(torch.randn(1, 8, 32, 40, 8, generator=g).abs())
    planes = gpu(torch.stack((400.0 + 50.0 * torch.rand(1, 32, 40, generator=g), 2.0 + torch.rand(1, 32, 40, generator=g)), dim=-1))
    imgs = gpu(synthetic.images(1, 3, 64, 96, 0)[0])

    def regularise():
        bounds = torch.zeros(reg.BOUND_ROWS, ops.ABSMAX_FLOATS, device=DEV)
        ops.absmax(vol, out=bounds[0])
        depth, conf = reg.features_cl(vol, x_absmax=bounds, logits=True, planes=planes)
        return [depth.clone(), conf.clone()]                       # the ATen copy right behind the last launch

    def features():
        out = fnet.forward_cl(imgs)
        return [out[k].clone() for k in sorted(out)]

    return regularise, features


@pytest.mark.parametrize("which", [0, 1], ids=["costreg+head", "featurenet"])
def test_back_to_back_launches_see_their_predecessors_outputs(hip, monkeypatch, which):
    """Write-through stores drop their lines from L2; what makes a layer's output visible to the next launch is still the kernel boundary.  20
    rounds with nothing between the launches but the stream's order, each result copied by ATen at once, against the same chain with a device
    synchronisation after every launch."""
    from rc_mvsnet_amd import _lib
    chain = _chains()[which]
    with torch.no_grad():
        chain()                                                        # (weights packed, LDS limits raised)
        torch.cuda.synchronize()
        fast = [chain() for _ in range(20)]
        torch.cuda.synchronize()
        real_call = _lib.call

        def synced(name, *args):
            real_call(name, *args)
            torch.cuda.synchronize()

        monkeypatch.setattr(_lib, "call", synced)
        want = chain()
        torch.cuda.synchronize()
    for r, got in enumerate(fast):
        for a, b in zip(got, want):
            assert torch.equal(a, b), f"round {r}: differs from the synchronised chain"
    assert all(bool(torch.isfinite(t).all()) for t in want)


# ------------------------------------------------------------------------------------------ descriptor limit
def test_launchers_refuse_spans_of_2_to_the_31_bytes(hip):
    """Host side only: sizes whose output span reaches 2^31 bytes are refused before any launch (the pointers are never dereferenced: a few floats
    stand in for tensors that are not allocated)."""
    from rc_mvsnet_amd import _lib
    lib = _lib.load()
    t = torch.zeros(64, device=DEV)
    p, null, st = ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(None), ctypes.c_void_p(None)
    torch.cuda.synchronize()

    def refused(rc):
        assert rc != 0 and b"32-bit" in lib.rcmvs_last_error_string()

    # conv2d (planar tile kernel): one image's 16384 x 16384 x 8-channel map = 2^33 bytes
    refused(lib.rcmvs_conv2d_fwd(p, p, null, null, null, p, 1, 16384, 16384, 8, 8, 3, 1, 0, st))
    # fused stem / pair / tile kernels: one view's map
    refused(lib.rcmvs_conv2d_stem_fwd(p, p, p, p, p, p, p, p, 1, 16384, 16384, st))
    refused(lib.rcmvs_conv2d_pair_fwd(p, p, p, p, p, p, p, 1, 8192, 8192, 16, st))
    # the folded FPN level: all maps of the call in one span
    refused(lib.rcmvs_fpn_out_folded_mfma(p, p, p, p, null, 4, 8192, 8192, st))
    # K1: a view block of 3 x 8192 x 8192 x 8 floats; its plane spans (one per (batch element, plane)) are smaller than that
    refused(lib.rcmvs_warp_variance_hint_fwd(p, p, p, p, p, 1, 3, 8, 4, 8192, 8192, 0, st))
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0
