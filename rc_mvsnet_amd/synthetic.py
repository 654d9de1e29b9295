"""Seeded synthetic DTU-shaped inputs and non-degenerate weights (no dataset / checkpoint
is reachable here).  Shapes, camera model and depth range follow SURVEY.md section 8d:

  K(1/4 res) = [[361.54125*W/640, 0, 82.900625*W/640], [0, 360.3975*H/512, 66.383875*H/512], [0,0,1]]
  view v: rotation about y by 0.08*v rad, centre C = (60v, 10v, 0) mm, E = [R | -R C]
  proj[:, v, 0] = E, proj[:, v, 1, :3, :3] = K (x1, x2, x4 for stages 1..3, as
  datasets/dtu_test.py:215-224 builds them);  depth_values = 425 + 2.65*arange(192).

Everything is generated on the CPU with fixed seeds so that the golden generator, the
oracle, the tests and bench.py all see bit-identical tensors.
"""
import math

import numpy as np
import torch

NUM_DEPTH_VALUES = 192


def cameras(V, H, W):
    """Returns K_quarter (3,3) float64 and a list of V extrinsics (4,4) float64."""
    K = np.array([[361.54125 * W / 640.0, 0.0, 82.900625 * W / 640.0],
                  [0.0, 360.3975 * H / 512.0, 66.383875 * H / 512.0],
                  [0.0, 0.0, 1.0]])
    Es = []
    for v in range(V):
        a = 0.08 * v
        R = np.array([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
        C = np.array([60.0 * v, 10.0 * v, 0.0])
        E = np.eye(4)
        E[:3, :3] = R
        E[:3, 3] = -R @ C
        Es.append(E)
    return K, Es


def proj_matrices(B, V, H, W):
    """{'stage1','stage2','stage3'}: (B,V,2,4,4) float32."""
    K, Es = cameras(V, H, W)
    out = {}
    for s, mul in (("stage1", 1.0), ("stage2", 2.0), ("stage3", 4.0)):
        p = np.zeros((V, 2, 4, 4), dtype=np.float32)
        for v in range(V):
            p[v, 0] = Es[v]
            Ks = K.copy()
            Ks[:2] *= mul
            p[v, 1, :3, :3] = Ks
        out[s] = torch.from_numpy(np.broadcast_to(p, (B, V, 2, 4, 4)).copy())
    return out


def depth_values(B):
    return (425.0 + 2.65 * torch.arange(NUM_DEPTH_VALUES, dtype=torch.float32)).reshape(1, -1).repeat(B, 1)


def images(B, V, H, W, seed=0):
    """Smooth-ish seeded images, roughly ImageNet-normalised range: (B,V,3,H,W) float32."""
    g = torch.Generator().manual_seed(seed)
    out = torch.zeros(B * V, 3, H, W)
    for div, amp in ((16, 1.0), (4, 0.5), (1, 0.25)):
        n = torch.randn(B * V, 3, max(H // div, 1), max(W // div, 1), generator=g)
        out += amp * torch.nn.functional.interpolate(n, size=(H, W), mode="bilinear", align_corners=False)
    return out.reshape(B, V, 3, H, W).contiguous()


def cascade_inputs(B=1, V=3, H=512, W=640, seed=0):
    """(imgs, proj_matrices, depth_values) of CascadeMVSNet[_eval].forward."""
    return images(B, V, H, W, seed), proj_matrices(B, V, H, W), depth_values(B)


# ----------------------------------------------------------------------------------------
# weights with the reference's state_dict names
# ----------------------------------------------------------------------------------------
def _bn(sd, rng, name, c):
    sd[name + ".weight"] = torch.from_numpy(rng.uniform(0.5, 1.5, c).astype(np.float32))
    sd[name + ".bias"] = torch.from_numpy((0.1 * rng.standard_normal(c)).astype(np.float32))
    sd[name + ".running_mean"] = torch.from_numpy((0.1 * rng.standard_normal(c)).astype(np.float32))
    sd[name + ".running_var"] = torch.from_numpy(rng.uniform(0.5, 1.5, c).astype(np.float32))
    sd[name + ".num_batches_tracked"] = torch.tensor(0, dtype=torch.long)


def _w(rng, shape, fan_in, gain=1.0):
    bound = gain * math.sqrt(3.0 / fan_in)
    return torch.from_numpy(rng.uniform(-bound, bound, shape).astype(np.float32))


def cost_reg_specs(cin, base=8):
    """(name, kind, cin, cout) of CostRegNet (models/modules.py:470-489)."""
    b = base
    return [("conv0", "conv", cin, b), ("conv1", "conv", b, 2 * b), ("conv2", "conv", 2 * b, 2 * b),
            ("conv3", "conv", 2 * b, 4 * b), ("conv4", "conv", 4 * b, 4 * b), ("conv5", "conv", 4 * b, 8 * b),
            ("conv6", "conv", 8 * b, 8 * b), ("conv7", "deconv", 8 * b, 4 * b), ("conv9", "deconv", 4 * b, 2 * b),
            ("conv11", "deconv", 2 * b, b)]


def cascade_state_dict(seed=0, feat_channels=(32, 16, 8), prob_gain=20.0):
    """238 tensors named like CascadeMVSNet[_eval].state_dict() (fpn, 3 stages, cr base 8).
    BN statistics are randomised and prob.weight is scaled so that the probability volume
    is peaked instead of flat."""
    rng = np.random.RandomState(seed)
    sd = {}
    b = 8
    for name, ci, co, k in (("conv0.0", 3, b, 3), ("conv0.1", b, b, 3), ("conv1.0", b, 2 * b, 5), ("conv1.1", 2 * b, 2 * b, 3),
                            ("conv1.2", 2 * b, 2 * b, 3), ("conv2.0", 2 * b, 4 * b, 5), ("conv2.1", 4 * b, 4 * b, 3),
                            ("conv2.2", 4 * b, 4 * b, 3)):
        sd[f"feature.{name}.conv.weight"] = _w(rng, (co, ci, k, k), ci * k * k, math.sqrt(2.0))
        _bn(sd, rng, f"feature.{name}.bn", co)
    sd["feature.out1.weight"] = _w(rng, (4 * b, 4 * b, 1, 1), 4 * b)
    sd["feature.inner1.weight"] = _w(rng, (4 * b, 2 * b, 1, 1), 2 * b)
    sd["feature.inner1.bias"] = torch.from_numpy((0.1 * rng.standard_normal(4 * b)).astype(np.float32))
    sd["feature.inner2.weight"] = _w(rng, (4 * b, b, 1, 1), b)
    sd["feature.inner2.bias"] = torch.from_numpy((0.1 * rng.standard_normal(4 * b)).astype(np.float32))
    sd["feature.out2.weight"] = _w(rng, (2 * b, 4 * b, 3, 3), 4 * b * 9)
    sd["feature.out3.weight"] = _w(rng, (b, 4 * b, 3, 3), 4 * b * 9)
    for s, cin in enumerate(feat_channels):
        sd.update(cost_reg_state_dict(rng, f"cost_regularization.{s}", cin, prob_gain=prob_gain))
    return sd


def feature_unet_state_dict(seed=0, base=8, num_stage=3):
    """State dict of FeatureNet(base, num_stage, arch_mode='unet') (models/modules.py:363-401): the trunk of the 'fpn' form, the
    DeConv2dFuse merges and the 1x1 output convs; BN statistics randomised."""
    rng = np.random.RandomState(seed)
    sd, b = {}, base
    for name, ci, co, k in (("conv0.0", 3, b, 3), ("conv0.1", b, b, 3), ("conv1.0", b, 2 * b, 5), ("conv1.1", 2 * b, 2 * b, 3),
                            ("conv1.2", 2 * b, 2 * b, 3), ("conv2.0", 2 * b, 4 * b, 5), ("conv2.1", 4 * b, 4 * b, 3),
                            ("conv2.2", 4 * b, 4 * b, 3)):
        sd[f"{name}.conv.weight"] = _w(rng, (co, ci, k, k), ci * k * k, math.sqrt(2.0))
        _bn(sd, rng, f"{name}.bn", co)
    sd["out1.weight"] = _w(rng, (4 * b, 4 * b, 1, 1), 4 * b)
    for n, (name, ci, co) in enumerate((("deconv1", 4 * b, 2 * b), ("deconv2", 2 * b, b))[:num_stage - 1]):
        sd[f"{name}.deconv.conv.weight"] = _w(rng, (ci, co, 3, 3), ci * 9 / 4, math.sqrt(2.0))        # ConvTranspose2d: (in, out, k, k)
        _bn(sd, rng, f"{name}.deconv.bn", co)
        sd[f"{name}.conv.conv.weight"] = _w(rng, (co, 2 * co, 3, 3), 2 * co * 9, math.sqrt(2.0))
        _bn(sd, rng, f"{name}.conv.bn", co)
        sd[f"out{n + 2}.weight"] = _w(rng, (co, co, 1, 1), co)
    return sd


def cascade_unet_state_dict(seed=0, prob_gain=1.0):
    """State dict of CascadeMVSNet[_eval](arch_mode='unet') (3 stages, cr base 8): the 'unet' pyramid + the cost regularisations of
    cascade_state_dict (a smooth probability head by default)."""
    sd = {"feature." + k: v for k, v in feature_unet_state_dict(seed).items()}
    sd.update({k: v for k, v in cascade_state_dict(seed, prob_gain=prob_gain).items() if k.startswith("cost_regularization.")})
    return sd


def cost_reg_state_dict(rng, prefix, cin, base=8, prob_gain=20.0):
    sd = {}
    for name, kind, ci, co in cost_reg_specs(cin, base):
        shape = (co, ci, 3, 3, 3) if kind == "conv" else (ci, co, 3, 3, 3)
        sd[f"{prefix}.{name}.conv.weight"] = _w(rng, shape, ci * 27, math.sqrt(2.0))
        _bn(sd, rng, f"{prefix}.{name}.bn", co)
    sd[f"{prefix}.prob.weight"] = _w(rng, (1, base, 3, 3, 3), base * 27, prob_gain)
    return sd


def render_state_dict(seed=1, n_src=3, vol_src=None):
    """82 tensors named like Rendering_Consistency_Net.state_dict() (netdepth 6, width 128).  vol_src: source views behind the warped
    volume feature the volume network reads (32 + 3 vol_src input channels; default n_src = the reference's 3; 4 = the five-view
    extension of Neural_Volume_Net, models/render_models.py:750)."""
    rng = np.random.RandomState(seed)
    sd = {}
    p = "MVSNet.cost_reg_2"
    for name, kind, ci, co in cost_reg_specs(32 + 3 * (n_src if vol_src is None else vol_src), 8):
        if kind == "conv":
            sd[f"{p}.{name}.conv.weight"] = _w(rng, (co, ci, 3, 3, 3), ci * 27)
            _bn(sd, rng, f"{p}.{name}.bn", co)
        else:
            sd[f"{p}.{name}.0.weight"] = _w(rng, (ci, co, 3, 3, 3), ci * 27 / 8.0)
            _bn(sd, rng, f"{p}.{name}.1", co)
    q = "network_fn.nerf"

    def lin(name, ci, co, gain=math.sqrt(2.0)):
        sd[f"{q}.{name}.weight"] = _w(rng, (co, ci), ci, gain)
        sd[f"{q}.{name}.bias"] = torch.from_numpy((0.05 * rng.standard_normal(co)).astype(np.float32))
    lin("pts_linears.0", 63, 128)
    for i in range(1, 5):
        lin(f"pts_linears.{i}", 128, 128)
    lin("pts_linears.5", 191, 128)
    lin("pts_bias", 8 + 4 * n_src, 128, 1.0)
    lin("views_linears.0", 131, 64)
    lin("feature_linear", 128, 128, 1.0)
    lin("alpha_linear", 128, 1, 1.0)
    lin("rgb_linear", 64, 3, 1.0)
    # pts_bias centred on 1 so that the multiplicative bias does not kill the trunk
    sd[f"{q}.pts_bias.bias"] = sd[f"{q}.pts_bias.bias"] + 1.0
    return sd


# ----------------------------------------------------------------------------------------
# rendering-branch batch (keys of datasets/dtu_train.py:344-364 that the renderer reads)
# ----------------------------------------------------------------------------------------
def render_batch(V, H, W, seed=0):
    K, Es = cameras(V, H, W)
    Kfull = K.copy()
    Kfull[:2] *= 4.0
    w2cs = np.stack(Es).astype(np.float32)
    c2ws = np.stack([np.linalg.inv(E) for E in Es]).astype(np.float32)
    intr = np.stack([Kfull] * V).astype(np.float32)
    nf = np.stack([np.array([425.0, 425.0 + 2.65 * 191], dtype=np.float32)] * V)
    return {"imgs": images(1, V, H, W, seed), "w2cs": torch.from_numpy(w2cs)[None], "c2ws": torch.from_numpy(c2ws)[None],
            "intrinsics": torch.from_numpy(intr)[None], "near_fars": torch.from_numpy(nf)[None],
            "depths_h": torch.zeros(1, V, H, W), "proj_mats": torch.zeros(1, V, 3, 4)}


def render_randoms(H, W, n_rays=1024, n_samples=128, seed=0):
    """The injected random draws of the sampler: pix (2,N) int64 rows (x, y); eps; u."""
    g = torch.Generator().manual_seed(seed)
    xs = torch.randint(0, W, (n_rays,), generator=g)
    ys = torch.randint(0, H, (n_rays,), generator=g)
    eps = torch.randn(n_rays, n_samples, generator=g)
    u = torch.rand(n_rays // 2, n_samples, generator=g)
    return torch.stack((xs, ys)), eps, u


# ----------------------------------------------------------------------------------------
# a multi-view-consistent scan for the fusion filter
# ----------------------------------------------------------------------------------------
def _surface(X, Y):
    return 650.0 + 40.0 * np.sin(X / 80.0) * np.cos(Y / 60.0)


def fusion_scan(V=5, H=48, W=64, seed=0, n_src=4):
    """Depth maps of one smooth world surface seen from V cameras (so that they reproject onto each other), with seeded
    noise, a band of gross outliers per view, random confidences and 8-bit images.
    Returns dict: K (V,3,3) f32, E (V,4,4) f32, depth (V,H,W) f32, conf (V,H,W) f32, img (V,H,W,3) uint8, pairs."""
    Kq, Es = cameras(V, H, W)
    K = Kq.copy()
    K[:2] *= 4.0
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = np.linalg.inv(K) @ np.stack([xs.ravel(), ys.ravel(), np.ones(H * W)])
    depth = np.zeros((V, H, W), np.float32)
    for v in range(V):
        Ei = np.linalg.inv(Es[v])
        d = np.full(H * W, 650.0)
        for _ in range(25):                                   # fixed-point ray / surface intersection
            Pw = Ei[:3, :3] @ (rays * d) + Ei[:3, 3:4]
            d = d + (_surface(Pw[0], Pw[1]) - Pw[2])
        d = d + 0.25 * rng.standard_normal(H * W)
        d = d.reshape(H, W)
        d[:, (7 * v) % W:(7 * v) % W + 5] *= 1.06             # a band that fails the 1 % depth test
        depth[v] = d.astype(np.float32)
    conf = (0.55 + 0.45 * rng.random((V, H, W))).astype(np.float32)
    img = (255.0 * rng.random((V, H, W, 3))).astype(np.uint8)
    pairs = [(v, [(v + k) % V for k in range(1, n_src + 1)]) for v in range(V)]
    return {"K": np.broadcast_to(K.astype(np.float32), (V, 3, 3)).copy(), "E": np.stack(Es).astype(np.float32),
            "depth": depth, "conf": conf, "img": img, "pairs": pairs}


def write_fusion_scan(scan, pair_folder, out_folder, image_ext="png", depth_line="425.0 2.5"):
    """Lay the scan out the way the reference's filter_depth reads it (eval_rcmvsnet_dtu.py:341-368): pair.txt in
    pair_folder, cams/ + images/ + depth_est/ + confidence/ under out_folder (= its scan_folder)."""
    import os
    from PIL import Image
    from .data_io import save_pfm
    for sub in ("cams", "images", "depth_est", "confidence"):
        os.makedirs(os.path.join(out_folder, sub), exist_ok=True)
    os.makedirs(pair_folder, exist_ok=True)
    V = len(scan["depth"])
    with open(os.path.join(pair_folder, "pair.txt"), "w") as f:
        f.write("%d\n" % V)
        for ref, srcs in scan["pairs"]:
            f.write("%d\n%d %s\n" % (ref, len(srcs), " ".join("%d %.3f" % (s, 100.0 - i) for i, s in enumerate(srcs))))
    for v in range(V):
        with open(os.path.join(out_folder, "cams", "{:0>8}_cam.txt".format(v)), "w") as f:
            f.write("extrinsic\n")
            for row in scan["E"][v]:
                f.write(" ".join(repr(float(x)) for x in row) + "\n")
            f.write("\nintrinsic\n")
            for row in scan["K"][v]:
                f.write(" ".join(repr(float(x)) for x in row) + "\n")
            f.write("\n" + depth_line + "\n")
        # the reference opens '<view>.jpg'; PNG bytes under that name keep the fixture lossless (PIL sniffs the content)
        Image.fromarray(scan["img"][v]).save(os.path.join(out_folder, "images", "{:0>8}.jpg".format(v)), format=image_ext)
        save_pfm(os.path.join(out_folder, "depth_est", "{:0>8}.pfm".format(v)), scan["depth"][v])
        save_pfm(os.path.join(out_folder, "confidence", "{:0>8}.pfm".format(v)), scan["conf"][v])


def write_tanks_scan(scan, folder, depth_line="300.0 1100.0"):
    """The Tanks-and-Temples layout datasets/tanks.py reads: <folder>/{pair.txt, cams_1/<view:08d>_cam.txt, images/<view:08d>.jpg}
    with ``depth_min depth_max`` on the camera file's last line."""
    import os
    import shutil
    write_fusion_scan(scan, folder, folder, depth_line=depth_line)
    shutil.rmtree(os.path.join(folder, "cams_1"), ignore_errors=True)
    os.rename(os.path.join(folder, "cams"), os.path.join(folder, "cams_1"))


def tanks_fusion_scan(V=5, hw=(64, 96), orig_hw=(75, 100), seed=0, n_src=4):
    """A fusion scan in the Tanks-and-Temples situation (eval_rcmvsnet_tanks.py:269-330): depth maps at the network size
    ``hw`` while images and camera files describe the original size ``orig_hw`` (the filter rescales the intrinsics by
    img_wh / original and resizes the colour image)."""
    scan = fusion_scan(V=V, H=hw[0], W=hw[1], seed=seed, n_src=n_src)
    K = scan["K"].astype(np.float64)
    K[:, 0, :] *= orig_hw[1] / hw[1]
    K[:, 1, :] *= orig_hw[0] / hw[0]
    scan["K"] = K.astype(np.float32)
    rng = np.random.default_rng(seed + 100)
    scan["img"] = (255.0 * rng.random((V, orig_hw[0], orig_hw[1], 3))).astype(np.uint8)
    return scan


def write_tanks_fusion_scan(scan, scan_folder, out_folder):
    """scan_folder: pair.txt, cams_1/, images/ ; out_folder: depth_est/, confidence/ (eval_rcmvsnet_tanks.py:269-300)."""
    import os
    import shutil
    write_fusion_scan(scan, scan_folder, scan_folder)
    shutil.rmtree(os.path.join(scan_folder, "cams_1"), ignore_errors=True)
    os.rename(os.path.join(scan_folder, "cams"), os.path.join(scan_folder, "cams_1"))
    for sub in ("depth_est", "confidence"):
        os.makedirs(out_folder, exist_ok=True)
        shutil.rmtree(os.path.join(out_folder, sub), ignore_errors=True)
        shutil.move(os.path.join(scan_folder, sub), os.path.join(out_folder, sub))


def dtu_eval_scan(n_stl=20000, n_data=24000, extent=120.0, res=4.0, seed=0, outlier_frac=0.02, cluster_frac=0.05, noise=0.3):
    """A DTU-like scoring problem (rc_mvsnet_amd/dtu_eval.py): smooth height-field patches as the ground truth (stl, uniform
    samples), the reconstruction (data) = samples of the same patches with Gaussian noise, dense clusters (spacing well below
    0.2 mm) and far outliers; an ObsMask of Res-sized voxels around the stl points (dilated by one voxel), its BB and a ground
    plane that leaves a slab of stl points below it.  -> dict data (n_data,3) fp32, stl (n_stl,3) fp32, obs_mask (s1,s2,s3)
    bool indexed [x,y,z], bb (2,3) fp64, res, plane (4,) fp64."""
    rng = np.random.default_rng(seed)
    n_patch = 6

    def patch_points(k, n):
        p = rng.integers(0, n_patch, n)
        u = rng.random(n) * 0.45 * extent
        v = rng.random(n) * 0.45 * extent
        ox, oy = (p % 3) * 0.32 * extent, (p // 3) * 0.5 * extent
        x, y = ox + u, oy + v
        z = 0.1 * extent * (1 + p % 2) + 3.0 * np.sin(0.05 * x + p) + 2.0 * np.cos(0.07 * y - p)
        return np.stack([x, y, z], 1)

    stl = patch_points(0, n_stl)
    n_out = int(outlier_frac * n_data)
    n_clu = int(cluster_frac * n_data)
    surf = patch_points(1, n_data - n_out - n_clu) + rng.normal(0, noise, (n_data - n_out - n_clu, 3))
    centres = patch_points(2, max(1, n_clu // 50))
    clusters = centres[rng.integers(0, len(centres), n_clu)] + rng.normal(0, 0.05, (n_clu, 3))
    lo, hi = stl.min(0), stl.max(0)
    far = lo - 0.5 * extent + rng.random((n_out, 3)) * (hi - lo + extent)
    data = np.concatenate([surf, clusters, far])[rng.permutation(n_data)]
    return dict(data=data.astype(np.float32), **_dtu_truth(stl, res))


def _dtu_truth(stl, res):
    """stl (n,3) fp64 -> the scan's stl (fp32), an ObsMask of Res-sized voxels around the stl points (dilated by one voxel), its BB
    (the stl box widened by 10) and a ground plane 2 above the lowest stl point."""
    lo, hi = stl.min(0), stl.max(0)
    bb = np.stack([lo - 10.0, hi + 10.0]).astype(np.float64)
    size = np.floor((bb[1] - bb[0]) / res).astype(int) + 1
    v = np.floor((stl - bb[0]) / res + 0.5).astype(int)
    mask = np.zeros(size, dtype=bool)
    mask[v[:, 0], v[:, 1], v[:, 2]] = True
    grown = mask.copy()
    for a in range(3):
        for s in (-1, 1):
            grown |= np.roll(mask, s, axis=a)
    plane = np.array([0.0, 0.0, 1.0, -(lo[2] + 2.0)])
    return {"stl": stl.astype(np.float32), "obs_mask": grown, "bb": bb, "res": float(res), "plane": plane}


def _height(x, y):
    return 3.0 * np.sin(0.05 * x) + 2.0 * np.cos(0.07 * y) + 0.5 * np.sin(0.9 * x + 0.4 * y)


def dtu_eval_mesh(nx=200, ny=150, edge=0.4, n_stl=20000, res=4.0, seed=0, offset=0.15, jitter=0.25):
    """A DTU-like mesh scoring problem (dtu_eval.evaluate_mesh): the reconstruction is a triangulated height field over an
    nx x ny vertex grid of spacing ``edge`` (two triangles per cell, vertices jittered in x / y by up to ``jitter`` * edge and
    raised by a smooth error of amplitude ``offset``); the ground truth (stl) is n_stl uniform samples of the exact surface, with
    ObsMask and BB as in dtu_eval_scan and a ground plane above the lowest fifth of the surface.  -> dict verts (nx*ny,3) fp32, faces (2(nx-1)(ny-1),3) int32, stl, obs_mask, bb,
    res, plane."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(nx) * edge, np.arange(ny) * edge, indexing="xy")
    x = gx + (rng.random(gx.shape) - 0.5) * 2 * jitter * edge
    y = gy + (rng.random(gy.shape) - 0.5) * 2 * jitter * edge
    z = _height(x, y) + offset * np.sin(0.3 * x) * np.cos(0.2 * y)
    verts = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)
    i = (np.arange(ny - 1)[:, None] * nx + np.arange(nx - 1)[None, :]).ravel()
    faces = np.concatenate([np.stack([i, i + 1, i + nx], 1), np.stack([i + 1, i + nx + 1, i + nx], 1)]).astype(np.int32)
    su = rng.random(n_stl) * (nx - 1) * edge
    sv = rng.random(n_stl) * (ny - 1) * edge
    stl = np.stack([su, sv, _height(su, sv)], 1)
    truth = _dtu_truth(stl, res)
    zlo, zhi = stl[:, 2].min(), stl[:, 2].max()
    truth["plane"] = np.array([0.0, 0.0, 1.0, -(zlo + 0.2 * (zhi - zlo))])     # the lowest fifth of the surface lies below it
    return dict(verts=verts.astype(np.float32), faces=faces, **truth)


# ----------------------------------------------------------------------------------------
# a DTU training folder (datasets/dtu_train.py layout) for the training loader
# ----------------------------------------------------------------------------------------
def write_dtu_train_folder(folder, scans, n_views, seed, hw=(512, 640), raw_hw=(1200, 1600)):
    """Write a small folder in the layout of Yao Yao's preprocessed DTU training set and return the path of its list file:

        Cameras/pair.txt, Cameras/train/<view:08d>_cam.txt        quarter-resolution intrinsics of ``cameras(n_views, *hw)``
        Rectified/<scan>_train/rect_<view+1:03d>_<light>_r5000.png  7 lights per view, ``hw`` RGB
        Depths_raw/<scan>/depth_map_<view:04d>.pfm                  ``raw_hw`` depth of the smooth surface of ``fusion_scan``
        Depths_raw/<scan>/depth_visual_<view:04d>.png               ``raw_hw`` 8-bit visibility (values around the loader's > 10 test)

    Image pixel (y, x) is raw pixel (88 + 2 y, 160 + 2 x) for the default sizes, the relation the loader's half-size + centre crop
    assumes.  Every view lists all the others as sources."""
    import os
    from PIL import Image
    from .data_io import save_pfm
    H, W = hw
    RH, RW = raw_hw
    Kq, Es = cameras(n_views, H, W)
    Kf = Kq.copy()
    Kf[:2] *= 4.0
    os.makedirs(os.path.join(folder, "Cameras", "train"), exist_ok=True)
    with open(os.path.join(folder, "Cameras", "pair.txt"), "w") as f:
        f.write("%d\n" % n_views)
        for v in range(n_views):
            srcs = [(v + k) % n_views for k in range(1, n_views)]
            f.write("%d\n%d %s\n" % (v, len(srcs), " ".join("%d %.3f" % (s, 100.0 - i) for i, s in enumerate(srcs))))
    for v in range(n_views):
        with open(os.path.join(folder, "Cameras", "train", "{:0>8}_cam.txt".format(v)), "w") as f:
            f.write("extrinsic\n")
            for row in Es[v].astype(np.float32):
                f.write(" ".join(repr(float(x)) for x in row) + "\n")
            f.write("\nintrinsic\n")
            for row in Kq.astype(np.float32):
                f.write(" ".join(repr(float(x)) for x in row) + "\n")
            f.write("\n425.0 2.5\n")
    # raw pixel -> ray of the full-resolution camera (x_img = (x_raw - ox) / 2)
    oy, ox = (RH // 2 - H) // 2 * 2, (RW // 2 - W) // 2 * 2
    ys, xs = np.meshgrid((np.arange(RH, dtype=np.float64) - oy) / 2.0, (np.arange(RW, dtype=np.float64) - ox) / 2.0, indexing="ij")
    rays = np.linalg.inv(Kf) @ np.stack([xs.ravel(), ys.ravel(), np.ones(RH * RW)])
    yy, xx = np.meshgrid(np.linspace(-1.0, 1.0, RH), np.linspace(-1.0, 1.0, RW), indexing="ij")
    for si, scan in enumerate(scans):
        rng = np.random.default_rng(seed + 1000 * si)
        os.makedirs(os.path.join(folder, "Rectified", scan + "_train"), exist_ok=True)
        os.makedirs(os.path.join(folder, "Depths_raw", scan), exist_ok=True)
        for v in range(n_views):
            Ei = np.linalg.inv(Es[v])
            d = np.full(RH * RW, 650.0 + 5.0 * si)
            for _ in range(4):                                    # fixed-point ray / surface intersection, as fusion_scan
                Pw = Ei[:3, :3] @ (rays * d) + Ei[:3, 3:4]
                d = d + (_surface(Pw[0], Pw[1]) + 5.0 * si - Pw[2])
            save_pfm(os.path.join(folder, "Depths_raw", scan, "depth_map_{:0>4}.pfm".format(v)), d.reshape(RH, RW).astype(np.float32))
            r2 = (xx / 0.9) ** 2 + (yy / 0.8) ** 2
            visual = np.where(r2 < 1.0, 255, np.where(r2 < 1.1, 11, np.where(r2 < 1.2, 10, 0))).astype(np.uint8)
            Image.fromarray(visual).save(os.path.join(folder, "Depths_raw", scan, "depth_visual_{:0>4}.png".format(v)), compress_level=1)
            base = images(1, 1, H, W, seed + 100 * si + v)[0, 0].numpy().transpose(1, 2, 0)          # smooth, roughly unit range
            base = base + 0.1 * rng.standard_normal((H, W, 3))
            for light in range(7):
                img = np.clip(128.0 + (40.0 + 8.0 * light) * base, 0.0, 255.0).astype(np.uint8)
                Image.fromarray(img).save(os.path.join(folder, "Rectified", scan + "_train", "rect_{:0>3}_{}_r5000.png".format(v + 1, light)),
                                          compress_level=1)
    lst = os.path.join(folder, "train_list.txt")
    with open(lst, "w") as f:
        f.write("".join(s + "\n" for s in scans))
    return lst


# ----------------------------------------------------------------------------------------
# depth maps for the colour-map tests and a Tanks-and-Temples tree for the evaluation driver
# ----------------------------------------------------------------------------------------
def depth_vis_map(H, W, seed=0, outliers=0.03, noise=0.25):
    """One (H,W) fp32 depth map the way the network leaves it: the smooth surface of ``fusion_scan`` over the pixel grid plus
    seeded noise, and a fraction ``outliers`` of far values (2x to 6x the depth), which is what makes the reference colour up to
    the 95th percentile and not up to the maximum."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = _surface(xs * (640.0 / max(W, 1)), ys * (480.0 / max(H, 1))) + 0.3 * xs * (640.0 / max(W, 1)) + noise * rng.standard_normal((H, W))
    if outliers > 0:
        far = rng.random((H, W)) < outliers
        d = np.where(far, d * (2.0 + 4.0 * rng.random((H, W))), d)
    return d.astype(np.float32)


def write_tanks_tree(root, split="intermediate", scenes=("Family", "Horse"), V=7, hw=(64, 96), orig_hw=(75, 100), seed=0, n_src=6,
                     depth_line="425.0 935.0"):
    """<root>/<split>/<scene>/{pair.txt, cams_1/, images/} for each scene (real scene names, tiny images): what
    ``mvs_dataset.TanksDataset`` and ``fusion.filter_depth_tanks`` read.  The camera files hold the intrinsics at the ORIGINAL
    image size (datasets/tanks.py divides their first two rows by 4 for the coarsest stage).  Returns {scene: scan}."""
    import os
    import shutil
    out = {}
    for i, scene in enumerate(scenes):
        scan = tanks_fusion_scan(V=V, hw=hw, orig_hw=orig_hw, seed=seed + i, n_src=n_src)
        folder = os.path.join(root, split, scene)
        write_tanks_scan(scan, folder, depth_line=depth_line)
        for sub in ("depth_est", "confidence"):                     # write_fusion_scan's network outputs are not part of a data folder
            shutil.rmtree(os.path.join(folder, sub), ignore_errors=True)
        out[scene] = scan
    return out


def _similarity(axis, deg, scale, shift):
    """4x4 fp64: scale * (rotation by deg degrees about axis), then the shift"""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    t = math.radians(deg)
    T = np.eye(4)
    T[:3, :3] = scale * (np.eye(3) + math.sin(t) * K + (1.0 - math.cos(t)) * (K @ K))
    T[:3, 3] = shift
    return T


def tanks_fscore_scene(n_gt=5000, n_est=5000, tau=0.01, seed=0, rot_deg=3.0, shift_tau=3.0, scale=1.01, outlier_frac=0.1, missing_frac=0.25,
                       noise_tau=0.2):
    """A Tanks-and-Temples-shaped scoring problem with coordinates of order 1.  gt (n_gt,3) fp32: a bumpy closed surface
    (radius 1 + 0.12 sin 3x cos 2y sin 2z about the origin) sampled at random directions.  est (n_est,3) fp32, in a frame of its
    own: (1 - outlier_frac) of it are ground-truth points with z below the (1 - missing_frac) quantile (the top of the surface is
    missing) plus Gaussian noise of noise_tau * tau, the rest uniform outliers in the box; all mapped by T_true^-1.  T_true
    (est -> gt frame) is a 20 degree, scale 1.7 similarity; init = D T_true with the KNOWN error D: rot_deg degrees about a
    tilted axis, a shift of shift_tau * tau per axis, scale ``scale``.  volume: a concave (L-shaped) polygon prism about z that
    cuts one corner of the surface off.  -> dict(gt, est, T_true, init, D, volume=dict(axis, axis_min, axis_max, polygon (m,3)), tau)."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n_gt, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = 1.0 + 0.12 * np.sin(3.0 * d[:, 0]) * np.cos(2.0 * d[:, 1]) * np.sin(2.0 * d[:, 2] + 0.5)
    gt = (d * r[:, None]).astype(np.float32)
    n_out = int(round(outlier_frac * n_est))
    low = np.flatnonzero(gt[:, 2] < np.quantile(gt[:, 2], 1.0 - missing_frac))
    pick = low[rng.integers(0, len(low), n_est - n_out)]
    good = gt[pick].astype(np.float64) + rng.normal(0.0, noise_tau * tau, (n_est - n_out, 3))
    far = rng.uniform(-1.2, 1.2, (n_out, 3))
    est_gt_frame = np.concatenate([good, far])[rng.permutation(n_est)]
    T_true = _similarity((0.3, -0.5, 0.8), 20.0, 1.7, (0.4, -0.2, 0.3))
    D = _similarity((0.6, 0.3, -0.7), rot_deg, scale, (shift_tau * tau, -shift_tau * tau, 0.5 * shift_tau * tau))
    inv = np.linalg.inv(T_true)
    est = (est_gt_frame @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    polygon = np.array([[-1.3, -1.3], [1.3, -1.3], [1.3, 0.35], [0.4, 0.35], [0.4, 1.3], [-1.3, 1.3]])
    polygon = np.concatenate([polygon, np.zeros((len(polygon), 1))], 1)
    volume = {"axis": 2, "axis_min": -0.95, "axis_max": 1.3, "polygon": polygon}
    return {"gt": gt, "est": est, "T_true": T_true, "init": D @ T_true, "D": D, "volume": volume, "tau": float(tau)}


def write_tanks_gt_tree(root, plydir, scenes=("Barn", "Truck"), n_gt=5000, n_est=5000, n_cams=12, seed=0, taus=None):
    """The five files of every scene as rc_mvsnet_amd.tanks_fscore reads them: <root>/<scene>/<scene>.ply (ground truth),
    <scene>.json (Open3D's SelectionPolygonVolume), <scene>_trans.txt (the scene's ``init``), <scene>_COLMAP_SfM.log (n_cams
    camera-to-world poses in the estimate's frame) and <plydir>/<scene>.ply (the estimate).  taus: {scene: tau} (default
    tanks_fscore.SCENE_TAU).  Returns {scene: tanks_fscore_scene's dict}."""
    import json
    import os
    from .fusion import ply_bytes
    if taus is None:
        from .tanks_fscore import SCENE_TAU as taus
    os.makedirs(plydir, exist_ok=True)
    out = {}
    for i, scene in enumerate(scenes):
        s = tanks_fscore_scene(n_gt=n_gt, n_est=n_est, tau=taus[scene], seed=seed + i)
        folder = os.path.join(root, scene)
        os.makedirs(folder, exist_ok=True)
        grey = np.full((1, 3), 128, dtype=np.uint8)
        for path, pts in ((os.path.join(folder, f"{scene}.ply"), s["gt"]), (os.path.join(plydir, f"{scene}.ply"), s["est"])):
            with open(path, "wb") as f:
                f.write(ply_bytes(pts, np.repeat(grey, len(pts), 0)))
        v = s["volume"]
        with open(os.path.join(folder, f"{scene}.json"), "w") as f:
            json.dump({"axis_max": v["axis_max"], "axis_min": v["axis_min"], "bounding_polygon": v["polygon"].tolist(),
                       "class_name": "SelectionPolygonVolume", "orthogonal_axis": "XYZ"[v["axis"]], "version_major": 1, "version_minor": 0}, f)
        np.savetxt(os.path.join(folder, f"{scene}_trans.txt"), s["init"], fmt="%.17g")
        rng = np.random.default_rng(1000 + seed + i)
        with open(os.path.join(folder, f"{scene}_COLMAP_SfM.log"), "w") as f:
            for c in range(n_cams):
                pose = _similarity(rng.normal(size=3), rng.uniform(0.0, 180.0), 1.0, rng.uniform(-2.0, 2.0, 3))
                f.write(f"{c} {c} {n_cams}\n" + "".join(" ".join("%.17g" % x for x in row) + "\n" for row in pose))
        out[scene] = s
    return out


# ----------------------------------------------------------------------------------------
# a COLMAP sparse model for rc_mvsnet_amd/colmap_import.py
# ----------------------------------------------------------------------------------------
def _rotmat_to_qvec(R):
    """3x3 rotation -> (w, x, y, z) with w >= 0"""
    t = np.trace(R)
    if t > 0:
        s = math.sqrt(t + 1.0) * 2.0
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = math.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2.0
        q = np.zeros(4)
        q[0], q[1 + i], q[1 + j], q[1 + k] = (R[k, j] - R[j, k]) / s, 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s
    return q if q[0] >= 0 else -q


def colmap_arrays(n_images=6, n_points=400, hw=(64, 96), seed=0, radius=4.0, extent=1.3, arc_deg=60.0, keep=1.0):
    """Cameras on a ring arc of ``arc_deg`` degrees and radius ``radius`` looking at the origin, n_points uniform in the box
    [-extent, extent]^3; an image observes the points its frustum holds (inside the hw image, in front), each kept with
    probability ``keep``.  -> dict: extrinsics (n,4,4), centres (n,3), intrinsics (n,3,3), points (m,3), offsets (n+1,) int64,
    ids int32 (per image ascending), uv [n] of (c,2) pixel positions, hw."""
    rng = np.random.default_rng(seed)
    H, W = hw
    K = np.array([[1.2 * W, 0.0, W / 2.0], [0.0, 1.212 * W, H / 2.0], [0.0, 0.0, 1.0]])
    pts = rng.uniform(-extent, extent, (n_points, 3))
    E, C = np.zeros((n_images, 4, 4)), np.zeros((n_images, 3))
    lists, uvs, offsets = [], [], np.zeros(n_images + 1, dtype=np.int64)
    for k in range(n_images):
        a = math.radians(arc_deg) * (k / max(n_images - 1, 1) - 0.5)
        c = np.array([radius * math.sin(a), 0.15 * radius * math.sin(3.0 * a + 0.4), -radius * math.cos(a)])
        z = -c / np.linalg.norm(c)
        x = np.cross(np.array([0.0, 1.0, 0.0]), z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        E[k, :3, :3], E[k, :3, 3], E[k, 3, 3], C[k] = R, -R @ c, 1.0, c
        cam = pts @ R.T + E[k, :3, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            u = K[0, 0] * cam[:, 0] / cam[:, 2] + K[0, 2]
            v = K[1, 1] * cam[:, 1] / cam[:, 2] + K[1, 2]
        seen = (cam[:, 2] > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        if keep < 1.0:
            seen &= rng.random(n_points) < keep
        idx = np.flatnonzero(seen).astype(np.int32)
        lists.append(idx)
        uvs.append(np.stack([u[idx], v[idx]], 1))
        offsets[k + 1] = offsets[k] + len(idx)
    return {"extrinsics": E, "centres": C, "intrinsics": np.broadcast_to(K, (n_images, 3, 3)).copy(), "points": pts, "offsets": offsets,
            "ids": np.concatenate(lists).astype(np.int32), "uv": uvs, "hw": (H, W)}


# moderate barrel distortion in each polynomial model's own parameter order (after the focal lengths and the principal point)
COLMAP_DISTORTION = {"SIMPLE_RADIAL": [-0.12], "RADIAL": [-0.12, 0.03], "OPENCV": [-0.12, 0.03, 0.004, -0.003],
                     "FULL_OPENCV": [-0.12, 0.03, 0.004, -0.003, 0.01, 0.02, -0.01, 0.005]}


def colmap_model(n_images=6, n_points=400, hw=(64, 96), seed=0, camera_model="PINHOLE", ext="jpg", distortion=None, **kwargs):
    """colmap_arrays as COLMAP's records, with what a reader has to cope with: image ids 10, 12, ... listed in shuffled order, point
    ids 5, 8, ... listed in shuffled order, 2-D points in shuffled order with unmatched ones (point3D_id -1) and one observation
    listed twice.  -> dict(cameras, images, points, truth=the colmap_arrays dict in renumbered order).  ``camera_model`` may be a
    polynomial model (SIMPLE_RADIAL, RADIAL, OPENCV, FULL_OPENCV) with ``distortion`` = its coefficients in its own order (default
    COLMAP_DISTORTION); the 2-D points stay the pinhole projections, which the import does not read."""
    A = colmap_arrays(n_images, n_points, hw, seed, **kwargs)
    rng = np.random.default_rng(seed + 7)
    H, W = hw
    K = A["intrinsics"][0]
    if camera_model in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL"):
        A["intrinsics"][:, 1, 1] = K[0, 0]
        params = [K[0, 0], K[0, 2], K[1, 2]]
    else:
        params = [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]
    if camera_model in COLMAP_DISTORTION:
        coeffs = list(COLMAP_DISTORTION[camera_model] if distortion is None else distortion)
        if len(coeffs) != len(COLMAP_DISTORTION[camera_model]):
            raise ValueError(f"{camera_model} takes {len(COLMAP_DISTORTION[camera_model])} distortion coefficients, got {len(coeffs)}")
        params = params + coeffs
    elif distortion is not None:
        raise ValueError(f"{camera_model} has no distortion coefficients")
    cameras = [{"id": 3, "model": camera_model, "width": W, "height": H, "params": [float(p) for p in params]}]
    p2d_dtype = np.dtype([("x", "<f8"), ("y", "<f8"), ("id", "<i8")])
    images, tracks = [], [[] for _ in range(n_points)]
    for k in range(n_images):
        idx = A["ids"][A["offsets"][k]:A["offsets"][k + 1]]
        n_free = 3 + k
        p2d = np.zeros(len(idx) + n_free + (1 if k == 0 and len(idx) else 0), dtype=p2d_dtype)
        p2d["x"][:len(idx)], p2d["y"][:len(idx)], p2d["id"][:len(idx)] = A["uv"][k][:, 0], A["uv"][k][:, 1], 5 + 3 * idx.astype(np.int64)
        p2d["x"][len(idx):], p2d["y"][len(idx):], p2d["id"][len(idx):] = rng.uniform(0, W, len(p2d) - len(idx)), rng.uniform(0, H, len(p2d) - len(idx)), -1
        if k == 0 and len(idx):
            p2d[-1] = p2d[0]                                       # the same 3-D point observed twice
        p2d = p2d[rng.permutation(len(p2d))]
        for at, pid in enumerate(p2d["id"]):
            if pid >= 0:
                tracks[(int(pid) - 5) // 3].append((10 + 2 * k, at))
        images.append({"id": 10 + 2 * k, "qvec": _rotmat_to_qvec(A["extrinsics"][k, :3, :3]), "tvec": A["extrinsics"][k, :3, 3].copy(),
                       "camera_id": 3, "name": "view_%03d.%s" % (k, ext), "points2D": p2d})
    order = rng.permutation(n_points)
    points = {"ids": 5 + 3 * order.astype(np.int64), "xyz": A["points"][order], "rgb": rng.integers(0, 256, (n_points, 3)).astype(np.uint8),
              "error": rng.uniform(0.1, 1.0, n_points), "tracks": [np.array(tracks[i], dtype=np.int32).reshape(-1, 2) for i in order]}
    return {"cameras": cameras, "images": [images[i] for i in rng.permutation(n_images)], "points": points, "truth": A}


def write_colmap_model(model, folder, binary=False):
    """cameras / images / points3D of a colmap_model as .txt (numbers by repr: they read back to the same doubles) or .bin"""
    import os
    import struct
    os.makedirs(folder, exist_ok=True)
    model_ids = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2, "RADIAL": 3, "OPENCV": 4, "OPENCV_FISHEYE": 5, "FULL_OPENCV": 6}
    P = model["points"]
    if binary:
        with open(os.path.join(folder, "cameras.bin"), "wb") as f:
            f.write(struct.pack("<Q", len(model["cameras"])))
            for c in model["cameras"]:
                f.write(struct.pack("<iiQQ", c["id"], model_ids[c["model"]], c["width"], c["height"]) + struct.pack("<%dd" % len(c["params"]), *c["params"]))
        with open(os.path.join(folder, "images.bin"), "wb") as f:
            f.write(struct.pack("<Q", len(model["images"])))
            for im in model["images"]:
                f.write(struct.pack("<i7di", im["id"], *im["qvec"], *im["tvec"], im["camera_id"]) + im["name"].encode() + b"\0")
                f.write(struct.pack("<Q", len(im["points2D"])) + im["points2D"].tobytes())
        with open(os.path.join(folder, "points3D.bin"), "wb") as f:
            f.write(struct.pack("<Q", len(P["ids"])))
            for i in range(len(P["ids"])):
                f.write(struct.pack("<Q3d3BdQ", int(P["ids"][i]), *P["xyz"][i], *[int(v) for v in P["rgb"][i]], float(P["error"][i]), len(P["tracks"][i])))
                f.write(P["tracks"][i].astype("<i4").tobytes())
        return
    with open(os.path.join(folder, "cameras.txt"), "w") as f:
        f.write("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n")
        for c in model["cameras"]:
            f.write("%d %s %d %d %s\n" % (c["id"], c["model"], c["width"], c["height"], " ".join(repr(float(p)) for p in c["params"])))
    with open(os.path.join(folder, "images.txt"), "w") as f:
        f.write("# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n"
                "#   POINTS2D[] as (X, Y, POINT3D_ID)\n")
        for im in model["images"]:
            f.write("%d %s %d %s\n" % (im["id"], " ".join(repr(float(v)) for v in list(im["qvec"]) + list(im["tvec"])), im["camera_id"], im["name"]))
            f.write(" ".join("%r %r %d" % (float(p["x"]), float(p["y"]), int(p["id"])) for p in im["points2D"]) + "\n")
    with open(os.path.join(folder, "points3D.txt"), "w") as f:
        f.write("# 3D point list with one line of data per point:\n#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n")
        for i in range(len(P["ids"])):
            f.write("%d %s %d %d %d %r %s\n" % (int(P["ids"][i]), " ".join(repr(float(v)) for v in P["xyz"][i]), *[int(v) for v in P["rgb"][i]],
                                               float(P["error"][i]), " ".join("%d %d" % (a, b) for a, b in P["tracks"][i])))


def write_colmap_images(model, folder, seed=0):
    """small random images under the names the model lists (the format follows the extension), at the camera's size"""
    import os
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    rng = np.random.default_rng(seed)
    cams = {c["id"]: c for c in model["cameras"]}
    for im in model["images"]:
        c = cams[im["camera_id"]]
        Image.fromarray((255.0 * rng.random((c["height"], c["width"], 3))).astype(np.uint8)).save(os.path.join(folder, im["name"]))
