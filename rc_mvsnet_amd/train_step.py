"""Synthetic-input driver reproducing the call sequence of one reference training iteration
(train_rcmvsnet.py:145-204,279-312,330-376,397-446): forward #1 of CascadeMVSNet (returns the stage-1
volume_feature_no_ref), forward #2 on augmented images, Rendering_Consistency_Net.forward on the detached
pseudo depth, ONE backward over the summed losses, optimizer step.

The losses are the reference's own (rc_mvsnet_amd/losses.py: UnsupLossMultiStage on forward #1, AugLossMultiStage against
the detached pseudo depth on forward #2, MSE + SL1Loss on the rendered rays), each a fused HIP call.  Everything runs on the
HIP library; there is no CPU path (tools/train_bench.py can swap the two network forwards for the oracle's op graph to
time the PyTorch-ROCm equivalent).
The renderer is hard-wired to 4 views (1 ref + 3 src; SURVEY.md header note 2).
"""
import types

import torch

from . import synthetic
from .casmvsnet import CascadeMVSNet
from .render_consist_net import Rendering_Consistency_Net


def render_args(n_samples=128):
    return types.SimpleNamespace(multires=10, i_embed=0, pts_dim=3, dir_dim=3, netdepth=6, netwidth=128, net_type="v0",
                                 netchunk=1024, ckpt=None, N_samples=n_samples, N_importance=0, perturb=1.0, use_viewdirs=True,
                                 white_bkgd=False, raw_noise_std=0.0, pad=0, img_downscale=1.0, use_color_volume=False,
                                 multires_views=4)


def build(device, ndepths=(48, 32, 8), n_samples=128, seed=0):
    model = CascadeMVSNet(ndepths=list(ndepths), depth_interals_ratio=[4, 2, 1])
    model.load_state_dict(synthetic.cascade_state_dict(seed), strict=True)
    model_nerf = Rendering_Consistency_Net(render_args(n_samples))
    model_nerf.load_state_dict(synthetic.render_state_dict(seed + 1), strict=True)
    model, model_nerf = model.to(device), model_nerf.to(device)
    opt = torch.optim.Adam(list(model.parameters()) + list(model_nerf.parameters()), lr=1e-4, betas=(0.9, 0.999))
    return model, model_nerf, opt


def make_data_parallel(modules, lr=1e-4):
    """The data-parallel form of a training setup (BASELINE configs[3]; train_rcmvsnet.py:524-525,565-578): every BatchNorm becomes a
    SyncBatchNorm, ONE Adam over all parameters (the converted modules own new parameter objects), and a parallel.GradSync that averages
    all gradients in one reduce-scatter + all-gather message.  Needs an initialised process group.  -> (modules, optimizer, grad_sync);
    used by `bench.py --workload train_step --gpus N` and by tests/test_multiproc_cpu.py over gloo."""
    from . import parallel
    modules = [torch.nn.SyncBatchNorm.convert_sync_batchnorm(m) for m in modules]
    opt = torch.optim.Adam([p for m in modules for p in m.parameters()], lr=lr, betas=(0.9, 0.999))
    return modules, opt, parallel.GradSync(modules)


def synthetic_sample(device, H=512, W=640, V=4, seed=0):
    imgs, pm, dv = synthetic.cascade_inputs(1, V, H, W, seed)
    batch = synthetic.render_batch(V, H, W, seed)
    to = lambda t: t.to(device)
    return to(imgs), {k: to(v) for k, v in pm.items()}, to(dv), {k: to(v) for k, v in batch.items()}


DLOSSW = (0.5, 1.0, 2.0)      # --dlossw default, train_rcmvsnet.py:61


def train_step(model, model_nerf, opt, imgs, proj, depth_values, batch, w_aug=0.01, cascade_fn=None, render_fn=None, grad_sync=None,
               imgs_aug=None, loss_imgs=None):
    """One iteration with the reference's losses (train_rcmvsnet.py:279-312,330-376,397-446); returns a dict of scalar losses
    (python floats).  cascade_fn(model, imgs, proj, depth_values) / render_fn(model_nerf, volume_feature, pseudo_depth, batch)
    default to the modules' own forward.  grad_sync: a parallel.GradSync over both models (data-parallel training: the
    gradients live in its flat buffer and are averaged over the ranks with one message before the optimizer step).
    imgs_aug / loss_imgs (B,V,3,H,W): what a training loader supplies (mvs_dataset.DTUTrainDataset) -- the colour-augmented
    images forward #2 reads (sample["imgs_aug"], :410-415) and the per-image centred images the photometric loss reads
    (sample["center_imgs"], :345).  None (synthetic inputs) uses ``imgs`` in their place."""
    from . import losses
    cascade_fn = cascade_fn or (lambda m, *a: m(*a))
    render_fn = render_fn or (lambda m, *a: m(*a))
    model.train()
    model_nerf.train()
    if grad_sync is not None:
        grad_sync.zero()
    else:
        opt.zero_grad(set_to_none=True)
    dlossw = list(DLOSSW)
    outputs, volume_feature = cascade_fn(model, imgs, proj, depth_values)          # forward #1 (:342)
    loss_base, _ = losses.UnsupLossMultiStage()(outputs, imgs if loss_imgs is None else loss_imgs, proj, dlossw=dlossw)  # (:345)
    pseudo_depth = outputs["depth"].detach()
    aug_src = imgs if imgs_aug is None else imgs_aug
    ref_img, filter_mask = losses.random_image_mask(aug_src[:, 0], (imgs.shape[3] // 3, imgs.shape[4] // 3))   # (:412)
    imgs_aug = torch.cat((ref_img.unsqueeze(1), aug_src[:, 1:]), dim=1)
    outputs_aug, _ = cascade_fn(model, imgs_aug, proj, depth_values)               # forward #2 (:415)
    loss_aug, _ = losses.AugLossMultiStage()(outputs_aug, pseudo_depth, None, filter_mask, dlossw=dlossw)
    loss_aug = loss_aug * w_aug                                                    # (:420-424)
    rgb, _, _, depth_pred, _, _, rays_depth, target = render_fn(model_nerf, volume_feature, pseudo_depth, dict(batch))   # (:285)
    img_loss = torch.mean((rgb - target) ** 2)                                     # img2mse (:291)
    depth_loss = losses.SL1Loss()(depth_pred, rays_depth, rays_depth > 0)          # (:295-297)
    loss = loss_base + loss_aug + img_loss + depth_loss
    loss.backward()                                                                # one backward over both forwards (:311)
    if grad_sync is not None:
        grad_sync.sync()
    opt.step()
    return {"loss": float(loss.detach()), "base": float(loss_base.detach()), "aug": float(loss_aug.detach()),
            "render": float((img_loss + depth_loss).detach())}
