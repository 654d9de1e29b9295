"""Training loader without a GPU: the host half of mvs_dataset.DTUTrainDataset against items recorded from the reference's
own loader (tests/golden/train_dataset.npz, written by make_golden_train_dataset.py), the augmentation draws, the device half
on the CPU emulation, train_step's two new inputs, and the training driver's schedule / checkpoints / resume."""
import json
import os
import types
import zlib

import numpy as np
import pytest
import torch

import train_dataset_oracle as O
from rc_mvsnet_amd import _lib, mvs_dataset, synthetic, train_driver

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "train_dataset.npz"))
NVIEWS = int(GOLD["nviews"])
PLAIN = ("depth_values", "w2cs", "c2ws", "near_fars", "proj_mats", "intrinsics", "view_ids", "light_id", "affine_mat", "affine_mat_inv",
         "c2ws_all")


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dtu_train"))
    lst = synthetic.write_dtu_train_folder(d, [str(s) for s in GOLD["scans"]], int(GOLD["n_views_folder"]), int(GOLD["seed"]))
    return d, lst


def dense_keys(item):
    out = {"depths_h": item["depths_h"]}
    for k in ("depth", "mask"):
        for s, v in item[k].items():
            out[k + ":" + s] = v
    return out


def check_item_against_golden(item, idx):
    """every non-image key of an item (or of a host half) against the reference's; shared with the GPU test"""
    tag = "%d:" % idx
    for k in PLAIN:
        assert np.array_equal(item[k], GOLD[tag + k]) and np.asarray(item[k]).dtype == GOLD[tag + k].dtype, k
    assert item["scan"] == str(GOLD[tag + "scan"])
    for k, v in dense_keys(item).items():
        crc = GOLD[tag + k + ":crc"]
        assert v.shape == tuple(crc[1:]) and str(v.dtype) == str(GOLD[tag + k + ":dtype"]), k
        assert np.array_equal(v[..., ::8, ::8], GOLD[tag + k]), k
        assert zlib.crc32(np.ascontiguousarray(v).tobytes()) == int(crc[0]), k          # the full array, through its checksum


def golden_aug(idx):
    tag = "%d:" % idx
    return {"order": GOLD[tag + "aug_order"], "factors": GOLD[tag + "aug_factors"], "gamma": GOLD[tag + "aug_gamma"]}


def test_oracle_matches_reference_golden(folder):
    """the oracle (Pillow + torch CPU ops) on the decoded files with the recorded parameters gives the reference's image tensors
    (the recorded run used these very calls for ColorJitter; ToTensor / gamma / Normalize / center_image ran in the reference)"""
    from PIL import Image
    d, _ = folder
    idx = int(GOLD["items"][0])
    aug = golden_aug(idx)
    for v, vid in enumerate(GOLD["%d:view_ids" % idx]):
        raw = np.array(Image.open(os.path.join(d, "Rectified/scan1_train/rect_{:0>3}_0_r5000.png".format(vid + 1))), dtype=np.uint8)
        assert np.array_equal(O.images_seg(raw)[:, ::16, ::16], GOLD["%d:imgs" % idx][v])
        assert np.array_equal(O.images_aug(raw, aug["order"][v], aug["factors"][v], aug["gamma"][v])[:, ::16, ::16], GOLD["%d:imgs_aug" % idx][v])
        assert np.array_equal(O.center_image_reference(raw)[:, ::16, ::16], GOLD["%d:center_imgs" % idx][v])


def test_host_half_matches_reference(folder):
    d, lst = folder
    ds = mvs_dataset.DTUTrainDataset(d, lst, "train", NVIEWS, 192, 1.06, device="cpu")
    assert len(ds) == int(GOLD["len"])
    for idx in GOLD["items"]:
        host = ds.load_host(int(idx))
        check_item_against_golden(host, int(idx))
        assert host["raw"].shape == (NVIEWS, 512, 640, 3) and host["raw"].dtype == np.uint8
    with pytest.raises(ValueError):
        mvs_dataset.DTUTrainDataset(d, lst, "test", NVIEWS)


def test_items_on_emulation_match_reference(folder, emu):
    """the whole item, device half on the emulated kernels, with the reference's recorded augmentation parameters replayed"""
    d, lst = folder
    ds = mvs_dataset.DTUTrainDataset(d, lst, "train", NVIEWS, 192, 1.06, device="cpu")
    idx = int(GOLD["items"][1])
    host = ds.load_host(idx)
    host["aug"] = golden_aug(idx)
    item = ds.to_device(host)
    check_item_and_images_against_golden(item, idx, atol=1e-6)
    batch = ds.render_batch(item)
    assert batch["imgs"].shape == (1, NVIEWS, 3, 512, 640) and batch["w2cs"].shape == (1, NVIEWS, 4, 4)
    assert batch["depths_h"].shape == (1, NVIEWS, 512, 640) and batch["near_fars"].dtype == torch.float32


# center_imgs: the golden is the reference's fp32 numpy computation -- np.mean / np.var over axes (0, 1) of an (H, W, 3) fp32
# array, a strided reduction that numpy accumulates naively in fp32 over 327 680 values -- while the kernel rounds an fp64
# result once.  The distance between the golden and the fp64 oracle over the golden's two items, measured on the CPU with no
# code under test involved, is 2.541e-4 in conftest.rel_err terms (test_center_golden_distance_is_as_recorded re-measures
# it).  Bound = 1e-6 (kernel vs fp64 oracle) + that distance, rounded up to 2.6e-4.
CENTER_GOLDEN_DISTANCE = 2.6e-4


def check_item_and_images_against_golden(item, idx, atol):
    from conftest import rel_err
    check_item_against_golden(item, idx)
    tag = "%d:" % idx
    for s in ("stage1", "stage2", "stage3"):
        assert np.array_equal(item["proj_matrices"][s], GOLD[tag + "proj_matrices:" + s]), s
    for k in ("imgs", "imgs_aug"):
        assert tuple(item[k].shape) == (NVIEWS, 3, 512, 640)
        assert np.allclose(item[k][:, :, ::16, ::16].cpu().numpy(), GOLD[tag + k], rtol=0, atol=atol), k
    err = rel_err(item["center_imgs"][:, :, ::16, ::16].cpu(), GOLD[tag + "center_imgs"])
    print(f"center_imgs vs reference golden (item {idx}): rel_err {err:.3e}")
    assert err <= 1e-6 + CENTER_GOLDEN_DISTANCE


def test_center_golden_distance_is_as_recorded(folder):
    from PIL import Image
    from conftest import rel_err
    d, _ = folder
    worst = 0.0
    for idx in GOLD["items"]:
        scan, light = str(GOLD["%d:scan" % idx]), int(GOLD["%d:light_id" % idx])
        for v, vid in enumerate(GOLD["%d:view_ids" % idx]):
            raw = np.array(Image.open(os.path.join(d, "Rectified/{}_train/rect_{:0>3}_{}_r5000.png".format(scan, vid + 1, light))), dtype=np.uint8)
            worst = max(worst, rel_err(GOLD["%d:center_imgs" % idx][v], O.center_image(raw)[:, ::16, ::16]))
    print(f"reference fp32 center_image vs fp64 oracle: rel_err {worst:.3e}")
    assert worst <= CENTER_GOLDEN_DISTANCE


def test_augmentation_draws(folder):
    d, lst = folder
    ds = mvs_dataset.DTUTrainDataset(d, lst, "train", NVIEWS, device="cpu", seed=3)
    a, b = ds.load_host(5)["aug"], ds.load_host(5)["aug"]
    other = ds.load_host(6)["aug"]
    for k in a:
        assert np.array_equal(a[k], b[k]), k                                     # a function of (seed, epoch, idx)
    assert not np.array_equal(a["factors"], other["factors"])
    ds.set_epoch(1)
    c = ds.load_host(5)["aug"]
    assert not np.array_equal(a["factors"], c["factors"]) and not np.array_equal(a["gamma"], c["gamma"])
    ds2 = mvs_dataset.DTUTrainDataset(d, lst, "train", NVIEWS, device="cpu", seed=4)
    assert not np.array_equal(a["factors"], ds2.load_host(5)["aug"]["factors"])
    orders = set()
    for idx in range(0, 70, 3):
        aug = ds.load_host(idx)["aug"]
        assert aug["order"].shape == (NVIEWS, 4) and aug["factors"].dtype == np.float32
        for v in range(NVIEWS):
            assert sorted(aug["order"][v]) == [0, 1, 2, 3]
            orders.add(tuple(aug["order"][v]))
            for k, (lo, hi) in enumerate(mvs_dataset.JITTER_RANGES):
                assert lo <= aug["factors"][v, k] <= hi
            assert mvs_dataset.GAMMA_RANGE[0] <= aug["gamma"][v] <= mvs_dataset.GAMMA_RANGE[1]
    assert len(orders) > 12


def test_random_view(folder):
    d, lst = folder
    ds = mvs_dataset.DTUTrainDataset(d, lst, "train", NVIEWS, device="cpu", random_view=True, seed=1)
    seen = set()
    for idx in range(0, 35, 7):
        h = ds.load_host(idx)
        ref, srcs = ds.metas[idx][2], ds.metas[idx][3]
        ids = [int(x) for x in h["view_ids"]]
        assert ids[0] == ref and len(set(ids)) == NVIEWS and set(ids[1:]) <= set(srcs)
        assert ids == [int(x) for x in ds.load_host(idx)["view_ids"]]
        seen.add(tuple(srcs.index(i) for i in ids[1:]))
    assert any(s != (0, 1, 2) for s in seen)


def test_missing_and_odd_files(folder, tmp_path):
    import shutil
    d, lst = folder
    small = str(tmp_path / "d")
    for sub in ("Cameras", "Rectified/scan1_train", "Depths_raw/scan1"):
        shutil.copytree(os.path.join(d, sub), os.path.join(small, sub))
    one = str(tmp_path / "list.txt")
    open(one, "w").write("scan1\n")
    ds = mvs_dataset.DTUTrainDataset(small, one, "train", NVIEWS, device="cpu")
    for v in range(5):
        if v != 0:
            os.remove(os.path.join(small, "Depths_raw/scan1/depth_map_{:0>4}.pfm".format(v)))
    # a source view without a depth map contributes the reference's (1,1) zeros (dtu_train.py:303-308); next to a (512,640)
    # map np.stack then refuses the item, in the reference and here alike
    with pytest.raises(ValueError, match="same shape"):
        ds.load_host(0)
    os.rename(os.path.join(small, "Depths_raw/scan1/depth_map_0000.pfm"), os.path.join(small, "Depths_raw/scan1/depth_map_0004.pfm"))
    with pytest.raises(_lib.RcmvsError, match="missing"):                       # a reference view without a depth map
        ds.load_host(0)
    from rc_mvsnet_amd.data_io import save_pfm
    save_pfm(os.path.join(small, "Depths_raw/scan1/depth_map_0004.pfm"), np.ones((600, 800), np.float32))
    with pytest.raises(_lib.RcmvsError, match="raw size"):
        ds.load_host(7 * 4)


def test_loader_fails_loudly_without_a_gpu(folder):
    d, lst = folder
    ds = mvs_dataset.DTUTrainDataset(d, lst, "train", NVIEWS, device="cpu")
    with pytest.raises(_lib.RcmvsError):
        ds[0]


def test_prefetch_keeps_order(folder, monkeypatch):
    d, lst = folder
    ds = mvs_dataset.DTUTrainDataset(d, lst, "train", NVIEWS, device="cpu")
    monkeypatch.setattr(ds, "to_device", lambda host: host)
    order = [9, 3, 40, 3, 69]
    got = list(mvs_dataset.prefetch(ds, indices=order, workers=3, depth=4))
    for idx, h in zip(order, got):
        want = ds.load_host(idx)
        assert np.array_equal(h["raw"], want["raw"]) and np.array_equal(h["aug"]["factors"], want["aug"]["factors"]) and h["scan"] == want["scan"]


def test_train_step_new_inputs_on_emulation(emu):
    """train_step on the emulated loss kernels at a small size, with stand-ins for the two networks (their forwards take minutes on
    the emulation and are not what changes): without the new arguments, and with both None, the losses are the same numbers;
    given, imgs_aug is what forward #2 reads and loss_imgs what the photometric loss reads."""
    from rc_mvsnet_amd import train_step as ts
    dev = torch.device("cpu")
    H, W = 32, 48
    seen = []

    def cascade_fn(model, imgs, proj, dv):
        seen.append(imgs)
        g = imgs[:, 0].mean(1, keepdim=True)                                   # (B,1,H,W)
        out = {}
        for k, f in (("stage1", 4), ("stage2", 2), ("stage3", 1)):
            out[k] = {"depth": (650.0 + model.weight.sum() * torch.nn.functional.avg_pool2d(g, f)).squeeze(1)}
        out["depth"] = out["stage3"]["depth"]
        return out, None

    def render_fn(model_nerf, vol, pseudo, batch):
        rgb = model_nerf.weight.sum() * torch.ones(8, 3)
        depth = model_nerf.weight.sum() * torch.ones(8) + 600.0
        return rgb, None, None, depth, None, None, torch.full((8,), 640.0), torch.zeros(8, 3)

    def run(**kw):
        torch.manual_seed(0)
        np.random.seed(0)
        model, model_nerf = torch.nn.Linear(2, 2), torch.nn.Linear(2, 2)
        opt = torch.optim.Adam(list(model.parameters()) + list(model_nerf.parameters()), lr=1e-4)
        imgs, proj, dv, batch = ts.synthetic_sample(dev, H=H, W=W, V=4)
        kw = {k: (v(imgs) if callable(v) else v) for k, v in kw.items()}
        del seen[:]
        out = ts.train_step(model, model_nerf, opt, imgs, proj, dv, batch, cascade_fn=cascade_fn, render_fn=render_fn, **kw)
        return out, imgs, list(seen)

    plain, imgs, fwd = run()
    none, _, _ = run(imgs_aug=None, loss_imgs=None)
    assert plain == none and all(np.isfinite(v) for v in plain.values())
    assert torch.equal(fwd[1][:, 1:], imgs[:, 1:])                               # forward #2 read the plain source views
    given, imgs, fwd = run(imgs_aug=lambda i: i * 0.9 + 0.05, loss_imgs=lambda i: i * 1.1 - 0.2)
    assert all(np.isfinite(v) for v in given.values())
    assert torch.equal(fwd[0], imgs) and torch.equal(fwd[1][:, 1:], (imgs * 0.9 + 0.05)[:, 1:])
    masked = fwd[1][:, 0] != (imgs * 0.9 + 0.05)[:, 0]
    assert masked.any() and not masked.all()                                     # random_image_mask ran on the augmented reference view
    assert given["base"] != plain["base"] and given["aug"] != plain["aug"] and given["render"] == plain["render"]
    only_loss, _, _ = run(loss_imgs=lambda i: i * 1.1 - 0.2)
    assert only_loss["base"] == given["base"] and only_loss["aug"] == plain["aug"]


def test_train_step_signature_keeps_the_old_call():
    import inspect
    from rc_mvsnet_amd import train_step as ts
    sig = inspect.signature(ts.train_step)
    assert sig.parameters["imgs_aug"].default is None and sig.parameters["loss_imgs"].default is None
    assert list(sig.parameters)[:7] == ["model", "model_nerf", "opt", "imgs", "proj", "depth_values", "batch"]


# ---------------------------------------------------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------------------------------------------------
def test_schedule_matches_the_reference_formulas():
    assert [train_driver.adjust_w_aug(e, 0.01) for e in (0, 1, 2, 3, 5, 7, 9, 14)] == [0.01, 0.02, 0.02, 0.04, 0.08, 0.16, 0.32, 0.32]
    ms, gamma = train_driver.parse_lrepochs("10,12,14:2", 100)
    assert ms == [1000, 1200, 1400] and gamma == 0.5
    lr = lambda s: train_driver.warmup_multistep_lr(1e-4, s, ms, gamma)        # noqa: E731
    assert lr(0) == pytest.approx(1e-4 / 3) and lr(250) == pytest.approx(1e-4 * (1 / 3 * 0.5 + 0.5)) and lr(500) == 1e-4
    assert lr(999) == 1e-4 and lr(1000) == 5e-5 and lr(1200) == 2.5e-5 and lr(5000) == 1.25e-5
    # torch's own scheduler base class driven by the same formula: the values the reference's subclass hands the optimizer
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-4)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: train_driver.warmup_multistep_lr(1.0, s, [4, 6], 0.5, warmup_iters=3))
    seen = []
    for _ in range(8):
        seen.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    assert seen == pytest.approx([train_driver.warmup_multistep_lr(1e-4, s, [4, 6], 0.5, warmup_iters=3) for s in range(8)])


class _Stub(torch.utils.data.Dataset):
    """six items, no files: the driver's loop only needs load_host / to_device / render_batch / set_epoch"""
    device = torch.device("cpu")

    def __init__(self):
        self.epochs = []

    def __len__(self):
        return 6

    def set_epoch(self, e):
        self.epochs.append(e)

    def load_host(self, idx):
        return idx

    def to_device(self, idx):
        z = torch.zeros(1, 3, 2, 2)
        return {"imgs": z, "imgs_aug": z + 1, "center_imgs": z + 2, "proj_matrices": {"stage1": np.zeros((1, 2, 4, 4), np.float32)},
                "depth_values": np.zeros(4, np.float32), "scan": "s%d" % idx}

    def render_batch(self, item):
        return {"imgs": item["imgs"][None]}


def _driver_args(logdir, **kw):
    args = train_driver.parser().parse_args(["--trainpath", "x", "--trainlist", "y", "--logdir", logdir, "--summary_freq", "1",
                                             "--lrepochs", "1,2:2", "--workers", "2"])
    for k, v in kw.items():
        setattr(args, k, v)
    return args


def test_driver_checkpoints_and_resume(tmp_path):
    logdir = str(tmp_path / "log")
    os.makedirs(logdir)
    calls = []

    def step(model, model_nerf, opt, w_aug, imgs, proj, depth_values, batch, imgs_aug, loss_imgs):
        assert imgs.shape == (1, 1, 3, 2, 2) and float(imgs_aug.mean()) == 1.0 and float(loss_imgs.mean()) == 2.0
        calls.append(opt.param_groups[0]["lr"])
        loss = (model.weight ** 2).sum() + (model_nerf.weight ** 2).sum()
        opt.zero_grad()
        loss.backward()
        opt.step()
        return {"loss": float(loss.detach()), "base": 0.0, "aug": w_aug, "render": 0.0}

    def fresh():
        torch.manual_seed(0)
        m, n = torch.nn.Linear(2, 2), torch.nn.Linear(2, 2)
        return m, n, torch.optim.Adam(list(m.parameters()) + list(n.parameters()), lr=1e-4)

    m, n, opt = fresh()
    ds = _Stub()
    rec = train_driver.train(_driver_args(logdir, epochs=2), ds, m, n, opt, 0, step_fn=step, out=open(os.devnull, "w"))
    assert ds.epochs == [0, 1] and [r["step"] for r in rec] == list(range(12))
    assert sorted(os.listdir(logdir)) == ["model_000000_cas.ckpt", "model_000000_nerf.ckpt", "model_000001_cas.ckpt", "model_000001_nerf.ckpt",
                                          "train_log.jsonl"]
    cas = torch.load(os.path.join(logdir, "model_000001_cas.ckpt"))
    assert sorted(cas) == ["epoch", "model", "optimizer"] and cas["epoch"] == 1
    assert sorted(torch.load(os.path.join(logdir, "model_000001_nerf.ckpt"))) == ["model"]
    assert sorted(r["scan"] for r in rec[:6]) == ["s%d" % i for i in range(6)] and [r["scan"] for r in rec[:6]] != [r["scan"] for r in rec[6:]]
    assert all(r["loader_wait_ms"] >= 0 and r["step_ms"] > 0 for r in rec)
    assert rec[0]["aug"] == 0.01 and rec[6]["aug"] == 0.02                         # adjust_w_aug from the second epoch on
    full_lrs = list(calls)
    # resume from the first epoch's checkpoint into fresh objects: the second epoch repeats step for step
    os.remove(os.path.join(logdir, "model_000001_cas.ckpt"))
    os.remove(os.path.join(logdir, "model_000001_nerf.ckpt"))
    m2, n2, opt2 = fresh()
    start = train_driver.load_checkpoint(*train_driver.latest_checkpoint(logdir), m2, n2, opt2)
    assert start == 1
    del calls[:]
    ds2 = _Stub()
    rec2 = train_driver.train(_driver_args(logdir, epochs=2), ds2, m2, n2, opt2, start, step_fn=step, out=open(os.devnull, "w"))
    assert ds2.epochs == [1] and [r["step"] for r in rec2] == list(range(6, 12)) and calls == full_lrs[6:]
    assert [(r["scan"], r["loss"], r["lr"]) for r in rec2] == [(r["scan"], r["loss"], r["lr"]) for r in rec[6:]]
    assert torch.equal(m2.weight, m.weight) and torch.equal(n2.weight, n.weight)
    lines = [json.loads(x) for x in open(os.path.join(logdir, "train_log.jsonl"))]
    assert len(lines) == 18 and set(lines[0]) >= {"epoch", "step", "lr", "loss", "base", "aug", "render", "step_ms", "loader_wait_ms"}
