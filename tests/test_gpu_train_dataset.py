"""GPU: the training loader -- the image preparation kernels (csrc/train_aug.hip) against the Pillow / torch oracle at full
size, loader items against the reference's recorded items, and real training steps through train_driver on a DTU-layout folder."""
import json
import os

import numpy as np
import pytest
import torch

import train_dataset_oracle as O
from rc_mvsnet_amd import _lib, mvs_dataset, synthetic, train_driver
from test_train_aug_cpu import check_against_oracle
from test_train_dataset_cpu import GOLD, NVIEWS, check_item_and_images_against_golden, golden_aug

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dtu_train"))
    lst = synthetic.write_dtu_train_folder(d, [str(s) for s in GOLD["scans"]], int(GOLD["n_views_folder"]), int(GOLD["seed"]))
    return d, lst


def _aug(orders, factors, gammas):
    return {"order": np.array(orders, np.int32), "factors": np.array(factors, np.float32), "gamma": np.array(gammas, np.float64)}


PARAMETER_SETS = [
    # contrast first, contrast last, hue +0.5 / -0.5 / 0, factors at the ends of their ranges
    _aug([(1, 0, 2, 3), (0, 2, 3, 1), (3, 1, 0, 2), (2, 3, 1, 0)],
         [(0.7, 1.6, 1.2, 0.5), (1.8, 0.3, 0.6, -0.5), (1.0, 1.0, 1.0, 0.0), (2.0, 2.0, 1.5, 0.31)], [0.5, 2.0, 1.0, 1.37]),
    _aug([(0, 1, 2, 3), (3, 2, 1, 0), (1, 3, 2, 0), (2, 0, 3, 1)],
         [(0.0, 1.0, 0.5, -0.2), (1.3, 0.0, 1.5, 0.07), (0.45, 1.99, 0.9, -0.49), (1.1, 0.8, 1.0, 0.25)], [0.73, 1.9, 0.51, 1.0]),
]


@pytest.mark.parametrize("case", [0, 1, "drawn"])
def test_full_size_against_oracle(case):
    _lib.load()
    rng = np.random.default_rng(11)
    raw = rng.integers(0, 256, (4, 512, 640, 3), dtype=np.uint8)
    raw[1] = (raw[1] // 3 + 60)                                            # a low-contrast view
    aug = mvs_dataset.draw_aug(torch.Generator().manual_seed(2), 4) if case == "drawn" else PARAMETER_SETS[case]
    out = mvs_dataset.prepare_train_images(raw, aug, DEV, return_u8=True)
    # atol 1e-6: the tables hold torch's own values; the freedom left is torch's vector-lane vs scalar pow (<= 1 ulp of a value
    # <= 1, 6e-8) divided by std >= 0.224, plus one rounding at |x| <= 2.7
    check_against_oracle(raw, aug, out, atol=1e-6)


def test_odd_size_and_constant_image():
    _lib.load()
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 256, (3, 77, 101, 3), dtype=np.uint8)
    raw[2] = 113                                                            # constant: variance 0 -> zeros, not NaN
    aug = _aug([(2, 1, 3, 0), (3, 0, 1, 2), (1, 2, 0, 3)], [(1.4, 0.2, 0.8, 0.5), (0.6, 1.7, 1.4, -0.5), (1.2, 0.9, 1.1, 0.0)], [0.6, 1.8, 1.1])
    out = mvs_dataset.prepare_train_images(raw, aug, DEV, return_u8=True)
    check_against_oracle(raw, aug, out, atol=1e-6)
    assert torch.equal(out["center_imgs"][2], torch.zeros(3, 77, 101, device=DEV))
    assert all(torch.isfinite(out[k]).all() for k in ("imgs", "imgs_aug", "center_imgs"))


def test_two_runs_are_bit_identical():
    _lib.load()
    raw = np.random.default_rng(8).integers(0, 256, (4, 512, 640, 3), dtype=np.uint8)
    aug = PARAMETER_SETS[0]
    a = mvs_dataset.prepare_train_images(raw, aug, DEV, return_u8=True)
    b = mvs_dataset.prepare_train_images(raw, aug, DEV, return_u8=True)
    for k in ("imgs", "imgs_aug", "center_imgs", "jitter_u8", "sums"):
        assert torch.equal(a[k], b[k]), k


def test_bad_input_is_refused():
    _lib.load()
    raw = np.zeros((1, 8, 8, 3), np.uint8)
    for aug in (_aug([(0, 1, 1, 3)], [(1, 1, 1, 0)], [1.0]), _aug([(0, 1, 2, 3)], [(1, 1, 1, 0.7)], [1.0]),
                _aug([(0, 1, 2, 3)], [(1, float("nan"), 1, 0)], [1.0]), _aug([(0, 1, 2, 3)], [(-1, 1, 1, 0)], [1.0])):
        with pytest.raises(_lib.RcmvsError):
            mvs_dataset.prepare_train_images(raw, aug, DEV)


def test_loader_items_match_reference(folder):
    _lib.load()
    d, lst = folder
    ds = mvs_dataset.DTUTrainDataset(d, lst, "train", NVIEWS, 192, 1.06, device=DEV)
    assert len(ds) == int(GOLD["len"])
    for idx in GOLD["items"]:
        host = ds.load_host(int(idx))
        host["aug"] = golden_aug(int(idx))                                  # replay the parameters the reference's run drew
        item = ds.to_device(host)
        assert item["imgs"].is_cuda and item["imgs_aug"].is_cuda and item["center_imgs"].is_cuda
        check_item_and_images_against_golden(item, int(idx), atol=1e-6)
    item = ds[3]                                                            # the loader's own draws
    assert all(torch.isfinite(item[k]).all() for k in ("imgs", "imgs_aug", "center_imgs"))
    assert not torch.equal(item["imgs"], item["imgs_aug"])


def test_prefetch_keeps_order(folder):
    _lib.load()
    d, lst = folder
    ds = mvs_dataset.DTUTrainDataset(d, lst, "train", NVIEWS, device=DEV, seed=2)
    order = [12, 5, 66, 5]
    got = list(mvs_dataset.prefetch(ds, indices=order, workers=3, depth=4))
    loader = torch.utils.data.DataLoader(torch.utils.data.Subset(ds, order), batch_size=None, num_workers=0)
    for idx, g, via_loader in zip(order, got, loader):
        want = ds[idx]
        assert g["scan"] == want["scan"] and int(g["light_id"]) == int(want["light_id"]) and np.array_equal(g["view_ids"], want["view_ids"])
        for k in ("imgs", "imgs_aug", "center_imgs"):
            assert torch.equal(g[k], want[k]) and torch.equal(via_loader[k], want[k]), k


def test_three_training_steps_through_the_driver(folder, tmp_path):
    import warnings
    from rc_mvsnet_amd import train_step as ts
    _lib.load()
    warnings.simplefilter("ignore")
    d, lst = folder
    logdir = str(tmp_path / "log")
    rec = train_driver.main(["--trainpath", d, "--trainlist", lst, "--logdir", logdir, "--epochs", "1", "--max_steps_per_epoch", "3",
                             "--summary_freq", "1", "--workers", "2"])
    assert len(rec) == 3
    for r in rec:
        assert all(np.isfinite(r[k]) for k in ("loss", "base", "aug", "render")), r
    print("driver steps:", json.dumps(rec))
    cas, nerf = train_driver.checkpoint_paths(logdir, 0)
    assert os.path.exists(cas) and os.path.exists(nerf)
    model, model_nerf, opt = ts.build(torch.device(DEV))
    assert train_driver.load_checkpoint(cas, nerf, model, model_nerf, opt) == 1          # strict=True inside
