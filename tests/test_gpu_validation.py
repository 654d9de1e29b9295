"""The validation pass on the GPU: csrc/depth_metrics.hip against the fp64 oracle (tests/validation_oracle.py) and the
reference's recorded scalars, the validation loader against the reference's recorded items (image bytes included),
``validation.validate`` over a synthetic folder with seeded weights, and one ``train_driver`` run with ``--testlist``."""
import json
import os
import zlib

import numpy as np
import pytest
import torch

import validation_oracle as O
from conftest import GOLDEN
from rc_mvsnet_amd import mvs_dataset, synthetic, train_driver, train_step, validation

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(GOLDEN, "validation.npz"))
STAGES = ("stage1", "stage2", "stage3")
DEV = "cuda:0"
SUM_RTOL = 1e-10          # a re-ordered fp64 sum of at most 327 680 exact non-negative terms: n * 2^-53 = 3.6e-11 (test_validation_emu_cpu.py)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dtu_val"))
    lst = synthetic.write_dtu_train_folder(d, [str(s) for s in GOLD["scans"]], int(GOLD["n_views_folder"]), int(GOLD["seed"]))
    return d, lst


def golden_case(name):
    return [tuple(GOLD["case:%s:%s%d" % (name, k, s)] for k in ("est", "gt", "mask")) for s in (1, 2, 3)]


def run(triples, dlossw=None, **kw):
    t = [[torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))[None].to(DEV) for a in tr] for tr in triples]
    return validation.depth_metrics({s: {"depth": t[k][0]} for k, s in enumerate(STAGES)}, {s: t[k][1] for k, s in enumerate(STAGES)},
                                    {s: t[k][2] for k, s in enumerate(STAGES)}, dlossw=dlossw, **kw)


def check_against_oracle(rec, want):
    for k in validation.COUNT_KEYS:
        print(k, rec[k], want[k])
        assert rec[k] == want[k], k
    for k in validation.SUM_KEYS + validation.SCALAR_KEYS:
        print(k, rec[k], want[k])
        if np.isnan(want[k]):
            assert np.isnan(rec[k]), k
        else:
            assert abs(rec[k] - want[k]) <= SUM_RTOL * abs(want[k]), (k, rec[k], want[k])


def random_triples(sizes, seed):
    rng = np.random.default_rng(seed)
    out = []
    for shape in sizes:
        est = (500.0 + 300.0 * rng.random(shape)).astype(np.float32)
        gt = (est + rng.choice([0.2, 1.0, 3.0, 6.0, 20.0], shape) * rng.standard_normal(shape)).astype(np.float32)
        mask = rng.choice(np.array([0.0, 0.5, 0.500001, 1.0], dtype=np.float32), shape)
        out.append((est, gt, mask))
    return out


@pytest.mark.parametrize("sizes", [[(128, 160), (256, 320), (512, 640)], [(31, 43), (63, 85), (125, 171)]])
def test_kernel_against_oracle(sizes):
    triples = random_triples(sizes, 11)
    validation.reset_workspaces()                                # so that the count below is of this test's calls
    table = torch.full((4, validation.RECORD), -1.0, dtype=torch.float64, device=DEV)
    row, img = run(triples, [0.5, 1.0, 2.0], table=table, slot=1, images=True)
    check_against_oracle(validation.record_to_dict(row), O.record(triples, [0.5, 1.0, 2.0]))
    # back to back on one stream and one workspace, no reset in between, OTHER data in between (a stale read of an earlier
    # call's partials would show): each against the oracle, the repeats of the first set with identical bits
    other = random_triples(sizes, 12)
    run(triples, [0.5, 1.0, 2.0], table=table, slot=2)
    run(other, [0.5, 1.0, 2.0], table=table, slot=0)
    run(triples, [0.5, 1.0, 2.0], table=table, slot=3)
    host = table.cpu().numpy()
    assert np.array_equal(host[1].view(np.int64), host[2].view(np.int64)) and np.array_equal(host[1].view(np.int64), host[3].view(np.int64))
    check_against_oracle(validation.record_to_dict(host[0]), O.record(other, [0.5, 1.0, 2.0]))
    assert host[0, 0] != host[1, 0] and (host[1, 28:] == 0.0).all() and len(validation._WORKSPACES) == 1
    est, gt, mask = (torch.from_numpy(a)[None] for a in triples[2])
    assert np.array_equal(img["depth_est"].cpu().numpy().view(np.int32), (est * mask).numpy().view(np.int32))
    assert np.array_equal(img["errormap"].cpu().numpy().view(np.int32), ((est - gt).abs() * mask).numpy().view(np.int32))


@pytest.mark.parametrize("name", ["mixed", "exact", "empty", "odd"])
def test_kernel_against_reference_golden(name):
    triples = golden_case(name)
    w = [float(x) for x in GOLD["dlossw"]]
    rec = validation.record_to_dict(run(triples, w))
    check_against_oracle(rec, O.record(triples, w))
    ref = GOLD["case:%s:scalars" % name]
    for i, k in enumerate(validation.SCALAR_KEYS):          # 2 x the golden's measured fp32 distance from fp64 (test_validation_cpu.py)
        assert abs(rec[k] - float(ref[i])) <= 1.9e-7 * max(abs(float(ref[i])), 1e-3), (k, rec[k], float(ref[i]))


def test_empty_mask_and_nan():
    triples = random_triples([(16, 20), (32, 40), (64, 80)], 5)
    empty = [(e, g, np.zeros_like(m)) for e, g, m in triples]
    check_against_oracle(validation.record_to_dict(run(empty)), O.record(empty))
    est = triples[2][0].copy()
    mask = triples[2][2].copy()
    est[3, 3], mask[3, 3] = np.nan, 1.0
    est[5, 5], mask[5, 5] = np.nan, 0.0
    nan = [triples[0], triples[1], (est, triples[2][1], mask)]
    check_against_oracle(validation.record_to_dict(run(nan)), O.record(nan))


def test_loader_items_match_reference(folder):
    d, lst = folder
    ds = mvs_dataset.DTUValDataset(d, lst, "test", int(GOLD["nviews"]), 192, 1.06, device=DEV)
    assert len(ds) == int(GOLD["len"])
    got = list(mvs_dataset.prefetch(ds, indices=[int(i) for i in GOLD["items"]], workers=2))
    for idx, item in zip(GOLD["items"], got):
        tag = "%d:" % idx
        imgs = item["imgs"].cpu().numpy()
        assert item["imgs"].is_cuda and imgs.dtype == np.float32 and list(imgs.shape) == list(GOLD[tag + "imgs:crc"][1:])
        assert np.array_equal(imgs[..., ::16, ::16], GOLD[tag + "imgs"])
        assert zlib.crc32(np.ascontiguousarray(imgs).tobytes()) == int(GOLD[tag + "imgs:crc"][0])      # every byte of the reference's imgs
        for s in STAGES:
            assert np.array_equal(item["proj_matrices"][s], GOLD[tag + "proj_matrices:" + s])
            assert np.array_equal(item["proj_dev"][s][0].cpu().numpy(), GOLD[tag + "proj_matrices:" + s])
            for k in ("depth", "mask"):
                crc = GOLD[tag + k + ":" + s + ":crc"]
                dev = item[k + "_dev"][s].cpu().numpy()
                assert dev.shape == (1,) + tuple(crc[1:]) and np.array_equal(dev[0], item[k][s])
                assert zlib.crc32(np.ascontiguousarray(dev).tobytes()) == int(crc[0])
        assert np.array_equal(item["depth_values_dev"][0].cpu().numpy(), GOLD[tag + "depth_values"])
    # every byte value through the conversion kernel: numpy's fp32 division, bit for bit
    raw = np.arange(256, dtype=np.uint8).repeat(3).reshape(16, 16, 3)
    conv = mvs_dataset.prepare_image(raw, (16, 16), DEV, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)).cpu().numpy()
    want = np.arange(256, dtype=np.float32).reshape(16, 16) / np.float32(255)
    assert all(np.array_equal(conv[c].view(np.int32), want.view(np.int32)) for c in range(3))


def test_validate_on_a_synthetic_folder(folder):
    """The metrics are checked on the depth the model itself produced (the oracle applied to that output), so this is about the
    metrics and the loop; one item's depth is also compared end to end with the ATen oracle at the existing depth tolerance."""
    from oracle import cascade
    d, lst = folder
    ds = mvs_dataset.DTUValDataset(d, lst, "test", 5, 192, 1.06, device=DEV)
    model, _, _ = train_step.build(torch.device(DEV), seed=0)
    model.train()
    kept = []

    def forward(m, imgs, proj, dv):
        assert not m.training and not torch.is_grad_enabled()
        outputs, _ = m(imgs, proj, dv)
        kept.append({s: outputs[s]["depth"].clone() for s in STAGES})
        return outputs

    idx = [0, 36, 69]
    w = [0.5, 1.0, 2.0]
    records, mean = validation.validate(model, ds, dlossw=w, indices=idx, workers=2, summary_freq=2, forward_fn=forward)
    assert model.training and len(records) == 3 and len(kept) == 3
    for i, rec in zip(idx, records):
        host = ds.load_host(i)
        est = kept[idx.index(i)]
        triples = [(est[s][0].cpu().numpy(), host["depth"][s], host["mask"][s]) for s in STAGES]
        check_against_oracle(rec, O.record(triples, w))
        assert rec["n_stage3"] == int((host["mask"]["stage3"] > 0.5).sum()) > 100000
        assert all(np.isfinite(rec[k]) for k in validation.SCALAR_KEYS)
    for k in validation.SCALAR_KEYS:
        assert mean[k] == sum(r[k] for r in records) / 3
    # the default forward (no hook) gives the same records: bit-identical runs
    again, _ = validation.validate(model, ds, dlossw=w, indices=idx, workers=2, summary_freq=10)
    assert [[r[k] for k in validation.SCALAR_KEYS] for r in again] == [[r[k] for k in validation.SCALAR_KEYS] for r in records]
    # end to end against the reference's op graph on the CPU (oracle impl="aten"), item 0
    item = ds[0]
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    pm = {s: torch.from_numpy(item["proj_matrices"][s])[None] for s in STAGES}
    dv = torch.from_numpy(item["depth_values"])[None]
    with torch.no_grad():
        ref = cascade.forward_eval(item["imgs"][None].cpu(), pm, dv, sd, (48, 32, 8), (4, 2, 1), impl="aten")
    rng = float(dv[0, -1] - dv[0, 0])
    err = float((kept[0]["stage3"].cpu() - ref["depth"]).abs().mean()) / rng
    print("depth L1 / range vs the ATen oracle: %.3e" % err)
    assert err < 1e-4


def test_train_driver_with_testlist(folder, tmp_path):
    d, lst = folder
    one = str(tmp_path / "val_list.txt")
    open(one, "w").write("scan2\n")
    logdir = str(tmp_path / "log")
    train_driver.main(["--trainpath", d, "--trainlist", lst, "--logdir", logdir, "--epochs", "2", "--max_steps_per_epoch", "1",
                       "--summary_freq", "2", "--testlist", one, "--max_val_items", "3", "--workers", "2", "--val-images", str(tmp_path / "img")])
    lines = [json.loads(x) for x in open(os.path.join(logdir, "train_log.jsonl"))]
    full = [x for x in lines if x.get("phase") == "fulltest"]
    assert [x["epoch"] for x in full] == [0, 1] and all(x["items"] == 3 for x in full)
    assert all(np.isfinite(x[k]) for x in full for k in validation.SCALAR_KEYS)
    assert [(x["epoch"], x["item"]) for x in lines if x.get("phase") == "test"] == [(0, 0), (0, 2), (1, 0), (1, 2)]
    assert len(os.listdir(tmp_path / "img")) == 4
    model, model_nerf, opt = train_step.build(torch.device(DEV), seed=1)
    assert train_driver.load_checkpoint(*train_driver.latest_checkpoint(logdir), model, model_nerf, opt) == 2      # loadable
    # --mode test on those weights: one pass, the same numbers as the validation after the last epoch
    out = train_driver.main(["--mode", "test", "--testpath", d, "--logdir", logdir, "--resume", "--testlist", one,
                             "--max_val_items", "3", "--workers", "2"])
    assert len(out) == 1 and out[0]["phase"] == "fulltest"
    assert [out[0][k] for k in validation.SCALAR_KEYS] == [full[1][k] for k in validation.SCALAR_KEYS]
