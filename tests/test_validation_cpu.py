"""The validation pass without a GPU: the fp64 oracle against the reference's recorded scalars, the validation loader's host
half against the reference's recorded items, ``validation.validate`` (stand-in forward, metrics on the emulated kernel) and the
driver's scheduling, logging and refusals."""
import json
import os
import zlib

import numpy as np
import pytest
import torch

import validation_oracle as O
from conftest import GOLDEN
from rc_mvsnet_amd import _lib, fusion, mvs_dataset, synthetic, train_driver, validation

GOLD = np.load(os.path.join(GOLDEN, "validation.npz"))
STAGES = ("stage1", "stage2", "stage3")


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dtu_val"))
    lst = synthetic.write_dtu_train_folder(d, [str(s) for s in GOLD["scans"]], int(GOLD["n_views_folder"]), int(GOLD["seed"]))
    return d, lst


@pytest.fixture
def emu_val(emu, monkeypatch):
    monkeypatch.setattr(validation, "_chk", fusion._chk)
    monkeypatch.setattr(validation, "_stream", fusion._stream)
    monkeypatch.setattr(validation, "_WORKSPACES", {})
    return emu


def golden_case(name):
    return [tuple(GOLD["case:%s:%s%d" % (name, k, s)] for k in ("est", "gt", "mask")) for s in (1, 2, 3)]


def test_keys_are_the_references():
    assert tuple(str(k) for k in GOLD["scalar_keys"]) == validation.SCALAR_KEYS == O.SCALAR_KEYS
    assert validation.RECORD >= len(validation.SCALAR_KEYS) + len(validation.SUM_KEYS) + len(validation.COUNT_KEYS)


def test_oracle_matches_reference_golden():
    """The reference accumulates in fp32, the oracle in fp64.  Their distance on the golden's triples, no code under test
    involved, was measured at 9.5e-8 of the value at most (generator run: worst case 9.504e-08); the allowance is twice that."""
    worst = 0.0
    for name in GOLD["cases"]:
        want = O.record(golden_case(str(name)), list(GOLD["dlossw"]))
        ref = GOLD["case:%s:scalars" % name]
        for i, k in enumerate(O.SCALAR_KEYS):
            r = abs(want[k] - float(ref[i])) / max(abs(float(ref[i])), 1e-3)
            worst = max(worst, r)
            assert r <= 1.9e-7, (name, k, want[k], float(ref[i]))       # 2 x 9.5e-8 measured
    print("worst relative distance of the golden from the fp64 oracle: %.3e" % worst)


def test_golden_cases_hit_every_branch():
    """by the data alone: errors on both sides of 1 mm, exactly 2 / 4 / 8, an empty band, a size that is not a multiple of 4,
    the four mask values"""
    est, gt, mask = golden_case("exact")[2]
    e = np.abs(est - gt)[mask > 0.5]
    assert all((e == t).any() for t in (0.0, 1.0, 2.0, 4.0, 8.0)) and (e < 1).any() and (e > 1).any()
    ref = dict(zip(O.SCALAR_KEYS, GOLD["case:empty:scalars"]))
    assert ref["thres4mm_abserror"] == 0.0 and ref["thres8mm_abserror"] == 0.0 and ref["thres2mm_abserror"] > 0.0
    assert all(golden_case("odd")[k][0].size % 4 != 0 for k in range(3))
    for name in GOLD["cases"]:
        for _, _, m in golden_case(str(name)):
            assert set(np.unique(m)) == {np.float32(0.0), np.float32(0.5), np.float32(0.500001), np.float32(1.0)}
    # the inclusive ends matter in the recorded numbers: counting an error of exactly 2 in one band only would move them
    w = O.record(golden_case("exact"))
    assert w["band2mm_count"] + w["band4mm_count"] + w["band8mm_count"] > int(((e >= 0) & (e <= 8)).sum())


def test_host_half_matches_reference(folder):
    d, lst = folder
    ds = mvs_dataset.DTUValDataset(d, lst, "test", int(GOLD["nviews"]), 192, 1.06, device="cpu")
    assert len(ds) == int(GOLD["len"]) == 2 * 5 * 7
    for idx in GOLD["items"]:
        host = ds.load_host(int(idx))
        tag = "%d:" % idx
        for s in STAGES:
            assert np.array_equal(host["proj_matrices"][s], GOLD[tag + "proj_matrices:" + s]) and host["proj_matrices"][s].dtype == np.float32
            for k in ("depth", "mask"):
                v, crc = host[k][s], GOLD[tag + k + ":" + s + ":crc"]
                assert v.dtype == np.float32 and list(v.shape) == list(crc[1:])
                assert np.array_equal(v[::8, ::8], GOLD[tag + k + ":" + s])
                assert zlib.crc32(np.ascontiguousarray(v).tobytes()) == int(crc[0]), (k, s)
        assert np.array_equal(host["depth_values"], GOLD[tag + "depth_values"]) and host["depth_values"].dtype == np.float32
        raw = host["raw"].numpy()
        assert raw.dtype == np.uint8 and raw.shape == (5, 512, 640, 3)
        want = raw.astype(np.float32) / np.float32(255)                                   # read_img: bytes / 255 in fp32, nothing else
        assert np.array_equal(want.transpose(0, 3, 1, 2)[..., ::16, ::16], GOLD[tag + "imgs"])
        assert zlib.crc32(np.ascontiguousarray(want.transpose(0, 3, 1, 2)).tobytes()) == int(GOLD[tag + "imgs:crc"][0])
    scan, light, ref, srcs = ds.metas[int(GOLD["items"][1])]
    assert (scan, light, ref) == ("scan2", 6, 4) and list(ds.load_host(int(GOLD["items"][1]))["view_ids"]) == [ref] + srcs[:4]


def test_loader_fails_loudly_without_a_gpu(folder):
    d, lst = folder
    ds = mvs_dataset.DTUValDataset(d, lst, "test", 5, device="cpu")
    with pytest.raises(_lib.RcmvsError):
        ds[0]
    with pytest.raises(ValueError):
        mvs_dataset.DTUValDataset(d, lst, "eval", 5, device="cpu")


# ---------------------------------------------------------------------------------------------------------------- validate()
class _ValStub:
    """items whose estimate, ground truth and mask are seeded arrays; the 'forward' hands the estimate through"""
    device = torch.device("cpu")

    def __init__(self, n=5):
        self.n = n
        self.loaded = []

    def __len__(self):
        return self.n

    def triples(self, idx):
        rng = np.random.default_rng(100 + idx)
        out = []
        for shape in ((4, 6), (8, 12), (16, 24)):
            est = (600.0 + 50.0 * rng.random(shape)).astype(np.float32)
            gt = (est + (1.0 + 2.0 * idx) * rng.standard_normal(shape)).astype(np.float32)
            mask = (rng.random(shape) < 0.3 + 0.1 * idx).astype(np.float32)              # masks of different sizes: pooled != mean of items
            out.append((est, gt, mask))
        return out

    def load_host(self, idx):
        self.loaded.append(idx)
        return idx

    def to_device(self, idx):
        t = self.triples(idx)
        return {"imgs": torch.zeros(1, 3, 2, 2), "proj_dev": {}, "depth_values_dev": torch.zeros(1, 4), "idx": idx,
                "est": {s: torch.from_numpy(t[k][0])[None] for k, s in enumerate(STAGES)},
                "depth_dev": {s: torch.from_numpy(t[k][1])[None] for k, s in enumerate(STAGES)},
                "mask_dev": {s: torch.from_numpy(t[k][2])[None] for k, s in enumerate(STAGES)}}


def _stub_forward(ds):
    seen = []

    def forward(model, imgs, proj, depth_values):
        assert not model.training and not torch.is_grad_enabled()
        idx = len(seen)
        seen.append(idx)
        t = ds.triples(forward.order[idx])
        return {s: {"depth": torch.from_numpy(t[k][0])[None]} for k, s in enumerate(STAGES)}
    forward.order = list(range(len(ds)))
    forward.seen = seen
    return forward


def test_validate_mean_of_items_and_flag(emu_val, tmp_path):
    ds = _ValStub(5)
    model = torch.nn.Linear(2, 2)
    model.train()
    fwd = _stub_forward(ds)
    summaries = []
    stats = {}
    records, mean = validation.validate(model, ds, dlossw=[0.5, 1.0, 2.0], workers=2, summary_freq=2, forward_fn=fwd,
                                        on_summary=lambda i, r: summaries.append((i, r["loss"])), image_dir=str(tmp_path / "img"), stats=stats)
    assert model.training                                                # restored
    assert len(records) == 5 and fwd.seen == [0, 1, 2, 3, 4] and stats["items"] == 5 and stats["loader_wait_s"] >= 0
    want = [O.record(ds.triples(i), [0.5, 1.0, 2.0]) for i in range(5)]
    for r, w in zip(records, want):
        for k in validation.COUNT_KEYS:
            assert r[k] == w[k]
        for k in validation.SCALAR_KEYS:
            assert abs(r[k] - w[k]) <= 1e-10 * abs(w[k])
    assert [i for i, _ in summaries] == [0, 2, 4] and [v for _, v in summaries] == [records[i]["loss"] for i in (0, 2, 4)]
    # DictAverageMeter's mean: over items of the per-item values ...
    for k in validation.SCALAR_KEYS:
        assert mean[k] == sum(r[k] for r in records) / 5
    # ... which is not the pooled mean over pixels
    pooled = sum(r["sum_abs_error"] for r in records) / sum(r["n_stage3"] for r in records)
    assert abs(pooled - mean["abs_depth_error"]) > 1e-3 * pooled
    assert sorted(os.listdir(tmp_path / "img")) == sorted("%06d_%s.pfm" % (i, n) for i in (0, 2, 4) for n in ("depth_est", "errormap"))
    from rc_mvsnet_amd.data_io import read_pfm
    t = ds.triples(2)[2]
    assert np.array_equal(read_pfm(str(tmp_path / "img" / "000002_errormap.pfm"))[0], np.abs(t[0] - t[1]) * t[2])
    # eval-mode module stays in eval mode; a subset in another order; an exception restores the flag too
    model.eval()
    fwd = _stub_forward(ds)
    fwd.order = [3, 1]
    rec2, _ = validation.validate(model, ds, dlossw=[0.5, 1.0, 2.0], indices=[3, 1], workers=1, summary_freq=10, forward_fn=fwd)
    assert not model.training and [r["loss"] for r in rec2] == [records[3]["loss"], records[1]["loss"]]
    model.train()

    def boom(*a):
        raise RuntimeError("boom")
    with pytest.raises(RuntimeError, match="boom"):
        validation.validate(model, ds, forward_fn=boom, workers=1)
    assert model.training
    assert validation.validate(model, ds, indices=[], forward_fn=boom) == ([], {})


# ------------------------------------------------------------------------------------------------------------------ the driver
class _TrainStub:
    device = torch.device("cpu")

    def __len__(self):
        return 3

    def set_epoch(self, e):
        pass

    def load_host(self, idx):
        return idx

    def to_device(self, idx):
        z = torch.zeros(1, 3, 2, 2)
        return {"imgs": z, "imgs_aug": z, "center_imgs": z, "proj_matrices": {"stage1": np.zeros((1, 2, 4, 4), np.float32)},
                "depth_values": np.zeros(4, np.float32), "scan": "s%d" % idx}

    def render_batch(self, item):
        return {"imgs": item["imgs"][None]}


def _args(logdir, *extra, **kw):
    args = train_driver.parser().parse_args(["--trainpath", "x", "--trainlist", "y", "--logdir", logdir, "--summary_freq", "2",
                                             "--lrepochs", "1,2:2", "--workers", "1"] + list(extra))
    for k, v in kw.items():
        setattr(args, k, v)
    return args


def _step(model, model_nerf, opt, w_aug, **kw):
    return {"loss": 1.0, "base": 0.0, "aug": w_aug, "render": 0.0}


def _fresh():
    torch.manual_seed(0)
    m, n = torch.nn.Linear(2, 2), torch.nn.Linear(2, 2)
    return m, n, torch.optim.Adam(list(m.parameters()) + list(n.parameters()), lr=1e-4)


def test_driver_defaults_are_the_references():
    a = train_driver.parser().parse_args(["--trainpath", "x", "--trainlist", "y", "--logdir", "z"])
    assert (a.mode, a.testpath, a.testlist, a.eval_freq, a.dlossw, a.val_num_view) == ("train", None, None, 1, "0.5,1.0,2.0", 5)


def test_driver_schedules_validation(emu_val, tmp_path):
    ds_val = _ValStub(3)
    fwd = _stub_forward(ds_val)
    passes = []

    def validate_fn(model, dataset, **kw):
        del fwd.seen[:]
        passes.append((len(os.listdir(logdir)), kw["dlossw"], list(kw["indices"])))      # the epoch's checkpoint is already there
        return validation.validate(model, dataset, forward_fn=fwd, **kw)

    logdir = str(tmp_path / "log")
    os.makedirs(logdir)
    m, n, opt = _fresh()
    sink = open(os.devnull, "w")
    rec = train_driver.train(_args(logdir, epochs=4, eval_freq=3), _TrainStub(), m, n, opt, 0, step_fn=_step, out=sink,
                             val_dataset=ds_val, validate_fn=validate_fn)
    lines = [json.loads(x) for x in open(os.path.join(logdir, "train_log.jsonl"))]
    full = [x for x in lines if x.get("phase") == "fulltest"]
    test = [x for x in lines if x.get("phase") == "test"]
    assert [x["epoch"] for x in full] == [0, 3]                          # epoch % eval_freq == 0, and the last epoch
    assert [(x["epoch"], x["item"]) for x in test] == [(0, 0), (0, 2), (3, 0), (3, 2)]
    assert [p[0] for p in passes] == [3, 9] and passes[0][1] == [0.5, 1.0, 2.0] and passes[0][2] == [0, 1, 2]
    want = [O.record(ds_val.triples(i), [0.5, 1.0, 2.0]) for i in range(3)]
    for k in validation.SCALAR_KEYS:
        assert abs(full[0][k] - sum(w[k] for w in want) / 3) <= 1e-10 * abs(full[0][k]) and np.isfinite(full[0][k])
        assert full[0][k] == full[1][k]
    assert set(validation.SCALAR_KEYS) <= set(test[0]) and full[0]["items"] == 3
    # without a validation set: the same training records, no test lines
    logdir2 = str(tmp_path / "log2")
    os.makedirs(logdir2)
    m2, n2, opt2 = _fresh()
    rec2 = train_driver.train(_args(logdir2, epochs=4), _TrainStub(), m2, n2, opt2, 0, step_fn=_step, out=sink)
    strip = lambda rs: [{k: v for k, v in r.items() if k not in ("step_ms", "loader_wait_ms")} for r in rs]     # noqa: E731
    assert strip(rec) == strip(rec2)
    lines2 = [json.loads(x) for x in open(os.path.join(logdir2, "train_log.jsonl"))]
    assert all("phase" not in x for x in lines2) and strip(lines2) == strip([x for x in lines if "phase" not in x])


def test_mode_test_needs_weights_and_a_list(tmp_path):
    logdir = str(tmp_path / "log")
    os.makedirs(logdir)
    base = ["--trainpath", "x", "--trainlist", "y", "--logdir", logdir]
    with pytest.raises(SystemExit, match="loadckpt"):
        train_driver.main(base + ["--mode", "test", "--testlist", "z"])
    with pytest.raises(SystemExit, match="loadckpt"):
        train_driver.main(base + ["--mode", "test", "--testlist", "z", "--resume"])       # nothing to resume from
    with pytest.raises(SystemExit, match="testlist"):
        train_driver.main(base + ["--mode", "test", "--loadckpt", "c"])
    train_driver.check_mode(_args(logdir, "--mode", "test", "--testlist", "z", "--loadckpt", "c"), False)
    train_driver.check_mode(_args(logdir, "--mode", "test", "--testlist", "z", "--resume"), True)
    train_driver.check_mode(_args(logdir), False)
    # the test mode needs no training folder; the train mode does
    only = ["--logdir", logdir, "--mode", "test", "--testlist", "z", "--loadckpt", "c"]
    train_driver.check_mode(train_driver.parser().parse_args(only + ["--testpath", "t"]), False)
    with pytest.raises(SystemExit, match="testpath"):
        train_driver.check_mode(train_driver.parser().parse_args(only), False)
    with pytest.raises(SystemExit, match="trainpath"):
        train_driver.main(["--logdir", logdir, "--trainlist", "y"])
