"""csrc/depth_metrics.hip on the CPU emulation of tests/emu, driven through rc_mvsnet_amd.validation on CPU tensors: counts equal
to the literal fp64 oracle's (tests/validation_oracle.py) exactly, fp64 sums within the bound of a re-ordered fp64 sum, the
reference's inclusive / strict comparisons at errors of exactly 2, 4 and 8 mm, empty masks, NaN, the self-resetting ticket, the
two images, and the validation loader's device half."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import validation_oracle as O
from conftest import GOLDEN, REPO
from rc_mvsnet_amd import _lib, fusion, mvs_dataset, synthetic, validation

GOLD = np.load(os.path.join(GOLDEN, "validation.npz"))
# A sum of n fp64 terms added in another order differs by at most about n * 2^-53 relative to the sum of the magnitudes; the
# terms are exact in fp64 (d is an fp32 difference, 0.5 d^2 and |d| - 0.5 lose nothing), all non-negative, and n <= 327 680
# (512 x 640): 327 680 * 2^-53 = 3.6e-11 < 1e-10.
SUM_RTOL = 1e-10


@pytest.fixture
def emu_val(emu, monkeypatch):
    monkeypatch.setattr(validation, "_chk", fusion._chk)          # the emu fixture routes fusion / ops / mvs_dataset; this module too
    monkeypatch.setattr(validation, "_stream", fusion._stream)
    monkeypatch.setattr(validation, "_WORKSPACES", {})
    return emu


def golden_case(name):
    return [tuple(GOLD["case:%s:%s%d" % (name, k, s)] for k in ("est", "gt", "mask")) for s in (1, 2, 3)]


def run(triples, dlossw=None, **kw):
    t = [[torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))[None] for a in tr] for tr in triples]
    outputs = {"stage%d" % (k + 1): {"depth": t[k][0]} for k in range(3)}
    return validation.depth_metrics(outputs, {"stage%d" % (k + 1): t[k][1] for k in range(3)},
                                    {"stage%d" % (k + 1): t[k][2] for k in range(3)}, dlossw=dlossw, **kw)


def check_against_oracle(rec, want):
    for k in validation.COUNT_KEYS:
        print(k, rec[k], want[k])
        assert rec[k] == want[k], k                                  # integers: exactly
    for k in validation.SUM_KEYS + validation.SCALAR_KEYS:
        print(k, rec[k], want[k])
        if np.isnan(want[k]):
            assert np.isnan(rec[k]), k
        else:
            assert abs(rec[k] - want[k]) <= SUM_RTOL * abs(want[k]), (k, rec[k], want[k])


def random_triples(sizes, seed, nan_at=None):
    rng = np.random.default_rng(seed)
    out = []
    for shape in sizes:
        est = (500.0 + 300.0 * rng.random(shape)).astype(np.float32)
        gt = (est + rng.choice([0.2, 1.0, 3.0, 6.0, 20.0], shape) * rng.standard_normal(shape)).astype(np.float32)
        mask = rng.choice(np.array([0.0, 0.5, 0.500001, 1.0], dtype=np.float32), shape)
        out.append((est, gt, mask))
    return out


@pytest.mark.parametrize("name", ["mixed", "exact", "empty", "odd"])
def test_golden_cases_against_oracle_and_reference(emu_val, name):
    triples = golden_case(name)
    w = [float(x) for x in GOLD["dlossw"]]
    rec = validation.record_to_dict(run(triples, w))
    check_against_oracle(rec, O.record(triples, w))
    # the reference's own fp32 scalars: within its accumulation error, measured in tests/test_validation_cpu.py
    # (test_oracle_matches_reference_golden) as the golden's distance from the fp64 oracle, 9.5e-8 relative at most, times 2
    ref = GOLD["case:%s:scalars" % name]
    for i, k in enumerate(validation.SCALAR_KEYS):
        assert abs(rec[k] - float(ref[i])) <= 1.9e-7 * max(abs(float(ref[i])), 1e-3), (k, rec[k], float(ref[i]))


def test_boundaries_are_the_references(emu_val):
    """errors of exactly 2, 4, 8: in both neighbouring bands (inclusive ends), not above the threshold (strict)"""
    est = np.full((1, 8), 650.5, dtype=np.float32)
    gt = est - np.array([[2.0, -2.0, 4.0, -4.0, 8.0, -8.0, 0.0, 1.0]], dtype=np.float32)
    assert np.array_equal(np.abs(est - gt), [[2, 2, 4, 4, 8, 8, 0, 1]])
    mask = np.ones((1, 8), dtype=np.float32)
    rec = validation.record_to_dict(run([(est, gt, mask)] * 3))
    assert (rec["count_gt2mm"], rec["count_gt4mm"], rec["count_gt8mm"]) == (4, 2, 0)
    assert (rec["band2mm_count"], rec["band4mm_count"], rec["band8mm_count"]) == (4, 4, 4)
    assert (rec["band2mm_sum"], rec["band4mm_sum"], rec["band8mm_sum"]) == (5.0, 12.0, 24.0)
    assert rec["thres2mm_error"] == 0.5 and rec["thres8mm_accu"] == 1.0 and rec["thres4mm_abserror"] == 3.0
    # smooth-L1: 0.5 d^2 below 1, |d| - 0.5 from 1 on (an error of exactly 1 gives 0.5 on either branch)
    assert rec["sl1_stage3"] == 2 * 1.5 + 2 * 3.5 + 2 * 7.5 + 0.0 + 0.5
    check_against_oracle(rec, O.record([(est, gt, mask)] * 3))
    # the mask's own threshold: 0.5 is out, the next fp32 value up is in
    mask = np.array([[0.0, 0.5, np.nextafter(np.float32(0.5), np.float32(1)), 0.500001, 1.0, 0.0, 0.0, 0.0]], dtype=np.float32)
    assert validation.record_to_dict(run([(est, gt, mask)] * 3))["n_stage3"] == 3


def test_empty_mask_and_nan(emu_val):
    triples = random_triples([(4, 5), (8, 10), (16, 20)], 1)
    empty = [(e, g, np.zeros_like(m)) for e, g, m in triples]
    rec = validation.record_to_dict(run(empty, [0.5, 1.0, 2.0]))
    want = O.record(empty, [0.5, 1.0, 2.0])
    assert all(np.isnan(want[k]) for k in validation.SCALAR_KEYS[:9]) and all(want[k] == 0.0 for k in validation.SCALAR_KEYS[9:])
    check_against_oracle(rec, want)
    # one empty stage poisons the loss only
    part = [empty[0], triples[1], triples[2]]
    rec = validation.record_to_dict(run(part))
    assert np.isnan(rec["loss"]) and np.isfinite(rec["depth_loss"]) and rec["n_stage1"] == 0
    check_against_oracle(rec, O.record(part))
    # a NaN estimate: comparisons false, sums NaN -- inside the mask only
    est = triples[2][0].copy()
    mask = triples[2][2].copy()
    est[3, 3], mask[3, 3] = np.nan, 1.0
    est[5, 5], mask[5, 5] = np.nan, 0.0
    nan = [triples[0], triples[1], (est, triples[2][1], mask)]
    rec = validation.record_to_dict(run(nan))
    want = O.record(nan)
    assert np.isnan(want["abs_depth_error"]) and np.isnan(want["loss"]) and not np.isnan(want["thres2mm_error"])
    check_against_oracle(rec, want)


@pytest.mark.parametrize("sizes", [[(128, 160), (256, 320), (512, 640)], [(31, 43), (63, 85), (125, 171)], [(1, 1), (1, 2), (1, 3)]])
def test_sizes_repeat_and_images(emu_val, sizes):
    """the validation shape, an odd one (scalar tails; more than one block per stage) and a tiny one; a second call on the same
    workspace without any reset gives the same bits (the ticket put itself back); the images are est * mask and |est - gt| * mask"""
    triples = random_triples(sizes, 7)
    table = torch.full((3, validation.RECORD), -1.0, dtype=torch.float64)
    row, img = run(triples, [0.5, 1.0, 2.0], table=table, slot=1, images=True)
    check_against_oracle(validation.record_to_dict(row), O.record(triples, [0.5, 1.0, 2.0]))
    assert torch.all(table[0] == -1.0) and torch.all(table[2] == -1.0) and torch.all(table[1, 28:] == 0.0)
    again = run(triples, [0.5, 1.0, 2.0], table=table, slot=2)
    assert np.array_equal(table[1].numpy().view(np.int64), again.numpy().view(np.int64))
    assert len(validation._WORKSPACES) == 1
    est, gt, mask = (torch.from_numpy(a)[None] for a in triples[2])
    assert np.array_equal(img["depth_est"].numpy().view(np.int32), (est * mask).numpy().view(np.int32))
    assert np.array_equal(img["errormap"].numpy().view(np.int32), ((est - gt).abs() * mask).numpy().view(np.int32))


def test_unaligned_planes_take_the_scalar_path(emu_val):
    triples = random_triples([(5, 7), (9, 11), (17, 23)], 3)
    want = O.record(triples)
    t = []
    for tr in triples:
        t.append([torch.from_numpy(np.concatenate([np.zeros(1, np.float32), a.ravel()]))[1:].view(1, *a.shape) for a in tr])   # 4 bytes off
    assert all(x.data_ptr() % 16 != 0 for x in t[2])
    row = validation.depth_metrics({"stage%d" % (k + 1): {"depth": t[k][0]} for k in range(3)}, {"stage%d" % (k + 1): t[k][1] for k in range(3)},
                                   {"stage%d" % (k + 1): t[k][2] for k in range(3)})
    check_against_oracle(validation.record_to_dict(row), want)


def test_reference_names(emu_val):
    triples = golden_case("mixed")
    t = [[torch.from_numpy(a)[None] for a in tr] for tr in triples]
    outputs = {"stage%d" % (k + 1): {"depth": t[k][0]} for k in range(3)}
    gt_ms, mask_ms = {"stage%d" % (k + 1): t[k][1] for k in range(3)}, {"stage%d" % (k + 1): t[k][2] for k in range(3)}
    want = O.record(triples, [0.5, 1.0, 2.0])
    loss, depth_loss = validation.cas_mvsnet_loss(outputs, gt_ms, mask_ms, dlossw=[0.5, 1.0, 2.0])
    assert loss.dim() == 0 and loss.dtype == torch.float32 and float(loss) == np.float32(want["loss"]) and float(depth_loss) == np.float32(want["depth_loss"])
    assert float(validation.cas_mvsnet_loss(outputs, gt_ms, mask_ms)[0]) == np.float32(O.record(triples)["loss"])
    est, gt, mask = t[2]
    for thres, band in ((2, [0, 2.0]), (4, [2.0, 4.0]), (8, [4.0, 8.0])):
        v = validation.Thres_metrics(est, gt, mask > 0.5, thres)
        assert v.dim() == 0 and float(v) == np.float32(want["thres%dmm_error" % thres])
        assert float(validation.AbsDepthError_metrics(est, gt, mask > 0.5, band)) == np.float32(want["thres%dmm_abserror" % thres])
    assert float(validation.AbsDepthError_metrics(est, gt, mask > 0.5)) == np.float32(want["abs_depth_error"])
    assert len(validation._WORKSPACES) == 1                      # cas_mvsnet_loss's; the per-plane wrappers keep none
    with pytest.raises(_lib.RcmvsError, match="not one of"):
        validation.Thres_metrics(est, gt, mask > 0.5, 3)
    with pytest.raises(_lib.RcmvsError, match="not one of"):
        validation.AbsDepthError_metrics(est, gt, mask > 0.5, [8.0, 14.0])


def test_refusals(emu_val):
    triples = random_triples([(4, 5), (8, 10), (16, 20)], 2)
    two = [tuple(np.stack([a, a]) for a in tr) for tr in triples]
    t = [[torch.from_numpy(a) for a in tr] for tr in two]
    with pytest.raises(_lib.RcmvsError, match="batch 1"):
        validation.depth_metrics({"stage%d" % (k + 1): {"depth": t[k][0]} for k in range(3)}, {"stage%d" % (k + 1): t[k][1] for k in range(3)},
                                 {"stage%d" % (k + 1): t[k][2] for k in range(3)})
    with pytest.raises(_lib.RcmvsError, match="row 4"):
        run(triples, table=torch.zeros((4, validation.RECORD), dtype=torch.float64), slot=4)
    with pytest.raises(_lib.RcmvsError, match="differ"):
        run([triples[0], triples[1], (triples[2][0], triples[2][1], triples[1][2])])
    with pytest.raises(_lib.RcmvsError, match="one weight per stage"):
        run(triples, [1.0, 2.0])


def test_workspace_is_dropped_after_a_failed_call_and_reset_per_pass(emu_val, monkeypatch):
    """a workspace whose ticket may be part-drawn is never reused: a failing call forgets it, reset_workspaces forgets all,
    the cache does not grow past MAX_WORKSPACES, and a poisoned ticket is gone after the reset"""
    triples = random_triples([(4, 5), (8, 10), (16, 20)], 2)
    want = O.record(triples)
    check_against_oracle(validation.record_to_dict(run(triples)), want)
    (key, ws), = validation._WORKSPACES.items()
    assert ws.data_ptr() % 128 == 0
    real = emu_val.rcmvs_depth_metrics
    monkeypatch.setattr(validation._lib, "_lib", type("L", (), {"__getattr__": lambda self, n: (lambda *a: 7) if n == "rcmvs_depth_metrics" else getattr(emu_val, n)})())
    with pytest.raises(_lib.RcmvsError):
        run(triples)
    assert key not in validation._WORKSPACES
    monkeypatch.setattr(validation._lib, "_lib", emu_val)
    assert real is emu_val.rcmvs_depth_metrics
    run(triples)
    validation._WORKSPACES[key][:4] = torch.tensor([1, 0, 0, 0], dtype=torch.uint8)      # a ticket left part-drawn by a lost launch
    table = torch.full((1, validation.RECORD), -1.0, dtype=torch.float64)
    other = random_triples([(4, 5), (8, 10), (16, 20)], 9)
    run(other, table=table)
    assert validation.record_to_dict(table[0])["sl1_stage3"] != O.record(other)["sl1_stage3"]   # the hazard: a block that is not the last one adds up
    validation.reset_workspaces()
    check_against_oracle(validation.record_to_dict(run(triples, table=table)), want)
    for k in range(validation.MAX_WORKSPACES + 3):
        run(random_triples([(1, 1 + k), (1, 2), (1, 3)], k))
    assert len(validation._WORKSPACES) <= validation.MAX_WORKSPACES


def test_cpu_tensors_raise_without_the_emulation():
    triples = random_triples([(4, 5), (8, 10), (16, 20)], 2)
    with pytest.raises(_lib.RcmvsError):
        run(triples)


def test_symbols_are_exported():
    import ctypes
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("rcmvs_depth_metrics", "rcmvs_depth_metrics_timed", "rcmvs_depth_metrics_workspace_bytes"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    fn = lib.rcmvs_depth_metrics_workspace_bytes
    fn.argtypes, fn.restype = [ctypes.c_longlong] * 3, ctypes.c_longlong
    assert fn(128 * 160, 256 * 320, 512 * 640) == 128 + 105 * 128 and fn(1, 1, 1) == 128 + 3 * 128 and fn(0, 1, 1) < 0
    one = ctypes.c_void_p(16)
    assert lib.rcmvs_depth_metrics(None, one, one, ctypes.c_longlong(4), one, one, one, ctypes.c_longlong(4), one, one, one, ctypes.c_longlong(4),
                                   None, one, 0, None, None, one, None) < 0


@pytest.mark.parametrize("order", ["1", "2"])
def test_other_thread_orders_give_the_same_bits(order, tmp_path):
    """RCMVS_EMU_ORDER=1|2 schedules every block's threads in another order between synchronisation points: a missing barrier
    would change the record.  Run in a child process (the order is read when the library is loaded)."""
    script = tmp_path / "run.py"
    script.write_text(
        "import sys, os\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np, torch, conftest\n"
        "from rc_mvsnet_amd import validation, fusion\n"
        "lib = conftest.load_emu_lib()\n"
        "conftest.route_to_emulation(lib, setattr)\n"
        "validation._chk, validation._stream = fusion._chk, fusion._stream\n"
        "import test_validation_emu_cpu as T\n"
        "tr = T.random_triples([(31, 43), (63, 85), (125, 171)], 7)\n"
        "a = T.run(tr, [0.5, 1.0, 2.0]).numpy().copy()\n"
        "b = T.run(tr, [0.5, 1.0, 2.0]).numpy().copy()\n"
        "assert np.array_equal(a.view(np.int64), b.view(np.int64))\n"
        "sys.stdout.write(a.tobytes().hex())\n" % (REPO, os.path.join(REPO, "tests")))
    outs = []
    for o in ("0", order):
        env = dict(os.environ, RCMVS_EMU_ORDER=o)
        outs.append(subprocess.run([sys.executable, str(script)], env=env, check=True, capture_output=True, text=True).stdout)
    assert len(outs[0]) == 2 * 8 * validation.RECORD and outs[0] == outs[1]


# ------------------------------------------------------------------------------------------------------- the loader on the emulation
@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dtu_val"))
    lst = synthetic.write_dtu_train_folder(d, [str(s) for s in GOLD["scans"]], int(GOLD["n_views_folder"]), int(GOLD["seed"]))
    return d, lst


def test_prepare_image_is_the_fp32_division_for_every_byte(emu_val):
    """equal sizes, mean 0, std 1: rcmvs_prepare_image gives float(b) / 255.0f, what numpy's fp32 division gives, bit for bit"""
    raw = np.arange(256, dtype=np.uint8).repeat(3).reshape(16, 16, 3)
    got = mvs_dataset.prepare_image(raw, (16, 16), "cpu", mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)).numpy()
    want = np.arange(256, dtype=np.float32).reshape(16, 16) / np.float32(255)
    for c in range(3):
        assert np.array_equal(got[c].view(np.int32), want.view(np.int32))


def test_items_on_emulation_match_reference(emu_val, folder):
    d, lst = folder
    ds = mvs_dataset.DTUValDataset(d, lst, "test", int(GOLD["nviews"]), 192, 1.06, device="cpu")
    assert len(ds) == int(GOLD["len"])
    for idx in GOLD["items"]:
        item = ds[int(idx)]
        tag = "%d:" % idx
        imgs = item["imgs"].numpy()
        assert imgs.dtype == np.float32 and list(imgs.shape) == list(GOLD[tag + "imgs:crc"][1:])
        assert np.array_equal(imgs[..., ::16, ::16], GOLD[tag + "imgs"])
        assert zlib.crc32(np.ascontiguousarray(imgs).tobytes()) == int(GOLD[tag + "imgs:crc"][0])       # every byte of the reference's imgs
        for s in ("stage1", "stage2", "stage3"):
            assert np.array_equal(item["proj_dev"][s][0].numpy(), GOLD[tag + "proj_matrices:" + s])
            for k in ("depth", "mask"):
                dev = item[k + "_dev"][s]
                assert dev.shape == (1,) + item[k][s].shape and np.array_equal(dev[0].numpy(), item[k][s])
        assert np.array_equal(item["depth_values_dev"][0].numpy(), GOLD[tag + "depth_values"])
