"""csrc/depth_colormap.hip on the CPU emulation of tests/emu, driven through rc_mvsnet_amd.depth_vis on CPU tensors: every case of
tests/golden/tanks_eval.npz (recorded from the reference's write_depth_img_2) equal in every byte, vmin / vmax bit-equal; the
selection alone against np.sort on 200 seeded sizes with heavy ties, negative values and both zeros; two runs identical; another
thread order gives the same bytes.  The 1056 x 1920 case runs with RCMVS_EMU_FULL=1 (minutes on the emulation; the GPU suite
always runs it)."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO
from rc_mvsnet_amd import _lib, depth_vis, fusion, synthetic

GOLD = np.load(os.path.join(GOLDEN, "tanks_eval.npz"))
CASES = [str(c) for c in GOLD["cases"]]


@pytest.fixture
def emu_vis(emu, monkeypatch):
    monkeypatch.setattr(depth_vis, "_chk", fusion._chk)            # the emu fixture routes fusion / ops / mvs_dataset; this module too
    monkeypatch.setattr(depth_vis, "_stream", fusion._stream)
    monkeypatch.setattr(depth_vis, "_DEVICE", {})
    return emu


def colour(depth, **kw):
    rgb, vm = depth_vis.depth_colormap(torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32)), **kw)
    return rgb.numpy(), vm.numpy()


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.int32), np.asarray(b, dtype=np.float32).view(np.int32))


def numpy_percentile_fp32(values, percentile):
    """numpy's linear percentile of fp32 values with the virtual index in fp32 (what numpy 2.x computes for an fp32 array),
    from a full sort: the brute force the selection is checked against."""
    s = np.sort(values.ravel())
    n = s.size
    v = np.float32(n - 1) * (np.float32(percentile) / np.float32(100))
    lo = min(int(np.floor(v)), n - 1)
    hi = min(lo + 1, n - 1)
    g = np.float32(v - np.floor(v))
    a, b = s[lo], s[hi]
    d = np.float32(b - a)
    return np.float32(a + np.float32(d * g)) if g < 0.5 else np.float32(b - np.float32(d * np.float32(np.float32(1) - g)))


def test_fixture_records_its_versions():
    assert str(GOLD["numpy_version"]) and str(GOLD["matplotlib_version"]) and float(GOLD["percentile"]) == 95.0
    assert {"ramp", "outliers", "r33x47", "r1x7", "r5x1", "constant", "ties", "int21", "frac42", "narrow", "nan", "wide"} <= set(CASES)
    assert all(str(GOLD["case:%s:outcome" % c]) == "image" for c in CASES)          # the reference raises for none of them, the NaN map included


@pytest.mark.parametrize("name", CASES)
def test_golden_cases_equal_the_reference_in_every_byte(emu_vis, name):
    depth, want, vm = GOLD["case:%s:depth" % name], GOLD["case:%s:image" % name], GOLD["case:%s:vminmax" % name]
    rgb, got = colour(depth)
    print(name, depth.shape, "vmin/vmax", got, "reference", vm, "differing bytes", int((rgb != want).sum()))
    assert rgb.dtype == np.uint8 and rgb.shape == want.shape
    if name == "nan":
        assert np.isnan(got).all() and np.isnan(vm).all()
    else:
        assert same_bits(got, vm)
    assert np.array_equal(rgb, want)


def test_golden_holds_what_the_cases_promise():
    """the fixture's own claims: ties across the selected rank, an integer and a fractional virtual index, and a case that tells
    the fp32 arithmetic from an fp64 one"""
    t = np.sort(GOLD["case:ties:depth"].ravel())
    vmax = GOLD["case:ties:vminmax"][1]
    assert (t == vmax).sum() > 100 and t[1899] == vmax == t[1900]
    assert np.float32(20) * (np.float32(95) / np.float32(100)) == 19.0
    assert np.float32(41) * (np.float32(95) / np.float32(100)) != np.floor(np.float32(41) * (np.float32(95) / np.float32(100)))
    # An all-fp32 and an all-fp64 Normalize pick different table entries on the wide case, so the golden can tell the forms apart.
    # The reference's image there is neither: matplotlib rounds d - vmin to fp32 and divides in fp64 (csrc/depth_colormap_math.h),
    # which test_golden_cases_equal_the_reference_in_every_byte[wide] pins.
    d, (vmin, vmax) = GOLD["case:wide:depth"], GOLD["case:wide:vminmax"]
    x32 = (d - vmin) / np.float32(vmax - vmin)
    x64 = ((d.astype(np.float64) - np.float64(vmin)) / (np.float64(vmax) - np.float64(vmin))).astype(np.float32)
    differ = int((np.trunc(np.minimum(x32, 1) * 256) != np.trunc(np.minimum(x64, 1) * 256)).sum())
    print("pixels of the wide case at which an fp64 Normalize picks another table entry:", differ)
    assert differ >= 8


def test_full_size_case(emu_vis):
    if os.environ.get("RCMVS_EMU_FULL") != "1":
        pytest.skip("the 1056 x 1920 map takes minutes on the emulation: set RCMVS_EMU_FULL=1 (tests/test_gpu_tanks_eval.py always runs it)")
    H, W, seed = (int(x) for x in GOLD["full:dims"])
    depth = synthetic.depth_vis_map(H, W, seed)
    assert zlib.crc32(depth.tobytes()) == int(GOLD["full:depth_crc"])
    rgb, vm = colour(depth)
    assert same_bits(vm, GOLD["full:vminmax"])
    assert np.array_equal(rgb[::16, ::16], GOLD["full:image"])
    assert zlib.crc32(np.ascontiguousarray(rgb).tobytes()) == int(GOLD["full:crc"])


def test_selection_against_a_full_sort(emu_vis):
    """200 seeded maps of up to 4 096 values: few distinct values (heavy ties), negative values, -0 and +0, huge and tiny
    magnitudes, random percentiles including 0 and 100.  vmin and vmax equal the sort's (== : the two zeros compare equal)."""
    rng = np.random.default_rng(2025)
    for trial in range(200):
        n = int(rng.integers(1, 4097))
        h = int(rng.choice([d for d in range(1, min(n, 64) + 1) if n % d == 0]))
        kind = trial % 5
        if kind == 0:
            vals = rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30)
        elif kind == 1:
            vals = rng.choice(rng.standard_normal(int(rng.integers(1, 6))), n)                     # at most 5 distinct values
        elif kind == 2:
            vals = rng.choice(np.array([-0.0, 0.0, 1.0, -1.0, 1e-40, -1e-40]), n)                   # both zeros, denormals
        elif kind == 3:
            vals = np.round(rng.standard_normal(n) * 3.0)                                          # small integers of both signs
        else:
            vals = 500.0 + 300.0 * rng.random(n)
        vals = vals.astype(np.float32).reshape(h, n // h)
        pct = float(rng.choice([0.0, 100.0, 95.0, 50.0, 100.0 * rng.random()]))
        _, vm = colour(vals, percentile=pct)
        want = numpy_percentile_fp32(vals, pct)
        assert vm[0] == vals.min() and vm[1] == want, (trial, n, pct, vm, vals.min(), want)
        if trial % 10 == 0:                                                                          # and numpy itself agrees with the restatement
            assert np.percentile(vals, np.float32(pct)) == want, (trial, n, pct)


def test_two_runs_are_identical_and_the_workspace_is_reused(emu_vis):
    depth = synthetic.depth_vis_map(77, 131, seed=21)
    a, va = colour(depth)
    other, _ = colour(synthetic.depth_vis_map(5, 9, seed=22))                                      # another size in between, same workspace
    b, vb = colour(depth)
    assert np.array_equal(a, b) and same_bits(va, vb) and len(depth_vis._DEVICE) == 1
    assert other.shape == (5, 9, 3)


def test_edges_of_the_map(emu_vis):
    """values equal to vmax are the last entry (x * 256 == 256 -> 255), the 5 % above it too; the minimum is the first entry;
    a caller's table is used as given; an unaligned map takes the scalar loads"""
    depth = synthetic.depth_vis_map(40, 52, seed=30)
    rgb, vm = colour(depth)
    last, first = depth_vis.MAGMA_R[255], depth_vis.MAGMA_R[0]
    assert (depth >= vm[1]).sum() >= 0.05 * depth.size - 1
    assert (rgb[depth >= vm[1]] == last).all() and (rgb[depth == vm[0]] == first).all()
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    g, _ = colour(depth, lut=grey)
    x = (depth - vm[0]) / np.float32(vm[1] - vm[0]) * np.float32(256)
    want = np.where(x >= 256, 255, np.trunc(np.minimum(x, 255))).astype(np.uint8)
    assert np.array_equal(g[..., 0], want) and np.array_equal(g[..., 1], want)
    off = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), depth.ravel()]))[1:].view(40, 52)
    assert off.data_ptr() % 16 != 0
    assert np.array_equal(depth_vis.depth_colormap(off)[0].numpy(), rgb)


def test_refusals(emu_vis):
    d = torch.zeros((4, 5))
    with pytest.raises(_lib.RcmvsError, match="percentile"):
        depth_vis.depth_colormap(d, percentile=100.5)
    with pytest.raises(_lib.RcmvsError, match=r"\(H, W\)"):
        depth_vis.depth_colormap(torch.zeros((1, 4, 5)))
    with pytest.raises(_lib.RcmvsError, match=r"\(256, 3\)"):
        depth_vis.depth_colormap(d, lut=np.zeros((255, 3), np.uint8))


def test_cpu_tensors_raise_without_the_emulation():
    with pytest.raises(_lib.RcmvsError):
        depth_vis.depth_colormap(torch.zeros((4, 5)))


@pytest.mark.parametrize("order", ["1", "2"])
def test_other_thread_orders_give_the_same_bytes(order, tmp_path):
    """RCMVS_EMU_ORDER=1|2 schedules every block's threads in another order between synchronisation points: a missing barrier
    would change the image.  Run in a child process (the order is read when the library is loaded)."""
    script = tmp_path / "run.py"
    script.write_text(
        "import sys, os\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np, torch, conftest\n"
        "from rc_mvsnet_amd import depth_vis, fusion, synthetic\n"
        "lib = conftest.load_emu_lib()\n"
        "conftest.route_to_emulation(lib, setattr)\n"
        "depth_vis._chk, depth_vis._stream = fusion._chk, fusion._stream\n"
        "rgb, vm = depth_vis.depth_colormap(torch.from_numpy(synthetic.depth_vis_map(61, 149, seed=5)))\n"
        "sys.stdout.write(rgb.numpy().tobytes().hex() + vm.numpy().tobytes().hex())\n" % (REPO, os.path.join(REPO, "tests")))
    outs = []
    for o in ("0", order):
        env = dict(os.environ, RCMVS_EMU_ORDER=o)
        outs.append(subprocess.run([sys.executable, str(script)], env=env, check=True, capture_output=True, text=True).stdout)
    assert len(outs[0]) == 2 * (61 * 149 * 3 + 8) and outs[0] == outs[1]
