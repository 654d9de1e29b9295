"""The F-score's kernels (csrc/pc_register.hip) on the CPU emulation of tests/emu, driven through rc_mvsnet_amd/tanks_fscore.py on
CPU tensors and checked against the fp64 oracle (tests/tanks_fscore_oracle.py): crop flags and voxel outputs bit for bit, the ICP
moments within 1e-12 relative, histogram counts exactly.  The emulation runs blocks one after another, so this also pins that no
result depends on the blocks' order."""
import numpy as np
import pytest
import torch

import tanks_fscore_oracle as O
from rc_mvsnet_amd import _lib, dtu_eval, fusion, tanks_fscore as F


@pytest.fixture
def emu_tf(emu, monkeypatch):
    _lib.bind(emu)                                               # the emu fixture binds the primary header's table; the extension's too
    for mod in (dtu_eval, F):                                    # the emu fixture routes fusion / ops; these two modules too
        monkeypatch.setattr(mod, "_chk", fusion._chk)
        monkeypatch.setattr(mod, "_stream", fusion._stream)
    return emu


L_POLY = np.array([[0.1, 0.1], [0.9, 0.1], [0.9, 0.5], [0.5, 0.5], [0.5, 0.9], [0.1, 0.9]])


def _T():
    c, s = np.cos(0.3), np.sin(0.3)
    T = np.eye(4)
    T[:3, :3] = 1.3 * np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    T[:3, 3] = (0.2, -0.1, 0.05)
    return T


def test_crop_on_emulated_kernels(emu_tf):
    rng = np.random.default_rng(0)
    pts = rng.random((2000, 3)).astype(np.float32)
    pts[:40, 1] = 0.5                                            # a coordinate equal to a vertex's (v for some axis, u for another)
    pts[40:80, 0] = 0.5                                          # on a vertical edge
    pts[80:90, 2] = np.float32(0.2)
    pts[90:100, 2] = np.float32(0.8)
    for axis in (0, 1, 2):
        for T in (None, _T()):
            vol = F.make_volume(axis, float(np.float32(0.2)), float(np.float32(0.8)), L_POLY)
            flags, kept = F.crop(torch.from_numpy(pts), vol, T)
            want, q = O.crop(pts, axis, vol["axis_min"], vol["axis_max"], L_POLY, T)
            assert np.array_equal(flags.numpy(), want)
            assert np.array_equal(kept.numpy(), q[want])
            assert 0 < want.sum() < len(pts)


def test_voxel_down_sample_on_emulated_kernels(emu_tf):
    rng = np.random.default_rng(1)
    pts = np.concatenate([rng.random((1200, 3)) * 2.0 - 1.0, rng.normal(0.3, 0.01, (700, 3)),
                          np.repeat(rng.random((50, 3)), 2, axis=0)]).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    for voxel in (0.25, 0.05, 1e-4):                             # 1e-4: 2e4 voxels per axis, a 44-bit key (6 radix passes)
        got = F.voxel_down_sample(torch.from_numpy(pts), voxel).numpy()
        want = O.voxel_down_sample(pts, voxel)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), voxel
    assert len(O.voxel_down_sample(pts, 0.25)) < 600 < len(O.voxel_down_sample(pts, 1e-4))


def test_icp_step_on_emulated_kernels(emu_tf):
    rng = np.random.default_rng(2)
    tgt = (rng.random((1500, 3)) + 1.0).astype(np.float32)
    tgt = np.concatenate([tgt, tgt[:60]])                        # exact duplicates: the tie case
    src = (tgt[rng.integers(0, len(tgt), 2000)] + rng.normal(0, 0.02, (2000, 3))).astype(np.float32)
    T = np.eye(4)
    T[:3, 3] = (0.01, -0.02, 0.015)
    max_dist = 0.035
    target = F.IcpTarget(torch.from_numpy(tgt), max_dist)
    mom, corr = F.icp_step(torch.from_numpy(src), target, T, max_dist, want_corr=True)
    want, wcorr = O.icp_step(src, tgt, T, max_dist)
    assert 0.3 < want[0] / len(src) < 0.95
    assert np.array_equal(corr.numpy(), wcorr)
    assert mom[0] == want[0]
    assert np.all(np.abs(mom[1:] - want[1:]) <= 1e-12 * np.abs(want[1:]))
    r = F.icp(torch.from_numpy(src), target, max_dist, T, max_iter=3)
    w = O.icp(src, tgt, max_dist, T, max_iter=3)
    assert r["iterations"] == w["iterations"] and np.abs(r["transformation"] - w["transformation"]).max() <= 1e-9


def test_dist_hist_on_emulated_kernels(emu_tf):
    rng = np.random.default_rng(3)
    tau, nbins = 0.01, 499
    w = tau / 100.0
    d = np.concatenate([rng.random(1800) * 0.06, np.full(100, 5 * tau), np.zeros(50), np.arange(50) * w])
    counts, below = F.dist_hist(torch.from_numpy(d), tau, nbins, w)
    b = np.floor(d / w)
    want = np.bincount(b[(b >= 0) & (b < nbins)].astype(np.int64), minlength=nbins).astype(np.uint64)
    assert counts.dtype == np.uint64 and np.array_equal(counts, want)
    assert below == int((d < tau).sum())


def test_evaluate_on_emulated_kernels(emu_tf):
    from rc_mvsnet_amd import synthetic
    s = synthetic.tanks_fscore_scene(n_gt=1500, n_est=1200, tau=0.05, seed=4)
    v = F.make_volume(s["volume"]["axis"], s["volume"]["axis_min"], s["volume"]["axis_max"], s["volume"]["polygon"])
    got = F.evaluate(torch.from_numpy(s["est"]), torch.from_numpy(s["gt"]), s["T_true"], v, s["tau"])
    want = O.evaluate(s["est"], s["gt"], s["T_true"], (v["axis"], v["axis_min"], v["axis_max"], v["polygon"]), s["tau"])
    for k in ("precision", "recall", "n_est", "n_gt"):
        assert got[k] == want[k], k
    assert abs(got["fscore"] - want["fscore"]) <= 1e-15 * want["fscore"]
    assert np.array_equal(got["hist_est"], want["hist_est"]) and np.array_equal(got["hist_gt"], want["hist_gt"])
    assert 0.5 < got["precision"] < 1.0 and 0.3 < got["recall"] < 1.0
