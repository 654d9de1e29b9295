"""The cases and checks of the COLMAP-import kernels, shared by tests/test_gpu_colmap_import.py (device "cuda:0") and
tests/test_colmap_import_emu_cpu.py (the CPU emulation, device "cpu"): same models, same bounds, against tests/colmap_oracle.py."""
import math
import os

import numpy as np
import pytest
import torch

import colmap_oracle as O
from rc_mvsnet_amd import _lib, colmap_import as CI, colmap_io, scan_io, synthetic

NUM_SRC = 5


def to(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def ring(n, radius=4.0, arc_deg=70.0):
    a = np.radians(arc_deg) * (np.arange(n) / max(n - 1, 1) - 0.5)
    return np.stack([radius * np.sin(a), 0.3 * np.sin(3.0 * a + 0.4), -radius * np.cos(a)], 1)


def csr(lists):
    offsets = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    return offsets, np.concatenate(lists).astype(np.int32)


def subset(rng, pool, size, must=()):
    pool = np.setdiff1d(pool, must)
    return np.sort(np.concatenate([np.array(must, dtype=np.int64), rng.choice(pool, size - len(must), replace=False)]))


def score_case(name):
    """-> (centres, points, offsets, ids).  Point 0 is seen by every image of the models that share anything; in "n9" point 1 sits on
    the centre of camera 2 and the list lengths 1, 63, 64, 65, 257 cross the wave and block strides."""
    rng = np.random.default_rng({"n2": 1, "n3_interleaved": 2, "n3_ranges": 3, "n9": 4}[name])
    m = 400
    points = rng.uniform(-1.3, 1.3, (m, 3))
    everything = np.arange(m)
    if name == "n2":
        centres = ring(2, arc_deg=12.0)
        lists = [subset(rng, everything, 64, [0]), subset(rng, everything, 257, [0])]
    elif name == "n3_interleaved":                               # image 2 shares nothing, although its id range overlaps the others'
        centres = ring(3)
        lists = [subset(rng, everything[0::2], 65, [0]), subset(rng, everything[0::2], 63, [0]), subset(rng, everything[1::2], 100)]
    elif name == "n3_ranges":                                    # image 2 shares nothing: its ids lie above the others' (the early out)
        centres = ring(3)
        lists = [subset(rng, everything[:200], 65, [0]), subset(rng, everything[:200], 120, [0]), subset(rng, everything[200:], 64)]
    else:
        centres = ring(9)
        points[1] = centres[2]
        lengths = [1, 63, 64, 65, 257, 120, 200, 30, 257]
        lists = [subset(rng, everything, L, [0, 1] if i in (2, 3, 4) else [0]) for i, L in enumerate(lengths)]
    return (centres, points) + csr(lists)


def duplicate_case():
    """images 1 and 2 are exact duplicates (same centre, same list); image 3 shares nothing with anyone"""
    rng = np.random.default_rng(11)
    points = rng.uniform(-1.3, 1.3, (300, 3))
    centres = ring(4)
    centres[2] = centres[1]
    dup = subset(rng, np.arange(200), 90)
    lists = [subset(rng, np.arange(200), 130), dup, dup.copy(), subset(rng, np.arange(200, 300), 40)]
    return (centres, points) + csr(lists)


def run_scores(dev, case):
    centres, points, offsets, ids = case
    return CI.pair_scores(to(dev, centres), to(dev, points), to(dev, offsets), to(dev, ids)).cpu().numpy()


def check_scores(dev, name):
    case = score_case(name)
    want, common = O.pair_scores(*case)
    got = run_scores(dev, case)
    err = np.abs(got - want)
    print(f"{name}: max |delta| {err.max():.3e}, max common {common.max()}, bound at it {1e-12 * (1 + common.max()):.3e}")
    assert (err <= 1e-12 * (1 + common)).all()
    assert np.array_equal(bits(got), bits(got.T)) and (np.diag(got) == 0).all()
    assert (got[common == 0] == 0).all()
    assert np.array_equal(bits(run_scores(dev, case)), bits(got))               # two runs: the same bits
    if name.startswith("n3"):
        assert (common[2] == 0).all() and common[0, 1] > 0
    else:
        assert (common + np.eye(len(common), dtype=np.int64) > 0).all()          # point 0 is shared by every pair
    return got


def check_ordering(dev):
    case = score_case("n9")
    want, _ = O.pair_scores(*case)
    lists, counts = O.top_views(want, NUM_SRC)
    for i, row in enumerate(want):                               # the precondition, on the oracle alone: no near tie in what is listed
        s = np.sort(row[np.arange(len(row)) != i])[::-1][:NUM_SRC + 1]
        s = s[s > 0]
        assert len(s) == NUM_SRC + 1 and (np.abs(np.diff(s)) > 1e-9 * s[:-1]).all(), (i, s)
    scores = CI.pair_scores(*(to(dev, a) for a in case))
    ids, top, cnt = (t.cpu().numpy() for t in CI.top_views(scores, NUM_SRC))
    assert ids.dtype == np.int32 and np.array_equal(ids, np.array(lists, dtype=np.int32))
    assert np.array_equal(cnt, counts)
    table = scores.cpu().numpy()
    assert np.array_equal(bits(top), bits(np.take_along_axis(table, ids.astype(np.int64), 1)))


def check_duplicates(dev):
    case = duplicate_case()
    scores = CI.pair_scores(*(to(dev, a) for a in case))
    table = scores.cpu().numpy()
    want, _ = O.pair_scores(*case)
    assert table[0, 1] > 0 and bits(table[0, 1]) == bits(table[0, 2])            # the tie, to the bit
    k = 3
    ids, top, cnt = (t.cpu().numpy() for t in CI.top_views(scores, k))
    assert ids[0].tolist() == [1, 2, -1] and top[0, 2] == 0                       # the lower index first; image 3 (score 0) is absent
    assert ids[3].tolist() == [-1, -1, -1] and (top[3] == 0).all()
    assert cnt.tolist() == [2, 2, 2, 0]
    lists, counts = O.top_views(want, k)
    assert [[j for j in row if j >= 0] for row in ids.tolist()] == lists and np.array_equal(cnt, counts)
    ids1, _, cnt1 = (t.cpu().numpy() for t in CI.top_views(scores, 1))            # fewer slots than partners: the count still says 2
    assert ids1[:, 0].tolist() == [1, 0, 0, -1] and cnt1.tolist() == [2, 2, 2, 0]


DEPTH_LENGTHS = (2, 99, 100, 101, 257, 5000)


def depth_case():
    """-> (points, zrows, offsets, ids, ranks, extrinsics).  Points 3000.. repeat points 0.. (repeated z values); image 4 (257
    points, ranks 2 and 254) looks the other way, so its 1 % rank lands on a negative z."""
    rng = np.random.default_rng(21)
    m = 6000
    points = rng.uniform(-1.3, 1.3, (m, 3))
    points[3000:] = points[:3000]
    n = len(DEPTH_LENGTHS)
    E = np.zeros((n, 4, 4))
    for k in range(n):
        E[k] = synthetic._similarity(rng.normal(size=3), rng.uniform(0.0, 40.0), 1.0, (0.0, 0.0, 0.0))
        E[k, :3, 3] = (0.1 * k, -0.2, 4.0)
    E[4, 2, :3] = -E[4, 2, :3]
    E[4, 2, 3] = 0.3
    lists = [subset(rng, np.arange(m), L) for L in DEPTH_LENGTHS]
    lists[5] = np.sort(np.concatenate([np.arange(2000), np.arange(3000, 5000), rng.choice(np.arange(5000, 6000), 1000, replace=False)]))
    offsets, ids = csr(lists)
    ranks = np.array([O.ranks(L) for L in DEPTH_LENGTHS], dtype=np.int32)
    return points, np.ascontiguousarray(E[:, 2, :]), offsets, ids, ranks, E


def check_depth_ranks(dev):
    points, zrows, offsets, ids, ranks, E = depth_case()
    assert ranks.tolist() == [[0, 1], [0, 98], [1, 99], [1, 99], [2, 254], [50, 4950]]
    want = O.depth_ranks(points, zrows, offsets, ids, ranks)
    z5 = O.depths(points, zrows[5], ids[offsets[5]:offsets[6]])
    assert len(np.unique(z5)) <= 3000 and want[4, 0] < 0 < want[4, 1]            # repeated values; the negative 1 % depth
    got = CI.depth_ranges(to(dev, points), to(dev, zrows), to(dev, offsets), to(dev, ids), to(dev, ranks)).cpu().numpy()
    assert np.array_equal(bits(got), bits(want))
    # other ranks, the first and last of a list and ranks outside it among them
    r2 = np.array([[0, 1], [98, 99], [99, 100], [100, 101], [-1, 256], [4999, 5000]], dtype=np.int32)
    got2 = CI.depth_ranges(to(dev, points), to(dev, zrows), to(dev, offsets), to(dev, ids), to(dev, r2)).cpu().numpy()
    for i, L in enumerate(DEPTH_LENGTHS):
        z = np.sort(O.depths(points, zrows[i], ids[offsets[i]:offsets[i + 1]]))
        for q in range(2):
            if 0 <= r2[i, q] < L:
                assert bits(got2[i, q]) == bits(z[r2[i, q]]), (i, q)
            else:
                assert math.isnan(got2[i, q]), (i, q)
    # host validation: the image whose 1 % depth is negative is named
    n = len(DEPTH_LENGTHS)
    M = {"image_ids": np.arange(1, n + 1), "names": ["v%d.jpg" % k for k in range(n)], "offsets": offsets, "ids": ids, "points": points,
         "extrinsics": E, "centres": np.zeros((n, 3)), "intrinsics": np.zeros((n, 3, 3)), "sizes": np.zeros((n, 2), dtype=np.int64),
         "files": {"images": "images.txt"}}
    with pytest.raises(_lib.RcmvsError, match=r"image 5 \(v4\.jpg\): depth_min"):
        CI.import_scene(M, "nowhere", "nowhere", device=dev)


def check_end_to_end(dev, tmp_path):
    from rc_mvsnet_amd.mvs_dataset import MVSDataset
    model = synthetic.colmap_model(n_images=6, n_points=400, hw=(64, 96), seed=0)
    sparse, images, out = str(tmp_path / "sparse"), str(tmp_path / "photos"), str(tmp_path / "test" / "scene")
    synthetic.write_colmap_model(model, sparse)
    synthetic.write_colmap_images(model, images)
    summary = CI.import_scene(sparse, images, out, max_d=48, interval_scale=1.0, num_src=NUM_SRC, device=dev)
    M = colmap_io.read_model(sparse)
    truth = model["truth"]
    assert summary["images"] == 6 and summary["points"] == 400 and summary["skipped_refs"] == [] and summary["refs"] == 6
    # pair.txt: the oracle's lists
    want, _ = O.pair_scores(M["centres"], M["points"], M["offsets"], M["ids"])
    lists, _ = O.top_views(want, NUM_SRC)
    pairs = scan_io.read_pair_file(os.path.join(out, "pair.txt"))
    assert pairs == [(i, lists[i]) for i in range(6)]
    # the depth line and the JPEG copy
    rk = np.array([O.ranks(c) for c in np.diff(M["offsets"])])
    dr = O.depth_ranks(M["points"], np.ascontiguousarray(M["extrinsics"][:, 2, :]), M["offsets"], M["ids"], rk)
    for k in range(6):
        with open(os.path.join(out, "cams", "%08d_cam.txt" % k)) as f:
            tail = [float(v) for v in f.read().split("\n")[11].split()]
        assert tail == [dr[k, 0], (dr[k, 1] - dr[k, 0]) / 47 / 1.0, 48.0, dr[k, 1]]
        with open(os.path.join(images, M["names"][k]), "rb") as a, open(os.path.join(out, "images", "%08d.jpg" % k), "rb") as b:
            assert a.read() == b.read()
    ds = MVSDataset(str(tmp_path / "test"), ["scene"], mode="test", nviews=3, max_h=64, max_w=96, device=dev)
    assert len(ds) == 6
    item = ds[0]
    views = [pairs[0][0]] + pairs[0][1][:2]
    assert tuple(item["imgs"].shape) == (3, 3, 64, 96)
    proj = item["proj_matrices"]["stage1"]
    Kq = truth["intrinsics"].copy()
    Kq[:, :2] /= 4.0
    for i, v in enumerate(views):
        assert np.allclose(proj[i, 0], truth["extrinsics"][v].astype(np.float32), rtol=1e-6, atol=1e-6)
        assert np.allclose(proj[i, 1, :3, :3], Kq[v].astype(np.float32), rtol=1e-6, atol=0)
    assert item["depth_values"][0] == np.float32(dr[views[0], 0])
    return summary
