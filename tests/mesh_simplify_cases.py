"""The cases and checks of the mesh simplification kernels (csrc/mesh_simplify.hip through rc_mvsnet_amd/mesh_simplify.py), shared by
tests/test_gpu_mesh_simplify.py (device "cuda:0") and tests/test_mesh_simplify_emu_cpu.py (the CPU emulation, device "cpu"), against
tests/mesh_simplify_oracle.py.  Every comparison is bit equality, after every round: the 1-ring, the locked flags, the edge states,
the keys, best1 / best2, the selected and applied flags, remap, positions, quadrics, members, colour sums and the live count, then
the final mesh, its colours and the stats.  The known answers (a plane, a cube, the invariants of closed manifolds, the
independence of a round's collapses) are derived here in exact arithmetic, not fitted."""
import functools
from fractions import Fraction

import numpy as np
import torch

import mesh_clean_cases as MCC
import mesh_decimate_cases as MDC
import mesh_simplify_oracle as O
from rc_mvsnet_amd import _lib, mesh_simplify as MS

INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
same_bits, same_bits64, to_dev, host = MCC.same_bits, MDC.same_bits64, MCC.to_dev, MCC.host


def _mesh(v, faces, seed=0):
    v = np.asarray(v, np.float32).reshape(-1, 3)
    return v, np.asarray(faces, np.int32).reshape(-1, 3), np.random.default_rng(seed + 1).integers(0, 256, (len(v), 3), dtype=np.uint8)


# ---- builders ---------------------------------------------------------------------------------------------------------------
def grid_faces(rows, cols, first=0):
    idx = first + np.arange(rows * cols).reshape(rows, cols)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    return np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)])


def sheet(rows, cols, seed, jitter=0.0, bump=0.2):
    """a rows x cols height field 1 apart, z a smooth bump plus noise; jitter moves the vertices in x and y"""
    rng = np.random.default_rng(seed)
    y, x = np.divmod(np.arange(rows * cols), cols)
    p = np.stack([x + jitter * rng.uniform(-1, 1, x.size), y + jitter * rng.uniform(-1, 1, x.size), bump * np.sin(0.7 * x) * np.cos(0.5 * y) + 0.02 * rng.standard_normal(x.size)], 1)
    return p, grid_faces(rows, cols)


def padded_sheet(nv, order="shuffled"):
    """an 8 x (nv // 8) sheet and nv % 8 vertices no face uses: nv vertices in all, numbered along the rows or shuffled"""
    cols = nv // 8
    p, f = sheet(8, cols, nv)
    p = np.concatenate([p, np.full((nv - 8 * cols, 3), 0.5)])
    if order == "shuffled":
        number = np.random.default_rng(nv).permutation(nv)
        q = np.zeros_like(p)
        q[number] = p
        p, f = q, number[f][np.random.default_rng(nv + 1).permutation(len(f))]
    return _mesh(p, f, nv)


def tetrahedron():
    return _mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], [(0, 2, 1), (0, 1, 3), (1, 2, 3), (0, 3, 2)], 4)


def octahedron():
    p = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1.5], [0, 0, -1]]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    return _mesh(p, f, 8)


def bipyramid(n):
    """two apexes over a ring of n vertices: closed, every apex has n corners (a fan of n faces)"""
    t = 2 * np.pi * np.arange(n) / n
    rng = np.random.default_rng(n)
    ring = np.stack([np.cos(t), np.sin(t), 0.05 * rng.standard_normal(n)], 1)
    p = np.concatenate([ring, [[0, 0, 0.8], [0, 0, -0.6]]])
    i, j = np.arange(n), (np.arange(n) + 1) % n
    f = np.concatenate([np.stack([i, j, np.full(n, n)], 1), np.stack([j, i, np.full(n, n + 1)], 1)])
    return _mesh(p, f, n)


def sphere(n=12, r=1.0):
    """a closed latitude-longitude sphere: 2 poles and (n - 1) rings of 2 n vertices"""
    m = 2 * n
    lat = np.pi * np.arange(1, n) / n
    lon = 2 * np.pi * np.arange(m) / m
    p = [[0, 0, r]] + [[r * np.sin(a) * np.cos(b), r * np.sin(a) * np.sin(b), r * np.cos(a)] for a in lat for b in lon] + [[0, 0, -r]]
    f = []
    for j in range(m):
        f.append((0, 1 + j, 1 + (j + 1) % m))
    for i in range(n - 2):
        for j in range(m):
            a, b = 1 + i * m + j, 1 + i * m + (j + 1) % m
            f += [(a, a + m, b), (b, a + m, b + m)]
    last, south = 1 + (n - 2) * m, 1 + (n - 1) * m
    for j in range(m):
        f.append((south, last + (j + 1) % m, last + j))
    return _mesh(p, f, n)


def invalid_indices():
    """a sheet, then faces with indices -1 / nv / INT_MAX / INT_MIN and repeated ones"""
    p, f = sheet(6, 6, 66)
    nv = len(p)
    bad = [(3, 3, 4), (5, 6, 5), (-1, 0, 1), (0, nv, 1), (4, 5, INT_MAX), (INT_MIN, 1, 2), (0, 0, 0)]
    return _mesh(p, np.concatenate([f[:20], bad, f[20:]]), 66)


def nonfinite():
    """NaN, infinities, the largest fp32, 1e30, denormals and both zeros in an 8 x 8 sheet"""
    p, f = sheet(8, 8, 88)
    p = p.astype(np.float32)
    p[9] = [np.nan, 1.0, 0.0]
    p[18] = [2.0, np.inf, 0.0]
    p[27, 2] = -np.inf
    p[36] = [3.4e38, -3.4e38, 3.4e38]
    p[45, 0] = 1e30
    p[54] = [1e-45, -1e-40, -0.0]
    p[20, 2], p[21, 2] = -0.0, 0.0
    return _mesh(p, f, 88)


def minus_zero():
    """a flat 5 x 5 sheet in the plane x = 0 whose smallest coordinates are -0.0 and +0.0 side by side"""
    p, f = sheet(5, 5, 55, bump=0.0)
    p = np.stack([np.zeros(25), p[:, 0], p[:, 1]], 1).astype(np.float32)
    p[::2, 0] = -0.0
    p[0, 1], p[1, 2] = -0.0, -0.0
    return _mesh(p, f, 55)


def duplicates_and_fin():
    """an octahedron with one face repeated, one repeated in the opposite orientation, and a fin on one edge: edges of multiplicity 3
    and 4 lock their ends"""
    v, f, _ = octahedron()
    v = np.concatenate([v, [[2, 2, 0]]])
    return _mesh(v, np.concatenate([f, [(0, 2, 4), (4, 1, 2), (0, 2, 6)]]), 9)


def double_face():
    """two faces on the same three vertices in opposite orientation: every edge has multiplicity 2 and fails the link condition"""
    return _mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [(0, 1, 2), (0, 2, 1)], 2)


def crumpled():
    """a sheet whose vertices are moved by up to 0.45 of the spacing: collapses that would fold a neighbouring face over"""
    p, f = sheet(10, 10, 45, jitter=0.45, bump=0.0)
    return _mesh(p, f, 45)


def plane(n=17):
    """a planar n x n grid over the unit square (n - 1 a power of two: dyadic coordinates), z = 0"""
    y, x = np.divmod(np.arange(n * n), n)
    return _mesh(np.stack([x / (n - 1.0), y / (n - 1.0), np.zeros(n * n)], 1), grid_faces(n, n), n)


def cube(n=9):
    """a closed unit cube, each side an n x n grid (n - 1 a power of two: dyadic coordinates), outward orientation; n = 9: 386
    vertices, 768 faces"""
    m = n - 1
    number, pts, faces = {}, [], []

    def vid(p):
        if p not in number:
            number[p] = len(pts)
            pts.append(p)
        return number[p]

    for axis in range(3):
        for side in (0, m):
            for i in range(m):
                for j in range(m):
                    def at(a, b):
                        q = [0, 0, 0]
                        q[axis], q[(axis + 1) % 3], q[(axis + 2) % 3] = side, a, b
                        return vid(tuple(q))
                    quad = [at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)]      # counter-clockwise seen from +axis
                    if side == 0:
                        quad.reverse()
                    faces += [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
    return _mesh(np.array(pts) / float(m), faces, n)


STRIP = MDC.strip
ALL = {"target_faces": 0}
# name -> (builder, option sets of simplify)
CASES = {
    "empty": (lambda: _mesh(np.zeros((0, 3)), np.zeros((0, 3))), [ALL, {"ratio": 0.5}]),
    "one_face": (lambda: _mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [(0, 1, 2)]), [ALL, {"target_faces": 0, "drop_unreferenced": False}]),
    "two_faces": (lambda: _mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.25]], [(0, 1, 2), (1, 3, 2)]), [ALL]),
    "tetrahedron": (tetrahedron, [ALL]),
    "octahedron": (octahedron, [ALL, {"target_faces": 6}]),
    "double_face": (double_face, [ALL]),
    "duplicates_and_fin": (duplicates_and_fin, [ALL, {"target_faces": 0, "drop_unreferenced": False}]),
    "invalid_indices": (invalid_indices, [ALL, {"ratio": 0.5, "drop_unreferenced": False}]),
    "nonfinite": (nonfinite, [ALL, {"ratio": 0.5}]),
    "minus_zero": (minus_zero, [ALL]),
    "crumpled": (crumpled, [ALL]),
    "specks_4097": (functools.partial(MDC.specks, 4097), [ALL]),
    # budget, error bound and round limit on one closed surface of 528 faces (sphere(12): 266 vertices)
    "sphere": (sphere, [{"ratio": 0.5}, {"target_faces": 522}, {"target_faces": 528}, {"target_faces": 529}, {"target_faces": 0, "max_error": 0.0},
                        {"target_faces": 0, "max_error": 1e-7}, {"target_faces": 0, "max_rounds": 1}, {"target_faces": 0, "max_rounds": 0},
                        {"ratio": 0.1, "drop_unreferenced": False}]),
    # the known answers: equal costs leave the entry number to decide, one or two collapses a round, so the large ones take
    # hundreds of rounds: seconds on the device, minutes on the emulation, which runs the small ones
    "plane_17": (plane, [{"target_faces": 0, "max_error": 0.0}]),
    "cube_9": (cube, [{"target_faces": 0, "max_error": 0.0}]),
    "plane_9": (functools.partial(plane, 9), [{"target_faces": 0, "max_error": 0.0}]),
    "cube_5": (functools.partial(cube, 5), [{"target_faces": 0, "max_error": 0.0}]),
}
for _n in (24, 25, 48, 50, 600):                                 # mesh_clean's ring sort changes path at 48 entries: 24 / 25 faces at the apex
    CASES[f"fan_{_n}"] = (functools.partial(bipyramid, _n), [{"ratio": 0.5}] if _n == 600 else [ALL])
# the sort's 256-element blocks and the scan's 2048-element tiles: strips (all rim: nothing may collapse) and sheets (two rounds)
for _nv in (255, 256, 257, 2047, 2048, 2049, 4097):
    for _order in ("ascending", "descending", "shuffled") if _nv in (257, 2049) else ("shuffled",):
        CASES[f"strip_{_nv}_{_order}"] = (functools.partial(STRIP, _nv, _order), [ALL])
    CASES[f"sheet_{_nv}"] = (functools.partial(padded_sheet, _nv), [{"ratio": 0.25, "max_rounds": 2}])
CASES["sheet_257_ascending"] = (functools.partial(padded_sheet, 257, "ascending"), [{"ratio": 0.25}])

CLOSED = ("tetrahedron", "octahedron", "sphere", "cube_9", "cube_5", "fan_24", "fan_25", "fan_48", "fan_50", "fan_600")      # closed manifolds: the invariants hold after every round
# what a case is there for, asserted on the oracle's stats of its FIRST option set (a callable: on the stats)
KNOWN = {
    "empty": {"faces_out": 0, "vertices_out": 0, "rounds": 0, "stop": "target"},
    "one_face": {"faces_out": 1, "locked_vertices": 3, "stop": "nothing_selected", "collapses": [0]},
    "two_faces": {"faces_out": 2, "locked_vertices": 4, "collapses": [0]},
    "tetrahedron": {"faces_out": 4, "vertices_out": 4, "rejected_link": 6, "locked_vertices": 0, "collapses": [0], "stop": "nothing_selected"},
    "octahedron": {"locked_vertices": 0, "collapses": lambda c: c[0] == 1},
    "double_face": {"faces_out": 2, "rejected_link": 3, "locked_vertices": 0},
    "duplicates_and_fin": {"locked_vertices": lambda n: n >= 4},
    "invalid_indices": {"faces_in": 57, "valid_faces_in": 50},
    "nonfinite": {"nonfinite_vertices": 3, "nonfinite_faces": lambda n: n > 0},
    "crumpled": {"rejected_flip": lambda n: n > 0},
    "specks_4097": {"faces_out": 4097, "vertices_out": 3 * 4097, "locked_vertices": 3 * 4097, "collapses": [0]},
    "strip_2049_shuffled": {"faces_out": 2047, "locked_vertices": 2049, "collapses": [0]},
    "sphere": {"valid_faces_in": 528, "faces_out": 264, "stop": "target"},
}
KNOWN_BY_OPTION = {
    ("sphere", 1): {"collapses": [3], "faces_out": 522, "stop": "target"},          # the budget cuts the first round's set
    ("sphere", 2): {"rounds": 0, "faces_out": 528, "vertices_out": 266, "stop": "target"},
    ("sphere", 3): {"rounds": 0, "faces_out": 528},
    ("sphere", 4): {"faces_out": 528, "stop": "nothing_selected", "rejected_cost": lambda n: n > 0},
    ("sphere", 6): {"rounds": 1, "stop": "max_rounds"},
    ("sphere", 7): {"rounds": 0, "stop": "max_rounds", "faces_out": 528},
    ("octahedron", 1): {"faces_out": 6, "collapses": [1]},
}


@functools.lru_cache(maxsize=None)
def case(name):
    v, f, rgb = CASES[name][0]()
    for a in (v, f, rgb):
        a.setflags(write=False)
    return v, f, rgb


@functools.lru_cache(maxsize=None)
def reference(name, k):
    v, f, rgb = case(name)
    return O.simplify(v, f, rgb, **CASES[name][1][k])


def case_keys():
    return [(name, k) for name in CASES for k in range(len(CASES[name][1]))]


# ---- properties -------------------------------------------------------------------------------------------------------------
def edge_stats(faces, nv):
    """-> (boundary edges, non-manifold edges, Euler characteristic, consistently oriented) of the valid faces"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < nv)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    f = f[ok]
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    und, cnt = np.unique(np.sort(d, 1), axis=0, return_counts=True)
    oriented = len(np.unique(d, axis=0)) == len(d)               # no directed edge twice
    return int((cnt == 1).sum()), int((cnt > 2).sum()), len(np.unique(f)) - len(und) + len(f), oriented


def closed_rings(r):
    """per vertex the set of itself and its ring, from a round's CSR arrays"""
    rs, rl, nbr = r["row_start"], r["row_len"], r["nbr"]
    return [set(nbr[rs[w]:rs[w] + rl[w]].tolist()) | {w} for w in range(len(rl))]


def check_independent(r, what):
    """no two applied (and no two selected) edges of a round have endpoints within each other's closed rings"""
    rings = closed_rings(r)
    rs = r["row_start"]
    for flags in ("selected", "applied"):
        ends = []
        for i in np.nonzero(r[flags])[0]:
            u = int(np.searchsorted(rs, i, side="right") - 1)
            ends.append((u, int(r["nbr"][i])))
        near = [rings[u] | rings[v] for u, v in ends]
        owner = {}
        for k, zone in enumerate(near):
            for w in zone:
                owner.setdefault(w, []).append(k)
        for k, (u, v) in enumerate(ends):
            for w in (u, v):
                assert owner[w] == [k], (what, flags, "edge", (u, v), "lies in the closed rings of another edge of the round")


def check_rounds(name, faces_in, nv, rounds, what):
    """the invariants of every round of a run (the oracle's, or the device's taken back to numpy)"""
    before = edge_stats(faces_in, nv)
    for r, after in rounds:
        check_independent(r, what)
        assert r["live_before"] - r["live"] == 2 * r["applied_edges"], (what, r["live_before"], r["live"], r["applied_edges"])
        assert ((r["applied"] <= r["selected"]) & (r["selected"] <= (r["edge"] == O.EDGE_OK))).all(), what
        if name in CLOSED:
            now = edge_stats(after["faces"], nv)
            assert now[:2] == (0, 0) and now[2] == before[2] and now[3], (what, before, now)


def frac(a):
    return [[Fraction(float(x)) for x in row] for row in np.asarray(a)]


# ---- the checks -----------------------------------------------------------------------------------------------------------
ROUND_ARRAYS = ("row_start", "row_len", "nbr", "mult", "locked", "edge", "key", "best1", "best2", "selected", "applied", "remap")
ROUND_COUNTS = ("locked_vertices", "candidates", "reject_cost", "reject_link", "reject_flip", "paths", "selected_edges", "applied_edges", "max_cost", "live", "live_before")


def device_state(s):
    return {"verts": host(s["verts"]), "faces": host(s["faces"]), "quad": host(s["quad"]), "members": host(s["members"]), "csum": None if s["csum"] is None else host(s["csum"])}


def same_state(got, want, what):
    alive = want["members"] > 0                                   # a vertex that was merged away keeps what it held; nobody reads it
    assert np.array_equal(got["members"], want["members"]), (what, "members")
    assert same_bits(got["verts"][alive], want["verts"][alive]) and same_bits64(got["quad"][alive], want["quad"][alive]), (what, "positions or quadrics")
    assert np.array_equal(got["faces"], want["faces"]), (what, "faces")
    assert (want["csum"] is None) == (got["csum"] is None) and (want["csum"] is None or np.array_equal(got["csum"][alive], want["csum"][alive])), (what, "colour sums")


def device_round(dev, r):
    out = {k: host(r[k]) for k in ROUND_ARRAYS}
    for k in ("key", "best1", "best2"):
        out[k] = out[k].view(np.uint64)
    out.update({k: r[k] for k in ROUND_COUNTS})
    return out


def check_case(dev, name, k, twice=False):
    """option set k of the case: the state after begin and after every round, what every round decides, the final mesh and the stats
    equal to the oracle's in every bit; the invariants on both"""
    v, f, rgb = case(name)
    opts = CASES[name][1][k]
    what = (name, opts)
    wv, wf, wc, wstats, wrun = reference(name, k)
    known = dict(KNOWN.get(name, {}) if k == 0 else {}, **KNOWN_BY_OPTION.get((name, k), {}))
    for key, value in known.items():
        assert value(wstats[key]) if callable(value) else wstats[key] == value, (what, key, wstats[key])
    check_rounds(name, f, len(v), wrun["rounds"], what)
    # round by round
    tv, tf, tc = to_dev(dev, v, f, rgb)
    s = MS.begin(tv, tf, tc)
    same_state(device_state(s), wrun["first"], (what, "begin"))
    assert s["live"] == wstats["valid_faces_in"] and s["frame"] == O.frame(*O.bounds(v)), what
    got_rounds = []
    for n, (wr, wafter) in enumerate(wrun["rounds"]):
        gr = device_round(dev, MS.round(s, wstats["target_faces"], wstats["max_error"]))
        entries = int(wr["row_start"][-1])                        # the CSR entries in use: what lies behind them is never read
        for key in ROUND_ARRAYS:
            used = entries if key in ("nbr", "mult") else len(wr[key])
            assert np.array_equal(gr[key][:used], wr[key][:used]), (what, "round", n, key)
        for key in ROUND_COUNTS:
            assert gr[key] == wr[key], (what, "round", n, key, gr[key], wr[key])
        after = device_state(s)
        same_state(after, wafter, (what, "round", n))
        got_rounds.append((gr, after))
    check_rounds(name, f, len(v), got_rounds, (what, "device"))
    # the whole call
    gv, gf, gc, gstats = MS.simplify(tv, tf, tc, **opts)
    print(f"{name} {opts}: {gstats}")
    assert gv.dtype == torch.float32 and gf.dtype == torch.int32 and gc.dtype == torch.uint8
    assert gstats == wstats, (what, gstats, wstats)
    assert same_bits(host(gv), wv) and np.array_equal(host(gf), wf) and np.array_equal(host(gc), wc), what
    assert torch.equal(tv.view(torch.int32), torch.from_numpy(v.copy()).view(torch.int32).to(tv.device)) and torch.equal(tf, torch.from_numpy(f.copy()).to(tf.device)), (what, "the input was written")
    plain = MS.simplify(tv, tf, None, **opts)
    assert plain[2] is None and plain[3] == gstats and torch.equal(plain[0].view(torch.int32), gv.view(torch.int32)) and torch.equal(plain[1], gf), what
    if twice:
        again = MS.simplify(*to_dev(dev, v, f, rgb), **opts)
        assert again[3] == gstats and torch.equal(again[0].view(torch.int32), gv.view(torch.int32)) and torch.equal(again[1], gf) and torch.equal(again[2], gc), what
    return gv, gf, gc, gstats


def check_untouched_vertices(dev):
    """a vertex no collapse touched is a copy in every bit, and the survivors keep their input order"""
    v, f, rgb = case("nonfinite")
    gv, gf, gc, stats = MS.simplify(*to_dev(dev, v, f, rgb), ratio=0.5, drop_unreferenced=False)
    _, _, _, _, run = O.simplify(v, f, rgb, ratio=0.5, drop_unreferenced=False)
    touched = np.zeros(len(v), bool)
    for r, _ in run["rounds"]:
        for i in np.nonzero(r["applied"])[0]:
            touched[[int(np.searchsorted(r["row_start"], i, side="right") - 1), int(r["nbr"][i])]] = True
    alive = run["rounds"][-1][1]["members"] > 0
    assert stats["vertices_out"] == alive.sum() and (~touched).sum() > 10
    at = np.cumsum(alive) - 1
    keep = alive & ~touched
    assert same_bits(host(gv)[at[keep]], v[keep]) and np.array_equal(host(gc)[at[keep]], rgb[keep])


def check_refusals(dev):
    """bad arguments of the module, by name"""
    tv, tf, tc = to_dev(dev, *case("octahedron"))
    nan = float("nan")
    for kw, pattern in (({}, "exactly one"), ({"target_faces": 4, "ratio": 0.5}, "exactly one"), ({"target_faces": -1}, "target_faces"), ({"target_faces": 1.5}, "target_faces"),
                        ({"ratio": -0.1}, "ratio"), ({"ratio": 1.5}, "ratio"), ({"ratio": nan}, "ratio"), ({"ratio": 0.5, "max_error": -1.0}, "max_error"),
                        ({"ratio": 0.5, "max_error": nan}, "max_error"), ({"ratio": 0.5, "max_rounds": -1}, "max_rounds"), ({"ratio": 0.5, "max_rounds": 2.5}, "max_rounds")):
        try:
            MS.simplify(tv, tf, tc, **kw)
        except _lib.RcmvsError as e:
            assert pattern in str(e), (kw, str(e))
        else:
            raise AssertionError(f"{kw} was accepted")
    for bad in ((tv.double(), tf, None), (tv, tf.long(), None), (tv, tf, tc[:3]), (tv[:, :2], tf, None)):
        try:
            MS.simplify(*bad, ratio=0.5)
        except _lib.RcmvsError:
            pass
        else:
            raise AssertionError("a malformed mesh was accepted")
    for args, pattern in (((5, 0.5), "not both"), ((0, 0.0, 1.0), "needs a target"), ((-3, 0.0), "target_faces"), ((0, 2.0), "ratio")):
        try:
            MS.simplify_options(*args)
        except _lib.RcmvsError as e:
            assert pattern in str(e), (args, str(e))
        else:
            raise AssertionError(f"simplify_options{args} was accepted")
    assert MS.simplify_options() is None and MS.simplify_options(0, 0.0) is None
    assert MS.simplify_options(100) == {"target_faces": 100} and MS.simplify_options(0, 0.25, 1e-6) == {"ratio": 0.25, "max_error": 1e-6}


# ---- known answers ----------------------------------------------------------------------------------------------------------
def check_plane(dev, n=17):
    """the planar n x n grid under max_error = 0, target 0: every output vertex has z = +0.0 in every bit, the rim is untouched, the
    area is the unit square's exactly, and interior vertices have gone"""
    v, f, rgb = case(f"plane_{n}")
    gv, gf, gc, stats = check_case(dev, f"plane_{n}", 0)
    ov, of = host(gv), host(gf)
    assert (ov[:, 2].view(np.uint32) == 0).all(), "a vertex left the plane z = +0.0"
    rim = lambda p: p[(p[:, 0] == 0) | (p[:, 0] == 1) | (p[:, 1] == 0) | (p[:, 1] == 1)]      # noqa: E731
    assert same_bits(rim(ov), rim(v)) and len(rim(v)) == 4 * (n - 1) == stats["locked_vertices"]
    P = frac(ov)
    area2 = sum((P[b][0] - P[a][0]) * (P[c][1] - P[a][1]) - (P[b][1] - P[a][1]) * (P[c][0] - P[a][0]) for a, b, c in of.tolist())
    assert area2 == 2, f"twice the area is {area2}, not 2"
    interior_in, interior_out = len(v) - 4 * (n - 1), len(ov) - 4 * (n - 1)
    print(f"plane_{n}: interior vertices {interior_in} -> {interior_out}, faces {len(f)} -> {len(of)}, rounds {stats['rounds']}, stop {stats['stop']}")
    assert 0 <= interior_out < interior_in and stats["max_cost"] == 0.0 and len(of) < len(f)
    return stats


def on_cube(p):
    """per vertex: it lies exactly on the unit cube's surface"""
    inside = ((p >= 0) & (p <= 1)).all(1)
    return inside & ((p == 0) | (p == 1)).any(1)


def cube_corner_miss(p):
    """the largest distance from a corner of the unit cube to the nearest vertex"""
    corners = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float64)
    return float(np.sqrt(((corners[:, None, :] - p.astype(np.float64)[None]) ** 2).sum(2)).min(1).max())


def check_cube(dev, n=9):
    """the closed unit cube (sides of n x n vertices) under max_error = 0, target 0: the eight corners survive in every bit, every output vertex lies exactly on
    the cube, the signed volume is exactly 1, the mesh stays closed, oriented, manifold, of Euler characteristic 2; clustering at
    no fewer faces misses the corners"""
    from rc_mvsnet_amd import mesh_decimate as MD
    v, f, rgb = case(f"cube_{n}")
    gv, gf, gc, stats = check_case(dev, f"cube_{n}", 0)
    ov, of = host(gv), host(gf)
    corners = {bytes(np.array(c, np.float32).tobytes()) for c in [(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)]}
    assert corners <= {r.tobytes() for r in ov}, "a corner of the cube was lost"
    assert on_cube(ov).all(), "a vertex left the cube's surface"
    P = frac(ov)
    det = lambda a, b, c: (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]))      # noqa: E731
    volume6 = sum(det(P[a], P[b], P[c]) for a, b, c in of.tolist())
    assert volume6 == 6, f"six times the signed volume is {volume6}, not 6"
    assert edge_stats(of, len(ov)) == (0, 0, 2, True)
    assert len(of) < len(f) and stats["max_cost"] == 0.0
    # clustering: the coarsest of these cells that still gives at least as many faces
    tv, tf, tc = to_dev(dev, v, f, rgb)
    chosen = None
    for cell in (0.5, 0.375, 0.25, 0.1875, 0.125):
        cv, cf, _, cstats = MD.decimate(tv, tf, tc, cell=cell)
        if cstats["faces_out"] >= len(of):
            chosen = (cell, cstats["faces_out"], cube_corner_miss(host(cv)))
            break
    assert chosen is not None
    line = f"cube_{n}: collapse {len(f)} -> {len(of)} faces in {stats['rounds']} rounds, corner miss {cube_corner_miss(ov)}; clustering cell {chosen[0]}: {chosen[1]} faces, corner miss {chosen[2]}"
    print(line)
    assert cube_corner_miss(ov) == 0.0 and chosen[2] > 0.0
    return line


# ---- a real extraction ------------------------------------------------------------------------------------------------------
def check_extraction(dev, ratios=(0.5, 0.1)):
    """the two spheres and the speck of mesh_clean_cases.check_extraction at ratio 0.5 and 0.1: equal to the oracle, closed and
    manifold after every round -> per ratio (stats, verts, faces)"""
    verts, faces, rgb = MCC.scene_volume(dev).extract(1)
    v, f, c = host(verts), host(faces), host(rgb)
    before = edge_stats(f, len(v))
    out = {}
    for ratio in ratios:
        wv, wf, wc, wstats, wrun = O.simplify(v, f, c, ratio=ratio)
        gv, gf, gc, gstats = MS.simplify(verts, faces, rgb, ratio=ratio)
        print(f"extraction {ratio}: {gstats}")
        assert gstats == wstats and same_bits(host(gv), wv) and np.array_equal(host(gf), wf) and np.array_equal(host(gc), wc), ratio
        for r, after in wrun["rounds"]:
            now = edge_stats(after["faces"], len(v))
            assert now[:2] == (0, 0) and now[2] == before[2] and r["live_before"] - r["live"] == 2 * r["applied_edges"], (ratio, before, now)
        assert gstats["stop"] == "target" and gstats["faces_out"] in (wstats["target_faces"], wstats["target_faces"] - 1) and edge_stats(wf, len(wv))[:3] == before[:3]
        out[ratio] = (gstats, host(gv), host(gf))
    return out


# ---- end to end -------------------------------------------------------------------------------------------------------------
def check_end_to_end(dev, tmp_path, sparse):
    """mesh_scan(..., simplify_ratio=0.5) on the small scan of tsdf_cases.check_end_to_end, dense or sparse: the PLY is the oracle's
    simplification of the mesh mesh_scan writes without the option, colours included, and the summary carries the stats; without the
    option the PLY and the summary's keys are what they were; after clustering the collapse runs on the clustered mesh"""
    import tsdf_cases as C
    from rc_mvsnet_amd import dtu_io, tsdf_mesh as TM
    pair_folder, out_folder = C.write_scan(tmp_path)
    raw, again, ply, both = (str(tmp_path / "out" / n) for n in ("raw.ply", "again.ply", "simplified.ply", "both.ply"))
    kw = dict(resolution=32, device=dev, sparse=sparse)
    plain = TM.mesh_scan(pair_folder, out_folder, out_folder, raw, C.PROB, C.NCONS, C.DIST, C.DEPTH, **kw)
    off = TM.mesh_scan(pair_folder, out_folder, out_folder, again, C.PROB, C.NCONS, C.DIST, C.DEPTH, simplify_faces=0, simplify_ratio=0.0, **kw)
    assert open(raw, "rb").read() == open(again, "rb").read() and dict(off, mesh=raw) == plain and "simplify" not in plain
    summary = TM.mesh_scan(pair_folder, out_folder, out_folder, ply, C.PROB, C.NCONS, C.DIST, C.DEPTH, simplify_ratio=0.5, **kw)
    assert set(summary) == set(plain) | {"simplify"}
    verts, faces, rgb = dtu_io.read_ply_mesh_rgb(raw)
    wv, wf, wc, wstats, _ = O.simplify(verts, faces, rgb, ratio=0.5, keep_rounds=False)
    gv, gf, gc = dtu_io.read_ply_mesh_rgb(ply)
    print("end to end:", summary["simplify"])
    assert summary["simplify"] == wstats and 0 < wstats["faces_out"] < wstats["faces_in"]
    assert same_bits(gv, wv) and np.array_equal(gf, wf) and np.array_equal(gc, wc)
    assert summary["vertices"] == len(gv) == wstats["vertices_out"] and summary["faces"] == len(gf) == wstats["faces_out"]
    assert {k: v for k, v in summary.items() if k not in ("simplify", "mesh", "vertices", "faces", "unreferenced_vertices")} == \
           {k: v for k, v in plain.items() if k not in ("mesh", "vertices", "faces", "unreferenced_vertices")}
    two = TM.mesh_scan(pair_folder, out_folder, out_folder, both, C.PROB, C.NCONS, C.DIST, C.DEPTH, decimate_voxels=1.5, simplify_ratio=0.5, **kw)
    assert list(two).index("decimate") < list(two).index("simplify") and two["simplify"]["faces_in"] == two["decimate"]["faces_out"] > two["simplify"]["faces_out"]
    try:
        TM.mesh_scan(pair_folder, out_folder, out_folder, both, C.PROB, C.NCONS, C.DIST, C.DEPTH, simplify_faces=10, simplify_ratio=0.5, **kw)
    except _lib.RcmvsError as e:
        assert "not both" in str(e)
    else:
        raise AssertionError("two targets were accepted")
    return pair_folder, out_folder, summary
