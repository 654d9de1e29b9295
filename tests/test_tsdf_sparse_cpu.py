"""The block-sparse TSDF volume, oracle and host logic only (no kernel runs here): the marking rule's cases hit what they are
there for, the theorem -- with no skipped pixel the sparse mesh is the dense mesh in another order -- on the two oracles, the
oracle's own re-ordering, the grid planning and the header's tables."""
import numpy as np
import pytest

import tsdf_cases as C
import tsdf_oracle as O
import tsdf_sparse_cases as SC
import tsdf_sparse_oracle as S
from rc_mvsnet_amd import _lib, tsdf_mesh as TM


def test_header_constants_and_entry_points():
    want = {"BLOCK": 8, "MAX_BLOCKS": 1 << 27, "MAX_ACTIVE": 1 << 19, "MARK_SPAN": 4}
    assert all(_lib.CONSTANTS["RCMVS_TSDF_SP_" + k] == v for k, v in want.items())
    assert (S.BLOCK, S.MARK_SPAN) == (want["BLOCK"], want["MARK_SPAN"]) and _lib.CONSTANTS["RCMVS_VERSION"] == 106
    assert any(p.endswith("tsdf_sparse.h") for p in _lib.EXT_HEADERS)
    for name in ("mark", "build", "integrate", "mesh_count", "mesh_emit"):
        a, b = _lib.EXT_SIGNATURES["rcmvs_tsdf_sp_" + name], _lib.EXT_SIGNATURES["rcmvs_tsdf_sp_" + name + "_timed"]
        assert b[:len(a) - 1] == a[:-1] and len(b) == len(a) + 2                  # the twin takes two events before the stream


@pytest.mark.parametrize("name", list(SC.SCENES))
def test_theorem_on_the_two_oracles(name):
    sp = SC.check_scene_on_the_oracles(name)
    assert sp["faces"].min() >= 0 and sp["faces"].max() < len(sp["verts"])


def test_oracle_mark_of_every_case_is_deterministic_and_in_range():
    for name in SC.MARK:
        flags, skipped = SC.mark_reference(name)
        assert flags.shape == (80,) and set(np.unique(flags)) <= {0, 1} and skipped >= 0


def test_oracle_build():
    for name, (bdims, blocks) in SC.BUILD.items():
        flags = np.zeros(bdims[0] * bdims[1] * bdims[2], np.uint8)
        flags[list(blocks)] = 1
        mask_words, word_rank, active = S.build(flags)
        bits = [(int(mask_words[b >> 5]) >> (b & 31)) & 1 for b in range(len(flags))]
        assert bits == list(flags) and int(word_rank[-1]) == len(active) == int(flags.sum())
        for slot, b in enumerate(int(x) for x in active):                                            # the slot lookup of the contract
            assert int(word_rank[b >> 5]) + bin(int(mask_words[b >> 5]) & ((1 << (b & 31)) - 1)).count("1") == slot


def test_oracle_reordering_is_the_identity_when_one_block_is_the_grid():
    """bdims (1, 1, 1): the allocated order is the dense order, so the sparse oracle must return the dense oracle's mesh as it is"""
    f = C.sphere_field((8, 8, 8), C.UNIT, (3.7, 4.2, 3.9), 2.6)
    state = {"dsum": f.astype(np.float32).ravel(), "wsum": np.ones(512, np.float32), "csum": None}
    want = O.extract(state["dsum"], state["wsum"], None, C.UNIT, (8, 8, 8), 1)
    got = S.extract(state, C.UNIT, (1, 1, 1), [0], 1)
    assert np.array_equal(S.voxel_of_alloc((1, 1, 1), [0]), np.arange(512))
    assert all(np.array_equal(got[k], want[k]) for k in ("verts", "faces", "edge_mask", "tri_count", "vert_start", "tri_start"))


def test_extraction_cases_hit_what_they_are_there_for():
    eight = SC.extract_reference("sphere_on_the_corner_of_8")
    ok, euler = O.closed_and_oriented(eight["faces"])
    assert ok and euler == 2
    assert not O.closed_and_oriented(SC.extract_reference("sphere_7_of_8")["faces"])[0]
    assert len(SC.extract_reference("all_inside")["faces"]) == 0


def test_plan_sparse_grid():
    origin, voxel, bdims, trunc = TM.plan_sparse_grid([0.0, 1.0, 2.0], [48.0, 25.0, 14.0], resolution=48)
    assert voxel == 1.0 and trunc == 3.0 and origin == [-3.0, -2.0, -1.0] and bdims == [7, 4, 3]         # 54 x 30 x 18 voxels, rounded up
    origin, voxel, bdims, trunc = TM.plan_sparse_grid([0.0, 1.0, 2.0], [48.0, 25.0, 14.0], voxel=0.5, trunc_voxels=2.0, pad=False)
    assert origin == [0.0, 1.0, 2.0] and bdims == [12, 6, 3] and trunc == 1.0
    assert TM.plan_sparse_grid([0, 0, 0], [1, 1, 1])[1] == 1.0 / 1024                                     # the default resolution
    assert TM.plan_sparse_grid([0, 0, 0], [4096, 4096, 4096], voxel=1.0, pad=False)[2] == [512, 512, 512]  # exactly 2^27 blocks
    for bad in (dict(lo=[0, 0, 0], hi=[1, 1, float("nan")]), dict(lo=[0, 0, 0], hi=[1, -1, 1]), dict(lo=[0, 0, 0], hi=[0, 0, 0]),
                dict(lo=[0, 0, 0], hi=[1, 1, 1], voxel=0.0), dict(lo=[0, 0, 0], hi=[4097, 4096, 4096], voxel=1.0, pad=False),
                dict(lo=[0, 0, 0], hi=[1, 1, 1], voxel=1e-30)):
        with pytest.raises(_lib.RcmvsError):
            TM.plan_sparse_grid(**bad)
    with pytest.raises(_lib.RcmvsError, match="bdims"):
        TM.SparseTsdfVolume((0, 0, 0), 1.0, (1 << 10, 1 << 10, 1 << 8), "cpu")
    with pytest.raises(_lib.RcmvsError, match="voxel"):
        TM.SparseTsdfVolume((0, 0, 0), 0.0, (1, 1, 1), "cpu")
