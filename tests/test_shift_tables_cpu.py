"""The planner is shift-equivariant (no GPU): the host plan of a list moved by (df, dk) holds exactly what tests/shift_util.py's
expected_clone derives from the host plan of the list itself — over every table, on every layout the planner has.  That is what
lets tests/test_gpu_shift_tables.py compare a shifted CLONE (csrc/plan_pack.hip) with a freshly planned plan of the moved list;
and expected_clone itself is checked here on bitmaps made by hand."""
import numpy as np
import pytest

import shift_util as su
from batrack_amd.plan import PLAN_ARRAYS, Plan


def host_plan(ii, jj, kk, n_buf, p_tot, fixedp):
    return Plan(ii, jj, kk, n_buf, p_tot, fixedp, upload=False)


@pytest.mark.parametrize("name", list(su.FIXTURES))
def test_the_plan_of_a_moved_list_is_the_moved_plan(name):
    fx = su.fixture(name)
    df = 3
    dk = df * fx.M
    a = host_plan(fx.ii, fx.jj, fx.kk, fx.n_buf, fx.p_tot, fx.fixedp)
    A = a.arrays()
    assert fx.layout(A, a.info), (name, {k: a.info[k] for k in ("n", "m", "tiles", "slots", "pairs", "nnz_blocks")})
    ii, jj, kk, fixedp = su.moved(fx, df)
    b = host_plan(ii, jj, kk, fx.n_buf, fx.p_tot, fixedp)
    B = b.arrays()
    assert fx.layout(B, b.info)
    want = su.expected_clone(A, df, dk)
    assert su.differing(want, B, PLAN_ARRAYS, mask_from=B) == []
    assert {k: v for k, v in a.info.items() if k not in su.INFO_MOVES} == {k: v for k, v in b.info.items() if k not in su.INFO_MOVES}
    assert b.info["fixedp"] == a.info["fixedp"] + df and b.info["n_all"] == a.info["n_all"] + df
    assert fx.n_buf >= a.info["n_all"] + su.SLACK and su.max_shift(fx) >= 3


def test_the_largest_shift_is_bounded_by_either_buffer():
    assert su.max_shift(su.fixture("tile")) == su.SLACK                       # the pose buffer
    fx = su.fixture("loose")
    assert su.max_shift(fx) == 7 < fx.n_buf - (int(max(fx.ii.max(), fx.jj.max())) + 1)      # the patch buffer


U = lambda *w: np.array(w, np.uint32)


def test_expected_bitmap_by_hand():
    e = lambda bits, dk: su.expected_clone({"act_bits": bits, "act_rank": su.rank_of(bits)}, 0, dk)
    # bit 31 of word 0 moved by 1: bit 0 of word 1
    r = e(U(0x80000000, 0, 0), 1)
    assert r["act_bits"].tolist() == [0, 1, 0] and r["act_rank"].tolist() == [0, 0, 1]
    # ... by 31: bit 30 of word 1; bit 0 by 31: bit 31 of word 0
    r = e(U(0x80000001, 0, 0), 31)
    assert r["act_bits"].tolist() == [0x80000000, 0x40000000, 0] and r["act_rank"].tolist() == [0, 1, 2]
    # a multiple of 32: whole words move, nothing crosses a word
    r = e(U(0x80000001, 0x00010000, 0, 0), 64)
    assert r["act_bits"].tolist() == [0, 0, 0x80000001, 0x00010000] and r["act_rank"].tolist() == [0, 0, 0, 2]
    # onto the last bit of the bitmap, and one further: gone
    r = e(U(0x5, 0), 61)
    assert r["act_bits"].tolist() == [0, 0xA0000000] and r["act_rank"].tolist() == [0, 0]
    assert e(U(0x5, 0), 62)["act_bits"].tolist() == [0, 0x40000000]
    assert e(U(0x5, 0), 64)["act_bits"].tolist() == [0, 0]
    # against a bit-by-bit statement, over many words
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 1 << 32, 70, dtype=np.uint64).astype(np.uint32)
    bits[40:] = 0
    for dk in (0, 1, 31, 32, 33, 95, 960):
        flat = np.unpackbits(bits.view(np.uint8), bitorder="little")
        moved = np.concatenate([np.zeros(dk, np.uint8), flat])[:flat.size]
        r = e(bits, dk)
        assert np.array_equal(r["act_bits"], np.packbits(moved, bitorder="little").view(np.uint32))
        assert np.array_equal(r["act_rank"], np.concatenate([[0], np.cumsum(moved.reshape(-1, 32).sum(1))[:-1]]))
        p = np.flatnonzero(moved)
        assert np.array_equal(su.track_of(r["act_bits"], r["act_rank"], p), np.arange(p.size))


def test_expected_index_tables_by_hand():
    src = {"kx": np.array([3, 9], np.int32), "tile_kx": np.array([3, 9, -1, -1], np.int32), "tile_ij": np.array([2 | 5 << 16, 0], np.int32),
           "pair_i": np.array([2], np.int32), "pair_j": np.array([5], np.int32), "tile_npair": np.array([1], np.int32),
           "edge_words": su.edge_words([2, 2], [5, 5], [3, 9]), "slot_edge": np.array([1, 0, -1], np.int32),
           "trk_of_patch": np.array([-1, -1, -1, 0, -1, -1, -1, -1, -1, 1, -1, -1, -1, -1, -1, -1], np.int32)}
    r = su.expected_clone(src, 2, 4)
    assert r["kx"].tolist() == [7, 13] and r["tile_kx"].tolist() == [7, 13, -1, -1]
    assert r["tile_ij"].tolist() == [4 | 7 << 16, 2 | 2 << 16]
    assert r["pair_i"].tolist() == [4] and r["pair_j"].tolist() == [7] and r["slot_edge"].tolist() == [1, 0, -1]
    assert np.array_equal(r["edge_words"], su.edge_words([4, 4], [7, 7], [7, 13]))
    assert np.flatnonzero(r["trk_of_patch"] >= 0).tolist() == [7, 13]
    assert su.valid_mask(src, "tile_ij").tolist() == [True, False] and su.valid_mask(src, "tile_kx").all()
    assert su.differing(r, dict(r, tile_ij=np.array([4 | 7 << 16, 0], np.int32)), ["tile_ij"], mask_from=r) == []
    assert su.differing(r, dict(r, tile_ij=np.array([4 | 7 << 16, 0], np.int32)), ["tile_ij"]) != []
