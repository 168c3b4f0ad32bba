"""-m gpu: the tables of shifted clones (bt_plan_create_shifted{,_any,_spec}, bt_plan_preshift + bt_plan_spec_bind), read back
from the clone's device buffer and compared entry for entry — integer equality, no tolerance — with tests/shift_util.py's
expected_clone (what the shift kernels of csrc/plan_pack.hip must make of the SOURCE plan's tables) and, under valid_mask, with
the plan bt_plan_create builds for the moved list (tests/test_shift_tables_cpu.py: the planner is shift-equivariant on these
lists).  Every layout the planner has is cloned, through every entry point; k_act_shift, the frame fields of tile_ij and the
verdict kernels are taken to their limits.  The table comparisons come first in every test: a clone with a wrong table is
never stepped."""
import numpy as np
import pytest
import torch

import shift_util as su
from batrack_amd.plan import Plan, Stepper

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = su.DEVICE_TABLES + ("edge_words",)
ENTRIES = ("shifted", "shifted_any", "spec", "preshift")
FIGURES = ("jacobian_kernel", "edge_precision", "solver_mode", "ws_layout", "workspace_bytes", "info")

T = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.int64), device=DEV)


def tables(plan):
    return {n: plan.array(n) for n in NAMES}


def figures(plan):
    return {f: getattr(plan, f) for f in FIGURES}


def clone(entry, src, lst, n_buf, p_tot, df, sync=True):
    """The clone of `src` for the list lst = (ii, jj, kk, fixedp) (device tensors), df frames on, through one entry point"""
    ii, jj, kk, fixedp = lst
    if entry == "shifted":
        return Plan.shifted(src, ii, jj, kk, n_buf, p_tot, fixedp, sync=sync)
    if entry == "shifted_any":
        pl, matched = Plan.shifted_any([src], ii, jj, kk, n_buf, p_tot, fixedp, sync=sync)
        assert matched is (src if pl is not None else None)
        return pl
    if entry == "spec":
        pl = Plan.shifted_spec(src, ii, jj, kk, n_buf, p_tot, fixedp)
        assert pl is None or pl.speculative
        return pl
    pl = Plan.preshift(src, df)
    if pl is not None:
        assert pl.unbound and pl.bind(ii, jj, kk, n_buf, p_tot, fixedp)
    return pl


def check_tables(pl, want, fresh_tables, lst_np):
    """(a): every table of the clone is expected_clone(source tables) exactly, the fresh plan's under valid_mask, and its packed
    list the new list's"""
    got = tables(pl)
    assert su.differing(got, want, NAMES) == []
    assert su.differing(got, fresh_tables, NAMES, mask_from=fresh_tables) == []
    assert np.array_equal(got["edge_words"], su.edge_words(*lst_np[:3]))
    return got


def step(plan, inp):
    """one pose+structure step -> (poses_out, patches_out, status)"""
    f = lambda a: torch.as_tensor(a, device=DEV)
    poses, patches = f(inp["poses"]), f(inp["patches"])
    st = Stepper(plan, DEV)
    P, X = torch.empty_like(poses), torch.empty_like(patches)
    st.step(poses, patches, f(inp["mono"]), f(inp["intrinsics"]), f(inp["targets3"]), 3, f(inp["weights"]), P, X,
            list(inp["bounds"]), 1e-4, 10.0, 0.05, "huber", False)
    torch.cuda.synchronize()
    return P.cpu().numpy(), X.cpu().numpy(), st.status(), inp["poses"]


def same_step(a, b):
    """the gates of tests/test_gpu_shifted_plan.py: status 0, rel 1e-6 (two executions: the float64 atomics' order), a real step"""
    rel = lambda x, y: np.linalg.norm(x.astype(np.float64) - y) / np.linalg.norm(y)
    assert a[2] == b[2] == 0
    assert rel(a[0], b[0]) < 1e-6 and rel(a[1], b[1]) < 1e-6
    assert np.abs(a[0] - a[3]).max() > 0


def source(fx):
    src = Plan(T(fx.ii), T(fx.jj), T(fx.kk), fx.n_buf, fx.p_tot, fx.fixedp)
    route = (src.jacobian_kernel, src.solver_mode, src.built_on_device)
    assert route == (fx.kernel, fx.solver, fx.device), (fx.name, route, src.info)
    return src


def moved_lists(fx, df, dk=None):
    lst_np = su.moved(fx, df, dk)
    return lst_np, tuple(T(a) for a in lst_np[:3]) + (lst_np[3],)


# ------------------------------------------------------------------ (a) every layout, every entry point
@pytest.mark.parametrize("name", list(su.FIXTURES))
def test_clone_tables_of_every_layout_through_every_entry_point(name):
    fx = su.fixture(name)
    src = source(fx)
    A = tables(src)
    assert A["edge_words"].size == fx.ii.size and np.array_equal(A["edge_words"], su.edge_words(fx.ii, fx.jj, fx.kk))
    stepped = None
    for df in (1, 3, su.max_shift(fx)):
        dk = df * fx.M
        lst_np, lst = moved_lists(fx, df)
        fresh = Plan(*lst[:3], fx.n_buf, fx.p_tot, lst[3])
        F, want = tables(fresh), su.expected_clone(A, df, dk)
        for entry in (ENTRIES if df <= 3 else ("preshift",)):
            pl = clone(entry, src, lst, fx.n_buf, fx.p_tot, df)
            assert pl is not None, (entry, df)
            check_tables(pl, want, F, lst_np)
            assert pl.confirm() and not pl.__dict__.get("speculative")
            assert figures(pl) == figures(fresh), (entry, df)
            if stepped is None and entry == "shifted":                       # one step per fixture, behind the table comparisons
                inp = su.step_inputs(*lst_np[:3], fx.n_buf, fx.p_tot, seed=3)
                stepped = step(pl, inp), step(fresh, inp)
            pl.close()
        fresh.close()
    same_step(*stepped)
    # one frame beyond the largest shift fits neither buffer
    assert Plan.preshift(src, su.max_shift(fx) + 1) is None


def test_the_stream_kernel_steps_alike_every_time():
    """What the comparison of two plans' steps rests on, on the one fixture where it did not hold: k_stream's two waves flushed
    their register accumulators through the row and pair lists of the PREVIOUS cameras while the first wave to finish already
    wrote the next tile's (no barrier in between) — on this list (few cameras, hot rows of S, tiles that run across source
    frames) two steps of ONE plan differed by 6e-3 in the poses, most times.  Float64 atomics in another order: 1e-9."""
    fx = su.fixture("stream")
    src = source(fx)
    inp = su.step_inputs(fx.ii, fx.jj, fx.kk, fx.n_buf, fx.p_tot, seed=3)
    first = step(src, inp)
    for _ in range(5):
        same_step(step(src, inp), first)


# ------------------------------------------------------------------ (b) clones of clones
@pytest.mark.parametrize("name", ["tile", "etile_dev"])
def test_five_generations_through_mixed_entry_points(name):
    fx = su.fixture(name)
    src = source(fx)
    A = tables(src)
    n_buf, p_tot = fx.n_buf, fx.p_tot
    at = lambda cum: moved_lists(fx, cum)[1]
    c1 = clone("shifted", src, at(1), n_buf, p_tot, 1)
    # an unbound clone is no source, an unconfirmed one neither
    unbound = Plan.preshift(c1, 2)
    assert unbound is not None and Plan.preshift(unbound, 1) is None and Plan.shifted(unbound, *at(4)[:3], n_buf, p_tot, at(4)[3]) is None
    assert Plan.shifted_spec(unbound, *at(4)[:3], n_buf, p_tot, at(4)[3]) is None
    assert unbound.bind(*at(3)[:3], n_buf, p_tot, at(3)[3])
    assert Plan.preshift(unbound, 1) is None and Plan.shifted(unbound, *at(4)[:3], n_buf, p_tot, at(4)[3]) is None      # bound, not confirmed
    assert Plan.shifted_spec(unbound, *at(4)[:3], n_buf, p_tot, at(4)[3]) is None
    assert unbound.confirm()
    c2 = unbound
    c3 = clone("spec", c2, at(4), n_buf, p_tot, 1)
    assert c3 is not None and Plan.preshift(c3, 1) is None and Plan.shifted(c3, *at(6)[:3], n_buf, p_tot, at(6)[3]) is None
    assert Plan.shifted_any([c3], *at(6)[:3], n_buf, p_tot, at(6)[3]) == (None, None)
    assert c3.confirm()
    c4, matched = Plan.shifted_any([c3, c2, c1], *at(6)[:3], n_buf, p_tot, at(6)[3])
    assert c4 is not None and matched is c3
    c5 = clone("preshift", c4, at(7), n_buf, p_tot, 1)
    assert c5 is not None and c5.confirm()
    lst_np, lst = moved_lists(fx, 7)
    fresh = Plan(*lst[:3], n_buf, p_tot, lst[3])
    F = tables(fresh)
    check_tables(c5, su.expected_clone(A, 7, 7 * fx.M), F, lst_np)
    assert figures(c5) == figures(fresh)
    # a clone made ahead of its list can be read before it is bound, the last frame of the buffers included
    c6 = Plan.preshift(c5, 1)
    assert c6 is not None and c6.unbound and Plan.preshift(c5, 2) is None
    lst_np, lst = moved_lists(fx, 8)
    fresh8 = Plan(*lst[:3], n_buf, p_tot, lst[3])
    check_tables(c6, su.expected_clone(A, 8, 8 * fx.M), tables(fresh8), lst_np)
    # and the sources are what they were
    assert su.differing(tables(src), A, NAMES) == [] and su.differing(tables(c5), su.expected_clone(A, 7, 7 * fx.M), NAMES) == []
    inp = su.step_inputs(*moved_lists(fx, 7)[0][:3], n_buf, p_tot, seed=5)
    same_step(step(c5, inp), step(fresh, inp))


# ------------------------------------------------------------------ (c) the bitmap kernel
def bitmap_list(p_tot, per):
    """300 tracks in 8 frames: at bits 0 and 31 of a word, across the word boundary, in the last word of a thread's chunk of `per`
    words and the first of the next, the rest anywhere in the lower half of the buffer"""
    rng = np.random.default_rng(p_tot)
    nwords = (p_tot + 31) // 32
    fixed = np.unique([0, 31, 32, 63, 32 * per - 1, 32 * per, 32 * (2 * per - 1) + 31, 32 * 2 * per, 32 * (nwords // 2) - 1])
    rest = rng.choice(np.setdiff1d(np.arange(p_tot // 2), fixed), 300 - fixed.size, replace=False)
    kx = np.unique(np.concatenate([fixed, rest]))
    assert kx.size == 300
    kk = np.repeat(kx, 3)
    ii = kk % 4
    jj = ii + np.tile(np.arange(1, 4), kx.size)
    return ii.astype(np.int64), jj.astype(np.int64), kk.astype(np.int64)


BITMAP_SIZES = {1024: 32768, 1025: 32769, 8192: 8192 * 32 - 7}         # words of the bitmap -> p_tot
_BITMAP = {}


def bitmap_source(nwords):
    """(source plan, its tables, its list): one per size, shared by the cases"""
    if nwords not in _BITMAP:
        p_tot = BITMAP_SIZES[nwords]
        per = (nwords + 1023) // 1024
        ii, jj, kk = bitmap_list(p_tot, per)
        src = Plan(T(ii), T(jj), T(kk), 16, p_tot, 1)
        A = tables(src)
        assert A["act_bits"].size == nwords and per == {1024: 1, 1025: 2, 8192: 8}[nwords]
        _BITMAP[nwords] = (src, A, (ii, jj, kk), p_tot, per)
    return _BITMAP[nwords]


@pytest.mark.parametrize("nwords", list(BITMAP_SIZES))
@pytest.mark.parametrize("dk", ["1", "31", "32", "33", "32per", "32per+1", "last"])
def test_track_bitmap_moved_by_every_kind_of_shift(nwords, dk):
    """k_act_shift: per = 1 | 2 with idle tail threads (1025 words: 513 threads have work) | 8; bit remainders 1 and 31, none with
    a word offset, carries across a thread's chunk, the highest bit onto the bitmap's last"""
    src, A, (ii, jj, kk), p_tot, per = bitmap_source(nwords)
    dk = {"1": 1, "31": 31, "32": 32, "33": 33, "32per": 32 * per, "32per+1": 32 * per + 1, "last": p_tot - 1 - int(kk.max())}[dk]
    df = 0 if dk == 1 else 1                                   # (bt_plan_create_shifted takes any dk >= 0 with any df)
    lst_np = (ii + df, jj + df, kk + dk, 1 + df)
    lst = tuple(T(a) for a in lst_np[:3]) + (lst_np[3],)
    pl = Plan.shifted(src, *lst[:3], 16, p_tot, lst[3])
    assert pl is not None
    fresh = Plan(*lst[:3], 16, p_tot, lst[3])
    got = check_tables(pl, su.expected_clone(A, df, dk), tables(fresh), lst_np)
    assert figures(pl) == figures(fresh)
    kx = fresh.array("kx")
    assert np.array_equal(su.track_of(got["act_bits"], got["act_rank"], kx), np.arange(kx.size))
    assert int(su.popcount32(got["act_bits"]).sum()) == kx.size == 300
    if dk == p_tot - 1 - int(kk.max()):
        assert got["act_bits"][-1] >> ((p_tot - 1) & 31) == 1
    # one patch further and the list leaves the buffer: an error, like bt_plan_create's
    if dk == p_tot - 1 - int(kk.max()):
        with pytest.raises(RuntimeError):
            Plan.shifted(src, lst[0], lst[1], lst[2] + 1, 16, p_tot, lst[3])


# ------------------------------------------------------------------ (d) the frame fields
def test_frame_fields_at_the_last_frame_of_the_largest_buffer():
    from batrack_amd import graphgen
    n_buf, M = 32768, 64
    g = graphgen.make_graph(12, M, 6, seed=4)
    fx = su.Fixture("n_buf_32768", g.ii, g.jj, g.kk, n_buf, n_buf * M, 2, M, "k_tile", 0, True, None)
    src = Plan(T(fx.ii), T(fx.jj), T(fx.kk), fx.n_buf, fx.p_tot, fx.fixedp)
    A = tables(src)
    df = n_buf - 12
    assert su.max_shift(fx) == df
    lst_np, lst = moved_lists(fx, df)
    fresh = Plan(*lst[:3], fx.n_buf, fx.p_tot, lst[3])
    F, want = tables(fresh), su.expected_clone(A, df, df * M)
    assert (want["tile_ij"] >> 16).max() == 32767 == want["pair_j"].max() and want["kx"].max() == fx.p_tot - 1
    stepped = None
    for entry in ENTRIES:
        pl = clone(entry, src, lst, fx.n_buf, fx.p_tot, df)
        assert pl is not None, entry
        check_tables(pl, want, F, lst_np)
        assert pl.confirm() and figures(pl) == figures(fresh)
        if stepped is None:
            inp = su.step_inputs(*lst_np[:3], fx.n_buf, fx.p_tot, seed=3)
            stepped = step(pl, inp), step(fresh, inp)
    same_step(*stepped)
    # one frame more fits no buffer
    beyond_np, beyond = moved_lists(fx, df + 1)
    assert Plan.preshift(src, df + 1) is None
    assert Plan.shifted_spec(src, *beyond[:3], fx.n_buf, fx.p_tot, beyond[3]) is None
    with pytest.raises(RuntimeError):                                  # (its list names frame 32768: an index out of range)
        Plan.shifted(src, *beyond[:3], fx.n_buf, fx.p_tot, beyond[3])
    pl = clone("shifted", src, lst, fx.n_buf, fx.p_tot, df)
    check_tables(pl, want, F, lst_np)


# ------------------------------------------------------------------ (e) the verdicts
class Verdicts:
    """A list of E edges (tracks of 5 observations, cut to length), its plan, and what a correct clone one frame on must hold"""
    def __init__(self, E):
        from batrack_amd import graphgen
        g = graphgen.make_graph(16, 64, 5, seed=8)
        self.n_buf, self.M, self.df = 24, 64, 1
        self.p_tot = self.n_buf * self.M
        self.ii, self.jj, self.kk = (np.ascontiguousarray(a[:E], np.int64) for a in (g.ii, g.jj, g.kk))
        assert self.ii.size == E
        self.src = Plan(T(self.ii), T(self.jj), T(self.kk), self.n_buf, self.p_tot, 1)
        self.good_np = (self.ii + 1, self.jj + 1, self.kk + self.M, 2)
        self.good = tuple(T(a) for a in self.good_np[:3]) + (2,)
        self.fresh = Plan(*self.good[:3], self.n_buf, self.p_tot, 2)
        self.F = tables(self.fresh)
        self.want = su.expected_clone(tables(self.src), 1, self.M)
        self.rounds = 0

    def altered(self, **delta):
        """the correct list with field[pos] += d for every field=(pos, d)"""
        arrs = dict(ii=self.good_np[0].copy(), jj=self.good_np[1].copy(), kk=self.good_np[2].copy())
        for f, (pos, d) in delta.items():
            arrs[f][pos] += d
        return T(arrs["ii"]), T(arrs["jj"]), T(arrs["kk"])

    def good_clone_passes(self, entry):
        """after a refusal: the correct list still clones through the same entry point, and every table is right"""
        pl = clone(entry, self.src, self.good, self.n_buf, self.p_tot, 1)
        assert pl is not None
        check_tables(pl, self.want, self.F, self.good_np)
        assert pl.confirm() and not pl.__dict__.get("speculative") and not pl.__dict__.get("invalid")
        self.rounds += entry in ("spec", "preshift")

    def refused(self, lst, error):
        """`lst` through the three kinds of verdict: no plan (error: an index out of range — raised, never accepted)"""
        a = (self.n_buf, self.p_tot, 2)
        if error:
            with pytest.raises(RuntimeError):
                Plan.shifted(self.src, *lst, *a)
        else:
            assert Plan.shifted(self.src, *lst, *a) is None
        self.good_clone_passes("shifted")
        for entry in ("spec", "preshift"):
            pl = clone(entry, self.src, lst + (2,), self.n_buf, self.p_tot, 1)
            assert pl is not None and pl.speculative
            if error:
                with pytest.raises(RuntimeError):
                    pl.confirm()
            else:
                assert pl.confirm() is False
            assert pl.invalid and pl.speculative and pl.confirm() is False          # it stays no plan of anything
            self.rounds += 1
            self.good_clone_passes(entry)


@pytest.mark.parametrize("E", [4096, 4097])
def test_one_deviating_edge_anywhere_is_found_out(E):
    """k_shift_match, k_pack_match_expect, k_match_done: E % 256 = 0 and 1; the deviation at edge 0 (whose difference
    k_shift_match takes as the reference), next to it, on either side of a workgroup boundary, at the last edge"""
    v = Verdicts(E)
    for pos in (0, 1, 255, 256, E - 1):
        for field in ("ii", "jj", "kk"):
            v.refused(v.altered(**{field: (pos, 1)}), error=False)
    assert v.rounds > 16                                       # (the sixteen verdict slots were all used again)


@pytest.mark.parametrize("E", [4096, 4097])
def test_a_deviation_that_keeps_the_packed_word_is_an_index_out_of_range(E):
    """jj + 65536 where ii + 1 belongs, ii + 65536 where kk + 1 belongs: the 64-bit word is the moved list's own through the carry
    between its fields, the index is outside the buffers — reported as such by every verdict, never accepted"""
    v = Verdicts(E)
    same_words = lambda lst: all(np.array_equal(pack(*(a.cpu().numpy() for a in lst)), pack(*v.good_np[:3]))
                                 for pack in (su.edge_words, lambda i, j, k: (k << 32) + (i << 16) + j))      # packed by OR, and as a sum
    for pos in (0, 256, E - 1):
        # (the lowest set bit of the upper field, so that the word is the same whether its fields are OR-ed or added)
        c = int(v.good_np[0][pos] & -v.good_np[0][pos])
        lst = v.altered(ii=(pos, -c), jj=(pos, 65536 * c))
        assert c > 0 and same_words(lst)
        v.refused(lst, error=True)
        c = int(v.good_np[2][pos] & -v.good_np[2][pos])
        lst = v.altered(kk=(pos, -c), ii=(pos, 65536 * c))
        assert c > 0 and same_words(lst)
        v.refused(lst, error=True)
    # one index out of range, at the last edge only
    for field, d in (("kk", v.p_tot), ("jj", v.n_buf), ("ii", -v.n_buf)):
        v.refused(v.altered(**{field: (E - 1, d)}), error=True)
    assert v.rounds > 16


# ------------------------------------------------------------------ (f) lifetime
def test_a_clone_outlives_its_source_and_the_sources_buffer():
    fx = su.fixture("tile")
    src = source(fx)
    A = tables(src)
    lst_np, lst = moved_lists(fx, 2)
    fresh = Plan(*lst[:3], fx.n_buf, fx.p_tot, lst[3])
    F, want = tables(fresh), su.expected_clone(A, 2, 2 * fx.M)
    other = su.moved(fx, 5)
    other_t = tuple(T(a) for a in other[:3])
    torch.cuda.synchronize()                                   # (sync=False: the caller vouches for the index tensors)
    for entry in ("shifted", "shifted_any"):
        src = source(fx)
        pl = clone(entry, src, lst, fx.n_buf, fx.p_tot, 2, sync=False)
        src.close()                                            # at once: the copies out of its buffer may still be queued
        again = Plan(*other_t, fx.n_buf, fx.p_tot, other[3])   # a plan of the same size takes the recycled buffer
        assert pl is not None
        check_tables(pl, want, F, lst_np)
        assert figures(pl) == figures(fresh)
        again.close(); pl.close()


def test_plans_that_are_no_source():
    from batrack_amd.parallel import partition_tracks, plan_range
    fx = su.fixture("tile")
    lst_np, lst = moved_lists(fx, 1)
    a = (fx.n_buf, fx.p_tot)
    own = plan_range(partition_tracks(fx.kk, 2)[1], fx.p_tot)
    rank = Plan(T(fx.ii), T(fx.jj), T(fx.kk), *a, fx.fixedp, own=own)
    assert rank.uploaded and rank.E < fx.ii.size
    host = Plan(fx.ii, fx.jj, fx.kk, *a, fx.fixedp, upload=False)
    for src in (rank, host):
        assert Plan.shifted(src, *lst[:3], *a, lst[3]) is None
        assert Plan.shifted_any([src], *lst[:3], *a, lst[3]) == (None, None)
        assert Plan.shifted_spec(src, *lst[:3], *a, lst[3]) is None
        assert Plan.preshift(src, 1) is None
    assert rank.array("edge_words").size == 0 and host.array("edge_words").size == 0
