"""The tracker-iteration kernels at their limits (batrack_amd/csrc/track_iter.hip, include/batrack_track.h): every F, LRR and C
path of k_track_tokens and k_track_apply, token counts around the 16-row tile, more tiles than waves, the sine at arguments of
1e5 rad against a truth at the same float32 argument, guard rows around every buffer of the raw entry points, the reach of a
non-finite value, and the position embedding at coordinates up to FLT_MAX.

Tolerances.  No bound is derived from the kernel under test.  Copies, samples and single adds are compared bit for bit with
the float32 restatement of tests/track_iter_util.py on the same GPU.  Sums are held to the project's convention,
    max |kernel - float64 restatement| <= 2 x max |float32 restatement - float64 restatement|   on the same inputs,
where the maximum is taken over all the calls of one parametrised case: a maximum over a single token's few values is a
noisy estimate of either error, over some thousands of values it is not.  Rows and columns built to make the float32
restatement itself lose digits (a row of mean 1e3 and spread 1e-2; biases that saturate the GELU) are held to the same
convention in a group of their own, so that their wide gate does not cover the ordinary values."""
import numpy as np
import pytest
import torch

import track_iter_util as U
from batrack_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
UNIT = 2.0 ** -24                       # float32 unit roundoff
TOK = ("coords", "coords_sub", "fcorrs", "ffeats", "track_mask", "vis", "pos", "time", "w_flow", "b_flow")
PAR = ("gamma", "beta", "w_u", "b_u")
SCALES = {False: dict(stride=4.0, Dz=24.0, d_range=19.5, d_near=0.5, use_log_depth=False),
          True: dict(stride=4.0, Dz=24.0, d_range=3.7, d_near=-0.7, use_log_depth=True)}


def ti():
    from batrack_amd.frontend import track_iter
    return track_iter


def gen(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return g, lambda *s: torch.randn(*s, device=DEV, generator=g)


def cast(t, dtype):
    return t if t is None or dtype is None else t.to(dtype)


class Pool:
    """The 2x convention over the calls of one case: feed() per call and group, check() once."""
    def __init__(self, what):
        self.what, self.err, self.gate = what, {}, {}

    def feed(self, group, got, r32, r64):
        if got.numel():
            assert bool(torch.isfinite(got).all()), (self.what, group)
            self.err[group] = max(self.err.get(group, 0.0), float((got.double() - r64).abs().max()))
            self.gate[group] = max(self.gate.get(group, 0.0), float((r32.double() - r64).abs().max()))

    def check(self):
        for group in self.err:
            err, gate = self.err[group], self.gate[group]
            print(f"{self.what} {group}: max |kernel - float64| {err:.3e}, gate (the float32 restatement's) {gate:.3e}")
        for group in self.err:
            assert self.err[group] <= 2 * self.gate[group], (self.what, group, self.err[group], self.gate[group])


# ------------------------------------------------------------------------------------------------------------------ tokens
def token_inputs(S, N, F, LRR, C, seed, sub=False):
    g, r = gen(seed)
    E = F + LRR + C + 2
    return dict(coords=torch.cat([r(S, N, 2) * 3 + 10, r(S, N, 1) + 5], -1), coords_sub=0.5 * r(S, N, 3) if sub else None,
                fcorrs=r(S, N, LRR), ffeats=r(S, N, C), track_mask=(r(S, N) > 0).float(), vis=r(S, N) * 4, pos=r(N, E), time=r(S, E),
                w_flow=(torch.rand(F, U.EMB, device=DEV, generator=g) - 0.5) / 7, b_flow=r(F) / 14)


def kernel_tokens(a, fix):
    return ti().build_tokens(*(a[k] for k in TOK), fix)


def ref_tokens(a, fix, dtype=None):
    return U.tokens(*(cast(a[k], dtype) for k in TOK), fix)


# every value of F in {1, 15, 16, 17, 130, 143, 144}, LRR in {1, 63, 64, 65}, C in {1, 16, 127, 128}; the eight corners first
TOKEN_SHAPES = [(1, 1, 1), (1, 1, 128), (1, 65, 1), (1, 65, 128), (144, 1, 1), (144, 1, 128), (144, 65, 1), (144, 65, 128),
                (15, 63, 16), (16, 64, 127), (17, 63, 127), (130, 64, 16), (143, 65, 16)]
TOKEN_GRIDS = [(1, 1), (1, 17), (7, 5), (3, 11), (16, 4)]               # 1, 17, 35, 33 and 64 tokens


@pytest.mark.parametrize("F,LRR,C", TOKEN_SHAPES)
def test_token_kernel_shapes(F, LRR, C):
    """Both mask settings, with and without coords_sub, five (S, N): the copy columns bit for bit, the flow columns
    under the convention pooled over the twenty calls of the shape."""
    pool = Pool(f"tokens F={F} LRR={LRR} C={C}")
    for i, (S, N) in enumerate(TOKEN_GRIDS):
        for sub in (False, True):
            a = token_inputs(S, N, F, LRR, C, 1000 * F + 10 * LRR + C + 7 * i, sub)
            r64 = ref_tokens(a, 1, torch.float64)[..., :F]
            for fix in (0, 1):
                x = kernel_tokens(a, fix)
                r32 = ref_tokens(a, fix)
                assert x.shape == (N, S, F + LRR + C + 2) and x.dtype == torch.float32 and x.is_contiguous()
                assert torch.equal(x[..., F:], r32[..., F:]), (S, N, sub, fix)
                pool.feed("flow", x[..., :F], r32[..., :F], r64)
    pool.check()


# ------------------------------------------------------------------------------------------------------------------- apply
def apply_inputs(S, N, C, seed, stress=True):
    """The arguments of one state update.  With 15 tokens or more the last four rows of delta stress the normalisation: a
    constant row, a row of mean 1e3 and spread 1e-2, one entry of 1e6 among small ones, an all-zero row.  `kind` [S, N] names
    them (an index into ROW_KINDS; 0: an ordinary row): on some the float32 restatement itself loses digits, and each kind is
    gated by itself."""
    g, r = gen(seed)
    delta = torch.cat([r(N, S, 3) * 0.5, r(N, S, C)], -1)
    kind = torch.zeros(S, N, dtype=torch.long, device=DEV)
    tokens = S * N
    if stress and tokens >= 15:
        rows = delta.view(tokens, 3 + C)
        rows[tokens - 1, 3:] = 0.75
        rows[tokens - 2, 3:] = 1e3 + 1e-2 * r(C)
        rows[tokens - 3, 3:] = 0.1 * r(C)
        rows[tokens - 3, 3 + C // 2] = 1e6
        rows[tokens - 4, 3:] = 0.0
        for k in (1, 2, 3, 4):
            kind[(tokens - k) % S, (tokens - k) // S] = k
    return dict(delta=delta, gamma=1 + 0.1 * r(C), beta=0.1 * r(C), w_u=(torch.rand(C, C, device=DEV, generator=g) - 0.5) * 2 / C ** 0.5,
                b_u=r(C) / 11, state=torch.cat([r(S, N, 2) * 3 + 10, r(S, N, 1) + 5], -1), ffeats=r(S, N, C),
                total=torch.cat([r(S, N, 2) * 3 + 10, r(S, N, 1) + 5], -1), dyn_mask=torch.sigmoid(r(N)), kind=kind)


def kernel_apply(b, static, log):
    """-> (state, ffeats, out), the inputs left as they are."""
    state, ffeats = b["state"].clone(), b["ffeats"].clone()
    extra = dict(total=b["total"], dyn_mask=b["dyn_mask"]) if static else {}
    out = ti().apply_delta(b["delta"], *(b[k] for k in PAR), state, ffeats, **SCALES[log], **extra)
    return state, ffeats, out


def ref_apply(b, static, log, dtype=None):
    extra = dict(total=cast(b["total"], dtype), dyn_mask=cast(b["dyn_mask"], dtype)) if static else {}
    return U.apply(cast(b["delta"], dtype), *(cast(b[k], dtype) for k in PAR), cast(b["state"], dtype), cast(b["ffeats"], dtype),
                   **SCALES[log], **extra)


ROW_KINDS = ("ordinary rows", "the constant row", "the row of mean 1e3", "the row with an entry of 1e6", "the all-zero row")
APPLY_GRIDS = [(1, 1), (3, 5), (16, 1), (1, 17), (7, 9), (5, 13), (1, 67)]     # 1, 15, 16, 17, 63, 65 and 67 tokens


@pytest.mark.parametrize("C", [16, 32, 48, 112, 128])
def test_apply_kernel_shapes(C):
    """The dynamic and the static pass, with and without the log depth, seven token counts: the state bit for bit,
    features and output under the convention pooled over the calls of one pass setting.  Then biases of +-8 and +-40, which
    saturate the GELU both ways: those four columns in a group of their own, and the -40 column exactly unchanged (erff is
    -1 below -10 / sqrt 2, the update is 0.5 v (1 + -1) = -0)."""
    for static in (False, True):
        for log in (False, True):
            pool = Pool(f"apply C={C} static={static} log={log}")
            for i, (S, N) in enumerate(APPLY_GRIDS):
                b = apply_inputs(S, N, C, 100 * C + 10 * i + 2 * static + log)
                state, ffeats, out = kernel_apply(b, static, log)
                s32, f32_, o32 = ref_apply(b, static, log)
                _, f64, o64 = ref_apply(b, static, log, torch.float64)
                assert out.shape == (S, N, 3) and out.dtype == torch.float32
                assert torch.equal(state, s32), (C, S, N, static, log)
                for k, name in enumerate(ROW_KINDS):
                    m = b["kind"] == k
                    pool.feed("features, " + name, ffeats[m], f32_[m], f64[m])
                pool.feed("output", out, o32, o64)
            pool.check()
    sat = torch.tensor([1, 5, 9, 13], device=DEV)
    rest = torch.ones(C, dtype=torch.bool, device=DEV)
    rest[sat] = False
    pool = Pool(f"apply C={C} saturating biases")
    for static in (False, True):
        b = apply_inputs(1, 67, C, 100 * C + 77 + static, stress=False)
        b["b_u"][sat] = torch.tensor([8.0, -8.0, 40.0, -40.0], device=DEV)
        state, ffeats, out = kernel_apply(b, static, False)
        s32, f32_, o32 = ref_apply(b, static, False)
        _, f64, o64 = ref_apply(b, static, False, torch.float64)
        assert torch.equal(state, s32) and torch.equal(ffeats[..., 13], b["ffeats"][..., 13])
        assert bool((ffeats[..., 9] - b["ffeats"][..., 9] > 30).all())
        pool.feed("saturated columns", ffeats[..., sat], f32_[..., sat], f64[..., sat])
        pool.feed("other columns", ffeats[..., rest], f32_[..., rest], f64[..., rest])
    pool.check()


# ------------------------------------------------------------------------------------------------- more tiles than waves
def track_slice(a, sl):
    """The arguments of a call for the tracks `sl` alone."""
    per_track = dict(coords=1, coords_sub=1, fcorrs=1, ffeats=1, track_mask=1, vis=1, pos=0, delta=0, state=1, total=1, dyn_mask=0, kind=1)
    return {k: (v if v is None or k not in per_track else (v[sl] if per_track[k] == 0 else v[:, sl]).contiguous()) for k, v in a.items()}


def test_more_tiles_than_waves():
    """S = 3 and the smallest N whose tokens exceed 16 x 8 x n_cu (k_track_tokens' waves; four times k_track_apply's)
    and are no multiple of 16: some wave takes a second tile, and that tile is partial.  The whole tensor: copy columns and
    state bit-equal to the float32 restatement.  Three 40-track slices (first, middle, last): flow columns and features
    bit-equal to the kernels' own output for those tracks submitted alone (fix_track_mask = 1: a token depends on its own
    track only) — placement independence, not a tolerance — and under the convention against float64."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    S, F, LRR, C = 3, U.F, U.LRR, U.C
    N = 16 * 8 * n_cu // S + 1
    while S * N % 16 == 0:
        N += 1
    assert S * N > 16 * 8 * n_cu and S * N % 16
    full = token_inputs(S, N, F, LRR, C, 31, sub=True)
    b = apply_inputs(S, N, C, 32, stress=False)
    slices = [slice(0, 40), slice(N // 2 - 20, N // 2 + 20), slice(N - 40, N)]
    pool = Pool(f"N={N} ({S * N} tokens, {n_cu} CUs)")
    for static in (False, True):
        a = full if static else dict(full, coords_sub=None)
        x, r32 = kernel_tokens(a, 1), ref_tokens(a, 1)
        assert torch.equal(x[..., F:], r32[..., F:])
        state, ffeats, out = kernel_apply(b, static, False)
        s32, _, o32 = ref_apply(b, static, False)
        assert torch.equal(state, s32)
        for sl in slices:
            qa, qb = track_slice(a, sl), track_slice(b, sl)
            assert torch.equal(x[sl][..., :F], kernel_tokens(qa, 1)[..., :F]), (static, sl)
            _, f_alone, o_alone = kernel_apply(qb, static, False)
            assert torch.equal(ffeats[:, sl], f_alone) and torch.equal(out[:, sl], o_alone), (static, sl)
            pool.feed("flow", x[sl][..., :F], r32[sl][..., :F], ref_tokens(qa, 1, torch.float64)[..., :F])
            _, f32_, o32s = ref_apply(qb, static, False)
            _, f64, o64 = ref_apply(qb, static, False, torch.float64)
            pool.feed("features", ffeats[:, sl], f32_, f64)
            pool.feed("output", out[:, sl], o32s, o64)
    pool.check()


def test_position_embedding_grid_stride():
    """E = 456 and the smallest N with N x E above 65536 x 256: k_pos_embed's grid-stride loop takes a second step.
    Bit-equal to the float32 restatement over the whole tensor."""
    H, W, E = 96, 128, U.E
    N = 65536 * 256 // E + 1
    assert N * E > 65536 * 256
    g = torch.Generator(device=DEV).manual_seed(33)
    xy = torch.rand(N, 2, device=DEV, generator=g) * torch.tensor([W + 3.0, H + 3.0], device=DEV) - 2.0
    tabx, taby = ti().pos_tables(H, W, E, DEV)
    got = ti().pos_embed_rows(H, W, E, xy)
    assert got.shape == (N, E) and torch.equal(got, U.pos_embed(tabx, taby, xy))


# ---------------------------------------------------------------------------------------------------------------- the sine
SINE_AMPLITUDES = [0.0, 1e-30, 2.0, 30.0, 100.0]


def test_sine_at_the_float32_argument():
    """Flows of amplitude 0, 1e-30, 2, 30 and 100 px (arguments v d_k up to 1.2e5 rad), pos = time = 0.  The truth is
    float64 with sine and cosine evaluated AT the float32 product fl(v d_k), as the header defines the embedding, so that
    the rounding of the argument is on neither side.  The assertion is an a-priori bound per element,
        200 u (sum_k |emb_k w_k| + |b|) + 4 u sum_{k < 192} |w_k|,   u = 2^-24:
    a 196-term float32 chain in any order and the bias add, and 4 ulp for each sine and cosine.  Printed beside it, as
    information: max |kernel - truth| and max |float32 restatement - truth| on the same inputs.
    Measured on an MI355X (the first measurement of the kernel's summation beside torch's; not a gate):
        amplitude   max |arg|   kernel      restatement   kernel / restatement   largest error / bound
        0           0           3.182e-07   2.404e-07     1.32                   0.007
        1e-30       3.7e-27     2.314e-07   2.861e-07     0.81                   0.005
        2           7.3e+03     8.624e-07   8.594e-07     1.00                   0.015
        30          1.19e+05    1.104e-06   1.317e-06     0.84                   0.014
        100         3.83e+05    3.529e-06   3.529e-06     1.00                   0.013"""
    S, N, F = 8, 48, U.F
    d = torch.arange(0, 64, 2, dtype=torch.float32, device=DEV) * (1000.0 / 64)
    for i, amp in enumerate(SINE_AMPLITUDES):
        a = token_inputs(S, N, F, 1, 1, 400 + i)
        g, r = gen(500 + i)
        a["coords"] = amp * r(S, N, 3)
        a["coords"][0] = 0.0
        if amp >= 30.0:
            a["coords"][1, 0, 0], a["coords"][2, 1, 1], a["coords"][3, 2, 2] = 109.5, -112.25, 123.0
        a["pos"], a["time"] = torch.zeros_like(a["pos"]), torch.zeros_like(a["time"])
        flow = (a["coords"] - a["coords"][0:1]).permute(1, 0, 2)                             # float32, as the kernel forms it
        arg = flow[..., None] * d                                                            # ONE float32 multiply
        if amp >= 30.0:
            assert float(arg.abs().max()) > 1e5
        pe = torch.stack([torch.sin(arg.double()), torch.cos(arg.double())], -1).reshape(N, S, 192)
        emb = torch.cat([pe, flow.double()], -1)
        w, bias = a["w_flow"].double(), a["b_flow"].double()
        truth = emb @ w.t() + bias
        bound = 200 * UNIT * (emb.abs() @ w.abs().t() + bias.abs()) + 4 * UNIT * w[:, :192].abs().sum(1)
        e_ker = (kernel_tokens(a, 1)[..., :F].double() - truth).abs()
        e_ref = float((ref_tokens(a, 1)[..., :F].double() - truth).abs().max())
        print(f"amplitude {amp:g}: max |kernel - truth| {float(e_ker.max()):.3e}, max |float32 restatement - truth| {e_ref:.3e}, "
              f"ratio {float(e_ker.max()) / max(e_ref, 1e-300):.2f}; largest error / bound {float((e_ker / bound).max()):.3f}, max |arg| {float(arg.abs().max()):.4g}")
        assert bool((e_ker <= bound).all()), (amp, float((e_ker / bound).max()))


# ------------------------------------------------------------------------------------------------------ reach and padding
GUARD, SENTINEL = 64, -12345.5


def guarded(t, fill):
    """t inside a larger buffer filled with `fill`: (buffer, the view that holds t)."""
    buf = torch.full((t.numel() + 2 * GUARD,), fill, device=DEV)
    inner = buf[GUARD:GUARD + t.numel()]
    inner.copy_(t.reshape(-1))
    return buf, inner


def untouched(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("S,N,C,fix", [(3, 37, 128, 0), (3, 37, 48, 1), (1, 1, 16, 0)])
def test_guard_rows_through_the_raw_entry_points(S, N, C, fix):
    """Every input followed and preceded by NaN, every output inside a buffer of sentinels: the results equal the
    front end's on plain tensors, nothing non-finite is read, no sentinel is written.  111 tokens: a partial last tile."""
    L = _lib.lib()
    F, LRR = U.F, 65
    a = token_inputs(S, N, F, LRR, C, 61, sub=True)
    want = kernel_tokens(a, fix)
    nan = {k: guarded(a[k], float("nan")) for k in TOK}
    xbuf, x = guarded(torch.zeros_like(want), SENTINEL)
    xbuf[GUARD:-GUARD] = SENTINEL
    rc = L.bt_track_tokens(*(nan[k][1].data_ptr() for k in TOK), S, N, F, LRR, C, fix, x.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc == _lib.BT_OK and torch.equal(x.view_as(want), want) and untouched(xbuf)

    b = apply_inputs(S, N, C, 62)
    for static in (False, True):
        for log in (False, True):
            s_want, f_want, o_want = kernel_apply(b, static, log)
            assert bool(torch.isfinite(f_want).all()) and bool(torch.isfinite(o_want).all())
            nan = {k: guarded(b[k], float("nan")) for k in ("delta", "total", "dyn_mask") + PAR}
            sbuf, state = guarded(b["state"], SENTINEL)
            fbuf, ffeats = guarded(b["ffeats"], SENTINEL)
            obuf, out = guarded(torch.full_like(o_want, SENTINEL), SENTINEL)
            sc = SCALES[log]
            rc = L.bt_track_apply(nan["delta"][1].data_ptr(), *(nan[k][1].data_ptr() for k in PAR), state.data_ptr(), ffeats.data_ptr(),
                                  nan["total"][1].data_ptr() if static else None, nan["dyn_mask"][1].data_ptr() if static else None, S, N, C,
                                  sc["stride"], sc["Dz"], sc["d_range"], sc["d_near"], int(log), out.data_ptr(), stream())
            torch.cuda.synchronize()
            assert rc == _lib.BT_OK
            assert torch.equal(state.view_as(s_want), s_want) and torch.equal(ffeats.view_as(f_want), f_want) and torch.equal(out.view_as(o_want), o_want)
            assert untouched(sbuf) and untouched(fbuf) and untouched(obuf)

    H, W, E = 16, 24, U.E
    tabx, taby = ti().pos_tables(H, W, E, DEV)
    want = ti().pos_embed_rows(H, W, E, a["coords"][0])
    nan = [guarded(t, float("nan")) for t in (tabx, taby, a["coords"][0])]
    obuf, out = guarded(torch.full_like(want, SENTINEL), SENTINEL)
    rc = L.bt_track_pos_embed(nan[0][1].data_ptr(), nan[1][1].data_ptr(), H, W, E, nan[2][1].data_ptr(), 3, N, out.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc == _lib.BT_OK and torch.equal(out.view_as(want), want) and untouched(obuf)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_reach_of_a_non_finite_value_in_the_state_update(bad):
    """One non-finite delta feature: that token's feature row, all of it, and nothing else.  One non-finite delta
    coordinate: that element of state and of out.  The static pass: a NaN in `total` reaches its element of out alone, a NaN
    in dyn_mask[n] the 3 S elements of out of track n; neither reaches the state.  Everything else: the clean call's bits."""
    S, N, C = 3, 37, 128
    b = apply_inputs(S, N, C, 63, stress=False)
    n, t = 22, 1
    for static in (False, True):
        clean = kernel_apply(b, static, False)
        assert all(bool(torch.isfinite(c).all()) for c in clean)

        def run(**over):
            return kernel_apply(dict(b, **over), static, False)

        def only(got, cells):
            """got = (state, ffeats, out); cells: the same, boolean: where the result may and must be non-finite."""
            for g_, c_, m in zip(got, clean, cells):
                assert not bool(torch.isfinite(g_[m]).any()) and torch.equal(g_[~m], c_[~m])

        none = [torch.zeros_like(c, dtype=torch.bool) for c in clean]
        delta = b["delta"].clone()
        delta[n, t, 3 + 77] = bad
        cells = [m.clone() for m in none]
        cells[1][t, n, :] = True
        only(run(delta=delta), cells)
        delta = b["delta"].clone()
        delta[n, t, 2] = bad
        cells = [m.clone() for m in none]
        cells[0][t, n, 2] = cells[2][t, n, 2] = True
        only(run(delta=delta), cells)
        if static:
            total = b["total"].clone()
            total[t, n, 0] = bad
            cells = [m.clone() for m in none]
            cells[2][t, n, 0] = True
            only(run(total=total), cells)
            dyn = b["dyn_mask"].clone()
            dyn[n] = float("nan")
            cells = [m.clone() for m in none]
            cells[2][:, n, :] = True
            only(run(dyn_mask=dyn), cells)


def test_no_tracks():
    """N = 0: empty results from the front end, BT_OK and nothing written through the raw entry points."""
    S, C, E = 3, U.C, U.E
    z = lambda *s: torch.zeros(*s, device=DEV)
    x = ti().build_tokens(z(S, 0, 3), None, z(S, 0, U.LRR), z(S, 0, C), z(S, 0), z(S, 0), z(0, E), z(S, E), z(U.F, U.EMB), z(U.F), 0)
    assert x.shape == (0, S, E) and x.dtype == torch.float32
    out = ti().apply_delta(z(0, S, 3 + C), z(C), z(C), z(C, C), z(C), z(S, 0, 3), z(S, 0, C), 4.0, 24.0, 19.5, 0.5)
    assert out.shape == (S, 0, 3) and out.dtype == torch.float32
    pos = ti().pos_embed_rows(16, 24, E, z(0, 2))
    assert pos.shape == (0, E) and pos.dtype == torch.float32
    L = _lib.lib()
    buf = torch.full((256,), SENTINEL, device=DEV)
    p = buf.data_ptr()
    assert L.bt_track_tokens(*([p] * 10), S, 0, U.F, U.LRR, C, 0, p, stream()) == _lib.BT_OK
    assert L.bt_track_apply(*([p] * 9), S, 0, C, 4.0, 24.0, 19.5, 0.5, 0, p, stream()) == _lib.BT_OK
    assert L.bt_track_pos_embed(p, p, 16, 24, E, p, 3, 0, p, stream()) == _lib.BT_OK
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())


# -------------------------------------------------------------------------------------------------------- far coordinates
def same_values(a, b):
    """Equal element for element, -0 and +0 alike, NaN where the other has NaN."""
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def test_position_embedding_at_far_coordinates():
    """Every pair of 19 finite coordinates from inside the map to FLT_MAX (tests/golden/pos_embed_far.npz, recorded from
    the reference's sample_pos_embed): the kernel equals the fixture wherever the reference's result is finite, -0 and +0
    alike, is non-finite exactly where the reference is, and equals the float32 restatement on the same GPU everywhere."""
    Fx = np.load(U.FAR_GOLD)
    H, W, E = int(Fx["H"]), int(Fx["W"]), int(Fx["E"])
    xy, want = torch.from_numpy(Fx["xy"]).to(DEV), torch.from_numpy(Fx["out"]).to(DEV)
    assert bool(torch.isfinite(xy).all())
    got = ti().pos_embed_rows(H, W, E, xy)
    finite = torch.isfinite(want)
    wrong = ((got != want) & finite).any(1) | (torch.isfinite(got) != finite).any(1)
    print(f"{int(wrong.sum())} of {xy.shape[0]} pairs differ from the reference:", xy[wrong].tolist())
    assert not bool(wrong.any())
    assert same_values(got, U.pos_embed(*ti().pos_tables(H, W, E, DEV), xy))


def test_non_finite_coordinates_stay_in_their_row():
    """NaN and +-inf in x, in y and in both, among ordinary rows: those rows are non-finite throughout, every other row
    has the clean call's bits."""
    H, W, E = 16, 24, U.E
    g = torch.Generator(device=DEV).manual_seed(66)
    xy = torch.rand(70, 2, device=DEV, generator=g) * torch.tensor([W + 3.0, H + 3.0], device=DEV) - 2.0
    clean = ti().pos_embed_rows(H, W, E, xy)
    bad_rows = []
    for k, v in enumerate((float("nan"), float("inf"), -float("inf"))):
        for j, cols in enumerate(([0], [1], [0, 1])):
            row = 3 + 7 * (3 * k + j)
            xy[row, cols] = v
            bad_rows.append(row)
    got = ti().pos_embed_rows(H, W, E, xy)
    bad = torch.zeros(70, dtype=torch.bool, device=DEV)
    bad[bad_rows] = True
    assert bool(torch.isfinite(clean).all()) and not bool(torch.isfinite(got[bad]).any()) and torch.equal(got[~bad], clean[~bad])
