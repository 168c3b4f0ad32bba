"""CPU half of the tracker iteration (include/batrack_track.h): the reference's fixture (tests/golden/track_iter.npz, made by
its unmodified MDTracker.forward_iteration and sample_pos_embed) against the torch restatement in tests/track_iter_util.py;
the input digests, the signatures, the ABI's refusals, the exported symbols, the operators' schemas, install() and the
import surface — none of which touch a GPU."""
import ctypes
import inspect
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import track_iter_util as U
from batrack_amd import _lib

D = dict(np.load(U.GOLD))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def restated_chain(c, dtype=torch.float32):
    """The case's calls through the restatement, chained on its own state.  The correlation values are not part of the
    fixture (the lookup has its own): zeros stand in, and only the columns after them are compared.  The features that a
    call's tokens copy are the fixture's (the reference's state before the call), so that the copy is compared bit for bit;
    the restatement's own feature chain is compared under the gate."""
    T = U.case_tensors(c, dtype)
    spec, sc = T["spec"], U.scale_args(T["scale"])
    S, N = spec["S"], spec["N"]
    tabx, taby = U.pos_tables(spec["H"], spec["W"])
    time = U.time_table(S)
    pos = U.pos_embed(tabx, taby, T["coords"][0])
    pos_static = U.pos_embed(tabx, taby, (T["coords"] - T["coords_dyn"])[0])
    coords, coords_dyn, ffeats, ffeats_static = T["coords"], T["coords_dyn"], T["ffeats"], T["ffeats"]
    par = [T[k] for k in ("gamma", "beta", "w_u", "b_u")]
    zeros = torch.zeros(S, N, U.LRR, dtype=dtype)
    dyn_mask = torch.sigmoid(T["dyn_logit"])[0, :, 0]
    calls = []
    for k in range(spec["iters"] + spec["static"]):
        first = k in (0, spec["iters"])                                          # both chains start from feat_init
        fe = T["ffeats"] if first else torch.from_numpy(D[f"{c}.{k - 1}.ffeats"]).to(dtype)
        if k < spec["iters"]:
            x = U.tokens(coords, None, zeros, fe, T["track_mask"], T["vis"], pos, time, T["w_flow"], T["b_flow"], spec["fix"])
            coords, ffeats, out = U.apply(T["deltas"][k], *par, coords, ffeats, **sc)
            calls.append(dict(x=x, state=coords, ffeats=ffeats, out=out))
        else:
            x = U.tokens(coords, coords_dyn, zeros, fe, T["track_mask"], T["vis"], pos_static, time, T["w_flow"], T["b_flow"], spec["fix"])
            coords_dyn, ffeats_static, out = U.apply(T["deltas"][k], *par, coords_dyn, ffeats_static, total=coords, dyn_mask=dyn_mask, **sc)
            calls.append(dict(x=x, state=coords_dyn, ffeats=ffeats_static, out=out))
    return dict(pos=pos, pos_static=pos_static, time=time, calls=calls)


@pytest.fixture(scope="module", params=list(U.CASES))
def case(request):
    return request.param, restated_chain(request.param)


def test_generator_reproduces_the_fixtures_inputs(case):
    c, _ = case
    d = U.make_inputs(**U.CASES[c])
    for name in U.INPUTS:
        assert np.array_equal(U.digest(d[name]), D[f"{c}.digest.{name}"]), name
        assert np.array_equal(d[name], d[name].astype(np.float32).astype(np.float64))          # float32 values


def test_restatement_reproduces_the_reference(case):
    """float32 restatement against the reference's float32 run: pos, time, the coordinate state and the copy columns after
    the correlation values bit for bit; the flow columns, the features and the output coordinates within the gate (the
    reference's own float32-vs-float64 difference)."""
    c, r = case
    spec = U.CASES[c]
    assert torch.equal(r["pos"], torch.from_numpy(D[f"{c}.pos"]))
    assert torch.equal(r["time"], torch.from_numpy(D[f"{c}.time"]))
    if spec["static"]:
        assert torch.equal(r["pos_static"], torch.from_numpy(D[f"{c}.pos_static"]))
    assert len(r["calls"]) == spec["iters"] + spec["static"]
    for k, call in enumerate(r["calls"]):
        assert torch.equal(call["state"], torch.from_numpy(D[f"{c}.{k}.state"])), (c, k)
        assert np.array_equal(U.digest(call["x"][..., U.F + U.LRR:].numpy()), D[f"{c}.{k}.tail_digest"]), (c, k)
        assert D[f"{c}.{k}.copy_digest"].shape == (3,)
        for name, got in (("flow", call["x"][..., :U.F]), ("ffeats", call["ffeats"]), ("out", call["out"])):
            gate = float(D[f"gate.{c}.{k}.{name}"])
            err = float((got.double() - torch.from_numpy(D[f"{c}.{k}.{name}"]).double()).abs().max())
            print(f"case {c} call {k} {name}: max |restatement - ref32| {err:.3e}, gate {gate:.3e}")
            assert 0 < gate < 5e-3
            assert err <= gate, (c, k, name, err, gate)


def test_fixture_cases_cover_what_they_claim():
    sp = U.CASES
    assert (sp["a"]["S"], sp["a"]["N"], sp["a"]["fix"], sp["a"]["iters"], sp["a"]["static"]) == (3, 5, 0, 2, 2)
    assert (sp["b"]["S"], sp["b"]["N"], sp["b"]["fix"], sp["b"]["iters"], sp["b"]["static"]) == (12, 6, 1, 1, 1)
    assert (sp["c"]["S"], sp["c"]["N"], sp["c"]["fix"], sp["c"]["iters"], sp["c"]["static"]) == (2, 65, 0, 1, 0)
    assert (sp["d"]["S"], sp["d"]["N"], sp["d"]["iters"], sp["d"]["static"]) == (1, 1, 1, 0)
    assert sp["a"]["S_init"] < sp["a"]["S"]                                      # the padding of the state and of the mask
    b = U.make_inputs(**sp["b"])["coords_init"][0, 0]
    outside = (b[:, 0] < 0) | (b[:, 0] > sp["b"]["W"] - 1) | (b[:, 1] < 0) | (b[:, 1] > sp["b"]["H"] - 1)
    assert outside.sum() == 3                                                    # the position sample clamps
    # the reshape quirk mixes mask and visibility in case a: some token's slot 0 is a visibility value
    T = U.case_tensors("a")
    assert not torch.equal(U.mask_columns(T["track_mask"], T["vis"], 0), U.mask_columns(T["track_mask"], T["vis"], 1))
    flow = D["a.1.flow"]
    assert np.isfinite(flow).all() and float((T["coords"][1:] - T["coords"][:1]).abs().max()) * 968.75 > 1e3      # arguments of 1e3 rad and more


def test_separable_tables_are_the_full_table():
    H, W = 16, 24
    tabx, taby = U.pos_tables(H, W)
    full = U.full_table(H, W)
    assert torch.equal(full[..., :U.E // 2], tabx[None].expand(H, -1, -1)) and torch.equal(full[..., U.E // 2:], taby[:, None].expand(-1, W, -1))
    xy = torch.tensor([[3.25, 7.5], [-2.0, 1.0], [30.0, 20.5], [0.0, 0.0], [23.0, 15.0]])
    assert torch.equal(U.pos_embed(tabx, taby, xy), U.pos_embed_full_table(H, W, U.E, xy))
    from batrack_amd.frontend import track_iter
    assert np.array_equal(track_iter._sincos_1d(U.E // 2, np.arange(W, dtype=np.float32)), U.sincos_1d(U.E // 2, W))
    assert np.array_equal(track_iter._sincos_1d(U.E, np.arange(12, dtype=np.float32)), U.sincos_1d(U.E, 12))


def test_restatement_reproduces_the_reference_at_far_coordinates():
    """tests/golden/pos_embed_far.npz: the reference's sample_pos_embed at every pair of 19 finite coordinates up to FLT_MAX.
    The restatement equals it wherever the reference's result is finite (-0 and +0 alike) and is non-finite exactly where
    the reference is.  Beyond 2^31 the reference's finite results are not zeros: a coordinate there meets a fractional one
    in range in 26 pairs whose four terms cancel only up to rounding (values up to 1e31)."""
    F = np.load(U.FAR_GOLD)
    H, W, E = int(F["H"]), int(F["W"]), int(F["E"])
    values, xy, want = torch.from_numpy(F["values"]), torch.from_numpy(F["xy"]), torch.from_numpy(F["out"])
    assert (H, W, E) == (U.FAR_H, U.FAR_W, U.FAR_E) and torch.equal(values, U.far_values(W)) and torch.equal(xy, U.far_pairs(values))
    assert bool(torch.isfinite(xy).all()) and want.shape == (values.numel() ** 2, E)
    got = U.pos_embed(*U.pos_tables(H, W, E), xy)
    finite = torch.isfinite(want)
    assert torch.equal(torch.isfinite(got), finite)
    assert bool((got[finite] == want[finite]).all())
    near = (xy.abs() < 2.0 ** 31).all(1)
    assert bool(finite[near].all()) and int(near.sum()) == 11 * 11               # where the int32 floor is defined: all finite
    far_finite = finite.all(1) & ~near
    assert int((~finite.all(1)).sum()) == 48 and int((want[far_finite] != 0).any(1).sum()) == 26
    assert os.path.getsize(U.FAR_GOLD) < 8 * 1024


def test_fixture_stays_small():
    assert os.path.getsize(U.GOLD) < 523 * 1024


def test_signatures_are_the_references():
    from batrack_amd.frontend import track_iter
    got = [str(inspect.signature(f)) for f in (track_iter.sample_pos_embed, track_iter.forward_iteration)]
    assert got == list(D["signatures"])
    assert got[0] == "(grid_size, embed_dim, coords)"
    assert got[1] == "(self, fmaps, dmaps, coords_init, coords_dyn_init, feat_init=None, vis_init=None, track_mask=None, iters=4)"


def test_symbols_are_exported_and_sources_listed():
    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "batrack_track.h")).read()
    for name in ("bt_track_pos_embed", "bt_track_tokens", "bt_track_apply"):
        assert hasattr(L, name), name
        assert name in header, name
    assert "track_iter.hip" in _lib.SOURCES
    assert any(h.endswith("batrack_track.h") for h in _lib.HEADERS)
    assert "tracker iteration" in _lib.ERRORS[_lib.BT_EUNSUPPORTED]
    import batrack_amd.frontend
    assert "track_iter" in batrack_amd.frontend.__doc__


def test_abi_refuses_before_launching():
    """Argument checks return their codes before anything is enqueued (no GPU needed: nothing is launched)."""
    L = _lib.lib()
    p = ctypes.c_void_p(256)                           # never dereferenced: every call below is refused first
    EINVAL, EUNS, OK = _lib.BT_EINVAL, _lib.BT_EUNSUPPORTED, _lib.BT_OK
    ok = dict(tabx=p, taby=p, H=16, W=24, E=456, coords=p, cstride=3, N=0, out=p)
    pe = lambda **k: L.bt_track_pos_embed(*(dict(ok, **k)[n] for n in ok), None)
    assert pe() == OK
    for name in ("tabx", "taby", "coords", "out"):
        assert pe(**{name: None}) == EINVAL, name
    for k in (dict(H=0), dict(W=0), dict(E=0), dict(E=455), dict(cstride=1), dict(N=-1)):
        assert pe(**k) == EINVAL, k
    for k in (dict(H=32769), dict(W=32769), dict(E=65538), dict(N=1 << 31)):
        assert pe(**k) == EUNS, k

    ptrs = ("coords", "coords_sub", "fcorrs", "ffeats", "track_mask", "vis", "pos", "time", "w_flow", "b_flow")
    ok = dict({n: p for n in ptrs}, S=12, N=0, F=130, LRR=196, C=128, fix=0, x=p)
    tk = lambda **k: L.bt_track_tokens(*(dict(ok, **k)[n] for n in ok), None)
    assert tk() == OK and tk(coords_sub=None) == OK and tk(F=144, fix=1) == OK
    for name in ptrs[:1] + ptrs[2:] + ("x",):
        assert tk(**{name: None}) == EINVAL, name
    for k in (dict(S=0), dict(N=-1), dict(F=0), dict(LRR=0), dict(C=0)):
        assert tk(**k) == EINVAL, k
    for k in (dict(F=145), dict(LRR=65537), dict(C=65537), dict(S=1 << 16, N=1 << 15), dict(S=12, N=(1 << 31) // 12 + 1)):
        assert tk(**k) == EUNS, k

    f = ctypes.c_float
    ptrs = ("delta", "gamma", "beta", "w_u", "b_u", "state", "ffeats", "total", "dyn_mask")
    ok = dict({n: p for n in ptrs}, S=12, N=0, C=128, stride=f(4), Dz=f(128), d_range=f(19.5), d_near=f(0.5), log=0, out=p)
    ap = lambda **k: L.bt_track_apply(*(dict(ok, **k)[n] for n in ok), None)
    assert ap() == OK and ap(total=None, dyn_mask=None) == OK and ap(C=16, log=1) == OK
    for name in ptrs[:7] + ("out",):
        assert ap(**{name: None}) == EINVAL, name
    assert ap(dyn_mask=None) == EINVAL                  # the static pass needs its mask
    for k in (dict(S=0), dict(N=-1), dict(C=0), dict(C=120), dict(C=8)):
        assert ap(**k) == EINVAL, k
    for k in (dict(C=144), dict(S=1 << 16, N=1 << 15)):
        assert ap(**k) == EUNS, k


def test_operator_schemas():
    ops = _lib.torch_ops(strict=True)
    assert str(ops.track_pos_embed.default._schema) == "batrack_hip::track_pos_embed(Tensor tabx, Tensor taby, Tensor coords) -> Tensor"
    assert str(ops.track_tokens.default._schema) == (
        "batrack_hip::track_tokens(Tensor coords, Tensor? coords_sub, Tensor fcorrs, Tensor ffeats, Tensor track_mask, Tensor vis, "
        "Tensor pos, Tensor time, Tensor w_flow, Tensor b_flow, bool fix_track_mask) -> Tensor")
    assert str(ops.track_apply.default._schema) == (
        "batrack_hip::track_apply(Tensor delta, Tensor gamma, Tensor beta, Tensor w_u, Tensor b_u, Tensor(a!) state, Tensor(b!) ffeats, "
        "Tensor? total, Tensor? dyn_mask, float stride, float dz, float d_range, float d_near, bool use_log_depth) -> Tensor")


def test_cpu_tensors_raise():
    from batrack_amd.frontend import track_iter
    T = U.case_tensors("d")
    with pytest.raises(RuntimeError, match="GPU"):
        track_iter.sample_pos_embed((16, 24), U.E, T["coords"][None])
    z = torch.zeros
    with pytest.raises(RuntimeError, match="GPU"):
        track_iter.build_tokens(T["coords"], None, z(1, 1, U.LRR), T["ffeats"], T["track_mask"], T["vis"], z(1, U.E), z(1, U.E),
                                T["w_flow"], T["b_flow"], 0)
    with pytest.raises(RuntimeError, match="GPU"):
        track_iter.apply_delta(T["deltas"][0], T["gamma"], T["beta"], T["w_u"], T["b_u"], T["coords"], T["ffeats"], 4.0, 24.0, 19.5, 0.5)
    ops = _lib.torch_ops(strict=True)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.track_pos_embed(z(24, 228), z(16, 228), z(1, 2))


def test_install_rebinds_both_and_returns_the_old_ones():
    from batrack_amd.frontend import track_iter
    tracker = types.ModuleType("stand_in_tracker")
    old_pos, old_fwd = (lambda grid_size, embed_dim, coords: None), (lambda self: None)
    tracker.sample_pos_embed = old_pos
    tracker.MDTracker = type("MDTracker", (), {"forward_iteration": old_fwd})
    assert track_iter.install(tracker) == (old_pos, old_fwd)
    assert tracker.sample_pos_embed is track_iter.sample_pos_embed
    assert tracker.MDTracker.forward_iteration is track_iter.forward_iteration
    assert track_iter.install(tracker) == (track_iter.sample_pos_embed, track_iter.forward_iteration)


def test_import_surface():
    """Importing batrack_amd does not import the front end; importing the module loads no native library and no oracle."""
    code = ("import sys; import batrack_amd; assert not any(m.startswith('batrack_amd.frontend') for m in sys.modules); "
            "import batrack_amd.frontend.track_iter; from batrack_amd import _lib; "
            "assert 'oracle' not in sys.modules and _lib._lib is None and _lib._torch_ops is None; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
