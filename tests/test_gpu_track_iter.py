"""GPU half of the tracker iteration (batrack_amd/csrc/track_iter.hip): the kernels against the reference's fixture —
bit-equal where the arithmetic is a copy, a sample or one add, and within twice the reference's own float32 error (the gate)
where it is a sum — and at the tracker's real shape against the restatement of tests/track_iter_util.py run in float64 on the
same GPU, under that restatement's own float32 error computed here.  No gate is derived from the kernel under test.

Why twice the gate: the kernel and the reference's float32 run carry the same argument-rounding term (the flow times up to
968.75 rad/px, rounded to float32), which the gate bounds; each adds its own rounding of sincosf, erff and the sums, of the
size the gate also bounds.  A fast-math sine misses this by orders of magnitude."""
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import track_iter_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D = dict(np.load(U.GOLD))


def ti():
    from batrack_amd.frontend import track_iter
    return track_iter


def fix(name):
    return torch.from_numpy(D[name]).to(DEV)


def lookup(T, coords, ffeats):
    from batrack_amd.frontend.corr import CorrBlock
    blk = CorrBlock(T["fmaps"], num_levels=U.LEVELS, radius=U.RADIUS)
    blk.corr(ffeats[None])
    return blk.sample(coords[None][..., :2])[0]


def within(got, name, c, k, what):
    gate = float(D[f"gate.{c}.{k}.{name}"])
    err = float((got.double() - fix(f"{c}.{k}.{name}").double()).abs().max())
    print(f"case {c} call {k} {what}: max |kernel - ref32| {err:.3e}, gate {gate:.3e}")
    assert err <= 2 * gate, (c, k, what, err, gate)


@pytest.mark.parametrize("c", list(U.CASES))
def test_fixture_cases_through_the_kernels(c):
    T = U.case_tensors(c, device=DEV)
    spec, sc = T["spec"], U.scale_args(T["scale"])
    S, N, H, W, it = spec["S"], spec["N"], spec["H"], spec["W"], spec["iters"]
    pos = ti().pos_embed_rows(H, W, U.E, T["coords"][0])
    pos_static = ti().pos_embed_rows(H, W, U.E, (T["coords"] - T["coords_dyn"])[0])
    time = ti().time_table(S, U.E, DEV)
    assert torch.equal(pos, fix(f"{c}.pos")) and torch.equal(time, fix(f"{c}.time"))
    if spec["static"]:
        assert torch.equal(pos_static, fix(f"{c}.pos_static"))
    assert torch.equal(ti().sample_pos_embed((H, W), U.E, T["coords"][None]), pos.t()[None])
    coords, coords_dyn = T["coords"].clone(), T["coords_dyn"].clone()
    ffeats, ffeats_static = T["ffeats"].clone(), T["ffeats"].clone()
    par = [T[k] for k in ("gamma", "beta", "w_u", "b_u")]
    dyn_mask = torch.sigmoid(T["dyn_logit"])[0, :, 0].contiguous()
    for k in range(it + spec["static"]):
        static = k >= it
        fe, p = (ffeats_static, pos_static) if static else (ffeats, pos)
        fcorrs = lookup(T, coords - coords_dyn if static else coords, fe)
        args = (coords, coords_dyn if static else None, fcorrs, fe, T["track_mask"], T["vis"], p, time, T["w_flow"], T["b_flow"], spec["fix"])
        x = ti().build_tokens(*args)
        assert x.shape == (N, S, U.E) and x.dtype == torch.float32 and x.is_contiguous()
        assert torch.equal(x, ti().build_tokens(*args))                                  # bit-stable from call to call
        within(x[..., :U.F], "flow", c, k, "flow columns")
        copy = torch.cat([fcorrs.permute(1, 0, 2), fe.permute(1, 0, 2), U.mask_columns(T["track_mask"], T["vis"], spec["fix"])], -1)
        assert torch.equal(x[..., U.F:], (copy + p[:, None, U.F:]) + time[None, :, U.F:])   # the copy columns, bit for bit
        if k in (0, it):                                                                 # the features are still feat_init: the reference's bits
            assert np.array_equal(U.digest(x[..., U.F + U.LRR:].cpu().numpy()), D[f"{c}.{k}.tail_digest"])
        if static:
            out = ti().apply_delta(T["deltas"][k], *par, coords_dyn, ffeats_static, total=coords, dyn_mask=dyn_mask, **sc)
        else:
            out = ti().apply_delta(T["deltas"][k], *par, coords, ffeats, **sc)
        assert torch.equal(coords_dyn if static else coords, fix(f"{c}.{k}.state")), (c, k)   # one float add: bit-equal
        within(ffeats_static if static else ffeats, "ffeats", c, k, "features")
        within(out, "out", c, k, "output coordinates")
    if not spec["static"]:
        assert torch.equal(coords_dyn, T["coords_dyn"])


class Prepared(nn.Module):
    def __init__(self, outputs):
        super().__init__()
        self.outputs, self.seen = list(outputs), []

    def forward(self, *args):
        self.seen.append([a.detach().clone() for a in args])
        return self.outputs[len(self.seen) - 1]


def stand_in_tracker(c):
    """A plain object with what forward_iteration reads: real torch modules for the small layers, prepared deltas for the
    two transformers (the fixture's), recorders for vis_predictor and motion_label_block."""
    spec = U.CASES[c]
    d = U.make_inputs(**spec)
    t = lambda a: torch.as_tensor(a, dtype=torch.float32, device=DEV)

    def lin(w, b):
        m = nn.Linear(w.shape[1], w.shape[0]).to(DEV)
        m.weight.data.copy_(t(w))
        m.bias.data.copy_(t(b))
        return m
    norm = nn.GroupNorm(1, U.C).to(DEV)
    norm.weight.data.copy_(t(d["gamma"]))
    norm.bias.data.copy_(t(d["beta"]))
    it, sc = spec["iters"], d["scale"]
    me = types.SimpleNamespace(
        corr_levels=U.LEVELS, corr_radius=U.RADIUS, input_dim=U.E, latent_dim=U.C, fix_track_mask=bool(spec["fix"]),
        zeroMLPflow=lin(d["w_flow"], d["b_flow"]), norm=norm, ffeat_updater=nn.Sequential(lin(d["w_u"], d["b_u"]), nn.GELU()),
        updateformer=Prepared(t(d["deltas"][:it])), updateformer_dyn=Prepared(t(d["deltas"][it:])),
        vis_predictor=Prepared([torch.zeros(spec["S"] * spec["N"], 1, device=DEV)]), motion_label_block=Prepared([t(d["dyn_logit"])]),
        stride=int(sc["stride"]), Dz=int(sc["Dz"]), d_near=sc["d_near"], d_far=sc["d_far"], use_log_depth=sc["use_log_depth"],
        dynamic_mask_detach=True, static_iters=spec["static"])
    inputs = dict(fmaps=t(d["fmaps"]), dmaps=None, coords_init=t(d["coords_init"]), coords_dyn_init=t(d["coords_dyn_init"]),
                  feat_init=t(d["feat_init"]), vis_init=t(d["vis_init"]), track_mask=t(d["track_mask"]), iters=it)
    return me, inputs


def test_forward_iteration_chained_over_case_a():
    """The whole loop, S_init < S, with the fixture's prepared deltas: every recorded x and the returned tuple."""
    c = "a"
    spec = U.CASES[c]
    S, N, it, st = spec["S"], spec["N"], spec["iters"], spec["static"]
    me, inputs = stand_in_tracker(c)
    with torch.no_grad():
        coord, depth, static, vis_e, dynamic_e, feat_back = ti().forward_iteration(me, **inputs)
    assert feat_back is inputs["feat_init"] and len(coord) == len(depth) == it and len(static) == st
    T = U.case_tensors(c, device=DEV)
    time, mask = fix(f"{c}.time"), U.mask_columns(T["track_mask"], T["vis"], spec["fix"])
    xs = [s[0] for s in me.updateformer.seen + me.updateformer_dyn.seen]
    assert len(xs) == it + st
    for k, x in enumerate(xs):
        assert x.shape == (1, N, S, U.E)
        x, p = x[0], fix(f"{c}.pos_static" if k >= it else f"{c}.pos")
        within(x[..., :U.F], "flow", c, k, "x: flow columns")
        lo = U.F + U.LRR
        assert torch.equal(x[..., lo + U.C:], (mask + p[:, None, lo + U.C:]) + time[None, :, lo + U.C:])      # mask and visibility
        if k in (0, it):
            assert np.array_equal(U.digest(x[..., lo:].cpu().numpy()), D[f"{c}.{k}.tail_digest"])
        else:                                                                            # the features after the previous call
            want = (fix(f"{c}.{k - 1}.ffeats").permute(1, 0, 2) + p[:, None, lo:lo + U.C]) + time[None, :, lo:lo + U.C]
            err, gate = float((x[..., lo:lo + U.C].double() - want.double()).abs().max()), float(D[f"gate.{c}.{k - 1}.ffeats"])
            print(f"call {k} x: feature columns {err:.3e}, gate {gate:.3e}")
            assert err <= 2 * gate + 2.4e-7 * float(want.abs().max())                    # and the two adds' own rounding
        assert torch.isfinite(x[..., U.F:lo]).all() and x[..., U.F:lo].abs().max() > 0.1     # the lookup's values are there
    for k in range(it):
        assert coord[k].shape == (1, S, N, 2) and depth[k].shape == (1, S, N, 1)
        within(torch.cat([coord[k], depth[k]], -1)[0], "out", c, k, "returned coordinates")
    for k in range(st):
        assert static[k].shape == (1, S, N, 3)
        within(static[k][0], "out", c, it + k, "returned static coordinates")
    seen_ffeats, seen_coords = me.motion_label_block.seen[0]
    assert torch.equal(seen_coords[0], fix(f"{c}.{it - 1}.state"))
    within(seen_ffeats[0], "ffeats", c, it - 1, "features handed to the motion label")
    assert torch.equal(me.vis_predictor.seen[0][0].reshape(S, N, U.C), seen_ffeats[0])
    assert vis_e.shape == (1, S, N) and torch.equal(dynamic_e, fix(f"{c}.dynamic_e")) and torch.equal(vis_e, fix(f"{c}.vis_e"))


def small_call(S=3, N=5, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    coords = torch.cat([r(S, N, 2) * 3 + 10, r(S, N, 1) + 5], -1)
    return dict(coords=coords, fcorrs=r(S, N, U.LRR), ffeats=r(S, N, U.C), track_mask=(r(S, N) > 0).float(), vis=r(S, N) * 4,
                pos=r(N, U.E), time=r(S, U.E), w_flow=r(U.F, U.EMB) / 14, b_flow=r(U.F) / 14)


def tokens_of(a, fix_flag, **over):
    a = dict(a, **over)
    return ti().build_tokens(a["coords"], a.get("coords_sub"), a["fcorrs"], a["ffeats"], a["track_mask"], a["vis"], a["pos"], a["time"],
                             a["w_flow"], a["b_flow"], fix_flag)


def test_both_mask_settings_where_the_reshape_mixes_them():
    a = small_call()
    last = {}
    for flag in (0, 1):
        x = tokens_of(a, flag)
        want = (U.mask_columns(a["track_mask"], a["vis"], flag) + a["pos"][:, None, -2:]) + a["time"][None, :, -2:]
        assert torch.equal(x[..., -2:], want)
        last[flag] = x
    assert torch.equal(last[0][..., :-2], last[1][..., :-2]) and not torch.equal(last[0][..., -2:], last[1][..., -2:])
    # setting 0: token (n = 0, t = 0) holds track_mask[0, 0], track_mask[1, 0] — two frames of one track, not (mask, vis)
    m0 = last[0][0, 0, -2:] - a["pos"][0, -2:] - a["time"][0, -2:]
    assert torch.allclose(m0, torch.stack([a["track_mask"][0, 0], a["track_mask"][1, 0]]), atol=1e-5)


def test_strided_views_are_accepted():
    a = small_call(S=4, N=7)
    S, N = 4, 7
    c4 = torch.zeros(1, S, N, 4, device=DEV)
    c4[0, ..., :3] = a["coords"]
    H, W = 16, 24
    want = ti().pos_embed_rows(H, W, U.E, a["coords"][0, :, :2].contiguous())
    assert torch.equal(ti().pos_embed_rows(H, W, U.E, a["coords"][0]), want)               # rows of the [S, N, 3] state, in place
    assert torch.equal(ti().pos_embed_rows(H, W, U.E, c4[0, 0, :, :2]), want)
    assert torch.equal(ti().sample_pos_embed((H, W), U.E, c4[..., :3]), want.t()[None])
    assert torch.equal(ti().sample_pos_embed((H, W), U.E, a["coords"][None][..., :2]), want.t()[None])
    x = tokens_of(a, 0)
    assert torch.equal(tokens_of(a, 0, coords=c4[0, ..., :3], ffeats=a["ffeats"].permute(1, 0, 2).contiguous().permute(1, 0, 2),
                                 vis=a["vis"].t().contiguous().t()), x)


def test_one_nan_coordinate_stays_in_its_token():
    a = small_call(S=3, N=37)
    a["coords"][1, 2, 0] = float("nan")
    x = tokens_of(a, 0)
    bad = ~torch.isfinite(x).all(-1)                                  # [N, S]
    want = torch.zeros_like(bad)
    want[2, 1] = True
    assert torch.equal(bad, want)
    assert not torch.isfinite(x[2, 1, :U.F]).any() and torch.isfinite(x[2, 1, U.F:]).all()
    a["coords"][1, 2, 0] = float("inf")
    assert torch.equal(~torch.isfinite(tokens_of(a, 0)).all(-1), want)


def real_call(N, S=12, H=96, W=128, seed=5):
    g = torch.Generator(device=DEV).manual_seed(seed + N)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    start = torch.rand(1, N, 3, device=DEV, generator=g) * torch.tensor([W - 1.0, H - 1.0, float(W)], device=DEV)
    coords = (start + 2.0 * r(S, N, 3) * (torch.arange(S, device=DEV) > 0)[:, None, None]).contiguous()
    tabx, taby = ti().pos_tables(H, W, U.E, DEV)
    a = dict(coords=coords, fcorrs=r(S, N, U.LRR), ffeats=r(S, N, U.C), track_mask=(r(S, N) > 0).float(), vis=r(S, N) * 4,
             pos=U.pos_embed(tabx, taby, coords[0]), time=ti().time_table(S, U.E, DEV), w_flow=(torch.rand(U.F, U.EMB, device=DEV, generator=g) - 0.5) / 7,
             b_flow=r(U.F) / 14)
    b = dict(delta=torch.cat([r(N, S, 3) * 0.5, r(N, S, U.C)], -1), gamma=1 + 0.1 * r(U.C), beta=0.1 * r(U.C),
             w_u=(torch.rand(U.C, U.C, device=DEV, generator=g) - 0.5) / 5.6, b_u=r(U.C) / 11, coords_dyn=0.5 * r(S, N, 3),
             dyn_mask=torch.sigmoid(r(N)))
    return a, b


def sliced(a, sl, dtype):
    per_track = {"coords": 1, "coords_sub": 1, "fcorrs": 1, "ffeats": 1, "track_mask": 1, "vis": 1, "pos": 0, "delta": 0, "coords_dyn": 1,
                 "dyn_mask": 0, "state": 1, "total": 1}
    out = {}
    for k, v in a.items():
        v = v[sl] if per_track.get(k) == 0 else (v[:, sl] if per_track.get(k) == 1 else v)
        out[k] = v.to(dtype) if dtype is not None and k not in ("pos", "time") else v        # the tables stay float32, as in the reference
    return out


def test_real_shape_against_the_float64_restatement():
    """S = 12, N = 2400.  fix_track_mask = 1 so that a slice of tracks is self-contained.  On two 128-track slices the kernel
    stays within twice the restatement's own float32-vs-float64 error; on the whole tensor the copy columns, the position
    embedding and the coordinate state equal the float32 restatement bit for bit."""
    S, N, H, W = 12, 2400, 96, 128
    a, b = real_call(N)
    assert torch.equal(ti().pos_embed_rows(H, W, U.E, a["coords"][0]), a["pos"])
    assert torch.equal(a["pos"][:64], U.pos_embed_full_table(H, W, U.E, a["coords"][0, :64]))
    sc = dict(stride=4.0, Dz=128.0, d_range=19.5, d_near=0.5, use_log_depth=False)
    par = [b[k] for k in ("gamma", "beta", "w_u", "b_u")]
    tok = lambda q, sub: U.tokens(q["coords"], sub, q["fcorrs"], q["ffeats"], q["track_mask"], q["vis"], q["pos"], q["time"], q["w_flow"], q["b_flow"], 1)
    for static in (False, True):
        sub = b["coords_dyn"] if static else None
        x = tokens_of(a, 1, coords_sub=sub)
        r32 = tok(a, sub)
        assert torch.equal(x[..., U.F:], r32[..., U.F:])
        state, ffeats = (b["coords_dyn"] if static else a["coords"]).clone(), a["ffeats"].clone()
        extra = dict(total=a["coords"], dyn_mask=b["dyn_mask"]) if static else {}
        s32, f32_, o32 = U.apply(b["delta"], *par, state, ffeats, **sc, **extra)
        out = ti().apply_delta(b["delta"], *par, state, ffeats, **sc, **extra)
        assert torch.equal(state, s32)
        got = dict(flow=x[..., :U.F], ffeats=ffeats, out=out)
        for sl in (slice(0, 128), slice(N - 128 - 5, N - 5)):
            q32, q64 = sliced(dict(a, coords_sub=sub) if static else a, sl, None), sliced(dict(a, coords_sub=sub) if static else a, sl, torch.float64)
            ref = {32: {}, 64: {}}
            for bits, q, dt in ((32, q32, None), (64, q64, torch.float64)):
                ref[bits]["flow"] = tok(q, q.get("coords_sub"))[..., :U.F]
                p = sliced(dict(delta=b["delta"], state=b["coords_dyn"] if static else a["coords"], ffeats=a["ffeats"],
                                **({"total": a["coords"], "dyn_mask": b["dyn_mask"]} if static else {})), sl, dt)
                pp = [v.to(dt) if dt else v for v in par]
                _, ref[bits]["ffeats"], ref[bits]["out"] = U.apply(p["delta"], *pp, p["state"], p["ffeats"], **sc,
                                                                   **({"total": p["total"], "dyn_mask": p["dyn_mask"]} if static else {}))
            for name, g_ in got.items():
                gs = g_[sl] if name == "flow" else g_[:, sl]
                gate = float((ref[32][name].double() - ref[64][name]).abs().max())
                err = float((gs.double() - ref[64][name]).abs().max())
                print(f"static {static} tracks {sl.start}:{sl.stop} {name}: max |kernel - restatement64| {err:.3e}, gate (its float32 run) {gate:.3e}")
                assert 0 < gate < 2e-2
                assert err <= 2 * gate, (static, sl, name, err, gate)


def test_a_token_build_allocates_only_its_output():
    a, _ = real_call(2400)
    tokens_of(a, 0)                                                   # the tables, the library and the operator are loaded
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    x = tokens_of(a, 0)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise} bytes, x {x.numel() * 4} bytes")
    assert rise <= x.numel() * 4 + (1 << 20), (rise, x.numel() * 4)


def test_install_on_a_stand_in_tracker():
    """install() on a stand-in module: the rebound method, called as the tracker calls it, runs the kernels."""
    tracker = types.ModuleType("stand_in_tracker")
    tracker.sample_pos_embed = old = lambda grid_size, embed_dim, coords: None
    tracker.MDTracker = type("MDTracker", (), {})
    assert ti().install(tracker) == (old, None)
    me, inputs = stand_in_tracker("d")
    obj = tracker.MDTracker()
    obj.__dict__.update(vars(me))
    with torch.no_grad():
        coord, depth, static, vis_e, dynamic_e, _ = obj.forward_iteration(**inputs)
    within(torch.cat([coord[0], depth[0]], -1)[0], "out", "d", 0, "installed method: returned coordinates")
    assert static == [] and torch.equal(tracker.sample_pos_embed((16, 24), U.E, inputs["coords_init"])[0].t(), fix("d.pos"))


def test_refusals():
    a = small_call()
    with pytest.raises(RuntimeError):
        tokens_of(a, 0, w_flow=torch.zeros(145, U.EMB, device=DEV), b_flow=torch.zeros(145, device=DEV),
                  pos=torch.zeros(5, U.E + 15, device=DEV), time=torch.zeros(3, U.E + 15, device=DEV))       # F > 144
    with pytest.raises(RuntimeError):
        tokens_of(a, 0, pos=a["pos"][:, :-1].contiguous())                                                      # a shape that disagrees
    S, N, Cb = 3, 5, 144
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(RuntimeError):
        ti().apply_delta(z(N, S, 3 + Cb), z(Cb), z(Cb), z(Cb, Cb), z(Cb), z(S, N, 3), z(S, N, Cb), 4.0, 24.0, 19.5, 0.5)   # C > 128
    with pytest.raises(RuntimeError, match="in place"):
        ti().apply_delta(z(N, S, 3 + U.C), z(U.C), z(U.C), z(U.C, U.C), z(U.C), z(N, S, 3).permute(1, 0, 2), z(S, N, U.C), 4.0, 24.0, 19.5, 0.5)
    with pytest.raises(RuntimeError, match="together"):
        ti().apply_delta(z(N, S, 3 + U.C), z(U.C), z(U.C), z(U.C, U.C), z(U.C), z(S, N, 3), z(S, N, U.C), 4.0, 24.0, 19.5, 0.5, total=z(S, N, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        tokens_of(a, 0, coords=a["coords"].cpu())
