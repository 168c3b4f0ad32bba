"""`BA_rgbd_droid` — the reference's bundle-adjustment entry point
(main/backend/ba.py:217-339), same signature and argument
meaning, executed by the gfx950 kernels behind include/batrack_ba.h.

Called exactly as BATRACK.update() does (main/batrack.py:869-875):

    Gs, patches = BA_rgbd_droid(Gs, patches, patches_monodisp, intrinsics,
                                targets_3d[..., :2], targets_3d[..., 2:], weights, lmbda,
                                ii, jj, kk, bounds, ep=ep, fixedp=t0,
                                structure_only=..., loss=..., alpha=0.05)

Behaviour kept from the reference: returns NEW tensors (inputs untouched); with
structure_only (or no free pose) the input SE3 object itself is returned
(ba.py:336-339); `targets_disp` is accepted and never read; the whole disparity
buffer is clamped to [1e-3, 10] (ba.py:333); a failed Cholesky leaves the poses
re-normalised but unmoved (ba.py:9-13), nothing raises.

There is no CPU path: tensors must live on a ROCm device and the HIP library
must be built, otherwise this raises.
"""
import os
import weakref
from concurrent.futures import ThreadPoolExecutor

import torch

from .. import _lib
from ..plan import Plan, Stepper
from .lietorch import SE3

_WORKER = None       # one long-lived host thread (the planner keeps edge-sized scratch per thread)
_cuda = torch.cuda   # (the waits for the index tensors go through this name: a test of the cache's policy puts a fake there)

# How far down the ladder a new list's plan may be looked for: built only, as a shifted copy of a cached plan, as a copy ASSUMED to
# be one (no wait for the comparison), as such a copy made AHEAD of the list.  Each rung above the first has its switch.
BUILD_ONLY, SHIFTED, SPECULATIVE, AHEAD = range(4)
_SWITCHES = ("BT_PLAN_SHIFT", "BT_PLAN_SPECULATE", "BT_PLAN_PRESHIFT")


def _ladder(upto=AHEAD):
    """How far the ladder goes, as far as `upto`.  The switches are read when the decision is made (tests and tools flip them between
    calls), and no more of them than the caller asks about (a read costs most of a microsecond)."""
    for rung in range(upto):
        if os.environ.get(_SWITCHES[rung], "1") == "0":
            return rung
    return upto


def _ident(ii, jj, kk):
    """What an in-place edit or a reallocation of the index tensors changes (their identity is checked beside it)."""
    return (ii._version, jj._version, kk._version, ii.data_ptr(), jj.data_ptr(), kk.data_ptr())


def _key(ii, jj, kk, n_buf, p_tot, fixedp, device):
    return (id(ii), id(jj), id(kk)) + _ident(ii, jj, kk) + (ii.numel(), int(fixedp), int(n_buf), int(p_tot), str(device))


class _Entry:
    """One cached plan."""
    __slots__ = ("stepper", "refs", "calls", "pre_tried")

    def __init__(self, stepper, ii, jj, kk):
        self.stepper = stepper
        self.refs = tuple(weakref.ref(t) for t in (ii, jj, kk))   # the list the plan is of (a key's id()s may be another tensor's by now)
        self.calls = 0               # calls that found the plan in place, counted behind their steps
        self.pre_tried = False       # the clone ahead has been decided on (made or not): once per plan


class _Call:
    """The last call's list and plan: an update() makes 2 x ITER calls on one list."""
    __slots__ = ("entry", "ii", "jj", "kk", "ident", "fixedp", "n_buf", "p_tot", "device")

    def __init__(self, entry, ii, jj, kk, fixedp, n_buf, p_tot, device):
        self.entry, self.ii, self.jj, self.kk, self.ident = entry, ii, jj, kk, _ident(ii, jj, kk)
        self.fixedp, self.n_buf, self.p_tot, self.device = fixedp, n_buf, p_tot, device


class PlanCache:
    """The plans behind `BA_rgbd_droid`, one per (edge list, fixedp): the caller keeps self.ii/jj/kk alive and unmodified across the
    2*ITER calls of an update() (batrack.py:869-875) and replaces the tensors when edges are appended / removed (batrack.py:189-204).

    Threads: `prefetch(background=True)` runs its `build` on the worker thread — `_build(speculate=False)`, i.e. the synchronous
    shifted copy or the planner, and the `Stepper` around the plan.  That reads a snapshot of `plans` (`_candidates`) and may set
    `last_shift`; the caller's thread takes the result from the pending entry's box.  All else belongs to the caller's thread."""

    def __init__(self):
        self.plans = {}           # key -> _Entry, oldest first; 8 at most
        self.ahead = {}           # _Entry -> the stepper of its clone for the NEXT list, made ahead (Plan.preshift); 3 at most
        self.pending = {}         # key -> (future, result box, (ii, jj, kk)): plans being built by prefetch; 4 at most
        self.last = None          # _Call
        self.last_shift = None    # frame shift of the last plan that was made as a shifted copy (survives `clear`)
        self.calls_before = 0     # how many calls the previous list got: decides when the next clone is made (survives `clear`)

    def get(self, ii, jj, kk, n_buf, p_tot, fixedp, device):
        """(the list's stepper, it was found in place as the plan of the call before — this is not the first call of an update())."""
        c = self.last
        # (`_ident` spelled out: seven of an update()'s eight calls end here, in front of the GPU's work)
        if (c is not None and c.ii is ii and c.jj is jj and c.kk is kk
                and c.ident == (ii._version, jj._version, kk._version, ii.data_ptr(), jj.data_ptr(), kk.data_ptr())
                and c.fixedp == fixedp and c.n_buf == n_buf and c.p_tot == p_tot and c.device == device):
            return c.entry.stepper, True
        if c is not None:
            self.calls_before = c.entry.calls + 1
        entry = self._lookup(ii, jj, kk, n_buf, p_tot, fixedp, device)
        self.last = _Call(entry, ii, jj, kk, fixedp, n_buf, p_tot, device)
        return entry.stepper, False

    def settle(self, stepper):
        """Settle a speculative plan.  True: it is the list's plan.  False: the guess was wrong — the plan is out of the cache.  An
        error of the confirmation itself (an index out of range in the new list) also takes it out before it is raised again: a
        caller that catches it and calls once more must not step on the unconfirmed clone."""
        try:
            ok = stepper.plan.confirm()
        except Exception:
            self._discard(stepper)
            raise
        if not ok:
            self._discard(stepper)
        return ok

    def after_step(self):
        """Behind the enqueued step of a call that found its plan in place: counts the call and, behind ONE call per plan, makes the
        clone for the list the NEXT update() will most likely bring — this plan's, moved up by the shift that was right last time
        (~45 us).  The first call of the next update(), which has the GPU idle behind it, is left with one comparison kernel."""
        e = self.last.entry
        e.calls += 1                                  # this was call number e.calls + 1 on the plan
        if e.pre_tried:
            return
        # WHEN: behind a call that leaves the host ~45 us it can spend unnoticed, i.e. with that much GPU work queued in front of it.  The
        # first call of an update() is late by its plan; the host catches up by ~10-25 us a call (a structure-only step is 19 us of
        # kernels, a pose+structure one 61): behind call 2 the clone cost the update() 16-37 us (the GPU ran dry before call 3 arrived),
        # behind call 5 or 7 nothing (tools/gpu_update_floor.py, AB_AT).  So: call 5 where the update()s have that many calls (how many the
        # previous list got), else call 3, else 2.  BT_PLAN_PRESHIFT_AT: the measurement's override.
        at = os.environ.get("BT_PLAN_PRESHIFT_AT")
        at = int(at) if at else (5 if self.calls_before >= 6 else 3 if self.calls_before >= 4 else 2)
        if e.calls + 1 < at:
            return
        df, stepper = self.last_shift, e.stepper
        if df is None or stepper.plan.speculative:
            return
        e.pre_tried = True
        if _ladder() < AHEAD:
            return
        pl = Plan.preshift(stepper.plan, df)
        if pl is not None:
            while len(self.ahead) >= 3:
                self.ahead.pop(next(iter(self.ahead)))
            # (the clone shares its source's workspace, as a clone made in the call does: same layout, same stream, taking turns)
            self.ahead[e] = Stepper(pl, stepper.device, stepper.ws)
            # ... and the room the next update()'s plan will need in the cache is made now (destroying a plan is not free either)
            old = next(iter(self.plans), None)
            if len(self.plans) >= 8 and self.plans[old] is not e:
                self._evict(old)

    def prefetch(self, ii, jj, kk, n_buf, p_tot, fixedp, dev, background):
        key = _key(ii, jj, kk, n_buf, p_tot, fixedp, dev)
        if key in self.plans or key in self.pending:
            return
        # A clone made ahead for this list (during the previous update()) waits for it: nothing to build.  It is NOT bound
        # here — measured (tools/gpu_update_floor.py, PREFETCH=1 AB=1): with the comparison launched at prefetch time the update() took
        # 0.412 ms against 0.38-0.39 with the first BA call launching it — in front of the step the comparison also wakes the idle GPU
        # while the host is still preparing the step's launches.
        if self._clone_ahead(ii, n_buf, p_tot, fixedp) is not None:
            return
        ready, caller_stream = _cuda.Event(), _cuda.current_stream(dev)
        ready.record(caller_stream)                                # the indices are complete once this has passed
        box = {}

        def build():
            try:
                ready.synchronize()
                # the current device and stream are per host thread: the workspace is allocated and zero-filled on the stream
                # the steps will run on, so its accumulators are clear before the first of them whatever stream that is
                with _cuda.device(dev), _cuda.stream(caller_stream):
                    box["stepper"] = Stepper(self._build(ii, jj, kk, n_buf, p_tot, fixedp, False, speculate=False)[0], dev)
            except BaseException as e:                              # reported (or retried in the open) by _lookup
                box["error"] = e

        while len(self.pending) >= 4:                              # stale prefetches (edge lists that were never used)
            self.pending.pop(next(iter(self.pending)))[0].result()
        if background:
            global _WORKER
            if _WORKER is None:
                _WORKER = ThreadPoolExecutor(max_workers=1, thread_name_prefix="batrack-plan")
            self.pending[key] = (_WORKER.submit(build), box, (ii, jj, kk))
        else:
            build()
            if "error" in box:
                raise box["error"]
            self._store(key, box["stepper"], ii, jj, kk)

    def clear(self):
        """Forgets every plan, clone and prefetch, but not `last_shift` and `calls_before`: the caller's window goes on as it did."""
        for fut, _, _ in list(self.pending.values()):
            fut.result()
        self.pending.clear()
        self.ahead.clear()
        self.plans.clear()
        self.last = None

    def _store(self, key, stepper, ii, jj, kk):
        if len(self.plans) >= 8:
            self._evict(next(iter(self.plans)))
        entry = self.plans[key] = _Entry(stepper, ii, jj, kk)
        return entry

    def _evict(self, key):
        """A plan leaves the cache, and the clone made ahead from it with it (it is of no use without its source)."""
        entry = self.plans.pop(key, None)
        self.ahead.pop(entry, None)                   # (first: the clone goes before its source)

    def _discard(self, stepper):
        """A plan whose speculation failed: out of the cache, with the shift that was assumed and the clones made ahead under it."""
        for key in [k for k, e in list(self.plans.items()) if e.stepper is stepper]:
            self._evict(key)
        if self.last is not None and self.last.entry.stepper is stepper:
            self.last = None
        self.last_shift = None
        self.ahead.clear()

    def _lookup(self, ii, jj, kk, n_buf, p_tot, fixedp, device):
        key = _key(ii, jj, kk, n_buf, p_tot, fixedp, device)
        hit = self.plans.get(key)
        if hit is not None:
            if all(r() is t for r, t in zip(hit.refs, (ii, jj, kk))):
                return hit
            self._evict(key)
        pend = self.pending.pop(key, None)
        if pend is not None:                          # prefetch is building exactly this one: wait for it
            future, box, held = pend
            future.result()
            if "stepper" in box and all(h is t for h, t in zip(held, (ii, jj, kk))):
                return self._store(key, box["stepper"], ii, jj, kk)
            if "error" in box and not isinstance(box["error"], Exception):
                raise box["error"]                    # KeyboardInterrupt and the like; ordinary errors are re-raised by the build below
        pl, ws = self._build(ii, jj, kk, n_buf, p_tot, fixedp, True)
        return self._store(key, pl if isinstance(pl, Stepper) else Stepper(pl, device, ws), ii, jj, kk)

    def _candidates(self, ii, n_buf, p_tot):
        """The cached plans a list may be a shift of — as many edges, in the same buffers — most recent first.  (The figures straight
        from the plans' dicts: every frame passes here.  A snapshot: the worker thread comes here while the cache may change.)"""
        E, nb, pt = ii.numel(), int(n_buf), int(p_tot)
        try:
            cached = list(self.plans.values())
        except RuntimeError:
            return
        for e in reversed(cached):
            inf = e.stepper.plan.info
            if inf["E"] == E and inf["n_buf"] == nb and inf["p_tot"] == pt:
                yield e

    def _assumed_source(self, ii, n_buf, p_tot, fixedp):
        """The cached plan a list is ASSUMED to be a shift of: the most recent one `last_shift` frames behind `fixedp` that is itself
        settled — the first such candidate, whatever becomes of the attempt."""
        if self.last_shift is None or _ladder(SPECULATIVE) < SPECULATIVE:
            return None
        fp = int(fixedp)
        for e in self._candidates(ii, n_buf, p_tot):
            if fp - e.stepper.plan.info["fixedp"] == self.last_shift and not e.stepper.plan.speculative:
                return e
        return None

    def _clone_ahead(self, ii, n_buf, p_tot, fixedp):
        """The probe: the clone made ahead that `_speculate` would try to bind to this list, or None.  Nothing is touched."""
        clone = self.ahead.get(self._assumed_source(ii, n_buf, p_tot, fixedp))
        return clone if clone is not None and clone.plan.info["fixedp"] == int(fixedp) else None

    def _speculate(self, ii, jj, kk, n_buf, p_tot, fixedp):
        """The plan of a list ASSUMED to be an earlier one moved up by the shift that was right last time — no synchronisation, no host
        wait, `settle` after the first step: a clone made ahead (with its stepper) bound to the list by one comparison kernel, else a
        clone made here (Plan.shifted_spec).  (plan or stepper, workspace to share) or None."""
        e = self._assumed_source(ii, n_buf, p_tot, fixedp)
        if e is None:
            return None
        clone = self.ahead.pop(e, None)
        if clone is not None and clone.plan.info["fixedp"] == int(fixedp) and clone.plan.bind(ii, jj, kk, n_buf, p_tot, fixedp):
            return clone, e.stepper.ws                # made (stepper and all) while the previous update()'s steps ran: only the comparison is left
        pl = Plan.shifted_spec(e.stepper.plan, ii, jj, kk, n_buf, p_tot, fixedp)
        return (pl, e.stepper.ws) if pl is not None else None

    def _build(self, ii, jj, kk, n_buf, p_tot, fixedp, sync, speculate=True):
        """A new plan: as a shifted copy of one of the most recent plans (the caller's window in steady state repeats its edge list
        with all frame / patch indices moved up, batrack.py:189-212, :858 — ~0.1 ms on the device), else from scratch (host analysis,
        ~1 ms for the 138k-edge window).  With `speculate` the copy is first made on an assumption (`_speculate`): BA_rgbd_droid settles
        it behind the call's step and repeats the call on a properly built plan where the assumption was wrong.
        Returns (plan or stepper, workspace to share or None)."""
        if speculate:
            got = self._speculate(ii, jj, kk, n_buf, p_tot, fixedp)
            if got is not None:
                return got
        if sync:
            # once, here: the index tensors must be complete before any of the builds below reads them on the plan stream
            # (Plan.shifted_any may return before it gets to synchronise, so nothing below relies on it having done so)
            _cuda.current_stream(ii.device).synchronize()
        if _ladder(SHIFTED) >= SHIFTED:
            fp = int(fixedp)
            cands = [e.stepper.plan for e in self._candidates(ii, n_buf, p_tot) if e.stepper.plan.info["fixedp"] < fp]
            # (with a keyframe stride of 2 the match is two updates back: the frame shift that worked last time is tried first)
            cands.sort(key=lambda pl: fp - pl.info["fixedp"] != self.last_shift)
            if cands:                                  # (one comparison pass and one host wait for all of them; a list that matches none is built the ordinary way)
                pl, matched = Plan.shifted_any(cands[:3], ii, jj, kk, n_buf, p_tot, fixedp, sync=False)
                if pl is not None:
                    self.last_shift = fp - matched.info["fixedp"]
                    return pl, None
        return Plan(ii, jj, kk, n_buf, p_tot, fixedp, sync=False), None


_PLANS = PlanCache()


def _print_residual(poses, patches, intrinsics, targets_2d, ii, jj, kk, bounds):
    """What the reference prints under PRINT=True (ba.py:244-245): the mean over the edges of |v * r|, r = target - reprojection,
    v = Z > 0.2 and |r| < 250 and inside the bounds (ba.py:228-242) — a debugging aid, computed beside the step (the fused
    reprojection kernel, include/batrack_projective.h) and synchronising like the reference's .item()."""
    from . import projective_ops as pops
    coords, v = pops.transform(poses, patches, intrinsics, ii, jj, kk, valid=True)
    p = coords.shape[3]
    c = coords[..., p // 2, p // 2, :]
    r = targets_2d - c
    v = (v[..., p // 2, p // 2] if v.dim() == 4 else v).reshape(r.shape[:-1]).float()
    v = v * (r.norm(dim=-1) < 250).float()
    v = v * ((c[..., 0] > bounds[0]) & (c[..., 1] > bounds[1]) & (c[..., 0] < bounds[2]) & (c[..., 1] < bounds[3])).float()
    print((r * v[..., None]).norm(dim=-1).mean().item())


def prefetch_plan(ii, jj, kk, n_buf, p_tot, fixedp, device=None, background=True):
    """Build the plan of an edge list ahead of the BA calls that will use it.

    The caller knows `(ii, jj, kk)` and `fixedp` of an `update()` as soon as it has appended / removed factors —
    a whole tracker pass before it calls `BA_rgbd_droid` (batrack.py:983-993: `append_factors`, then
    `predict_target`, then `update`).  Called there, this takes the per-frame plan (host analysis + table upload,
    ~1.5 ms for the 138k-edge window) off the critical path: a host thread builds it while the GPU and the main
    thread are busy; the first `BA_rgbd_droid` call with the same tensors picks it up (or waits for it).
    The index tensors must not be modified in place afterwards (the reference replaces them, it never edits them
    between `append_factors` and `update`)."""
    dev = torch.device(device) if device is not None else ii.device
    if dev.type != "cuda":
        raise RuntimeError("prefetch_plan: the edge list must be on the GPU (no CPU fallback in batrack_amd)")
    if ii.numel() == 0:
        return
    _lib.lib()
    _PLANS.prefetch(ii, jj, kk, n_buf, p_tot, fixedp, dev, background)


def clear_plan_cache():
    _PLANS.clear()


def _f32c(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"BA_rgbd_droid: `{what}` must be on the GPU (no CPU fallback in batrack_amd)")
    if t.dtype != torch.float32:
        raise TypeError(f"BA_rgbd_droid: `{what}` must be float32 (batrack.py:74-91), got {t.dtype}")
    return t


def _enqueue(stepper, P, patches, patches_monodisp, intrinsics, targets_2d, weights, bounds, lmbda, ep, alpha, loss, so, lm_trk):
    """The step of one call, enqueued on the current stream: (poses_out [1, n_buf, 7] — the input's where `so` —, out_patches
    [1, p_tot, 3, 1, 1])."""
    if stepper._ops is not None:
        # the whole call in ONE operator (csrc/torch_ops.cpp ba_droid: the views the ABI needs, the output tensors, the step):
        # the tensor operations below cost 28 us of host time a call, more than a structure-only step takes on the GPU
        return stepper._ops.ba_droid.default(stepper.plan.handle.value, stepper.ws, P, patches, patches_monodisp, intrinsics,
                                             targets_2d, weights, [float(b) for b in bounds], float(lmbda), float(ep),
                                             float(alpha), _lib.LOSS[loss], so, lm_trk)
    n_buf, p_tot, E = P.shape[1], patches.shape[1], targets_2d.numel() // 2
    Pc = P.contiguous()
    pat = patches.reshape(p_tot, 3).contiguous()
    mono = patches_monodisp
    if mono.numel() == p_tot and not mono.is_contiguous() and p_tot > 1:
        # the caller's prior is a strided view (patches_local[:, :, mid, 2:], batrack.py:866): used in place through mono_stride
        # (only a genuine stride >= 1: an expanded tensor — stride 0 — or a negative stride is materialised instead)
        d = [i for i, n in enumerate(mono.shape) if n == p_tot]
        if len(d) == 1 and mono.stride(d[0]) >= 1:
            mono = torch.as_strided(mono, (p_tot,), (mono.stride(d[0]),), mono.storage_offset())
        else:
            mono = mono.reshape(-1).contiguous()
    else:
        mono = mono.reshape(-1)
    intr = intrinsics.reshape(-1, 4).contiguous()
    tg = targets_2d
    tg = tg.reshape(E, 2) if tg.is_contiguous() else tg[0]
    if tg.stride(1) != 1:                          # the caller's view has strides (3, 1): used in place
        tg = tg.contiguous()
    w = weights.reshape(E, 2).contiguous()
    patches_out = torch.empty_like(pat)
    poses_out = Pc if so else torch.empty_like(Pc)
    stepper.step(Pc, pat, mono, intr, tg, tg.stride(0), w, poses_out, patches_out,
                 bounds, lmbda, ep, alpha, loss, so, lmbda_per_track=lm_trk)
    return poses_out.view(1, n_buf, 7), patches_out.view(1, p_tot, 3, 1, 1)


def BA_rgbd_droid(poses, patches, patches_monodisp, intrinsics, targets_2d, targets_disp, weights, lmbda,
                  ii, jj, kk, bounds, ep=100.0, PRINT=False, fixedp=1, structure_only=False,
                  loss='trivial', alpha=0.5):
    _lib.lib()                                   # raises if the HIP library is missing
    P = _f32c(poses.data, "poses")
    if P.dim() != 3 or P.shape[0] != 1 or P.shape[-1] != 7:
        raise ValueError("poses must wrap a [1, N, 7] tensor (batch b = 1, ba.py:218)")
    if patches.dim() == 5 and patches.shape[0] == 1 and patches.shape[2] == 3 and patches.shape[3] == patches.shape[4] and patches.shape[3] > 1:
        # Patch size p > 1 (BA-Track itself uses 1, batrack.py:45).  The reference projects the patch's CENTRE pixel (ba.py:228-230:
        # coords[..., p//2, p//2, :]), takes the depth prior at its first pixel (disps[:, kx, 0, 0], ba.py:307) and adds dZ to the
        # whole disparity plane of the patch (ba.py:332-334).  A patch's disparity plane holds ONE value in the reference's callers
        # (the tracker fills it per patch); for such patches that is the p = 1 step on the centres with the result broadcast
        # back.  Planes that are not constant are refused: the clamp of ba.py:333 would act on each pixel separately.
        pp = patches.shape[3]
        disps = patches[:, :, 2]
        if not bool((disps == disps[..., :1, :1]).all()):
            raise NotImplementedError("BA_rgbd_droid: patches of size > 1 whose disparity plane is not constant over the patch")
        centre = patches[:, :, :, pp // 2, pp // 2].contiguous()[..., None, None]
        new_poses, out_c = BA_rgbd_droid(poses, centre, patches_monodisp, intrinsics, targets_2d, targets_disp, weights, lmbda,
                                         ii, jj, kk, bounds, ep=ep, PRINT=PRINT, fixedp=fixedp, structure_only=structure_only,
                                         loss=loss, alpha=alpha)
        out = patches.clone()
        out[:, :, 2] = out_c[:, :, 2].expand(-1, -1, pp, pp)
        return new_poses, out
    if patches.dim() < 3 or patches.shape[0] != 1 or patches.shape[2] != 3 or patches.numel() != 3 * patches.shape[1]:
        raise ValueError("patches must be [1, P_tot, 3, p, p] (batrack.py:45: p = 1)")
    if loss not in _lib.LOSS:
        raise NotImplementedError(loss)              # ba.py:98-99
    n_buf, p_tot, E = P.shape[1], patches.shape[1], ii.numel()
    if E == 0:
        raise ValueError("empty edge list")
    dev = P.device
    for t, what in ((patches, "patches"), (patches_monodisp, "patches_monodisp"), (intrinsics, "intrinsics"), (targets_2d, "targets_2d"), (weights, "weights")):
        _f32c(t, what)
    if patches_monodisp.numel() != p_tot or intrinsics.numel() != 4 * n_buf:
        raise ValueError("patches_monodisp / intrinsics do not match the patch / pose buffers")
    if targets_2d.shape[-1] != 2 or targets_2d.numel() != 2 * E:
        raise ValueError("targets_2d must be [1, E, 2]")
    stepper, in_place = _PLANS.get(ii, jj, kk, n_buf, p_tot, fixedp, dev)
    lmbda_in = lmbda                             # (what a repeated call after a failed speculation must be given again)
    lm_trk = None
    if isinstance(lmbda, torch.Tensor):
        if lmbda.numel() == 1:
            lmbda = float(lmbda)
        else:
            # a per-track tensor is checked against the plan's track count: a speculative clone carries its SOURCE's count, so
            # the speculation is settled first (a wrong guess is rebuilt here, before anything is enqueued)
            if stepper.plan.speculative and not _PLANS.settle(stepper):
                stepper, in_place = _PLANS.get(ii, jj, kk, n_buf, p_tot, fixedp, dev)
        if isinstance(lmbda, float):
            pass
        elif lmbda.numel() == stepper.plan.m:           # ba.py:299-300: lmbda.reshape(*C.shape), one value per distinct track
            lm_trk = _f32c(lmbda, "lmbda").reshape(-1).contiguous()
            lmbda = 0.0
        else:
            raise ValueError(f"a lmbda tensor must hold 1 or m = {stepper.plan.m} values (ba.py:299-300), got {lmbda.numel()}")
    so = bool(structure_only) or stepper.plan.n == 0
    poses_out, out_patches = _enqueue(stepper, P, patches, patches_monodisp, intrinsics, targets_2d, weights, bounds, lmbda, ep, alpha,
                                      loss, so, lm_trk)
    if PRINT:
        _print_residual(poses, patches, intrinsics, targets_2d, ii, jj, kk, bounds)
    if stepper.plan.speculative and not _PLANS.settle(stepper):
        # the list was no shifted copy after all: what was just enqueued is void (the inputs are untouched) — once more, properly
        return BA_rgbd_droid(poses, patches, patches_monodisp, intrinsics, targets_2d, targets_disp, weights, lmbda_in, ii, jj, kk, bounds,
                             ep=ep, PRINT=False, fixedp=fixedp, structure_only=structure_only, loss=loss, alpha=alpha)
    if in_place:
        _PLANS.after_step()                      # (behind this call's launches: the clone for the next update()'s list)
    return (poses, out_patches) if so else (SE3(poses_out), out_patches)
