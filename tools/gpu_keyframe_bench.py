#!/usr/bin/env python3
"""Timing of the keyframe step (bt_keyframe_decide -> bt_edges_prune -> bt_rows_shift through
batrack_amd.frontend.keyframe.prune_keyframe) -> profiles/r15_keyframe.txt.

Window-shaped edge lists at the Sintel shape (M 256, about 138k edges) and the DAVIS shape (M 400, about 216k edges), grown
by the replay's own bookkeeping (sequence.WindowedBA with a BA that does nothing, ground-truth poses written in; n 37,
KEYFRAME_INDEX 5 so that the candidate has edges from both neighbours under kf_stride 2).  Three
calls per shape: keyframe() that removes the frame, keyframe() that keeps it, keyframe_simple().  Two formulations on the
same GPU, alternating in one process, each on a fresh copy of the state:
  new      prune_keyframe: at most six launches + the two SE3 launches of dP, one 32-byte read-back;
  parent   what the replay could do before: motionmag as boolean-mask gathers + pops.flow_mag + .mean().item() (twice),
           tstamps_[.].item() (twice), remove_factors as boolean-mask gathers (two rounds of six), the index fix-ups, and
           the reference's row-by-row copies of the buffers (batrack.py:1026-1073 restated in torch).
Host wall time around a synchronise (what a frame pays), median and 10 % / 90 % quantiles; device events around the three
stages alone (no read-back) for the kernels' time against the byte model: the index passes read 40 B per edge (decide
16 B, count 24 B), the scatter reads 52 B per edge and writes 52 B per kept edge.  Also the two magnitudes against a float64
evaluation, for the parent's fused float32 formulation and for the kernel, on the fixture of tests/golden/keyframe.npz.

    python tools/gpu_keyframe_bench.py [--reps 30] [--out profiles/r15_keyframe.txt]
    rocprofv3 --kernel-trace --memory-copy-trace -d DIR -- python tools/gpu_keyframe_bench.py --trace new --calls 3    (runs of their own)
    python tools/gpu_keyframe_bench.py --trace-db LABEL=DB ... --out FILE      (appends launches and read-backs per call)
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from batrack_amd import _lib, graphgen  # noqa: E402
from batrack_amd.backend import projective_ops as pops  # noqa: E402
from batrack_amd.backend.lietorch import SE3  # noqa: E402
from batrack_amd.frontend.keyframe import KeyframeConfig, prune_keyframe  # noqa: E402
from batrack_amd.sequence import SlamConfig, SyntheticObservations, WindowedBA  # noqa: E402

DEV = "cuda:0"
SHAPES = (("Sintel", 256, graphgen.SINTEL), ("DAVIS", 400, graphgen.DAVIS))
N_FRAMES = 37               # the frame that has just appended its factors: 540 edges per track slot
KF_INDEX = 5                # with kf_stride 2 the sources are the odd frames: k = n - 5 = 32 has edges from 31 and from 33
BUFFERS = ("tstamps_", "poses_", "patches_", "intrinsics_", "patches_local_", "patches_local_vis_", "patches_local_static_",
           "patches_local_weights_", "patches_valid_")
EDGES = ("ii", "jj", "kk", "targets_3d", "weights", "weights_pose")


def window_state(M, cam):
    """The replay's state after N_FRAMES frames (kf_stride 2, S_slam 12, REMOVAL_WINDOW 20), ground-truth poses, on the GPU."""
    obs = SyntheticObservations(n_frames=N_FRAMES, M=M, seed=1, cam=cam)
    cfg = SlamConfig(PATCHES_PER_FRAME=M, BUFFER_SIZE=N_FRAMES + 4, USE_MAP_FILTERING=False)
    trk = WindowedBA(obs, lambda Gs, patches, *a, **k: (Gs, patches), cfg, device=DEV)
    trk.run()
    trk.poses_[:N_FRAMES] = torch.as_tensor(obs.poses_gt, dtype=torch.float32, device=DEV)
    return trk


def snapshot(trk):
    return {k: getattr(trk, k).clone() for k in BUFFERS + EDGES}


def new_call(st, trk, thresh, candidate):
    cfg = KeyframeConfig(KEYFRAME_INDEX=KF_INDEX, KEYFRAME_THRESH=thresh, REMOVAL_WINDOW=trk.cfg.REMOVAL_WINDOW)
    return prune_keyframe(st["poses_"], st["patches_"].view(-1, 3, 1, 1), st["intrinsics_"], st["ii"], st["jj"], st["kk"], st["targets_3d"],
                          st["weights"], st["weights_pose"], n=trk.n, M=trk.M, kf_stride=2, cfg=cfg,
                          frame_buffers=[st[k] for k in BUFFERS], candidate=candidate)


def parent_call(st, trk, thresh, candidate):
    """batrack.py:1026-1073 / :1020-1024 in the torch operations the package had before the kernels."""
    n, M, N = trk.n, trk.M, trk.N
    ii, jj, kk, t3, w, wp = (st[k] for k in EDGES)

    def remove(mask):
        keep = ~mask
        return ii[keep], jj[keep], kk[keep], t3[:, keep], w[:, keep], wp[:, keep]
    if candidate:
        k = n - KF_INDEX
        G, pat, K = SE3(st["poses_"].view(1, N, 7)), st["patches_"].view(1, N * M, 3, 1, 1), st["intrinsics_"].view(1, N, 4)
        m = 0.0
        for i in (k - 1, k + 1):
            sel = (ii == i) & (jj == k)
            m += pops.flow_mag(G, pat, K, ii[sel], jj[sel], kk[sel], beta=0.5).mean().item()
        if m / 2 < thresh:
            t0, t1 = st["tstamps_"][k - 1].item(), st["tstamps_"][k].item()
            dP = SE3(st["poses_"][k][None]) * SE3(st["poses_"][k - 1][None]).inv()
            ii, jj, kk, t3, w, wp = remove((ii == k) | (jj == k))
            kk[ii > k] -= M
            ii[ii > k] -= 1
            jj[jj > k] -= 1
            for i in range(k, n - 1):
                for b in BUFFERS:
                    st[b][i] = st[b][i + 1]
            n -= 1
    return remove(kk // M < n - trk.cfg.REMOVAL_WINDOW)


CALLS = (("keyframe(), removed", 1e9, True), ("keyframe(), kept", -1.0, True), ("keyframe_simple()", 0.0, False))


def stage_events(st, trk, thresh, candidate, reps):
    """Device time of the three stages alone, enqueued through the C ABI (no dP, no read-back), us per call."""
    L = _lib.lib()
    E = st["ii"].numel()
    ws = torch.empty(L.bt_keyframe_workspace_bytes(E) // 8 + 1, dtype=torch.int64, device=DEV)
    k = trk.n - KF_INDEX if candidate else -1
    idx = [st[x] for x in ("ii", "jj", "kk")]
    pay = [st[x][0].contiguous() for x in ("targets_3d", "weights", "weights_pose")]
    outs = [torch.empty_like(t) for t in idx + pay]
    bufs = (_lib.RowBuffer * len(BUFFERS))(*[_lib.RowBuffer(st[b].data_ptr(), st[b][0].numel() * st[b].element_size()) for b in BUFFERS])
    s = torch.cuda.current_stream().cuda_stream
    P, pat, K = st["poses_"], st["patches_"], st["intrinsics_"]
    ts = []
    for r in range(reps + 5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        L.bt_keyframe_decide(k, *(t.data_ptr() for t in idx), E, P.data_ptr(), P.shape[0], pat.data_ptr(), trk.N * trk.M, 1, K.data_ptr(),
                             0.5, thresh, ws.data_ptr(), s)
        L.bt_edges_prune(k, trk.n, trk.M, trk.cfg.REMOVAL_WINDOW, *(t.data_ptr() for t in idx + pay), E, *(t.data_ptr() for t in outs),
                         ws.data_ptr(), s)
        if k >= 0:
            L.bt_rows_shift(bufs, len(BUFFERS), k, trk.n, ws.data_ptr(), s)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    Eo = int(ws[1].item())
    return np.array(ts[5:]), Eo


def wall_us(fn, state0, reps, warmup=3):
    ts = []
    for r in range(reps + warmup):
        st = {k: v.clone() for k, v in state0.items()}
        torch.cuda.synchronize()
        tic = time.perf_counter()
        fn(st)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - tic) * 1e6)
    return np.array(ts[warmup:])


def magnitudes(out):
    import keyframe_util as ku
    z = np.load(ku.GOLDEN)
    up = lambda a: torch.as_tensor(a.copy(), device=DEV)
    out("flow magnitudes on the fixture's pairs (tests/golden/keyframe.npz), relative error against a float64 torch evaluation:")
    worst = {"parent": 0.0, "kernel": 0.0}
    for c in ("a", "d", "f"):
        d = ku.load_case(c, z)
        n, k = int(d["n_in"]), int(d["n_in"]) - int(d["KEYFRAME_INDEX"])
        r = prune_keyframe(up(d["poses_in"]), up(d["patches_in"]).view(-1, 3, 1, 1), up(d["intrinsics_in"]), up(d["ii_in"]), up(d["jj_in"]),
                           up(d["kk_in"]), up(d["targets_3d_in"])[None], up(d["weights_in"])[None], up(d["weights_pose_in"])[None], n=n,
                           M=int(d["M"]), kf_stride=int(d["kf_stride"]), cfg=KeyframeConfig(KEYFRAME_INDEX=int(d["KEYFRAME_INDEX"]),
                           KEYFRAME_THRESH=-1.0, REMOVAL_WINDOW=int(d["REMOVAL_WINDOW"])))
        for i, got in ((k - 1, r.mag_prev), (k + 1, r.mag_next)):
            w = ku.mean_flow64(d["poses_in"], d["patches_in"], d["intrinsics_in"], d["ii_in"], d["jj_in"], d["kk_in"], i, k)
            if np.isnan(w):
                continue
            ii, jj, kk = up(d["ii_in"]), up(d["jj_in"]), up(d["kk_in"])
            sel = (ii == i) & (jj == k)
            par = pops.flow_mag(SE3(up(d["poses_in"])[None]), up(d["patches_in"]).reshape(1, -1, 3, 1, 1), up(d["intrinsics_in"])[None],
                                ii[sel], jj[sel], kk[sel], beta=0.5).mean().item()
            worst["parent"] = max(worst["parent"], abs(par - w) / w)
            worst["kernel"] = max(worst["kernel"], abs(got - w) / w)
            out(f"  case {c} ({i} -> {k}), {int(sel.sum())} edges: float64 {w:.9f}; parent's fused float32 mean {par:.9f} rel {abs(par - w) / w:.2e}; "
                f"kernel {got:.9f} rel {abs(got - w) / w:.2e}")
    out(f"  largest: parent {worst['parent']:.2e}, kernel {worst['kernel']:.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_keyframe.txt"))
    ap.add_argument("--trace", choices=("new", "parent"), help="--calls removing keyframe() calls at the DAVIS shape, nothing written: for rocprofv3")
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--trace-db", nargs="+", help="LABEL=DB pairs (new1, new3, parent1, parent3): append launches and read-backs per call, then exit")
    args = ap.parse_args()
    if args.trace_db:
        import sqlite3
        cnt = {}
        for item in args.trace_db:
            label, db = item.split("=", 1)
            cur = sqlite3.connect(db).cursor()
            kern = cur.execute("select count(*) from kernels").fetchone()[0]
            try:
                d2h = cur.execute("select count(*) from memory_copies where name like '%DEVICE_TO_HOST%'").fetchone()[0]
            except sqlite3.Error:
                d2h = None
            cnt[label] = (kern, d2h)
        with open(args.out, "a") as fh:
            fh.write("launches and read-backs of one removing keyframe() at the DAVIS shape, from rocprofv3 --kernel-trace --memory-copy-trace in runs "
                     f"of their own: (a run of 3 calls - a run of 1 call) / 2, less the {len(BUFFERS + EDGES)} clone launches of the call's fresh state copy\n")
            for f in ("new", "parent"):
                (k1, c1), (k3, c3) = cnt[f + "1"], cnt[f + "3"]
                rb = "not resolved by this trace:" if not c3 else f"{(c3 - c1) / 2:g}"
                fh.write(f"  {f}: {(k3 - k1) / 2 - len(BUFFERS + EDGES):g} kernel launches, {rb} device-to-host copies per call (totals {k1} / {k3} kernels)\n")
        return
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing is measured without one")
    if args.trace:
        trk = window_state(*SHAPES[1][1:])
        s0 = snapshot(trk)
        fn = new_call if args.trace == "new" else parent_call
        for _ in range(args.calls):
            fn({k: v.clone() for k, v in s0.items()}, trk, 1e9, True)
        torch.cuda.synchronize()
        return
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out(f"keyframe step on {torch.cuda.get_device_name(0)}: prune_keyframe (new) against the boolean-mask / .item() / row-copy formulation (parent)")
    out(f"host wall time around a synchronise, the two alternating, {args.reps} calls each on a fresh copy of the state; us median [10 % .. 90 %]")
    for name, M, cam in SHAPES:
        trk = window_state(M, cam)
        s0 = snapshot(trk)
        E = s0["ii"].numel()
        out(f"{name}: M {M}, n {trk.n}, E {E}, candidate k {trk.n - KF_INDEX}, {KF_INDEX - 1} rows of {len(BUFFERS)} buffers to move")
        for label, thresh, cand in CALLS:
            a = new_call({k: v.clone() for k, v in s0.items()}, trk, thresh, cand)
            b = parent_call({k: v.clone() for k, v in s0.items()}, trk, thresh, cand)
            same = all(torch.equal(x, y) for x, y in zip((a.ii, a.jj, a.kk, a.targets_3d, a.weights, a.weights_pose), b))
            t = {}
            for r in range(2):                                   # alternate the two formulations
                for f, fn in (("new", new_call), ("parent", parent_call)):
                    t.setdefault(f, []).append(wall_us(lambda st: fn(st, trk, thresh, cand), s0, args.reps // 2))
            q = {f: np.quantile(np.concatenate(v), [0.5, 0.1, 0.9]) for f, v in t.items()}
            dev, Eo = stage_events(s0, trk, thresh, cand, args.reps)
            bytes_ = (40 if cand else 24) * E + 52 * E + 52 * Eo
            if a.removed:
                bytes_ += 2 * sum(s0[k][0].numel() * s0[k].element_size() for k in BUFFERS) * (KF_INDEX - 1)
            dm = np.median(dev)
            out(f"  {label}: removed {a.removed}, E_out {a.ii.numel()}, same lists as the parent's: {same}; "
                f"new {q['new'][0]:.0f} [{q['new'][1]:.0f} .. {q['new'][2]:.0f}] us, parent {q['parent'][0]:.0f} [{q['parent'][1]:.0f} .. {q['parent'][2]:.0f}] us "
                f"= {q['parent'][0] / q['new'][0]:.1f}x; the stages' device time {dm:.1f} us [{np.quantile(dev, 0.1):.1f} .. {np.quantile(dev, 0.9):.1f}] "
                f"for {bytes_ / 1e6:.1f} MB of the byte model = {bytes_ / dm / 1e3:.0f} GB/s")
    magnitudes(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
