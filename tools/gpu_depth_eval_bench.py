#!/usr/bin/env python3
"""Timing of the global-alignment stage's output and depth metrics at the Sintel size (50 x 436 x 1024 = 22.3M pixels):
bt_ga_scaled_dmaps (byte model 8 B/pixel) and bt_depth_metrics (median: 4 radix passes + the metric pass at ~9 B/pixel each;
lstsq: 2 passes; none: 1), by CUDA events over repeated calls; the same metrics in numpy on the host (tests/depth_util.py,
the reference's compute_errors arithmetic); one global_alignment_loop iteration at T = 50.  Run under rocprofv3
--kernel-trace --stats for the per-kernel times.

    python tools/gpu_depth_eval_bench.py [--reps 50] [--no-host]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from batrack_amd import _lib  # noqa: E402
from batrack_amd.evaluation import depth_metrics  # noqa: E402

HBM_PEAK = 8.0e12                                            # B/s, spec


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3                    # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    dev = "cuda:0"
    T, H, W = 50, 436, 1024
    n = T * H * W
    g = torch.Generator(device=dev).manual_seed(0)
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    print(f"device {torch.cuda.get_device_name(0)}; T x H x W = {T} x {H} x {W} = {n / 1e6:.1f}M pixels; HBM peak {HBM_PEAK / 1e12:.1f} TB/s (spec)")

    dm = torch.rand(T, 1, H, W, generator=g, device=dev) * 10 + 0.5
    out = torch.empty_like(dm)
    for gh, gw in ((4, 4), (12, 12)):
        fs = torch.randn(T, gh, gw, generator=g, device=dev)
        sh = torch.zeros(T, device=dev)
        call = lambda: _lib.check(L.bt_ga_scaled_dmaps(dm.data_ptr(), fs.data_ptr(), sh.data_ptr(), out.data_ptr(), T, gh, gw, H, W, st), "scaled")
        us = timed(call, args.reps)
        by = 8.0 * n
        print(f"bt_ga_scaled_dmaps grid {gh}x{gw}: {us:8.1f} us  {by / us / 1e3:7.0f} GB/s = {100 * by / us / 1e-6 / HBM_PEAK:4.1f} % of peak "
              f"(byte model {by / 1e6:.0f} MB)")

    gt = torch.exp(torch.rand(T, H, W, generator=g, device=dev) * 6.0 - 1.5)
    pred = gt * 0.4 * torch.exp(0.3 * torch.randn(T, H, W, generator=g, device=dev))
    mask = (torch.rand(T, H, W, generator=g, device=dev) < 0.9).to(torch.uint8)
    ws = torch.empty(int(L.bt_depth_metrics_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    res = torch.empty(11, dtype=torch.float64, device=dev)
    passes = {"none": 1, "median": 5, "lstsq": 2}
    for name, code in (("none", 0), ("median", 1), ("lstsq", 2)):
        call = lambda: _lib.check(L.bt_depth_metrics(gt.data_ptr(), pred.data_ptr(), mask.data_ptr(), n, 1e-2, 1e2, code, ws.data_ptr(),
                                                     res.data_ptr(), st), "metrics")
        us = timed(call, args.reps)
        by = 9.0 * n * passes[name]
        print(f"bt_depth_metrics {name:6s}: {us:8.1f} us  ({passes[name]} passes over 9 B/pixel: {by / us / 1e3:7.0f} GB/s = "
              f"{100 * by / us / 1e-6 / HBM_PEAK:4.1f} % of peak)")
    r = depth_metrics(gt, pred, mask.bool())
    print("metrics (median):", np.array2string(r[:8], precision=5), "count", int(r[8]))

    if not args.no_host:
        from depth_util import np_depth_metrics
        gh_, ph_, mh_ = gt.cpu().numpy(), pred.cpu().numpy(), mask.cpu().numpy().astype(bool)
        t0 = time.perf_counter()
        ref = np_depth_metrics(gh_, ph_, mh_, scaling="median")
        t1 = time.perf_counter()
        print(f"numpy compute_errors (median) on the host, same arrays: {(t1 - t0) * 1e3:8.1f} ms  "
              f"(threads: OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS')}); max rel diff of the 5 sums "
              f"{np.abs(r[:5] / ref[:5] - 1).max():.1e}, a1..a3 equal: {bool((r[5:8] == ref[5:8]).all())}")

    from test_gpu_global_refine import make_case
    from batrack_amd.global_refine import RefineLosses, global_alignment_iter
    d = make_case(50, 256, 11, seed=1)
    t = lambda k: torch.as_tensor(np.asarray(d[k]), device=dev)
    net = RefineLosses(t("trajs_2d"), t("trajs_disp"), t("trajs_disp_mono"), t("trajs_vis"), t("trajs_static"), t("jj"), t("intrinsics"),
                       t("grid_query_frames"), t("trajs_scales"), t("frame_scales_"), t("frame_shifts"), t("pose"), H, W, 20.0,
                       loss_weight_dict={"spatial_loss": 5.0, "inter_frame_loss": 0.3, "pts_3d_loss": 1.0, "cam_smooth_vec_loss": 1.0,
                                         "scale_smoothness_loss": 0.3}, refine_intrinsics=True)
    ps = [net.trajs_scales, net.frame_scales_, net.pose, net.K]
    for p in ps:
        p.requires_grad_(True)
    opt = torch.optim.Adam([{"params": [p], "lr": 1e-2} for p in ps], lr=1e-2, betas=(0.9, 0.9))
    it = lambda k: global_alignment_iter(net, k, 20, 1e-2, 1e-6, opt, "cosine")
    it(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(1, 11):
        it(k)
    torch.cuda.synchronize()
    print(f"global_alignment_iter T=50 N=256 S=11 (run_global_refine.py weights, pose and K free): "
          f"{(time.perf_counter() - t0) / 10 * 1e3:8.2f} ms per iteration (wall, incl. the loss read back)")


if __name__ == "__main__":
    main()
