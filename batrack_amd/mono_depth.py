"""The mono-depth stage's numeric step (main/mono_depth/get_mono_depth.py) on the HIP kernels: relative mono disparity
(DepthAnything) aligned to metric depth (UniDepth), bit for bit what the reference computes in numpy.

  align_mono_depth    GPU tensors in, GPU tensors out (bt_mono_align, include/batrack_depth.h); nothing synchronises.
  intrinsics_to_fov, align_depth, align_davis_demo
                      the reference's file-level functions with its signatures: they find, read and write the same files.
The camera matrix K is host arithmetic on T scalars and stays in numpy."""
import glob
import os

import numpy as np
import torch

from . import _lib

_DTYPES = {torch.float32: _lib.BT_DEPTH_F32, torch.float64: _lib.BT_DEPTH_F64}


def align_mono_depth(mono_disp, metric_depth, *, out=None, return_stats=False):
    """get_mono_depth.py:52-140 for a scene of T frames on the device: `mono_disp` [T,H,W] (cast to float32, as the reference
    casts it) and `metric_depth` [T,H,W] float32 or float64, GPU tensors of the same resolution.  Returns the metric depth
    [T,H,W] in metric_depth's dtype (into `out` if given: a contiguous tensor of that shape, dtype and device).
    Enqueued on the current stream; nothing synchronises unless `return_stats`, which also returns the per-frame scales and
    shifts ([T] GPU tensors), the aligns (a_s, a_c, n) as a [3] GPU tensor and k, the frame whose (scale, shift) is used,
    as an int."""
    for name, x in (("mono_disp", mono_disp), ("metric_depth", metric_depth)):
        if not isinstance(x, torch.Tensor):
            raise TypeError(f"align_mono_depth: {name} must be a torch tensor on the GPU, not {type(x).__name__}")
    if metric_depth.dtype not in _DTYPES:
        raise TypeError(f"align_mono_depth: metric_depth must be float32 or float64, not {metric_depth.dtype}")
    if mono_disp.dtype not in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
        raise TypeError(f"align_mono_depth: mono_disp must be a floating-point tensor, not {mono_disp.dtype}")
    if metric_depth.dim() != 3 or metric_depth.numel() == 0:
        raise ValueError(f"align_mono_depth: metric_depth must be a non-empty [T,H,W] tensor, not {tuple(metric_depth.shape)}")
    if mono_disp.shape != metric_depth.shape:
        raise ValueError(f"align_mono_depth: mono_disp {tuple(mono_disp.shape)} and metric_depth {tuple(metric_depth.shape)} must "
                         "have the same frames and resolution (resampling between resolutions is not provided)")
    if not (mono_disp.is_cuda and metric_depth.is_cuda) or mono_disp.device != metric_depth.device:
        raise RuntimeError("align_mono_depth: mono_disp and metric_depth must be tensors on the same GPU (no CPU fallback in batrack_amd)")
    dev = metric_depth.device
    mono = mono_disp.to(torch.float32).contiguous()
    metric = metric_depth.contiguous()
    if out is None:
        out = torch.empty_like(metric)
    elif (not isinstance(out, torch.Tensor) or out.shape != metric.shape or out.dtype != metric.dtype or out.device != dev
          or not out.is_contiguous()):
        raise ValueError("align_mono_depth: `out` must be a contiguous tensor of metric_depth's shape, dtype and device")
    T = metric.shape[0]
    hw, dt = metric.numel() // T, _DTYPES[metric.dtype]
    L = _lib.lib()
    wb = L.bt_mono_align_workspace_bytes(T, hw, dt)
    if wb < 0:
        _lib.check(int(wb), "bt_mono_align_workspace_bytes")
    ws = torch.empty(int(wb), dtype=torch.uint8, device=dev)
    stats = None
    if return_stats:
        stats = (torch.empty(T, dtype=metric.dtype, device=dev), torch.empty(T, dtype=metric.dtype, device=dev),
                 torch.empty(3, dtype=metric.dtype, device=dev), torch.empty(1, dtype=torch.int64, device=dev))
    ptr = lambda i: stats[i].data_ptr() if stats else None
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(L.bt_mono_align(mono.data_ptr(), metric.data_ptr(), T, hw, dt, out.data_ptr(), ptr(0), ptr(1), ptr(2), ptr(3),
                                   ws.data_ptr(), st), "bt_mono_align")
    if not return_stats:
        return out
    return out, stats[0], stats[1], stats[2], int(stats[3].item())


def intrinsics_to_fov(K, depth):
    """The horizontal field of view in degrees of the camera matrix K for an image as wide as `depth` (get_mono_depth.py:10-18),
    in K's dtype."""
    width = depth.shape[-1]
    return np.rad2deg(2 * np.arctan(width / (2 * K[0, 0])))


def scene_intrinsics(fovs, height, width):
    """K of get_mono_depth.py:105-120: the focal length of the median field of view for an image of height x width, the
    principal point at its centre (float64 [3, 3]; the focal length is computed in the fovs' dtype)."""
    half = np.median(fovs) / 2.0
    focal = width / (2 * np.tan(np.radians(half)))
    K = np.eye(3)
    K[0, 0] = focal * 1.0
    K[1, 1] = focal * 1.0
    K[0, 2] = width / 2.0
    K[1, 2] = height / 2.0
    return K


def _image_size(path):
    """(height, width) of an image as cv2.imread(path).shape[:2] gives it.  cv2 applies an EXIF orientation: one other than 1
    would swap or mirror the axes, so it is refused."""
    from PIL import Image
    with Image.open(path) as im:
        orientation = im.getexif().get(0x0112, 1)
        if orientation != 1:
            raise ValueError(f"{path}: EXIF orientation {orientation} is not supported (cv2.imread would rotate the image)")
        width, height = im.size
    return height, width


def align_depth(mono_depth_path, metric_depth_path, scene_name, datapath, save_depth_dir, save_K_dir):
    """get_mono_depth.py:21-150 with the alignment on the GPU: the scene's `<mono_depth_path>/<scene_name>/*.npy` disparities and
    `<metric_depth_path>/<scene_name>/*.npz` metric depths (keys 'depth', 'intrinsics'), paired in sorted order up to the shorter
    list; the first image of `datapath` (*.jpg, then *.png) gives the image size.  Writes `<name>.npy` (the depth, in the metric
    depth's dtype) to save_depth_dir and `<name>_intrinsics.npy` (K, float64) to save_K_dir for every pair, `<name>` the metric
    file's basename: the reference's files, bit for bit."""
    os.makedirs(save_depth_dir, exist_ok=True)
    os.makedirs(save_K_dir, exist_ok=True)
    print(datapath)
    images = sorted(glob.glob(os.path.join(str(datapath), "*.jpg"))) + sorted(glob.glob(os.path.join(str(datapath), "*.png")))
    mono_files = sorted(glob.glob(os.path.join(f"{mono_depth_path}/{scene_name}", "*.npy")))
    metric_files = sorted(glob.glob(os.path.join(f"{metric_depth_path}/{scene_name}", "*.npz")))
    print(f"Found {len(mono_files)} mono depth files and {len(metric_files)} metric depth files for scene: {scene_name}")
    if len(mono_files) != len(metric_files):
        print(f"WARNING: Mismatch in number of depth files! Mono: {len(mono_files)}, Metric: {len(metric_files)}")
    height, width = _image_size(images[0])
    monos, metrics, fovs = [], [], []
    for mono_file, metric_file in zip(mono_files, metric_files):
        mono = np.float32(np.load(mono_file))
        with np.load(metric_file) as z:
            depth, K = z["depth"], z["intrinsics"]
        fovs.append(intrinsics_to_fov(K, depth))
        if mono.shape != depth.shape:
            raise ValueError(f"{mono_file} {mono.shape} and {metric_file} {depth.shape}: resampling between resolutions is not provided")
        monos.append(mono)
        metrics.append(depth)
    if not metrics:
        raise ValueError(f"align_depth: no pair of mono and metric depth files for scene {scene_name}")
    dtypes = {m.dtype for m in metrics}
    if len(dtypes) != 1 or metrics[0].dtype not in (np.float32, np.float64):
        raise TypeError(f"align_depth: the metric depths must all be float32 or all float64, not {sorted(map(str, dtypes))}")
    if not torch.cuda.is_available():
        raise RuntimeError("align_depth: needs a GPU (no CPU fallback in batrack_amd)")
    dev = torch.device("cuda", torch.cuda.current_device())
    depth = align_mono_depth(torch.as_tensor(np.stack(monos), device=dev), torch.as_tensor(np.stack(metrics), device=dev)).cpu().numpy()
    K = scene_intrinsics(fovs, height, width)
    for t, metric_file in enumerate(metric_files[:len(metrics)]):
        name = os.path.basename(metric_file.replace(".npz", ""))
        np.save(os.path.join(save_depth_dir, name + ".npy"), depth[t])
        np.save(os.path.join(save_K_dir, name + "_intrinsics.npy"), K)


def align_davis_demo(depth_dir, data_dir, save_name="unidepth_da"):
    """get_mono_depth.py:154-166: align_depth for every scene under `<depth_dir>/depthAny_disp`, with the metric depths of
    `<depth_dir>/unidepthv2`, the images of `<data_dir>/<scene>`, and the results under `<depth_dir>/<save_name>/<scene>` and
    `<depth_dir>/<save_name>_intrinsics/<scene>`."""
    metric_depth_path = f"{depth_dir}/unidepthv2"
    mono_depth_path = f"{depth_dir}/depthAny_disp"
    for scene_name in os.listdir(mono_depth_path):
        print(scene_name)
        align_depth(mono_depth_path, metric_depth_path, scene_name, f"{data_dir}/{scene_name}",
                    f"{depth_dir}/{save_name}/{scene_name}", f"{depth_dir}/{save_name}_intrinsics/{scene_name}")
