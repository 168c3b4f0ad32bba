"""What the two clients of the convolution tile (csrc/conv_tile.hpp), encoder.py and tracker.py, share on the Python side:
the argument check, the packed-weight cache, the 3 x 3 repack, the `out` tensor and the ctypes route's workspace.  Private to
the front end; importing it loads no native library."""
import torch

from .. import _lib

KCHUNK = 8                   # BT_WINDOW_KCHUNK: input channels a K chunk


def _gpu(name, t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{what}: `{name}` must be a tensor on the GPU (there is no CPU fallback in batrack_amd)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{what}: `{name}` must be float32")
    return t.detach()


def cached(cache, owner, tensors, build, extra=()):
    """`build()`, kept in the weak dictionary `cache` under the module `owner` and redone when one of `tensors` (the first
    a weight) is replaced, written to (`_version`) or moved to another device, or when `extra` no longer compares equal."""
    key = tuple(v for t in tensors for v in (t.data_ptr(), t._version)) + (str(tensors[0].device),) + tuple(extra)
    hit = cache.get(owner)
    if hit is None or hit[0] != key:
        hit = cache[owner] = (key, build())
    return hit[1]


def bias_of(conv):
    return conv.bias.detach().float().contiguous()


def repack3x3(w):
    """[m, c, 3, 3] -> [c / 8, 9, 8, m]: packed[c // 8, 3 ky + kx, c % 8, o] = w[o, c, ky, kx], the layout the kernels stage.
    A permutation (any device)."""
    m, c = w.shape[:2]
    return w.detach().float().permute(1, 2, 3, 0).reshape(c // KCHUNK, KCHUNK, 9, m).permute(0, 2, 1, 3).contiguous()


def out_tensor(out, shape, device, what, text, same_device=True):
    """A new float32 tensor of `shape` on `device` when `out` is None; else `out`, which must be `text`."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
            and tuple(out.shape) == tuple(shape) and (out.device == device or not same_device)):
        raise RuntimeError(f"{what}: `out` must be {text}")
    return out


def scratch(nbytes, device, what):
    """The ctypes route's workspace of `nbytes` (0: the sizes are refused); it needs no initialisation."""
    if nbytes == 0:
        raise RuntimeError(f"{what}: " + _lib.ERRORS[_lib.BT_EUNSUPPORTED])
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)
