"""The first step of a frame on the device: the reference's `generate_patches(image)` (main/batrack.py:230-325) in the mode
`PATCH_GEN: grid_grad_<G>`, `init_depth(patches, depth, mode='dmap')` (:917-934) and the colour row of `colors_`
(:978-979), as at most two launches and no host read: bt_image_gradient -> bt_patch_generate
(batrack_amd/csrc/patch_gen.hip; include/batrack_patches.h holds the specification).

    r = generate_patches(image [3,H,W] uint8 | float32, depth [H,W] float32, cfg=PatchGenConfig(),
                         out_patches=self.patches_[self.n], out_colors=self.colors_[self.n])

`image` is taken as it lies: a permuted view of an [H,W,3] array costs no copy.  `draws=(ux, uy)`, each [G*G, 8*gm]
float32, are the two uniform draws of :291-292; `draws=None` draws them as the reference does, `torch.rand` twice, x
first, under `generator`.  `rows="reference"` ranks as the reference does (its normalised row is computed from the
normalised column, :307-309, so only the top of the gradient map is read); `rows="image"` ranks by the candidate's own
row.  Ties are broken as `torch.argsort(stable=True)` does.  `out_patches` ([M,3,1,1]) and `out_colors` ([M,3] uint8)
are rows of the caller's `patches_` / `colors_` buffers, written in place.

`r.g` is a view of a map buffer kept per device: the next call on that device overwrites it.  GPU tensors only; no CPU
fallback."""
import collections
import dataclasses

import torch

from .. import _lib


@dataclasses.dataclass
class PatchGenConfig:
    """The keys of the reference's `slam:` block this step reads (names kept; configs/davis_demo.yaml values)."""
    PATCH_GEN: str = "grid_grad_20"
    PATCHES_PER_FRAME: int = 400
    rows: str = "reference"

    def grid(self):
        """(G, gm): cells a side, patches a cell."""
        parts = str(self.PATCH_GEN).split("_")
        if len(parts) != 3 or parts[:2] != ["grid", "grad"] or not parts[2].isdigit() or int(parts[2]) < 1:
            raise ValueError(f"PATCH_GEN '{self.PATCH_GEN}' is not supported: only 'grid_grad_<G>' has a device path")
        G, M = int(parts[2]), int(self.PATCHES_PER_FRAME)
        if M < 1 or M % (G * G) != 0:
            raise ValueError(f"PATCHES_PER_FRAME {M} is not a positive multiple of the {G}x{G} cells of '{self.PATCH_GEN}'")
        if self.rows not in _lib.BT_PATCH_ROWS:
            raise ValueError(f"rows '{self.rows}' is neither 'reference' nor 'image'")
        return G, M // (G * G)


PatchResult = collections.namedtuple("PatchResult", "patches clr colors coords sel g")

_maps = {}


def _image(image, what):
    if not isinstance(image, torch.Tensor) or not image.is_cuda:
        raise RuntimeError(f"{what}: `image` must be a tensor on the GPU (there is no CPU fallback in batrack_amd)")
    if image.dim() != 3 or image.shape[0] != 3:
        raise RuntimeError(f"{what}: `image` must be [3, H, W]")
    if image.dtype == torch.uint8:
        return _lib.BT_IMAGE_U8
    if image.dtype == torch.float32:
        return _lib.BT_IMAGE_F32
    raise RuntimeError(f"{what}: `image` must be uint8 or float32")


def _gradient_into(image, dtype, g, what):
    _, H, W = image.shape
    st = torch.cuda.current_stream(image.device).cuda_stream
    _lib.check(_lib.lib().bt_image_gradient(image.data_ptr(), dtype, H, W, *image.stride(), g.data_ptr(), st), what)


def image_gradient(image):
    """`__image_gradient_2` (:214-221) of one image: [1, 1, (H+1)//4, (W+1)//4] float32, a fresh tensor."""
    dtype = _image(image, "image_gradient")
    _, H, W = image.shape
    g = torch.empty((1, 1, max((H + 1) // 4, 0), max((W + 1) // 4, 0)), dtype=torch.float32, device=image.device)
    with torch.cuda.device(image.device):
        _gradient_into(image, dtype, g, "bt_image_gradient")
    return g


def generate_patches(image, depth, cfg=None, *, draws=None, generator=None, out_patches=None, out_colors=None):
    """See the module's text.  Returns PatchResult(patches [1,M,3,1,1], clr [1,M,3], colors [M,3] uint8, coords [M,2],
    sel [M] int32, g [1,1,Hp,Wp])."""
    cfg = cfg or PatchGenConfig()
    G, gm = cfg.grid()
    dtype = _image(image, "generate_patches")
    dev = image.device
    _, H, W = image.shape
    if not isinstance(depth, torch.Tensor) or depth.device != dev or depth.dtype != torch.float32 or depth.numel() != H * W:
        raise RuntimeError("generate_patches: `depth` must be a float32 tensor of H*W elements on the image's GPU")
    depth = depth.reshape(H, W).contiguous()
    M, C = G * G * gm, 8 * gm
    with torch.cuda.device(dev):
        if draws is None:
            ux = torch.rand((G * G, C), device=dev, generator=generator)
            uy = torch.rand((G * G, C), device=dev, generator=generator)
        else:
            ux, uy = draws
            for t in (ux, uy):
                if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float32 or t.numel() != G * G * C:
                    raise RuntimeError(f"generate_patches: `draws` must be two float32 tensors of [{G * G}, {C}] on the image's GPU")
            ux, uy = ux.contiguous(), uy.contiguous()
        f32 = dict(dtype=torch.float32, device=dev)
        if out_patches is None:
            out_patches = torch.empty((M, 3, 1, 1), **f32)
        elif (not isinstance(out_patches, torch.Tensor) or out_patches.device != dev or out_patches.dtype != torch.float32
              or out_patches.numel() != 3 * M or not out_patches.is_contiguous()):
            raise RuntimeError(f"generate_patches: `out_patches` must be a contiguous float32 row of {M} x 3 on the image's GPU")
        if out_colors is None:
            out_colors = torch.empty((M, 3), dtype=torch.uint8, device=dev)
        elif (not isinstance(out_colors, torch.Tensor) or out_colors.device != dev or out_colors.dtype != torch.uint8
              or out_colors.numel() != 3 * M or not out_colors.is_contiguous()):
            raise RuntimeError(f"generate_patches: `out_colors` must be a contiguous uint8 row of {M} x 3 on the image's GPU")
        Hp, Wp = max((H + 1) // 4, 0), max((W + 1) // 4, 0)
        buf = _maps.get(dev)
        if buf is None or buf.numel() < Hp * Wp:
            buf = _maps[dev] = torch.empty(max(Hp * Wp, 1), **f32)
        g = buf[:Hp * Wp].view(1, 1, Hp, Wp)
        clr = torch.empty((1, M, 3), **f32)
        coords = torch.empty((M, 2), **f32)
        sel = torch.empty(M, dtype=torch.int32, device=dev)
        _gradient_into(image, dtype, g, "bt_image_gradient")
        a = _lib.PatchArgs(g=g.data_ptr(), Hp=Hp, Wp=Wp, image=image.data_ptr(), dtype=dtype, rows_mode=_lib.BT_PATCH_ROWS[cfg.rows],
                           H=H, W=W, stride_c=image.stride(0), stride_y=image.stride(1), stride_x=image.stride(2),
                           depth=depth.data_ptr(), ux=ux.data_ptr(), uy=uy.data_ptr(), G=G, gm=gm, patches=out_patches.data_ptr(),
                           clr=clr.data_ptr(), colors=out_colors.data_ptr(), coords=coords.data_ptr(), sel=sel.data_ptr())
        _lib.check(_lib.lib().bt_patch_generate(a, torch.cuda.current_stream(dev).cuda_stream), "bt_patch_generate")
    return PatchResult(out_patches.view(1, M, 3, 1, 1), clr, out_colors.view(M, 3), coords, sel, g)
