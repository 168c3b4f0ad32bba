"""Patch selection and depth initialisation of a new frame on the device: `image_gradient` and `generate_patches`
(batrack_amd/frontend/patches.py over csrc/patch_gen.hip) against the numpy / torch-CPU restatement of
include/batrack_patches.h (tests/patches_util.py) and the fixture made from the reference's unmodified `generate_patches`
and `init_depth` (tests/golden/patch_gen.npz)."""
import numpy as np
import pytest
import torch

import patches_util as pu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# 37x270: three workgroups across; the others: smaller than a pooling window's reach, a single cell, odd sides, the fixture's
SIDES = [(3, 3), (4, 4), (7, 7), (16, 16), (33, 65), (50, 70), (64, 96), (37, 270)]
LAYOUTS = ("u8_hwc", "u8_planar", "f32_planar")


@pytest.fixture(scope="module")
def golden():
    return np.load(pu.GOLDEN)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def to_device(chw, layout):
    """[3, H, W] numpy -> the GPU tensor of that layout, as a [3, H, W] view."""
    if layout == "u8_hwc":
        return torch.as_tensor(np.ascontiguousarray(chw.transpose(1, 2, 0)), device=DEV).permute(2, 0, 1)
    return torch.as_tensor(np.ascontiguousarray(chw.astype(np.float32 if layout == "f32_planar" else np.uint8)), device=DEV)


def device_image(d):
    im = torch.as_tensor(d["image"].copy(), device=DEV)
    return im.permute(2, 0, 1) if int(d["hwc"]) else im


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("H,W", SIDES)
def test_gradient_bit_equal_to_numpy(H, W, layout):
    from batrack_amd.frontend.patches import image_gradient
    rng = np.random.default_rng(H * 1000 + W)
    chw = rng.integers(0, 256, (3, H, W)).astype(np.uint8)
    img = to_device(chw, layout)
    g = image_gradient(img)
    want = pu.grad_map_np(chw if layout != "f32_planar" else chw.astype(np.float32))
    assert g.shape == (1, 1, (H + 1) // 4, (W + 1) // 4)
    assert same_bits(g[0, 0].cpu().numpy(), want)
    assert np.array_equal(img.cpu().numpy(), chw.astype(img.cpu().numpy().dtype))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("value", [0, 255])
def test_gradient_of_a_constant_image(value, layout):
    """All zero: a zero map.  All 255: only the border of the padded image carries a gradient."""
    from batrack_amd.frontend.patches import image_gradient
    chw = np.full((3, 50, 70), value, np.uint8)
    g = image_gradient(to_device(chw, layout))[0, 0].cpu().numpy()
    assert same_bits(g, pu.grad_map_np(chw))
    assert not g[1:-1, 1:-1].any() and bool(g[0].all()) == (value != 0) and bool(g[:, 0].all()) == (value != 0)


def test_gradient_of_unaligned_rows():
    """uint8 rows that start at every offset within a 4-byte word: the kernel fetches whole aligned words."""
    from batrack_amd.frontend.patches import image_gradient
    rng = np.random.default_rng(11)
    H, W = 21, 45                                             # 3*W and W are odd: the rows' alignment changes from row to row
    chw = rng.integers(0, 256, (3, H, W)).astype(np.uint8)
    want = pu.grad_map_np(chw)
    for off in range(4):
        buf = torch.zeros(3 * H * W + 8, dtype=torch.uint8, device=DEV)
        buf[off:off + 3 * H * W] = torch.as_tensor(np.ascontiguousarray(chw.transpose(1, 2, 0)).reshape(-1), device=DEV)
        assert same_bits(image_gradient(buf[off:off + 3 * H * W].view(H, W, 3).permute(2, 0, 1))[0, 0].cpu().numpy(), want), ("hwc", off)
        buf[off:off + 3 * H * W] = torch.as_tensor(chw.reshape(-1), device=DEV)
        assert same_bits(image_gradient(buf[off:off + 3 * H * W].view(3, H, W))[0, 0].cpu().numpy(), want), ("planar", off)
    # neither layout: a column stride of 2
    wide = torch.zeros((3, H, 2 * W), dtype=torch.uint8, device=DEV)
    wide[:, :, ::2] = torch.as_tensor(chw, device=DEV)
    assert same_bits(image_gradient(wide[:, :, ::2])[0, 0].cpu().numpy(), want)


@pytest.fixture(scope="module")
def through(golden):
    """Every fixture case through generate_patches with the recorded draws, once."""
    from batrack_amd.frontend.patches import PatchGenConfig, generate_patches
    out = {}
    for c in pu.CASES:
        d = pu.load_case(c, golden)
        G = int(d["G"])
        ins = dict(image=device_image(d), depth=torch.as_tensor(d["depth"].copy(), device=DEV),
                   ux=torch.as_tensor(d["ux"].copy(), device=DEV), uy=torch.as_tensor(d["uy"].copy(), device=DEV))
        r = generate_patches(ins["image"], ins["depth"], PatchGenConfig(f"grid_grad_{G}", G * G), draws=(ins["ux"], ins["uy"]))
        res = {k: getattr(r, k).cpu().numpy() for k in r._fields}
        out[c] = (d, ins, res)
    return out


@pytest.mark.parametrize("case", pu.CASES)
def test_fixture_through_the_kernels(through, case):
    d, ins, r = through[case]
    G = int(d["G"])
    M = G * G
    H, W = d["depth"].shape
    assert r["patches"].shape == (1, M, 3, 1, 1) and r["clr"].shape == (1, M, 3) and r["colors"].shape == (M, 3)
    assert r["colors"].dtype == np.uint8 and r["sel"].dtype == np.int32 and r["coords"].shape == (M, 2)
    # the map: the restatement bit for bit, the reference's CPU map within the derived bound
    assert same_bits(r["g"][0, 0], pu.grad_map_np(pu.image_chw(d)))
    assert (np.abs(r["g"][0, 0].astype(np.float64) - d["g"]) <= pu.G_RTOL * np.abs(d["g"])).all()
    # the selection: admissible everywhere; forced where one candidate stands alone, and there the reference's numbers
    assert pu.admissible(d["scores"], r["sel"], 1)
    one = pu.single_candidate_cells(d["scores"])
    pat = r["patches"].reshape(M, 3)
    assert np.array_equal(r["sel"][one], d["scores"].argmax(1)[one])
    assert same_bits(pat[one], d["patches"][one]) and same_bits(r["clr"][0][one], d["clr"][one])
    assert np.array_equal(r["colors"][one], torch.as_tensor(d["clr"][one]).to(torch.uint8).numpy())
    # every cell: the rows are the restatement's at the device's own selection
    xg, yg = pu.candidates(d["ux"], d["uy"], G, H, W)
    want = pu.patch_rows(pu.image_chw(d), d["depth"], xg, yg, r["sel"], 1)
    assert same_bits(pat, want["patches"]) and same_bits(r["clr"][0], want["clr"])
    assert same_bits(r["colors"], want["colors"]) and same_bits(r["coords"], want["coords"])
    if case == "B":
        assert np.isnan(pat[:, 2]).sum() == 1 and (pat[:, 2] == 100.0).any()
    # inputs untouched
    assert same_bits(ins["image"].cpu().numpy(), pu.image_chw(d)) and same_bits(ins["depth"].cpu().numpy(), d["depth"])
    assert same_bits(ins["ux"].cpu().numpy(), d["ux"]) and same_bits(ins["uy"].cpu().numpy(), d["uy"])


def test_rows_of_the_callers_buffers(through):
    from batrack_amd.frontend.patches import PatchGenConfig, generate_patches
    d, ins, first = through["A"]
    M = int(d["M"])
    patches_ = torch.full((4, M, 3, 1, 1), -7.0, device=DEV)
    colors_ = torch.full((4, M, 3), 9, dtype=torch.uint8, device=DEV)
    r = generate_patches(ins["image"], ins["depth"], PatchGenConfig("grid_grad_4", M), draws=(ins["ux"], ins["uy"]),
                         out_patches=patches_[2], out_colors=colors_[2])
    assert r.patches.data_ptr() == patches_[2].data_ptr() and r.colors.data_ptr() == colors_[2].data_ptr()
    assert same_bits(patches_[2].cpu().numpy(), first["patches"][0]) and same_bits(colors_[2].cpu().numpy(), first["colors"])
    for row in (0, 1, 3):
        assert bool((patches_[row] == -7.0).all()) and bool((colors_[row] == 9).all())
    with pytest.raises(RuntimeError):
        generate_patches(ins["image"], ins["depth"], PatchGenConfig("grid_grad_4", M), out_patches=patches_[:, 0])


@pytest.mark.parametrize("gm", [1, 2])
def test_rows_image_against_the_restatement(through, gm):
    from batrack_amd.frontend.patches import PatchGenConfig, generate_patches
    d, ins, _ = through["A"]
    G = int(d["G"])
    rng = np.random.default_rng(3)
    ux, uy = (d["ux"], d["uy"]) if gm == 1 else (rng.random((G * G, 8 * gm), np.float32), rng.random((G * G, 8 * gm), np.float32))
    up = lambda a: torch.as_tensor(a.copy(), device=DEV)
    r = generate_patches(ins["image"], ins["depth"], PatchGenConfig(f"grid_grad_{G}", G * G * gm, rows="image"), draws=(up(ux), up(uy)))
    want = pu.restate(pu.image_chw(d), d["depth"], ux, uy, G, gm, rows="image")
    sel = r.sel.cpu().numpy()
    assert pu.admissible(want["scores"], sel, gm)
    ref_mode = pu.restate(pu.image_chw(d), d["depth"], ux, uy, G, gm)
    assert not np.array_equal(want["sel"], ref_mode["sel"])                  # the two modes rank differently here
    at = pu.patch_rows(pu.image_chw(d), d["depth"], want["xg"], want["yg"], sel, gm)
    assert same_bits(r.patches.cpu().numpy().reshape(-1, 3), at["patches"]) and same_bits(r.clr[0].cpu().numpy(), at["clr"])
    assert same_bits(r.coords.cpu().numpy(), at["coords"])


def test_a_call_repeats_bit_for_bit(through):
    from batrack_amd.frontend.patches import PatchGenConfig, generate_patches
    d, ins, first = through["C"]
    G = int(d["G"])
    r = generate_patches(ins["image"], ins["depth"], PatchGenConfig(f"grid_grad_{G}", G * G), draws=(ins["ux"], ins["uy"]))
    for k in r._fields:
        assert same_bits(getattr(r, k).cpu().numpy(), first[k]), k


def test_default_draws_are_torch_rand_twice(through):
    from batrack_amd.frontend.patches import PatchGenConfig, generate_patches
    d, ins, _ = through["A"]
    cfg = PatchGenConfig("grid_grad_4", 32)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1234)
    a = generate_patches(ins["image"], ins["depth"], cfg, generator=gen)
    gen.manual_seed(1234)
    ux = torch.rand((16, 16), device=DEV, generator=gen)
    uy = torch.rand((16, 16), device=DEV, generator=gen)
    b = generate_patches(ins["image"], ins["depth"], cfg, draws=(ux, uy))
    for k in ("patches", "clr", "colors", "coords", "sel"):
        assert same_bits(getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()), k
    xg, yg = pu.candidates(ux.cpu().numpy(), uy.cpu().numpy(), 4, 64, 96)
    want = pu.patch_rows(pu.image_chw(d), d["depth"], xg, yg, a.sel.cpu().numpy(), 2)
    assert same_bits(a.coords.cpu().numpy(), want["coords"])


def test_cpu_tensors_raise(golden):
    from batrack_amd.frontend.patches import generate_patches, image_gradient
    d = pu.load_case("A", golden)
    img = torch.as_tensor(d["image"].copy()).permute(2, 0, 1)
    with pytest.raises(RuntimeError, match="GPU"):
        image_gradient(img)
    with pytest.raises(RuntimeError, match="GPU"):
        generate_patches(img, torch.as_tensor(d["depth"].copy()))
    with pytest.raises(RuntimeError, match="depth"):
        generate_patches(img.to(DEV), torch.as_tensor(d["depth"].copy()))
