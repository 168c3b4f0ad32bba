#!/usr/bin/env python3
"""sha256 digests of everything the implicit-GEMM convolution kernels of csrc/conv_tile.hpp write (bt_embed_conv,
bt_encoder_head, bt_res_block, bt_encoder_stem), for comparing two builds of the library bit for bit -> profiles/r27_conv_tile.txt.

The library is the one batrack_amd._lib loads: BT_LIB_PATH names a measurement build (the parent's, built from a git worktree
into _var/parent/), nothing the tree's own.  Every call goes through ctypes to the C ABI on seeded inputs; the packed weights
are seeded values in the packed shapes.  For the head, the block and the stem the workspace is filled with zero bytes first and its
defined parts are digested too — the raw maps, the per-tile partials, the mean / rstd arrays — so that a sum whose order
changed is seen even where the output happens not to move.

    BT_LIB_PATH=_var/parent/libbatrack_ba.so python tools/gpu_conv_bits.py --out parent.json      (one fresh process per library)
    python tools/gpu_conv_bits.py --out branch.json
    python tools/gpu_conv_bits.py --compare parent.json branch.json                                  (exit status 1 on a difference)

Cases, the smallest that reach every path and one workload shape each:
  embed_conv  2 frames: 9 x 17, 16 x 33, 96 x 128
  head        2 frames: outputs 1 x 1, 9 x 17, 11 x 12 from levels of 2, 1, 1/2 and 1/4 of the output's sides (rounded up, one row
              more at the first); 96 x 128 from 192 x 256, 96 x 128, 48 x 64, 24 x 32
  block       the six (c_in, c_out, stride) shapes of the trunk at 2 x c_in x 11 x 19; 64 -> 64 stride 1 at 9 x 17, 64 -> 96 stride 2
              at 17 x 33, both on a 1 x 1 map; 64 -> 64 stride 1 at 1 x 64 x 192 x 256 and 128 -> 128 stride 1 at 2 x 128 x 24 x 32
  stem        2 frames of 3 x 1 x 1; 3 x 16 x 64 (two tiles, fewer than the three a workgroup takes, float4 rows); 3 x 31 x 67 (six
              tiles); 3 x 33 x 65 (nine tiles, 33 columns: scalar stores and k_stem_norm<1>); one frame of 3 x 384 x 512
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
C, EMB_CHUNKS, CA, CB, CC, CD, CMID, COUT = 128, 24, 64, 96, 128, 128, 256, 128
EMBED_CASES = ((2, 9, 17), (2, 16, 33), (2, 96, 128))
HEAD_CASES = ((2, (1, 1), None), (2, (9, 17), None), (2, (11, 12), None), (2, (96, 128), ((192, 256), (96, 128), (48, 64), (24, 32))))
SHAPES = ((64, 64, 1), (64, 96, 2), (96, 96, 1), (96, 128, 2), (128, 128, 1), (128, 128, 2))
BLOCK_CASES = tuple((2, ci, co, s, 11, 19) for ci, co, s in SHAPES) + (
    (2, 64, 64, 1, 9, 17), (2, 64, 96, 2, 17, 33), (2, 64, 64, 1, 1, 1), (2, 64, 96, 2, 1, 1), (1, 64, 64, 1, 192, 256), (2, 128, 128, 1, 24, 32))
CIMG, CSTEM = 3, 64
STEM_CASES = ((2, 1, 1), (2, 16, 64), (2, 31, 67), (2, 33, 65), (1, 384, 512))


def compare(a, b):
    A, B = json.load(open(a)), json.load(open(b))
    keys = sorted(set(A["digests"]) | set(B["digests"]))
    bad = [k for k in keys if A["digests"].get(k) != B["digests"].get(k)]
    for k in bad:
        print(f"DIFFERS {k}: {A['digests'].get(k)} {B['digests'].get(k)}")
    print(f"{len(keys)} digests ({A['library']} against {B['library']}): {len(bad)} differ")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A.json", "B.json"))
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    if not args.out:
        ap.error("--out or --compare")
    import torch
    from batrack_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing is digested without one")
    L, dig = _lib.lib(), {}
    st = lambda: torch.cuda.current_stream().cuda_stream

    def rnd(seed, *shape, scale=1.0):
        return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)

    def sha(key, t):
        torch.cuda.synchronize()
        dig[key] = hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()

    def zeros_ws(nbytes):
        return torch.zeros((nbytes + 7) // 8, dtype=torch.float64, device=DEV)

    def parts(key, ws, sizes):
        """`sizes`: (name, dtype, elements) of the workspace's parts in order, each beginning 16-byte aligned."""
        raw, off = ws.view(torch.uint8), 0
        for name, dtype, n in sizes:
            off = (off + 15) & ~15
            nb = n * torch.empty(0, dtype=dtype).element_size()
            sha(f"{key} {name}", raw[off:off + nb].view(dtype))
            off += nb

    tiles = lambda h, w: ((h + 7) // 8) * ((w + 15) // 16)

    freqs = (2.0 ** torch.linspace(0.0, 10.0, 10)).to(DEV)
    for k, (F, h, w) in enumerate(EMBED_CASES):
        fnet, dm = rnd(10 + k, F, C, h, w), rnd(20 + k, F, h, w, scale=3.0)
        zr = torch.stack([dm.min(), dm.max()])
        wp, bias = rnd(30 + k, EMB_CHUNKS, 9, 8, C, scale=0.03), rnd(40 + k, C, scale=0.3)
        out = torch.zeros(F, C, h, w, device=DEV)
        rc = L.bt_embed_conv(fnet.data_ptr(), *fnet.stride(), dm.data_ptr(), zr.data_ptr(), wp.data_ptr(), bias.data_ptr(), freqs.data_ptr(),
                             F, 0, F, h, w, C, out.data_ptr(), st())
        assert rc == _lib.BT_OK, rc
        sha(f"embed_conv {F} x {h} x {w} out", out)

    for k, (F, (h, w), sizes) in enumerate(HEAD_CASES):
        if sizes is None:
            sizes = ((2 * h + 1, 2 * w), (h, w), ((h + 1) // 2, (w + 1) // 2), ((h + 3) // 4, (w + 3) // 4))
        lv = [rnd(100 + 10 * k + i, F, c, *s) for i, (c, s) in enumerate(zip((CA, CB, CC, CD), sizes))]
        w2, b2 = rnd(150 + k, (CA + CB + CC + CD) // 8, 9, 8, CMID, scale=0.03), rnd(160 + k, CMID, scale=0.3)
        w3, b3 = rnd(170 + k, CMID, COUT, scale=0.06), rnd(180 + k, COUT, scale=0.3)
        ws = zeros_ws(L.bt_encoder_head_workspace_bytes(F, h, w))
        out = torch.zeros(F, COUT, h, w, device=DEV)
        lvs = [_lib.EncoderLevel(t.data_ptr(), *t.shape[1:], *t.stride()) for t in lv]
        rc = L.bt_encoder_head(*(ctypes.byref(v) for v in lvs), w2.data_ptr(), b2.data_ptr(), CMID, w3.data_ptr(), b3.data_ptr(), COUT, F, h, w,
                               ws.data_ptr(), out.data_ptr(), st())
        assert rc == _lib.BT_OK, rc
        key = f"head {F} x {h} x {w}"
        sha(f"{key} out", out)
        parts(key, ws, (("raw map", torch.float32, F * CMID * h * w), ("partials", torch.float64, F * tiles(h, w) * CMID * 2)))

    for k, (F, ci, co, s, h, w) in enumerate(BLOCK_CASES):
        x = rnd(200 + k, F, ci, h, w).abs()
        w1, b1 = rnd(250 + k, ci // 8, 9, 8, co, scale=0.05), rnd(300 + k, co, scale=0.3)
        w2, b2 = rnd(350 + k, co // 8, 9, 8, co, scale=0.05), rnd(400 + k, co, scale=0.3)
        wd, bd = (rnd(450 + k, ci, co, scale=0.15), rnd(500 + k, co, scale=0.3)) if s == 2 else (None, None)
        ho, wo, maps = (h - 1) // s + 1, (w - 1) // s + 1, 2 if s == 1 else 3
        ws = zeros_ws(L.bt_res_block_workspace_bytes(F, co, h, w, s))
        out = torch.zeros(F, co, ho, wo, device=DEV)
        lx = _lib.EncoderLevel(x.data_ptr(), *x.shape[1:], *x.stride())
        blk = _lib.ResBlock(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), wd.data_ptr() if s == 2 else None,
                            bd.data_ptr() if s == 2 else None, ci, co, s)
        rc = L.bt_res_block(ctypes.byref(lx), ctypes.byref(blk), F, ws.data_ptr(), out.data_ptr(), st())
        assert rc == _lib.BT_OK, rc
        key = f"block {ci} -> {co} stride {s} at {F} x {ci} x {h} x {w}"
        sha(f"{key} out", out)
        parts(key, ws, (("raw maps", torch.float32, maps * F * co * ho * wo), ("partials", torch.float64, maps * F * tiles(ho, wo) * co * 2),
                        ("mean, rstd", torch.float32, maps * F * co * 2)))

    for k, (F, h, w) in enumerate(STEM_CASES):
        x = rnd(600 + k, F, CIMG, h, w)
        wp, bias = rnd(650 + k, 7, CIMG, 8, CSTEM, scale=0.1), rnd(700 + k, CSTEM, scale=0.3)
        wp[:, :, 7, :] = 0.0                                           # the eighth kx is a zero weight
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        ws = zeros_ws(L.bt_encoder_stem_workspace_bytes(F, h, w))
        out = torch.zeros(F, CSTEM, ho, wo, device=DEV)
        lx = _lib.EncoderLevel(x.data_ptr(), *x.shape[1:], *x.stride())
        rc = L.bt_encoder_stem(ctypes.byref(lx), wp.data_ptr(), bias.data_ptr(), CSTEM, F, ws.data_ptr(), out.data_ptr(), st())
        assert rc == _lib.BT_OK, rc
        key = f"stem {F} x {CIMG} x {h} x {w}"
        sha(f"{key} out", out)
        parts(key, ws, (("partials", torch.float64, F * tiles(ho, wo) * CSTEM * 2), ("mean, rstd", torch.float32, F * CSTEM * 2)))

    with open(args.out, "w") as fh:
        json.dump({"library": _lib.LIB_PATH, "device": torch.cuda.get_device_name(0), "digests": dig}, fh, indent=1)
    print(f"{len(dig)} digests of {_lib.LIB_PATH} -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
