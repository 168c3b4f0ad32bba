"""Shared by the correlation-lookup tests, the fixture generator and the measurement tool: the seeded inputs, the numpy
restatement of include/batrack_corr.h, and the volume formulation (what the fused lookup replaces) in torch."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "corr_lookup.npz")

# the fixture's cases: (b) has odd map sizes (the pooling floors) and takes the generic kernel, (c) is the model's map size
CASES = dict(a=dict(seed=31, S=4, C=128, H=48, W=64, N=64, L=4, r=3),
             b=dict(seed=32, S=3, C=64, H=45, W=61, N=48, L=3, r=4),
             c=dict(seed=33, S=2, C=128, H=96, W=128, N=32, L=4, r=3))
N_SPECIAL = 8                # the first queries of every frame sit on chosen positions (make_inputs)


def make_inputs(seed, S, C, H, W, N, B=1, **_):
    """Standard-normal maps and targets, and a three-column coordinate tensor whose first two columns are (x, y): uniform
    over the map, about 15 % moved up to 8 pixels outside it; per frame query 0 on (0, 0), 1 on (W-1, H-1), 2 far outside
    at (-40, -40), 3 .. 7 on quarter-pixel positions.  Everything rounded to float32, returned as float64 arrays:
    fmaps [B,S,C,H,W], targets [B,S,N,C], coords3 [B,S,N,3]."""
    rng = np.random.default_rng(seed)
    fmaps = rng.standard_normal((B, S, C, H, W))
    targets = rng.standard_normal((B, S, N, C))
    x, y = rng.uniform(0, W - 1, (B, S, N)), rng.uniform(0, H - 1, (B, S, N))
    outside = rng.random((B, S, N)) < 0.15
    side = rng.integers(0, 4, (B, S, N))
    dist = rng.uniform(0.0, 8.0, (B, S, N))
    x = np.where(outside & (side == 0), -dist, np.where(outside & (side == 1), W - 1 + dist, x))
    y = np.where(outside & (side == 2), -dist, np.where(outside & (side == 3), H - 1 + dist, y))
    x[..., 0], y[..., 0] = 0.0, 0.0
    x[..., 1], y[..., 1] = W - 1.0, H - 1.0
    x[..., 2], y[..., 2] = -40.0, -40.0
    x[..., 3:N_SPECIAL], y[..., 3:N_SPECIAL] = np.round(x[..., 3:N_SPECIAL] * 4) / 4, np.round(y[..., 3:N_SPECIAL] * 4) / 4
    coords3 = np.stack([x, y, rng.uniform(0.1, 2.0, (B, S, N))], -1)
    r32 = lambda a: a.astype(np.float32).astype(np.float64)
    return r32(fmaps), r32(targets), r32(coords3)


def digest(a):
    """Three float64 sums that move when any element of the array does."""
    a = np.asarray(a, np.float64).ravel()
    return np.array([a.sum(), (a * a).sum(), (a * (np.arange(a.size) % 97)).sum()])


def level_sizes(H, W, L):
    return [(H >> l, W >> l) for l in range(L)]


def np_pyramid(fmaps, L):
    """[S', C, H, W] -> the L levels; a level is the 2 x 2 mean of the one before at stride 2, an odd last row / column dropped."""
    levels = [fmaps]
    for _ in range(L - 1):
        f = levels[-1]
        h, w = f.shape[-2] // 2, f.shape[-1] // 2
        q = f.dtype.type(0.25)
        levels.append((((f[..., 0:2 * h:2, 0:2 * w:2] + f[..., 0:2 * h:2, 1:2 * w:2]) + f[..., 1:2 * h:2, 0:2 * w:2])
                       + f[..., 1:2 * h:2, 1:2 * w:2]) * q)
    return levels


def np_corr_lookup(fmaps, targets, coords, L, r, dtype=np.float64):
    """include/batrack_corr.h in numpy, every operation in `dtype`.  fmaps [S', C, H, W], targets [S', N, C],
    coords [S', N, 2] -> [S', N, L * (2r+1)^2]."""
    fmaps, targets, coords = (np.asarray(a, dtype) for a in (fmaps, targets, coords))
    Sp, C = fmaps.shape[:2]
    D, d = 2 * r + 2, 2 * r + 1
    sqrt_c = dtype(np.sqrt(np.float32(C)))                           # the reference divides by a float32 square root
    sidx = np.arange(Sp)[:, None, None, None]
    out = []
    for l, F in enumerate(np_pyramid(fmaps, L)):
        Hl, Wl = F.shape[-2:]
        c = coords / dtype(2 ** l)
        x0, y0 = np.floor(c[..., 0]), np.floor(c[..., 1])
        fx, fy = (c[..., 0] - x0)[..., None, None], (c[..., 1] - y0)[..., None, None]
        xs = x0.astype(np.int64)[..., None] - r + np.arange(D)       # [S', N, D]
        ys = y0.astype(np.int64)[..., None] - r + np.arange(D)
        valid = ((ys >= 0) & (ys < Hl))[..., :, None] & ((xs >= 0) & (xs < Wl))[..., None, :]      # [S', N, Dy, Dx]
        rows = F.transpose(0, 2, 3, 1)[sidx, np.clip(ys, 0, Hl - 1)[..., :, None], np.clip(xs, 0, Wl - 1)[..., None, :]]
        dots = np.where(valid, np.einsum("snyxc,snc->snyx", rows, targets) / sqrt_c, dtype(0))
        dt = dots.transpose(0, 1, 3, 2)                              # [x, y]: the first window index moves x
        one = dtype(1)
        o = ((one - fx) * (one - fy) * dt[..., :d, :d] + fx * (one - fy) * dt[..., 1:, :d]
             + (one - fx) * fy * dt[..., :d, 1:] + fx * fy * dt[..., 1:, 1:])
        out.append(o.reshape(Sp, -1, d * d))
    return np.concatenate(out, -1)


def volume_pyramid(fmaps, L):
    """[B,S,C,H,W] -> the L levels [B*S,C,H_l,W_l] of the volume formulation (built once per block, as the fused pyramid is)."""
    import torch.nn.functional as F
    levels = [fmaps.reshape(-1, *fmaps.shape[2:])]
    for _ in range(L - 1):
        levels.append(F.avg_pool2d(levels[-1], 2, stride=2))
    return levels


def volume_lookup(fmaps, targets, coords, L, r, pyramid=None):
    """What the fused lookup replaces, in torch on the tensors' device and in their dtype: per level the full correlation
    volume by a matrix product, divided by sqrt(C), sampled bilinearly with zero padding at the window's positions.
    fmaps [B,S,C,H,W], targets [B,S,N,C], coords [B,S,N,2] -> [B,S,N,L*(2r+1)^2]; `pyramid`: volume_pyramid(fmaps, L), made
    here when not given."""
    import torch
    import torch.nn.functional as F
    B, S, C, H, W = fmaps.shape
    N, d = targets.shape[2], 2 * r + 1
    pyramid = volume_pyramid(fmaps, L) if pyramid is None else pyramid
    off = torch.arange(-r, r + 1, device=fmaps.device, dtype=fmaps.dtype)
    scale = torch.sqrt(torch.tensor(float(C), dtype=torch.float32, device=fmaps.device))
    out = []
    for l, f in enumerate(pyramid):
        Hl, Wl = f.shape[-2:]
        vol = (torch.matmul(targets.reshape(B * S, N, C), f.reshape(B * S, C, Hl * Wl)) / scale).reshape(B * S * N, 1, Hl, Wl)
        c = coords.reshape(B * S * N, 1, 1, 2) / 2 ** l
        gx = (c[..., 0] + off.view(1, d, 1)).expand(-1, d, d)        # the first window index moves x,
        gy = (c[..., 1] + off.view(1, 1, d)).expand(-1, d, d)        # the second moves y
        grid = torch.stack([2 * gx / (Wl - 1) - 1, 2 * gy / (Hl - 1) - 1], -1)
        smp = F.grid_sample(vol, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        out.append(smp.reshape(B, S, N, d * d))
    return torch.cat(out, -1)


def load_case(c):
    """The case's generated inputs (checked against the fixture's digests by the CPU test) as [S', ...] arrays with a
    two-column coords, and the spec."""
    spec = CASES[c]
    fmaps, targets, coords3 = make_inputs(**spec)
    return fmaps[0], targets[0], coords3[0], spec


# ---------------------------------------------------------------------------------- inputs at the limits (the *_limits tests)
def limit_inputs(seed, S, C, H, W, N):
    """make_inputs for any N >= 1: generated with at least N_SPECIAL queries and cut to the first N, so that the special
    queries come first — 0 on (0, 0), 1 on (W-1, H-1), 2 far outside, 3 .. on quarter-pixel positions.  Returns
    fmaps [S,C,H,W], targets [S,N,C], coords [S,N,2], float32 values as float64 arrays."""
    fmaps, targets, coords3 = make_inputs(seed, S, C, H, W, max(N, N_SPECIAL))
    return fmaps[0], targets[0, :, :N], coords3[0, :, :N, :2]


def edge_queries(H, W, r):
    """Coordinates a network can put out, as a list of (kind, x, y) with x, y float32 values:
    'nonfinite' — +inf, -inf or NaN in x, in y or in both (every output is NaN);  'far' — +-3e9, +-(1e6 +- 0.5), 2^24 + 1
    (every output is exactly 0);  'zero' — -0.0 and 1e-30 (the query on (0, 0), up to the gate);  'edge' — the integer
    positions W-1, W-1+r, W+r, -r, -r-1 and the same on y, the other coordinate inside the map (W+r and -r-1 are the first
    whose level-0 window is wholly outside: `outside` below)."""
    inf, nan, f = np.inf, np.nan, lambda v: float(np.float32(v))
    q = []
    for v in (inf, -inf, nan):
        q += [("nonfinite", v, 5.0), ("nonfinite", 5.0, v), ("nonfinite", v, v)]
    q += [("nonfinite", inf, nan), ("nonfinite", -inf, inf)]
    for v in (3e9, -3e9, 1e6 + 0.5, 1e6 - 0.5, -(1e6 + 0.5), -(1e6 - 0.5), 2.0 ** 24 + 1):
        q += [("far", f(v), 5.0), ("far", 5.0, f(v)), ("far", f(v), f(v))]
    q += [("far", f(3e9), f(-3e9))]
    q += [("zero", -0.0, -0.0), ("zero", f(1e-30), f(1e-30)), ("zero", -0.0, f(1e-30))]
    for v in (W - 1, W - 1 + r, -r):
        q += [("edge", float(v), 5.0)]
    for v in (H - 1, H - 1 + r, -r):
        q += [("edge", 5.0, float(v))]
    for v in (W + r, -r - 1):
        q += [("outside", float(v), 5.0)]
    for v in (H + r, -r - 1):
        q += [("outside", 5.0, float(v))]
    q += [("outside", float(W + r), float(-r - 1))]
    return q


def planted_inputs(seed, S, C, H, W, N, r):
    """limit_inputs with edge_queries(H, W, r) planted from query N_SPECIAL on in every frame.  Returns fmaps, targets,
    coords [S,N,2] (float64 arrays of float32 values), kinds [N] (the query's kind, '' for the others), and `calm`: coords
    with every planted query on (5, 5)."""
    fmaps, targets, coords = limit_inputs(seed, S, C, H, W, N)
    q = edge_queries(H, W, r)
    assert N >= N_SPECIAL + len(q)
    kinds = np.array([""] * N, dtype=object)
    calm = coords.copy()
    for k, (kind, x, y) in enumerate(q, N_SPECIAL):
        coords[:, k], calm[:, k], kinds[k] = (x, y), (5.0, 5.0), kind
    return fmaps, targets, coords, kinds, calm


def volume_lookup_cpu64(fmaps, targets, coords, L, r):
    """volume_lookup on the CPU in float64, numpy in and out: [S,C,H,W], [S,N,C], [S,N,2] -> [S,N,L*(2r+1)^2]."""
    import torch
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))[None]
    return volume_lookup(t(fmaps), t(targets), t(coords), L, r)[0].numpy()
