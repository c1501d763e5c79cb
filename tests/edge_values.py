"""Helper of test_gpu_edge_values.py, test_edge_values_cpu.py and test_oracle_ops.py (not collected by pytest): the planes,
flow fields and special patterns on which the non-convolution kernels, their oracle twins and the torch operations they
restate are compared as bit patterns.

  SPECIALS          +-0, +-2^-149, +-0.5, +-1.5, +-2.5, 2^23+1, +-inf, two NaN payloads, FLT_MAX
  pixel / quantised / subnormal / islands     image planes (N, C, H, W)
  flow()            one flow field of a named kind
  warp_classes()    which edge classes of flow_warp a (plane, flow) pair reaches, from a numpy restatement of its coordinates
  bits_equal()      math_sweep.compare on two arrays: NaN payloads exempt and counted
"""
import numpy as np

import math_sweep as ms

F = np.float32


def bits(*u):
    return np.array(u, np.uint32).view(np.float32)


SPECIALS = bits(0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x3f000000, 0xbf000000, 0x3fc00000, 0xbfc00000,
                0x40200000, 0xc0200000, 0x4b000001, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001, 0x7f7fffff)
assert SPECIALS[10] == F(2 ** 23 + 1) and SPECIALS[15] == np.finfo(F).max and SPECIALS[8] == F(2.5)

NEG0 = bits(0x80000000)[0]


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def pixel(shape, seed=1):
    """the pixel image: uniform in [0, 255)"""
    return (_rng(seed, *shape).random(shape, dtype=F) * 255).astype(F)


def quantised(shape, seed=2):
    """the quantised image: rint(N(0, 0.6)), about 60 % zeros of both signs (rint of a small negative number is -0).
    Where the plane has room: an all -0 2x2 window at the top left, a window that mixes the signs next to it, and a 3x3
    block of -0 in the interior."""
    x = np.rint(_rng(seed, *shape).standard_normal(shape) * 0.6).astype(F)
    H, W = shape[-2:]
    if H >= 2 and W >= 2:
        x[..., 0:2, 0:2] = NEG0
    if H >= 2 and W >= 4:
        x[..., 0:2, 2:4] = np.array([[NEG0, 0.0], [0.0, NEG0]], F)
    if H >= 7 and W >= 7:
        x[..., 3:6, 3:6] = NEG0
    return x


def subnormal(shape, seed=3):
    """subnormals of both signs, a third of the elements zeros of both signs"""
    r = _rng(seed, *shape)
    u = r.integers(1, 1 << 23, shape, dtype=np.uint32)
    u[r.random(shape) < 1 / 3] = 0
    u |= r.integers(0, 2, shape, dtype=np.uint32) << np.uint32(31)
    return u.view(F)


def islands(shape, seed=4):
    """ordinary values with +inf, -inf and NaN islands (single elements and, where the plane has room, a 2x2 block each)"""
    r = _rng(seed, *shape)
    x = (r.standard_normal(shape) * 10).astype(F)
    pick = r.random(shape)
    x[pick < 0.02] = np.inf
    x[(pick >= 0.02) & (pick < 0.04)] = -np.inf
    x[(pick >= 0.04) & (pick < 0.06)] = np.nan
    H, W = shape[-2:]
    if H >= 8 and W >= 8:
        x[..., 0:2, 4:6], x[..., 4:6, 0:2], x[..., 6:8, 6:8] = np.inf, -np.inf, np.nan
    x.reshape(-1)[0] = np.nan                         # the smallest planes get one too
    return x


def minus_zero_windows():
    """(1, 1, 4, 6): six 2x2 windows whose plain sum or quotient is -0 — four -0 (x3, x1 below), one -2^-149 among -0 (the
    quotient -2^-151 rounds to -0) — and one of four -2^-149, whose quotient is -2^-149.  F.avg_pool2d gives +0 for the
    first five: its sum starts at +0 and its quotient is added to a zeroed output."""
    x = np.full((1, 1, 4, 6), NEG0, F)
    x[0, 0, 2, 2] = bits(0x80000001)[0]
    x[0, 0, 2:, 4:] = bits(0x80000001)[0]
    return x, bits(0, 0, 0, 0, 0, 0x80000001).reshape(1, 1, 2, 3)


IMAGES = {"pixel": pixel, "quantised": quantised}
RESAMPLE_DATA = {"quantised": quantised, "subnormal": subnormal, "islands": islands}

WARP_PLANES = [(2, 1, 37, 53), (1, 3, 9, 11), (1, 1, 2, 2), (1, 1, 3, 130)]
WARP_DEGENERATE = [(1, 1, 1, 7), (1, 1, 7, 1)]        # cx or cy = 0: pmctf_flow_warp_f32 refuses H < 2 or W < 2
FLOWS = ["normal", "integer", "half", "pzero", "nzero", "big", "inf", "nan"]


def flow(kind, n, H, W, seed=5):
    """(n, 2, H, W): normal (sigma 6); integer (exact grid hits: all four weights 0 or 1) and half-integer displacements;
    +0; -0; +-1e30; +-inf; NaN on half of the positions of either component"""
    r = _rng(seed, n, H, W, FLOWS.index(kind))
    shape = (n, 2, H, W)
    sgn = np.where(r.random(shape) < 0.5, F(-1), F(1))
    if kind == "normal":
        return (r.standard_normal(shape) * 6).astype(F)
    if kind == "integer":
        return np.rint(r.standard_normal(shape) * 3).astype(F)
    if kind == "half":
        return (np.rint(r.standard_normal(shape) * 3) + 0.5).astype(F)
    if kind == "pzero":
        return np.zeros(shape, F)
    if kind == "nzero":
        return np.full(shape, NEG0, F)
    if kind == "big":
        return (sgn * F(1e30)).astype(F)
    if kind == "inf":
        return (sgn * F(np.inf)).astype(F)
    if kind == "nan":
        f = (r.standard_normal(shape) * 2).astype(F)
        f[r.random(shape) < 0.5] = np.nan
        return f
    raise KeyError(kind)


def lin_tables(H, W):
    import torch
    return torch.linspace(-1.0, 1.0, W).numpy(), torch.linspace(-1.0, 1.0, H).numpy()


def warp_classes(fl, H, W):
    """numpy float32 restatement of flow_warp's coordinates (one rounding per written operation, fmax / fmin as the C
    functions: a NaN operand loses) -> the set of edge classes the field reaches"""
    lx, ly = lin_tables(H, W)
    out = set()
    with np.errstate(all="ignore"):
        for ax, comp, lin, size in (("x", fl[:, 0], lx.reshape(1, 1, W), W), ("y", fl[:, 1], ly.reshape(1, H, 1), H)):
            c, m = F(size - 1) / F(2), F(size - 1)
            raw = ((lin + comp / c) + F(1)) * c
            i = np.fmin(m, np.fmax(raw, F(0)))
            assert np.isfinite(i).all() and (i >= 0).all() and (i <= m).all()      # every position is inside the image
            w = i - np.floor(i)
            if (w == 0).any(): out.add("w==0")
            if (np.floor(i) + 1 > m).any(): out.add(ax + "1ok false")
            if (~(raw >= 0)).any(): out.add("clamp low")
            if (raw > m).any(): out.add("clamp high")
    return out


WARP_CLASSES = {"w==0", "x1ok false", "y1ok false", "clamp low", "clamp high"}

RESAMPLE_SHAPES = [(2, 3, 36, 60), (1, 2, 7, 9), (1, 1, 2, 2), (1, 1, 8, 8)]
UP_ONLY_SHAPES = [(1, 2, 1, 13), (1, 1, 7, 1)]

LSTM_SHAPES = [(2, 3, 30, 44, 1), (1, 32, 6, 10, 32)]


def lstm_data(shape, seed=6):
    """xh: the special set on a third of the elements, normals (sigma 3) elsewhere; cell: normals with +-0 and +-inf"""
    n, c, h, w, cc = shape
    r = _rng(seed, *shape)
    xh = (r.standard_normal((n, c, h, w)) * 3).astype(F)
    pick = r.random(xh.shape) < 1 / 3
    xh[pick] = SPECIALS[r.integers(0, SPECIALS.size, int(pick.sum()))]
    cell = r.standard_normal((n, cc, h, w)).astype(F)
    k = r.integers(0, 12, cell.shape)
    for v, val in enumerate((F(0), NEG0, F(np.inf), F(-np.inf))):
        cell[k == v] = val
    return xh, cell


def specials_plane(shape, seed=7):
    """every special pattern at least once (tiled), the rest ordinary values"""
    r = _rng(seed, *shape)
    x = r.standard_normal(shape).astype(F)
    flat = x.reshape(-1)
    idx = r.permutation(flat.size)[:min(flat.size, 4 * SPECIALS.size)]
    flat[idx] = np.resize(SPECIALS, idx.size)
    return x


# planes_to_u8: rint(clamp(x, 0, 255)) with ties to even; fmaxf(NaN, 0) is 0, so a NaN becomes 0 by the written clamp
U8_PATTERNS = [(np.nan, 0), (np.inf, 255), (-np.inf, 0), (0.5, 0), (1.5, 2), (254.5, 254), (255.5, 255), (-0.5, 0),
               (-0.0, 0), (0.0, 0), (2.5, 2), (1e-45, 0), (3.4028235e38, 255), (127.49999, 127), (127.5, 128)]


def bits_equal(got, want, what):
    """assert equal uint32 patterns; where both are NaN the payload is exempt (math_sweep.compare).  -> exempt count"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    g, w = got.reshape(-1).view(np.uint32), want.reshape(-1).view(np.uint32)
    count, first, exempt = ms.compare(g, w)
    assert count == 0, (f"{what}: {count} / {g.size} bit patterns differ; first at {np.unravel_index(first, got.shape)}: "
                        f"got {int(g[first]):#010x}, want {int(w[first]):#010x}")
    return exempt


def zero_signs(x):
    """(has +0, has -0)"""
    u = np.ascontiguousarray(x).view(np.uint32)
    return bool((u == 0).any()), bool((u == 0x80000000).any())
