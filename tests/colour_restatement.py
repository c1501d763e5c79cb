"""The colour arithmetic of DESIGN 5s restated in numpy int64, from the definition alone: the tests of pmctf_colour and of
csrc/picture_colour.hip are measured against this file, which imports nothing of the product.

A colour description is (matrix, range): matrix in MATRICES with exact rationals (Kr, Kb), Kg = 1 - Kr - Kb; range "full"
or "limited".  RGB is full range 0..M, M = 2^b - 1, at the depth b of the YCbCr picture.  Every coefficient is
round_half_even(c * 2^29) of its exact value, except the forward G column, which is set so that each row's integer sum is
exact (the Y row sums to round_half_even(sY / M * 2^29), the chroma rows to 0).
out = clamp((k0 x0 + k1 x1 + k2 x2 + (o << 29) + (1 << 28)) >> 29, 0, M)."""
import functools
from fractions import Fraction

import numpy as np

F = 29
MATRICES = {"bt601": (Fraction(299, 1000), Fraction(114, 1000)), "bt709": (Fraction(2126, 10000), Fraction(722, 10000)),
            "bt2020": (Fraction(2627, 10000), Fraction(593, 10000))}
RANGES = ("full", "limited")
# name -> (depth, kind, component order or plane order)
LAYOUTS = {"rgb24": (8, "packed", "rgb"), "bgr24": (8, "packed", "bgr"), "rgba": (8, "packed", "rgba"),
           "bgra": (8, "packed", "bgra"), "rgb48": (16, "packed", "rgb"), "gbrp": (8, "planar", "gbr"),
           "gbrp10": (10, "planar", "gbr"), "gbrp12": (12, "planar", "gbr"), "gbrp16": (16, "planar", "gbr")}


def scales(rng, b):
    """-> (sY, sC, oY, oC)"""
    M = (1 << b) - 1
    if rng == "full":
        return M, M, 0, 1 << (b - 1)
    return 219 << (b - 8), 224 << (b - 8), 16 << (b - 8), 1 << (b - 1)


def exact_rows(matrix, rng, b):
    """-> (forward rows, inverse rows) as Fractions"""
    kr, kb = MATRICES[matrix]
    kg = 1 - kr - kb
    M = (1 << b) - 1
    sy, sc, _, _ = scales(rng, b)
    fy = Fraction(sy, M)
    fcb, fcr = Fraction(sc) / (2 * (1 - kb) * M), Fraction(sc) / (2 * (1 - kr) * M)
    fwd = [[fy * kr, fy * kg, fy * kb], [fcb * -kr, fcb * -kg, fcb * (1 - kb)], [fcr * (1 - kr), fcr * -kg, fcr * -kb]]
    a, cb, cr = Fraction(M, sy), 2 * (1 - kb) * M / Fraction(sc), 2 * (1 - kr) * M / Fraction(sc)
    inv = [[a, Fraction(0), cr], [a, -kb / kg * cb, -kr / kg * cr], [a, cb, Fraction(0)]]
    return fwd, inv


def rhe(x):
    return round(Fraction(x))                            # Python rounds a Fraction half to even


@functools.lru_cache(maxsize=None)
def tables(matrix, rng, b):
    """-> (forward 3x3, inverse 3x3, (oY, oC, oC)) as Python ints; the rational arithmetic is done once per case"""
    fwd, inv = exact_rows(matrix, rng, b)
    sy, _, oy, oc = scales(rng, b)
    kf = [[rhe(c * 2 ** F) for c in row] for row in fwd]
    sums = [rhe(Fraction(sy, (1 << b) - 1) * 2 ** F), 0, 0]
    for row, s in zip(kf, sums):
        row[1] = s - row[0] - row[2]
    ki = [[rhe(c * 2 ** F) for c in row] for row in inv]
    return kf, ki, (oy, oc, oc)


def _rows(k, x, o, top):
    x = [np.asarray(v, np.int64) for v in x]
    out = []
    for r in range(3):
        acc = k[r][0] * x[0] + k[r][1] * x[1] + k[r][2] * x[2] + (np.int64(o[r]) << F) + (np.int64(1) << (F - 1))
        out.append(np.clip(acc >> F, 0, top))
    return out


def forward(r, g, b, matrix, rng, depth):
    """R, G, B integer arrays -> (Y, Cb, Cr) int64 arrays; inputs are masked to `depth` bits"""
    kf, _, o = tables(matrix, rng, depth)
    top = (1 << depth) - 1
    return _rows(kf, [np.asarray(v, np.int64) & top for v in (r, g, b)], o, top)


def inverse(y, cb, cr, matrix, rng, depth):
    """Y, Cb, Cr integer arrays -> (R, G, B) int64 arrays"""
    _, ki, o = tables(matrix, rng, depth)
    top = (1 << depth) - 1
    return _rows(ki, [(np.asarray(v, np.int64) & top) - off for v, off in zip((y, cb, cr), o)], (0, 0, 0), top)


def exact_forward(rgb, matrix, rng, depth):
    """one (R, G, B) triple -> the exact rational (Y, Cb, Cr), clamped to 0..M"""
    fwd, _ = exact_rows(matrix, rng, depth)
    _, _, oy, oc = scales(rng, depth)
    top = (1 << depth) - 1
    return [min(max(sum(c * v for c, v in zip(row, rgb)) + o, 0), top) for row, o in zip(fwd, (oy, oc, oc))]


def exact_inverse(ycc, matrix, rng, depth):
    _, inv = exact_rows(matrix, rng, depth)
    _, _, oy, oc = scales(rng, depth)
    top = (1 << depth) - 1
    x = [ycc[0] - oy, ycc[1] - oc, ycc[2] - oc]
    return [min(max(sum(c * v for c, v in zip(row, x)), 0), top) for row in inv]


# ------------------------------------------------------------------------------------------------------------- layouts
def dtype(layout):
    return np.uint8 if LAYOUTS[layout][0] == 8 else np.dtype("<u2")


def frame_bytes(layout, h, w):
    depth, _, order = LAYOUTS[layout]
    return h * w * len(order) * (1 if depth == 8 else 2)


def unpack_rgb(surface, layout, h, w):
    """the bytes of a surface (uint8 array) -> (R, G, B) flat int64 arrays of h * w, as stored (not masked)"""
    _, kind, order = LAYOUTS[layout]
    data = np.frombuffer(np.ascontiguousarray(surface, np.uint8)[:frame_bytes(layout, h, w)].tobytes(), dtype(layout))
    data = data.astype(np.int64)
    comps = data.reshape(h * w, len(order)).T if kind == "packed" else data.reshape(len(order), h * w)
    return tuple(comps[order.index(c)] for c in "rgb")


def pack_rgb(r, g, b, layout, h, w):
    """(R, G, B) -> the bytes of the surface (uint8 array); alpha is 255"""
    _, kind, order = LAYOUTS[layout]
    src = {"r": r, "g": g, "b": b, "a": np.full(h * w, 255)}
    comps = np.stack([np.asarray(src[c]).reshape(-1) for c in order])
    flat = (comps.T if kind == "packed" else comps).astype(dtype(layout)).reshape(-1)
    return np.frombuffer(flat.tobytes(), np.uint8).copy()


def rgb_to_planar(surface, layout, h, w, matrix, rng):
    """a surface's bytes -> the packed planar 4:4:4 picture (Y, Cb, Cr planes) in the layout's sample type"""
    depth = LAYOUTS[layout][0]
    y, cb, cr = forward(*unpack_rgb(surface, layout, h, w), matrix, rng, depth)
    return np.concatenate([y, cb, cr]).astype(np.uint8 if depth == 8 else np.uint16)


def planar_to_rgb(frame, layout, h, w, matrix, rng):
    """a packed planar 4:4:4 picture -> the surface's bytes"""
    depth = LAYOUTS[layout][0]
    n = h * w
    frame = np.asarray(frame).reshape(-1)
    r, g, b = inverse(frame[:n], frame[n:2 * n], frame[2 * n:3 * n], matrix, rng, depth)
    return pack_rgb(r, g, b, layout, h, w)
