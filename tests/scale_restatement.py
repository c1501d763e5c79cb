"""The integer picture resampling of DESIGN 5l restated in numpy and exact rationals, the yardstick of
tests/test_picture_scale_cpu.py and tests/test_gpu_picture_scale.py.  Written from the definition, not from pmctf_scale.py.

One axis, n_in -> n_out samples, phase offset `phase` (a rational):
    scale = n_in / n_out;  fs = max(scale, 1);  support = 2 fs
    output i:  c = scale (i + 1/2) + phase
               xmin = max(trunc(c - support + 1/2), 0);  xmax = min(trunc(c + support + 1/2), n_in)
               w_j = W((j - c + 1/2) / fs), j in [xmin, xmax), divided by their sum      (W: Catmull-Rom, a = -1/2)
               q_j = floor(16384 w_j + 1/2); the largest q_j (first of equals) absorbs 16384 - sum q
A plane of b-bit samples:  t = (sum q x + 32) >> 6 along x, then out = clamp((sum q t + 2^21) >> 22, 0, 2^b - 1) along y.
Nothing here touches torch or the product."""
import functools
from fractions import Fraction as Fr
from math import floor, trunc

import numpy as np

ONE = 16384


def W(x):
    x = abs(x)
    if x >= 2:
        return Fr(0)
    if x >= 1:
        return Fr(-1, 2) * x ** 3 + Fr(5, 2) * x ** 2 - 4 * x + 2
    return Fr(3, 2) * x ** 3 - Fr(5, 2) * x ** 2 + 1


def real_rows(n_in, n_out, phase=0):
    """-> [(xmin, [normalised real weights as Fractions])] per output sample"""
    scale = Fr(n_in, n_out)
    fs = scale if scale > 1 else Fr(1)
    support = 2 * fs
    out = []
    for i in range(n_out):
        c = scale * (Fr(i) + Fr(1, 2)) + Fr(phase)
        lo = max(trunc(c - support + Fr(1, 2)), 0)
        hi = min(trunc(c + support + Fr(1, 2)), n_in)
        w = [W((Fr(j) - c + Fr(1, 2)) / fs) for j in range(lo, hi)]
        total = sum(w, Fr(0))
        out.append((lo, [v / total for v in w]))
    return out


def int_rows(n_in, n_out, phase=0):
    """-> [(xmin, [integer coefficients summing to 16384])] per output sample"""
    out = []
    for lo, w in real_rows(n_in, n_out, phase):
        q = [floor(v * ONE + Fr(1, 2)) for v in w]
        best = 0
        for k in range(1, len(q)):
            if q[k] > q[best]:
                best = k
        q[best] += ONE - sum(q)
        out.append((lo, q))
    return out


def tables(n_in, n_out, phase=0):
    """-> (start int32 [n_out], coef int16 [n_out][T], T): rows zero-filled to the longest"""
    rows = int_rows(n_in, n_out, phase)
    T = max(len(q) for _, q in rows)
    start = np.array([lo for lo, _ in rows], np.int32)
    coef = np.zeros((n_out, T), np.int16)
    for i, (_, q) in enumerate(rows):
        coef[i, :len(q)] = q
    return start, coef, T


def left_phase(n_in, n_out):
    """horizontal chroma phase of MPEG-2 siting"""
    return Fr(n_in, n_out) / 4 - Fr(1, 4)


@functools.lru_cache(maxsize=None)
def _matrix(n_in, n_out, phase, integer=True):
    """the axis as a dense (n_out, n_in) matrix: int64 coefficients, or float64 real weights (kept per axis: read only)"""
    m = np.zeros((n_out, n_in), np.int64 if integer else np.float64)
    for i, (lo, q) in enumerate(int_rows(n_in, n_out, phase) if integer else real_rows(n_in, n_out, phase)):
        for k, v in enumerate(q):
            m[i, lo + k] = v if integer else float(v)
    return m


def resize_plane(x, h_out, w_out, b, phase_x=0, phase_y=0):
    """one plane of b-bit integers -> (h_out, w_out), same dtype: horizontal pass first, int64 throughout (the floor
    division of numpy's >> on negative int64 is the arithmetic shift)"""
    x = np.asarray(x)
    h_in, w_in = x.shape
    mx = _matrix(w_in, w_out, phase_x)
    my = _matrix(h_in, h_out, phase_y)
    t = (x.astype(np.int64) @ mx.T + 32) >> 6
    assert np.abs(t).max() < 2 ** 31, "the horizontal pass fits int32"
    o = (my @ t + (1 << 21)) >> 22
    return np.clip(o, 0, (1 << b) - 1).astype(x.dtype)


def resize_plane_real(x, h_out, w_out, phase_x=0, phase_y=0):
    """the same filter with its real weights, float64, unrounded: what torch's antialiased bicubic computes"""
    x = np.asarray(x, np.float64)
    h_in, w_in = x.shape
    return _matrix(h_in, h_out, phase_y, False) @ (x @ _matrix(w_in, w_out, phase_x, False).T)


def split(frame, h, w):
    """packed 4:2:0 picture -> (Y, Cb, Cr) views"""
    hc, wc = h // 2, w // 2
    return (frame[:h * w].reshape(h, w), frame[h * w:h * w + hc * wc].reshape(hc, wc), frame[h * w + hc * wc:].reshape(hc, wc))


def resize_yuv420(frame, h_in, w_in, h_out, w_out, b, chroma_loc="center"):
    """one packed planar 4:2:0 picture (1-D integer array of h_in*w_in*3/2 samples) -> the packed h_out x w_out picture"""
    assert chroma_loc in ("center", "left") and not (h_in | w_in | h_out | w_out) & 1
    frame = np.asarray(frame)
    assert frame.shape == (h_in * w_in * 3 // 2,)
    y, cb, cr = split(frame, h_in, w_in)
    px = left_phase(w_in // 2, w_out // 2) if chroma_loc == "left" else 0
    out = [resize_plane(y, h_out, w_out, b)] + [resize_plane(c, h_out // 2, w_out // 2, b, phase_x=px) for c in (cb, cr)]
    return np.concatenate([p.reshape(-1) for p in out])
