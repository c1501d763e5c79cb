"""Yardsticks of the per-plane quality tests, in plain numpy and torch on the CPU: per-plane squared-error sums
in int64, per-plane MS-SSIM by the restatement of tests/quality_restatement.py with one channel at the data range
2^b - 1 (that function takes both already; it is imported and left alone), PSNR in float64, and the test pictures."""
import math

import numpy as np
import torch

import quality_restatement as qr

SUBSAMPLING = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}            # format -> (sx, sy)
FLOOR = 16 * 2.0 ** -24                                                # the rule of DESIGN 5e
SSE_SIZES = ((6, 10), (18, 34), (100, 132))                            # (h, w)
MSSSIM_SIZES = ((162, 170), (161, 323), (192, 256))                    # planes, (h, w)
DEPTHS = (8, 10, 16)
NOISE = (0.002, 0.02, 0.1)                                             # standard deviation as a fraction of the data range


def plane_shapes(h, w, fmt):
    sx, sy = SUBSAMPLING[fmt]
    return (h, w), (h // sy, w // sx), (h // sy, w // sx)


def frame_samples(h, w, fmt):
    return sum(a * b for a, b in plane_shapes(h, w, fmt))


def split(frame, h, w, fmt):
    """a packed picture (flat integer array) -> its three planes"""
    out, at = [], 0
    for a, b in plane_shapes(h, w, fmt):
        out.append(np.asarray(frame[at:at + a * b]).reshape(a, b))
        at += a * b
    assert at == len(frame)
    return out


def sse(frame_a, frame_b, h, w, fmt):
    """(Y, Cb, Cr) sums of squared differences in int64, as Python ints"""
    out = []
    for p, q in zip(split(frame_a, h, w, fmt), split(frame_b, h, w, fmt)):
        d = p.astype(np.int64) - q.astype(np.int64)
        out.append(int((d * d).sum()))
    return tuple(out)


def psnr(err, n, bitdepth):
    return math.inf if err == 0 else 10.0 * math.log10(float((1 << bitdepth) - 1) ** 2 * n / err)


def yuv(y, cb, cr):
    return (6.0 * y + cb + cr) / 8.0


def ms_ssim(plane_a, plane_b, bitdepth, dtype=torch.float64, scale=1.0):
    """one plane against another -> (MS-SSIM, means [5] of (cs, ssim)); scale multiplies both planes and the data range
    (the invariance the kernels rest on)"""
    a = torch.from_numpy(np.asarray(plane_a).astype(np.float64)) * scale
    b = torch.from_numpy(np.asarray(plane_b).astype(np.float64)) * scale
    v, means = qr.ms_ssim(a[None], b[None], dtype, data_range=float((1 << bitdepth) - 1) * scale)
    return v, [m[0] for m in means]


def bound(v64, v32):
    """|hip - r64| <= max(2 |r32 - r64|, 16 * 2^-24)"""
    return max(2.0 * abs(v32 - v64), FLOOR)


def random_frame(h, w, fmt, bitdepth, seed):
    """a packed picture of uniform samples over the whole range, 0 and 2^b - 1 included"""
    r = np.random.default_rng(seed)
    f = r.integers(0, 1 << bitdepth, frame_samples(h, w, fmt)).astype(np.uint8 if bitdepth == 8 else np.uint16)
    f[0], f[-1] = 0, (1 << bitdepth) - 1
    return f


def plane_pair(h, w, bitdepth, sigma, seed=0):
    """One plane and a distorted copy, integer arrays of the depth's type: a smooth pattern with a fine texture over nearly
    the whole range, the copy with N(0, sigma * range) noise added, rounded and clamped to the range (the clamp is live at
    the strongest noise)."""
    top = float((1 << bitdepth) - 1)
    r = np.random.default_rng(1000 * seed + 7 * h + w + bitdepth)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 0.5 + 0.4 * np.sin(xx / 17.0 + yy / 29.0) * np.cos(yy / 13.0 - xx / 41.0) + 0.08 * (r.random((h, w)) - 0.5)
    a = np.rint(np.clip(base, 0.0, 1.0) * top)
    b = np.clip(np.rint(a + sigma * top * r.standard_normal((h, w))), 0.0, top)
    dt = np.uint8 if bitdepth == 8 else np.uint16
    return a.astype(dt), b.astype(dt)


def synth_frames(h, w, fmt, bitdepth, n, seed=0):
    """n packed pictures of a slowly moving smooth pattern with a fine texture, every plane over most of the range"""
    top = float((1 << bitdepth) - 1)
    r = np.random.default_rng(seed)
    dt = np.uint8 if bitdepth == 8 else np.uint16
    texture = [0.06 * (r.random(s) - 0.5) for s in plane_shapes(h, w, fmt)]
    out = []
    for k in range(n):
        planes = []
        for p, (rows, cols) in enumerate(plane_shapes(h, w, fmt)):
            yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
            yy, xx = yy * (h / rows), xx * (w / cols) + 1.5 * k
            v = 0.5 + (0.38 - 0.1 * p) * np.sin(xx / (15.0 + 4 * p) + yy / 27.0) * np.cos(yy / (11.0 + 3 * p) - xx / 37.0)
            planes.append(np.rint(np.clip(v + texture[p], 0.0, 1.0) * top).astype(dt).reshape(-1))
        out.append(np.concatenate(planes))
    return out
