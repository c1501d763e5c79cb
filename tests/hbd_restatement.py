"""High-bit-depth picture I/O restated in numpy, the yardstick of tests/test_high_bitdepth_cpu.py and
tests/test_gpu_high_bitdepth.py.  With b the bit depth (9..16), s = b - 8 and max = 2^b - 1:

    in    x = float32(v) * 2^-s                       (exact: v has 16 bits, the factor is a power of two)
    out   v_hat = rint(clamp(x * 2^s, 0, max))        (ties to even, NaN -> 0; the product is exact or overflows to inf)
    sse   sum (v_hat - v)^2 per plane, in integers    (v = org * 2^s)
    psnr  10 log10(max^2 n / sse), float64; YUV-PSNR (6 Y + Cb + Cr) / 8

Nothing here touches torch or the product."""
import math

import numpy as np


def pad_size(h, w, psize):
    return -(-h // psize) * psize, -(-w // psize) * psize


def to_planes(frame_u16, h, w, b, psize):
    """one picture as it lies in the file (h*w*3/2 uint16 samples) -> (y_pad (1,1,Hp,Wp), c_pad (2,1,Hp/2,Wp/2),
    y_org (1,1,h,w), c_org (2,1,h/2,w/2)) float32, zero padded right and bottom"""
    frame_u16 = np.asarray(frame_u16)
    assert frame_u16.dtype == np.uint16 and frame_u16.shape == (h * w * 3 // 2,) and not (h | w | psize) & 1
    hc, wc = h // 2, w // 2
    Hp, Wp = pad_size(h, w, psize)
    down = np.float32(2.0 ** -(b - 8))
    y_org = (frame_u16[:h * w].astype(np.float32) * down).reshape(1, 1, h, w)
    c_org = (frame_u16[h * w:].astype(np.float32) * down).reshape(2, 1, hc, wc)
    y_pad = np.zeros((1, 1, Hp, Wp), np.float32)
    c_pad = np.zeros((2, 1, Hp // 2, Wp // 2), np.float32)
    y_pad[:, :, :h, :w] = y_org
    c_pad[:, :, :hc, :wc] = c_org
    return y_pad, c_pad, y_org, c_org


def to_u16(x, h, w, b):
    """padded float32 planes (N,1,Hp,Wp) -> (N,h,w) uint16"""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 4 and x.shape[1] == 1
    with np.errstate(over="ignore", invalid="ignore"):
        v = x[:, 0, :h, :w] * np.float32(2.0 ** (b - 8))
    v = np.where(np.isnan(v), np.float32(0.0), v)
    v = np.rint(np.clip(v, np.float32(0.0), np.float32((1 << b) - 1)))          # np.rint: ties to even
    return v.astype(np.uint16)


def sse(rec_y, rec_c, org_y, org_c, h, w, b):
    """(Y, Cb, Cr) sums of squared differences at b bits, Python integers (one term can be 65535^2 and a plane holds
    millions: int64 holds every sum here, Python integers hold any)"""
    rec = (to_u16(rec_y, h, w, b)[0], *to_u16(rec_c, h // 2, w // 2, b))
    up = np.float32(2.0 ** (b - 8))
    org = (np.asarray(org_y)[0, 0] * up, np.asarray(org_c)[0, 0] * up, np.asarray(org_c)[1, 0] * up)
    out = []
    for r, o in zip(rec, org):
        assert o.shape == r.shape and np.array_equal(o, np.rint(o)), "the originals are integers at b bits"
        d = r.astype(np.int64) - o.astype(np.int64)
        out.append(sum(int(v) for v in (d * d).sum(axis=1)))                   # row sums stay far below 2^63
    return tuple(out)


def psnr(sse_value, n, b):
    return math.inf if sse_value == 0 else 10.0 * math.log10(float((1 << b) - 1) ** 2 * n / sse_value)


def yuv_psnr(sse3, h, w, b):
    """-> {"y","cb","cr","yuv"} from the three sums of one h x w picture"""
    n = h * w
    q = {"y": psnr(sse3[0], n, b), "cb": psnr(sse3[1], n // 4, b), "cr": psnr(sse3[2], n // 4, b)}
    q["yuv"] = (6.0 * q["y"] + q["cb"] + q["cr"]) / 8.0
    return q


def synth_hbd(W, H, N, b, seed, low_bits=True):
    """[(Y, Cb, Cr)] uint16 arrays: pmctf_synth.synth_yuv420 shifted up to b bits, plus seeded low bits when asked (without
    them every sample is a multiple of 2^(b-8): the parity anchor's source)"""
    import pmctf_synth
    s = b - 8
    rng = np.random.default_rng(seed)
    out = []
    for planes in pmctf_synth.synth_yuv420(W, H, N, seed=seed):
        pic = []
        for p in planes:
            v = p.astype(np.uint16) << s
            if low_bits:
                v = v + rng.integers(0, 1 << s, p.shape, dtype=np.uint16)
            pic.append(v.astype(np.uint16))
        out.append(tuple(pic))
    return out


def flat(planes):
    """(Y, Cb, Cr) arrays -> the picture as one array in file order"""
    return np.concatenate([np.asarray(p).reshape(-1) for p in planes])
