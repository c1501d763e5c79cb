"""The sequence-structure pre-analysis restated in numpy integers, the yardstick of tests/test_sequence_structure_cpu.py and
tests/test_gpu_sequence_structure.py.  With b the bit depth (8..16) and s = b - 8, per luma original x (float32, v * 2^-s):

    u        = rint(clamp(x * 2^s, 0, 65535))          (an integer; NaN -> 0)
    hist[k]  = number of samples with min(u >> s, 255) == k
    sad      = sum |u_cur - u_prev|
    hist_l1  = sum_k |hist_cur[k] - hist_prev[k]|
    mad      = sad / (h w 2^s)                          (8-bit units)
    hd       = hist_l1 / (2 h w)                        (0..1)

Nothing here touches torch or the product."""
import numpy as np


def luma_u(x, b):
    """float32 luma plane -> int64 samples at b bits"""
    x = np.asarray(x)
    assert x.dtype == np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        v = x * np.float32(2.0 ** (b - 8))
    v = np.where(np.isnan(v), np.float32(0.0), v)
    return np.rint(np.clip(v, np.float32(0.0), np.float32(65535.0))).astype(np.int64)


def activity(cur, prev, b):
    """-> (hist: 256 Python ints, sad: Python int, or None without a prev)"""
    u = luma_u(cur, b)
    bins = np.minimum(u >> (b - 8), 255).reshape(-1)
    hist = [int(v) for v in np.bincount(bins, minlength=256)]
    if prev is None:
        return hist, None
    d = np.abs(u - luma_u(prev, b))
    return hist, sum(int(v) for v in d.reshape(d.shape[-2], -1).sum(axis=1))


def figures(lumas, b):
    """what pmctf_seq.sequence_activity returns, for a list of float32 luma planes of one size"""
    out = {"sad": [None], "hist_l1": [None], "mad": [None], "hd": [None]}
    h, w = lumas[0].shape[-2:]
    prev_hist = activity(lumas[0], None, b)[0]
    for t in range(1, len(lumas)):
        hist, sad = activity(lumas[t], lumas[t - 1], b)
        l1 = sum(abs(a - c) for a, c in zip(hist, prev_hist))
        out["sad"].append(sad)
        out["hist_l1"].append(l1)
        out["mad"].append(sad / (h * w * 2 ** (b - 8)))
        out["hd"].append(l1 / (2 * h * w))
        prev_hist = hist
    return out


CUT_W, CUT_H, CUT_AT = 132, 100, 6


def cut_sequence():
    """[(Y, Cb, Cr)] uint8: six pictures of synth_yuv420(132, 100, 6, seed=1234), then six of seed 77 with the luma
    (y >> 1) + 8: a scene change at picture 6"""
    import pmctf_synth
    a = pmctf_synth.synth_yuv420(CUT_W, CUT_H, CUT_AT, seed=1234)
    b = [((y >> 1) + 8, u, v) for y, u, v in pmctf_synth.synth_yuv420(CUT_W, CUT_H, CUT_AT, seed=77)]
    return a + [tuple(p.astype(np.uint8) for p in pic) for pic in b]


def cut_figures():
    return figures([pic[0].astype(np.float32) for pic in cut_sequence()], 8)
