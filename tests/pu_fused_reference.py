"""Cases and reference of test_gpu_pu_fused.py (no GPU import): the fused PredictUpdate kernel (csrc/pu_fused.hip)
against the oracle's C primitives composed in the kernel's written order — not through the engine, which gives it one
synthetic weight set and whichever (rule, skip_rule) pair follows from the plane size.  Four seeded random layers
1 -> 16 -> 16 -> 16 -> 1 at two weight scales (0.1, and 8: most tanh values saturate), every (rule, skip_rule) pair,
mode 0 with two scale factors, mode 1 with both signs and a non-zero lifting bias, on planes of H = 2, exactly one 8x32
tile, one row and one column past a tile, whole tiles on three planes, and 37x53.

Shares of the 37x53 elements in which two references differ (measured on the oracle alone, asserted >= 0.5 in
test_pu_fused_reference_cpu.py):
  mode 0, rule chain vs blocks:                 scale 0.1: 0.73 - 0.75     scale 8: 0.96
  mode 1, the six pairs of (rule, skip_rule):   scale 0.1: 0.56 - 0.68     scale 8: 0.94 - 0.97
  saturated tanh values at scale 8:             mode 0: 0.92     mode 1: 0.69
with x = normal * 0.1 (scale 0.1) or * 4 (scale 8) in mode 0, x = normal * 50 and a lifting bias of 37.7 in mode 1,
`other` = normal.  What did NOT meet the bound: mode 0 at scale 0.1 with x = normal * 1 and more (0.09 - 0.34: x swamps
the last bit of pu * 0.1, so a larger input hides the rule), and mode 1 with a lifting bias of 0.3125 (skip_rule pairs
0.02 - 0.39: next to |x| ~ 50 the bias falls below the rounding of the three products, whichever rule adds it)."""
import functools

import numpy as np

SHAPES = [(1, 2, 1), (1, 8, 32), (2, 9, 33), (3, 16, 64), (1, 37, 53)]
SCALES = {"w0.1": 0.1, "saturating": 8.0}
RULES = [(0, 0), (0, 1), (1, 0), (1, 1)]          # (rule of the four layers, rule of the 3x1 lifting filter)
MODE0_C = (1.0, 0.7071067)
MODE0_AMPLITUDE = {0.1: 0.1, 8.0: 4.0}          # of x in mode 0, per weight scale
F = np.float32


@functools.lru_cache(maxsize=None)
def weights(scale):
    """((w1, b1), (w2, b2), (w3, b3), (w4, b4)) OIHW float32, and the lifting filter (w0, w1, w2, bias)"""
    g = np.random.default_rng(int(scale * 1000) + 7)
    layers = tuple(((g.standard_normal((co, ci, 3, 3), dtype=F) * F(scale)).astype(F), (g.standard_normal(co, dtype=F) * F(scale)).astype(F))
                   for ci, co in ((1, 16), (16, 16), (16, 16), (16, 1)))
    lift = g.standard_normal(3, dtype=F)
    return layers, (float(lift[0]), float(lift[1]), float(lift[2]), float(F(37.7)))


@functools.lru_cache(maxsize=None)
def inputs(shape, scale):
    """(x for mode 0, x for mode 1, other), each (N, 1, H, W) normal times the amplitudes of the module docstring"""
    N, H, W = shape
    g = np.random.default_rng(N * 10000 + H * 100 + W)
    return tuple((g.standard_normal((N, 1, H, W), dtype=F) * F(a)).astype(F) for a in (MODE0_AMPLITUDE[scale], 50.0, 1.0))


def pu_reference(x, layers, rule):
    """(PredictUpdate(x), share of the two tanh layers' values that are exactly +-1) from the oracle's convolution and tanh"""
    from pmctf_oracle import clib
    (w1, b1), (w2, b2), (w3, b3), (w4, b4) = layers
    c1 = clib.conv2d(x, w1, b1, 1, (1, 1), rule)
    t1 = clib.tanh(c1)
    t = clib.conv2d(t1, w2, b2, 1, (1, 1), rule)
    t2 = clib.tanh(t)
    t = clib.conv2d(t2, w3, b3, 1, (1, 1), rule) + c1
    saturated = float(np.mean(np.abs(np.concatenate([t1.ravel(), t2.ravel()])) == 1))
    return clib.conv2d(t, w4, b4, 1, (1, 1), rule), saturated


@functools.lru_cache(maxsize=None)
def reference(shape, scale, rule, skip_rule, mode):
    """mode 0: {c: out};  mode 1: {sign: out}.  float32 steps in the kernel's order.  Plus the saturated share."""
    layers, lift = weights(scale)
    return compose(inputs(shape, scale), layers, lift, rule, skip_rule, mode)


def compose(data, layers, lift, rule, skip_rule, mode):
    from pmctf_oracle import clib
    x0, x1, other = data
    if mode == 0:
        pu, sat = pu_reference(x0, layers, rule)
        return {c: (x0 + pu * F(0.1)) * F(c) for c in MODE0_C}, sat
    xp = np.pad(x1, ((0, 0), (0, 0), (1, 1), (0, 0)), mode="reflect")
    skip = clib.conv2d(xp, np.array(lift[:3], F).reshape(1, 1, 3, 1), np.array([lift[3]], F), 1, (0, 0), skip_rule)
    pu, sat = pu_reference(skip / F(256), layers, rule)
    br = skip + (pu * F(256)) * F(0.1)
    return {1.0: other + br, -1.0: other - br}, sat


# ---- zeros of both signs ---------------------------------------------------------------------------------------------------
# The kernel masks every layer's halo to 0 by hand and starts its chains at `rule ? 0.0f : bias`: the data on which a masked
# slot, a skipped tap or a chain started at the wrong zero shows is the zero data of the two convolution censuses
# (valu_conv_census.case_data(..., data="zeros")): column patches of -0, +0, -2^-149 and ordinary values, every weight in
# [0.25, 0.375), every bias -0 — the lifting filter's too.  With them a -0 patch stays -0 through all four layers, both
# tanh, the residual add and the lifting arithmetic, except where a zero of a halo is multiplied in.  `other` has the same
# patches, so that other +- branch keeps the sign.  "today": the same inputs under the weights and biases of weights(0.1).
ZERO_SHAPES = [(2, 9, 33), (1, 37, 53)]
ZERO_BIASES = ["neg0", "today"]


def _zero_plane(shape, seed):
    import valu_conv_census as vc
    N, H, W = shape
    # patches as for a 9x9 filter (10 columns each): four 3x3 layers in a row reach four columns into a patch from either side
    return vc.case_data((seed, "dense", (N, 1, H, W, 1, 9, 9, 1, 4, 4), 0, 0, 0.0, 0, True, None, None, {"data": "zeros"}))["x"]


@functools.lru_cache(maxsize=None)
def zero_inputs(shape):
    """(x for mode 0, x for mode 1, other): three planes of the zero data"""
    return tuple(_zero_plane(shape, f"pu_fused_{k}_{shape}") for k in ("x0", "x1", "other"))


@functools.lru_cache(maxsize=None)
def zero_weights(biases):
    if biases == "today":
        return weights(0.1)
    g = np.random.default_rng(5)
    neg0 = lambda n: np.full(n, -0.0, F)
    layers = tuple(((F(0.25) + g.random((co, ci, 3, 3), dtype=F) * F(0.125)).astype(F), neg0(co))
                   for ci, co in ((1, 16), (16, 16), (16, 16), (16, 1)))
    lift = (F(0.25) + g.random(3, dtype=F) * F(0.125)).astype(F)
    return layers, (float(lift[0]), float(lift[1]), float(lift[2]), -0.0)


@functools.lru_cache(maxsize=None)
def zero_reference(shape, biases, rule, skip_rule, mode):
    layers, lift = zero_weights(biases)
    return compose(zero_inputs(shape), layers, lift, rule, skip_rule, mode)[0]
