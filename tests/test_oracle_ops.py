"""The oracle's non-convolution primitives (oracle/c/pm_ops.c) against the torch CPU operations they restate, as bit
patterns, on the edge data of edge_values.py: zeros of both signs, subnormals, infinities, NaNs, flow fields that land on the
grid, between grid points, outside the image and nowhere.  The HIP kernels are line-for-line twins of these primitives
(test_gpu_edge_values.py holds them to the primitives); this file is what ties the pair to the real operation.

Where ATen takes another evaluation order than the one PM-F32 writes down (bilinear resampling of small
planes, bilinear downsampling of subnormals) nothing is asserted equal: the measured counts are recorded below, and a
machine whose ATen gives other counts skips with that reason, as test_math_sweep_cpu.py does for libm."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import edge_values as ev
import math_sweep as ms

ATEN_THREADS = 4            # ATen's resampling kernels pick their path by plane size AND intra-op thread count


@pytest.fixture(autouse=True)
def _aten_threads():
    old = torch.get_num_threads()
    torch.set_num_threads(ATEN_THREADS)
    yield
    torch.set_num_threads(old)


def _normal(shape, seed=8):
    return (np.random.default_rng([seed, *shape]).standard_normal(shape) * 10).astype(np.float32)


DATA = dict(ev.RESAMPLE_DATA, normal=_normal)


def _count(got, want):
    return ms.compare(np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1))[0]


def _interp(x, scale):
    return F.interpolate(torch.from_numpy(x), scale_factor=scale, mode="bilinear", align_corners=False).numpy()


@pytest.mark.parametrize("shape", ev.WARP_PLANES + ev.WARP_DEGENERATE, ids=lambda s: "x".join(map(str, s)))
def test_flow_warp_is_grid_sample(shape):
    """pm_flow_warp against F.grid_sample(bilinear, border, align_corners=True) of the grid the reference builds
    (TorchK.flow_warp): both images, every flow kind, one flow field shared and one per plane.  Non-finite positions clamp
    into the image on both sides (ATen orders its clamp so that a NaN becomes 0); a 1-row or 1-column plane divides by 0."""
    from pmctf_oracle import clib
    from pmctf_oracle.kernels import TorchK
    N, _, H, W = shape
    lx, ly = ev.lin_tables(H, W)
    signs = [False, False]
    for iname, image in ev.IMAGES.items():
        im = image(shape)
        for kind in ev.FLOWS:
            for fn in sorted({1, N}):
                fl = ev.flow(kind, fn, H, W)
                ref = clib.flow_warp(im, fl, lx, ly)
                with np.errstate(all="ignore"):
                    want = TorchK().flow_warp(torch.from_numpy(im), torch.from_numpy(fl).expand(N, -1, -1, -1)).numpy()
                ev.bits_equal(ref, want, f"flow_warp {shape} {iname} image, {kind} flow, {fn} field(s)")
                signs = [a or b for a, b in zip(signs, ev.zero_signs(ref))]
    assert all(signs) or min(H, W) < 7, "no output zero of one sign"       # the -0 block needs a 7x7 plane


def test_avgpool2_never_gives_minus_zero():
    """F.avg_pool2d adds the four inputs to an accumulator that starts at +0, and adds the quotient to an output it has set
    to +0: a window of four -0 gives +0, a window that mixes the signs gives +0, a negative sum whose quarter underflows
    gives +0, and nothing else moves.  (The sum once started at a00 and the quotient was stored: 0x80000000 in the first
    and the last case.)"""
    from pmctf_oracle import clib
    x = ev.quantised((2, 3, 36, 60))
    assert (x[..., 0:2, 0:2].view(np.uint32) == 0x80000000).all()
    assert sorted(x[0, 0, 0:2, 2:4].view(np.uint32).reshape(-1).tolist()) == [0, 0, 0x80000000, 0x80000000]
    got = clib.avgpool2(x)
    assert (got[..., 0, 0].view(np.uint32) == 0).all() and (got[..., 0, 1].view(np.uint32) == 0).all()
    ev.bits_equal(got, F.avg_pool2d(torch.from_numpy(x), 2, 2).numpy(), "avgpool2 on the quantised plane")
    neg, want = ev.minus_zero_windows()
    got = clib.avgpool2(neg)
    ev.bits_equal(got, F.avg_pool2d(torch.from_numpy(neg), 2, 2).numpy(), "avgpool2 on -0")
    ev.bits_equal(got, want, "avgpool2 on -0")


@pytest.mark.parametrize("shape", ev.RESAMPLE_SHAPES + [(1, 1, 40, 60)], ids=lambda s: "x".join(map(str, s)))
def test_avgpool2_is_avg_pool2d(shape):
    from pmctf_oracle import clib
    for name, data in DATA.items():
        x = data(shape)
        ev.bits_equal(clib.avgpool2(x), F.avg_pool2d(torch.from_numpy(x), 2, 2).numpy(), f"avgpool2 {shape} {name}")


@pytest.mark.parametrize("shape", ev.RESAMPLE_SHAPES + ev.UP_ONLY_SHAPES + [(1, 2, 40, 72), (1, 1, 200, 300)],
                         ids=lambda s: "x".join(map(str, s)))
def test_bilinear_on_quantised_planes_is_interpolate(shape):
    """on integer-valued planes (what the kernels read in production next to pixels) every product with a weight k/16 is
    exact, so that ATen's evaluation orders coincide: identical at every size and factor, odd sizes and 1-wide planes
    included, zeros of both signs among the results"""
    from pmctf_oracle import clib
    x = ev.quantised(shape)
    for f in (2, 4, 8):
        ev.bits_equal(clib.bilinear_up(x, f), _interp(x, f), f"bilinear_up x{f} {shape}")
        if shape[2] >= f and shape[3] >= f:
            ev.bits_equal(clib.bilinear_down(x, f), _interp(x, 1 / f), f"bilinear_down /{f} {shape}")


# planes on which ATen's vectorised path runs with ATEN_THREADS threads: the order pm_ops.c writes down
LARGE = [("up", 2, (1, 2, 40, 72)), ("up", 4, (1, 2, 40, 72)), ("up", 8, (1, 2, 40, 72)), ("up", 2, (2, 3, 36, 60)),
         ("down", 2, (1, 1, 200, 300)), ("down", 4, (1, 1, 256, 512)), ("down", 8, (1, 1, 1024, 1024))]


def _interpolate_is_the_recorded_one():
    """ATen's resampling paths depend on the CPU: is this machine's F.interpolate the one whose small-plane deviations are
    recorded below (one probe per direction)?"""
    from pmctf_oracle import clib
    for key in (("up", 2, (1, 1, 8, 8), "normal"), ("down", 2, (1, 2, 40, 72), "normal")):
        way, f, shape, name = key
        x = DATA[name](shape)
        got = clib.bilinear_up(x, f) if way == "up" else clib.bilinear_down(x, f)
        if _count(got, _interp(x, f if way == "up" else 1 / f)) != RECORDED[key]:
            return False
    return True


@pytest.mark.parametrize("case", LARGE, ids=lambda c: f"{c[0]}{c[1]}-" + "x".join(map(str, c[2])))
def test_bilinear_on_large_planes_is_interpolate(case):
    """ordinary values and +-inf / NaN islands; upsampling also on subnormals.  On a machine whose F.interpolate is not the
    recorded one (another evaluation path on its CPU) a difference skips with that reason instead of failing."""
    from pmctf_oracle import clib
    way, f, shape = case
    for name in ("normal", "islands") + (("subnormal",) if way == "up" else ()):
        x = DATA[name](shape)
        got = clib.bilinear_up(x, f) if way == "up" else clib.bilinear_down(x, f)
        want = _interp(x, f if way == "up" else 1 / f)
        if _count(got, want) and not _interpolate_is_the_recorded_one():
            pytest.skip("this machine's F.interpolate is not the recorded one (its small-plane deviations differ from RECORDED): "
                        "another evaluation path of ATen on this CPU")
        ev.bits_equal(got, want, f"bilinear_{way} by {f} {shape} {name}")


# Known deviations, measured with torch 2.x CPU on x86-64 (AVX2), 4 intra-op threads: elements whose bit pattern differs
# from F.interpolate's.  All are differences of the last bit (or of a subnormal's last bits), none on quantised planes.
# (way, factor, plane, data): count
RECORDED = {
    ("up", 2, (1, 1, 8, 8), "normal"): 111, ("up", 4, (1, 1, 8, 8), "normal"): 459, ("up", 8, (1, 1, 8, 8), "normal"): 1863,
    ("up", 2, (1, 2, 7, 9), "normal"): 216, ("up", 4, (1, 2, 7, 9), "normal"): 936, ("up", 8, (1, 2, 7, 9), "normal"): 3647,
    ("up", 2, (1, 2, 1, 13), "normal"): 22, ("up", 2, (1, 1, 7, 1), "normal"): 5, ("up", 2, (1, 1, 2, 2), "normal"): 3,
    ("down", 2, (1, 2, 40, 72), "normal"): 422, ("down", 4, (1, 2, 40, 72), "normal"): 116,
    ("down", 8, (1, 2, 40, 72), "normal"): 22, ("down", 2, (2, 3, 36, 60), "normal"): 961,
    ("down", 4, (1, 1, 200, 300), "normal"): 1146, ("down", 8, (1, 1, 200, 300), "normal"): 262,
    ("down", 8, (1, 1, 512, 512), "normal"): 1227,
    # subnormal inputs: a * 0.5 rounds, and ATen's order differs from the written one at every plane size
    ("down", 2, (1, 1, 200, 300), "subnormal"): 1716, ("down", 2, (1, 1, 1024, 1024), "subnormal"): 31114,
}


@pytest.mark.parametrize("key", list(RECORDED), ids=lambda k: f"{k[0]}{k[1]}-" + "x".join(map(str, k[2])) + f"-{k[3]}")
def test_recorded_deviations_from_interpolate(key):
    """the deviations DESIGN.md section 2 lists are the ones this machine's ATen shows; a machine on which ATen evaluates these
    planes in another order (its paths depend on the CPU) skips"""
    from pmctf_oracle import clib
    way, f, shape, name = key
    x = DATA[name](shape)
    got = clib.bilinear_up(x, f) if way == "up" else clib.bilinear_down(x, f)
    want = _interp(x, f if way == "up" else 1 / f)
    count = _count(got, want)
    if count != RECORDED[key]:
        pytest.skip(f"this machine's ATen differs from the oracle on {count} elements here, {RECORDED[key]} are recorded: "
                    "another evaluation path of F.interpolate")
    # Either order is a convex combination of at most four inputs with at most four roundings, each of at most half a unit
    # of the last place of the largest input (or 2^-150 among subnormals): the two differ by at most four such units.
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    unit = max(float(np.abs(x).max()) * 2.0 ** -23, 2.0 ** -149)
    assert d.max() <= 4 * unit, f"a recorded deviation of {d.max() / unit:.2f} units of the last place of the largest input"


@pytest.mark.parametrize("shape", [(1, 8, 9, 11), (2, 64, 37, 51), (1, 6, 19, 23)], ids=lambda s: "x".join(map(str, s)))
def test_dwconv_is_grouped_conv2d(shape):
    """pm_dwconv2d (3x3, padded taps skipped) against F.conv2d(groups=C) on zero-rich and ordinary planes, bias -0 on the
    zero-rich one"""
    from pmctf_oracle import clib
    n, c, h, w = shape
    r = np.random.default_rng([9, *shape])
    wt = (r.random((c, 1, 3, 3), dtype=np.float32) * np.float32(0.125) + np.float32(0.25)).astype(np.float32)
    for name, x, b in (("quantised", ev.quantised(shape), np.full(c, ev.NEG0, np.float32)),
                       ("normal", _normal(shape), r.standard_normal(c).astype(np.float32))):
        ref = clib.dwconv2d(x, wt, b)
        want = F.conv2d(torch.from_numpy(x), torch.from_numpy(wt), torch.from_numpy(b), padding=1, groups=c).numpy()
        ev.bits_equal(ref, want, f"dwconv {shape} {name}")
        if name == "quantised":
            assert all(ev.zero_signs(ref))


@pytest.mark.parametrize("shape", [(2, 1, 36, 60), (1, 1, 200, 300), (4, 1, 2, 16)], ids=lambda s: "x".join(map(str, s)))
def test_lift_skip_filter_is_conv2d_on_the_reflected_plane(shape):
    """the lifting skip filter (reflection pad of one row, 3x1 convolution; model.py lift_skip) under the rule aten_rules.py
    assigns to its shape, against F.conv2d on planes ATen hands to its direct convolution"""
    from pmctf_oracle import aten_rules, clib
    n, c, h, w = shape
    r = np.random.default_rng([10, *shape])
    w3 = r.standard_normal((1, 1, 3, 1)).astype(np.float32)
    rule = aten_rules.conv_kxk_sum_rule(1, 1, 3, 1, n, h + 2, w)
    for name, x, b in (("quantised", ev.quantised(shape), np.array([ev.NEG0], np.float32)),
                       ("normal", _normal(shape), np.array([0.3125], np.float32))):
        xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (0, 0)), mode="reflect")
        ref = clib.conv2d(xp, w3, b, 1, (0, 0), rule)
        want = F.conv2d(torch.from_numpy(xp), torch.from_numpy(w3), torch.from_numpy(b)).numpy()
        ev.bits_equal(ref, want, f"lift_skip {shape} {name} rule {rule}")
