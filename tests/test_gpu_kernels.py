"""HIP primitives vs the oracle's C restatement: bit-exact (PM-F32 arithmetic spec)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rng(seed):
    return np.random.default_rng(seed)


def nhwc(x):  # numpy NCHW -> torch NHWC on device
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 1))).cuda()


def nchw(t):  # torch NHWC device -> numpy NCHW
    return t.cpu().numpy().transpose(0, 3, 1, 2)


def assert_same(a, b, what):
    """float32 arrays as bit patterns: -0 is not +0, and two NaNs are equal whatever their payloads (math_sweep.compare);
    integer arrays by value"""
    a = np.asarray(a); b = np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == np.float32:
        import math_sweep as ms
        ua, ub = np.ascontiguousarray(a).view(np.uint32).reshape(-1), np.ascontiguousarray(b).view(np.uint32).reshape(-1)
        count, first, _ = ms.compare(ua, ub)
        if count:
            i = np.unravel_index(first, a.shape)
            raise AssertionError(f"{what}: {count} / {a.size} bit patterns differ; first at {tuple(int(k) for k in i)}: "
                                 f"{a[i]!r} ({int(ua[first]):#010x}) vs {b[i]!r} ({int(ub[first]):#010x})")
        return
    neq = a != b
    if neq.any():
        i = np.argwhere(neq)[0]
        raise AssertionError(f"{what}: {neq.sum()} / {a.size} elements differ; first at {tuple(i)}: "
                             f"{a[tuple(i)]!r} vs {b[tuple(i)]!r}")


CONV_CASES = [
    # N, Cin, H, W, Cout, K, stride, pad, act, slope, nres
    (1, 112, 40, 72, 112, 3, 1, 1, 2, 0.2, 0),     # ContextResidual conv (small plane -> 8x16 tiles)
    (1, 112, 264, 520, 112, 3, 1, 1, 0, 0.0, 2),   # big plane -> 8x32 tiles, ragged edges, 2 residual adds
    (2, 64, 33, 47, 64, 3, 1, 1, 2, 0.2, 1),       # PostProcess ResBlock, odd sizes, batch 2
    (1, 8, 36, 60, 32, 7, 1, 3, 1, 0.0, 0),        # SpyNet conv1 (Cin=8: half chunk)
    (1, 32, 36, 60, 64, 7, 1, 3, 1, 0.0, 0),       # SpyNet conv2
    (1, 16, 72, 120, 2, 7, 1, 3, 0, 0.0, 0),       # SpyNet conv5 (Cout=2)
    (1, 16, 64, 64, 1, 3, 1, 1, 0, 0.0, 0),        # PredictUpdate conv4
    (1, 16, 64, 64, 16, 3, 1, 1, 3, 0.0, 0),       # PredictUpdate conv2 + tanh
    (2, 16, 150, 203, 16, 3, 1, 1, 3, 0.0, 0),     # persistent 16->16 kernel: ragged tiles, two planes, tanh
    (1, 16, 129, 130, 16, 3, 1, 1, 0, 0.0, 1),     # persistent 16->16 kernel: residual add
    (1, 16, 130, 141, 16, 3, 1, 1, 2, 0.1, 2),     # persistent 16->16 kernel: leaky, two residual adds, ragged tiles
    (3, 16, 96, 64, 16, 3, 1, 1, 0, 0.0, 0),       # persistent 16->16 kernel: only whole tiles, three planes (XCD bands)
    (1, 64, 64, 96, 64, 3, 2, 1, 2, 0.01, 0),      # stride-2 3x3
    (1, 64, 64, 96, 64, 1, 2, 0, 0, 0.0, 0),       # stride-2 1x1 (downsample)
    (1, 256, 18, 30, 192, 1, 1, 0, 0, 0.0, 0),     # four-part prior adaptor 1x1 256->192
    (1, 128, 20, 36, 128, 3, 1, 1, 2, 0.2, 1),     # masked residual block (weights pre-masked)
    (1, 32, 40, 64, 3, 3, 1, 1, 0, 0.0, 0),        # LSTM3 conv_in 32->3
    (1, 1, 64, 80, 16, 3, 1, 1, 3, 0.0, 0),        # small-cin 1->16 + tanh
    (2, 2, 37, 53, 112, 3, 1, 1, 0, 0.0, 0),       # small-cin 2->112
    (1, 2, 64, 96, 64, 3, 2, 1, 2, 0.01, 0),       # small-cin stride 2
    (1, 3, 30, 40, 3, 3, 1, 1, 0, 0.0, 1),         # 3->3 with residual
    (1, 1, 45, 83, 112, 3, 1, 1, 2, 0.2, 0),       # strip kernel: 1->112, ragged width, leaky
    (2, 1, 18, 16, 64, 3, 1, 1, 0, 0.0, 2),        # strip kernel: 1->64, one strip per row, two residual adds
    (1, 1, 20, 36, 128, 3, 1, 1, 3, 0.0, 0),       # strip kernel: 1->128 + tanh
    (1, 3, 17, 40, 192, 3, 1, 1, 0, 0.0, 1),       # strip kernel: 3->192 (3 cout groups -> 4 waves, one idle)
    (2, 64, 37, 45, 1, 3, 1, 1, 0, 0.0, 1),        # few-cout kernel: PostProcess 64->1 with residual, 4 chunks
    (1, 16, 33, 70, 1, 3, 1, 1, 2, 0.1, 2),        # few-cout kernel: 16->1, leaky, two residuals
    (1, 192, 37, 53, 768, 1, 1, 0, 2, 0.1, 0),     # 1x1 GEMM kernel: MV-codec 192->768, ragged pixel count, 3 k-chunks
    (1, 768, 18, 31, 192, 1, 1, 0, 0, 0.0, 1),     # 1x1 GEMM kernel: 768->192 with residual, 12 k-chunks
    (2, 64, 130, 129, 256, 1, 1, 0, 1, 0.0, 0),    # 1x1 GEMM kernel: 64-pixel workgroups (>= 32768 px), one k-chunk
    (1, 80, 20, 36, 40, 1, 1, 0, 0, 0.0, 2),       # 1x1 GEMM kernel: 5 channel blocks (odd), cout not a multiple of 16
    (1, 48, 9, 7, 24, 1, 1, 0, 3, 0.0, 0),         # 1x1 GEMM kernel: fewer pixels than one workgroup tile, tanh
    (2, 112, 37, 41, 112, 1, 1, 0, 2, 0.2, 1),     # 1x1 GEMM kernel: 7 cout tiles on 4 waves (one wave with a single live tile)
]


@pytest.mark.parametrize("rule", [0, 1], ids=["chain", "blocks"])
@pytest.mark.parametrize("case", CONV_CASES, ids=[f"c{i}" for i in range(len(CONV_CASES))])
def test_conv2d_bitexact(cuda, case, rule):
    """every layer shape of the path, under both summation rules (include/pmctf_hip.h PMCTF_SUM_*)"""
    from pmctf_oracle import clib
    from pMCTF.hip import ops
    N, Cin, H, W, Cout, K, S, P, act, slope, nres = case
    r = _rng(1000 + Cin * 7 + Cout)
    x = r.standard_normal((N, Cin, H, W), dtype=np.float32) * 3
    w = (r.standard_normal((Cout, Cin, K, K), dtype=np.float32) * 0.05).astype(np.float32)
    b = r.standard_normal(Cout, dtype=np.float32)
    ref = clib.conv2d(x, w, b, S, (P, P), rule)
    if act == 1:
        ref = np.maximum(ref, 0)
    elif act == 2:
        ref = np.where(ref > 0, ref, ref * np.float32(slope)).astype(np.float32)
    elif act == 3:
        ref = clib.tanh(ref)
    res = [r.standard_normal(ref.shape, dtype=np.float32) for _ in range(nres)]
    for q in res:
        ref = ref + q
    conv = ops.Conv2d(torch.from_numpy(w), torch.from_numpy(b), S, (P, P), rule=rule)
    y = conv(nhwc(x), act=act, slope=slope, res1=nhwc(res[0]) if nres > 0 else None,
             res2=nhwc(res[1]) if nres > 1 else None)
    torch.cuda.synchronize()
    assert_same(nchw(y), ref, f"conv {case}")


def _random_conv_cases(seed, count):
    """Seeded draw over everything the conv entry points accept: channel counts on and off the 16-channel chunk, filters
    1/3/5/7 (5x5 only exists on the generic kernels), strides 1-3, 'same' / 'valid' / asymmetric padding, planes smaller
    than one tile and smaller than the filter's reach, 1-3 planes, every activation, 0-2 residual adds."""
    r = _rng(seed)
    cases = []
    while len(cases) < count:
        cin = int(r.choice([1, 2, 3, 4, 8, 12, 16, 20, 32, 48, 64, 80, 112, 128, 192]))
        cout = int(r.choice([1, 2, 3, 5, 16, 17, 24, 32, 40, 64, 96, 112, 128, 192, 256]))
        k = int(r.choice([1, 3, 3, 3, 5, 7]))
        s = int(r.choice([1, 1, 1, 2, 3]))
        ph, pw = (int(v) for v in r.choice([0, k // 2, k // 2, k - 1], size=2))
        n = int(r.choice([1, 1, 2, 3]))
        h, w = int(r.integers(max(1, k - 2 * ph), 70)), int(r.integers(max(1, k - 2 * pw), 90))
        if cin * cout * k * k * 4 > 64 * 1024 and cin <= 4:
            continue                                    # the small-cin kernel keeps its filter in 64 KB of LDS
        cases.append((n, cin, h, w, cout, k, s, ph, pw, int(r.integers(0, 5)), float(r.choice([0.0, 0.01, 0.2])),
                      int(r.integers(0, 3))))
    return cases


@pytest.mark.parametrize("rule", [0, 1, 32, 96], ids=["chain", "blocks", "reduce32", "reduce96"])
@pytest.mark.parametrize("seed", [101, 202, 303])
def test_conv2d_random_shapes_bitexact(cuda, seed, rule):
    """Fuzz of pmctf_conv2d_nhwc_opts_f32 / _smallcin_f32 / _fewcout_f32 behind ops.Conv2d against the oracle's C
    convolution, under both summation rules (PMCTF_SUM_CHAIN / PMCTF_SUM_BLOCKS): whatever kernel variant the dispatcher
    picks for a shape, the bits are PM-F32's for that rule."""
    from pmctf_oracle import clib
    from pMCTF.hip import ops
    for case in _random_conv_cases(seed, 24):
        n, cin, h, w_, cout, k, s, ph, pw, act, slope, nres = case
        if rule >= 16 and (cin <= 4 or (cout <= 2 and cin in (16, 64))):
            continue                                    # reduce-B exists on the matrix-core path only
        r = _rng(seed * 1000 + cin + cout + h)
        x = r.standard_normal((n, cin, h, w_), dtype=np.float32) * 2
        wt = (r.standard_normal((cout, cin, k, k), dtype=np.float32) * 0.1).astype(np.float32)
        b = r.standard_normal(cout, dtype=np.float32)
        ref = clib.conv2d(x, wt, b, s, (ph, pw), rule)
        if act == 1:
            ref = np.maximum(ref, 0)
        elif act == 2:
            ref = np.where(ref > 0, ref, ref * np.float32(slope)).astype(np.float32)
        elif act == 3:
            ref = clib.tanh(ref)
        elif act == 4:
            ref = clib.sigmoid(ref)
        res = [r.standard_normal(ref.shape, dtype=np.float32) for _ in range(nres)]
        for q in res:
            ref = ref + q
        conv = ops.Conv2d(torch.from_numpy(wt), torch.from_numpy(b), s, (ph, pw), rule=rule)
        y = conv(nhwc(x), act=act, slope=slope, res1=nhwc(res[0]) if nres > 0 else None,
                 res2=nhwc(res[1]) if nres > 1 else None)
        torch.cuda.synchronize()
        assert_same(nchw(y), ref, f"conv (N, Cin, H, W, Cout, K, S, pad_h, pad_w, act, slope, nres) = {case}")


def test_conv2d_denormals_and_specials(cuda):
    """MFMA f32 must behave as an fmaf chain also on subnormal products / tiny accumulators."""
    from pmctf_oracle import clib
    from pMCTF.hip import ops
    r = _rng(5)
    x = r.standard_normal((1, 16, 32, 32), dtype=np.float32)
    x[:, ::2] *= np.float32(1e-22)
    w = r.standard_normal((16, 16, 3, 3), dtype=np.float32) * np.float32(1e-20)
    b = np.zeros(16, np.float32)
    ref = clib.conv2d(x, w, b, 1, (1, 1))
    y = ops.Conv2d(torch.from_numpy(w), torch.from_numpy(b), 1, (1, 1))(nhwc(x))
    torch.cuda.synchronize()
    assert_same(nchw(y), ref, "denormal conv")


@pytest.mark.parametrize("shape", [(2, 64, 37, 51), (1, 112, 20, 36), (1, 6, 19, 23), (1, 192, 3, 2),
                                   (2, 128, 331, 421)])      # the last one is large enough for the column-walking kernel
def test_dwconv_bitexact(cuda, shape):
    from pmctf_oracle import clib
    from pMCTF.hip import ops
    r = _rng(7)
    x = r.standard_normal(shape, dtype=np.float32)
    w = r.standard_normal((shape[1], 1, 3, 3), dtype=np.float32)
    b = r.standard_normal(shape[1], dtype=np.float32)
    ref = clib.dwconv2d(x, w, b)
    y = ops.DepthwiseConv2d(torch.from_numpy(w), torch.from_numpy(b))(nhwc(x))
    assert_same(nchw(y), ref, "dwconv")


@pytest.mark.parametrize("shape", [(1, 1, 64, 96), (2, 1, 37, 53), (1, 3, 36, 60)])
def test_flow_warp_bitexact(cuda, shape):
    from pmctf_oracle import clib
    from pMCTF.hip import ops
    N, Cc, H, W = shape
    r = _rng(11)
    im = (r.random(shape, dtype=np.float32) * 255).astype(np.float32)
    flow = (r.standard_normal((1, 2, H, W), dtype=np.float32) * 6).astype(np.float32)
    flow[0, 0, 0, :] = 1000.0   # far outside: border clamp
    flow[0, 1, :, 0] = -1000.0
    lx = torch.linspace(-1.0, 1.0, W).numpy(); ly = torch.linspace(-1.0, 1.0, H).numpy()
    for sign in (1.0, -1.0):
        ref = clib.flow_warp(im, flow * np.float32(sign), lx, ly)
        out = ops.flow_warp(torch.from_numpy(im).cuda(), torch.from_numpy(flow).cuda(),
                            torch.from_numpy(lx).cuda(), torch.from_numpy(ly).cuda(), sign)
        assert_same(out.cpu().numpy(), ref, f"warp sign {sign}")


def test_resample_bitexact(cuda):
    from pmctf_oracle import clib
    from pMCTF.hip import ops
    r = _rng(13)
    x = (r.standard_normal((2, 3, 36, 60), dtype=np.float32) * 10).astype(np.float32)
    xt = torch.from_numpy(x).cuda()
    assert_same(ops.avgpool2(xt).cpu().numpy(), clib.avgpool2(x), "avgpool2")
    assert_same(ops.bilinear_up2(xt, 2.0).cpu().numpy(), clib.bilinear_up2(x) * np.float32(2), "up2")
    assert_same(ops.bilinear_down2(xt, 2.0).cpu().numpy(), clib.bilinear_down2(x) / np.float32(2), "down2")
    x = (r.standard_normal((1, 2, 40, 72), dtype=np.float32) * 10).astype(np.float32)       # me_downsample factors
    xt = torch.from_numpy(x).cuda()
    for f in (2, 4, 8):
        assert_same(ops.bilinear_up2(xt, float(f), f).cpu().numpy(), clib.bilinear_up(x, f) * np.float32(f), f"up x{f}")
        assert_same(ops.bilinear_down2(xt, 1.0, f).cpu().numpy(), clib.bilinear_down(x, f), f"down /{f}")


@pytest.mark.parametrize("shape", [(1, 112, 44, 72, 112, 3, 1), (2, 64, 70, 100, 64, 3, 1), (1, 112, 264, 520, 112, 3, 1),
                                   (1, 16, 140, 150, 16, 3, 1),
                                   (1, 32, 48, 80, 64, 7, 1), (1, 64, 45, 70, 32, 7, 1), (2, 32, 37, 50, 16, 7, 1),
                                   (1, 64, 64, 96, 128, 3, 2), (1, 192, 20, 36, 256, 1, 1),
                                   # the shapes the block-sum variants of the specialised 3x3 kernels are launched on
                                   (1, 112, 144, 240, 112, 3, 2), (1, 128, 40, 72, 128, 3, 1), (2, 32, 60, 100, 32, 3, 1),
                                   (1, 112, 150, 250, 112, 3, 1), (1, 112, 36, 60, 112, 3, 1)])
@pytest.mark.parametrize("rule", [0, 1], ids=["chain", "blocks"])
def test_conv2d_launch_shapes_do_not_change_results(cuda, shape, rule):
    """Every way of cutting a convolution into workgroups (cout-tile split, row split, tile size, kernel variant)
    gives the same bits, under either summation rule: pmctf_conv2d_set_option only moves work around."""
    from pmctf_oracle import clib
    from pMCTF.hip import lib, ops
    N, Cin, H, W, Cout, K, S = shape
    r = _rng(77 + Cin + H)
    x = r.standard_normal((N, Cin, H, W), dtype=np.float32)
    w = (r.standard_normal((Cout, Cin, K, K), dtype=np.float32) * 0.05).astype(np.float32)
    b = r.standard_normal(Cout, dtype=np.float32)
    ref = clib.conv2d(x, w, b, S, (K // 2, K // 2), rule)
    conv = ops.Conv2d(torch.from_numpy(w), torch.from_numpy(b), S, (K // 2, K // 2), rule=rule)
    xd = nhwc(x)
    L = lib.hip()
    defaults = {"WAVE": 1, "NT": 0, "MSPLIT_PX": 70000, "SPLIT": 1, "BIGPX": 131072, "V1": 0, "V2": 0, "RES": 0, "MSPLIT_NT": 1,
                "C16": 1, "C16_WGS": 512, "C16_OCC": 2, "NBUF1": 1, "K33": 1, "WAVE_SMALL": 1, "K11": 1, "K77": 1, "K33_SMALL": 1, "BIGPX_NOSPLIT": 200000}
    settings = [{}, {"MSPLIT_PX": 0}, {"MSPLIT_PX": 1 << 40}, {"SPLIT": 0, "MSPLIT_PX": 0},
                {"SPLIT": 0, "MSPLIT_PX": 0, "BIGPX_NOSPLIT": 0}, {"SPLIT": 0, "MSPLIT_PX": 0, "BIGPX_NOSPLIT": 1 << 40}, {"BIGPX": 0, "MSPLIT_PX": 0},
                {"NT": 1, "MSPLIT_PX": 0}, {"NT": 2, "MSPLIT_PX": 0}, {"NT": 4, "MSPLIT_PX": 0},
                {"NT": 4, "MSPLIT_PX": 0, "WAVE": 0}, {"V1": 1, "MSPLIT_PX": 0}, {"V2": 1, "MSPLIT_PX": 0},
                {"V2": 1, "MSPLIT_PX": 1 << 40}, {"RES": 1, "MSPLIT_PX": 1 << 40}, {"RES": 2, "MSPLIT_PX": 1 << 40}, {"MSPLIT_NT": 2, "MSPLIT_PX": 1 << 40},
                {"MSPLIT_NT": 4, "MSPLIT_PX": 1 << 40}, {"C16": 0}, {"C16_WGS": 3}, {"C16_OCC": 0}, {"C16_OCC": 0, "C16_WGS": 3}, {"C16_OCC": 3}, {"C16_OCC": 4},
                # the shape-specialised kernels against the generic ones
                {"K33": 0, "NT": 4, "MSPLIT_PX": 0}, {"K33": 0, "NT": 1, "MSPLIT_PX": 0}, {"K77": 0, "NT": 4, "MSPLIT_PX": 0},
                {"K11": 0}, {"WAVE_SMALL": 0, "MSPLIT_PX": 1 << 40}, {"WAVE_SMALL": 1, "MSPLIT_PX": 1 << 40},
                {"NBUF1": 0, "NT": 4, "MSPLIT_PX": 0}, {"K33_SMALL": 0, "MSPLIT_PX": 1 << 40, "WAVE_SMALL": 0},
                {"K33_SMALL": 1, "MSPLIT_PX": 1 << 40, "WAVE_SMALL": 0}]
    try:
        for st in settings:
            for k, v in {**defaults, **st}.items():
                assert L.pmctf_conv2d_set_option(k.encode(), v) == 0
            y = conv(xd)
            torch.cuda.synchronize()
            assert_same(nchw(y), ref, f"conv {shape} with options {st}")
    finally:
        for k, v in defaults.items():
            L.pmctf_conv2d_set_option(k.encode(), v)
    assert L.pmctf_conv2d_set_option(b"NO_SUCH_KNOB", 1) != 0


def test_conv3x3_cin1_dual_output(cuda):
    """PredictUpdate conv1: conv and tanh(conv) from one launch, both bit-exact"""
    from pmctf_oracle import clib
    from pMCTF.hip import ops
    r = _rng(5)
    x = r.standard_normal((2, 1, 37, 70), dtype=np.float32) * 40
    w = (r.standard_normal((16, 1, 3, 3), dtype=np.float32) * 0.1).astype(np.float32)
    b = r.standard_normal(16, dtype=np.float32)
    for rule in (0, 1):
        ref = clib.conv2d(x, w, b, 1, (1, 1), rule)
        conv = ops.Conv2d(torch.from_numpy(w), torch.from_numpy(b), 1, (1, 1), rule=rule)
        y, y2 = ops.conv3x3_cin1_dual(conv, nhwc(x), ops.ACT_TANH)
        torch.cuda.synchronize()
        assert_same(nchw(y), ref, f"conv1 rule {rule}")
        assert_same(nchw(y2), clib.tanh(ref), f"tanh(conv1) rule {rule}")


@pytest.mark.parametrize("shape", [(1, 112, 112, 37, 53), (2, 64, 64, 48, 64), (1, 64, 112, 16, 32), (3, 112, 64, 7, 90)])
def test_split_precision_conv_tracks_the_exact_kernel(cuda, shape):
    """conv_split.hip, the AUXILIARY reduced-precision 3x3 kernel (bf16 MFMA, operands split into 3 / 2 / 1 planes): not
    bit-exact by design — checked against the exact f32 kernel to the accuracy each split promises, on sizes that do not
    divide into its 16x32 tiles, with activation and both residual inputs, and for run-to-run determinism."""
    from pMCTF.hip import ops
    n, cin, cout, h, w = shape
    rng = _rng(h * w + cin)
    wt = torch.from_numpy((rng.standard_normal((cout, cin, 3, 3)) * 0.05).astype(np.float32))
    b = torch.from_numpy(rng.standard_normal(cout).astype(np.float32))
    x = torch.from_numpy(rng.standard_normal((n, h, w, cin)).astype(np.float32)).cuda()
    r1 = torch.from_numpy(rng.standard_normal((n, h, w, cout)).astype(np.float32)).cuda()
    r2 = torch.from_numpy(rng.standard_normal((n, h, w, cout)).astype(np.float32)).cuda()
    exact = ops.Conv2d(wt, b, 1, (1, 1))(x, act=ops.ACT_LEAKY, slope=0.2, res1=r1, res2=r2)
    old = ops.SPLIT_MIN_PX
    ops.SPLIT_MIN_PX = 0
    try:
        for ns, tol in ((3, 3e-6), (2, 3e-4), (1, 3e-2)):
            conv = ops.Conv2d(wt, b, 1, (1, 1), split=ns)
            assert conv.split == ns
            y = conv(x, act=ops.ACT_LEAKY, slope=0.2, res1=r1, res2=r2)
            err = (y - exact).abs().max().item() / exact.abs().max().item()
            assert err < tol, (ns, err)
            assert torch.equal(y, conv(x, act=ops.ACT_LEAKY, slope=0.2, res1=r1, res2=r2)), "not deterministic"
            assert err > 0, ns                              # the split kernel really ran
    finally:
        ops.SPLIT_MIN_PX = old


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 112, 44, 70), (2, 112, 18, 36), (1, 32, 100, 66)])
def test_split_precision_conv_at_parity_class(cuda, shape):
    """The stride-2 form of the auxiliary kernel (the quarter-resolution context convolutions, ops.conv_at_class): against
    the exact kernel at the same positions — which itself equals the full convolution sampled at that parity class —
    for all four classes, with activation and residual, on sizes that do not divide into 8x32 tiles; deterministic."""
    from pMCTF.hip import ops
    n, cin, h, w = shape
    rng = _rng(h * w + cin + 1)
    wt = torch.from_numpy((rng.standard_normal((112, cin, 3, 3)) * 0.05).astype(np.float32))
    b = torch.from_numpy(rng.standard_normal(112).astype(np.float32))
    x = torch.from_numpy(rng.standard_normal((n, h, w, cin)).astype(np.float32)).cuda()
    r1 = torch.from_numpy(rng.standard_normal((n, h // 2, w // 2, 112)).astype(np.float32)).cuda()
    exact_conv = ops.Conv2d(wt, b, 1, (1, 1))
    full = exact_conv(x)
    old = ops.SPLIT_MIN_PX
    ops.SPLIT_MIN_PX = 0
    try:
        for cls in range(4):
            py, px = cls >> 1, cls & 1
            exact = ops.conv_at_class(exact_conv, x, cls, act=ops.ACT_LEAKY, slope=0.2, res1=r1)
            assert torch.equal(ops.conv_at_class(exact_conv, x, cls), full[:, py::2, px::2].contiguous())
            for ns, tol in ((3, 3e-6), (2, 3e-4), (1, 3e-2)):
                conv = ops.Conv2d(wt, b, 1, (1, 1), split=ns)
                assert conv.split == ns
                y = ops.conv_at_class(conv, x, cls, act=ops.ACT_LEAKY, slope=0.2, res1=r1)
                err = (y - exact).abs().max().item() / exact.abs().max().item()
                assert 0 < err < tol, (cls, ns, err)          # > 0: the split kernel really ran
                assert torch.equal(y, ops.conv_at_class(conv, x, cls, act=ops.ACT_LEAKY, slope=0.2, res1=r1))
    finally:
        ops.SPLIT_MIN_PX = old


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(1, 3, 3, 3, 48, 88, 2), (1, 2, 112, 3, 37, 53, 2), (1, 4, 16, 3, 20, 36, 2), (2, 3, 3, 3, 17, 40, 2),
                                  (1, 1, 1, 3, 96, 176, 3), (1, 1, 1, 3, 33, 47, 3), (2, 1, 1, 3, 20, 30, 3)])
def test_small_plane_rules_bitexact(cuda, case):
    """PMCTF_SUM_GEMM / PMCTF_SUM_GEMV_3X3 (the orders of ATen's im2col + sgemm path on small planes, include/pmctf_hip.h) in
    the small-cin kernel against the oracle's restatement, with activation and residual"""
    from pmctf_oracle import clib
    from pMCTF.hip import ops
    n, cin, cout, k, h, w, rule = case
    rng = _rng(h * w + cin)
    x = (rng.standard_normal((n, cin, h, w)) * 2).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, k, k)) * 0.2).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    r1 = rng.standard_normal((n, cout, h, w)).astype(np.float32)
    ref = clib.conv2d(x, wt, b, 1, (k // 2, k // 2), rule)
    ref = np.where(ref > 0, ref, ref * np.float32(0.2)).astype(np.float32) + r1
    conv = ops.Conv2d(torch.from_numpy(wt), torch.from_numpy(b), 1, (k // 2, k // 2), rule=rule)
    y = conv(torch.from_numpy(x).permute(0, 2, 3, 1).contiguous().cuda(), act=ops.ACT_LEAKY, slope=0.2,
             res1=torch.from_numpy(r1).permute(0, 2, 3, 1).contiguous().cuda())
    assert_same(y.permute(0, 3, 1, 2).cpu().numpy(), ref, f"rule {rule}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 112, 144, 240), (2, 112, 44, 72), (1, 112, 30, 52)])
def test_conv_at_parity_class_under_the_block_rule(cuda, shape):
    """ops.conv_at_class with summation rule "blocks" (the quarter-resolution context convolutions
    follow ATen's order too): the same bits as the full convolution under that rule at the positions of the class,
    whichever kernel the plane size selects (stride-2 pipelined kernel from 8 000 output pixels up, cout-split below)."""
    from pmctf_oracle import clib
    from pMCTF.hip import ops
    n, cin, h, w = shape
    rng = _rng(h * w + 7)
    wt = (rng.standard_normal((112, cin, 3, 3)) * 0.05).astype(np.float32)
    b = rng.standard_normal(112).astype(np.float32)
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    ref = clib.conv2d(x, wt, b, 1, (1, 1), 1)
    conv = ops.Conv2d(torch.from_numpy(wt), torch.from_numpy(b), 1, (1, 1), rule=ops.SUM_BLOCKS)
    xt = torch.from_numpy(x).permute(0, 2, 3, 1).contiguous().cuda()
    for cls in range(4):
        py, px = cls >> 1, cls & 1
        y = ops.conv_at_class(conv, xt, cls).permute(0, 3, 1, 2).cpu().numpy()
        assert_same(y, np.ascontiguousarray(ref[:, :, py::2, px::2]), f"class {cls}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", __import__("conv_census").GEOM_ZERO, ids=lambda c: c[0])
def test_conv_at_parity_class_on_zeros_of_both_signs(cuda, case):
    """the per-class padding of pmctf_conv2d_nhwc_geom_f32 (stride 2, a halo on one side only) on the zero data of the
    convolution censuses: all four classes under the case's rule are the oracle's full convolution at the positions of the
    class, bit for bit — the padded zero multiplied in on the edge the class pads, no tap invented on the other.  The
    preconditions (both zero signs; a skipping kernel would show on the padded edge) are asserted without a GPU in
    test_conv_census_cpu.py."""
    import conv_census as cc
    from pMCTF.hip import ops
    rid, (n, cin, h, w, cout), rule = case
    x, wt, b = cc.geom_zero_data(case)
    ref, _ = cc.geom_zero_reference(case)
    conv = ops.Conv2d(torch.from_numpy(wt), torch.from_numpy(b), 1, (1, 1), rule=rule)
    assert not conv.small and not conv.few and not conv.split
    xt = nhwc(x)
    for cls in range(4):
        assert_bits(nchw(ops.conv_at_class(conv, xt, cls)), ref[cls], f"{rid} class {cls}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 8, 5, 7), (1, 6, 9, 4), (3, 64, 6, 10), (1, 3, 4, 4)])
def test_nearest_up2_and_pixel_shuffle2_are_exact_copies(cuda, shape):
    """nearest x2 upsampling and nn.PixelShuffle(2) on NHWC (scalar and 16-byte forms: C % 4 == 0 or not) against the torch
    ops the reference uses (long_context.py:156-170 F.interpolate nearest, video_net.py subpel convs' PixelShuffle)"""
    import torch.nn.functional as F
    from pMCTF.hip import ops
    n, c, h, w = shape
    x = _rng(c * h).standard_normal((n, c, h, w), dtype=np.float32)
    up = ops.nearest_up2(nhwc(x))
    assert_same(nchw(up), F.interpolate(torch.from_numpy(x), scale_factor=2, mode="nearest").numpy(), "nearest_up2")
    x4 = _rng(c + w).standard_normal((n, 4 * c, h, w), dtype=np.float32)
    ps = ops.pixel_shuffle2(nhwc(x4))
    assert_same(nchw(ps), F.pixel_shuffle(torch.from_numpy(x4), 2).numpy(), "pixel_shuffle2")
    ps = ops.pixel_shuffle2(nhwc(x4), act=ops.ACT_LEAKY, slope=0.1)
    assert_same(nchw(ps), F.leaky_relu(F.pixel_shuffle(torch.from_numpy(x4), 2), 0.1).numpy(), "pixel_shuffle2 + leaky")


def test_elementwise_ops_every_layout(cuda):
    """pmctf_ew_f32 over the operand layouts the engine hands it — whole planes and whole NHWC tensors (the flat 16-byte
    form, with and without a vector tail), channel slices of NHWC tensors, row / column windows, a broadcast second
    operand, in place — every op against a numpy float32 restatement: bit-exact.  (Which kernel each layout reaches, and
    the special values, are the business of tests/ew_census.py.)"""
    import ew_census as ec
    from pMCTF.hip import ops
    r = _rng(99)

    def dev(x):
        return torch.from_numpy(x).cuda()
    layouts = []
    for shape in [(1, 1, 37, 53), (1, 1, 64, 96), (2, 3, 20, 36)]:                 # planar, dense: flat scalar / flat vec
        layouts.append(("planar", shape, lambda t: t, lambda t: t))
    layouts.append(("nhwc dense", (2, 16, 20, 36), lambda t: t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), None))
    layouts.append(("nhwc channel slice", (1, 8, 19, 23),
                    lambda t: torch.cat([t, t], 1).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)[:, 8:], None))
    layouts.append(("nhwc parity-class gather", (1, 12, 9, 11),          # as_nchw(t)[:, :, 1::2, 0::2] of a (1,18,22,12) tensor
                    lambda t: torch.nn.functional.interpolate(t, scale_factor=2, mode="nearest")
                    .permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)[:, :, 1::2, 0::2], None))
    layouts.append(("nhwc odd channel slice", (1, 8, 10, 14),            # 8 of 16 channels from channel 3 on: not 16-byte aligned
                    lambda t: torch.cat([t[:, :3], t, t[:, :5]], 1).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)[:, 3:11], None))
    layouts.append(("transposed planes", (2, 3, 37, 70), lambda t: t.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), None))
    layouts.append(("even rows", (1, 2, 9, 20), lambda t: torch.repeat_interleave(t, 2, dim=2)[:, :, ::2, :], None))
    layouts.append(("odd rows, ragged width", (2, 1, 7, 18), lambda t: torch.repeat_interleave(t, 2, dim=2)[:, :, 1::2, :], None))
    layouts.append(("row window", (1, 2, 16, 40), lambda t: torch.cat([t, t, t], 2)[:, :, 16:32], None))
    layouts.append(("column window", (2, 1, 18, 24), lambda t: torch.cat([t, t], 3)[:, :, :, 24:], None))
    binary = {ops.EW_ADD, ops.EW_SUB, ops.EW_MUL, ops.EW_DIV, ops.EW_ADD_MULS, ops.EW_SUB_MULS, ops.EW_ADD_MULS_MULS,
              ops.EW_ADD_MULS2, ops.EW_SUB_MULS2}
    for name, shape, place, _ in layouts:
        a = (r.standard_normal(shape, dtype=np.float32) * 3).astype(np.float32)
        b = (r.standard_normal(shape, dtype=np.float32) + np.float32(2.5)).astype(np.float32)
        ta, tb = place(dev(a)), place(dev(b))
        assert tuple(ta.shape) == shape
        for op in range(18):
            alpha, beta = (0.37, 2.25) if op != ops.EW_ROUND_CLAMP else (-2.0, 3.0)
            want = ec.expected(op, a, b, alpha, beta)                  # the restatement of the census, pinned to torch there
            got = ops.ew(op, ta, tb if op in binary else None, alpha, beta)
            assert_same(got.cpu().numpy(), want, f"ew op {op} on {name} {shape}")
        # second operand broadcast over the planes (stride 0), and the result written over the first operand
        b1 = b[:1, :1]
        got = ops.ew(ops.EW_SUB_MULS, ta, dev(b1).expand(*shape), 0.37)
        assert_same(got.cpu().numpy(), a - b1 * np.float32(0.37), f"ew broadcast on {name}")
        tc = ta.clone() if ta.is_contiguous() else place(dev(a))
        ops.ew(ops.EW_ADD, tc, tb, out=tc)
        assert_same(tc.cpu().numpy(), a + b, f"ew in place on {name}")


@pytest.mark.gpu
def test_lstm_gates_with_aten_thread_tails(cuda):
    """lstm_gates (long_context.py:20-33) against the oracle's primitives: sigmoid as ATen evaluates it with 8 intra-op
    threads on the reference's contiguous (planes, C, H, W) gate tensor — SLEEF on whole strides of 32 floats of a thread's
    slice, libm's expf on the rest (the (2, 3, 144, 240) tensor of the path: seven slices of 29 623 elements) — and the same
    values when two reference tensors are stacked into one batch (ref_planes)."""
    from pmctf_oracle import clib
    from pMCTF.hip import ops
    rng = _rng(77)
    for (n_ref, c, h, w, cc) in ((2, 3, 144, 240, 1), (1, 32, 36, 60, 32), (2, 3, 30, 44, 3)):
        xs, cells, refs = [], [], []
        for rep in range(2):
            x = (rng.standard_normal((n_ref, c, h, w)) * 3).astype(np.float32)
            cell = rng.standard_normal((n_ref, cc, h, w)).astype(np.float32)
            g = clib.sigmoid(x, 8)
            ct = clib.tanh(x)
            cn = g * cell + g * ct
            hid = g * clib.tanh(np.ascontiguousarray(cn))
            xs.append(x); cells.append(cell); refs.append((hid, cn))
        assert not np.array_equal(clib.sigmoid(xs[0], 8), clib.sigmoid(xs[0])) or (n_ref, c, h, w) != (2, 3, 144, 240)
        nhwc = lambda t: torch.from_numpy(np.ascontiguousarray(t.transpose(0, 2, 3, 1))).cuda()
        for rep in range(2):                                   # one reference tensor per call
            hid, cn = ops.lstm_gates(nhwc(xs[rep]), nhwc(cells[rep]), ref_planes=n_ref, aten_threads=8)
            assert_same(hid.permute(0, 3, 1, 2).cpu().numpy(), refs[rep][0], "hidden")
            assert_same(cn.permute(0, 3, 1, 2).cpu().numpy(), refs[rep][1], "cell")
        hid, cn = ops.lstm_gates(nhwc(np.concatenate(xs)), nhwc(np.concatenate(cells)), ref_planes=n_ref, aten_threads=8)
        assert_same(hid.permute(0, 3, 1, 2).cpu().numpy(), np.concatenate([r[0] for r in refs]), "hidden, stacked batch")
        assert_same(cn.permute(0, 3, 1, 2).cpu().numpy(), np.concatenate([r[1] for r in refs]), "cell, stacked batch")


def test_scale_index_rows_at_every_gpu_site(cuda):
    """Every GPU site that selects a CDF row from a scale (decode: fourstep_indexes, mv_fourpart_indexes; encode:
    fourstep_quant, ll_quant, mv_fourpart) against the reference formula's rows at +-64 ulps of each of the 255 row
    boundaries and on the special values (tests/golden/reference_scale_index_boundaries.npz), against the oracle on 10^6
    log-uniform scales in [1e-6, 1e3], and NaN to row 0."""
    from helpers import golden
    from pmctf_oracle import entropy
    from pMCTF.hip import ops
    g = entropy.GaussianTables()
    lmin, lstep = g.log_scale_min, g.log_scale_step
    d = golden("reference_scale_index_boundaries.npz")
    rnd = np.exp(_rng(11).uniform(np.log(1e-6), np.log(1e3), 10 ** 6)).astype(np.float32)
    sets = [("fixture", d["scale_x"], d["scale_row"].astype(np.int16)),
            ("log-uniform", rnd, g.build_indexes_cdef(torch.from_numpy(rnd)).numpy().astype(np.int16)),
            ("nan", np.full(64, np.nan, np.float32), np.zeros(64, np.int16))]
    for name, x, want in sets:
        n = x.size + (-x.size) % 32                           # whole rows of 16 (MV channels) x 2 (parity classes)
        s = np.concatenate([x, np.full(n - x.size, x[0], np.float32)])
        want = np.concatenate([want, np.full(n - x.size, want[0], np.int16)])
        sd = torch.from_numpy(s).cuda()
        # four-step sites: one plane of 2 x n/2, the four parity classes together cover every position
        H, W = 2, n // 2
        params = torch.stack([sd, torch.zeros_like(sd)], -1).view(1, H, W, 2).contiguous()
        x4 = torch.zeros(1, 1, H, W, device="cuda")
        got_i = torch.zeros(n, dtype=torch.int16, device="cuda")
        got_q = torch.zeros(n, dtype=torch.int16, device="cuda")
        for k in range(4):
            got_i += ops.fourstep_indexes(params, 1, H, W, k, lmin, lstep)
            sym = torch.zeros(n, dtype=torch.int16, device="cuda")
            idx = torch.zeros(n, dtype=torch.int16, device="cuda")
            ops.fourstep_quant(x4, params, torch.zeros_like(x4), sym, idx, 0, k, lmin, lstep)
            got_q += idx
        assert_same(got_i.cpu().numpy(), want, f"fourstep_indexes, {name}")
        assert_same(got_q.cpu().numpy(), want, f"fourstep_quant, {name}")
        sym = torch.zeros(n, dtype=torch.int16, device="cuda")
        idx = torch.zeros(n, dtype=torch.int16, device="cuda")
        ops.ll_quant(x4, params, sym, idx, 0, lmin, lstep)
        assert_same(idx.cpu().numpy(), want, f"ll_quant, {name}")
        # MV four-part sites: HW positions x 16 channels, scale of (p, cc) in all four channel groups; rows [16][HW]
        HW = n // 16
        sc = sd.view(HW, 1, 16).expand(HW, 4, 16).reshape(HW, 64)
        common = torch.cat([torch.ones(HW, 64, device="cuda"), sc, torch.zeros(HW, 64, device="cuda")], 1).contiguous()
        sp = torch.cat([sc, torch.zeros(HW, 64, device="cuda")], 1).contiguous()
        want_mv = want.reshape(HW, 16).T.reshape(-1)
        for t in range(4):
            got = ops.mv_fourpart_indexes(common, sp, 1, HW, t, lmin, lstep)
            assert_same(got.cpu().numpy(), want_mv, f"mv_fourpart_indexes t={t}, {name}")
        for t in range(4):
            y = torch.zeros(1, 1, HW, 64, device="cuda")
            sym = torch.zeros(16 * HW, dtype=torch.int16, device="cuda")
            idx = torch.zeros(16 * HW, dtype=torch.int16, device="cuda")
            ops.mv_fourpart_step(y, common, sp, torch.zeros(1, 1, HW, 64, device="cuda"), sym, idx, 0, t, lmin, lstep)
            assert_same(idx.cpu().numpy(), want_mv, f"mv_fourpart t={t}, {name}")


# ---- kernels that had no direct test, odd sizes, and one shape past the grid cap for every grid-stride kernel -----------
# Every grid-stride kernel of ew_ops.hip and basic_ops.hip caps its grid at 16384 workgroups of 256 threads (8192 for
# conv_smallcin_kernel): a launch with more work items than GRID_CAP makes every thread take a second trip of its loop.
GRID_CAP = 16384 * 256


def assert_bits(a, b, what):
    """every bit pattern equal, NaN payloads included"""
    assert_same(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32), what)


@pytest.mark.parametrize("hw", [(37, 53), (1, 7), (1152, 1920), (2100, 2000)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_spynet_pack8_is_the_concatenation(cuda, hw):
    """spynet_pack8 against torch.cat([im1 x3, warped x3, flow_up], 1) (video_net.py:116-119) in NHWC; odd sizes, the
    1080p level and one plane past the grid cap"""
    from pMCTF.hip import ops
    H, W = hw
    r = _rng(H + W)
    im1, wrp = (r.standard_normal((1, 1, H, W), dtype=np.float32) for _ in range(2))
    fu = r.standard_normal((1, 2, H, W), dtype=np.float32)
    want = np.concatenate([im1] * 3 + [wrp] * 3 + [fu], 1)
    got = ops.spynet_pack8(*(torch.from_numpy(a).cuda() for a in (im1, wrp, fu)))
    assert_bits(nchw(got), want, f"spynet_pack8 {H}x{W}")


@pytest.mark.parametrize("rule", [0, 1], ids=["chain", "blocks"])
@pytest.mark.parametrize("shape", [(1, 1, 2, 16), (2, 3, 2, 5), (1, 1, 37, 53), (2, 2, 16, 31), (1, 1, 2100, 2001)],
                         ids=lambda s: "x".join(map(str, s)))
def test_lift_skip3_bitexact(cuda, shape, rule):
    """lift_skip3 against the oracle's lifting skip filter (reflection pad of one row above and below, then the 3x1
    convolution under the same summation rule: oracle/pmctf_oracle/model.py lift_skip).  H = 2 (both reflections hit the
    same row), several planes, odd W, and a plane of more than 4.2 M elements (past the grid cap)."""
    from pmctf_oracle import clib
    from pMCTF.hip import ops
    n, c, H, W = shape
    r = _rng(H * W + rule)
    x = (r.standard_normal(shape, dtype=np.float32) * 50).astype(np.float32)
    w3 = r.standard_normal(3, dtype=np.float32)
    bias = np.float32(0.3125 + rule)
    xp = np.pad(x.reshape(n * c, 1, H, W), ((0, 0), (0, 0), (1, 1), (0, 0)), mode="reflect")
    want = clib.conv2d(xp, w3.reshape(1, 1, 3, 1), np.array([bias], np.float32), 1, (0, 0), rule).reshape(shape)
    got = ops.lift_skip3(torch.from_numpy(x).cuda(), w3, bias, rule)
    assert_bits(got.cpu().numpy(), want, f"lift_skip3 {shape} rule {rule}")


@pytest.mark.parametrize("shape", [(1, 5, 7, 6), (2, 9, 4, 64), (1, 1100, 1000, 8)], ids=lambda s: "x".join(map(str, s)))
def test_ffn3_mix_bitexact(cuda, shape):
    """ffn3_mix against leaky(x1, 0.1) + leaky(x2, 0.01) in float32 (video/layers.py:163-167), x = [x1 | x2] on the
    channels; zeros of both signs among the inputs; the last shape is past the grid cap"""
    from pMCTF.hip import ops
    n, h, w, c2 = shape
    r = _rng(h * w)
    x = (r.standard_normal(shape, dtype=np.float32) * 3).astype(np.float32)
    c = c2 // 2
    x[0, 0, 0, :] = np.float32(-0.0)                # -0 + -0 = -0
    x[0, 0, 1, :] = np.float32(0.0)                 # +0 + +0 = +0
    x[0, 0, 2, :c], x[0, 0, 2, c:] = np.float32(-0.0), np.float32(0.0)      # -0 + +0 = +0
    x[0, 0, 3, :c] = np.float32(-0.0)               # -0 + anything
    x1, x2 = x[..., :c], x[..., c:]
    want = np.where(x1 > 0, x1, x1 * np.float32(0.1)) + np.where(x2 > 0, x2, x2 * np.float32(0.01))
    assert (np.signbit(want) & (want == 0)).any() and (~np.signbit(want) & (want == 0)).any()
    got = ops.ffn3_mix(torch.from_numpy(x).cuda())
    assert n * h * w * c > GRID_CAP or shape[1] < 100
    assert_bits(got.cpu().numpy(), want.astype(np.float32), f"ffn3_mix {shape}")


@pytest.mark.parametrize("shape", [(3, 1, 37, 53), (3, 2, 36, 60), (3, 1, 1152, 1920)], ids=lambda s: "x".join(map(str, s)))
def test_flow_warp_one_flow_field_per_plane(cuda, shape):
    """flow_warp with flowN = N (one flow field per plane; test_flow_warp_bitexact shares one): N = 3, and at 1152x1920,
    where the three planes together are past the grid cap"""
    from pmctf_oracle import clib
    from pMCTF.hip import ops
    N, Cc, H, W = shape
    r = _rng(17)
    im = (r.random(shape, dtype=np.float32) * 255).astype(np.float32)
    flow = (r.standard_normal((N, 2, H, W), dtype=np.float32) * np.array([2, 6, 12], np.float32).reshape(3, 1, 1, 1)).astype(np.float32)
    flow[1, 0, 0, :] = 1000.0
    flow[2, 1, :, 0] = -1000.0
    lx = torch.linspace(-1.0, 1.0, W).numpy(); ly = torch.linspace(-1.0, 1.0, H).numpy()
    for sign in (1.0, -1.0):
        ref = clib.flow_warp(im, flow * np.float32(sign), lx, ly)
        assert not np.array_equal(ref[0], clib.flow_warp(im[:1], flow[1:2] * np.float32(sign), lx, ly)[0])
        out = ops.flow_warp(torch.from_numpy(im).cuda(), torch.from_numpy(flow).cuda(),
                            torch.from_numpy(lx).cuda(), torch.from_numpy(ly).cuda(), sign)
        assert_same(out.cpu().numpy(), ref, f"warp {shape} sign {sign}")


def test_resample_odd_sizes_and_tiny_planes(cuda):
    """avgpool2 and bilinear_down on odd H and odd W (the last row / column is dropped, as F.avg_pool2d and F.interpolate
    do); bilinear_up x2 / x4 / x8 on a 1x1 and a 1xW plane (every source index clamps); the factor-2 entry points"""
    import ctypes
    from pmctf_oracle import clib
    from pMCTF.hip import lib, ops
    r = _rng(23)
    for shape in ((2, 3, 37, 61), (1, 2, 36, 61), (1, 1, 37, 60), (1, 1, 3, 3), (1, 1, 9, 17)):
        x = (r.standard_normal(shape, dtype=np.float32) * 10).astype(np.float32)
        xt = torch.from_numpy(x).cuda()
        assert_same(ops.avgpool2(xt).cpu().numpy(), clib.avgpool2(x), f"avgpool2 {shape}")
        for f in (2, 4, 8):
            if shape[2] >= f and shape[3] >= f:
                assert_same(ops.bilinear_down2(xt, 1.0, f).cpu().numpy(), clib.bilinear_down(x, f), f"down /{f} {shape}")
    for shape in ((1, 1, 1, 1), (2, 1, 1, 1), (1, 2, 1, 13), (1, 1, 7, 1)):
        x = (r.standard_normal(shape, dtype=np.float32) * 10).astype(np.float32)
        xt = torch.from_numpy(x).cuda()
        for f in (2, 4, 8):
            assert_same(ops.bilinear_up2(xt, 1.0, f).cpu().numpy(), clib.bilinear_up(x, f), f"up x{f} {shape}")
    x = (r.standard_normal((1, 2, 9, 11), dtype=np.float32) * 10).astype(np.float32)        # pmctf_bilinear_{up,down}2_f32
    xt = torch.from_numpy(x).cuda()
    L, p = lib.hip(), lambda t: ctypes.c_void_p(t.data_ptr())
    up, dn = torch.empty(1, 2, 18, 22, device="cuda"), torch.empty(1, 2, 4, 5, device="cuda")
    assert L.pmctf_bilinear_up2_f32(p(xt), p(up), 2, 9, 11, 1.0, None) == 0
    assert L.pmctf_bilinear_down2_f32(p(xt), p(dn), 2, 9, 11, 1.0, None) == 0
    torch.cuda.synchronize()
    assert_same(up.cpu().numpy(), clib.bilinear_up2(x), "pmctf_bilinear_up2_f32")
    assert_same(dn.cpu().numpy(), clib.bilinear_down2(x), "pmctf_bilinear_down2_f32")


def test_grid_stride_kernels_past_the_grid_cap(cuda):
    """One shape with more work items than the grid cap for the remaining grid-stride kernels: nearest_up2 and
    pixel_shuffle2 (scalar and 16-byte forms), avgpool2, bilinear_up, bilinear_down, the generic depthwise kernel.
    (The depthwise strip kernel cannot get there: from 262 144 column threads on, an eighth of the strip threads, the
    column-walking kernel takes the layer; that one would need operands of 2.1 GB, and is not run past its cap.)"""
    import torch.nn.functional as F
    from pmctf_oracle import clib
    from pMCTF.hip import ops
    r = _rng(31)
    for (n, c, h, w) in ((1, 3, 600, 600), (1, 8, 1500, 1400)):                # scalar: 4nhwc items; vec4: nhwc/4
        assert (4 * n * h * w * c if c % 4 else n * h * w * c // 4) > GRID_CAP
        x = r.standard_normal((n, c, h, w), dtype=np.float32)
        assert_same(nchw(ops.nearest_up2(nhwc(x))), F.interpolate(torch.from_numpy(x), scale_factor=2, mode="nearest").numpy(),
                    f"nearest_up2 {(n, c, h, w)}")
    for (n, c, h, w) in ((1, 3, 600, 600), (1, 4, 2100, 2000)):
        assert (4 * n * h * w * c if c % 4 else n * h * w * c // 4) > GRID_CAP
        x4 = r.standard_normal((n, 4 * c, h, w), dtype=np.float32)
        want = F.leaky_relu(F.pixel_shuffle(torch.from_numpy(x4), 2), 0.1).numpy()
        assert_same(nchw(ops.pixel_shuffle2(nhwc(x4), act=ops.ACT_LEAKY, slope=0.1)), want, f"pixel_shuffle2 {(n, c, h, w)}")
    x = (r.standard_normal((1, 2, 3000, 3001), dtype=np.float32) * 10).astype(np.float32)
    xt = torch.from_numpy(x).cuda()
    assert 2 * 1500 * 1500 > GRID_CAP
    assert_same(ops.avgpool2(xt).cpu().numpy(), clib.avgpool2(x), "avgpool2 past the cap")
    assert_same(ops.bilinear_down2(xt, 1.0, 2).cpu().numpy(), clib.bilinear_down(x, 2), "bilinear_down past the cap")
    x = (r.standard_normal((1, 1, 1100, 1000), dtype=np.float32) * 10).astype(np.float32)
    assert 4 * x.size > GRID_CAP
    assert_same(ops.bilinear_up2(torch.from_numpy(x).cuda(), 1.0, 2).cpu().numpy(), clib.bilinear_up(x, 2), "bilinear_up past the cap")
    shape = (1, 6, 900, 800)                                                   # C % 4 != 0: the generic depthwise kernel
    assert np.prod(shape) > GRID_CAP
    x = r.standard_normal(shape, dtype=np.float32)
    w = r.standard_normal((6, 1, 3, 3), dtype=np.float32)
    b = r.standard_normal(6, dtype=np.float32)
    assert_same(nchw(ops.DepthwiseConv2d(torch.from_numpy(w), torch.from_numpy(b))(nhwc(x))), clib.dwconv2d(x, w, b),
                "generic dwconv past the cap")


@pytest.mark.parametrize("case", [
    # N, Cin, H, W, Cout, K, act, rule, work items, cap
    (1, 4, 540, 500, 8, 3, 2, 0, 540 * 500 * 8, 8192 * 256),          # conv_smallcin_kernel (Cin = 4): one thread per output
    (1, 2, 600, 500, 16, 3, 0, 1, 600 * 500 // 16, 16384),            # conv_smallcin_reg_kernel: 256 / Cout pixels per workgroup
    (1, 1, 2100, 2048, 32, 3, 3, 1, 2100 * 32 // 4, 16384),           # strip kernel: four 64-pixel strips per workgroup
    (1, 16, 2100, 2000, 1, 3, 0, 1, 263 * 63, 16384),                 # few-cout kernel 16 -> 1: one workgroup per 8x32 tile
    (1, 16, 2100, 2000, 2, 7, 0, 0, 263 * 63, 16384),                 # few-cout kernel 16 -> 2, 7x7
], ids=["smallcin", "smallcin_reg", "smallcin_strip", "fewcout_16_1", "fewcout_16_2_k7"])
def test_small_convolutions_past_the_grid_cap(cuda, case):
    """the vector-ALU convolutions on planes with more workgroups than their grid cap (few-cout: more 8x32 tiles than the
    other kernels' cap; its LDS form launches one workgroup per tile), against the oracle"""
    from pmctf_oracle import clib
    from pMCTF.hip import ops
    n, cin, h, w, cout, k, act, rule, items, cap = case
    assert items > cap
    r = _rng(cin * cout)
    x = r.standard_normal((n, cin, h, w), dtype=np.float32)
    wt = (r.standard_normal((cout, cin, k, k), dtype=np.float32) * 0.2).astype(np.float32)
    b = r.standard_normal(cout, dtype=np.float32)
    conv = ops.Conv2d(torch.from_numpy(wt), torch.from_numpy(b), 1, (k // 2, k // 2), rule=rule)
    assert conv.small or conv.few
    ref = clib.conv2d(x, wt, b, 1, (k // 2, k // 2), rule)
    if act == 2:
        ref = np.where(ref > 0, ref, ref * np.float32(0.1)).astype(np.float32)
    elif act == 3:
        ref = clib.tanh(ref)
    assert_same(nchw(conv(nhwc(x), act, 0.1)), ref, f"conv {case}")


def test_conv3x3_cin1_dual_past_the_grid_cap(cuda):
    """PredictUpdate conv1 with its tanh copy on a plane of more than 4.2 M pixels"""
    from pmctf_oracle import clib
    from pMCTF.hip import ops
    r = _rng(41)
    H, W = 2100, 2001
    assert H * W > GRID_CAP
    x = r.standard_normal((1, 1, H, W), dtype=np.float32)
    wt = (r.standard_normal((16, 1, 3, 3), dtype=np.float32) * 0.3).astype(np.float32)
    b = r.standard_normal(16, dtype=np.float32)
    conv = ops.Conv2d(torch.from_numpy(wt), torch.from_numpy(b), 1, (1, 1), rule=1)
    y, y2 = ops.conv3x3_cin1_dual(conv, nhwc(x), ops.ACT_TANH)
    ref = clib.conv2d(x, wt, b, 1, (1, 1), 1)
    assert_same(nchw(y), ref, "conv1")
    assert_same(nchw(y2), clib.tanh(ref), "tanh(conv1)")


def test_lstm_gates_without_aten_tails(cuda):
    """lstm_gates with aten_threads = 0 (test_lstm_gates_with_aten_thread_tails runs 8): SLEEF's sigmoid on every element,
    one cell plane broadcast over the channels or one per channel; the last shape is past the grid cap"""
    from pmctf_oracle import clib
    from pMCTF.hip import ops
    rng = _rng(78)
    for (n, c, h, w, cc) in ((2, 3, 144, 240, 1), (1, 32, 36, 60, 32), (1, 8, 800, 700, 1)):
        x = (rng.standard_normal((n, c, h, w)) * 3).astype(np.float32)
        cell = rng.standard_normal((n, cc, h, w)).astype(np.float32)
        g = clib.sigmoid(x)
        cn = g * cell + g * clib.tanh(x)
        hid = g * clib.tanh(np.ascontiguousarray(cn))
        got_h, got_c = ops.lstm_gates(nhwc(x), nhwc(cell), aten_threads=0)
        assert_same(nchw(got_h), hid, f"hidden {(n, c, h, w, cc)}")
        assert_same(nchw(got_c), cn, f"cell {(n, c, h, w, cc)}")
    assert 8 * 800 * 700 > GRID_CAP


@pytest.mark.parametrize("cin", [1, 16], ids=["smallcin", "mfma"])
def test_relu_epilogue_is_torch_relu_on_nan_and_negative_zero(cuda, cin):
    """the relu of the convolution epilogues (conv_epilogue.h act_c, pm::apply_act) is torch.relu bit for bit: a NaN stays a
    NaN and -0 stays -0 (max(0, v) as ATen's CPU kernel takes it).  A 1x1 layer that hands channel 0 through — weight 1 on
    it, +0 on the others, whose inputs are -0, bias -0, so that every product and the sum of a -0 input are -0 — against
    torch.relu of the oracle's convolution."""
    import math_sweep as ms
    from pmctf_oracle import clib
    from pMCTF.hip import ops
    H, W, cout = 8, 16, 16
    x = np.full((1, cin, H, W), -0.0, np.float32)
    x[0, 0] = _rng(5).standard_normal((H, W), dtype=np.float32)
    x[0, 0, 0, :6] = np.array([0x80000000, 0x00000000, 0x7fc00000, 0xffc00001, 0x80000001, 0xff800000], np.uint32).view(np.float32)
    wt = np.zeros((cout, cin, 1, 1), np.float32)
    wt[:, 0] = 1.0
    b = np.full(cout, -0.0, np.float32)
    conv = ops.Conv2d(torch.from_numpy(wt), torch.from_numpy(b), 1, (0, 0), rule=0)
    assert conv.small == (cin == 1) and not conv.few
    pre = clib.conv2d(x, wt, b, 1, (0, 0), 0)
    assert np.signbit(pre[0, 0, 0, 0]) and pre[0, 0, 0, 0] == 0 and np.isnan(pre[0, :, 0, 2:4]).all()
    want = torch.relu(torch.from_numpy(pre)).numpy()
    assert want.view(np.uint32)[0, 0, 0, 0] == 0x80000000 and np.isnan(want[0, :, 0, 2:4]).all()
    got = np.ascontiguousarray(nchw(conv(nhwc(x), ops.ACT_RELU, 0.0)))
    count, first, _ = ms.compare(got.reshape(-1), want.reshape(-1))
    assert count == 0, ms.describe("relu epilogue", np.arange(got.size), got.reshape(-1), want.reshape(-1), count, first)
