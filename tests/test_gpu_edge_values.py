"""flow_warp, avgpool2, bilinear_up / _down, lstm_gates and the copy kernels against the oracle on the edge data of
edge_values.py, as bit patterns (NaN payloads of computed results exempt, math_sweep.compare; copies carry every pattern
through unchanged).  Every output is written through the C entry into the middle of a sentinel-filled buffer, and the
sentinels on both sides must be intact.  test_oracle_ops.py ties the oracle's side to the torch operations."""
import ctypes

import numpy as np
import pytest
import torch

import edge_values as ev
import math_sweep as ms

pytestmark = pytest.mark.gpu

PAD = 64                    # sentinel words on either side of an output (256 bytes: the output stays 16-byte aligned)
SENT = 0x5A5A5A5A


def _ids(s):
    return "x".join(map(str, s))


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded:
    """n float32 (or, with itemsize 1, 4 * ceil(n / 4) bytes) in the middle of a sentinel-filled buffer"""

    def __init__(self, n, itemsize=4):
        self.words = n if itemsize == 4 else (n + 3) // 4
        self.buf = torch.full((self.words + 2 * PAD,), SENT, dtype=torch.int32, device="cuda")
        mid = self.buf[PAD:PAD + self.words]
        self.out = mid.view(torch.float32) if itemsize == 4 else mid.view(torch.uint8)

    def result(self, shape, what):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        assert (b[:PAD] == SENT).all() and (b[PAD + self.words:] == SENT).all(), f"{what}: wrote outside its output"
        mid = b[PAD:PAD + self.words]
        return mid.view(np.float32).reshape(shape) if shape is not None else mid

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf.cpu().numpy() == SENT).all())


@pytest.mark.parametrize("shape", ev.WARP_PLANES, ids=_ids)
def test_flow_warp_edge_values(cuda, shape):
    """both images x every flow kind x one shared flow field / one per plane x both signs.  Non-finite positions clamp into
    the image before the cast (fmaxf(NaN, 0) = 0), as test_edge_values_cpu.py asserts on the coordinates."""
    from pmctf_oracle import clib
    from pMCTF.hip import lib
    N, Cc, H, W = shape
    L = lib.hip()
    lx, ly = ev.lin_tables(H, W)
    dlx, dly = _dev(lx), _dev(ly)
    for iname, image in ev.IMAGES.items():
        im = image(shape)
        dim = _dev(im)
        for kind in ev.FLOWS:
            for fn in sorted({1, N}):
                fl = ev.flow(kind, fn, H, W)
                dfl = _dev(fl)
                for sign in (1.0, -1.0):
                    want = clib.flow_warp(im, fl * np.float32(sign), lx, ly)
                    g = Guarded(im.size)
                    assert L.pmctf_flow_warp_f32(_p(dim), _p(dfl), _p(dlx), _p(dly), _p(g.out), N, Cc, H, W, fn, sign, None) == 0
                    what = f"flow_warp {shape} {iname} image, {kind} flow, {fn} field(s), sign {sign}"
                    ev.bits_equal(g.result(shape, what), want, what)


@pytest.mark.parametrize("shape", ev.WARP_DEGENERATE, ids=_ids)
def test_flow_warp_refuses_one_row_and_one_column(cuda, shape):
    """(W - 1) / 2 or (H - 1) / 2 is 0 on these planes: the entry refuses them and writes nothing (the oracle and
    F.grid_sample agree on them, test_oracle_ops.py; the codec never warps such a plane)"""
    from pMCTF.hip import lib
    N, Cc, H, W = shape
    lx, ly = ev.lin_tables(H, W)
    g = Guarded(N * Cc * H * W)
    im, fl, dlx, dly = _dev(ev.pixel(shape)), _dev(ev.flow("normal", 1, H, W)), _dev(lx), _dev(ly)
    rc = lib.hip().pmctf_flow_warp_f32(_p(im), _p(fl), _p(dlx), _p(dly), _p(g.out), N, Cc, H, W, 1, 1.0, None)
    assert rc == -1 and g.untouched()


@pytest.mark.parametrize("shape", ev.RESAMPLE_SHAPES + ev.UP_ONLY_SHAPES, ids=_ids)
def test_resampling_edge_values(cuda, shape):
    """avgpool2, bilinear_up x2 / x4 / x8 (also times the factor, as the path scales flow fields) and bilinear_down /2 / /4 / /8
    (also divided by 2) on the quantised, the subnormal and the +-inf / NaN island planes"""
    from pmctf_oracle import clib
    from pMCTF.hip import lib
    N, Cc, H, W = shape
    L = lib.hip()
    for name, data in ev.RESAMPLE_DATA.items():
        x = data(shape)
        dx = _dev(x)
        if H >= 2 and W >= 2:
            want = clib.avgpool2(x)
            g = Guarded(want.size)
            assert L.pmctf_avgpool2_f32(_p(dx), _p(g.out), N * Cc, H, W, None) == 0
            ev.bits_equal(g.result(want.shape, "avgpool2"), want, f"avgpool2 {shape} {name}")
        for f in (2, 4, 8):
            for scale in (1.0, float(f)):
                with np.errstate(all="ignore"):
                    want = clib.bilinear_up(x, f) * np.float32(scale)
                g = Guarded(want.size)
                assert L.pmctf_bilinear_up_f32(_p(dx), _p(g.out), N * Cc, H, W, f, scale, None) == 0
                ev.bits_equal(g.result(want.shape, "bilinear_up"), want, f"bilinear_up x{f} times {scale} {shape} {name}")
            if H >= f and W >= f:
                for div in (1.0, 2.0):
                    with np.errstate(all="ignore"):
                        want = clib.bilinear_down(x, f) / np.float32(div)
                    g = Guarded(want.size)
                    assert L.pmctf_bilinear_down_f32(_p(dx), _p(g.out), N * Cc, H, W, f, div, None) == 0
                    ev.bits_equal(g.result(want.shape, "bilinear_down"), want, f"bilinear_down /{f} over {div} {shape} {name}")


def test_avgpool2_never_gives_minus_zero(cuda):
    """the windows of edge_values.minus_zero_windows: four -0, and a negative sum whose quarter underflows, give +0 as in
    F.avg_pool2d (test_oracle_ops.py); also the all -0 and mixed-sign windows planted in the quantised plane"""
    from pmctf_oracle import clib
    from pMCTF.hip import lib
    x, want = ev.minus_zero_windows()
    g, dx = Guarded(want.size), _dev(x)
    assert lib.hip().pmctf_avgpool2_f32(_p(dx), _p(g.out), 1, 4, 6, None) == 0
    ev.bits_equal(g.result(want.shape, "avgpool2"), want, "avgpool2 on windows of -0")
    q = ev.quantised((2, 3, 36, 60))
    g, dq = Guarded(q.size // 4), _dev(q)
    assert lib.hip().pmctf_avgpool2_f32(_p(dq), _p(g.out), 6, 36, 60, None) == 0
    got = g.result((2, 3, 18, 30), "avgpool2")
    assert (got[..., 0, 0:2].view(np.uint32) == 0).all()
    ev.bits_equal(got, clib.avgpool2(q), "avgpool2 on the quantised plane")


@pytest.mark.parametrize("threads", [0, 8], ids=["sleef", "aten8"])
@pytest.mark.parametrize("shape", ev.LSTM_SHAPES, ids=_ids)
def test_lstm_gates_edge_values(cuda, shape, threads):
    """xh from the special set (sigmoid and tanh of +-0, +-inf, NaN, the largest float, subnormals) and normals; cell with
    +-0 and +-inf, so that 0 * inf and inf - inf occur: against the oracle's maps and numpy's float32 algebra"""
    from pmctf_oracle import clib
    from pMCTF.hip import lib
    n, c, h, w, cc = shape
    xh, cell = ev.lstm_data(shape)
    with np.errstate(all="ignore"):
        g_ = clib.sigmoid(xh, threads) if threads else clib.sigmoid(xh)
        cn = g_ * cell + g_ * clib.tanh(xh)
        hid = g_ * clib.tanh(np.ascontiguousarray(cn))
    assert np.isnan(cn).any() and np.isinf(cn).any() and all(ev.zero_signs(cn))
    to_nhwc = lambda a: _dev(a.transpose(0, 2, 3, 1))
    gc, gh = Guarded(xh.size), Guarded(xh.size)
    dxh, dcell = to_nhwc(xh), to_nhwc(cell)
    rc = lib.hip().pmctf_lstm_gates_aten_f32(_p(dxh), _p(dcell), _p(gc.out), _p(gh.out), n * h * w, c, cc, h * w, n, threads,
                                             None)
    assert rc == 0
    back = lambda g, what: g.result((n, h, w, c), what).transpose(0, 3, 1, 2)
    ev.bits_equal(back(gc, "cell"), np.ascontiguousarray(cn), f"lstm_gates cell {shape}")
    ev.bits_equal(back(gh, "hidden"), np.ascontiguousarray(hid), f"lstm_gates hidden {shape}")


def _same_patterns(got, want, what):
    got, want = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} patterns changed; first at {tuple(bad[0])}: {int(got[tuple(bad[0])]):#010x}"


@pytest.mark.parametrize("c", [3, 8], ids=["scalar", "vec4"])
def test_copy_kernels_carry_every_pattern(cuda, c):
    """nearest_up2 and pixel_shuffle2 without activation, scalar and 16-byte forms, and spynet_pack8: every special pattern,
    NaN payloads and the sign of a zero included, arrives unchanged; pixel_shuffle2 with an activation is apply_act of the
    pattern (math_sweep.SPEC: torch.relu, the leaky restatement, the oracle's tanh and sigmoid)"""
    from pMCTF.hip import lib, ops
    L = lib.hip()
    n, h, w = 2, 5, 7
    x = ev.specials_plane((n, h, w, c))
    assert set(ev.SPECIALS.view(np.uint32).tolist()) <= set(x.view(np.uint32).reshape(-1).tolist())
    g, dx = Guarded(4 * x.size), _dev(x)
    assert L.pmctf_nearest_up2_nhwc_f32(_p(dx), _p(g.out), n, h, w, c, None) == 0
    _same_patterns(g.result((n, 2 * h, 2 * w, c), "nearest_up2"), x.repeat(2, axis=1).repeat(2, axis=2), f"nearest_up2 C={c}")
    x4 = ev.specials_plane((n, h, w, 4 * c), seed=8)
    shuffled = x4.reshape(n, h, w, c, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(n, 2 * h, 2 * w, c)
    acts = [(ops.ACT_NONE, None), (ops.ACT_RELU, "act_relu"), (ops.ACT_LEAKY, "act_leaky"), (ops.ACT_TANH, "act_tanh"),
            (ops.ACT_SIGMOID, "act_sigmoid")]
    dx4 = _dev(x4)
    for act, spec in acts:
        g = Guarded(x4.size)
        assert L.pmctf_pixel_shuffle2_nhwc_f32(_p(dx4), _p(g.out), n, h, w, c, act, ms.LEAKY_SLOPE, None) == 0
        got = g.result(shuffled.shape, "pixel_shuffle2")
        if spec is None:
            _same_patterns(got, shuffled, f"pixel_shuffle2 C={c}")
        else:
            want = ms.SPEC[spec](np.ascontiguousarray(shuffled).reshape(-1)).reshape(shuffled.shape)
            ev.bits_equal(got, want, f"pixel_shuffle2 C={c} {spec}")
    if c == 3:
        H, W = 5, 13
        im1, wrp = ev.specials_plane((1, 1, H, W), seed=9), ev.specials_plane((1, 1, H, W), seed=10)
        fu = ev.specials_plane((1, 2, H, W), seed=11)
        g, dev = Guarded(8 * H * W), [_dev(a) for a in (im1, wrp, fu)]
        assert L.pmctf_spynet_pack8_f32(_p(dev[0]), _p(dev[1]), _p(dev[2]), _p(g.out), H, W, None) == 0
        want = np.concatenate([im1] * 3 + [wrp] * 3 + [fu], 1).transpose(0, 2, 3, 1)
        _same_patterns(g.result((1, H, W, 8), "spynet_pack8"), want, "spynet_pack8")


@pytest.mark.parametrize("hw", [(3, 5), (4, 8)], ids=_ids)
def test_planes_to_u8_bytes_of_the_special_patterns(cuda, hw):
    """each pattern to its documented byte: rint(clamp(x, 0, 255)), ties to even, NaN to 0; a byte count that is and is not a
    multiple of four (the last bytes are written one by one)"""
    from pMCTF.hip import lib
    h, w = hw
    Hp, Wp = h + 2, w + 3
    vals = np.array([v for v, _ in ev.U8_PATTERNS], np.float32)
    byte = np.array([b for _, b in ev.U8_PATTERNS], np.uint8)
    pick = np.arange(2 * h * w) % vals.size
    x = np.full((2, Hp, Wp), 77.0, np.float32)
    x[:, :h, :w] = vals[pick].reshape(2, h, w)
    g, dx = Guarded(2 * h * w, itemsize=1), _dev(x)
    assert lib.hip().pmctf_planes_to_u8(_p(dx), _p(g.out), 2, Hp, Wp, h, w, None) == 0
    got = g.result(None, "planes_to_u8").view(np.uint8)
    assert (got[:2 * h * w] == byte[pick]).all(), (got[:2 * h * w], byte[pick])
    assert (got[2 * h * w:] == 0x5A).all(), "bytes past the last pixel were written"
