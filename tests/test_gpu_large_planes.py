"""The rows of large_planes.py on the GPU: byte offsets inside an image at and past 2^31 and 2^32, the size guards of the
dispatchers from both sides, the batch axis past 2^32.  Per row: the input is made on the device from a seeded generator and
never copied whole to the host; the output lies inside a larger buffer between 64 sentinel words on either side and is
prefilled with the sentinel; the launch key is asserted; the sentinels are checked on the device (both pads intact, no
output element left unwritten); windows of the input and of the output (the corners, the pixels at the 2^31 and k * 2^32
byte offsets of either operand, the last pixel, eight random ones) are copied to the host and compared with the oracle as
uint32 patterns; and the WHOLE output is compared, on the device, with the same operation recomputed in horizontal bands
of less than 2^31 bytes each, every band its own allocation with its halo rows (how work is cut never changes a sum, and the
bands are the regime the other censuses verify).  A row skips only when the device shows less free memory than the table
states for it; on an MI355X none may."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_census as cc
import ew_census as ec
import large_planes as lp

pytestmark = pytest.mark.gpu

CHUNK = 1 << 28                 # elements per piece of the chunked fills and comparisons (1 GiB)


def _normal(shape, gen, scale=1.0):
    """a device tensor of independent normal values x scale, filled in pieces of CHUNK elements from the row's generator"""
    t = torch.empty(shape, dtype=torch.float32, device="cuda")
    flat = t.view(-1)
    for i in range(0, flat.numel(), CHUNK):
        flat[i:i + CHUNK].normal_(0.0, float(scale), generator=gen)
    return t


def _guarded(shape):
    """(int32 buffer of PAD + n + PAD sentinel words, the float32 view of the n words in the middle)"""
    n = int(np.prod(shape))
    buf = torch.empty(n + 2 * lp.PAD, dtype=torch.int32, device="cuda")
    for i in range(0, buf.numel(), CHUNK):
        buf[i:i + CHUNK].fill_(lp.SENT)
    return buf, buf[lp.PAD:lp.PAD + n].view(torch.float32).view(shape)


def _check_sentinels(buf, what):
    assert bool((buf[:lp.PAD] == lp.SENT).all()) and bool((buf[-lp.PAD:] == lp.SENT).all()), f"{what}: wrote outside the output"
    body = buf[lp.PAD:-lp.PAD]
    for i in range(0, body.numel(), CHUNK):
        left = int((body[i:i + CHUNK] == lp.SENT).sum())
        assert left == 0, f"{what}: {left} output elements in [{i}, {i + CHUNK}) were never written"


def _same_bits(got, want, what, base, r):
    """two contiguous device tensors of one shape as int32, in pieces; base: flat index of got[0] inside the large output"""
    a, b = got.reshape(-1).view(torch.int32), want.reshape(-1).view(torch.int32)
    assert a.numel() == b.numel(), what
    for i in range(0, a.numel(), CHUNK):
        if not torch.equal(a[i:i + CHUNK], b[i:i + CHUNK]):
            ne = (a[i:i + CHUNK] != b[i:i + CHUNK])
            first = i + int(ne.nonzero()[0])
            where, byte = lp.first_difference(base + first, r)
            raise AssertionError(f"{what}: {int(ne.sum())} elements of this piece differ from the band run; first at (n, y, x, c) = "
                                 f"{where}, byte offset {byte:#x}: {float(got.reshape(-1)[first])!r} vs {float(want.reshape(-1)[first])!r}")


def _host_bits(a, b, what):
    a, b = (np.ascontiguousarray(v, dtype=np.float32) for v in (a, b))
    assert a.shape == b.shape, (what, a.shape, b.shape)
    ne = a.view(np.uint32) != b.view(np.uint32)
    if ne.any():
        i = tuple(np.argwhere(ne)[0])
        raise AssertionError(f"{what}: {int(ne.sum())}/{a.size} bit patterns differ from the oracle; first at window (y, x, c) = {i}: "
                             f"{a[i]!r} ({a.view(np.uint32)[i]:#010x}) vs {b[i]!r} ({b.view(np.uint32)[i]:#010x})")


class Knobs:
    def __init__(self, knobs):
        from pMCTF.hip import lib
        self.L, self.knobs = lib.hip(), knobs

    def __enter__(self):
        self.saved = {k: self.L.pmctf_conv2d_get_option(k.encode()) for k in cc.KNOBS}
        for k, v in {**cc.KNOBS, **self.knobs}.items():
            assert self.L.pmctf_conv2d_set_option(k.encode(), v) == 0, k

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            self.L.pmctf_conv2d_set_option(k.encode(), v)


def _conv_launch(L):
    buf = C.create_string_buffer(512)
    assert L.pmctf_conv2d_last_launch(buf, 512) == 0
    return cc.parse_launch(buf.value.decode())


class Op:
    """a row's operation: run(x, res, out, extra) on device NHWC tensors of any height -> what it launched"""

    def __init__(self, r):
        from pMCTF.hip import lib, ops
        self.r, self.L, self.ops = r, lib.hip(), ops
        rid, entry, g, rule, act, nres, knobs, expected, boundary, side = r
        N, Cin, H, W, Cout, K, S, pad = g[:8]
        self.w, self.b = lp.weights(r)
        if entry in ("conv", "conv_geom", "smallcin", "fewcout"):
            p = 1 if entry == "conv_geom" else pad
            self.conv = ops.Conv2d(torch.from_numpy(self.w), torch.from_numpy(self.b), 1 if entry == "conv_geom" else S, (p, p), rule=rule)
            assert (self.conv.small, self.conv.few) == (entry == "smallcin", entry == "fewcout") and not self.conv.split
        elif entry == "dw":
            self.conv = ops.DepthwiseConv2d(torch.from_numpy(self.w), torch.from_numpy(self.b))

    def out_rows(self, rows_in):
        N, Cin, H, W, Cout, K, S, pad = self.r[2][:8]
        if self.r[1] in ("nearest_up2", "pixel_shuffle2"):
            return 2 * rows_in
        if self.r[1] == "conv_geom":
            return (rows_in + pad) // 2          # rows whose first tap lies inside or on the padding above
        return (rows_in + 2 * pad - K) // S + 1

    def run(self, x, res, out, extra=None, out2=None):
        r, ops, L = self.r, self.ops, self.L
        entry, act, pad = r[1], r[4], r[2][7]
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        r1, r2 = (res + [None, None])[:2]
        if entry in ("conv", "smallcin", "fewcout"):
            self.conv(x, act=act, slope=lp.SLOPE, res1=r1, res2=r2, out=out)
            return _conv_launch(L) if entry == "conv" else ops.valu_conv_last_launch().rpartition(" grid ")[0]
        if entry == "conv_geom":
            N, H, W, Cin = x.shape
            assert tuple(out.shape) == (N, out.shape[1], W // 2, self.conv.Cout) and x.is_contiguous() and out.is_contiguous()
            rc = L.pmctf_conv2d_nhwc_geom_opts_f32(p(x), p(self.conv.w), p(self.conv.b), p(r1), p(r2), p(out), N, H, W, Cin, self.conv.Cout,
                                                   3, 3, 2, pad, pad, out.shape[1], W // 2, int(act), float(lp.SLOPE), self.conv.rule,
                                                   ops._opts(), ops._stream())
            assert rc == 0, rc
            return _conv_launch(L)
        if entry == "dw":
            self.conv(x, out=out)
            return ops.valu_conv_last_launch().rpartition(" grid ")[0]
        N, H, W, Cin = x.shape
        assert x.is_contiguous() and out.is_contiguous()
        if entry == "nearest_up2":
            assert L.pmctf_nearest_up2_nhwc_f32(p(x), p(out), N, H, W, Cin, ops._stream()) == 0
            return ops.ew_last_launch().rpartition(" grid ")[0]
        if entry == "pixel_shuffle2":
            assert L.pmctf_pixel_shuffle2_nhwc_f32(p(x), p(out), N, H, W, Cin // 4, 0, 0.0, ops._stream()) == 0
            return ops.ew_last_launch().rpartition(" grid ")[0]
        if entry == "ffn3_mix":
            assert L.pmctf_ffn3_mix_f32(p(x), p(out), N * H * W, Cin // 2, ops._stream()) == 0
            return None
        if entry == "lstm_gates":
            assert extra.is_contiguous() and out2.is_contiguous()
            assert L.pmctf_lstm_gates_f32(p(x), p(extra), p(out2), p(out), N * H * W, Cin, Cin, ops._stream()) == 0
            return None
        raise KeyError(entry)


def _skip_unless_memory(r):
    torch.cuda.empty_cache()                    # what earlier tests of the process left in torch's cache is free memory too
    free, _ = torch.cuda.mem_get_info()
    need = lp.need_bytes(r)
    if free < need:
        pytest.skip(f"{r[0]} needs {need / 2 ** 30:.1f} GiB of device memory, {free / 2 ** 30:.1f} GiB are free")


def _window_to_host(t, n, y0, x0, h, w):
    """rows [y0, y0 + h) x columns [x0, x0 + w) of image n of an (N, H, W, C) device tensor, zeros outside the image"""
    N, H, W, Cc = t.shape
    out = np.zeros((h, w, Cc), np.float32)
    a, b, c, d = max(y0, 0), min(y0 + h, H), max(x0, 0), min(x0 + w, W)
    if b > a and d > c:
        out[a - y0:b - y0, c - x0:d - x0] = t[n, a:b, c:d].cpu().numpy()
    return out


ROWS = [r[0] for r in lp.ROWS if r[1] != "ew" and r[1] not in lp.FOURSTEP]
FOURSTEP_ROWS = [r[0] for r in lp.ROWS if r[1] in lp.FOURSTEP]
EW_ROWS = [r[0] for r in lp.ROWS if r[1] == "ew"]


@pytest.mark.parametrize("rid", ROWS)
def test_large_plane_row(cuda, rid):
    r = lp.row(rid)
    rid, entry, g, rule, act, nres, knobs, expected, boundary, side = r
    _skip_unless_memory(r)
    N, Cin, H, W, Cout, K, S, pad = g[:8]
    Ho, Wo, Co = lp.out_dims(r)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(lp.seed(rid))
    op = Op(r)
    x = _normal((N, H, W, Cin), gen, 3.0)
    res = [_normal((N, Ho, Wo, Co), gen) for _ in range(nres)]
    extra = _normal((N, H, W, Cin), gen) if entry == "lstm_gates" else None
    buf, y = _guarded((N, Ho, Wo, Co))
    buf2, y2 = _guarded((N, Ho, Wo, Co)) if entry == "lstm_gates" else (None, None)
    with Knobs(knobs):
        launched = op.run(x, res, y, extra, y2)
        torch.cuda.synchronize()
        assert launched == expected, f"{rid}: expected {expected}, launched {launched}"
        _check_sentinels(buf, rid)
        if buf2 is not None:
            _check_sentinels(buf2, rid + " (cell)")
        # ---- windows against the oracle
        for win in lp.windows(r):
            what, n, oy0, ox0, h, wd = win
            iy0, ix0, ih, iw = lp.input_window(r, win)
            xw = _window_to_host(x, n, iy0, ix0, ih, iw)
            rw = [_window_to_host(q, n, oy0, ox0, h, wd) for q in res]
            ew = None if extra is None else _window_to_host(extra, n, oy0, ox0, h, wd)
            want = lp.window_reference(r, win, xw, op.w, op.b, rw, ew)
            if entry == "lstm_gates":
                _host_bits(_window_to_host(y, n, oy0, ox0, h, wd), want[0], f"{rid} hidden, {what} at ({n}, {oy0}, {ox0})")
                _host_bits(_window_to_host(y2, n, oy0, ox0, h, wd), want[1], f"{rid} cell, {what} at ({n}, {oy0}, {ox0})")
            else:
                _host_bits(_window_to_host(y, n, oy0, ox0, h, wd), want, f"{rid}, {what} at ({n}, {oy0}, {ox0})")
        # ---- the whole output against bands of less than 2^31 bytes
        up = 2 if entry in ("nearest_up2", "pixel_shuffle2") else 1
        for n, o0, o1, i0, i1 in lp.bands(r):
            xb = x[n:n + 1, i0:i1].clone()
            assert xb.numel() * 4 < lp.G31 and xb.data_ptr() != x.data_ptr()
            first = i0 * up // S if entry != "dw" else i0            # the large run's row of the band's output row 0
            rows = op.out_rows(i1 - i0)
            assert first + rows >= o1 and first <= o0, (rid, n, o0, o1, i0, i1, first, rows)
            rb = [q[n:n + 1, first:first + rows].clone() for q in res]
            eb = None if extra is None else extra[n:n + 1, i0:i1].clone()
            yb = torch.empty((1, rows, Wo, Co), dtype=torch.float32, device="cuda")
            yb2 = torch.empty_like(yb) if y2 is not None else None
            op.run(xb, rb, yb, eb, yb2)
            base = ((n * Ho + o0) * Wo) * Co
            _same_bits(y[n, o0:o1], yb[0, o0 - first:o1 - first], f"{rid} rows [{o0}, {o1}) of image {n}", base, r)
            if y2 is not None:
                _same_bits(y2[n, o0:o1], yb2[0, o0 - first:o1 - first], f"{rid} cell rows [{o0}, {o1}) of image {n}", base, r)
            del xb, rb, eb, yb, yb2
    del x, res, extra, buf, y, buf2, y2
    torch.cuda.empty_cache()


@pytest.mark.parametrize("rid", EW_ROWS)
def test_large_elementwise_row(cuda, rid):
    """pmctf_ew_f32 with EW_MULS on views of 2^31 elements and just under: the launch key, the sentinels, windows against the
    numpy restatement and the whole output against the same product taken by torch on pieces of the views"""
    from pMCTF.hip import ops
    r = lp.row(rid)
    _skip_unless_memory(r)
    N, Cc, H, W = r[2][:4]
    (na, aoff, sa), (no, so) = lp.ew_views(r)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(lp.seed(rid))
    abuf = _normal((na + 8,), gen, 3.0)
    buf, _ = _guarded((no,))
    a = torch.as_strided(abuf, (N, Cc, H, W), sa, aoff)
    out = torch.as_strided(buf.view(torch.float32), (N, Cc, H, W), so, lp.PAD)
    ops.ew(ops.EW_MULS, a, alpha=lp.EW_ALPHA, out=out)
    launched = ops.ew_last_launch().rpartition(" grid ")[0]
    torch.cuda.synchronize()
    assert launched == r[7], f"{rid}: expected {r[7]}, launched {launched}"
    _check_sentinels(buf, rid)
    a_hwc, o_hwc = a.permute(0, 2, 3, 1), out.permute(0, 2, 3, 1)            # (N, H, W, C) views, whatever the storage order
    for win in lp.windows(r):
        what, n, oy0, ox0, h, wd = win
        xw = a_hwc[n, oy0:oy0 + h, ox0:ox0 + wd].cpu().numpy()
        got = o_hwc[n, oy0:oy0 + h, ox0:ox0 + wd].cpu().numpy()
        _host_bits(got, ec.expected(ec.EW_MULS, np.ascontiguousarray(xw), None, lp.EW_ALPHA, 0.0), f"{rid}, {what} at ({n}, {oy0}, {ox0})")
    rows = max(1, CHUNK // (Cc * W))
    for n in range(N):
        for h0 in range(0, H, rows):
            want = (a[n, :, h0:h0 + rows] * lp.EW_ALPHA).contiguous()
            got = out[n, :, h0:h0 + rows].contiguous()
            if not torch.equal(got.view(torch.int32), want.view(torch.int32)):
                ne = (got.view(torch.int32) != want.view(torch.int32)).nonzero()[0].tolist()
                raise AssertionError(f"{rid}: image {n}, rows from {h0}: first difference at (c, y, x) = ({ne[0]}, {h0 + ne[1]}, {ne[2]})")
            del want, got
    del a, out, abuf, buf
    torch.cuda.empty_cache()


def _guarded16(n):
    """int16 output of n elements between 2 * PAD sentinel halves (the same 256 bytes as the float outputs' pads)"""
    buf = torch.empty(n + 4 * lp.PAD, dtype=torch.int16, device="cuda")
    for i in range(0, buf.numel(), 2 * CHUNK):
        buf[i:i + 2 * CHUNK].fill_(0x5A5A)
    return buf, buf[2 * lp.PAD:2 * lp.PAD + n]


def _check_sentinels16(buf, what):
    p = 2 * lp.PAD
    assert bool((buf[:p] == 0x5A5A).all()) and bool((buf[-p:] == 0x5A5A).all()), f"{what}: wrote outside the output"
    body = buf[p:-p]
    for i in range(0, body.numel(), 2 * CHUNK):
        left = int((body[i:i + 2 * CHUNK] == 0x5A5A).sum())
        assert left == 0, f"{what}: {left} output elements in [{i}, {i + 2 * CHUNK}) were never written"


def _same_ints(got, want, what, base, r):
    if not torch.equal(got, want):
        first = int((got.reshape(-1) != want.reshape(-1)).nonzero()[0])
        where, byte = lp.first_difference(base + first, r)
        raise AssertionError(f"{what}: differs from the band run; first at (n, y, x, c) = {where}, element {base + first}")


@pytest.mark.parametrize("rid", FOURSTEP_ROWS)
def test_large_fourstep_row(cuda, rid):
    """the four-step coder's element kernels with an NHWC parameter tensor past 2^32 bytes, full size and at the class
    positions only (there the plane index passes 2^31 too): sentinels, windows against the entropy tests' restatement,
    the whole of every output against bands"""
    import entropy_restatement as er
    from pMCTF.hip import lib, ops
    L = lib.hip()
    r = lp.row(rid)
    _skip_unless_memory(r)
    N, _, Hp, Wp = r[2][:4]
    H, W, _ = lp.out_dims(r)
    psub, k, quant = int(lp.upsampled(r) == 2), lp.FOURSTEP_K, r[1] == "fourstep_quant"
    lmin, lstep = er.lmin_lstep()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(lp.seed(rid))
    params = _normal((N, Hp, Wp, 2), gen)
    params[..., 0].abs_().mul_(3.0).add_(0.01)                    # scales over the rows of the table, means normal
    if quant:
        planes = _normal((N, H, W), gen, 3.0)
    else:
        planes = torch.empty((N, H, W), dtype=torch.int16, device="cuda")
        flat = planes.view(-1)
        for i in range(0, flat.numel(), CHUNK):
            flat[i:i + CHUNK].random_(-200, 201, generator=gen)
    p = lambda t: C.c_void_p(t.data_ptr())

    def run(pl, par, so_far, sym, idx):
        n, h, w = pl.shape
        assert pl.is_contiguous() and par.is_contiguous() and so_far.is_contiguous() and tuple(par.shape) == (n, h >> psub, w >> psub, 2)
        if quant:
            rc = L.pmctf_fourstep_quant_f32(p(pl), p(par), p(so_far), p(sym), p(idx), n, h, w, k, psub, float(lmin), float(lstep), ops._stream())
        else:
            rc = L.pmctf_fourstep_dequant_f32(p(pl), p(par), p(so_far), n, h, w, k, psub, ops._stream())
        assert rc == 0, rc

    buf, so_far = _guarded((N, H, W))
    bsym, sym = _guarded16(N * H * W) if quant else (None, None)
    bidx, idx = _guarded16(N * H * W) if quant else (None, None)
    run(planes, params, so_far, sym, idx)
    torch.cuda.synchronize()
    _check_sentinels(buf, rid + " so_far")
    if quant:
        _check_sentinels16(bsym, rid + " sym")
        _check_sentinels16(bidx, rid + " idx")
    for win in lp.windows(r):
        what, n, oy0, ox0, h, wd = win
        ey0, ex0, eh, ew_ = lp.even_window(win)
        iy0, ix0, ih, iw = lp.input_window(r, win)
        xw = params[n, iy0:iy0 + ih, ix0:ix0 + iw].cpu().numpy()
        pw = planes[n, ey0:ey0 + eh, ex0:ex0 + ew_].cpu().numpy()
        want = lp.window_reference(r, win, xw, extra=pw)
        where = f"{rid}, {what} at ({n}, {oy0}, {ox0})"
        _host_bits(so_far[n, oy0:oy0 + h, ox0:ox0 + wd].cpu().numpy(), want[0], where + " so_far")
        if quant:
            for name, t, v in (("sym", sym, want[1]), ("idx", idx, want[2])):
                got = t.view(N, H, W)[n, oy0:oy0 + h, ox0:ox0 + wd].cpu().numpy()
                assert (got == v).all(), f"{where} {name}: {int((got != v).sum())} of {got.size} differ"
    for n, o0, o1, i0, i1 in lp.bands(r):
        pb, xb = params[n:n + 1, i0:i1].clone(), planes[n:n + 1, o0:o1].clone()
        assert pb.numel() * 4 < lp.G31 and xb.numel() * 4 < lp.G31 and (o0 >> psub) == i0 and ((o1 + psub) >> psub) == i1 and o0 % 2 == 0
        sb = torch.empty((1, o1 - o0, W), dtype=torch.float32, device="cuda")
        yb, ib = (torch.empty((1, o1 - o0, W), dtype=torch.int16, device="cuda") for _ in range(2)) if quant else (None, None)
        run(xb, pb, sb, yb, ib)
        base = (n * H + o0) * W
        _same_bits(so_far[n, o0:o1], sb[0], f"{rid} so_far rows [{o0}, {o1})", base, r)
        if quant:
            _same_ints(sym.view(N, H, W)[n, o0:o1], yb[0], f"{rid} sym rows [{o0}, {o1})", base, r)
            _same_ints(idx.view(N, H, W)[n, o0:o1], ib[0], f"{rid} idx rows [{o0}, {o1})", base, r)
        del pb, xb, sb, yb, ib
    del params, planes, buf, so_far, bsym, sym, bidx, idx
    torch.cuda.empty_cache()


def test_knobs_are_back_at_their_defaults(cuda):
    import os
    from pMCTF.hip import lib
    L = lib.hip()
    for k, v in cc.KNOBS.items():
        if f"PMCTF_CONV_{k}" not in os.environ:
            assert L.pmctf_conv2d_get_option(k.encode()) == v, k
