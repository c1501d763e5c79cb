"""The scalar functions of csrc/pm_device_math.h as the GPU compiler builds them, against the oracle (which is pinned to
torch): every function of pmctf_math_probe_f32 on ALL 2^32 float32 bit patterns, the same values out of real kernels on the
stratified set S of math_sweep.py, and the CDF row of every non-negative scale.  The bar is bit equality; where both
results are NaN the payload is exempt, and counted in what the tests print.  The oracle is the specification."""
import time

import numpy as np
import pytest
import torch

import math_sweep as ms

pytestmark = pytest.mark.gpu


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32))


class Tally:
    """mismatches of one function over many pieces: count, first pattern with both results, NaN-payload exemptions"""

    def __init__(self):
        self.count, self.first, self.exempt, self.elements = {}, {}, {}, {}

    def check(self, name, got, want_bits, pattern_of):
        """got: device float32 tensor; want_bits: numpy uint32 of the same length; pattern_of(i): input of element i"""
        want = _i32(want_bits).cuda()
        got = got.reshape(-1).view(torch.int32)
        assert got.numel() == want.numel(), (name, got.numel(), want.numel())
        self.elements[name] = self.elements.get(name, 0) + got.numel()
        neq = got != want
        if not bool(neq.any()):
            return
        at = neq.nonzero()[:, 0]
        g, w, at = got[at].cpu().numpy().view(np.uint32), want[at].cpu().numpy().view(np.uint32), at.cpu().numpy()
        count, first, exempt = ms.compare(g, w)
        self.exempt[name] = self.exempt.get(name, 0) + exempt
        if count:
            if name not in self.first:
                self.first[name] = (f"{self.count.get(name, 0) + count} mismatches so far; first at input "
                                    f"{pattern_of(int(at[first])):#010x}: GPU {int(g[first]):#010x}, oracle {int(w[first]):#010x}")
            self.count[name] = self.count.get(name, 0) + count

    def report(self):
        return "; ".join(f"{n}: {self.elements[n]} elements, {self.count.get(n, 0)} mismatches, "
                         f"{self.exempt.get(n, 0)} both-NaN payload differences (exempt)" for n in self.elements)

    def assert_clean(self, what):
        print(f"{what}: {self.report()}")
        bad = {n: f"{self.count[n]} mismatches in all; {self.first[n]}" for n in self.count}
        assert not bad, f"{what}: {bad}; NaN-payload exemptions: {self.exempt}"


def test_every_function_on_every_float32_input(cuda):
    """Every probe code over all 2^32 patterns, 2^26 per chunk (256 MB of results on the device), against its oracle map;
    relu against torch.relu, leaky against numpy.  Zero mismatches, no tolerance.  The oracle's tanh runs once per chunk for
    both table homes and apply_act, its sigmoid once for sigmoidf_ and apply_act: seven oracle maps per chunk.

    Measured on an MI355X box with 16 CPU threads for the oracle: see DESIGN.md section 6b."""
    from pMCTF.hip import ops
    t0 = time.time()
    tally = Tally()
    out = torch.empty(ms.CHUNK, dtype=torch.float32, device="cuda")
    for first, n in ms.chunks():
        x = ms.chunk_bits(first, n).view(np.float32)
        want = {}
        for name, code, spec in ms.FUNCTIONS:
            got = ops.math_probe(code, None, first, n, slope=ms.LEAKY_SLOPE, out=out)     # runs while the oracle computes
            if spec not in want:              # one oracle tanh for both table homes and apply_act; likewise sigmoid
                want[spec] = spec(x).view(np.uint32)
            tally.check(name, got, want[spec], lambda i, first=first: first + i)
        if (first >> 26) % 8 == 7:
            print(f"  through {first + n - 1:#010x} after {time.time() - t0:.0f} s", flush=True)
    print(f"exhaustive sweep: {time.time() - t0:.0f} s")
    assert set(tally.elements.values()) == {1 << 32} and len(tally.elements) == len(ms.FUNCTIONS) == 12
    assert len(want) == 9                                     # seven oracle maps, torch.relu, numpy's leaky
    tally.assert_clean("all 2^32 inputs")


def test_probe_takes_given_patterns_and_any_length(cuda):
    """bits given instead of generated, lengths that are not a multiple of four (the scalar tail), a sweep that wraps"""
    from pMCTF.hip import ops
    bits = ms.special_patterns()
    for n in (1, 2, 3, 5, bits.size - 1, bits.size):
        for name in ("tanh_lds", "log", "act_leaky"):
            got = ops.math_probe(ms.CODE[name], _i32(bits[:n]).cuda(), slope=ms.LEAKY_SLOPE)
            count, first, _ = ms.compare(got.cpu().numpy(), ms.SPEC[name](bits[:n].view(np.float32)))
            assert count == 0, (name, n, hex(int(bits[first])))
    got = ops.math_probe(ms.CODE["exp"], None, 0xfffffffe, 7)
    want = ms.SPEC["exp"](np.array([0xfffffffe, 0xffffffff, 0, 1, 2, 3, 4], np.uint32).view(np.float32))
    assert ms.compare(got.cpu().numpy(), want)[0] == 0
    L = __import__("pMCTF.hip.lib", fromlist=["hip"]).hip()
    assert L.pmctf_math_probe_f32(0, None, 0, 4, None, 0.0, None) == -1
    assert L.pmctf_math_probe_f32(8, None, 0, 4, got.data_ptr(), 0.0, None) == -1         # PROBE_ACT + ACT_NONE: no function
    assert L.pmctf_math_probe_f32(13, None, 0, 4, got.data_ptr(), 0.0, None) == -1
    assert L.pmctf_math_probe_f32(0, None, 0, 0, got.data_ptr(), 0.0, None) == -1


def _padded(bits, multiple):
    pad = (-bits.size) % multiple
    return np.concatenate([bits, np.full(pad, bits[0], np.uint32)])


def test_ew_tanh_on_s_in_every_layout(cuda):
    """ops.ew(EW_TANH) on S through each kernel of pmctf_ew_f32: dense flat 16-byte form, odd-length flat scalar form,
    channel-fastest four-channel form (a channel slice of an NHWC tensor), transposed planes, generic strided view"""
    from pMCTF.hip import ops
    tally = Tally()
    for label, bits in ms.stratified():
        bits = _padded(bits, 2048 * 8)
        want = ms.SPEC["tanh"](bits.view(np.float32)).view(np.uint32)
        x = _i32(bits).cuda().view(torch.float32)
        M, W = bits.size, 2048
        H = M // W
        at = lambda i: int(bits[i])
        tally.check("flat vector", ops.ew(ops.EW_TANH, x.view(1, 1, H, W)), want, at)
        tally.check("flat scalar, odd length", ops.ew(ops.EW_TANH, x[:M - 1].view(1, 1, 1, M - 1)), want[:M - 1], at)
        t = torch.zeros(1, H, W // 8, 16, device="cuda")
        t[..., 8:] = x.view(1, H, W // 8, 8)
        got = ops.ew(ops.EW_TANH, ops.as_nchw(t)[:, 8:])                                  # logical (1, 8, H, W/8), NHWC storage
        tally.check("channel-fastest, C % 4 == 0", got.permute(0, 2, 3, 1).contiguous(), want, at)
        a = x.view(1, 1, W, H).permute(0, 1, 3, 2)                                        # element (h, w) at w * H + h
        got = ops.ew(ops.EW_TANH, a)
        assert got.is_contiguous()
        tally.check("transposed planes", got.permute(0, 1, 3, 2).contiguous(), want, at)
        buf = torch.zeros(1, 1, H, 2 * W, device="cuda")
        buf[..., ::2] = x.view(1, 1, H, W)
        tally.check("generic strided", ops.ew(ops.EW_TANH, buf[..., ::2]), want, at)
    assert len(tally.elements) == 5
    tally.assert_clean("ew(EW_TANH) on S")


@pytest.mark.parametrize("C", [3, 4], ids=["scalar", "vec4"])
def test_pixel_shuffle2_activations_on_s(cuda, C):
    """ops.pixel_shuffle2 with acts 1-4 (relu, leaky, tanh, sigmoid) through the scalar (C % 4 != 0) and the 16-byte kernel:
    a pure permutation, so the expected values are a reindexing of the oracle's: out[2h+i, 2w+j, c] = act(x[h, w, 4c+2i+j])"""
    from pMCTF.hip import ops
    tally = Tally()
    W = 64
    for label, bits in ms.stratified():
        bits = _padded(bits, W * 4 * C)
        H = bits.size // (W * 4 * C)
        x = _i32(bits).cuda().view(torch.float32).view(1, H, W, 4 * C)

        def shuffled(a):
            return np.ascontiguousarray(a.reshape(1, H, W, C, 2, 2).transpose(0, 1, 4, 2, 5, 3)).reshape(-1)
        src = shuffled(bits)
        for act, name in ((ops.ACT_RELU, "act_relu"), (ops.ACT_LEAKY, "act_leaky"), (ops.ACT_TANH, "act_tanh"),
                          (ops.ACT_SIGMOID, "act_sigmoid")):
            want = shuffled(ms.SPEC[name](bits.view(np.float32)).view(np.uint32))
            got = ops.pixel_shuffle2(x, act=act, slope=ms.LEAKY_SLOPE)
            assert tuple(got.shape) == (1, 2 * H, 2 * W, C)
            tally.check(name, got, want, lambda i: int(src[i]))
    assert len(tally.elements) == 4
    tally.assert_clean(f"pixel_shuffle2, C = {C}, on S")


@pytest.mark.parametrize("aten_threads", [0, 8])
def test_lstm_gates_on_s(cuda, aten_threads):
    """ops.lstm_gates on S, composed from the oracle's primitives exactly as test_lstm_gates_with_aten_thread_tails does:
    g = sigmoid(x) (with ATen's scalar tails for aten_threads = 8: three channels, so the eight slices end off a stride of
    32), cell' = g * cell + g * tanh(x), hidden = g * tanh(cell')"""
    from pmctf_oracle import clib
    from pMCTF.hip import ops
    tally = Tally()
    c, w = 3, 1021
    for label, bits in ms.stratified():
        bits = _padded(bits, c * w)
        h = bits.size // (c * w)
        x = bits.view(np.float32).reshape(1, c, h, w)
        cell = (((np.arange(x.size) % 7).astype(np.float32) - 3) * np.float32(0.25)).reshape(1, c, h, w)
        with np.errstate(all="ignore"):
            g = clib.sigmoid(x, aten_threads)
            cn = g * cell + g * clib.tanh(x)
            hid = g * clib.tanh(np.ascontiguousarray(cn))
        if aten_threads:
            assert (x.size + 7) // 8 % 32 != 0                    # the slices do have scalar tails
        nhwc = lambda t: torch.from_numpy(np.ascontiguousarray(t.transpose(0, 2, 3, 1))).cuda()
        got_h, got_c = ops.lstm_gates(nhwc(x), nhwc(cell), ref_planes=1, aten_threads=aten_threads)
        src = bits.reshape(1, c, h, w)
        at = lambda i: int(src.reshape(-1)[i])
        tally.check("cell", got_c.permute(0, 3, 1, 2).contiguous(), cn.view(np.uint32).reshape(-1), at)
        tally.check("hidden", got_h.permute(0, 3, 1, 2).contiguous(), hid.view(np.uint32).reshape(-1), at)
    tally.assert_clean(f"lstm_gates, aten_threads = {aten_threads}, on S")


def test_cdf_row_of_every_scale(cuda):
    """All 2^31 non-negative float32 patterns (the positive NaNs among them) and the negative NaNs' ends through one decode
    site (fourstep_indexes) and one encode site (ll_quant), against trunc(clamp((log(max(s, 1e-5)) - lmin) / step, 0, 255))
    with the oracle's log and numpy float32 for the rest; NaN takes row 0, the row of 1e-5, as
    test_scale_index_rows_at_every_gpu_site pins it (the product's max is s >= 1e-5 ? s : 1e-5).  Also covers the
    device's division."""
    from pmctf_oracle import clib, entropy
    from pMCTF.hip import ops
    g = entropy.GaussianTables()
    lmin, lstep = g.log_scale_min, g.log_scale_step
    n = 1 << 25
    bad = {}
    x4 = torch.zeros(1, 1, 2, n // 2, device="cuda")

    def pieces():
        for first in range(0, 1 << 31, n):
            yield first, ms.chunk_bits(first, n)
        yield 0xff800001, np.resize(np.array([0xff800001, 0xffc00000, 0xffffffff, 0xff800000 + 12345], np.uint32), n)   # negative NaNs
    for first, bits in pieces():
        x = bits.view(np.float32)
        with np.errstate(all="ignore"):
            s = np.where(np.isnan(x), np.float32(1e-5), np.maximum(x, np.float32(1e-5)))
            v = (clib.log(s) - np.float32(lmin)) / np.float32(lstep)
            want = np.clip(v, np.float32(0), np.float32(255)).astype(np.int16)
        wd = torch.from_numpy(want).cuda()
        sd = _i32(bits).cuda().view(torch.float32)
        params = torch.stack([sd, torch.zeros_like(sd)], -1).view(1, 2, n // 2, 2).contiguous()
        got_i = torch.zeros(n, dtype=torch.int16, device="cuda")
        for k in range(4):
            got_i += ops.fourstep_indexes(params, 1, 2, n // 2, k, lmin, lstep)
        sym = torch.zeros(n, dtype=torch.int16, device="cuda")
        got_q = torch.zeros(n, dtype=torch.int16, device="cuda")
        ops.ll_quant(x4, params, sym, got_q, 0, lmin, lstep)
        for site, got in (("fourstep_indexes", got_i), ("ll_quant", got_q)):
            neq = (got != wd).nonzero()[:, 0]
            if neq.numel() and site not in bad:
                i = int(neq[0])
                bad[site] = (f"{neq.numel()} rows differ in the piece that begins with {first:#010x}; first at scale {int(bits[i]):#010x}: "
                             f"GPU row {int(got[i])}, expected {int(want[i])}")
    assert not bad, bad
