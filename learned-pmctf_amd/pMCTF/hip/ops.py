"""Tensor-level wrappers over the C ABI (include/pmctf_hip.h).

torch is used here only for device memory (torch.empty), the current HIP stream and
host-side weight staging; every numeric operation is a call into libpmctf_hip.so.
Feature maps are NHWC float32 tensors of shape (N, H, W, C); single-channel planes
(N, 1, H, W) alias the same memory.
"""
import contextlib
import ctypes as C
import os
import threading

import numpy as np
import torch

from . import lib as _lib

ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3, 4
SUM_CHAIN, SUM_BLOCKS, SUM_GEMM, SUM_GEMV_3X3 = 0, 1, 2, 3        # PMCTF_SUM_* of include/pmctf_hip.h: the summation rule of a convolution

# Optional live timing of one conv signature with HIP events on the launch stream (bench.py: roofline of the
# dominant kernel).  CONV_PROBE = {"match": fn(conv, x, stride) -> bool, "events": [(start, end, flops)]}
CONV_PROBE = None
# planes below this keep the exact f32 kernels under the reduced-precision profile (too few tiles)
SPLIT_MIN_PX = int(os.environ.get("PMCTF_SPLIT_MIN_PX", "30000"))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class ConvLaunchOpts(C.Structure):
    """pmctf_conv_launch_opts (include/pmctf_hip.h): launch-shape options handed over WITH a launch; < 0 = process knob"""
    _fields_ = [("split", C.c_long), ("msplit_px", C.c_long)]


_tls = threading.local()


@contextlib.contextmanager
def launch_opts(opts):
    """Convolutions launched by the calling thread inside the block carry `opts` (a ConvLaunchOpts, or None) as their
    per-launch argument.  Nothing process-wide is touched: other host threads keep their own launch shapes."""
    prev = getattr(_tls, "opts", None)
    _tls.opts = opts
    try:
        yield
    finally:
        _tls.opts = prev


def _opts():
    o = getattr(_tls, "opts", None)
    return None if o is None else C.byref(o)


def _p(t):
    if t is None:
        return None
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), "expect dense float32 device tensor"
    return C.c_void_p(t.data_ptr())


def _dev(x):
    if not x.is_cuda:
        raise RuntimeError("pMCTF HIP ops need device tensors: there is no CPU fallback on the product path")
    return x.device


# filters larger than this go to the matrix-core kernel even with one or two couts (see Conv2d.__init__)
FEWCOUT_MAX_K = int(os.environ.get("PMCTF_FEWCOUT_MAX_K", "7"))


class Conv2d:
    """A packed nn.Conv2d (groups=1): weights re-laid out once for the MFMA kernel
    (Cin % 4 == 0) or kept OIHW for the small-Cin vector kernel."""

    def __init__(self, weight, bias, stride=1, padding=(0, 0), device="cuda", split=0, rule=SUM_CHAIN):
        """rule: the layer's summation rule (SUM_CHAIN / SUM_BLOCKS / a reduce-block size B >= 16, include/pmctf_hip.h),
        or a function (N, H, W) -> rule for layers whose rule follows from the reference tensor's shape (1x1 layers,
        pMCTF.hip.aten_rules) — part of the layer's arithmetic, chosen by whoever owns the layer (HipEngine.sum_rule),
        never by the launch shape.
        split = 1, 2 or 3: ALSO pack bf16-split weights for the auxiliary reduced-precision kernel (conv_split.hip) and
        use it on planes of at least SPLIT_MIN_PX output pixels when the shape is supported; 0 (default): exact f32 only."""
        w = weight.detach().to("cpu", torch.float32).contiguous()
        b = None if bias is None else bias.detach().to("cpu", torch.float32).contiguous()
        self.Cout, self.Cin, self.KH, self.KW = w.shape
        self.stride = int(stride)
        self.rule = rule if callable(rule) else int(rule)
        self.pad = (int(padding[0]), int(padding[1])) if isinstance(padding, (tuple, list)) else (int(padding),) * 2
        self.small = self.Cin <= 4
        L = _lib.hip()
        # one or two couts: vector-ALU kernel on plain OIHW weights (a matrix-core tile would be 15/16 empty)
        self.few = (not self.small and self.stride == 1 and self.KH == self.KW and self.pad == (self.KH // 2,) * 2
                    and bool(L.pmctf_conv2d_fewcout_supported(self.Cin, self.Cout, self.KH))
                    and self.KH <= FEWCOUT_MAX_K)
        if self.small or self.few:
            self.w = w.to(device)
            self.b = None if b is None else b.to(device)
        else:
            if self.Cin % 4:
                raise ValueError("MFMA conv path needs Cin % 4 == 0")
            n = L.pmctf_conv2d_packed_size(self.Cout, self.Cin, self.KH, self.KW)
            nb = L.pmctf_conv2d_packed_bias_size(self.Cout)
            wp = np.empty(n, np.float32)
            bp = np.empty(nb, np.float32)
            wn = w.numpy()
            bn = None if b is None else b.numpy()
            _lib.check(L.pmctf_conv2d_pack_weights(wn.ctypes.data, None if bn is None else bn.ctypes.data,
                                                   self.Cout, self.Cin, self.KH, self.KW,
                                                   wp.ctypes.data, bp.ctypes.data), "pack_weights")
            self.w = torch.from_numpy(wp).to(device)
            self.b = torch.from_numpy(bp).to(device)
        self.split = 0
        if (split and not self.small and not self.few and self.stride == 1 and self.KH == 3 and self.KW == 3
                and self.pad == (1, 1) and L.pmctf_conv3x3_split_supported(self.Cin, self.Cout)):
            n16 = L.pmctf_conv3x3_split_packed_size(self.Cout, self.Cin, int(split))
            wp16 = np.empty(n16, np.uint16)
            bp2 = np.empty(L.pmctf_conv2d_packed_bias_size(self.Cout), np.float32)
            wn = w.numpy()
            bn = None if b is None else b.numpy()
            _lib.check(L.pmctf_conv3x3_split_pack_weights(wn.ctypes.data, None if bn is None else bn.ctypes.data,
                                                          self.Cout, self.Cin, int(split), wp16.ctypes.data,
                                                          bp2.ctypes.data), "split pack_weights")
            self.w16 = torch.from_numpy(wp16.view(np.int16)).to(device)
            self.split = int(split)

    def out_shape(self, x):
        N, H, W, Cin = x.shape
        Ho = (H + 2 * self.pad[0] - self.KH) // self.stride + 1
        Wo = (W + 2 * self.pad[1] - self.KW) // self.stride + 1
        return (N, Ho, Wo, self.Cout)

    def __call__(self, x, act=ACT_NONE, slope=0.0, res1=None, res2=None, out=None, rule_hw=None):
        """rule_hw: (H, W) of the plane the REFERENCE evaluates this layer on, when x holds only some of its positions
        (a shape-dependent summation rule follows the reference's call, not this launch's)"""
        _dev(x)
        N, H, W, Cin = x.shape
        if Cin != self.Cin:
            raise ValueError(f"conv expects {self.Cin} input channels, got {Cin}")
        shp = self.out_shape(x)
        y = out if out is not None else torch.empty(shp, dtype=torch.float32, device=x.device)
        assert tuple(y.shape) == shp
        for r in (res1, res2):
            assert r is None or tuple(r.shape) == shp
        L = _lib.hip()
        rule = self.rule(N, *(rule_hw or (H, W))) if callable(self.rule) else self.rule
        if self.few:
            _lib.check(L.pmctf_conv2d_fewcout_f32(_p(x), _p(self.w), _p(self.b), _p(res1), _p(res2), _p(y), N, H, W, Cin,
                                                  self.Cout, self.KH, int(act), float(slope), rule, _stream()),
                       "conv2d_fewcout")
            return y
        probe = CONV_PROBE if (CONV_PROBE is not None and not torch.cuda.is_current_stream_capturing()
                               and CONV_PROBE["match"](self, x, self.stride)) else None
        if probe is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        use_split = self.split and N * H * W >= SPLIT_MIN_PX and int(act) <= ACT_LEAKY
        if use_split:                                       # auxiliary reduced-precision profile (never the parity path)
            _lib.check(L.pmctf_conv3x3_split_f32(_p(x), C.c_void_p(self.w16.data_ptr()), _p(self.b), _p(res1), _p(res2),
                                                 _p(y), N, H, W, Cin, self.Cout, self.split, int(act), float(slope),
                                                 _stream()), "conv3x3_split")
        elif self.small:
            _lib.check(L.pmctf_conv2d_smallcin_f32(_p(x), _p(self.w), _p(self.b), _p(res1), _p(res2), _p(y), N, H, W, Cin,
                                                   self.Cout, self.KH, self.KW, self.stride, self.pad[0], self.pad[1],
                                                   int(act), float(slope), rule, _stream()), "conv2d_smallcin")
        else:
            _lib.check(L.pmctf_conv2d_nhwc_opts_f32(_p(x), _p(self.w), _p(self.b), _p(res1), _p(res2), _p(y), N, H, W, Cin,
                                                    self.Cout, self.KH, self.KW, self.stride, self.pad[0], self.pad[1],
                                                    int(act), float(slope), rule, _opts(), _stream()), "conv2d")
        if probe is not None:
            e1.record()
            probe["events"].append((e0, e1, 2.0 * shp[0] * shp[1] * shp[2] * self.Cout * Cin * self.KH * self.KW))
            if "kernels" in probe and not use_split:
                buf = C.create_string_buffer(512)
                L.pmctf_conv2d_last_launch(buf, 512)
                probe["kernels"][buf.value.decode()] = probe["kernels"].get(buf.value.decode(), 0) + 1
        return y


def conv3x3_cin1_dual(conv, x, act2, out=None, out2=None):
    """conv: a 1->16 3x3 'same' Conv2d; x (N,H,W,1).  Returns (conv(x), act2(conv(x))) from one launch."""
    assert conv.small and conv.Cin == 1 and conv.Cout == 16 and conv.KH == 3 and conv.stride == 1 and conv.pad == (1, 1)
    N, H, W, _ = x.shape
    y = out if out is not None else torch.empty((N, H, W, 16), dtype=torch.float32, device=x.device)
    y2 = out2 if out2 is not None else torch.empty_like(y)
    assert tuple(y.shape) == tuple(y2.shape) == (N, H, W, 16)
    _lib.check(_lib.hip().pmctf_conv3x3_cin1_dual_f32(_p(x), _p(conv.w), _p(conv.b), _p(y), _p(y2), N, H, W, 16, int(act2),
                                                      0.0, conv.rule, _stream()), "conv3x3_cin1_dual")
    return y, y2


class DepthwiseConv2d:
    def __init__(self, weight, bias, device="cuda"):
        self.C, _, self.K, _ = weight.shape
        self.w = weight.detach().to(device, torch.float32).contiguous()
        self.b = None if bias is None else bias.detach().to(device, torch.float32).contiguous()

    def __call__(self, x, out=None):
        N, H, W, Cc = x.shape
        assert Cc == self.C
        y = out if out is not None else torch.empty_like(x)
        assert tuple(y.shape) == tuple(x.shape)
        _lib.check(_lib.hip().pmctf_dwconv2d_nhwc_f32(_p(x), _p(self.w), _p(self.b), _p(y), N, H, W, Cc, self.K,
                                                      _stream()), "dwconv2d")
        return y


def valu_conv_last_launch():
    """Measurement aid: 'kernel expression grid G' of the last small-Cin / cin1-dual / few-cout / depthwise convolution
    this thread launched (csrc/basic_ops.hip), '' when that call refused its arguments"""
    buf = C.create_string_buffer(160)
    _lib.check(_lib.hip().pmctf_valu_conv_last_launch(buf, 160), "valu_conv_last_launch")
    return buf.value.decode()


def flow_warp(im, flow, lin_x, lin_y, sign=1.0):
    """im (N,C,H,W) planar, flow (1|N,2,H,W) planar."""
    N, Cc, H, W = im.shape
    out = torch.empty_like(im)
    _lib.check(_lib.hip().pmctf_flow_warp_f32(_p(im), _p(flow), _p(lin_x), _p(lin_y), _p(out), N, Cc, H, W,
                                              flow.shape[0], float(sign), _stream()), "flow_warp")
    return out


def avgpool2(x):
    N, Cc, H, W = x.shape
    y = torch.empty((N, Cc, H // 2, W // 2), dtype=torch.float32, device=x.device)
    _lib.check(_lib.hip().pmctf_avgpool2_f32(_p(x), _p(y), N * Cc, H, W, _stream()), "avgpool2")
    return y


def bilinear_up2(x, scale=1.0, factor=2):
    """F.interpolate(bilinear, align_corners=False) to factor x the size (2, 4 or 8), result times `scale`"""
    N, Cc, H, W = x.shape
    y = torch.empty((N, Cc, factor * H, factor * W), dtype=torch.float32, device=x.device)
    _lib.check(_lib.hip().pmctf_bilinear_up_f32(_p(x), _p(y), N * Cc, H, W, int(factor), float(scale), _stream()),
               "bilinear_up")
    return y


def bilinear_down2(x, div=1.0, factor=2):
    """F.interpolate(bilinear, align_corners=False) to 1/factor of the size (2, 4 or 8), result divided by `div`"""
    N, Cc, H, W = x.shape
    y = torch.empty((N, Cc, H // factor, W // factor), dtype=torch.float32, device=x.device)
    _lib.check(_lib.hip().pmctf_bilinear_down_f32(_p(x), _p(y), N * Cc, H, W, int(factor), float(div), _stream()),
               "bilinear_down")
    return y


# ------------------------------------------------------------------------------------------------
# elementwise / layout family (pmctf_ew_f32): operands are logical (N,C,H,W) views with any strides
EW_COPY, EW_ADD, EW_SUB, EW_MUL, EW_DIV, EW_MULS, EW_DIVS, EW_ADD_MULS, EW_SUB_MULS, EW_ADD_MULS_MULS, \
    EW_CLAMP_MULS, EW_ROUND_CLAMP_MULS, EW_ROUND, EW_LEAKY, EW_ADD_MULS2, EW_SUB_MULS2, EW_ROUND_CLAMP, EW_TANH = range(18)

_I64x4 = C.c_int64 * 4


def _raw(t):
    assert t.is_cuda and t.dtype == torch.float32
    return C.c_void_p(t.data_ptr())


def as_nchw(t_nhwc):
    """NHWC storage (N,H,W,C) -> logical NCHW view (no copy)."""
    return t_nhwc.permute(0, 3, 1, 2)


def as_nhwc(t_nchw):
    """logical NCHW view whose storage is channels-last dense -> (N,H,W,C) dense tensor (no copy)."""
    v = t_nchw.permute(0, 2, 3, 1)
    if not v.is_contiguous():
        raise ValueError("tensor is not channels-last dense")
    return v


def empty_planar(n, c, h, w, device):
    return torch.empty((n, c, h, w), dtype=torch.float32, device=device)


def empty_nhwc(n, h, w, c, device):
    return torch.empty((n, h, w, c), dtype=torch.float32, device=device)


def ew(op, a, b=None, alpha=0.0, beta=0.0, out=None):
    """out = op(a, b) over logical (N,C,H,W) views (b may be broadcast with stride 0 via expand)."""
    N, Cc, H, W = a.shape
    if out is None:
        if Cc > 1 and a.stride(1) == 1:
            out = as_nchw(empty_nhwc(N, H, W, Cc, a.device))
        else:
            out = empty_planar(N, Cc, H, W, a.device)
    assert tuple(out.shape) == (N, Cc, H, W), (tuple(out.shape), (N, Cc, H, W))
    if b is not None and tuple(b.shape) != (N, Cc, H, W):
        b = b.expand(N, Cc, H, W)
    so, sa = _I64x4(*out.stride()), _I64x4(*a.stride())
    sb = _I64x4(*b.stride()) if b is not None else None
    cfast = 1 if (Cc > 1 and out.stride(1) == 1) else 0
    _lib.check(_lib.hip().pmctf_ew_f32(int(op), _raw(out), so, _raw(a), sa, None if b is None else _raw(b), sb,
                                       N, Cc, H, W, float(alpha), float(beta), cfast, _stream()), "ew")
    return out


def ew_last_launch():
    """Measurement aid: 'kernel expression[ channels| rows] grid G' of the last ew / nearest_up2 / pixel_shuffle2 this thread
    launched (csrc/ew_ops.hip), '' when that call refused its arguments"""
    buf = C.create_string_buffer(160)
    _lib.check(_lib.hip().pmctf_ew_last_launch(buf, 160), "ew_last_launch")
    return buf.value.decode()


def spynet_pack8(im1, warped, flow_up):
    _, _, H, W = im1.shape
    out = empty_nhwc(1, H, W, 8, im1.device)
    _lib.check(_lib.hip().pmctf_spynet_pack8_f32(_p(im1), _p(warped), _p(flow_up), _p(out), H, W, _stream()),
               "spynet_pack8")
    return out


def lift_skip3(x, w3, bias, rule=SUM_CHAIN):
    N, Cc, H, W = x.shape
    y = torch.empty_like(x)
    _lib.check(_lib.hip().pmctf_lift_skip3_f32(_p(x), _p(y), N * Cc, H, W, float(w3[0]), float(w3[1]), float(w3[2]),
                                               float(bias), int(rule), _stream()), "lift_skip3")
    return y


def predict_update_fused(x, other, pu, mode, c=1.0, sign=1.0, lift=(0.0, 0.0, 0.0, 0.0), skip_rule=SUM_CHAIN):
    """pu: (conv1, conv2, conv3, conv4) Conv2d objects of one PredictUpdate block.  mode 0: (x + PU(x)*0.1)*c;
    mode 1: other + sign * (skip + PU(skip/256)*256*0.1) with skip = reflect 3x1 conv of x (lift = w0, w1, w2, bias;
    skip_rule: summation rule of that 3x1 filter).  The four layers carry their own rule (one for the block)."""
    c1, c2, c3, c4 = pu
    N, Cc, H, W = x.shape
    assert Cc == 1 and c1.small and c4.few and not c2.small and not c2.few
    assert c1.rule == c2.rule == c3.rule == c4.rule
    out = torch.empty_like(x)
    _lib.check(_lib.hip().pmctf_predict_update_fused_f32(
        _p(x), _p(other), _p(out), _p(c1.w), _p(c1.b), _p(c2.w), _p(c2.b), _p(c3.w), _p(c3.b), _p(c4.w), _p(c4.b),
        N, H, W, int(mode), float(c), float(sign), float(lift[0]), float(lift[1]), float(lift[2]), float(lift[3]),
        c1.rule, int(skip_rule), _stream()), "predict_update_fused")
    return out


def nearest_up2(x):
    N, H, W, Cc = x.shape
    y = empty_nhwc(N, 2 * H, 2 * W, Cc, x.device)
    _lib.check(_lib.hip().pmctf_nearest_up2_nhwc_f32(_p(x), _p(y), N, H, W, Cc, _stream()), "nearest_up2")
    return y


def pixel_shuffle2(x, act=ACT_NONE, slope=0.0):
    N, H, W, C4 = x.shape
    assert C4 % 4 == 0
    y = empty_nhwc(N, 2 * H, 2 * W, C4 // 4, x.device)
    _lib.check(_lib.hip().pmctf_pixel_shuffle2_nhwc_f32(_p(x), _p(y), N, H, W, C4 // 4, int(act), float(slope),
                                                        _stream()), "pixel_shuffle2")
    return y


def ffn3_mix(x):
    N, H, W, C2 = x.shape
    y = empty_nhwc(N, H, W, C2 // 2, x.device)
    _lib.check(_lib.hip().pmctf_ffn3_mix_f32(_p(x), _p(y), N * H * W, C2 // 2, _stream()), "ffn3_mix")
    return y


def lstm_gates(xh, cell, ref_planes=None, aten_threads=0):
    """aten_threads > 0: torch.sigmoid as ATen splits the reference's (ref_planes, C, H, W) gate tensor over that many
    threads (include/pmctf_hip.h pmctf_lstm_gates_aten_f32); ref_planes defaults to the batch of xh"""
    N, H, W, Cc = xh.shape
    cell_out, hid_out = torch.empty_like(xh), torch.empty_like(xh)
    _lib.check(_lib.hip().pmctf_lstm_gates_aten_f32(_p(xh), _p(cell), _p(cell_out), _p(hid_out), N * H * W, Cc,
                                                    cell.shape[3], H * W, int(ref_planes or N), int(aten_threads),
                                                    _stream()), "lstm_gates")
    return hid_out, cell_out


def _p16(t, off):
    assert t.is_cuda and t.dtype == torch.int16 and t.is_contiguous()
    return C.c_void_p(t.data_ptr() + 2 * off)


def fourstep_quant(x, params, so_far, sym, idx, off, k, lmin, lstep):
    """params: (N,H,W,2), or (N,H/2,W/2,2) when computed only at the class-k positions"""
    N, _, H, W = x.shape
    sub = 0 if params.shape[1] == H else 1
    assert params.shape[1] * (1 + sub) == H and params.shape[2] * (1 + sub) == W
    _lib.check(_lib.hip().pmctf_fourstep_quant_f32(_p(x), _p(params), _p(so_far), _p16(sym, off), _p16(idx, off),
                                                   N, H, W, k, sub, float(lmin), float(lstep), _stream()),
               "fourstep_quant")


def conv_at_class(conv, x, cls, act=ACT_NONE, slope=0.0, res1=None, res2=None):
    """Evaluate the stride-1 'same' 3x3 conv `conv` only at the positions (2i+py, 2j+px) of parity class cls = 2*py+px:
    the same sums as the full conv at those positions (stride 2, top/left pad 1-py / 1-px, zeros outside)."""
    assert not conv.small and conv.stride == 1 and conv.KH == 3 and conv.KW == 3 and conv.pad == (1, 1)
    N, H, W, Cin = x.shape
    assert H % 2 == 0 and W % 2 == 0 and Cin == conv.Cin
    py, px = cls >> 1, cls & 1
    y = torch.empty((N, H // 2, W // 2, conv.Cout), dtype=torch.float32, device=x.device)
    probe = CONV_PROBE if (CONV_PROBE is not None and not torch.cuda.is_current_stream_capturing()
                           and CONV_PROBE["match"](conv, x, 2)) else None
    if probe is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    if conv.split and conv.Cout == 112 and y.shape[0] * y.shape[1] * y.shape[2] >= SPLIT_MIN_PX and int(act) <= ACT_LEAKY:
        _lib.check(_lib.hip().pmctf_conv3x3_split_geom_f32(_p(x), C.c_void_p(conv.w16.data_ptr()), _p(conv.b), _p(res1),
                                                           _p(res2), _p(y), N, H, W, Cin, conv.Cout, conv.split, 2, 1 - py,
                                                           1 - px, H // 2, W // 2, int(act), float(slope), _stream()),
                   "conv3x3_split_geom")
    else:
        _lib.check(_lib.hip().pmctf_conv2d_nhwc_geom_opts_f32(_p(x), _p(conv.w), _p(conv.b), _p(res1), _p(res2), _p(y), N, H,
                                                              W, Cin, conv.Cout, 3, 3, 2, 1 - py, 1 - px, H // 2, W // 2,
                                                              int(act), float(slope), conv.rule, _opts(), _stream()),
                   "conv2d_geom")
    if probe is not None:
        e1.record()
        probe["events"].append((e0, e1, 2.0 * y.numel() * Cin * 9))
    return y


def ll_quant(ll, params, sym, idx, off, lmin, lstep, ar_order=False):
    """ar_order: symbols in the sequential coder's order (position-major over the N planes)"""
    ll_hat = torch.empty_like(ll)
    _lib.check(_lib.hip().pmctf_ll_quant_f32(_p(ll), _p(params), _p(ll_hat), _p16(sym, off), _p16(idx, off),
                                             ll.numel(), ll.shape[0] if ar_order else 0, float(lmin), float(lstep),
                                             _stream()), "ll_quant")
    return ll_hat


def planes_to_u8(x, h, w):
    """decoder output stage: padded planes (N,1,Hp,Wp) float32 -> cropped (N,h,w) uint8, round-half-even of clamp(x, 0, 255)"""
    N, _, Hp, Wp = x.shape
    out = torch.empty((N, h, w), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.hip().pmctf_planes_to_u8(_p(x), C.c_void_p(out.data_ptr()), N, Hp, Wp, int(h), int(w), _stream()),
               "planes_to_u8")
    return out


def _pi16(t):
    assert t.is_cuda and t.dtype == torch.int16 and t.is_contiguous()
    return C.c_void_p(t.data_ptr())


def fourstep_indexes(params, N, H, W, k, lmin, lstep):
    idx = torch.empty(N * H * W, dtype=torch.int16, device=params.device)
    sub = 0 if params.shape[1] == H else 1
    _lib.check(_lib.hip().pmctf_fourstep_indexes_f32(_p(params), _pi16(idx), N, H, W, k, sub, float(lmin), float(lstep),
                                                     _stream()), "fourstep_indexes")
    return idx


def fourstep_dequant(sym, params, so_far, k):
    N, _, H, W = so_far.shape
    sub = 0 if params.shape[1] == H else 1
    _lib.check(_lib.hip().pmctf_fourstep_dequant_f32(_pi16(sym), _p(params), _p(so_far), N, H, W, k, sub, _stream()),
               "fourstep_dequant")


def mv_fourpart_indexes(common, sp, H, W, t, lmin, lstep):
    idx = torch.empty(16 * H * W, dtype=torch.int16, device=common.device)
    _lib.check(_lib.hip().pmctf_mv_fourpart_indexes_f32(_p(common), _p(sp), _pi16(idx), H, W, t, float(lmin),
                                                        float(lstep), _stream()), "mv_fourpart_indexes")
    return idx


def mv_fourpart_dequant(sym, common, sp, so_far, t):
    _, H, W, _ = so_far.shape
    _lib.check(_lib.hip().pmctf_mv_fourpart_dequant_f32(_pi16(sym), _p(common), _p(sp), _p(so_far), H, W, t, _stream()),
               "mv_fourpart_dequant")


def sym_to_nhwc(sym, H, W, Cc):
    out = torch.empty((1, H, W, Cc), dtype=torch.float32, device=sym.device)
    _lib.check(_lib.hip().pmctf_sym_to_nhwc_f32(_pi16(sym), _p(out), H * W, Cc, _stream()), "sym_to_nhwc")
    return out


def z_symbols(z, sym, idx, off):
    N, H, W, Cc = z.shape
    z_hat = torch.empty_like(z)
    _lib.check(_lib.hip().pmctf_z_symbols_f32(_p(z), _p(z_hat), _p16(sym, off), _p16(idx, off), H * W, Cc, _stream()),
               "z_symbols")
    return z_hat


def mv_fourpart_step(y, common, sp, so_far, sym, idx, off, t, lmin, lstep):
    N, H, W, Cc = y.shape
    assert N == 1 and Cc == 64
    _lib.check(_lib.hip().pmctf_mv_fourpart_step_f32(_p(y), _p(common), _p(sp), _p(so_far), _p16(sym, off),
                                                     _p16(idx, off), H, W, t, float(lmin), float(lstep), _stream()),
               "mv_fourpart_step")


def mv_dequant(so_far, common):
    y_hat = torch.empty_like(so_far)
    _lib.check(_lib.hip().pmctf_mv_dequant_f32(_p(so_far), _p(common), _p(y_hat), so_far.shape[1] * so_far.shape[2],
                                               _stream()), "mv_dequant")
    return y_hat


# ------------------------------------------------------------------------------------------------
# estimate mode (bit estimates / squared errors accumulate into device float64 tensors)
def _pd(t):
    assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
    return C.c_void_p(t.data_ptr())


def fourstep_estimate(x, params, so_far, k, bits):
    N, _, H, W = x.shape
    sub = 0 if params.shape[1] == H else 1
    assert params.shape[1] * (1 + sub) == H and params.shape[2] * (1 + sub) == W and bits.numel() == N
    _lib.check(_lib.hip().pmctf_fourstep_estimate_f32(_p(x), _p(params), _p(so_far), N, H, W, k, sub, _pd(bits),
                                                      _stream()), "fourstep_estimate")


def ll_estimate(ll_hat, params, bits):
    N, _, H, W = ll_hat.shape
    assert bits.numel() == N
    _lib.check(_lib.hip().pmctf_ll_estimate_f32(_p(ll_hat), _p(params), N, H * W, _pd(bits), _stream()), "ll_estimate")


def z_estimate(z, consts, bits):
    N, H, W, Cc = z.shape
    assert N == 1 and tuple(consts.shape) == (11, Cc)
    z_hat = torch.empty_like(z)
    _lib.check(_lib.hip().pmctf_z_estimate_f32(_p(z), _p(z_hat), _p(consts), H * W, Cc, _pd(bits), _stream()), "z_estimate")
    return z_hat


def mv_fourpart_estimate(y, common, sp, so_far, t, bits):
    N, H, W, Cc = y.shape
    assert N == 1 and Cc == 64
    _lib.check(_lib.hip().pmctf_mv_fourpart_estimate_f32(_p(y), _p(common), _p(sp), _p(so_far), H, W, t, _pd(bits),
                                                         _stream()), "mv_fourpart_estimate")


def sqdiff_sum(a, b, acc):
    assert a.shape == b.shape and a.is_contiguous() and b.is_contiguous()
    _lib.check(_lib.hip().pmctf_sqdiff_sum_f32(_p(a), _p(b), a.numel(), _pd(acc), _stream()), "sqdiff_sum")


# ------------------------------------------------------------------------------------------------
# picture quality (csrc/quality_ops.hip)
MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MSSSIM_MIN_SIDE = 160                   # (11 - 1) * 2^4: the smaller side must exceed it
QUALITY_FRONT_FLOATS, QUALITY_OUT_DOUBLES = 8192, 34        # PMCTF_QUALITY_* of include/pmctf_hip.h


def msssim_from_means(means):
    """means[s][c] = (mean cs, mean ssim) of scale s, channel c -> MS-SSIM: per channel the product of relu(cs_s)^w_s over
    scales 0..3 and relu(ssim_4)^w_4, then the mean over the channels; float64 on the host"""
    total = 0.0
    for c in range(3):
        v = 1.0
        for s, wgt in enumerate(MSSSIM_WEIGHTS):
            v *= max(float(means[s][c][1 if s == len(MSSSIM_WEIGHTS) - 1 else 0]), 0.0) ** wgt
        total += v
    return total / 3.0


def _psnr_from_sse(sse, n):
    import math
    return math.inf if sse == 0 else 10.0 * math.log10(255.0 ** 2 * n / sse)


def frame_quality(rec_y, rec_c, org_y, org_c, h, w, msssim=True, return_means=False):
    """Quality of one reconstructed frame as the harness reports it (test_pMCTF_flex.py:293-327): rec_y (1,1,Hp,Wp) /
    rec_c (2,1,Hp/2,Wp/2) padded, neither clamped nor rounded; org_y (1,1,h,w) / org_c (2,1,h/2,w/2) the originals.
    -> {"y","cb","cr","yuv","rgb": PSNR in dB (inf for identical pictures), "msssim", "sse": (Y, Cb, Cr, RGB) ints}.
    msssim: 0.0 when not asked for or when min(h, w) <= 128 (the harness's own guard); ValueError for
    128 < min(h, w) <= 160, where five scales do not fit.  One device->host copy.  return_means adds "means"
    [5][3][2] (scale, channel, (cs, ssim)), None without MS-SSIM."""
    h, w = int(h), int(w)
    rec_y, rec_c, org_y, org_c = (t.contiguous() for t in (rec_y, rec_c, org_y, org_c))
    Hp, Wp = rec_y.shape[-2:]
    if h <= 0 or w <= 0 or (h | w) & 1 or h > Hp or w > Wp:
        raise ValueError(f"picture size {h}x{w} must be even, positive and inside the padded {Hp}x{Wp}")
    if tuple(rec_c.shape) != (2, 1, Hp // 2, Wp // 2) or tuple(org_y.shape[-2:]) != (h, w) or \
            tuple(org_c.shape) != (2, 1, h // 2, w // 2) or rec_y.numel() != Hp * Wp or org_y.numel() != h * w:
        raise ValueError("expect luma (1,1,Hp,Wp) / chroma (2,1,Hp/2,Wp/2) reconstructions and un-padded originals")
    with_ms = bool(msssim) and min(h, w) > 128
    if with_ms and min(h, w) <= MSSSIM_MIN_SIDE:
        raise ValueError(f"MS-SSIM with five scales needs a smaller side above {MSSSIM_MIN_SIDE}, got {h}x{w}")
    L = _lib.hip()
    n_scratch = L.pmctf_msssim_scratch_floats(h, w) if with_ms else QUALITY_FRONT_FLOATS
    scratch = torch.empty(n_scratch, dtype=torch.float32, device=rec_y.device)
    out = torch.empty(QUALITY_OUT_DOUBLES, dtype=torch.float64, device=rec_y.device)
    _lib.check(L.pmctf_frame_quality_f32(_p(rec_y), _p(rec_c), _p(org_y), _p(org_c), Hp, Wp, h, w, int(with_ms),
                                         _p(scratch), _pd(out), _stream()), "frame_quality")
    host = out.cpu().tolist()                               # the frame's one copy to the host
    sse = tuple(int(v) for v in host[:4])
    assert all(float(s) == v for s, v in zip(sse, host[:4])), "squared-error sums are integers"
    n = h * w
    res = {"y": _psnr_from_sse(sse[0], n), "cb": _psnr_from_sse(sse[1], n // 4), "cr": _psnr_from_sse(sse[2], n // 4),
           "rgb": _psnr_from_sse(sse[3], 3 * n), "sse": sse}
    res["yuv"] = (6.0 * res["y"] + res["cb"] + res["cr"]) / 8.0
    means = [[(host[4 + 6 * s + 2 * c], host[5 + 6 * s + 2 * c]) for c in range(3)] for s in range(5)] if with_ms else None
    res["msssim"] = msssim_from_means(means) if with_ms else 0.0
    if return_means:
        res["means"] = means
    return res


# ------------------------------------------------------------------------------------------------
# pictures in and out (csrc/picture_ops.hip); 16-bit samples travel as torch.uint16
PICTURE_MAX_SIDE = 16384


def _pu8(t):
    if t is None:
        return None
    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous(), "expect dense uint8 device tensor"
    return C.c_void_p(t.data_ptr())


def _picture_size(h, w):
    h, w = int(h), int(w)
    if h <= 0 or w <= 0 or (h | w) & 1 or max(h, w) > PICTURE_MAX_SIDE:
        raise ValueError(f"4:2:0 pictures have even, positive sizes up to {PICTURE_MAX_SIDE} (got {h}x{w})")
    return h, w


def frame_to_rgb8(rec_y, rec_c, h, w):
    """One reconstructed frame as the harness saves it (test_pMCTF_flex.py:76-79,301-317): rec_y (1,1,Hp,Wp) / rec_c
    (2,1,Hp/2,Wp/2) padded float32, neither clamped nor rounded -> (h, w, 3) uint8 device tensor, the rounded RGB picture
    of frame_quality clipped to 0..255.  One launch."""
    h, w = _picture_size(h, w)
    for t in (rec_y, rec_c):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError("expect float32 tensors")
    rec_y, rec_c = rec_y.contiguous(), rec_c.contiguous()
    Hp, Wp = rec_y.shape[-2:]
    if (Hp | Wp) & 1 or h > Hp or w > Wp:
        raise ValueError(f"picture size {h}x{w} must lie inside the even padded size {Hp}x{Wp}")
    if rec_y.numel() != Hp * Wp or tuple(rec_c.shape) != (2, 1, Hp // 2, Wp // 2):
        raise ValueError("expect a luma (1,1,Hp,Wp) and a chroma (2,1,Hp/2,Wp/2) reconstruction")
    _dev(rec_y), _dev(rec_c)
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=rec_y.device)
    _lib.check(_lib.hip().pmctf_yuv420_to_rgb8_f32(_p(rec_y), _p(rec_c), _pu8(out), Hp, Wp, h, w, _stream()), "frame_to_rgb8")
    return out


def _planes_from(frame, h, w, bitdepth, psize, originals):
    """the body of planes_from_u8 (bitdepth None: bytes) and planes_from_u16 (9..16: 16-bit samples)"""
    from ..utils.stream_helper import get_padding_size
    h, w = _picture_size(h, w)
    dtype, word, unit = (torch.uint8, "uint8", "bytes") if bitdepth is None else (torch.uint16, "uint16", "samples")
    if bitdepth is not None:
        bitdepth = _bitdepth(bitdepth)
    psize = int(psize)
    if psize <= 0 or psize & 1:
        raise ValueError(f"psize must be even and positive (got {psize})")
    if not isinstance(frame, torch.Tensor) or frame.dtype != dtype:
        raise ValueError(f"expect a {word} tensor")
    if frame.numel() != h * w * 3 // 2:
        raise ValueError(f"a {h}x{w} 4:2:0 picture has {h * w * 3 // 2} {unit}, got {frame.numel()}")
    dev = _dev(frame)
    frame = frame.contiguous()
    _, right, _, bottom = get_padding_size(h, w, p=psize)
    Hp, Wp = h + bottom, w + right
    if max(Hp, Wp) > PICTURE_MAX_SIDE:
        raise ValueError(f"padded size {Hp}x{Wp} exceeds {PICTURE_MAX_SIDE}")
    y_pad = torch.empty((1, 1, Hp, Wp), dtype=torch.float32, device=dev)
    c_pad = torch.empty((2, 1, Hp // 2, Wp // 2), dtype=torch.float32, device=dev)
    y_org = torch.empty((1, 1, h, w), dtype=torch.float32, device=dev) if originals else None
    c_org = torch.empty((2, 1, h // 2, w // 2), dtype=torch.float32, device=dev) if originals else None
    planes = (_p(y_pad), _p(c_pad), _p(y_org), _p(c_org), Hp, Wp, h, w)
    if bitdepth is None:
        _lib.check(_lib.hip().pmctf_yuv420_u8_to_planes_f32(_pu8(frame), *planes, _stream()), "planes_from_u8")
    else:
        _lib.check(_lib.hip().pmctf_yuv420_u16_to_planes_f32(_pu16(frame), *planes, bitdepth, _stream()), "planes_from_u16")
    return y_pad, c_pad, y_org, c_org


def planes_from_u8(frame_u8, h, w, psize=128, originals=True):
    """One picture as it lies in a planar 8-bit 4:2:0 file (uint8 device tensor of h*w*3/2 bytes) -> (y_pad (1,1,Hp,Wp),
    c_pad (2,1,Hp/2,Wp/2), y_org (1,1,h,w), c_org (2,1,h/2,w/2)) float32: the model's inputs, zero padded right / bottom to
    multiples of psize, and the un-padded originals (None, None with originals=False).  One launch; the counterpart of
    planes_to_u8."""
    return _planes_from(frame_u8, h, w, None, psize, originals)


def planes_from_u16(frame_u16, h, w, bitdepth, psize=128, originals=True):
    """planes_from_u8 for one picture of a planar 4:2:0 file of `bitdepth` 9..16 (uint16 device tensor of h*w*3/2 samples,
    as little-endian words lie in the file): every sample v becomes v * 2^-(bitdepth - 8), exactly, so the planes keep the
    codec's 0..255 range.  -> (y_pad, c_pad, y_org, c_org) float32 as planes_from_u8.  One launch; the counterpart of
    planes_to_u16."""
    return _planes_from(frame_u16, h, w, bitdepth, psize, originals)


def planes_from(frame, h, w, bitdepth=8, psize=128, originals=True):
    """planes_from_u8 at bitdepth 8, planes_from_u16 above: with planes_to, the one place that chooses by depth"""
    return _planes_from(frame, h, w, None if bitdepth == 8 else bitdepth, psize, originals)


def planes_to(x, h, w, bitdepth=8):
    """planes_to_u8 at bitdepth 8, planes_to_u16 above"""
    return planes_to_u8(x, h, w) if bitdepth == 8 else planes_to_u16(x, h, w, bitdepth)


def rgb8_to_yuv420(rgb_u8):
    """(h, w, 3) uint8 RGB device tensor -> uint8 device tensor of h*w*3/2 bytes, one planar 4:2:0 picture in the file
    layout: rgb2ycbcr (pMCTF/utils/util.py:21-40) in float32, 2x2 mean of the unrounded chroma, round half to even."""
    if not isinstance(rgb_u8, torch.Tensor) or rgb_u8.dtype != torch.uint8:
        raise ValueError("expect a uint8 tensor")
    if rgb_u8.dim() != 3 or rgb_u8.shape[2] != 3:
        raise ValueError(f"expect an (h, w, 3) picture, got {tuple(rgb_u8.shape)}")
    h, w = _picture_size(rgb_u8.shape[0], rgb_u8.shape[1])
    dev = _dev(rgb_u8)
    rgb_u8 = rgb_u8.contiguous()
    out = torch.empty(h * w * 3 // 2, dtype=torch.uint8, device=dev)
    _lib.check(_lib.hip().pmctf_rgb8_to_yuv420_u8(_pu8(rgb_u8), _pu8(out), h, w, _stream()), "rgb8_to_yuv420")
    return out


# ------------------------------------------------------------------------------------------------
# high-bit-depth pictures: the uint16_t instantiations of csrc/picture_ops.hip, the error sums of csrc/picture_hbd.hip
HBD_MIN, HBD_MAX = 9, 16


def _pu16(t):
    assert t.is_cuda and t.dtype == torch.uint16 and t.is_contiguous(), "expect dense uint16 device tensor"
    return C.c_void_p(t.data_ptr())


def _bitdepth(bitdepth):
    b = int(bitdepth)
    if not HBD_MIN <= b <= HBD_MAX:
        raise ValueError(f"a 16-bit sample holds a bitdepth of {HBD_MIN}..{HBD_MAX} (got {bitdepth})")
    return b


def planes_to_u16(x, h, w, bitdepth):
    """planes_to_u8 for a `bitdepth` of 9..16: padded planes (N,1,Hp,Wp) float32 -> cropped (N,h,w) uint16,
    rint(clamp(x * 2^(bitdepth - 8), 0, 2^bitdepth - 1)), ties to even, NaN -> 0.  One launch."""
    bitdepth = _bitdepth(bitdepth)
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 1:
        raise ValueError("expect a float32 tensor of planes (N,1,Hp,Wp)")
    N, _, Hp, Wp = x.shape
    h, w = int(h), int(w)
    if h <= 0 or w <= 0 or h > Hp or w > Wp or max(Hp, Wp) > PICTURE_MAX_SIDE:
        raise ValueError(f"plane size {h}x{w} must be positive and inside the padded {Hp}x{Wp} (at most {PICTURE_MAX_SIDE})")
    dev = _dev(x)
    out = torch.empty((N, h, w), dtype=torch.uint16, device=dev)
    _lib.check(_lib.hip().pmctf_planes_to_u16(_p(x.contiguous()), _pu16(out), N, Hp, Wp, h, w, bitdepth, _stream()),
               "planes_to_u16")
    return out


def psnr_from_sse_hbd(sse, n, bitdepth):
    """10 log10(max^2 n / sse) with max = 2^bitdepth - 1, float64 on the host; inf for sse == 0"""
    import math
    return math.inf if sse == 0 else 10.0 * math.log10(float((1 << bitdepth) - 1) ** 2 * n / sse)


def frame_sse_hbd(rec_y, rec_c, org_y, org_c, h, w, bitdepth):
    """Quality of one reconstructed frame at `bitdepth` 9..16 bits: rec_y (1,1,Hp,Wp) / rec_c (2,1,Hp/2,Wp/2) padded, neither
    clamped nor rounded; org_y (1,1,h,w) / org_c (2,1,h/2,w/2) the originals as planes_from_u16 / read_gop return them.
    Both are taken back to `bitdepth`-bit integers (planes_to_u16's rounding for the reconstruction) and the squared
    differences are summed in 64-bit integers on the device.
    -> {"y","cb","cr","yuv": PSNR in dB against 2^bitdepth - 1 (inf for identical planes), "sse": (Y, Cb, Cr) ints}.
    One launch and one device->host copy."""
    h, w = int(h), int(w)
    bitdepth = _bitdepth(bitdepth)
    for t in (rec_y, rec_c, org_y, org_c):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError("expect float32 tensors")
    rec_y, rec_c, org_y, org_c = (t.contiguous() for t in (rec_y, rec_c, org_y, org_c))
    Hp, Wp = rec_y.shape[-2:]
    if h <= 0 or w <= 0 or (h | w) & 1 or h > Hp or w > Wp or (Hp | Wp) & 1 or max(Hp, Wp) > PICTURE_MAX_SIDE:
        raise ValueError(f"picture size {h}x{w} must be even, positive and inside the even padded {Hp}x{Wp}")
    if tuple(rec_c.shape) != (2, 1, Hp // 2, Wp // 2) or tuple(org_y.shape[-2:]) != (h, w) or \
            tuple(org_c.shape) != (2, 1, h // 2, w // 2) or rec_y.numel() != Hp * Wp or org_y.numel() != h * w:
        raise ValueError("expect luma (1,1,Hp,Wp) / chroma (2,1,Hp/2,Wp/2) reconstructions and un-padded originals")
    dev = _dev(rec_y)
    for t in (rec_c, org_y, org_c):
        _dev(t)
    out = torch.empty(3, dtype=torch.int64, device=dev)
    _lib.check(_lib.hip().pmctf_frame_sse_u16_f32(_p(rec_y), _p(rec_c), _p(org_y), _p(org_c), Hp, Wp, h, w, bitdepth,
                                                  C.c_void_p(out.data_ptr()), _stream()), "frame_sse_hbd")
    sse = tuple(v & 0xffffffffffffffff for v in out.cpu().tolist())          # the frame's one copy to the host
    n = h * w
    res = {"y": psnr_from_sse_hbd(sse[0], n, bitdepth), "cb": psnr_from_sse_hbd(sse[1], n // 4, bitdepth),
           "cr": psnr_from_sse_hbd(sse[2], n // 4, bitdepth), "sse": sse}
    res["yuv"] = (6.0 * res["y"] + res["cb"] + res["cr"]) / 8.0
    return res


# ------------------------------------------------------------------------------------------------
# resampling of packed 4:2:0 pictures (csrc/picture_scale.hip)
def resize_yuv420(frame, h_in, w_in, h_out, w_out, tables, taps, bitdepth=8):
    """One packed planar 4:2:0 picture (uint8 device tensor of h_in*w_in*3/2 bytes at bitdepth 8, uint16 of as many samples
    at 9..16) -> the packed picture of h_out x w_out, same type: the integer Catmull-Rom resampling of DESIGN 5l.
    tables: the four axis tables (luma x, luma y, chroma x, chroma y) as uint8 device tensors in the layout
    pmctf_scale.device_table uploads, taps: their four tap counts.  One launch."""
    h_in, w_in = _picture_size(h_in, w_in)
    h_out, w_out = _picture_size(h_out, w_out)
    bitdepth = int(bitdepth)
    dtype = torch.uint8 if bitdepth == 8 else torch.uint16
    if bitdepth != 8:
        _bitdepth(bitdepth)
    if 4 * h_out < h_in or h_out > 4 * h_in or 4 * w_out < w_in or w_out > 4 * w_in:
        raise ValueError(f"{h_in}x{w_in} -> {h_out}x{w_out}: the sizes differ by more than a factor of 4 on an axis")
    if not isinstance(frame, torch.Tensor) or frame.dtype != dtype:
        raise ValueError(f"expect a {dtype} tensor at bitdepth {bitdepth}")
    if frame.numel() != h_in * w_in * 3 // 2:
        raise ValueError(f"a {h_in}x{w_in} 4:2:0 picture has {h_in * w_in * 3 // 2} samples, got {frame.numel()}")
    dev = _dev(frame)
    frame = frame.contiguous()
    taps = [int(t) for t in taps]
    if len(tables) != 4 or len(taps) != 4:
        raise ValueError("expect four tables and four tap counts: luma x, luma y, chroma x, chroma y")
    for t, n_out, n in zip(tables, (w_out, h_out, w_out // 2, h_out // 2), taps):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not 1 <= n <= 20 or t.numel() != n_out * (4 + 2 * n):
            raise ValueError(f"a table of {n_out} rows of {n} taps is a uint8 tensor of {n_out * (4 + 2 * n)} bytes, 1..20 taps")
        if _dev(t) != dev:
            raise ValueError("the tables live on the picture's device")
    out = torch.empty(h_out * w_out * 3 // 2, dtype=dtype, device=dev)
    fn = _lib.hip().pmctf_resize_yuv420_u8 if bitdepth == 8 else _lib.hip().pmctf_resize_yuv420_u16
    _lib.check(fn((_pu8 if bitdepth == 8 else _pu16)(frame), C.c_void_p(out.data_ptr()), h_in, w_in, h_out, w_out,
                  *(_pu8(t.contiguous()) for t in tables), (C.c_int * 4)(*taps), bitdepth, _stream()), "resize_yuv420")
    return out


# ------------------------------------------------------------------------------------------------
# chroma format conversion of packed pictures (csrc/picture_chroma.hip)
CHROMA_SUBSAMPLING = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}            # format -> (sx, sy)


def chroma_frame_samples(h, w, fmt):
    """samples of one packed h x w picture of chroma format "420", "422" or "444" """
    if fmt not in CHROMA_SUBSAMPLING:
        raise ValueError(f"a chroma format is one of {sorted(CHROMA_SUBSAMPLING)} (got {fmt!r})")
    sx, sy = CHROMA_SUBSAMPLING[fmt]
    return h * w + 2 * (h // sy) * (w // sx)


def convert_chroma(frame, h, w, fmt_in, fmt_out, tables, taps, bitdepth=8):
    """One packed planar h x w picture of chroma format fmt_in ("420", "422", "444"; uint8 device tensor at bitdepth 8,
    uint16 at 9..16) -> the packed picture of fmt_out, same type: Y copied, Cb and Cr through the integer filter of DESIGN
    5l / 5m.  tables: the chroma planes' x and y axis tables as uint8 device tensors in the layout
    pmctf_scale.device_table uploads (pmctf_chroma.chroma_tables), taps: their two tap counts.  One launch."""
    h, w = _picture_size(h, w)
    bitdepth = int(bitdepth)
    dtype = torch.uint8 if bitdepth == 8 else torch.uint16
    if bitdepth != 8:
        _bitdepth(bitdepth)
    n_in, n_out = chroma_frame_samples(h, w, fmt_in), chroma_frame_samples(h, w, fmt_out)
    if not isinstance(frame, torch.Tensor) or frame.dtype != dtype:
        raise ValueError(f"expect a {dtype} tensor at bitdepth {bitdepth}")
    if frame.numel() != n_in:
        raise ValueError(f"a {h}x{w} {fmt_in} picture has {n_in} samples, got {frame.numel()}")
    dev = _dev(frame)
    frame = frame.contiguous()
    taps = [int(t) for t in taps]
    if len(tables) != 2 or len(taps) != 2:
        raise ValueError("expect two tables and two tap counts: chroma x, chroma y")
    (sx, sy) = CHROMA_SUBSAMPLING[fmt_out]
    for t, rows, n in zip(tables, (w // sx, h // sy), taps):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not 1 <= n <= 17 or t.numel() != rows * (4 + 2 * n):
            raise ValueError(f"a table of {rows} rows of {n} taps is a uint8 tensor of {rows * (4 + 2 * n)} bytes, 1..17 taps")
        if _dev(t) != dev:
            raise ValueError("the tables live on the picture's device")
    out = torch.empty(n_out, dtype=dtype, device=dev)
    fn = _lib.hip().pmctf_convert_chroma_u8 if bitdepth == 8 else _lib.hip().pmctf_convert_chroma_u16
    _lib.check(fn((_pu8 if bitdepth == 8 else _pu16)(frame), C.c_void_p(out.data_ptr()), h, w, int(fmt_in), int(fmt_out),
                  *(_pu8(t.contiguous()) for t in tables), (C.c_int * 2)(*taps), bitdepth, _stream()), "convert_chroma")
    return out


# ------------------------------------------------------------------------------------------------
# pixel layouts (csrc/picture_layout.hip)
# name -> (PMCTF_LAYOUT_* code, chroma format, bitdepth, container bytes, family)
LAYOUTS = {
    "nv12": (1, "420", 8, 1, "semi"), "nv21": (2, "420", 8, 1, "semi"), "nv16": (3, "422", 8, 1, "semi"),
    "p010": (4, "420", 10, 2, "semi"), "p012": (5, "420", 12, 2, "semi"), "p016": (6, "420", 16, 2, "semi"),
    "p210": (7, "422", 10, 2, "semi"), "p212": (8, "422", 12, 2, "semi"), "p216": (9, "422", 16, 2, "semi"),
    "yuyv": (10, "422", 8, 1, "pair"), "uyvy": (11, "422", 8, 1, "pair"),
    "y210": (12, "422", 10, 2, "pair"), "y212": (13, "422", 12, 2, "pair"), "y216": (14, "422", 16, 2, "pair"),
    "v210": (15, "422", 10, 4, "v210"),
}
LAYOUT_MAX_PITCH = 1 << 20
LAYOUT_MAX_LUMA_ROWS = 1 << 17


def layout_row_bytes(layout, w):
    """bytes of one row of a picture of width w in `layout`, without pitch padding (a v210 row ends on 128 bytes)"""
    _, _, _, container, family = LAYOUTS[layout]
    if family == "v210":
        return (w + 47) // 48 * 128
    return (2 if family == "pair" else 1) * w * container


def layout_geometry(layout, h, w, bitdepth=None, pitch=None, luma_rows=None):
    """-> (pitch, luma_rows, frame_bytes) of an h x w picture in `layout`, the defaults filled in (pitch: the row's bytes,
    luma_rows: h); frame_bytes is the offset of the last row's end.  ValueError naming the argument for an unknown layout,
    a bitdepth that is not the layout's, a pitch that is no multiple of the container, below the row's bytes or above
    2^20, luma_rows below h or above 2^17."""
    if layout not in LAYOUTS:
        raise ValueError(f"pixel_layout is one of {sorted(LAYOUTS)} (got {layout!r})")
    h, w = _picture_size(h, w)
    _, fmt, depth, container, family = LAYOUTS[layout]
    if bitdepth is not None and bitdepth != depth:
        raise ValueError(f"bitdepth {bitdepth!r} contradicts pixel_layout {layout!r}, which has {depth} bits")
    row = layout_row_bytes(layout, w)
    if pitch is None:
        pitch = row
    if isinstance(pitch, bool) or not isinstance(pitch, int) or pitch % container or not row <= pitch <= LAYOUT_MAX_PITCH:
        raise ValueError(f"pitch is a multiple of {container} bytes from {row} (a {layout} row of {w} pixels) to "
                         f"{LAYOUT_MAX_PITCH} (got {pitch!r})")
    if luma_rows is None:
        luma_rows = h
    if isinstance(luma_rows, bool) or not isinstance(luma_rows, int) or not h <= luma_rows <= LAYOUT_MAX_LUMA_ROWS:
        raise ValueError(f"luma_rows is {h} (the height) to {LAYOUT_MAX_LUMA_ROWS} (got {luma_rows!r})")
    if family == "semi":
        hc = h // CHROMA_SUBSAMPLING[fmt][1]
        return pitch, luma_rows, pitch * luma_rows + (hc - 1) * pitch + row
    return pitch, luma_rows, (h - 1) * pitch + row


def _layout_call(kind, planar, surface, layout, h, w, bitdepth, pitch, luma_rows):
    code, _, depth, _, _ = LAYOUTS[layout]
    args = (_ptr_of(surface), _ptr_of(planar)) if kind == "unpack" else (_ptr_of(planar), _ptr_of(surface))
    if depth == 8:
        fn = getattr(_lib.hip(), f"pmctf_{kind}_layout_u8")
        rc = fn(*args, code, h, w, pitch, luma_rows, _stream())
    else:
        fn = getattr(_lib.hip(), f"pmctf_{kind}_layout_u16")
        rc = fn(*args, code, h, w, depth, pitch, luma_rows, _stream())
    _lib.check(rc, f"{kind}_layout({layout})")


def _ptr_of(t):
    assert t.is_cuda and t.is_contiguous(), "expect a dense device tensor"
    return C.c_void_p(t.data_ptr())


def _check_surface(surface, need, what):
    if not isinstance(surface, torch.Tensor) or surface.dtype != torch.uint8 or surface.dim() != 1 or \
            not surface.is_contiguous():
        raise ValueError(f"{what}: a surface is a dense 1-D uint8 tensor")
    if surface.numel() < need:
        raise ValueError(f"{what}: the surface has {surface.numel()} bytes, the picture needs {need}")


def unpack_layout(surface, layout, h, w, bitdepth=None, pitch=None, luma_rows=None, out=None):
    """One picture as a surface or a capture file holds it (1-D uint8 device tensor of at least frame_bytes bytes, see
    layout_geometry) -> the packed planar picture of the layout's chroma format (uint8 at 8 bits, uint16 above; Y, Cb, Cr,
    tight, low-bit-aligned).  out: a dense tensor of that type and size to write into.  One launch."""
    pitch, luma_rows, need = layout_geometry(layout, h, w, bitdepth, pitch, luma_rows)
    _, fmt, depth, container, _ = LAYOUTS[layout]
    _check_surface(surface, need, "unpack_layout")
    dev = _dev(surface)
    if surface.data_ptr() % container:
        raise ValueError(f"unpack_layout: a {layout} surface is aligned to {container} bytes")
    dtype, n = torch.uint8 if depth == 8 else torch.uint16, chroma_frame_samples(h, w, fmt)
    if out is None:
        out = torch.empty(n, dtype=dtype, device=dev)
    elif not isinstance(out, torch.Tensor) or out.dtype != dtype or out.numel() != n or not out.is_contiguous() or \
            _dev(out) != dev:
        raise ValueError(f"unpack_layout: out is a dense {dtype} tensor of {n} samples on the surface's device")
    _layout_call("unpack", out, surface, layout, h, w, depth, pitch, luma_rows)
    return out


def pack_layout(frame, layout, h, w, bitdepth=None, pitch=None, luma_rows=None, out=None):
    """The inverse of unpack_layout: a packed planar picture -> its surface (1-D uint8 device tensor of frame_bytes bytes).
    out: a dense 1-D uint8 tensor of at least frame_bytes bytes to write into; what lies between a row's end and the pitch,
    between the planes and after the picture is left as it is.  Without out, such bytes are zero.  One launch."""
    pitch, luma_rows, need = layout_geometry(layout, h, w, bitdepth, pitch, luma_rows)
    _, fmt, depth, container, _ = LAYOUTS[layout]
    dtype, n = torch.uint8 if depth == 8 else torch.uint16, chroma_frame_samples(h, w, fmt)
    if not isinstance(frame, torch.Tensor) or frame.dtype != dtype or frame.numel() != n:
        raise ValueError(f"pack_layout: a {h}x{w} {layout} picture is a {dtype} tensor of {n} samples")
    dev = _dev(frame)
    frame = frame.contiguous()
    if out is None:
        tight = pitch == layout_row_bytes(layout, w) and luma_rows == h
        out = (torch.empty if tight else torch.zeros)(need, dtype=torch.uint8, device=dev)
    else:
        _check_surface(out, need, "pack_layout")
        if _dev(out) != dev:
            raise ValueError("pack_layout: out lives on the picture's device")
    if out.data_ptr() % container:
        raise ValueError(f"pack_layout: a {layout} surface is aligned to {container} bytes")
    _layout_call("pack", frame, out, layout, h, w, depth, pitch, luma_rows)
    return out


# ------------------------------------------------------------------------------------------------
# sequence structure pre-analysis (csrc/scene_ops.hip)
def luma_activity(cur, prev, bitdepth=8, hist=None, sad=None):
    """The luma histogram of one picture and its sum of absolute differences against the previous one, in integers at
    `bitdepth` 8..16 bits (pmctf_luma_activity_f32).  cur, prev: un-padded luma originals (1,1,h,w) float32 as
    planes_from_u8 / planes_from_u16 return them; prev may be None.
    -> (hist: 256 int32 counts of min(v >> (bitdepth - 8), 255), sad: one int64 or None without a prev), device tensors;
    nothing is copied to the host.  hist / sad: caller-supplied outputs (a contiguous int32 slice of 256 values, a
    contiguous int64 slice of one), so that a run of pictures is read back with one copy.  One launch and its clears."""
    b = int(bitdepth)
    if not 8 <= b <= HBD_MAX:
        raise ValueError(f"bitdepth is 8..{HBD_MAX} (got {bitdepth})")
    for t in (cur,) if prev is None else (cur, prev):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError("expect float32 tensors")
    if cur.dim() < 2 or cur.numel() != cur.shape[-2] * cur.shape[-1]:
        raise ValueError(f"expect one luma plane (1,1,h,w), got {tuple(cur.shape)}")
    h, w = int(cur.shape[-2]), int(cur.shape[-1])
    if not (1 <= h <= PICTURE_MAX_SIDE and 1 <= w <= PICTURE_MAX_SIDE):
        raise ValueError(f"plane sides are 1..{PICTURE_MAX_SIDE} (got {h}x{w})")
    if prev is not None and tuple(prev.shape) != tuple(cur.shape):
        raise ValueError(f"the previous picture is {tuple(prev.shape)}, this one {tuple(cur.shape)}")
    dev = _dev(cur)
    cur = cur.contiguous()
    if prev is not None:
        _dev(prev)
        prev = prev.contiguous()
    if hist is None:
        hist = torch.empty(256, dtype=torch.int32, device=dev)
    elif not (isinstance(hist, torch.Tensor) and hist.is_cuda and hist.dtype == torch.int32 and hist.is_contiguous()
              and hist.numel() == 256):
        raise ValueError("hist: a contiguous int32 device tensor of 256 values")
    if prev is None:
        if sad is not None:
            raise ValueError("sad: there is no sum without a previous picture")
    elif sad is None:
        sad = torch.empty(1, dtype=torch.int64, device=dev)
    elif not (isinstance(sad, torch.Tensor) and sad.is_cuda and sad.dtype == torch.int64 and sad.is_contiguous()
              and sad.numel() == 1):
        raise ValueError("sad: a contiguous int64 device tensor of one value")
    _lib.check(_lib.hip().pmctf_luma_activity_f32(_p(cur), None if prev is None else _p(prev), h, w, b,
                                                  C.c_void_p(hist.data_ptr()),
                                                  None if sad is None else C.c_void_p(sad.data_ptr()), _stream()),
               "luma_activity")
    return hist, sad


CRC32_TILE_BYTES = 4096                   # PMCTF_CRC32_TILE_BYTES of include/pmctf_hip.h
CRC32_MAX_SEGMENTS = 65535


def crc32(tensors, slices=None, out=None):
    """zlib.crc32 of the bytes of every tensor of a list, as stored (any dtype, any start address), taken on the device
    (pmctf_crc32_segments): ONE call into the library for the whole list and one device->host copy of 4 bytes per tensor.
    -> [int].  An empty tensor gives 0.  ValueError for a tensor that is not contiguous or not on the device.
    slices: workgroups per tensor (a launch shape, results do not depend on it); by default from the longest tensor, eight
    tiles of CRC32_TILE_BYTES per workgroup, at most 128.  out: an int32 device tensor that receives the values (one per
    tensor; by default a new one)."""
    tensors = list(tensors)
    for t in tensors:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError("crc32 hashes device tensors (there is no CPU path: use zlib.crc32 for bytes on the host)")
        if not t.is_contiguous():
            raise ValueError(f"crc32 hashes the bytes as stored: a tensor of shape {tuple(t.shape)} and strides "
                             f"{tuple(t.stride())} is not contiguous")
    S = len(tensors)
    if S == 0:
        return []
    if S > CRC32_MAX_SEGMENTS:
        raise ValueError(f"at most {CRC32_MAX_SEGMENTS} tensors per call (got {S})")
    dev = _dev(tensors[0])
    if any(t.device != dev for t in tensors):
        raise ValueError("crc32: the tensors of one call live on one device")
    lengths = [t.numel() * t.element_size() for t in tensors]
    table = []
    for t, n in zip(tensors, lengths):
        table += [t.data_ptr() if n else 0, n]
    segs = torch.tensor(table, dtype=torch.int64).to(dev)                   # pmctf_crc_segment[S]
    if slices is None:
        slices = max(1, min(128, -(-max(lengths) // (8 * CRC32_TILE_BYTES))))
    if out is None:
        out = torch.empty(S, dtype=torch.int32, device=dev)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.int32 and out.is_contiguous()
              and out.numel() == S):
        raise ValueError(f"out: a contiguous int32 device tensor of {S} values")
    _lib.check(_lib.hip().pmctf_crc32_segments(C.c_void_p(segs.data_ptr()), S, int(slices), C.c_void_p(out.data_ptr()),
                                               _stream()), "crc32")
    return [v & 0xffffffff for v in out.cpu().tolist()]


# ------------------------------------------------------------------------------------------------
# diagnostic (csrc/math_probe.hip): the device's scalar functions on raw float32 bit patterns; never on the codec's path
PROBE_TANH, PROBE_TANH_LDS, PROBE_SIGMOID, PROBE_SIGMOID_SCALAR, PROBE_LOG, PROBE_LOG_POLY, PROBE_EXP, \
    PROBE_GLIBC_EXP, PROBE_ACT = range(9)                    # PMCTF_PROBE_* of include/pmctf_hip.h; PROBE_ACT + ACT_*


def math_probe(fn, bits=None, first_bits=0, n=None, slope=0.0, out=None, device="cuda"):
    """y[i] = fn(bits[i]) for an int32 / uint32-as-int32 device tensor `bits`, or fn(first_bits + i) (mod 2^32) for
    i < n when bits is None.  Returns a float32 tensor of n results (view its bits with .view(torch.int32))."""
    if bits is not None:
        assert bits.is_cuda and bits.dtype == torch.int32 and bits.is_contiguous() and bits.dim() == 1
        n, device = bits.numel(), bits.device
    n = int(n)
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= n
    _lib.check(_lib.hip().pmctf_math_probe_f32(int(fn), None if bits is None else C.c_void_p(bits.data_ptr()),
                                               int(first_bits) & 0xffffffff, n, _p(out), float(slope), _stream()),
               "math_probe")
    return out[:n]
