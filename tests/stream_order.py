"""Stream order under delays: the instrument (delay, window, caller-stream choice), one row per stream-taking entry point
of include/pmctf_hip.h (ROWS), the entries without a stream parameter (EXEMPT) and the runner of a row.

The rest of the suite compares kernels with their references on the default stream, after everything has finished; a
kernel, a clear or a copy issued on the wrong stream gives the right bytes there whenever the GPU is quick enough.  A row
makes that deterministic: the inputs are uploaded BEHIND a bounded spin on the caller's stream S, so whatever the entry
enqueues anywhere but on S runs before its inputs exist and reads the poison that the buffers held (ordinary valid data:
a second draw of the same generator).  The expected bits are the same call made on the default stream with everything
synchronised: the arithmetic is held elsewhere, this table holds order.  DESIGN 6g.

Importing this module needs neither the product nor a GPU; torch, numpy and the product are imported where used.

Delays.  One spin kernel of torch.cuda._sleep per delay, its cycle count calibrated once per process with two timing
events (no clock rate assumed); never during a stream capture; never above MAX_DELAY_MS.
  KERNEL_ENQUEUE_MS   host time from the injection point (after the delay is enqueued) to the wrapper's return, measured
                      without a delay on an MI355X host: slowest row 0.36 ms (the batched LL decode, which builds and
                      uploads its job table), conv rounds + remainder 0.09 ms, median row 0.03 ms
  KERNEL_DELAY_MS     the one delay of every kernel row.  Three times the slowest is 1.1 ms; the rows use 10 ms, since a
                      control loses its window to a single scheduler tick of the host at 1 ms and the row would then
                      fail as unexercised.  check_row asserts the factor of three against the time it measures itself.
  ENGINE_ENQUEUE_MS   the same per mode of the engine cases (tests/stream_order_cases.py): host time between
                      two injection points, undelayed: a replayed pair 28 ms, a pair by stream launches 44 ms, a stage-
                      batched GOP 110 ms, a deferred GOP 115 ms, a pair with the decoder in the loop and a GOP decode
                      150 ms.  ENGINE_DELAY_MS is three times that, capped at MAX_DELAY_MS.
"""
import ctypes as C
import time

MAX_DELAY_MS = 250.0
KERNEL_ENQUEUE_MS = 0.36
KERNEL_DELAY_MS = 10.0
# per mode of tests/stream_order_cases.py: host milliseconds between two injection points, and the delays from them
ENGINE_ENQUEUE_MS = {"pairs": 28, "plans_off": 44, "batched": 110, "lazy": 115, "decoder": 150, "decode": 150}
ENGINE_DELAY_MS = {k: min(3.0 * v, MAX_DELAY_MS) for k, v in ENGINE_ENQUEUE_MS.items()}
GUARD = 256                              # bytes of sentinel on either side of an output the test owns
SENTINEL, GARBAGE = 0x5A, 0xA5           # bytes: outputs before the run; self-cleared outputs just before the call

# exports without a stream parameter, and why no row can hold them to one
EXEMPT = {
    "pmctf_conv2d_packed_size": "host arithmetic: a size",
    "pmctf_conv2d_packed_bias_size": "host arithmetic: a size",
    "pmctf_conv2d_pack_weights": "weight packer: host pointers in, host pointers out",
    "pmctf_conv3x3_split_packed_size": "host arithmetic: a size",
    "pmctf_conv3x3_split_pack_weights": "weight packer: host pointers in, host pointers out",
    "pmctf_ll_ar_packed_size": "host arithmetic: a size",
    "pmctf_ll_ar_pack_weights": "weight packer: host pointers in, host pointers out",
    "pmctf_ll_ar_scratch_floats": "host arithmetic: a size",
    "pmctf_msssim_scratch_floats": "host arithmetic: a size",
    "pmctf_conv2d_set_option": "option setter: host state only",
    "pmctf_conv2d_get_option": "option getter: host state only",
    "pmctf_conv2d_last_launch": "*_last_launch: host text of the calling thread",
    "pmctf_valu_conv_last_launch": "*_last_launch: host text of the calling thread",
    "pmctf_ew_last_launch": "*_last_launch: host text of the calling thread",
    "pmctf_conv2d_fewcout_supported": "*_supported: a table lookup on the host",
    "pmctf_conv3x3_split_supported": "*_supported: a table lookup on the host",
    "pmctf_ll_ar_batch_form": "the batched decode's kernel choice: host arithmetic",
}


# Every wait_event / wait_stream / record_stream / Event.record / .synchronize() of an event or a stream / non-blocking
# copy of pMCTF/hip/*.py and pMCTF/models/video/pMCTF_L.py, per function: (file, function, {kind: count}, what crosses,
# the cases of tests/stream_order_cases.py that put a delay in front of it).  tests/test_stream_order_cpu.py
# holds the table to the source: a site added later without a line here fails there.  No line is unreached.
SITES = [
    ("engine.py", "SymbolStream.to_host", {"record": 1},
     "the event a range-coder job waits for, behind the D2H copies of a bitstream's symbols", "1 (first GOP), 2, 3, 4, 5, 7"),
    ("engine.py", "SymbolStream.copy_to", {"non_blocking": 2},
     "symbols and CDF rows, device to pinned host buffers (the plan's own, replayed as copy nodes)", "1-5, 7"),
    ("engine.py", "RangeCoderPool._run", {"synchronize": 1},
     "a host thread waits for the copies before it reads the pinned buffers", "1-5; 7 starts it 50 ms late"),
    ("engine.py", "HipEngine.compress_stage_batched", {"record": 1},
     "lt_event: the batched luma lifting is done, the next stage's motion chain may read its L_t", "3, 4"),
    ("engine.py", "HipEngine.ll_ar_finish", {"synchronize": 1, "record_stream": 1},
     "the LL decode's side stream is drained before the host reads its coder state; ll goes to the caller's stream", "5, 6"),
    ("engine.py", "HipEngine._finish_files", {"record": 1, "wait_stream": 1, "record_stream": 1},
     "decoded subbands from the side streams back to the caller's stream; a GOP's decoded planes from the side streams "
     "(fed by the batch streams) back to the caller's stream", "5, 6"),
    ("engine.py", "HipEngine._finish_files.finish", {"wait_event": 1},
     "a side stream waits for what the caller's stream has decoded so far; a side stream waits for the caller's stream "
     "before a file's remaining subbands", "5, 6"),
    ("ops.py", "Conv2d.__call__", {"record": 2}, "timing events of the conv probe, on the launch's stream", "2 (probe on)"),
    ("ops.py", "conv_at_class", {"record": 2}, "timing events of the conv probe, on the launch's stream", "2 (probe on)"),
    ("pair_plan.py", "PairPlan._record", {"wait_stream": 2},
     "the capture stream joins the caller's stream before a recording and hands back after it", "1 (first GOP)"),
    ("pair_plan.py", "PairPlan.run", {"record": 6, "wait_event": 3, "wait_stream": 2},
     "motion done -> both coder streams; each bitstream's pinned copy -> its job; analyses -> syntheses; results -> caller",
     "1, 7 (timing events on in the delayed runs)"),
    ("pMCTF_L.py", "pMCTF.encode_stage_pairs", {"wait_event": 2, "wait_stream": 4, "record_stream": 3, "record": 1},
     "motion stream behind lt_event or the caller's stream, its fields back; with two streams: luma / chroma coders",
     "3, 4, 7; the two-stream branch: batched_multi"),
    ("pMCTF_L.py", "pMCTF.encode_one_stage", {"record": 1, "wait_event": 1, "wait_stream": 1, "record_stream": 1},
     "luma / chroma coders of a pair on the side streams, results back to the caller's stream", "plans_off_multi"),
]
SITE_KINDS = ("wait_event", "wait_stream", "record_stream", "record", "synchronize", "non_blocking")


# ------------------------------------------------------------------------------------------------------- the instrument
_rate = {}                               # device index -> spin cycles per millisecond


def calibrate(dev):
    """cycles of torch.cuda._sleep per millisecond on `dev`, from two spins of different length timed with events"""
    import torch
    key = torch.device(dev).index or 0
    if key in _rate:
        return _rate[key]
    assert not torch.cuda.is_current_stream_capturing(), "no delay during a stream capture"
    st = torch.cuda.current_stream(dev)
    times = []
    torch.cuda._sleep(100_000)                               # the first launch loads the kernel
    for cycles in (2_000_000, 20_000_000):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        torch.cuda._sleep(cycles)
        e1.record(st)
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    slope = (times[1] - times[0]) / 18_000_000.0             # ms per cycle; the difference drops the launch overhead
    if not (slope > 0 and times[1] > 3 * times[0] > 0) or times[1] > 2000:
        raise RuntimeError(f"torch.cuda._sleep does not spin in proportion to its argument here: 2e6 cycles "
                           f"{times[0]:.3f} ms, 2e7 cycles {times[1]:.3f} ms")
    _rate[key] = 1.0 / slope
    return _rate[key]


def delay(stream, ms):
    """one bounded spin of about `ms` milliseconds in front of whatever is enqueued on `stream` next"""
    import torch
    assert 0 < ms <= MAX_DELAY_MS, f"a delay is at most {MAX_DELAY_MS} ms (asked for {ms})"
    rate = calibrate(stream.device)
    with torch.cuda.stream(stream):
        assert not torch.cuda.is_current_stream_capturing(), "no delay during a stream capture"
        torch.cuda._sleep(int(rate * ms))


def window(a, b, ms=KERNEL_DELAY_MS):
    """Writes a marker on `a` behind a delay and reads it on `b` without any wait: True when the read saw the old value.
    False means the two streams are served in order (one hardware queue): a delay on `a` cannot expose a missing wait
    towards `b`.  The marker is the test's own buffer."""
    import torch
    dev = a.device
    marker = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    delay(a, ms)
    with torch.cuda.stream(a):
        marker.fill_(1)
    with torch.cuda.stream(b):
        seen = marker.clone()
    a.synchronize()
    b.synchronize()
    return int(seen.cpu()[0]) == 0


def pick_stream(dev, others=(), tries=8):
    """The caller's stream: the first of up to `tries` fresh streams whose windows hold against the default stream and
    against every stream of `others`, in both directions.  -> (stream, report): report lists every candidate's windows.
    AssertionError when none qualifies (the hardware queues are shared out otherwise than the case needs)."""
    import torch
    default = torch.cuda.default_stream(dev)
    keep, report = [], []
    for i in range(tries):
        s = torch.cuda.Stream(device=dev)
        keep.append(s)                                       # a released stream's queue would be handed out again
        res = [(name, window(s, o), window(o, s)) for name, o in [("default", default)] + list(others)]
        report.append((i, res))
        if all(f and r for _, f, r in res):
            return s, report
    raise AssertionError(f"none of {tries} fresh streams has a window against all of default + "
                         f"{[n for n, _ in others]}: {report}")


# ---------------------------------------------------------------------------------------------------------------- rows
class Case:
    """What a row runs.  inputs / poison: name -> numpy array, the data and an equally valid second draw of the same shape
    (a name missing from poison keeps its data: a buffer the entry needs in one state, such as zeroed scratch).
    fixed: name -> device tensor uploaded once, before any delay (weights, tables).  outs: name -> (shape, numpy dtype) of
    the outputs the test owns; acc: those the entry adds to (zeroed on S at step 4); clears: those the entry clears itself
    (garbage on S at step 5); inout: inputs the entry also writes.  call(t) -> tuple of whatever else the wrapper returns
    (tensors, or host values); t holds every buffer by name.  launched: optional predicate on t after the call (a launch
    descriptor that names the path the row is about)."""

    def __init__(self, inputs, call, poison=None, fixed=None, outs=None, acc=(), clears=(), inout=(), launched=None,
                 around=None):
        self.inputs, self.call, self.fixed = inputs, call, fixed or {}
        self.poison = dict(inputs, **(poison or {}))
        self.outs, self.acc, self.clears, self.inout = outs or {}, tuple(acc), tuple(clears), tuple(inout)
        self.launched, self.around = launched, around
        self.pinned = None


def _guarded(shape, dtype, dev):
    """-> (whole byte buffer with GUARD sentinel bytes on either side, the output view inside it)"""
    import numpy as np
    import torch
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    buf = torch.full((2 * GUARD + n,), SENTINEL, dtype=torch.uint8, device=dev)
    tdt = torch.from_numpy(np.zeros(1, dtype)).dtype
    return buf, buf[GUARD:GUARD + n].view(tdt).view(*shape)


def _bytes(v):
    import torch
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
    return repr(v).encode()


def run(case, dev, S=None, call_on=None, ms=0.0, poisoned=False):
    """One pass of the protocol.  S: the caller's stream (None: the default stream); call_on: the stream that is current
    while the wrapper runs (None: S; the control passes the default stream); ms: the delay in front of the uploads (0:
    none); poisoned: leave the poison in the inputs.  -> (list of byte strings: every owned output with its guards,
    every in/out buffer, everything returned; host milliseconds from the injection point to the wrapper's return)."""
    import contextlib
    import torch
    S = S or torch.cuda.default_stream(dev)
    call_on = call_on or S
    if case.pinned is None:
        case.pinned = {k: torch.from_numpy(a).pin_memory() for k, a in case.inputs.items()}
        case.fixed = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in case.fixed.items()}
    t, bufs = dict(case.fixed), {}
    with torch.cuda.stream(S):                               # step 1: poison in, sentinels in the outputs
        for k, a in case.poison.items():
            t[k] = torch.from_numpy(a).to(dev)
        for k, (shape, dt) in case.outs.items():
            bufs[k], t[k] = _guarded(shape, dt, dev)
    torch.cuda.synchronize(dev)
    with (case.around() if case.around else contextlib.nullcontext()), torch.cuda.stream(S):
        if ms:
            delay(S, ms)                                     # step 2
        t0 = time.perf_counter()
        if not poisoned:
            for k, p in case.pinned.items():                 # step 3
                t[k].copy_(p, non_blocking=True)
        for k in case.acc:                                   # step 4
            t[k].zero_()
        for k in case.clears:                                # step 5
            t[k].reshape(-1).view(torch.uint8).fill_(GARBAGE)
        with torch.cuda.stream(call_on):                     # step 6
            res = case.call(t)
        host_ms = (time.perf_counter() - t0) * 1e3
        if case.launched is not None:
            case.launched(t)
    S.synchronize()                                          # step 7
    if call_on is not S:
        call_on.synchronize()                                # the control's own stream, so that its results can be read
    res = res if isinstance(res, (tuple, list)) else (() if res is None else (res,))
    out = [_bytes(bufs[k]) for k in case.outs] + [_bytes(t[k]) for k in case.inout] + [_bytes(v) for v in res]
    return out, host_ms


def check_row(row, dev, S, ms=KERNEL_DELAY_MS, log=None):
    """the whole of a row: precondition, delayed run on S, control.  AssertionError names what failed."""
    import torch
    case = row.build()
    default = torch.cuda.default_stream(dev)
    want, _ = run(case, dev)
    again, host_ms = run(case, dev)
    assert want == again, f"{row.name}: the reference call does not repeat its own bits"
    poisoned, _ = run(case, dev, poisoned=True)
    assert poisoned != want, f"{row.name}: poison and data give the same bits: the row proves nothing"
    assert host_ms * 3 <= ms or ms >= MAX_DELAY_MS, \
        f"{row.name}: enqueueing took {host_ms:.2f} ms, the delay of {ms} ms is not three times that"
    got, _ = run(case, dev, S=S, ms=ms)
    assert len(got) == len(want)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, f"{row.name}: on its caller's stream behind a delay, outputs {bad} of {len(want)} differ " \
                    f"from the synchronised call: something of {row.entry} does not run in the stream's order"
    control, _ = run(case, dev, S=S, call_on=default, ms=ms)
    assert control != want, f"{row.name}: the control (wrapper on the default stream) reproduced the expected bits: " \
                            f"no window, the row is unexercised"
    if log is not None:
        log.append((row.name, host_ms))


class Row:
    def __init__(self, name, entry, build):
        self.name, self.entry, self.build = name, entry, build


# ------------------------------------------------------------------------------------------------------- row builders
def _rng(name):
    import zlib
    import numpy as np
    return np.random.default_rng(zlib.crc32(name.encode()))


def _normal(r, shape, scale=1.0):
    import numpy as np
    return (r.standard_normal(shape, dtype=np.float32) * np.float32(scale)).astype(np.float32)


def _two(draw):
    """(data, poison) from one generator function of the draw index"""
    return draw(0), draw(1)


def _simple(name, names_shapes, call, scale=3.0, **kw):
    """a case whose inputs are float32 normal draws: names_shapes name -> shape"""
    r = _rng(name)
    data = {k: _normal(r, s, scale) for k, s in names_shapes.items()}
    poison = {k: _normal(r, s, scale) for k, s in names_shapes.items()}
    return Case(data, call, poison, **kw)


def _conv(name, cin, cout, k, stride=1, pad=None, rule=0, split=0):
    """a packed ops.Conv2d with weights drawn from the row's name (uploaded and synchronised by its constructor)"""
    import torch
    from pMCTF.hip import ops
    r = _rng(name + " weights")
    w = torch.from_numpy(_normal(r, (cout, cin, k, k), 0.05))
    b = torch.from_numpy(_normal(r, (cout,)))
    conv = ops.Conv2d(w, b, stride, (k // 2, k // 2) if pad is None else pad, rule=rule, split=split)
    torch.cuda.synchronize()
    return conv


def _vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _conv_last_launch():
    from pMCTF.hip import lib
    buf = C.create_string_buffer(512)
    assert lib.hip().pmctf_conv2d_last_launch(buf, 512) == 0
    return buf.value.decode()


def _knobs(values, defaults):
    """context manager factory: conv launch knobs for the time of a run"""
    import contextlib

    @contextlib.contextmanager
    def cm():
        from pMCTF.hip import lib
        L = lib.hip()
        try:
            for k, v in {**defaults, **values}.items():
                assert L.pmctf_conv2d_set_option(k.encode(), v) == 0
            yield
        finally:
            for k, v in defaults.items():
                L.pmctf_conv2d_set_option(k.encode(), v)
    return cm


def _split_px():
    import contextlib

    @contextlib.contextmanager
    def cm():
        from pMCTF.hip import ops
        old, ops.SPLIT_MIN_PX = ops.SPLIT_MIN_PX, 0
        try:
            yield
        finally:
            ops.SPLIT_MIN_PX = old
    return cm


def b_conv_opts(name, shape, k=3, stride=1, rule=0, act=2, nres=1, launched=None, around=None):
    def build():
        from pMCTF.hip import ops
        n, cin, h, w, cout = shape
        conv = _conv(name, cin, cout, k, stride, rule=rule)
        ho, wo = conv.out_shape(_Shape((n, h, w, cin)))[1:3]
        shapes = {"x": (n, h, w, cin)}
        for i in range(nres):
            shapes[f"r{i}"] = (n, ho, wo, cout)

        def call(t):
            conv(t["x"], act=act, slope=0.2, res1=t.get("r0"), res2=t.get("r1"), out=t["y"])
        chk = None
        if launched is not None:
            def chk(t):
                s = _conv_last_launch()
                assert launched(s), f"{name}: launched {s!r}, not the path this row is about"
        return _simple(name, shapes, call, outs={"y": ((n, ho, wo, cout), "float32")}, launched=chk, around=around)
    return build


class _Shape:
    def __init__(self, shape):
        self.shape = shape


def b_conv_plain(name):
    """pmctf_conv2d_nhwc_f32 itself (the wrappers go through the _opts form)"""
    def build():
        from pMCTF.hip import lib, ops
        n, cin, h, w, cout = 1, 16, 33, 70, 32
        conv = _conv(name, cin, cout, 3)
        assert not conv.small and not conv.few

        def call(t):
            lib.check(lib.hip().pmctf_conv2d_nhwc_f32(_vp(t["x"]), _vp(conv.w), _vp(conv.b), _vp(t["r0"]), None, _vp(t["y"]),
                                                      n, h, w, cin, cout, 3, 3, 1, 1, 1, ops.ACT_LEAKY, 0.2, ops._stream()),
                      "conv2d_nhwc")
        return _simple(name, {"x": (n, h, w, cin), "r0": (n, h, w, cout)}, call, outs={"y": ((n, h, w, cout), "float32")})
    return build


def b_conv_geom(name, opts):
    """the explicit-geometry forms at one parity class: ops.conv_at_class (_geom_opts) or the plain _geom entry"""
    def build():
        from pMCTF.hip import lib, ops
        n, cin, h, w, cout = 2, 112, 18, 36, 112
        conv = _conv(name, cin, cout, 3, rule=1 if opts else 0)
        if opts:
            def call(t):
                return ops.conv_at_class(conv, t["x"], 2, act=ops.ACT_LEAKY, slope=0.2, res1=t["r0"])
            return _simple(name, {"x": (n, h, w, cin), "r0": (n, h // 2, w // 2, cout)}, call)

        def call(t):
            lib.check(lib.hip().pmctf_conv2d_nhwc_geom_f32(_vp(t["x"]), _vp(conv.w), _vp(conv.b), _vp(t["r0"]), None,
                                                           _vp(t["y"]), n, h, w, cin, cout, 3, 3, 2, 0, 1, h // 2, w // 2,
                                                           ops.ACT_LEAKY, 0.2, ops._stream()), "conv2d_geom")
        return _simple(name, {"x": (n, h, w, cin), "r0": (n, h // 2, w // 2, cout)}, call,
                       outs={"y": ((n, h // 2, w // 2, cout), "float32")})
    return build


def b_conv_split(name, geom):
    def build():
        from pMCTF.hip import ops
        n, cin, h, w, cout = (2, 112, 18, 36, 112) if geom else (1, 64, 16, 32, 112)
        conv = _conv(name, cin, cout, 3, split=3)
        assert conv.split == 3
        if geom:
            def call(t):
                return ops.conv_at_class(conv, t["x"], 1, act=ops.ACT_LEAKY, slope=0.2, res1=t["r0"])
            return _simple(name, {"x": (n, h, w, cin), "r0": (n, h // 2, w // 2, cout)}, call, around=_split_px())

        def call(t):
            conv(t["x"], act=ops.ACT_LEAKY, slope=0.2, res1=t["r0"], out=t["y"])
        return _simple(name, {"x": (n, h, w, cin), "r0": (n, h, w, cout)}, call,
                       outs={"y": ((n, h, w, cout), "float32")}, around=_split_px())
    return build


def b_cin1_dual(name):
    def build():
        from pMCTF.hip import ops
        conv = _conv(name, 1, 16, 3, rule=1)

        def call(t):
            ops.conv3x3_cin1_dual(conv, t["x"], ops.ACT_TANH, out=t["y"], out2=t["y2"])
        return _simple(name, {"x": (2, 37, 70, 1)}, call, scale=40.0,
                       outs={"y": ((2, 37, 70, 16), "float32"), "y2": ((2, 37, 70, 16), "float32")})
    return build


def b_dwconv(name):
    def build():
        import torch
        from pMCTF.hip import ops
        r = _rng(name + " weights")
        dw = ops.DepthwiseConv2d(torch.from_numpy(_normal(r, (6, 1, 3, 3))), torch.from_numpy(_normal(r, (6,))))
        torch.cuda.synchronize()
        return _simple(name, {"x": (1, 19, 23, 6)}, lambda t: dw(t["x"], out=t["y"]),
                       outs={"y": ((1, 19, 23, 6), "float32")})
    return build


def b_returning(name, shapes, fn, scale=3.0, **kw):
    """a wrapper that allocates and returns its outputs: fn(ops, t) -> tensor(s)"""
    def build():
        from pMCTF.hip import ops
        return _simple(name, shapes, lambda t: fn(ops, t), scale=scale, **kw)
    return build


def b_flow_warp(name):
    def build():
        import torch
        from pMCTF.hip import ops
        n, c, h, w = 2, 1, 37, 53
        fixed = {"lx": torch.linspace(-1.0, 1.0, w), "ly": torch.linspace(-1.0, 1.0, h)}
        r = _rng(name)
        draw = lambda: {"im": (r.random((n, c, h, w), dtype="float32") * 255).astype("float32"),
                        "flow": _normal(r, (1, 2, h, w), 6.0)}
        return Case(draw(), lambda t: ops.flow_warp(t["im"], t["flow"], t["lx"], t["ly"], -1.0), draw(), fixed=fixed)
    return build


def b_direct2(name, entry, down):
    """the factor-2 resampling entries no wrapper calls: pmctf_bilinear_up2_f32 / pmctf_bilinear_down2_f32"""
    def build():
        from pMCTF.hip import lib, ops
        nc, h, w = 3, 18, 30
        out = (1, nc, h // 2, w // 2) if down else (1, nc, 2 * h, 2 * w)

        def call(t):
            lib.check(getattr(lib.hip(), entry)(_vp(t["x"]), _vp(t["y"]), nc, h, w, 2.0, ops._stream()), entry)
        return _simple(name, {"x": (1, nc, h, w)}, call, scale=10.0, outs={"y": (out, "float32")})
    return build


def b_ew(name):
    def build():
        from pMCTF.hip import ops

        def call(t):
            ops.ew(ops.EW_ADD_MULS_MULS, t["a"], t["b"], 0.37, 2.25, out=t["y"])
        return _simple(name, {"a": (2, 3, 20, 36), "b": (2, 3, 20, 36)}, call, outs={"y": ((2, 3, 20, 36), "float32")})
    return build


def b_pu_fused(name):
    def build():
        from pMCTF.hip import ops
        pu = (_conv(name + "1", 1, 16, 3, rule=1), _conv(name + "2", 16, 16, 3, rule=1), _conv(name + "3", 16, 16, 3, rule=1),
              _conv(name + "4", 16, 1, 3, rule=1))

        def call(t):
            return ops.predict_update_fused(t["x"], t["other"], pu, 1, sign=-1.0, lift=(0.3, 0.5, -0.2, 37.7), skip_rule=1)
        return _simple(name, {"x": (2, 1, 37, 53), "other": (2, 1, 37, 53)}, call, scale=50.0)
    return build


def b_lstm_plain(name):
    def build():
        from pMCTF.hip import lib, ops
        shp = (1, 9, 11, 32)

        def call(t):
            lib.check(lib.hip().pmctf_lstm_gates_f32(_vp(t["xh"]), _vp(t["cell"]), _vp(t["c_out"]), _vp(t["h_out"]),
                                                     9 * 11, 32, 32, ops._stream()), "lstm_gates")
        return _simple(name, {"xh": shp, "cell": shp}, call, outs={"c_out": (shp, "float32"), "h_out": (shp, "float32")})
    return build


def _gauss():
    from pmctf_oracle import entropy
    g = entropy.GaussianTables()
    return float(g.log_scale_min), float(g.log_scale_step)


def _params(r, shape):
    """(scale, mean) pairs on the last axis: scales positive, over the rows of the table"""
    import numpy as np
    p = _normal(r, shape + (2,), 4.0)
    p[..., 0] = np.exp(r.uniform(np.log(0.2), np.log(60.0), shape)).astype(np.float32)
    return p


def b_fourstep(name, kind):
    """kind: quant | indexes | dequant | estimate, class k = 2, parameters at every position, two planes of 6 x 10"""
    def build():
        import numpy as np
        from pMCTF.hip import ops
        n, h, w, k = 2, 6, 10, 2
        lmin, lstep = _gauss()
        r = _rng(name)
        draw = lambda: {"x": _normal(r, (n, 1, h, w), 20.0), "params": _params(r, (n, h, w)),
                        "so_far": _normal(r, (n, 1, h, w), 20.0).round(),
                        "sym": r.integers(-40, 40, n * h * w).astype(np.int16)}
        d, p = draw(), draw()
        tot = n * h * w
        if kind == "quant":
            for q in (d, p):
                q.pop("sym")
            return Case(d, lambda t: ops.fourstep_quant(t["x"], t["params"], t["so_far"], t["sym"], t["idx"], 0, k, lmin,
                                                        lstep), p, inout=("so_far",),
                        outs={"sym": ((tot,), "int16"), "idx": ((tot,), "int16")})
        if kind == "indexes":
            d, p = {"params": d["params"]}, {"params": p["params"]}
            return Case(d, lambda t: ops.fourstep_indexes(t["params"], n, h, w, k, lmin, lstep), p)
        if kind == "dequant":
            for q in (d, p):
                q.pop("x")
            return Case(d, lambda t: ops.fourstep_dequant(t["sym"], t["params"], t["so_far"], k), p, inout=("so_far",))
        for q in (d, p):
            q.pop("sym")
        return Case(d, lambda t: ops.fourstep_estimate(t["x"], t["params"], t["so_far"], k, t["bits"]), p,
                    inout=("so_far",), outs={"bits": ((n,), "float64")}, acc=("bits",))
    return build


def b_ll_quant(name, estimate):
    def build():
        from pMCTF.hip import ops
        n, h, w = 2, 5, 9
        lmin, lstep = _gauss()
        r = _rng(name)
        draw = lambda: {"ll": _normal(r, (n, 1, h, w), 30.0).round(), "params": _params(r, (n, h, w))}
        if estimate:
            return Case(draw(), lambda t: ops.ll_estimate(t["ll"], t["params"], t["bits"]), draw(),
                        outs={"bits": ((n,), "float64")}, acc=("bits",))
        tot = n * h * w
        return Case(draw(), lambda t: ops.ll_quant(t["ll"], t["params"], t["sym"], t["idx"], 0, lmin, lstep, ar_order=True),
                    draw(), outs={"sym": ((tot,), "int16"), "idx": ((tot,), "int16")})
    return build


def b_z(name, kind):
    def build():
        import numpy as np
        from pMCTF.hip import ops
        h, w, c = 5, 7, 64
        r = _rng(name)
        if kind == "symbols":
            return _simple(name, {"z": (1, h, w, c)}, lambda t: ops.z_symbols(t["z"], t["sym"], t["idx"], 0), scale=6.0,
                           outs={"sym": ((h * w * c,), "int16"), "idx": ((h * w * c,), "int16")})
        if kind == "sym_to_nhwc":
            draw = lambda: {"sym": r.integers(-300, 300, h * w * c).astype(np.int16)}
            return Case(draw(), lambda t: ops.sym_to_nhwc(t["sym"], h, w, c), draw())
        import torch
        h = w = 1                                            # 64 elements: one wave, one atomic add
        consts = np.abs(_normal(r, (11, c))) + np.float32(0.1)
        consts[8:] = np.tanh(_normal(r, (3, c)))
        return _simple(name, {"z": (1, h, w, c)}, lambda t: ops.z_estimate(t["z"], t["consts"], t["bits"]), scale=6.0,
                       fixed={"consts": torch.from_numpy(consts)}, outs={"bits": ((1,), "float64")}, acc=("bits",))
    return build


def b_mv(name, kind):
    """the four-part prior's step t = 1 on a 2 x 2 plane: step | indexes | dequant | estimate | final dequant"""
    def build():
        import numpy as np
        from pMCTF.hip import ops
        h, w, step = 2, 2, 1
        hw = h * w
        lmin, lstep = _gauss()
        r = _rng(name)

        def draw():
            common = np.concatenate([np.abs(_normal(r, (hw, 64))) + np.float32(0.3), _params(r, (hw, 64))[..., 0],
                                     _normal(r, (hw, 64), 4.0)], 1).reshape(1, h, w, 192)
            sp = np.concatenate([_params(r, (hw, 64))[..., 0], _normal(r, (hw, 64), 4.0)], 1).reshape(1, h, w, 128)
            return {"y": _normal(r, (1, h, w, 64), 10.0), "common": np.ascontiguousarray(common),
                    "sp": np.ascontiguousarray(sp), "so_far": _normal(r, (1, h, w, 64), 10.0).round(),
                    "sym": r.integers(-40, 40, 16 * hw).astype(np.int16)}
        d, p = draw(), draw()
        drop = {"step": ("sym",), "indexes": ("y", "so_far", "sym"), "dequant": ("y",), "estimate": ("sym",),
                "final": ("y", "sp", "sym")}[kind]
        for q in (d, p):
            for k in drop:
                q.pop(k)
        if kind == "step":
            return Case(d, lambda t: ops.mv_fourpart_step(t["y"], t["common"], t["sp"], t["so_far"], t["sym"], t["idx"], 0,
                                                          step, lmin, lstep), p, inout=("so_far",),
                        outs={"sym": ((16 * hw,), "int16"), "idx": ((16 * hw,), "int16")})
        if kind == "indexes":
            return Case(d, lambda t: ops.mv_fourpart_indexes(t["common"], t["sp"], h, w, step, lmin, lstep), p)
        if kind == "dequant":
            return Case(d, lambda t: ops.mv_fourpart_dequant(t["sym"], t["common"], t["sp"], t["so_far"], step), p,
                        inout=("so_far",))
        if kind == "estimate":
            return Case(d, lambda t: ops.mv_fourpart_estimate(t["y"], t["common"], t["sp"], t["so_far"], step, t["bits"]),
                        p, inout=("so_far",), outs={"bits": ((1,), "float64")}, acc=("bits",))
        return Case(d, lambda t: ops.mv_dequant(t["so_far"], t["common"]), p)
    return build


def b_sqdiff(name):
    def build():
        from pMCTF.hip import ops
        # The float64 atomic adds of the estimate-mode entries (one per wave) arrive in any order, so a row's reference
        # repeats its own bits only where the order cannot matter: one wave per accumulator (fourstep, ll, z), terms
        # whose sum is exact in float64 whatever the order (mv: 256 float32 terms of 0.1 .. 32 bits), integers (here).
        r = _rng(name)
        draw = lambda: {k: r.integers(-60, 61, (3, 1, 37, 53)).astype("float32") for k in ("a", "b")}
        return Case(draw(), lambda t: ops.sqdiff_sum(t["a"], t["b"], t["sum"]), draw(), outs={"sum": ((1,), "float64")},
                    acc=("sum",))
    return build


# ---- pictures: samples are drawn in range; a reconstruction is a picture plus noise, neither clamped nor rounded
def _recon(r, hp, wp, top=255.0):
    import numpy as np
    mk = lambda s: (r.integers(0, int(top) + 1, s).astype(np.float32) + _normal(r, s, 2.0)).astype(np.float32)
    return mk((1, 1, hp, wp)), mk((2, 1, hp // 2, wp // 2))


def _orig(r, h, w, bitdepth=8):
    import numpy as np
    sc = np.float32(2.0 ** -(bitdepth - 8))
    mk = lambda s: (r.integers(0, 1 << bitdepth, s).astype(np.float32) * sc).astype(np.float32)
    return mk((1, 1, h, w)), mk((2, 1, h // 2, w // 2))


def b_quality(name, msssim):
    def build():
        from pMCTF.hip import ops
        h, w, hp, wp = (162, 164, 256, 256) if msssim else (10, 12, 128, 128)
        r = _rng(name)

        def draw():
            ry, rc = _recon(r, hp, wp)
            oy, oc = _orig(r, h, w)
            return {"ry": ry, "rc": rc, "oy": oy, "oc": oc}

        def call(t):
            q = ops.frame_quality(t["ry"], t["rc"], t["oy"], t["oc"], h, w, msssim=msssim, return_means=True)
            return (q["sse"], q["means"])
        return Case(draw(), call, draw())
    return build


def b_sse_hbd(name, direct):
    def build():
        from pMCTF.hip import lib, ops
        h, w, hp, wp, depth = 10, 12, 128, 128, 10
        r = _rng(name)

        def draw():
            ry, rc = _recon(r, hp, wp)
            oy, oc = _orig(r, h, w, depth)
            return {"ry": ry, "rc": rc, "oy": oy, "oc": oc}
        if not direct:
            return Case(draw(), lambda t: (ops.frame_sse_hbd(t["ry"], t["rc"], t["oy"], t["oc"], h, w, depth)["sse"],),
                        draw())

        def call(t):                                         # the entry's own clear, onto garbage the caller left on S
            lib.check(lib.hip().pmctf_frame_sse_u16_f32(_vp(t["ry"]), _vp(t["rc"]), _vp(t["oy"]), _vp(t["oc"]), hp, wp, h, w,
                                                        depth, _vp(t["sse"]), ops._stream()), "frame_sse_u16")
        return Case(draw(), call, draw(), outs={"sse": ((3,), "int64")}, clears=("sse",))
    return build


def b_picture(name, kind):
    def build():
        import numpy as np
        from pMCTF.hip import ops
        h, w = 10, 12
        r = _rng(name)
        n = h * w * 3 // 2
        if kind == "to_rgb8":
            draw = lambda: dict(zip(("ry", "rc"), _recon(r, 128, 128)))
            return Case(draw(), lambda t: ops.frame_to_rgb8(t["ry"], t["rc"], h, w), draw())
        if kind == "from_u8":
            draw = lambda: {"f": r.integers(0, 256, n).astype(np.uint8)}
            return Case(draw(), lambda t: ops.planes_from_u8(t["f"], h, w), draw())
        if kind == "from_u16":
            draw = lambda: {"f": r.integers(0, 1024, n).astype(np.uint16)}
            return Case(draw(), lambda t: ops.planes_from_u16(t["f"], h, w, 10), draw())
        if kind == "rgb_to_yuv":
            draw = lambda: {"rgb": r.integers(0, 256, (h, w, 3)).astype(np.uint8)}
            return Case(draw(), lambda t: ops.rgb8_to_yuv420(t["rgb"]), draw())
        draw = lambda: {"x": _recon(r, 128, 128)[1]}
        if kind == "to_u8":
            return Case(draw(), lambda t: ops.planes_to_u8(t["x"], 5, 7), draw())
        return Case(draw(), lambda t: ops.planes_to_u16(t["x"], 5, 7, 12), draw())
    return build


def b_resize(name, depth, size):
    def build():
        import numpy as np
        import torch
        import pmctf_scale
        (wi, hi), (wo, ho) = size
        rs = pmctf_scale.Resampler(wi, hi, wo, ho, "cuda", bitdepth=depth)
        torch.cuda.synchronize()
        r = _rng(name)
        dt = np.uint8 if depth == 8 else np.uint16
        draw = lambda: {"f": r.integers(0, 1 << depth, hi * wi * 3 // 2).astype(dt)}
        return Case(draw(), lambda t: rs(t["f"]), draw())
    return build


def b_chroma(name, depth, fmts):
    def build():
        import numpy as np
        import torch
        import pmctf_chroma
        w, h = 12, 10
        cv = pmctf_chroma.Converter(w, h, fmts[0], fmts[1], "cuda", bitdepth=depth)
        torch.cuda.synchronize()
        r = _rng(name)
        dt = np.uint8 if depth == 8 else np.uint16
        draw = lambda: {"f": r.integers(0, 1 << depth, pmctf_chroma.frame_samples(w, h, fmts[0])).astype(dt)}
        return Case(draw(), lambda t: cv(t["f"]), draw())
    return build


def b_layout(name, layout, pack):
    def build():
        import numpy as np
        from pMCTF.hip import ops
        h, w = 10, 12
        _, fmt, depth, _, _ = ops.LAYOUTS[layout]
        _, _, nbytes = ops.layout_geometry(layout, h, w)
        n = ops.chroma_frame_samples(h, w, fmt)
        r = _rng(name)
        dt = np.uint8 if depth == 8 else np.uint16
        if pack:
            draw = lambda: {"f": r.integers(0, 1 << depth, n).astype(dt)}
            return Case(draw(), lambda t: ops.pack_layout(t["f"], layout, h, w, out=t["s"]), draw(),
                        outs={"s": ((nbytes,), "uint8")})
        if depth == 8:
            draw = lambda: {"s": r.integers(0, 256, nbytes).astype(np.uint8)}
        else:                                                # a sample of depth b sits in a word as v << (16 - b)
            draw = lambda: {"s": (r.integers(0, 1 << depth, nbytes // 2) << (16 - depth)).astype("<u2").view(np.uint8)}
        return Case(draw(), lambda t: ops.unpack_layout(t["s"], layout, h, w, out=t["f"]), draw(), outs={"f": ((n,), dt)})
    return build


def b_luma(name, with_prev):
    def build():
        from pMCTF.hip import ops
        r = _rng(name)
        h, w = 37, 53
        draw = lambda: {"cur": _orig(r, h, w)[0], "prev": _orig(r, h, w)[0]}
        if with_prev:
            return Case(draw(), lambda t: ops.luma_activity(t["cur"], t["prev"], 8, hist=t["hist"], sad=t["sad"]) and (),
                        draw(), outs={"hist": ((256,), "int32"), "sad": ((1,), "int64")}, clears=("hist", "sad"))
        d, p = draw(), draw()
        d.pop("prev"), p.pop("prev")
        return Case(d, lambda t: ops.luma_activity(t["cur"], None, 8, hist=t["hist"]) and (), p,
                    outs={"hist": ((256,), "int32")}, clears=("hist",))
    return build


def b_crc(name):
    def build():
        import numpy as np
        from pMCTF.hip import ops
        r = _rng(name)
        draw = lambda: {"a": r.integers(0, 256, 5000).astype(np.uint8), "b": r.integers(0, 256, 37).astype(np.uint8)}
        return Case(draw(), lambda t: (ops.crc32([t["a"], t["b"]], out=t["crc"]),), draw(), outs={"crc": ((2,), "int32")})
    return build


def b_probe(name):
    def build():
        import numpy as np
        from pMCTF.hip import ops
        r = _rng(name)
        draw = lambda: {"bits": _normal(r, (4096,), 3.0).view(np.int32)}

        def call(t):
            ops.math_probe(ops.PROBE_TANH, t["bits"], out=t["y"])
        return Case(draw(), call, draw(), outs={"y": ((4096,), "float32")})
    return build


# ---- sequential LL decode: the poison is another model's packed weights (the stream, the tables and the entry state are
# those of the data: a decoder that holds the wrong model meets exactly this, and the kernels bound every read by n_words)
_ll = {}


def _ll_material():
    if not _ll:
        import numpy as np
        import ll_decode_helper as hp
        sets = hp.weight_sets(("s0", "s1"))
        _ll.update(hp=hp, sets=sets, planes=hp.ll_planes(),
                   tabs=tuple(np.ascontiguousarray(a, dtype=np.int32) for a in sets["s0"].tables.cdf_info()),
                   packed={k: hp.pack_weights(o.sd) for k, o in sets.items()},
                   lmin=float(sets["s0"].tables.log_scale_min), lstep=float(sets["s0"].tables.log_scale_step))
    return _ll


def b_ll_decode(name, entry, shape, rules, kernel=None, order="position"):
    """entry: plain (pmctf_ll_ar_decode_f32, all rules chain) | rules | batch (two jobs)"""
    def build():
        import numpy as np
        import torch
        from pMCTF.hip import lib, ops
        from pMCTF.hip.engine import HipEngine
        m = _ll_material()
        hp, tabs = m["hp"], m["tabs"]
        L = lib.hip()
        N, H, W = shape
        cols = tabs[0].shape[1]
        if kernel is not None:
            assert hp.kernel_for("default", rules[0], N, W, cols) == kernel, (name, kernel)
        jobs = 2 if entry == "batch" else 1
        cs = []
        for j in range(jobs):
            salt = sum(name.encode()) + j
            ll = hp.ll_for(m["planes"], N, H, W, salt)
            c = hp.make_case(m["sets"]["s0"], rules, ll, hp.side_symbols(salt, 5 + 4 * j, tabs),
                             hp.side_symbols(salt + 1, 24, tabs))
            if entry == "batch" and order == "plane" and N > 1:
                raise NotImplementedError
            cs.append(c)
        fixed = {"cdf": torch.from_numpy(tabs[0]), "sizes": torch.from_numpy(tabs[1]), "offs": torch.from_numpy(tabs[2])}
        nscr = L.pmctf_ll_ar_scratch_floats(N, H, W)
        inputs, poison = {"w": m["packed"]["s0"]}, {"w": m["packed"]["s1"]}
        for j, c in enumerate(cs):
            fixed[f"words{j}"] = torch.from_numpy(np.ascontiguousarray(c["words"]))
            inputs[f"scratch{j}"] = np.zeros(nscr, np.float32)
            inputs[f"state{j}"] = np.array([c["x0"], c["pos0"], 0], np.uint64).view(np.int64)
        outs = {f"ll{j}": ((N, H, W), "float32") for j in range(jobs)}
        c0 = cs[0]
        common = lambda t: (_vp(t["cdf"]), _vp(t["sizes"]), _vp(t["offs"]), cols, m["lmin"], m["lstep"])
        if entry == "batch":
            assert HipEngine.ll_batch_form(N, W, cols, order, rules[0]) in (1, 2)

            def call(t):
                table = np.zeros(jobs, HipEngine.LL_JOB)
                for j, c in enumerate(cs):
                    table[j] = (t["w"].data_ptr(), t[f"words{j}"].data_ptr(), c["words"].size, t[f"state{j}"].data_ptr(),
                                t[f"ll{j}"].data_ptr(), t[f"scratch{j}"].data_ptr(), rules, 0)
                t["table"] = torch.from_numpy(table.view(np.uint8)).to(t["w"].device)
                lib.check(L.pmctf_ll_ar_decode_batch_f32(_vp(t["table"]), jobs, *common(t), N, H, W,
                                                         HipEngine.LL_ORDERS[order], ops._stream()), "ll_ar_decode_batch")
            return Case(inputs, call, poison, fixed=fixed, outs=outs, inout=tuple(f"state{j}" for j in range(jobs)))
        inputs.pop("state0")
        outs["state"] = ((3,), "int64")

        def call(t):
            head = (_vp(t["w"]), _vp(t["words0"]), int(c0["words"].size), C.c_uint64(int(c0["x0"])), int(c0["pos0"]))
            tail = (_vp(t["ll0"]), _vp(t["scratch0"]), N, H, W, _vp(t["state"]))
            if entry == "plain":
                lib.check(L.pmctf_ll_ar_decode_f32(*head, *common(t), *tail, ops._stream()), "ll_ar_decode")
            else:
                lib.check(L.pmctf_ll_ar_decode_rules_f32(*head, *common(t), *tail, int(rules[0]), int(rules[1]),
                                                         int(rules[2]), ops._stream()), "ll_ar_decode_rules")
        return Case(inputs, call, poison, fixed=fixed, outs=outs)
    return build


_TILE_DEFAULTS = {"NT": 0, "MSPLIT_PX": 70000, "BSUM_TILEOUTER": 1}

ROWS = [
    # ---- matrix-core convolutions and their launch paths
    Row("conv2d_nhwc", "pmctf_conv2d_nhwc_f32", b_conv_plain("conv2d_nhwc")),
    Row("conv2d_nhwc_opts", "pmctf_conv2d_nhwc_opts_f32", b_conv_opts("conv2d_nhwc_opts", (2, 64, 33, 47, 64))),
    Row("conv2d_nhwc_opts rounds+remainder", "pmctf_conv2d_nhwc_opts_f32",
        b_conv_opts("conv rounds+remainder", (1, 16, 264, 520, 112), rule=1, act=0, nres=0,
                    launched=lambda s: " + " in s, around=_knobs({}, _TILE_DEFAULTS))),
    Row("conv2d_nhwc_opts blocks 4+3 tiles", "pmctf_conv2d_nhwc_opts_f32",
        b_conv_opts("conv blocks 4+3", (1, 16, 8, 32, 112), rule=1, act=0, nres=0,
                    launched=lambda s: "conv3x3s1_wave_kernel<4, 2, true, 0>" in s
                    and "conv3x3s1_wave_kernel<3, 2, true, 4>" in s,
                    around=_knobs({"NT": 4, "MSPLIT_PX": 0, "BSUM_TILEOUTER": 0}, _TILE_DEFAULTS))),
    Row("conv2d_nhwc_opts 1x1", "pmctf_conv2d_nhwc_opts_f32", b_conv_opts("conv 1x1", (1, 192, 18, 30, 128), k=1, nres=0)),
    Row("conv2d_nhwc_geom", "pmctf_conv2d_nhwc_geom_f32", b_conv_geom("conv2d_nhwc_geom", False)),
    Row("conv2d_nhwc_geom_opts", "pmctf_conv2d_nhwc_geom_opts_f32", b_conv_geom("conv2d_nhwc_geom_opts", True)),
    Row("conv3x3_split", "pmctf_conv3x3_split_f32", b_conv_split("conv3x3_split", False)),
    Row("conv3x3_split_geom", "pmctf_conv3x3_split_geom_f32", b_conv_split("conv3x3_split_geom", True)),
    # ---- vector-ALU convolutions
    Row("conv2d_smallcin", "pmctf_conv2d_smallcin_f32", b_conv_opts("conv2d_smallcin", (2, 2, 37, 53, 112), act=0, nres=0)),
    Row("conv3x3_cin1_dual", "pmctf_conv3x3_cin1_dual_f32", b_cin1_dual("conv3x3_cin1_dual")),
    Row("conv2d_fewcout", "pmctf_conv2d_fewcout_f32", b_conv_opts("conv2d_fewcout", (1, 16, 33, 70, 1), nres=2)),
    Row("dwconv2d_nhwc", "pmctf_dwconv2d_nhwc_f32", b_dwconv("dwconv2d_nhwc")),
    Row("predict_update_fused", "pmctf_predict_update_fused_f32", b_pu_fused("predict_update_fused")),
    # ---- warping, resampling, glue
    Row("flow_warp", "pmctf_flow_warp_f32", b_flow_warp("flow_warp")),
    Row("avgpool2", "pmctf_avgpool2_f32", b_returning("avgpool2", {"x": (2, 3, 37, 61)}, lambda o, t: o.avgpool2(t["x"]))),
    Row("bilinear_up2", "pmctf_bilinear_up2_f32", b_direct2("bilinear_up2", "pmctf_bilinear_up2_f32", False)),
    Row("bilinear_down2", "pmctf_bilinear_down2_f32", b_direct2("bilinear_down2", "pmctf_bilinear_down2_f32", True)),
    Row("bilinear_up", "pmctf_bilinear_up_f32",
        b_returning("bilinear_up", {"x": (1, 2, 9, 17)}, lambda o, t: o.bilinear_up2(t["x"], 4.0, 4))),
    Row("bilinear_down", "pmctf_bilinear_down_f32",
        b_returning("bilinear_down", {"x": (1, 2, 40, 72)}, lambda o, t: o.bilinear_down2(t["x"], 1.0, 8))),
    Row("ew", "pmctf_ew_f32", b_ew("ew")),
    Row("spynet_pack8", "pmctf_spynet_pack8_f32",
        b_returning("spynet_pack8", {"im1": (1, 1, 37, 53), "wrp": (1, 1, 37, 53), "fu": (1, 2, 37, 53)},
                    lambda o, t: o.spynet_pack8(t["im1"], t["wrp"], t["fu"]))),
    Row("lift_skip3", "pmctf_lift_skip3_f32",
        b_returning("lift_skip3", {"x": (2, 3, 2, 5)}, lambda o, t: o.lift_skip3(t["x"], (0.3, 0.5, -0.2), 0.3125, 1),
                    scale=50.0)),
    Row("nearest_up2", "pmctf_nearest_up2_nhwc_f32",
        b_returning("nearest_up2", {"x": (2, 5, 7, 8)}, lambda o, t: o.nearest_up2(t["x"]))),
    Row("pixel_shuffle2", "pmctf_pixel_shuffle2_nhwc_f32",
        b_returning("pixel_shuffle2", {"x": (2, 5, 7, 32)}, lambda o, t: o.pixel_shuffle2(t["x"], o.ACT_LEAKY, 0.1))),
    Row("ffn3_mix", "pmctf_ffn3_mix_f32", b_returning("ffn3_mix", {"x": (1, 5, 7, 6)}, lambda o, t: o.ffn3_mix(t["x"]))),
    Row("lstm_gates", "pmctf_lstm_gates_f32", b_lstm_plain("lstm_gates")),
    Row("lstm_gates_aten", "pmctf_lstm_gates_aten_f32",
        b_returning("lstm_gates_aten", {"xh": (2, 30, 44, 3), "cell": (2, 30, 44, 3)},
                    lambda o, t: o.lstm_gates(t["xh"], t["cell"], ref_planes=2, aten_threads=8))),
    # ---- quantisation and symbols, encoder and decoder side
    Row("fourstep_quant", "pmctf_fourstep_quant_f32", b_fourstep("fourstep_quant", "quant")),
    Row("ll_quant", "pmctf_ll_quant_f32", b_ll_quant("ll_quant", False)),
    Row("z_symbols", "pmctf_z_symbols_f32", b_z("z_symbols", "symbols")),
    Row("mv_fourpart_step", "pmctf_mv_fourpart_step_f32", b_mv("mv_fourpart_step", "step")),
    Row("mv_dequant", "pmctf_mv_dequant_f32", b_mv("mv_dequant", "final")),
    Row("fourstep_indexes", "pmctf_fourstep_indexes_f32", b_fourstep("fourstep_indexes", "indexes")),
    Row("fourstep_dequant", "pmctf_fourstep_dequant_f32", b_fourstep("fourstep_dequant", "dequant")),
    Row("mv_fourpart_indexes", "pmctf_mv_fourpart_indexes_f32", b_mv("mv_fourpart_indexes", "indexes")),
    Row("mv_fourpart_dequant", "pmctf_mv_fourpart_dequant_f32", b_mv("mv_fourpart_dequant", "dequant")),
    Row("sym_to_nhwc", "pmctf_sym_to_nhwc_f32", b_z("sym_to_nhwc", "sym_to_nhwc")),
    Row("planes_to_u8", "pmctf_planes_to_u8", b_picture("planes_to_u8", "to_u8")),
    # ---- sequential LL decode: every kernel the entries choose from, and the batch entry
    Row("ll_ar_decode", "pmctf_ll_ar_decode_f32", b_ll_decode("ll_ar_decode", "plain", (1, 3, 7), (0, 0, 0), "stream<1>")),
    Row("ll_ar_decode_rules row2", "pmctf_ll_ar_decode_rules_f32",
        b_ll_decode("ll rules row2", "rules", (2, 2, 88), (1, 32, 16), "row2<2>")),
    Row("ll_ar_decode_rules row", "pmctf_ll_ar_decode_rules_f32",
        b_ll_decode("ll rules row", "rules", (2, 2, 89), (1, 48, 0), "row<2>")),
    Row("ll_ar_decode_rules stream", "pmctf_ll_ar_decode_rules_f32",
        b_ll_decode("ll rules stream", "rules", (2, 3, 9), (0, 64, 112), "stream<2>")),
    Row("ll_ar_decode_rules v1", "pmctf_ll_ar_decode_rules_f32",
        b_ll_decode("ll rules v1", "rules", (3, 4, 6), (1, 32, 16), "v1 N=3")),
    Row("ll_ar_decode_batch", "pmctf_ll_ar_decode_batch_f32", b_ll_decode("ll batch", "batch", (1, 3, 7), (1, 32, 16))),
    Row("ll_ar_decode_batch two planes", "pmctf_ll_ar_decode_batch_f32",
        b_ll_decode("ll batch two planes", "batch", (2, 2, 89), (1, 48, 0))),
    # ---- estimate mode: the accumulators are zeroed on the caller's stream behind the delay
    Row("fourstep_estimate", "pmctf_fourstep_estimate_f32", b_fourstep("fourstep_estimate", "estimate")),
    Row("ll_estimate", "pmctf_ll_estimate_f32", b_ll_quant("ll_estimate", True)),
    Row("z_estimate", "pmctf_z_estimate_f32", b_z("z_estimate", "estimate")),
    Row("mv_fourpart_estimate", "pmctf_mv_fourpart_estimate_f32", b_mv("mv_fourpart_estimate", "estimate")),
    Row("sqdiff_sum", "pmctf_sqdiff_sum_f32", b_sqdiff("sqdiff_sum")),
    # ---- picture quality: the front end alone, and with the five MS-SSIM scales and the final sums
    Row("frame_quality front end", "pmctf_frame_quality_f32", b_quality("frame_quality front", False)),
    Row("frame_quality msssim", "pmctf_frame_quality_f32", b_quality("frame_quality msssim", True)),
    # ---- pictures in and out
    Row("yuv420_to_rgb8", "pmctf_yuv420_to_rgb8_f32", b_picture("yuv420_to_rgb8", "to_rgb8")),
    Row("yuv420_u8_to_planes", "pmctf_yuv420_u8_to_planes_f32", b_picture("yuv420_u8_to_planes", "from_u8")),
    Row("rgb8_to_yuv420_u8", "pmctf_rgb8_to_yuv420_u8", b_picture("rgb8_to_yuv420_u8", "rgb_to_yuv")),
    Row("yuv420_u16_to_planes", "pmctf_yuv420_u16_to_planes_f32", b_picture("yuv420_u16_to_planes", "from_u16")),
    Row("planes_to_u16", "pmctf_planes_to_u16", b_picture("planes_to_u16", "to_u16")),
    Row("frame_sse_u16", "pmctf_frame_sse_u16_f32", b_sse_hbd("frame_sse_u16", False)),
    Row("frame_sse_u16 clear", "pmctf_frame_sse_u16_f32", b_sse_hbd("frame_sse_u16 clear", True)),
    # ---- resampling and chroma conversion: both passes, and each pass alone (the other axis keeps its length)
    Row("resize_yuv420_u8", "pmctf_resize_yuv420_u8", b_resize("resize_u8", 8, ((20, 12), (12, 20)))),
    Row("resize_yuv420_u8 x pass", "pmctf_resize_yuv420_u8", b_resize("resize_u8 x", 8, ((20, 12), (12, 12)))),
    Row("resize_yuv420_u8 y pass", "pmctf_resize_yuv420_u8", b_resize("resize_u8 y", 8, ((20, 12), (20, 20)))),
    Row("resize_yuv420_u16", "pmctf_resize_yuv420_u16", b_resize("resize_u16", 10, ((20, 12), (12, 20)))),
    Row("convert_chroma_u8 420->444", "pmctf_convert_chroma_u8", b_chroma("chroma_u8 up", 8, ("420", "444"))),
    Row("convert_chroma_u8 444->422", "pmctf_convert_chroma_u8", b_chroma("chroma_u8 x", 8, ("444", "422"))),
    Row("convert_chroma_u8 422->420", "pmctf_convert_chroma_u8", b_chroma("chroma_u8 y", 8, ("422", "420"))),
    Row("convert_chroma_u16 444->420", "pmctf_convert_chroma_u16", b_chroma("chroma_u16", 12, ("444", "420"))),
    # ---- pixel layouts
    Row("unpack_layout_u8", "pmctf_unpack_layout_u8", b_layout("unpack_u8", "nv12", False)),
    Row("unpack_layout_u16", "pmctf_unpack_layout_u16", b_layout("unpack_u16", "p010", False)),
    Row("pack_layout_u8", "pmctf_pack_layout_u8", b_layout("pack_u8", "yuyv", True)),
    Row("pack_layout_u16", "pmctf_pack_layout_u16", b_layout("pack_u16", "v210", True)),
    # ---- scene analysis (with its clears), hashes, the diagnostic probe
    Row("luma_activity", "pmctf_luma_activity_f32", b_luma("luma_activity", True)),
    Row("luma_activity no prev", "pmctf_luma_activity_f32", b_luma("luma_activity no prev", False)),
    Row("crc32_segments", "pmctf_crc32_segments", b_crc("crc32_segments")),
    Row("math_probe", "pmctf_math_probe_f32", b_probe("math_probe")),
]
