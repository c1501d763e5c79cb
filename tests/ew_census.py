"""Census of the elementwise dispatcher of csrc/ew_ops.hip: a row for every kernel instantiation pmctf_ew_f32,
pmctf_nearest_up2_nhwc_f32 and pmctf_pixel_shuffle2_nhwc_f32 can launch on planes of tests' size, and a row next to every
condition of the dispatch.  A row names the kernel it must launch (what pmctf_ew_last_launch reports), so a moved condition
fails on the name instead of passing on another kernel.  Plain data and helpers: importing this module needs neither the
product nor a GPU.

A row of EW: (id, (N, C, H, W), cfast, out, a, b, expected for unary ops, expected for binary ops, options)
  out, a, b   (buffer, offset, strides): a view of `dims` into a buffer of that name, in elements.  Buffers "out", "a", "b"
              are separate allocations, 16-byte aligned, sentinel-filled; an operand whose buffer is "out" shares the
              output's allocation (in place).  b = None: no row of this id runs a binary op.
  expected    the launch expression, with " channels" / " rows" for the two forms of ew_c4_kernel
  options     ops: the op codes the row runs (default: all 18); the rows of 2^18 elements run two
Every op runs on operands drawn from the special set (edge_values.SPECIALS: for binary ops every pair of the set occurs on
planes of 256 elements and more: 0/0, x/0, inf-inf, 0*inf) and on ordinary values.  The whole output buffer is compared:
the sentinels around the view and, for strided outputs, the elements between the written ones.
"""
import numpy as np

import edge_values as ev
import math_sweep as ms

EW_COPY, EW_ADD, EW_SUB, EW_MUL, EW_DIV, EW_MULS, EW_DIVS, EW_ADD_MULS, EW_SUB_MULS, EW_ADD_MULS_MULS, \
    EW_CLAMP_MULS, EW_ROUND_CLAMP_MULS, EW_ROUND, EW_LEAKY, EW_ADD_MULS2, EW_SUB_MULS2, EW_ROUND_CLAMP, EW_TANH = range(18)
BINARY = (EW_ADD, EW_SUB, EW_MUL, EW_DIV, EW_ADD_MULS, EW_SUB_MULS, EW_ADD_MULS_MULS, EW_ADD_MULS2, EW_SUB_MULS2)
UNARY = tuple(op for op in range(18) if op not in BINARY)
NAMES = ["COPY", "ADD", "SUB", "MUL", "DIV", "MULS", "DIVS", "ADD_MULS", "SUB_MULS", "ADD_MULS_MULS", "CLAMP_MULS",
         "ROUND_CLAMP_MULS", "ROUND", "LEAKY", "ADD_MULS2", "SUB_MULS2", "ROUND_CLAMP", "TANH"]

FLAT_V, FLAT_S, TRANSPOSE = "ew_flat_kernel<true>", "ew_flat_kernel<false>", "ew_transpose_kernel"
C4_CH, C4_ROWS = "ew_c4_kernel<int> channels", "ew_c4_kernel<int> rows"
GEN_C, GEN_P = "ew_kernel<true, int>", "ew_kernel<false, int>"
# instantiations no row of THIS table reaches: they need 2^31 elements (8 GiB per operand) and are rows of the large-plane
# census (large_planes.py, the "ew_*__over" rows), next to their int neighbours just under 2^31
LARGE_PLANES = {"ew_c4_kernel<long>": "ew_c4__over", "ew_kernel<true, long>": "ew_cfast__over",
                "ew_kernel<false, long>": "ew_planar__over"}
SENT = 0x5A5A5A5A
PAD = 64                    # sentinel words before and after every view's extent


def params(op):
    return (-2.0, 3.0) if op == EW_ROUND_CLAMP else (0.37, 2.25)


def expected(op, a, b, alpha, beta):
    """numpy float32 restatement of ew_apply (one rounding per written operation)"""
    from pmctf_oracle import clib
    f = np.float32
    al, be = f(alpha), f(beta)
    with np.errstate(all="ignore"):
        if op == EW_COPY: return a.copy()
        if op == EW_ADD: return a + b
        if op == EW_SUB: return a - b
        if op == EW_MUL: return a * b
        if op == EW_DIV: return a / b
        if op == EW_MULS: return a * al
        if op == EW_DIVS: return a / al
        if op == EW_ADD_MULS: return a + b * al
        if op == EW_SUB_MULS: return a - b * al
        if op == EW_ADD_MULS_MULS: return (a + b * al) * be
        if op == EW_CLAMP_MULS: return np.clip(a * al, -be, be)
        if op == EW_ROUND_CLAMP_MULS: return np.rint(np.clip(a * al, -be, be))
        if op == EW_ROUND: return np.rint(a)
        if op == EW_LEAKY: return np.where(a > 0, a, a * al).astype(f)
        if op == EW_ADD_MULS2: return a + (b * al) * be
        if op == EW_SUB_MULS2: return a - (b * al) * be
        if op == EW_ROUND_CLAMP: return np.rint(np.clip(a, al, be))
        if op == EW_TANH: return clib.tanh(a)
    raise AssertionError(op)


def torch_op(op, a, b, alpha, beta):
    """the torch expression each PMCTF_EW_* code replaces (include/pmctf_hip.h), on CPU tensors"""
    import torch
    import torch.nn.functional as F
    if op == EW_COPY: return a.clone()
    if op == EW_ADD: return a + b
    if op == EW_SUB: return a - b
    if op == EW_MUL: return a * b
    if op == EW_DIV: return a / b
    if op == EW_MULS: return a * alpha
    if op == EW_DIVS: return a / alpha
    if op == EW_ADD_MULS: return a + b * alpha
    if op == EW_SUB_MULS: return a - b * alpha
    if op == EW_ADD_MULS_MULS: return (a + b * alpha) * beta
    if op == EW_CLAMP_MULS: return torch.clamp(a * alpha, -beta, beta)
    if op == EW_ROUND_CLAMP_MULS: return torch.round(torch.clamp(a * alpha, -beta, beta))
    if op == EW_ROUND: return torch.round(a)
    if op == EW_LEAKY: return F.leaky_relu(a, alpha)
    if op == EW_ADD_MULS2: return a + (b * alpha) * beta
    if op == EW_SUB_MULS2: return a - (b * alpha) * beta
    if op == EW_ROUND_CLAMP: return torch.round(torch.clamp(a, alpha, beta))
    raise AssertionError(op)               # EW_TANH is PM-F32's tanh: tests/test_oracle_math.py, test_math_sweep_cpu.py


# ---- strides of the layouts, in elements -------------------------------------------------------------------------------
def planar(d, row=None, rows=1):
    """dense planes; row: the distance between two rows (a column window), rows: every rows-th row of a taller plane"""
    N, C, H, W = d
    row = row or W
    return (C * H * rows * row, H * rows * row, rows * row, 1)


def nhwc(d, ct=None):
    """channels last; ct: the channel count of the tensor the view is a slice of"""
    N, C, H, W = d
    ct = ct or C
    return (H * W * ct, 1, W * ct, ct)


def transposed(d):
    N, C, H, W = d
    return (C * H * W, H * W, 1, H)


def _row(rid, d, cfast, out, a, b, unary, binary=None, **options):
    norm = lambda v, name: None if v is None else ((name, 0, v) if len(v) == 4 else v)
    return (rid, d, cfast, norm(out, "out"), norm(a, "a"), norm(b, "b"), unary, binary if binary is not None else unary, options)


D = (2, 4, 5, 8)            # 320 elements: every pair of the special set occurs; C % 4 == 0 and W % 4 == 0
D6 = (2, 6, 5, 8)           # C % 4 != 0
D7 = (2, 4, 5, 7)           # W % 4 != 0, total % 4 == 0
ODD = (1, 3, 5, 7)          # total % 4 != 0
T = (2, 3, 5, 11)           # the transposed form: two planes of three channels, H and W no multiples of the 32x32 tile
TWO = [EW_COPY, EW_ROUND]

EW = [
    # ---- one row per reachable expression ---------------------------------------------------------------------------
    _row("flat_vec", D, 0, planar(D), planar(D), planar(D), FLAT_V),
    _row("flat_vec_nhwc", D, 1, nhwc(D), nhwc(D), nhwc(D), FLAT_V),
    _row("flat_scalar", ODD, 0, planar(ODD), planar(ODD), planar(ODD), FLAT_S),
    _row("transpose", T, 0, planar(T), transposed(T), planar(T), TRANSPOSE, GEN_P),       # a binary op: the generic kernel
    _row("c4_channels", D, 1, nhwc(D), ("a", 4, nhwc(D, 12)), ("b", 8, nhwc(D, 16)), C4_CH),
    _row("c4_channels_out_slice", D, 1, ("out", 4, nhwc(D, 8)), nhwc(D), nhwc(D), C4_CH),
    _row("c4_rows", D, 0, planar(D), planar(D, rows=2), ("b", 8, planar(D, rows=2)), C4_ROWS),
    _row("c4_rows_out_window", D, 0, ("out", 4, planar(D, row=16)), planar(D), planar(D), C4_ROWS),
    _row("generic_cfast", D6, 1, nhwc(D6), ("a", 4, nhwc(D6, 12)), nhwc(D6), GEN_C),      # C % 4 != 0
    _row("generic_planar", D7, 0, planar(D7), ("a", 4, planar(D7, row=12)), planar(D7), GEN_P),        # W % 4 != 0
    # ---- neighbours of the flat form ----------------------------------------------------------------------------------
    _row("flat_out_misaligned", D, 0, ("out", 1, planar(D)), planar(D), planar(D), FLAT_S),
    _row("flat_a_misaligned", D, 0, planar(D), ("a", 3, planar(D)), planar(D), FLAT_S),
    _row("flat_b_misaligned", D, 0, planar(D), planar(D), ("b", 2, planar(D)), FLAT_V, FLAT_S),       # unary ops pass no b
    _row("flat_b_broadcast", D, 0, planar(D), planar(D), (0, 0, 8, 1), FLAT_V, C4_ROWS),              # b: one plane for all
    _row("flat_b_broadcast_w7", D7, 0, planar(D7), planar(D7), (0, 0, 7, 1), FLAT_V, GEN_P),
    _row("flat_size1_dims", (1, 1, 8, 40), 0, (12345, 777, 40, 1), (54321, 3, 40, 1), (7, 99, 40, 1), FLAT_V),
    _row("flat_size1_hw", (2, 4, 1, 1), 0, (4, 1, 999, 777), (4, 1, 5, 6), (4, 1, 1, 1), FLAT_V),
    _row("flat_in_place", D, 0, planar(D), ("out", 0, planar(D)), planar(D), FLAT_V),
    _row("flat_in_place_b", D, 0, planar(D), planar(D), ("out", 0, planar(D)), FLAT_V),
    # ---- neighbours of the channel form -------------------------------------------------------------------------------
    _row("c4_channels_a_misaligned", D, 1, nhwc(D), ("a", 3, nhwc(D, 12)), nhwc(D), GEN_C),
    _row("c4_channels_out_misaligned", D, 1, ("out", 2, nhwc(D, 8)), nhwc(D), nhwc(D), GEN_C),
    _row("c4_channels_b_misaligned", D, 1, nhwc(D), ("a", 4, nhwc(D, 12)), ("b", 1, nhwc(D, 8)), C4_CH, GEN_C),
    _row("c4_channels_odd_slice", D, 1, nhwc(D), ("a", 4, nhwc(D, 19)), nhwc(D), GEN_C),       # pixel stride 19: not 16-byte
    _row("c4_channels_b_odd_slice", D, 1, nhwc(D), ("a", 4, nhwc(D, 12)), ("b", 0, nhwc(D, 7)), C4_CH, GEN_C),
    _row("c4_channels_in_place", D, 1, ("out", 4, nhwc(D, 8)), ("out", 4, nhwc(D, 8)), nhwc(D), C4_CH),
    _row("c4_channels_b_broadcast", D, 1, nhwc(D), ("a", 4, nhwc(D, 12)), (0, 1, 0, 0), C4_CH),        # one pixel for all
    # ---- neighbours of the row form -----------------------------------------------------------------------------------
    _row("c4_rows_w7", D7, 0, planar(D7), planar(D7, rows=2), planar(D7, rows=2), GEN_P),
    _row("c4_rows_a_misaligned", D, 0, planar(D), ("a", 1, planar(D, rows=2)), planar(D), GEN_P),
    _row("c4_rows_out_misaligned", D, 0, ("out", 2, planar(D, row=16)), planar(D), planar(D), GEN_P),
    _row("c4_rows_b_misaligned", D, 0, planar(D), planar(D, rows=2), ("b", 3, planar(D, rows=2)), C4_ROWS, GEN_P),
    _row("c4_rows_odd_row_stride", D, 0, planar(D), ("a", 0, planar(D, row=9)), planar(D), GEN_P),
    _row("c4_rows_in_place", D, 0, ("out", 0, planar(D, rows=2)), ("out", 0, planar(D, rows=2)), planar(D), C4_ROWS),
    # ---- neighbours of the transposed form: H == 1 and W == 1 are dense (flat), planes that overlap or repeat are not ----
    _row("transpose_h1", (2, 3, 1, 11), 0, planar((2, 3, 1, 11)), transposed((2, 3, 1, 11)), None, FLAT_S),
    _row("transpose_w1", (2, 4, 7, 1), 0, planar((2, 4, 7, 1)), transposed((2, 4, 7, 1)), None, FLAT_V),
    _row("transpose_a_plane_repeats", T, 0, planar(T), (0, 0, 1, 5), None, GEN_P),            # plane strides below H * W
    _row("transpose_a_planes_overlap", (1, 2, 5, 11), 0, planar((1, 2, 5, 11)), (0, 5, 1, 5), None, GEN_P),
    _row("transpose_nc_65535", (1, 65535, 2, 2), 0, planar((1, 65535, 2, 2)), transposed((1, 65535, 2, 2)), None, TRANSPOSE,
         ops=TWO),
    _row("transpose_nc_65536", (1, 65536, 2, 2), 0, planar((1, 65536, 2, 2)), transposed((1, 65536, 2, 2)), None, GEN_P,
         ops=TWO),
    _row("transpose_one_plane", (1, 1, 33, 40), 0, planar((1, 1, 33, 40)), transposed((1, 1, 33, 40)), None, TRANSPOSE),
]
N_ROWS = 39

# nearest_up2 and pixel_shuffle2 choose their form by C % 4 alone: (id, entry, (N, H, W, C), expected)
COPIES = [
    ("nearest_scalar", "nearest_up2", (2, 5, 7, 6), "nearest_up2_kernel"),
    ("nearest_vec4", "nearest_up2", (2, 5, 7, 8), "nearest_up2_vec4_kernel"),
    ("nearest_c1", "nearest_up2", (1, 3, 3, 1), "nearest_up2_kernel"),
    ("shuffle_scalar", "pixel_shuffle2", (2, 5, 7, 6), "pixel_shuffle2_kernel"),
    ("shuffle_vec4", "pixel_shuffle2", (2, 5, 7, 4), "pixel_shuffle2_vec4_kernel"),
    ("shuffle_c1", "pixel_shuffle2", (1, 3, 3, 1), "pixel_shuffle2_kernel"),
]


def row(rid):
    return next(r for r in EW if r[0] == rid)


def ops_of(r):
    ops = r[8].get("ops", list(range(18)))
    return [op for op in ops if r[5] is not None or op in UNARY]


def expected_kernel(r, op):
    return r[7] if op in BINARY else r[6]


def all_expressions():
    return {r[6] for r in EW} | {r[7] for r in EW} | {c[3] for c in COPIES}


def parse_launch(s):
    """'kernel expression[ channels| rows] grid G' (pmctf_ew_last_launch) -> (expression with its form, G)"""
    expr, sep, grid = s.rpartition(" grid ")
    if not sep or not expr or not grid.isdigit():
        raise ValueError(f"not a launch record: {s!r}")
    return expr, int(grid)


# ---- buffers and views ---------------------------------------------------------------------------------------------------
def extent(d, view):
    """(first, one past the last) element of a view, relative to its buffer's origin"""
    _, off, st = view
    return off, off + sum((n - 1) * s for n, s in zip(d, st)) + 1


def layout(r):
    """-> {buffer name: length in elements}, PAD sentinels on both sides of the union of the views in it"""
    d = r[1]
    size = {}
    for view in (r[3], r[4], r[5]):
        if view is not None:
            lo, hi = extent(d, view)
            assert lo >= 0
            size[view[0]] = max(size.get(view[0], 0), hi)
    return {k: v + 2 * PAD + (-v) % 4 for k, v in size.items()}


def host_view(buf, d, view):
    _, off, st = view
    return np.lib.stride_tricks.as_strided(buf[PAD + off:], shape=d, strides=[4 * s for s in st], writeable=True)


def operands(r, data, seed=0):
    """host buffers of the row, sentinel-filled, with operand values written through the a and b views.
    data "specials": a walks the special set, b changes every 16 elements, so that every pair occurs within 256 elements;
    "normal": ordinary values, b away from 0"""
    d = r[1]
    n = int(np.prod(d))
    bufs = {k: np.full(v, SENT, np.uint32).view(np.float32) for k, v in layout(r).items()}
    rng = np.random.default_rng([11, seed, n])
    i = np.arange(n)
    if data == "specials":
        av = ev.SPECIALS[(i + seed) % 16]
        bv = ev.SPECIALS[(i // 16 + seed) % 16]
    else:
        av = (rng.standard_normal(n) * 3).astype(np.float32)
        bv = (rng.standard_normal(n) + 2.5).astype(np.float32)
    for view, vals in ((r[4], av), (r[5], bv)):
        if view is not None:
            host_view(bufs[view[0]], d, view)[...] = vals.reshape(d)
    return bufs


def reference(r, op, bufs):
    """the whole output buffer after the op: the restatement's values at the positions of the output view, every other
    element as it was"""
    d = r[1]
    a = np.ascontiguousarray(host_view(bufs[r[4][0]], d, r[4]))
    b = np.ascontiguousarray(host_view(bufs[r[5][0]], d, r[5])) if (r[5] is not None and op in BINARY) else None
    want = bufs["out"].copy()
    host_view(want, d, r[3])[...] = expected(op, a, b, *params(op))
    return want


def written_once(r):
    """no two index tuples of the output view address the same element"""
    d = r[1]
    idx = np.zeros(d, np.int64)
    for axis, (n, s) in enumerate(zip(d, r[3][2])):
        shape = [1] * 4
        shape[axis] = n
        idx = idx + (np.arange(n) * s).reshape(shape)
    return np.unique(idx).size == idx.size


def run_row(r, op, data, seed=0):
    """-> (launch record, the whole output buffer as the GPU left it, the reference buffer)"""
    import ctypes as C
    import torch
    from pMCTF.hip import lib, ops
    d = r[1]
    bufs = operands(r, data, seed)
    want = reference(r, op, bufs)
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in bufs.items()}
    for t in dev.values():
        assert t.data_ptr() % 16 == 0
    ptr = lambda view: C.c_void_p(dev[view[0]].data_ptr() + 4 * (PAD + view[1]))
    i64x4 = C.c_int64 * 4
    binary = op in BINARY
    alpha, beta = params(op)
    rc = lib.hip().pmctf_ew_f32(op, ptr(r[3]), i64x4(*r[3][2]), ptr(r[4]), i64x4(*r[4][2]), ptr(r[5]) if binary else None,
                                i64x4(*r[5][2]) if binary else None, *d, alpha, beta, r[2], None)
    assert rc == 0, (r[0], op, rc)
    launched = ops.ew_last_launch()
    torch.cuda.synchronize()
    return launched, dev["out"].cpu().numpy(), want


def compare(got, want):
    """-> mismatching elements of the whole buffer (NaN payloads exempt where both are NaN), index of the first"""
    count, first, _ = ms.compare(got.view(np.uint32), want.view(np.uint32))
    return count, first
