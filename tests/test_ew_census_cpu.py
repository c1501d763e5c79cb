"""The elementwise census (ew_census.py) against the text of csrc/ew_ops.hip, against the built library and against torch,
without a GPU: every kernel the three entry points can launch and every instantiation of it the library holds is a row's
expected kernel or listed as unreachable, every launch leaves a record, the conditions the neighbour rows sit next to are
worded as the table assumes, the rows are well formed, and the numpy restatement the GPU file compares with is the torch
operation each PMCTF_EW_* code replaces, bit for bit, on every pair of the special set."""
import os
import re

import numpy as np
import pytest
import torch

import edge_values as ev
import ew_census as ec
from test_valu_conv_census_cpu import _arguments, entry_body, vc_strip

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "learned-pmctf_amd")
SRC = os.path.join(PKG, "csrc", "ew_ops.hip")
LIB = os.path.join(PKG, "lib", "libpmctf_hip.so")            # built by conftest.py where it is missing
ENTRIES = ("pmctf_ew_f32", "pmctf_nearest_up2_nhwc_f32", "pmctf_pixel_shuffle2_nhwc_f32")
FORMS = (" channels", " rows")


@pytest.fixture(scope="module")
def source():
    with open(SRC) as f:
        return f.read()


def strip_form(expr):
    for form in FORMS:
        if expr.endswith(form):
            return expr[:-len(form)]
    return expr


def launched_expressions(source):
    """kernel expression + form of every PM_LAUNCH...( in the three entry points"""
    found, kinds = set(), set()
    for name in ENTRIES:
        body = entry_body(source, name)
        assert "clear_ew_launch();" in body.split("if (", 1)[0], f"{name} does not clear the record first"
        for m in re.finditer(r"\bPM_LAUNCH(\w*)\(", body):
            kinds.add(m.group(1))
            args = _arguments(body, m.end())
            found.add(vc_strip(args[0]) + args[1].strip('"'))
    assert kinds == {"_NOTED"}, f"a launch that leaves no record: PM_LAUNCH{sorted(kinds)}"
    return found


def instantiated(library, names):
    """the instantiations of the kernels `names` whose mangled names the built library holds, as launch expressions"""
    with open(library, "rb") as f:
        data = f.read()
    found = set()
    for name in names:
        for args in set(re.findall(rb"_ZN12_GLOBAL__N_1%d%s((?:I(?:Lb[01]E|[il])+E)?)E" % (len(name), name.encode()), data)):
            parts = [{b"Lb1E": "true", b"Lb0E": "false", b"i": "int", b"l": "long"}[p] for p in re.findall(rb"Lb[01]E|[il]", args[1:-1])]
            found.add(name + ("<" + ", ".join(parts) + ">" if parts else ""))
    return found


def test_every_launched_kernel_is_a_rows_expected_kernel(source):
    in_source = launched_expressions(source)
    assert len(in_source) == 15, sorted(in_source)
    import large_planes as lp
    reachable = {e for e in in_source if strip_form(e) not in ec.LARGE_PLANES}
    assert {strip_form(e) for e in in_source - reachable} == set(ec.LARGE_PLANES)
    for expr, rid in ec.LARGE_PLANES.items():                   # the 2^31-element forms: rows of the large-plane census
        assert strip_form(lp.row(rid)[7]) == expr and lp.row(rid)[1] == "ew" and lp.row(rid)[9] == "over", expr
        under = lp.row(rid.replace("__over", "__under"))
        assert strip_form(under[7]) == expr.replace("long", "int"), expr
    assert reachable == ec.all_expressions(), (f"without a row: {sorted(reachable - ec.all_expressions())}; "
                                               f"not in the source: {sorted(ec.all_expressions() - reachable)}")


def test_every_instantiation_in_the_library_has_a_row_or_a_reason(source):
    names = {strip_form(e).split("<")[0] for e in launched_expressions(source)}
    kernels = set(re.findall(r"__global__ (?:__launch_bounds__\(\d+\) )?void ((?:ew_|nearest_up2|pixel_shuffle2)\w*)\(", source))
    assert kernels == names, sorted(kernels ^ names)
    built = instantiated(LIB, names)
    rows = {strip_form(e) for e in ec.all_expressions()}
    large = set(ec.LARGE_PLANES)
    assert built == rows | large, (f"instantiated without a row: {sorted(built - rows - large)}; "
                                   f"in the table, not in the library: {sorted((rows | large) - built)}")
    assert not rows & large


def test_conditions_the_rows_sit_next_to(source):
    """the dispatch conditions as the source words them: a reworded or moved condition shows up here, and on the GPU as a
    wrong kernel name"""
    flat = " ".join(source.split())
    for text in ("const bool vec = (total & 3) == 0 && (((uintptr_t)out | (uintptr_t)a | (uintptr_t)b) & 15) == 0;",
                 "if (!b && H > 1 && W > 1 && vo.s[3] == 1 && vo.s[2] == W && va.s[2] == 1 && va.s[3] == H && (long)N * C < 65536 &&",
                 "const bool small = total < (1L << 31);",
                 "if (cfast && (C & 3) == 0 && vo.s[1] == 1 && va.s[1] == 1 && (!b || (sb && vb.s[1] == 1)) &&",
                 "if (!cfast && (W & 3) == 0 && vo.s[3] == 1 && va.s[3] == 1 && (!b || (sb && vb.s[3] == 1)) &&"):
        assert text in flat, text
    for name in ENTRIES[1:]:
        assert "if ((C & 3) == 0) {" in entry_body(source, name)


def test_rows_are_well_formed():
    ids = [r[0] for r in ec.EW]
    assert len(set(ids)) == len(ids) == ec.N_ROWS
    for r in ec.EW:
        rid, d, cfast, out, a, b, unary, binary, options = r
        assert cfast in (0, 1) and set(options) <= {"ops"} and out[0] == "out", rid
        assert ec.written_once(r), rid
        sizes = ec.layout(r)                                    # asserts that no view starts before its buffer
        for view in (out, a, b):
            if view is not None:
                assert ec.extent(d, view)[1] + 2 * ec.PAD <= sizes[view[0]], rid
        n = int(np.prod(d))
        assert n <= 1 << 18, rid
        if n > 4096:
            assert options.get("ops") == ec.TWO and rid.startswith("transpose_nc_"), rid
        assert ec.ops_of(r), rid


def test_every_expression_runs_every_op_it_can():
    """per reachable expression: a row that runs all 18 ops on it (the transposed form takes unary ops only), on a plane of
    at least 256 elements, so that every pair of the special set occurs"""
    for expr in (ec.FLAT_V, ec.FLAT_S, ec.C4_CH, ec.C4_ROWS, ec.GEN_C, ec.GEN_P, ec.TRANSPOSE):
        ops = set()
        for r in ec.EW:
            if int(np.prod(r[1])) >= (256 if expr != ec.FLAT_S else 100):
                ops |= {op for op in ec.ops_of(r) if ec.expected_kernel(r, op) == expr}
        assert ops == set(ec.UNARY if expr == ec.TRANSPOSE else range(18)), (expr, sorted(set(range(18)) - ops))
    r = ec.row("flat_vec")
    bufs = ec.operands(r, "specials")
    a, b = (ec.host_view(bufs[k], r[1], v).reshape(-1).view(np.uint32) for k, v in (("a", r[4]), ("b", r[5])))
    assert len(set(zip(a.tolist(), b.tolist()))) == 256
    assert set(ec.all_expressions()) >= {c[3] for c in ec.COPIES} and len({c[3] for c in ec.COPIES}) == 4


def test_neighbour_rows_name_the_other_kernel():
    """the families the census was asked to hold, by id"""
    e = lambda rid, op: ec.expected_kernel(ec.row(rid), op)
    U, B = ec.EW_COPY, ec.EW_ADD
    assert e("flat_scalar", B) == e("flat_out_misaligned", U) == e("flat_a_misaligned", U) == ec.FLAT_S
    assert (e("flat_b_misaligned", U), e("flat_b_misaligned", B)) == (ec.FLAT_V, ec.FLAT_S)
    assert (e("flat_b_broadcast", B), e("flat_b_broadcast_w7", B)) == (ec.C4_ROWS, ec.GEN_P)
    assert e("flat_size1_dims", B) == e("flat_size1_hw", B) == e("flat_in_place", B) == ec.FLAT_V
    for rid in ("c4_channels_a_misaligned", "c4_channels_out_misaligned", "c4_channels_odd_slice", "generic_cfast"):
        assert e(rid, U) == e(rid, B) == ec.GEN_C
    assert (e("c4_channels_b_misaligned", U), e("c4_channels_b_misaligned", B)) == (ec.C4_CH, ec.GEN_C)
    for rid in ("c4_rows_w7", "c4_rows_a_misaligned", "c4_rows_out_misaligned", "c4_rows_odd_row_stride", "generic_planar"):
        assert e(rid, U) == e(rid, B) == ec.GEN_P
    assert (e("transpose", U), e("transpose", B)) == (ec.TRANSPOSE, ec.GEN_P)
    assert (e("transpose_h1", U), e("transpose_w1", U)) == (ec.FLAT_S, ec.FLAT_V)
    assert (e("transpose_nc_65535", U), e("transpose_nc_65536", U)) == (ec.TRANSPOSE, ec.GEN_P)
    assert e("transpose_a_plane_repeats", U) == e("transpose_a_planes_overlap", U) == ec.GEN_P
    assert ec.row("transpose_nc_65535")[1] == (1, 65535, 2, 2) and ec.row("transpose_nc_65536")[1] == (1, 65536, 2, 2)
    assert e("c4_channels_in_place", B) == ec.C4_CH and e("c4_rows_in_place", B) == ec.C4_ROWS


@pytest.mark.parametrize("op", [op for op in range(18) if op != ec.EW_TANH], ids=lambda op: ec.NAMES[op])
def test_restatement_is_the_torch_operation(op):
    """ew_census.expected against the torch expression the op code replaces: every pair of the special set (0/0, x/0,
    inf - inf, 0 * inf, NaN through clamp, round and leaky_relu, ties of round) and ordinary values; 4096 elements, so that
    ATen's vectorised loop and its scalar tail both run"""
    i = np.arange(256)
    rng = np.random.default_rng(op)
    a = np.concatenate([ev.SPECIALS[i % 16], (rng.standard_normal(3843) * 3).astype(np.float32)])
    b = np.concatenate([ev.SPECIALS[i // 16], (rng.standard_normal(3843) + 2.5).astype(np.float32)])
    alpha, beta = ec.params(op)
    want = ec.torch_op(op, torch.from_numpy(a), torch.from_numpy(b), alpha, beta).numpy()
    got = ec.expected(op, a, b if op in ec.BINARY else None, alpha, beta)
    exempt = ev.bits_equal(got, want, f"restatement of {ec.NAMES[op]}")
    assert np.isnan(want).any() and (op not in ec.BINARY or all(ev.zero_signs(want)) or op == ec.EW_DIV)
    assert exempt <= 64


def test_reference_keeps_the_untouched_elements():
    r = ec.row("c4_rows_out_window")
    bufs = ec.operands(r, "normal")
    want = ec.reference(r, ec.EW_ADD, bufs).view(np.uint32)
    n = int(np.prod(r[1]))
    assert (want != ec.SENT).sum() == n and (want[:ec.PAD + 4] == ec.SENT).all() and (want[-ec.PAD:] == ec.SENT).all()
    lo, hi = ec.extent(r[1], r[3])
    assert hi - lo > n                                         # elements between the written ones


def test_parse_launch():
    assert ec.parse_launch("ew_c4_kernel<int> rows grid 3") == (ec.C4_ROWS, 3)
    assert ec.parse_launch("ew_flat_kernel<true> grid 1") == (ec.FLAT_V, 1)
    for bad in ("", "ew_transpose_kernel", "ew_transpose_kernel grid x"):
        with pytest.raises(ValueError):
            ec.parse_launch(bad)
