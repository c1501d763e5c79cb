"""The census table (conv_census.py) against the text of csrc/conv_mfma.hip and against the built library: every kernel
expression the dispatcher can launch, every instantiation of it the library holds and every tuning knob is in the
table, so a new kernel, instantiation or knob cannot land without a census row (or an UNREACHABLE entry) or a restored
default."""
import os
import re

import numpy as np
import pytest

import conv_census as cc

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "learned-pmctf_amd")
SRC = os.path.join(PKG, "csrc", "conv_mfma.hip")
LIB = os.path.join(PKG, "lib", "libpmctf_hip.so")            # built by conftest.py where it is missing


@pytest.fixture(scope="module")
def source():
    with open(SRC) as f:
        return f.read()


def _first_macro_argument(text, start):
    """the argument that begins at text[start], up to the first comma outside parentheses"""
    depth, i = 0, start
    while depth > 0 or text[i] != ",":
        depth += {"(": 1, ")": -1}.get(text[i], 0)
        i += 1
    return text[start:i]


def launched_expressions(source):
    """first argument of every CONV_LAUNCH( (outer parentheses stripped) + the literal of every direct note_launch(" """
    found = set()
    for m in re.finditer(r"\bCONV_LAUNCH\(", source):
        arg = _first_macro_argument(source, m.end())
        if arg.strip() != "kernel":                      # the macro's own definition
            found.add(cc.strip_parens(" ".join(arg.split())))
    found |= set(re.findall(r'\bnote_launch\("([^"]+)"', source))
    return found


def census_expressions():
    return {e[0] for r in cc.CENSUS for e in r[7]}


def _launch_key(name, a):
    """(kernel expression, MT, NT) under which note_launch reports the instantiation name<a...>"""
    if name in ("conv_mfma_kernel", "conv_mfma_bsum_kernel"):
        return (name + "<MT, NT, TW16>", a[0], a[1])
    if name == "conv_mfma_pipe_kernel":
        return (f"{name}<MT, NT, TW16, {a[3]}>", a[0], a[1])
    if name == "conv_mfma_wave_kernel":                     # <MT, MAXP, NBUF>, launched on 8x32 tiles only
        return (name + ("<MT, 7, 1>" if a[2] == 1 else "<MT, 7>"), a[0], 4)
    if name == "conv3x3s1_wave_kernel":                     # <MT, NBUF, BSUM, MOFF>, 8x32 tiles only
        if a[3] >= 0:
            return (f"{name}<{a[0]}, {a[1]}, true, {a[3]}>", 7, 4)
        return (name + ("<MT, NB, true>" if a[2] else f"<MT, {a[1]}>"), a[0], 4)
    if name == "conv3x3s1_pipe_kernel":                     # <MT, S, BSUM>, 4x16 tiles only
        return (name + (f"<MT, {a[1]}, true>" if a[2] else "<MT>" if a[1] == 1 else "<MT, 2>"), a[0], 1)
    if name == "conv7x7s1_pipe_kernel":
        return (name + ("<MT, NT, true>" if a[2] else "<MT, NT>"), a[0], a[1])
    if name == "conv_mfma_res_kernel":
        return (name + "<MT>", a[0], 1)
    if name == "conv16_band_kernel":
        return (name, a[0], 1)
    if name == "conv1x1_kernel":
        return (name + ("<MTW, NT, true>" if a[2] else "<MTW, NT>"), a[0], a[1])
    raise KeyError(name)


def instantiated_keys(library):
    """every convolution kernel instantiation whose (mangled) name the built library holds, as launch keys"""
    with open(library, "rb") as f:
        data = f.read()
    keys = set()
    for name, args in set(re.findall(rb"_ZN12_GLOBAL__N_1\d+(conv[a-z0-9_]+_kernel)I((?:L[ib]n?\d+E)+)EEvNS_8ConvArgsE", data)):
        keys.add(_launch_key(name.decode(), [(-1 if n else 1) * int(v) for n, v in re.findall(rb"L[ib](n?)(\d+)E", args)]))
    for plain, key in (("conv16_persistent_kernel", (1, 1)), ("conv3x3s1_blocks_tileouter_kernel", (7, 4))):
        if re.search(rb"_ZN12_GLOBAL__N_1\d+" + plain.encode() + rb"ENS_8ConvArgsE", data):
            keys.add((plain,) + key)
    return keys


def test_every_launched_expression_has_a_row(source):
    in_source = launched_expressions(source)
    assert len(in_source) >= 23, sorted(in_source)
    listed = census_expressions() | {u[0] for u in cc.UNREACHABLE}
    assert in_source == listed, f"without a census row: {sorted(in_source - listed)}; not in the source: {sorted(listed - in_source)}"


def test_every_instantiation_in_the_library_has_a_row_or_is_listed_unreachable(source):
    """the (expression, MT, NT) of every kernel the library was built with, against the rows' launch keys"""
    built = instantiated_keys(LIB)
    assert len(built) > 100 and {k[0] for k in built} == launched_expressions(source)
    rows = {(expr, mt, nt) for r in cc.CENSUS for expr, mt, nt, tw16 in r[7]}
    unreachable = {u[:3] for u in cc.UNREACHABLE}
    assert not rows & unreachable, sorted(rows & unreachable)
    assert all(u[3] for u in cc.UNREACHABLE)                 # each with the condition that excludes it
    assert built == rows | unreachable, (f"instantiated without a row: {sorted(built - rows - unreachable)}; "
                                         f"in the table, not in the library: {sorted((rows | unreachable) - built)}")


def test_knob_names_and_defaults(source):
    table = re.search(r"Knob g_knobs\[\] = \{(.*?)\};", source, re.S).group(1)
    knobs = {n: int(v) for n, v in re.findall(r'\{"([A-Z0-9_]+)",\s*(-?\d+),\s*false\}', table)}
    assert len(knobs) == 21 and knobs == cc.KNOBS
    for r in cc.CENSUS:
        assert set(r[6]) <= set(cc.KNOBS), r[0]


def test_row_ids_are_unique_and_rows_well_formed():
    ids = [r[0] for r in cc.CENSUS]
    assert len(set(ids)) == len(ids)
    for rid, geometry, rule, act, slope, nres, knobs, expected in cc.CENSUS:
        assert len(geometry) == 8 and rule in (0, 1, 32) and act in range(5) and nres in (0, 1, 2) and expected, rid
        assert rule != 32 or geometry[1] > 32, rid           # a reduce block of the whole depth is the chain
        assert max(cc.out_hw(geometry)) > 0 and (geometry[0] * geometry[2] * geometry[3] <= 34000 or rid.startswith("rowsplit")), rid


def test_every_expression_sees_two_residuals_and_a_partial_cout_tile():
    two_res, partial = set(), set()
    for rid, geometry, rule, act, slope, nres, knobs, expected in cc.CENSUS:
        for expr, *_ in expected:
            if nres == 2:
                two_res.add(expr)
            if geometry[4] % 16:
                partial.add(expr)
    every = census_expressions()
    assert every - two_res == set(), sorted(every - two_res)
    assert every - partial == cc.WHOLE_TILE_ONLY, sorted(every - partial)


def test_every_expression_sees_more_than_one_epilogue():
    epilogues = {}
    for rid, geometry, rule, act, slope, nres, knobs, expected in cc.CENSUS:
        for expr, *_ in expected:
            epilogues.setdefault(expr, set()).add((act, nres))
    assert all(len(v) > 1 for v in epilogues.values()), {k: v for k, v in epilogues.items() if len(v) < 2}


def test_parse_launch():
    s = ("(conv3x3s1_wave_kernel<MT, 2>) [MT=7 NT=4 TW16=2] grid 510x1x1 + "
         "conv3x3s1_blocks_tileouter_kernel [MT=7 NT=4 TW16=2] grid 17x1x2 + conv16_band_kernel [MT=3 NT=1 TW16=1] grid 768x1x1")
    assert cc.parse_launch(s) == [("conv3x3s1_wave_kernel<MT, 2>", 7, 4, 2), ("conv3x3s1_blocks_tileouter_kernel", 7, 4, 2),
                                  ("conv16_band_kernel", 3, 1, 1)]
    with pytest.raises(ValueError):
        cc.parse_launch("")
    with pytest.raises(ValueError):
        cc.parse_launch("(conv_mfma_kernel<MT, NT, TW16>) [MT=1 NT=1 TW16=1]")


def test_case_data_follows_the_row_id():
    a, b = cc.case_data(cc.row("wave33_nbuf1_mt1")), cc.case_data(cc.row("wave33_nbuf2_mt1"))
    assert a[0].shape == b[0].shape == (2, 32, 13, 37) and a[1].shape == (8, 32, 3, 3) and (a[0] != b[0]).any()
    assert len(a[3]) == 2 and a[3][0].shape == (2, 8, 13, 37) and a[0].dtype == a[1].dtype == a[3][1].dtype
    again = cc.case_data(cc.row("wave33_nbuf1_mt1"))
    assert all((p == q).all() for p, q in zip(a[:3], again[:3]))


# ---- the rows on special data (conv_census.DATA) --------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_every_expression_has_its_special_rows():
    """a zero, a no-bias and a subnormal row per launched expressions and rule the table runs them under; zero rows with a padded last k-step (Cin = 8 and 20) for the two generic kernels, the only ones that take
    Cin % 16 != 0, under both rules"""
    base = cc.CENSUS[:cc.N_BASE]
    assert not any(r[0] in cc.DATA for r in base) and all(r[0] in cc.DATA for r in cc.CENSUS[cc.N_BASE:])
    kinds = {}
    for r in cc.CENSUS[cc.N_BASE:]:
        kinds.setdefault(cc.DATA[r[0]], set()).add((tuple(e[0] for e in r[7]), r[2]))
    every = {(tuple(e[0] for e in r[7]), r[2]) for r in base}
    assert kinds["zeros"] == kinds["nobias"] == kinds["subnormal"] == every
    padded = [r for r in cc.CENSUS if cc.DATA.get(r[0]) == "zeros" and r[1][1] % 16]
    assert {(r[1][1], r[2], r[7][0][0]) for r in padded} == {(cin, rule, expr) for cin in (8, 20) for rule, expr in (
        (0, "conv_mfma_kernel<MT, NT, TW16>"), (1, "conv_mfma_bsum_kernel<MT, NT, TW16>"))}
    assert {r[7][0][2] for r in padded} >= {1, 2, 4}                      # on every tile shape
    for r in cc.CENSUS[cc.N_BASE:]:
        if cc.DATA[r[0]] != "nobias":
            assert r[5] == 0 and r[3] <= 2, r[0]                           # nothing that buries the sign of a zero
    assert cc.case_data(cc.row("wave33_nbuf1_mt1__nobias"))[2] is None


@pytest.mark.parametrize("rid", [r[0] for r in cc.CENSUS if cc.DATA.get(r[0]) in ("zeros", "subnormal")])
def test_precondition_of_the_special_row(rid):
    """zero rows: the plane has a border and an interior, the data is the shared generator's (-0 bias, the three patches),
    the oracle's output holds both signs of zero, and a kernel that skipped the taps outside the image instead of
    multiplying their zeros in would give other bits in at least one element of the border.  Subnormal rows: a subnormal
    result."""
    import valu_conv_census as vc
    from pmctf_oracle import clib
    r = cc.row(rid)
    (N, Cin, H, W, Cout, K, S, pad), rule = r[1], r[2]
    x, w, b, res = cc.case_data(r)
    out = clib.conv2d(x, w, b, S, (pad, pad), rule)
    if cc.DATA[rid] == "subnormal":
        assert vc.is_subnormal(out).any()
        return
    u = _bits(x)
    (a0, a1), (b0, b1), (c0, c1) = vc.zero_patches(K)
    assert (u[..., a0:a1] == 0x80000000).all() and (u[..., b0:b1] == 0).all() and (u[..., c0:c1] == 0x80000001).all()
    assert (_bits(b) == 0x80000000).all() and (w >= 0.25).all() and (w <= 0.375).all() and not res
    assert H >= 3 and W > c1
    o = _bits(out)
    assert (o == 0x80000000).any() and (o == 0).any(), f"{rid}: the oracle's output lacks a sign of zero"
    if pad:
        Ho, Wo = cc.out_hw(r[1])
        assert Ho >= 3 and Wo >= 3
        border = np.ones((Ho, Wo), bool)
        border[1:-1, 1:-1] = False
        skipped = _bits(cc.skipping_conv(x, w, b, S, pad, rule))
        differs = o != skipped
        assert differs[..., border].any(), f"{rid}: skipping the padded taps gives the oracle's bits on the whole border"
        # whatever differs, differs in the sign of a zero and in nothing else
        assert ((o[differs] | 0x80000000) == 0x80000000).all() and ((skipped[differs] | 0x80000000) == 0x80000000).all()


def test_skipping_conv_is_the_depthwise_oracle():
    """the construction behind the precondition, against the one oracle that does skip: on one channel the dense
    convolution of the -0-extended image equals the depthwise convolution, bit for bit"""
    import valu_conv_census as vc
    from pmctf_oracle import clib
    r = cc.row("wave33_nbuf1_mt1__zeros")
    x, w, b, _ = cc.case_data(r)
    x1, w1, b1 = x[:, :1], w[:1, :1], b[:1]
    assert (_bits(cc.skipping_conv(x1, w1, b1, 1, 1, 0)) == _bits(clib.dwconv2d(x1, w1, b1))).all()
    assert (_bits(clib.conv2d(x1, w1, b1, 1, (1, 1), 0)) != _bits(clib.dwconv2d(x1, w1, b1))).any()


@pytest.mark.parametrize("case", cc.GEOM_ZERO, ids=[c[0] for c in cc.GEOM_ZERO])
def test_precondition_of_the_per_class_zero_cases(case):
    """per parity class: the oracle's output holds both signs of zero; a kernel that skipped the taps outside the image
    would differ from it on the edges the class pads (class 0: the first row and column, class 3: the last; under rule
    blocks only on the last ones: class 0 is then a case where skipping and multiplying agree) and, away from the image's
    corners, on no edge it does not pad; whatever differs, differs in the sign of a zero only"""
    ref, skipped = cc.geom_zero_reference(case)
    for cls in range(4):
        py, px = cls >> 1, cls & 1
        o, s = _bits(ref[cls]), _bits(skipped[cls])
        assert (o == 0x80000000).any() and (o == 0).any(), (case[0], cls)
        d = o != s
        assert ((o[d] | 0x80000000) == 0x80000000).all() and ((s[d] | 0x80000000) == 0x80000000).all()
        padded_row, bare_row = (-1, 0) if py else (0, -1)
        padded_col, bare_col = (-1, 0) if px else (0, -1)
        # Under the chain from the bias (-0) any padded zero turns the sum to +0.  Where the chain starts at +0 the sign of
        # a sum of zeros is that of its last tap: a padded tap shows only where it comes after the image's, below or right.
        rule = case[2]
        assert d[..., padded_row, 1:-1].any() == (rule == 0 or py == 1), (case[0], cls)
        assert d[..., 1:-1, padded_col].any() == (rule == 0 or px == 1), (case[0], cls)
        assert not d[..., 1:-1, 1:-1].any() and not d[..., bare_row, 1:-1].any() and not d[..., 1:-1, bare_col].any(), (case[0], cls)
