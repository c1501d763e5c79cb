"""The census table (conv_census.py) against the text of csrc/conv_mfma.hip and against the built library: every kernel
expression the dispatcher can launch, every instantiation of it the library holds and every tuning knob is in the
table, so a new kernel, instantiation or knob cannot land without a census row (or an UNREACHABLE entry) or a restored
default."""
import os
import re

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
