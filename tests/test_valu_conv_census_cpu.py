"""The census table (valu_conv_census.py) against the text of csrc/basic_ops.hip, against the built library and against the
oracle, without a GPU: every kernel the four convolution entry points can launch and every instantiation of it the
library holds is a row's expected kernel, the two environment switches are the ones the table uses, every kernel has the
rows the census promises, and every row's data shows what the row needs it to show.

The preconditions.  A row under a rule other than the chain tests that rule only if the data tells it from the others:
the oracle's other rules must give other bits in at least half of the elements (measured: 0.53 in the worst row).  The
zero rows need both signs of zero in the oracle's output, the subnormal rows a subnormal value.

The zero-sign facts behind the zero rows, on x = -0 everywhere, w = 0.25, bias = -0, 3x3 'same' (asserted below):
clib.conv2d multiplies the zeros of its padded copy in, so under the chain the interior is -0 and the border
fmaf(+0, w, -0) = +0; under rule blocks the chain starts at +0 and everything is +0, as with F.conv2d; clib.dwconv2d
skips the taps outside the image and gives -0 everywhere, as depthwise F.conv2d does."""
import os
import re

import numpy as np
import pytest

import valu_conv_census as vc

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "learned-pmctf_amd")
SRC = os.path.join(PKG, "csrc", "basic_ops.hip")
LIB = os.path.join(PKG, "lib", "libpmctf_hip.so")            # built by conftest.py where it is missing
ENTRIES = ("pmctf_conv2d_smallcin_f32", "pmctf_conv3x3_cin1_dual_f32", "pmctf_conv2d_fewcout_f32", "pmctf_dwconv2d_nhwc_f32")
MACROS = ("PM_STRIP", "PM_SC", "PM_FC")


@pytest.fixture(scope="module")
def source():
    with open(SRC) as f:
        return f.read()


def entry_body(source, name):
    start = source.index(f'extern "C" int {name}(')
    return source[start:source.index("\n}\n", start)]


def _arguments(text, start):
    """the arguments of the call whose '(' is at text[start - 1], split at the commas outside brackets"""
    args, depth, at, i = [], 0, start, start
    while depth > 0 or text[i] != ")":
        if text[i] in "(<" and not (text[i] == "<" and text[i + 1] in "= "):
            depth += 1
        elif text[i] in ")>" and not (text[i] == ">" and text[i - 1] in "- "):
            depth -= 1
        elif text[i] == "," and depth == 0:
            args.append(text[at:i])
            at = i + 1
        i += 1
    return [a.strip() for a in args + [text[at:i]]]


def launched_expressions(source):
    """first argument of every PM_LAUNCH...( in the four entry points; inside PM_STRIP / PM_SC / PM_FC the macro's
    parameters are replaced by the arguments of each of its call sites"""
    found, forms = set(), set()
    for name in ENTRIES:
        body = entry_body(source, name)
        defines = {}                                           # macro -> (parameters, text of the definition)
        for m in re.finditer(r"#define (\w+)\(([^)]*)\)((?:.*\\\n)*.*)\n", body):
            defines[m.group(1)] = ([p.strip() for p in m.group(2).split(",")], m.group(3))
        assert set(defines) <= set(MACROS), sorted(defines)
        plain = body
        for macro, (params, text) in defines.items():
            plain = plain.replace(text, "")
            calls = [_arguments(plain, m.end()) for m in re.finditer(rf"(?<!#define ){macro}\(", plain)]
            calls = [c for c in calls if c != params]
            assert calls, macro
            for m in re.finditer(r"\bPM_LAUNCH(\w*)\(", text):
                forms.add(m.group(1))
                expr = _arguments(text, m.end())[0]
                for args in calls:
                    e = expr
                    for p, a in zip(params, args):
                        e = re.sub(rf"\b{p}\b", a, e)
                    found.add(vc_strip(e))
        for m in re.finditer(r"\bPM_LAUNCH(\w*)\(", plain):
            forms.add(m.group(1))
            found.add(vc_strip(_arguments(plain, m.end())[0]))
    assert forms == {"_NOTED"}, f"a launch of a convolution entry point that leaves no record: PM_LAUNCH{sorted(forms)}"
    return found


def vc_strip(expr):
    expr = " ".join(expr.split())
    return expr[1:-1].strip() if expr.startswith("(") and expr.endswith(")") else expr


def census_expressions():
    return {r[9] for r in vc.CENSUS}


def instantiated(library, names):
    """the instantiations of the kernel templates `names` whose mangled names the built library holds, as launch expressions"""
    with open(library, "rb") as f:
        data = f.read()
    found = set()
    for name in names:
        for args in set(re.findall(rb"_ZN12_GLOBAL__N_1%d%s((?:I(?:Li\d+E)+E)?)E" % (len(name), name.encode()), data)):
            nums = re.findall(rb"Li(\d+)E", args)
            found.add(name + ("<" + ", ".join(n.decode() for n in nums) + ">" if nums else ""))
    return found


def test_every_launched_kernel_is_a_rows_expected_kernel(source):
    in_source = launched_expressions(source)
    assert len(in_source) == 18, sorted(in_source)
    assert in_source == census_expressions(), (f"without a census row: {sorted(in_source - census_expressions())}; "
                                               f"not in the source: {sorted(census_expressions() - in_source)}")


def test_every_instantiation_in_the_library_has_a_row(source):
    names = {e.split("<")[0] for e in launched_expressions(source)}
    # every __global__ kernel of the file whose name says convolution is one of them: none is launched from elsewhere
    kernels = set(re.findall(r"__global__ (?:__launch_bounds__\(\d+\) )?void (\w*conv\w*)\(", source))
    assert kernels == names, sorted(kernels ^ names)
    built = instantiated(LIB, names)
    assert built == census_expressions(), (f"instantiated without a row: {sorted(built - census_expressions())}; "
                                           f"in the table, not in the library: {sorted(census_expressions() - built)}")


def test_environment_switches(source):
    bodies = "".join(entry_body(source, n) for n in ENTRIES)
    assert set(re.findall(r'getenv\("(\w+)"\)', bodies)) == set(vc.SWITCHES)
    assert {r[8] for r in vc.CENSUS} == {None, *vc.SWITCHES}
    # a switch that is off selects the kernel the row expects only through its own entry point
    assert {r[1] for r in vc.rows_for("PMCTF_FEWCOUT_LDS")} == {"fewcout"}
    assert {r[1] for r in vc.rows_for("PMCTF_DWCONV_COLUMN")} == {"dwconv"}


def test_thresholds_the_rows_sit_next_to(source):
    """the conditions the neighbour rows are written against, as the source words them: a reworded or moved threshold
    shows up here, and on the GPU as a wrong kernel name"""
    flat = " ".join(source.split())
    for text in ("KH == 3 && KW == 3 && stride == 1 && pad_h == 1 && pad_w == 1 && Cin <= 3 && Cout >= 32 && Cout <= 256 && (Cout & 3) == 0",
                 "if (!gemm && KH == KW && Cout <= 256 &&", "const bool gemm = rule == PMCTF_SUM_GEMM || rule == PMCTF_SUM_GEMV_3X3;",
                 "if (K == 3 && (C & 3) == 0) {", "if (column && threads_col >= 256L * 1024) {",
                 "const long threads_col = (long)N * ((H + 7) / 8) * ((W + 3) / 4) * (C / 4);"):
        assert text in flat, text
    threads = lambda N, C, H, W: N * ((H + 7) // 8) * ((W + 3) // 4) * (C // 4)
    assert threads(*vc.COLUMN_PLANE) >= 256 * 1024 > threads(*vc.BELOW_COLUMN_PLANE)
    N, C, H, W = vc.COLUMN_PLANE
    assert H % 8 and W % 4 and vc.BELOW_COLUMN_PLANE == (N, C, H, W - 4)


def test_rows_are_well_formed():
    ids = [r[0] for r in vc.CENSUS]
    assert len(set(ids)) == len(ids) == vc.N_ROWS
    big = 0
    for rid, entry, geometry, rule, act, slope, nres, bias, env, expected, options in vc.CENSUS:
        N, Cin, H, W, Cout, KH, KW, S, ph, pw = geometry
        assert entry in vc.RULES and (rule in vc.RULES[entry] or (entry == "dwconv" and rule == 0)), rid
        assert act in range(5) and nres in (0, 1, 2) and (nres == 0 or entry in vc.HAS_RESIDUALS), rid
        assert set(options) <= {"data", "seed", "y2", "c_entry"} and min(vc.out_hw(geometry)) > 0, rid
        assert rule != 3 or (Cin == 1 and KH == KW == 3), rid
        assert rule not in vc.GENERIC_ONLY_RULES or expected == vc.GENERIC, rid
        assert options.get("y2", True) or options.get("c_entry"), rid
        if N * H * W * Cout > 1 << 20:                          # larger than tiny only for the column kernel's threshold
            assert entry == "dwconv" and geometry[:4] in (vc.COLUMN_PLANE, vc.BELOW_COLUMN_PLANE), rid
            big += 1
    assert big == 6


def test_every_kernel_has_the_rows_the_census_promises():
    """per kernel expression: a row with two residuals (where the entry has residuals), a row without bias, a zero row
    under every rule the kernel accepts and a subnormal row, and ordinary rows under every rule it accepts"""
    for expr in sorted(census_expressions()):
        rows = [r for r in vc.CENSUS if r[9] == expr]
        entry = rows[0][1]
        assert {r[1] for r in rows} == {entry}
        rules = tuple(k for k in vc.RULES[entry] if expr == vc.GENERIC or k not in vc.GENERIC_ONLY_RULES) or (0,)
        kind = lambda r: r[10].get("data", "normal")
        if entry in vc.HAS_RESIDUALS:
            assert any(r[6] == 2 for r in rows), f"{expr}: no row with two residuals"
        assert any(not r[7] for r in rows), f"{expr}: no row without bias"
        assert {r[3] for r in rows if kind(r) == "zeros"} == set(rules), f"{expr}: zero rows under {rules}"
        assert any(kind(r) == "subnormal" for r in rows), f"{expr}: no subnormal row"
        assert {r[3] for r in rows if kind(r) not in ("zeros", "subnormal")} == set(rules), f"{expr}: rows under {rules}"
        assert len({(r[4], r[6]) for r in rows}) > 1 or entry == "dwconv", f"{expr}: one epilogue only"
    for r in vc.CENSUS:                                        # a zero row's plane has a border and an interior
        if r[10].get("data") == "zeros":
            assert r[2][2] >= 3 and r[2][3] > vc.zero_patches(max(r[2][5], r[2][6]))[2][1], r[0]
            assert max(r[2][8], r[2][9]) > 0, r[0]


def test_the_families_of_the_census():
    """the shapes the census was asked to hold, by name"""
    ids = {r[0] for r in vc.CENSUS}
    for cout in (32, 36, 112, 132, 256):
        assert {f"strip_cin{c}_cout{cout}" for c in (1, 2, 3)} <= ids
    dual = [r for r in vc.CENSUS if r[1] == "cin1_dual" and r[10].get("data") not in ("zeros", "subnormal")]
    assert {(r[3], r[4]) for r in dual} >= {(rule, act) for rule in (0, 1) for act in range(5)}
    assert any(r[10].get("y2") is False for r in dual) and {r[2][0] for r in dual} >= {1, 2, 3}
    assert {(r[2][2], r[2][3]) for r in dual} >= {(1, 1)} and any(r[2][2] == 1 < r[2][3] for r in dual)
    assert any(r[2][3] == 1 < r[2][2] for r in dual)
    for k, ci, co in vc.FEWCOUT:
        for kern, env in ((vc.LDS, None), (vc.PIX, "PMCTF_FEWCOUT_LDS")):
            rows = [r for r in vc.CENSUS if r[9] == kern % (k, ci, co) and r[10].get("data", "normal") == "normal" and r[7]]
            assert {r[8] for r in rows} == {env}
            assert {(r[2][2], r[2][3]) for r in rows} >= {(1, 1), (8, 32), (9, 33), (7, 31)}
            assert {(r[3], r[4], r[6]) for r in rows} >= {(rule, a, n) for rule in (0, 1) for a, n in ((2, 2), (1, 1), (0, 0))}
    assert {"few7x7_16to2_lds_rule0_3x3", "few7x7_16to2_pix_rule1_3x3"} <= ids
    gen = [r for r in vc.CENSUS if r[9] == vc.GENERIC]
    assert {(r[2][5], r[2][6]) for r in gen} >= {(3, 3), (5, 5), (7, 7), (1, 1), (3, 1), (1, 3)}
    assert any(r[2][4] > 256 for r in gen) and {r[2][1] for r in gen if r[3] == 2} >= {2, 3, 4}
    assert {(r[2][4], r[2][7], r[2][8]) for r in gen if r[3] == 3} >= {(1, 1, 1), (16, 1, 1), (1, 2, 0), (16, 2, 0)}
    reg = [r for r in vc.CENSUS if r[9].startswith("conv_smallcin_reg_kernel")]
    assert {r[2][4] for r in reg} >= {1, 3, 5, 17, 200, 256, 28, 30} and {r[2][7] for r in reg} >= {1, 2, 3}
    assert {r[2][8] for r in reg if r[9] == vc.REG % (1, 2)} >= {0, 1}
    dw = [r for r in vc.CENSUS if r[9] == vc.DW]
    assert {r[2][5] for r in dw} >= {1, 3, 5, 7} and {r[2][1] for r in dw if r[2][5] == 3} >= {3, 6}


def test_parse_launch():
    assert vc.parse_launch("conv_smallcin_reg_kernel<3, 2> grid 140") == ("conv_smallcin_reg_kernel<3, 2>", 140)
    assert vc.parse_launch("dwconv_kernel grid 1") == ("dwconv_kernel", 1)
    for bad in ("", "dwconv_kernel", "dwconv_kernel grid x", " grid 3"):
        with pytest.raises(ValueError):
            vc.parse_launch(bad)


def test_case_data_follows_the_seed():
    a, b = vc.case_data(vc.row("few3x3_16to1_lds_rule1_9x33")), vc.case_data(vc.row("few3x3_16to1_pix_rule1_9x33"))
    assert all(np.array_equal(a[k], b[k]) for k in ("x", "w", "b")) and len(a["res"]) == 2
    c = vc.case_data(vc.row("few3x3_16to1_lds_rule0_9x33"))
    assert a["x"].shape == c["x"].shape == (2, 16, 9, 33) and (a["x"] != c["x"]).any()
    assert vc.case_data(vc.row("nobias_dwconv"))["b"] is None
    z = vc.case_data(vc.row("zeros_conv3x3_cin1_pix16_rule0"))
    u = vc.bits(z["x"])
    assert (u[..., 0:4] == 0x80000000).all() and (u[..., 4:8] == 0).all() and (u[..., 8:12] == 0x80000001).all()
    assert (vc.bits(z["b"]) == 0x80000000).all() and (z["w"] >= 0.25).all() and (z["w"] < 0.375).all()


@pytest.mark.parametrize("rid", [r[0] for r in vc.CENSUS if r[2][:4] not in (vc.COLUMN_PLANE, vc.BELOW_COLUMN_PLANE)])
def test_precondition_of_the_row(rid):
    outs, ok, text = vc.reference(vc.row(rid))
    assert ok, text


def test_preconditions_of_the_large_rows():
    for r in vc.CENSUS:
        if r[2][:4] in (vc.COLUMN_PLANE, vc.BELOW_COLUMN_PLANE) and r[10].get("data"):
            outs, ok, text = vc.reference(r)
            assert ok, text


def test_zero_signs_of_the_oracle_and_of_aten():
    """the facts of the module docstring: which zeros the oracle's two convolutions and F.conv2d give on x = -0, w = 0.25,
    bias = -0.  A skipping dense kernel (-0 on the border under the chain) and a multiplying depthwise kernel (+0 on the
    border) are both visible against them."""
    import torch
    import torch.nn.functional as F
    from pmctf_oracle import clib
    NEG, POS = 0x80000000, 0
    x = np.full((1, 2, 5, 7), -0.0, np.float32)
    w = np.full((3, 2, 3, 3), 0.25, np.float32)
    b = np.full(3, -0.0, np.float32)
    interior = np.zeros((5, 7), bool)
    interior[1:-1, 1:-1] = True
    chain = vc.bits(clib.conv2d(x, w, b, 1, (1, 1), 0))
    assert (chain[..., interior] == NEG).all() and (chain[..., ~interior] == POS).all()
    assert (vc.bits(clib.conv2d(x, w, b, 1, (1, 1), 1)) == POS).all()
    assert (vc.bits(clib.conv2d(x[:, :1], w[:, :1], b, 1, (1, 1), 2)) == POS).all()
    gemv = vc.bits(clib.conv2d(x[:, :1], w[:, :1], b, 1, (1, 1), 3))
    assert (gemv[..., interior] == NEG).all() and (gemv[..., ~interior] == POS).all()
    assert (vc.bits(F.conv2d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), padding=1).numpy()) == POS).all()
    wd = np.full((2, 1, 3, 3), 0.25, np.float32)
    assert (vc.bits(clib.dwconv2d(x, wd, b[:2])) == NEG).all()
    assert (vc.bits(F.conv2d(torch.from_numpy(x), torch.from_numpy(wd), torch.from_numpy(b[:2]), padding=1, groups=2).numpy())
            == NEG).all()
    # the patch of -2^-149 is what gives -0 where the chain starts at +0: each product rounds to -0.  On the border the
    # sign is that of the last tap: +0 where a zero of the padding comes after the image's taps (the bottom and right edge)
    tiny = np.full((1, 1, 5, 7), np.array(0x80000001, np.uint32).view(np.float32), np.float32)
    blocks = vc.bits(clib.conv2d(tiny, w[:, :1], b, 1, (1, 1), 1))
    assert (blocks[..., interior] == NEG).all() and (blocks[..., -1, :] == POS).all() and (blocks[..., :, -1] == POS).all()
