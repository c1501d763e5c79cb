"""Reduced-resolution coding without a GPU: the product's resampling tables against tests/scale_restatement.py, the
restatement against torch's antialiased bicubic, the display_format.json header (round trip and every refusal), the new
entry points of csrc/picture_scale.hip (declared, bound, refusing bad arguments before any launch) and the command line."""
import ctypes as C
import importlib.util
import inspect
import json
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import scale_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (h_in, w_in, h_out, w_out): 2:1, non-integer down, up, down, 3:1, beyond-limit shapes of the filter alone, identity
SIZES = [(36, 64, 18, 32), (36, 64, 24, 44), (34, 50, 100, 132), (100, 132, 34, 50), (54, 96, 18, 32), (64, 64, 10, 6),
         (6, 10, 64, 64)]
AXES = sorted({(a, b) for hi, wi, ho, wo in SIZES + [(18, 34, 18, 34), (64, 64, 16, 16), (6, 10, 24, 40)]
               for a, b in ((hi, ho), (wi, wo), (hi // 2, ho // 2), (wi // 2, wo // 2))})


# ---------------------------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("n_in,n_out", AXES)
def test_tables_equal_the_restatement(n_in, n_out):
    import pmctf_scale
    for phase in (Fraction(0), sr.left_phase(n_in, n_out)):
        start, coef, taps = pmctf_scale.axis_table(n_in, n_out, phase)
        want_start, want_coef, want_taps = sr.tables(n_in, n_out, phase)
        assert taps == want_taps and list(start) == want_start.tolist()
        assert [list(r) for r in coef] == want_coef.tolist()
        assert all(sum(r) == 16384 for r in coef), "every row sums to 16384"
        if 4 * n_out >= n_in and n_out <= 4 * n_in:
            assert 1 <= taps <= 20, "the kernel's longest row, within the ratio limits"
        assert all(-32768 <= c <= 32767 for r in coef for c in r), "int16 coefficients"
        assert all(0 <= s < n_in for s in start) and list(start) == sorted(start), "start inside the axis, never decreasing"
        for s, r in zip(start, coef):
            assert all(c == 0 for k, c in enumerate(r) if s + k >= n_in), "taps past the edge are zero"
    assert pmctf_scale.chroma_phase(n_in, n_out, "left") == sr.left_phase(n_in, n_out)
    assert pmctf_scale.chroma_phase(n_in, n_out, "center") == 0


@pytest.mark.parametrize("n", (2, 3, 5, 18, 100))
def test_identity_is_a_single_tap(n):
    import pmctf_scale
    start, coef, _ = pmctf_scale.axis_table(n, n)
    for i, (s, r) in enumerate(zip(start, coef)):
        assert [c for c in r if c] == [16384] and s + list(r).index(16384) == i
    x = np.random.default_rng(n).integers(0, 256, (n, n + 2), dtype=np.uint8)
    assert np.array_equal(sr.resize_plane(x, n, n + 2, 8), x)


def test_longest_rows_at_the_limits():
    """the kernel holds 20 taps and the 80 source rows of a 16-row tile: 4:1 needs 17 taps and 15 * 4 + 1 + 17 rows"""
    import pmctf_scale
    for n_out in (2, 16, 250, 1000):
        start, _, taps = pmctf_scale.axis_table(4 * n_out, n_out)
        assert taps <= 17
        assert all(start[min(i + 15, n_out - 1)] + taps - start[i] <= 80 for i in range(0, n_out, 16))
    assert pmctf_scale.axis_table(10, 40)[2] <= 5
    assert pmctf_scale.axis_table(540, 1080, Fraction(-1, 8))[2] <= 5


def test_a_constant_plane_stays_constant():
    for b, v in ((8, 255), (8, 1), (10, 1023), (16, 65535)):
        x = np.full((20, 34), v, np.uint8 if b == 8 else np.uint16)
        for ho, wo in ((10, 18), (50, 40), (20, 34), (6, 130)):
            assert (sr.resize_plane(x, ho, wo, b) == v).all()
            assert (sr.resize_plane(x, ho, wo, b, phase_x=sr.left_phase(34, wo)) == v).all()


# ------------------------------------------------------------------------------------------ the restatement against torch
def _plane(h, w, b, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << b, (h, w), dtype=np.uint16)
    sat = rng.random((h, w))
    x[sat < 0.1] = 0
    x[sat > 0.9] = (1 << b) - 1
    return x


def _bound(h_in, w_in, h_out, w_out, b):
    t_h, t_v = sr.tables(w_in, w_out)[2], sr.tables(h_in, h_out)[2]
    return 0.5 + 1.5 * ((1 << b) - 1) * (t_h + t_v) / 16384


def _torch_reference(x, h_out, w_out, b):
    import torch.nn.functional as F
    ref = F.interpolate(torch.from_numpy(x.astype(np.float64))[None, None], size=(h_out, w_out), mode="bicubic",
                        antialias=True, align_corners=False)[0, 0].numpy()
    return np.clip(ref, 0.0, float((1 << b) - 1))


@pytest.mark.parametrize("b", (8, 10, 16))
@pytest.mark.parametrize("h_in,w_in,h_out,w_out", SIZES)
def test_restatement_against_torch_bicubic_antialias(h_in, w_in, h_out, w_out, b):
    """|out - torch| <= 0.5 + 1.5 max (T_h + T_v) / 16384 with torch's float64 result unrounded (clamped to 0..max as the
    integer result is: a clamp moves two numbers no further apart).

    Where the bound comes from.  A coefficient q / 16384 differs from its real weight by at most 1/2 / 16384, except the
    one that absorbs the rest of the row: the rest is at most T / 2 units, so a row's coefficients are off by at most
    (T/2 + T/2) / 16384 = T / 16384 in absolute sum.  Horizontal pass: the intermediate differs from the real one by at
    most max T_h / 16384 (plus 2^-9 from its 8 fractional bits).  The vertical pass multiplies that by the absolute sum of
    its real weights, below 1.5 for every clipped and renormalised Catmull-Rom window here, and adds its own coefficient
    error T_v / 16384 on intermediates of magnitude below 1.5 max.  The final rounding adds 1/2.  The 2^-9 term (times 1.5)
    is below the slack of 1.5 against the true absolute sums (1.25 in the interior)."""
    x = _plane(h_in, w_in, b, seed=h_in * 7 + w_out + b)
    got = sr.resize_plane(x, h_out, w_out, b).astype(np.float64)
    ref = _torch_reference(x, h_out, w_out, b)
    worst, bound = float(np.abs(got - ref).max()), _bound(h_in, w_in, h_out, w_out, b)
    print(f"{h_in}x{w_in}->{h_out}x{w_out} b={b}: max |out - torch| = {worst:.4f}, bound {bound:.4f}")
    assert worst <= bound
    # the float form of the same weights is torch's filter to rounding error: the definition is the same one
    real = np.clip(sr.resize_plane_real(x, h_out, w_out), 0.0, float((1 << b) - 1))
    assert float(np.abs(real - ref).max()) <= 1e-9 * (1 << b)


def test_a_slip_of_one_sample_breaks_the_bound():
    """the bound is tight enough to see a window or phase that is off by one: at 8 bits it is about 1.1"""
    h_in, w_in, h_out, w_out, b = 36, 64, 24, 44, 8
    x = _plane(h_in, w_in, b, seed=3)
    ref = _torch_reference(x, h_out, w_out, b)
    bound = _bound(h_in, w_in, h_out, w_out, b)
    assert bound < 1.2
    for slipped in (np.roll(x, 1, axis=1), np.roll(x, 1, axis=0)):
        assert float(np.abs(sr.resize_plane(slipped, h_out, w_out, b).astype(np.float64) - ref).max()) > bound
    half = sr.resize_plane(x, h_out, w_out, b, phase_x=Fraction(1, 2)).astype(np.float64)
    assert float(np.abs(half - ref).max()) > bound


def test_packed_picture_planes_and_siting():
    h, w, ho, wo, b = 20, 36, 10, 24, 8
    frame = np.random.default_rng(1).integers(0, 256, h * w * 3 // 2, dtype=np.uint8)
    y, cb, cr = sr.split(frame, h, w)
    for loc, px in (("center", 0), ("left", Fraction(36, 24) / 4 - Fraction(1, 4))):
        out = sr.resize_yuv420(frame, h, w, ho, wo, b, loc)
        oy, ocb, ocr = sr.split(out, ho, wo)
        assert np.array_equal(oy, sr.resize_plane(y, ho, wo, b))
        assert np.array_equal(ocb, sr.resize_plane(cb, ho // 2, wo // 2, b, phase_x=px))
        assert np.array_equal(ocr, sr.resize_plane(cr, ho // 2, wo // 2, b, phase_x=px))
    assert not np.array_equal(sr.resize_yuv420(frame, h, w, ho, wo, b, "left"), sr.resize_yuv420(frame, h, w, ho, wo, b))


# ------------------------------------------------------------------------------------------------------------ the header
def test_display_format_round_trip(tmp_path):
    import pmctf_scale
    assert pmctf_scale.read_display_format(str(tmp_path)) is None
    path = pmctf_scale.write_display_format(str(tmp_path), 132, 100, "left")
    assert os.path.basename(path) == "display_format.json"
    record = json.load(open(path))
    assert record == {"format_version": 1, "width": 132, "height": 100, "filter": "catmull-rom-aa/14", "chroma_loc": "left"}
    assert pmctf_scale.read_display_format(str(tmp_path)) == record
    assert pmctf_scale.read_display_format(str(tmp_path), 66, 50) == record
    assert pmctf_scale.read_display_format(str(tmp_path), 528, 400) == record
    assert pmctf_scale.read_display_format(str(tmp_path), 34, 26) == record


GOOD = {"format_version": 1, "width": 132, "height": 100, "filter": "catmull-rom-aa/14", "chroma_loc": "center"}


@pytest.mark.parametrize("change,coded", [
    ({"format_version": 2}, None), ({"format_version": "1"}, None), ({"format_version": None}, None),
    ({"filter": "lanczos3"}, None), ({"filter": 14}, None), ({"chroma_loc": "top"}, None), ({"chroma_loc": None}, None),
    ({"width": 131}, None), ({"height": 0}, None), ({"width": -2}, None), ({"width": 132.0}, None), ({"height": "100"}, None),
    ({"width": True}, None), ({"height": 16386}, None), ({"extra": 1}, None), ({"width": None}, None),
    ({}, (32, 50)), ({}, (132, 24)), ({}, (530, 100)), ({}, (132, 402)), ({}, (66, 51)),
])
def test_display_format_refusals(tmp_path, change, coded):
    import pmctf_scale
    record = dict(GOOD, **change)
    if change.get("width", 0) is None:
        del record["width"]
    with open(tmp_path / "display_format.json", "w") as f:
        json.dump(record, f)
    with pytest.raises(ValueError, match="display_format.json"):
        pmctf_scale.read_display_format(str(tmp_path), *(coded or ()))


def test_display_format_malformed_files_and_bad_writes(tmp_path):
    import pmctf_scale
    for text in ("", "{", "[1, 2]", "3", "\"catmull\""):
        (tmp_path / "display_format.json").write_text(text)
        with pytest.raises(ValueError, match="display_format.json"):
            pmctf_scale.read_display_format(str(tmp_path))
    os.remove(tmp_path / "display_format.json")
    for args in ((131, 100, "center"), (132, 100, "top"), (132, 0, "left"), (132.0, 100, "center")):
        with pytest.raises(ValueError):
            pmctf_scale.write_display_format(str(tmp_path), *args)
    assert not os.path.exists(tmp_path / "display_format.json")


def test_size_checks():
    import pmctf_scale
    pmctf_scale.check_sizes(132, 100, 66, 50)
    pmctf_scale.check_sizes(64, 64, 16, 256)
    for args in ((132, 100, 65, 50), (132, 100, 66, 24), (132, 100, 530, 100), (16386, 100, 8192, 100), (132, 100, 0, 50),
                 (132, 100, 66.0, 50), (131, 100, 66, 50)):
        with pytest.raises(ValueError):
            pmctf_scale.check_sizes(*args)
    assert pmctf_scale.parse_size("66x50") == (66, 50) and pmctf_scale.parse_size("1920X1080") == (1920, 1080)
    for text in ("66", "66x", "x50", "66x50x3", "65x50", "0x50", "-66x50", "6.6x50", "axb"):
        with pytest.raises(ValueError):
            pmctf_scale.parse_size(text)


# ------------------------------------------------------------------------------------------------- the public interface
def test_entry_points_and_keywords():
    import pmctf_gop
    import pmctf_layers
    import pmctf_rate
    import pmctf_scale
    import pmctf_seq
    for fn, base in ((pmctf_scale.encode_sequence, pmctf_gop.encode_sequence),
                     (pmctf_scale.encode_sequence_gops, pmctf_seq.encode_sequence_gops),
                     (pmctf_scale.encode_sequence_rate, pmctf_rate.encode_sequence_rate)):
        p = inspect.signature(fn).parameters
        assert p["coded_size"].default is None and p["chroma_loc"].default == "center"
        lead = [k for k, v in p.items() if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
        assert lead == list(inspect.signature(base).parameters)[:len(lead)] and lead[-1] == "device"
    for fn, base in ((pmctf_scale.decode_sequence_checked, pmctf_gop.decode_sequence_checked),
                     (pmctf_scale.decode_sequence_layer, pmctf_layers.decode_sequence_layer)):
        p = inspect.signature(fn).parameters
        assert list(p) == list(inspect.signature(base).parameters) + ["coded_size_output"]
        assert p["coded_size_output"].default is False
    with pytest.raises(ValueError, match="chroma_loc"):
        pmctf_scale.encode_sequence(None, "x.yuv", 132, 100, 8, 4, 3, "bins", "cpu", chroma_loc="top")
    with pytest.raises(RuntimeError, match="GPU"):
        pmctf_scale.encode_sequence(None, "x.yuv", 132, 100, 8, 4, 3, "bins", "cpu", coded_size=(66, 50))


def test_symbols_are_declared_bound_and_refuse_bad_arguments():
    from pMCTF.hip import lib, ops
    header = open(os.path.join(ROOT, "include", "pmctf_hip.h")).read()
    L = C.CDLL(lib.HIP_SO)
    for s in ("pmctf_resize_yuv420_u8", "pmctf_resize_yuv420_u16"):
        assert f"int {s}(" in header and s in lib.exported_symbols() and hasattr(L, s)
    assert list(inspect.signature(ops.resize_yuv420).parameters) == ["frame", "h_in", "w_in", "h_out", "w_out", "tables", "taps",
                                                                    "bitdepth"]
    # refused before any launch (and so without a GPU): the pointers are never looked at
    H = lib.hip()
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)
    taps = (C.c_int * 4)(4, 4, 4, 4)
    ok = (p, p, 18, 34, 18, 34, p, p, p, p, taps)
    for fn, depth in ((H.pmctf_resize_yuv420_u8, 8), (H.pmctf_resize_yuv420_u16, 10)):
        for k in (0, 1, 6, 7, 8, 9, 10):
            bad = list(ok)
            bad[k] = None
            assert fn(*bad, depth, None) == -1, k
        for sizes in ((17, 34, 18, 34), (18, 33, 18, 34), (18, 34, 18, 35), (18, 34, 0, 34), (18, 34, 4, 34), (18, 34, 74, 34),
                      (18, 34, 18, 8), (18, 34, 18, 138), (16386, 34, 16386, 34), (-18, 34, 18, 34)):
            assert fn(p, p, *sizes, p, p, p, p, taps, depth, None) == -1, sizes
        for t in ((0, 4, 4, 4), (4, 21, 4, 4), (4, 4, -1, 4), (4, 4, 4, 100)):
            assert fn(*ok[:10], (C.c_int * 4)(*t), depth, None) == -1, t
        odd = C.c_void_p(p.value + 2)
        assert fn(p, p, 18, 34, 18, 34, odd, p, p, p, taps, depth, None) == -1
    for depth in (0, 7, 9, 16):
        assert H.pmctf_resize_yuv420_u8(*ok, depth, None) == -1
    for depth in (8, 17, 0, -1):
        assert H.pmctf_resize_yuv420_u16(*ok, depth, None) == -1
    assert H.pmctf_resize_yuv420_u16(C.c_void_p(p.value + 1), p, *ok[2:], 10, None) == -1
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.resize_yuv420(torch.zeros(18 * 34 * 3 // 2, dtype=torch.uint8), 18, 34, 18, 34, [None] * 4, [4] * 4)
    with pytest.raises(ValueError):
        ops.resize_yuv420(torch.zeros(18 * 34 * 3 // 2, dtype=torch.uint8), 18, 34, 4, 34, [None] * 4, [4] * 4)


# ------------------------------------------------------------------------------------------------------ the command line
def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("extra,message", [
    (["--coded-size", "65x50"], "--coded-size"), (["--coded-size", "66"], "--coded-size"),
    (["--coded-size", "66x50x2"], "--coded-size"), (["--chroma-loc", "left"], "only with --coded-size"),
    (["--coded-size", "66x50", "--chroma-loc", "top"], "invalid choice"),
    (["--coded-size", "32x50"], "factor of 4"), (["--coded-size", "66x402"], "factor of 4"),
])
def test_encode_cli_refuses_bad_sizes(tmp_path, capsys, extra, message):
    src = tmp_path / "src.yuv"
    src.write_bytes(bytes(132 * 100 * 3 // 2 * 4))
    with pytest.raises(SystemExit) as e:
        _tool("encode_sequence").main(["--synth-seed", "0", "--width", "132", "--height", "100", "--gop", "4", *extra,
                                       str(src), str(tmp_path / "bins")])
    assert e.value.code == 2 and message in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "bins")


def test_decode_cli_has_the_option():
    text = open(os.path.join(ROOT, "tools", "decode_sequence.py")).read()
    assert "--coded-size-output" in text and "coded_size_output=a.coded_size_output" in text
