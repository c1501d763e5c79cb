"""Chroma formats and Y4M without a GPU: the product's phases and tables against tests/chroma_restatement.py,
the restatement against torch's antialiased bicubic, the Y4M header and reader (every accepted tag, every refusal),
source_format.json (round trip and every refusal), the new entry points of csrc/picture_chroma.hip (declared, bound,
refusing bad arguments before any launch), the keywords of pmctf_chroma's entry points and the command line."""
import ctypes as C
import importlib.util
import inspect
import json
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import chroma_restatement as cr
import scale_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ("420", "422", "444")
PAIRS = [(a, b) for a in FORMATS for b in FORMATS]
SIZES = [(2, 2), (6, 10), (100, 132)]                                  # (h, w)
ACCEPTED = {"420jpeg": ("420", 8, "center"), "420mpeg2": ("420", 8, "left"), "420": ("420", 8, "center"),
            "422": ("422", 8, "left"), "444": ("444", 8, "center"),
            **{f"{f}p{b}": (f, b, "left" if f == "422" else "center") for f in FORMATS for b in range(9, 17)}}


# ------------------------------------------------------------------------------------------------------ the arithmetic
def test_the_phase_formula_and_its_two_values():
    import pmctf_chroma
    import pmctf_scale
    assert pmctf_chroma.format_phase(1, 2, "left") == Fraction(-1, 2) == cr.phase(1, 2, "left")
    assert pmctf_chroma.format_phase(2, 1, "left") == Fraction(1, 4) == cr.phase(2, 1, "left")
    for s_in in (1, 2):
        for s_out in (1, 2):
            assert pmctf_chroma.format_phase(s_in, s_out, "center") == 0 == cr.phase(s_in, s_out, "center")
            assert pmctf_chroma.format_phase(s_in, s_out, "left") == cr.phase(s_in, s_out, "left")
        assert pmctf_chroma.format_phase(s_in, s_in, "left") == 0
    for bad in ((1, 2, "top"), (3, 1, "left"), (1, 4, "center")):
        with pytest.raises(ValueError):
            pmctf_chroma.format_phase(*bad)
    # the size-change phase next to it keeps its pinned values
    assert pmctf_scale.chroma_phase(66, 33, "left") == Fraction(1, 4) and pmctf_scale.chroma_phase(66, 33, "center") == 0


@pytest.mark.parametrize("fmt_in,fmt_out", PAIRS)
def test_tables_equal_the_restatement(fmt_in, fmt_out):
    import pmctf_chroma
    for h, w in SIZES:
        for loc in ("center", "left"):
            for (start, coef, taps), (want_start, want_coef, want_taps), n_in in zip(
                    pmctf_chroma.chroma_tables(w, h, fmt_in, fmt_out, loc), cr.axis_tables(h, w, fmt_in, fmt_out, loc),
                    (w // cr.SUB[fmt_in][0], h // cr.SUB[fmt_in][1])):
                assert all(sum(r) == 16384 for r in coef), "every row sums to 16384"
                assert 1 <= taps <= 17 and all(-32768 <= c <= 32767 for r in coef for c in r)
                assert all(0 <= s < n_in for s in start) and list(start) == sorted(start)
                if len(start) == n_in:                              # the axis keeps its length: the single-tap table, which
                    assert taps == 1 and list(start) == list(range(n_in))   # is the restatement's row without its zeros
                    assert [[c for c in r if c] for r in want_coef.tolist()] == [[16384]] * n_in
                    assert [s + list(r).index(16384) for s, r in zip(want_start.tolist(), want_coef.tolist())] == list(start)
                else:
                    assert taps == want_taps and list(start) == want_start.tolist()
                    assert [list(r) for r in coef] == want_coef.tolist()


def test_the_tables_the_issue_names():
    import pmctf_chroma
    (start, coef, taps), _ = pmctf_chroma.chroma_tables(132, 100, "444", "420", "left")
    assert list(coef[20][:7]) == [-512, 0, 4608, 8192, 4608, 0, -512] and not any(coef[20][7:]) and taps <= 17
    (start, coef, taps), _ = pmctf_chroma.chroma_tables(132, 100, "420", "444", "left")
    assert taps == 4 and max(max(r) for r in coef) == 18432
    assert list(coef[1][:3]) == [8674, 8674, -964]
    for i in range(0, 132, 2):                                           # even outputs are exact copies of input i / 2
        assert [c for c in coef[i] if c] == [16384] and start[i] + list(coef[i]).index(16384) == i // 2
    # interior rows of the down table are symmetric
    (start, coef, _), _ = pmctf_chroma.chroma_tables(132, 100, "444", "422", "left")
    for i in range(4, 60):
        row = list(coef[i][:7])
        assert row == row[::-1]


@pytest.mark.parametrize("b", (8, 10, 16))
def test_a_constant_plane_converts_to_itself(b):
    top = (1 << b) - 1
    dt = np.uint8 if b == 8 else np.uint16
    for v in (top, 1, top // 2):
        for fmt_in, fmt_out in PAIRS:
            for loc in ("center", "left"):
                frame = np.full(cr.samples(12, 20, fmt_in), v, dt)
                out = cr.convert(frame, 12, 20, fmt_in, fmt_out, b, loc)
                assert out.shape == (cr.samples(12, 20, fmt_out),) and (out == v).all()


def test_the_same_format_and_luma_are_copies():
    rng = np.random.default_rng(0)
    for fmt in FORMATS:
        frame = rng.integers(0, 256, cr.samples(10, 14, fmt), dtype=np.uint8)
        for loc in ("center", "left"):
            assert np.array_equal(cr.convert(frame, 10, 14, fmt, fmt, 8, loc), frame)
    frame = rng.integers(0, 1024, cr.samples(10, 14, "444"), dtype=np.uint16)
    assert np.array_equal(cr.convert(frame, 10, 14, "444", "420", 10)[:140], frame[:140])
    # 4:2:2 -> 4:2:0 leaves the columns alone: each column is the vertical 2:1 filter of the source column
    frame = rng.integers(0, 256, cr.samples(10, 14, "422"), dtype=np.uint8)
    cb = cr.split(frame, 10, 14, "422")[1]
    got = cr.split(cr.convert(frame, 10, 14, "422", "420", 8, "left"), 10, 14, "420")[1]
    assert np.array_equal(got, sr.resize_plane(cb, 5, 7, 8))


def _plane(h, w, b, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << b, (h, w), dtype=np.uint16)
    sat = rng.random((h, w))
    x[sat < 0.1] = 0
    x[sat > 0.9] = (1 << b) - 1
    return x


@pytest.mark.parametrize("b", (8, 10, 16))
@pytest.mark.parametrize("fmt_in,fmt_out", [p for p in PAIRS if p[0] != p[1]])
def test_restatement_against_torch_bicubic_antialias(fmt_in, fmt_out, b):
    """centre siting (torch has no phase): every chroma plane within DESIGN 5l's derived bound
    0.5 + 1.5 max (T_h + T_v) / 16384 of torch's float64 interpolate(bicubic, antialias=True), clamped as the integers are.
    T counts the coefficients of a row that carry a rounding error: an axis that keeps its length has the exact row
    (.., 0, 16384, 0, ..) and contributes T = 0, which is tighter than the length of its table."""
    import torch.nn.functional as F
    h, w = 36, 52
    frame = np.concatenate([_plane(r, c, b, seed=r + c + b + k).reshape(-1)
                            for k, (r, c) in enumerate(cr.plane_shapes(h, w, fmt_in))])
    frame = frame.astype(np.uint8 if b == 8 else np.uint16)
    out = cr.convert(frame, h, w, fmt_in, fmt_out, b, "center")
    (_, _, t_h), (_, _, t_v) = cr.axis_tables(h, w, fmt_in, fmt_out, "center")
    (sxi, syi), (sxo, syo) = cr.SUB[fmt_in], cr.SUB[fmt_out]
    t_h, t_v = (0 if sxi == sxo else t_h), (0 if syi == syo else t_v)
    bound = 0.5 + 1.5 * ((1 << b) - 1) * (t_h + t_v) / 16384
    for src, got in list(zip(cr.split(frame, h, w, fmt_in), cr.split(out, h, w, fmt_out)))[1:]:
        ref = F.interpolate(torch.from_numpy(src.astype(np.float64))[None, None], size=got.shape, mode="bicubic",
                            antialias=True, align_corners=False)[0, 0].numpy()
        worst = float(np.abs(got.astype(np.float64) - np.clip(ref, 0.0, float((1 << b) - 1))).max())
        print(f"{fmt_in}->{fmt_out} b={b}: max |out - torch| = {worst:.4f}, bound {bound:.4f}")
        assert worst <= bound


def test_left_siting_properties():
    """what torch cannot check: up-sampling by 2 with phase +1/4 copies input j to output 2 j exactly, and an interior row of
    the down filter at phase -1/2 is symmetric about output i's own position, input 2 i"""
    rng = np.random.default_rng(4)
    h, w, b = 12, 40, 10
    frame = rng.integers(0, 1 << b, cr.samples(h, w, "422"), dtype=np.uint16)
    up = cr.convert(frame, h, w, "422", "444", b, "left")              # 4:2:2 -> 4:4:4 enlarges along x alone
    for p422, p444 in list(zip(cr.split(frame, h, w, "422"), cr.split(up, h, w, "444")))[1:]:
        assert np.array_equal(p444[:, 0::2], p422)
    frame = rng.integers(0, 1 << b, cr.samples(h, w, "420"), dtype=np.uint16)
    up = cr.convert(frame, h, w, "420", "444", b, "left")              # and so do the even columns of 4:2:0 -> 4:4:4
    via = cr.convert(frame, h, w, "420", "422", b, "left")              # against the vertical pass alone
    for p422, p444 in list(zip(cr.split(via, h, w, "422"), cr.split(up, h, w, "444")))[1:]:
        assert np.array_equal(p444[:, 0::2], p422)
    rows = sr.int_rows(40, 20, cr.phase(1, 2, "left"))
    for i in range(3, 17):
        lo, q = rows[i]
        q = q[:7]
        assert q == q[::-1] and lo + 3 == 2 * i and q[3] == max(q)
    # a horizontal impulse at an even column of a 4:4:4 plane lands on one 4:2:0 sample, symmetric around it
    plane = np.zeros((4, 40), np.uint16)
    plane[:, 20] = 1023
    down = sr.resize_plane(plane, 4, 20, b, phase_x=cr.phase(1, 2, "left"))
    assert down[0].argmax() == 10 and np.array_equal(down[0, 7:10], down[0, 13:10:-1])


# ---------------------------------------------------------------------------------------------------------------- Y4M
@pytest.mark.parametrize("tag", sorted(ACCEPTED))
def test_every_accepted_tag_round_trips(tag, tmp_path):
    import pmctf_chroma
    fmt, depth, loc = ACCEPTED[tag]
    head = pmctf_chroma.parse_y4m_header(pmctf_chroma.y4m_header(20, 12, (30000, 1001), tag=tag))
    assert (head["chroma_format"], head["bitdepth"], head["chroma_loc"], head["tag"]) == (fmt, depth, loc, tag)
    assert (head["width"], head["height"], head["frame_rate"], head["interlace"]) == (20, 12, (30000, 1001), "p")
    # the tag the writer chooses reads back as the same format, depth and siting
    own = pmctf_chroma.parse_y4m_header(pmctf_chroma.y4m_header(20, 12, (25, 1), fmt, depth, loc))
    assert (own["chroma_format"], own["bitdepth"], own["chroma_loc"]) == (fmt, depth, loc)
    # a file of the restatement's writer through the product's reader, and back through the restatement's reader
    rng = np.random.default_rng(len(tag))
    frames = [rng.integers(0, 1 << depth, cr.samples(12, 20, fmt)).astype(np.uint8 if depth == 8 else np.uint16)
              for _ in range(3)]
    path = str(tmp_path / "a.y4m")
    cr.write_y4m(path, frames, 20, 12, tag, rate=(24, 1))
    r = pmctf_chroma.PlanarReader(path)
    assert (len(r), r.width, r.height, r.bitdepth, r.chroma_format, r.chroma_loc, r.frame_rate) == \
        (3, 20, 12, depth, fmt, loc, (24, 1))
    for want in frames:
        planes = r.read_one_frame()
        assert [p.shape for p in planes] == list(cr.plane_shapes(12, 20, fmt))
        assert planes[0].dtype == want.dtype and np.array_equal(np.concatenate([p.reshape(-1) for p in planes]), want)
    r.close()
    out = str(tmp_path / "b.y4m")
    with open(out, "wb") as f:
        f.write(pmctf_chroma.y4m_header(20, 12, (24, 1), fmt, depth, loc))
        for fr in frames:
            f.write(b"FRAME\n" + fr.astype("<u2" if depth > 8 else np.uint8).tobytes())
    info, back = cr.read_y4m(out)
    assert (info["W"], info["H"], info["F"], info["I"], info["A"]) == ("20", "12", "24:1", "p", "0:0")
    assert info["C"] == pmctf_chroma.y4m_tag(fmt, depth, loc) and all(np.array_equal(a, b) for a, b in zip(back, frames))


def test_header_defaults_and_frame_parameters(tmp_path):
    import pmctf_chroma
    head = pmctf_chroma.parse_y4m_header(b"YUV4MPEG2 W20 H12 F25:1\nFRAME\n")
    assert (head["tag"], head["chroma_format"], head["chroma_loc"], head["bitdepth"]) == ("420jpeg", "420", "center", 8)
    assert head["header_bytes"] == len(b"YUV4MPEG2 W20 H12 F25:1\n") and head["interlace"] == "?"
    assert pmctf_chroma.parse_y4m_header(b"YUV4MPEG2 W20 H12 I? XYSCSS=420JPEG XCOLORRANGE=LIMITED\n")["frame_rate"] is None
    frames = [np.full(cr.samples(12, 20, "420"), v, np.uint8) for v in (3, 9)]
    path = str(tmp_path / "p.y4m")
    cr.write_y4m(path, frames, 20, 12, None, frame_params="Ip Xnote")   # no C tag; FRAME lines with parameters
    r = pmctf_chroma.PlanarReader(path, 20, 12, bitdepth=8)
    assert len(r) == 2 and r.chroma_format == "420" and r.chroma_loc == "center"
    assert [int(r.read_one_frame()[2][0, 0]) for _ in range(2)] == [3, 9]
    with pytest.raises(AssertionError, match="ends inside a picture"):
        r.read_one_frame()
    for kw in (dict(width=22), dict(height=10), dict(bitdepth=10), dict(chroma_format="444")):
        with pytest.raises(ValueError, match="Y4M header"):
            pmctf_chroma.PlanarReader(path, **kw)
    assert pmctf_chroma.PlanarReader(path, chroma_loc="left").chroma_loc == "left"


@pytest.mark.parametrize("line,named", [
    ("W20 H12 C420paldv", "C420paldv"), ("W20 H12 C411", "C411"), ("W20 H12 C444alpha", "C444alpha"),
    ("W20 H12 Cmono", "Cmono"), ("W20 H12 Cmono16", "Cmono16"), ("W20 H12 C420p8", "C420p8"), ("W20 H12 C440", "C440"),
    ("W20 H12 It", "It"), ("W20 H12 Ib", "Ib"), ("W20 H12 Im", "Im"), ("H12 F25:1", "W tag"), ("W20 F25:1", "H tag"),
    ("W20 H12 F0:1", "F0:1"), ("W20 H12 F25:0", "F25:0"), ("W20 H12 F25", "F25"), ("W21 H12", "W21"), ("W20 H11", "H11"),
    ("W0 H12", "W0"), ("W16386 H12", "W16386"), ("W20 Hx", "Hx"),
])
def test_header_refusals_name_the_tag(line, named):
    import pmctf_chroma
    with pytest.raises(ValueError, match=named):
        pmctf_chroma.parse_y4m_header(f"YUV4MPEG2 {line}\n".encode())


def test_what_is_no_y4m_and_truncated_files(tmp_path):
    import pmctf_chroma
    for data in (b"", b"YUV4MPEG W20 H12\n", b"YUV4MPEG2 W20 H12", b"RIFF....\n"):
        with pytest.raises(ValueError, match="Y4M"):
            pmctf_chroma.parse_y4m_header(data)
    frames = [np.full(cr.samples(12, 20, "444"), v, np.uint8) for v in (1, 2, 3)]
    whole = str(tmp_path / "whole.y4m")
    cr.write_y4m(whole, frames, 20, 12, "444")
    data = open(whole, "rb").read()
    for cut in (100, cr.samples(12, 20, "444") - 1, 3):                  # inside the planes, one byte short, inside "FRAME\n"
        path = str(tmp_path / f"cut{cut}.y4m")
        open(path, "wb").write(data[:len(data) - cr.samples(12, 20, "444") - 6 + (6 - 3 if cut == 3 else 6 + cut)])
        r = pmctf_chroma.PlanarReader(path)
        assert len(r) == 2
        r.read_one_frame(), r.read_one_frame()
        with pytest.raises(AssertionError, match="ends inside a picture"):
            r.read_one_frame()
        r.close()
    bad = bytearray(data)
    at = data.index(b"FRAME", data.index(b"FRAME") + 1)
    bad[at:at + 5] = b"FRANE"
    open(tmp_path / "bad.y4m", "wb").write(bytes(bad))
    with pytest.raises(ValueError, match="FRAME marker"):
        pmctf_chroma.PlanarReader(str(tmp_path / "bad.y4m"))
    # a raw planar file of a stated format
    raw = str(tmp_path / "raw.yuv")
    open(raw, "wb").write(b"".join(f.tobytes() for f in frames) + b"xx")
    r = pmctf_chroma.PlanarReader(raw, 20, 12, chroma_format="444")
    assert len(r) == 3 and r.chroma_loc == "center" and [p.shape for p in r.read_one_frame()] == [(12, 20)] * 3
    with pytest.raises(ValueError, match="center"):
        pmctf_chroma.PlanarReader(raw, 20, 12, chroma_format="422", chroma_loc="center")


# --------------------------------------------------------------------------------------------------------- the header
GOOD = {"format_version": 1, "chroma_format": "444", "chroma_loc": "center", "filter": "catmull-rom-aa/14",
        "frame_rate": [30000, 1001]}


def test_source_format_round_trip(tmp_path):
    import pmctf_chroma
    assert pmctf_chroma.read_source_format(str(tmp_path)) is None
    path = pmctf_chroma.write_source_format(str(tmp_path), "444", "center", (30000, 1001))
    assert os.path.basename(path) == "source_format.json" and json.load(open(path)) == GOOD
    assert pmctf_chroma.read_source_format(str(tmp_path)) == GOOD
    pmctf_chroma.write_source_format(str(tmp_path), "422", "left", None)
    assert pmctf_chroma.read_source_format(str(tmp_path)) == dict(GOOD, chroma_format="422", chroma_loc="left", frame_rate=None)
    os.remove(path)
    for args in (("400", "center"), ("444", "top"), ("422", "center"), ("444", "center", (30, 0)), ("444", "center", 30)):
        with pytest.raises(ValueError):
            pmctf_chroma.write_source_format(str(tmp_path), *args)
    assert not os.path.exists(path)


@pytest.mark.parametrize("change", [
    {"format_version": 2}, {"format_version": "1"}, {"format_version": None}, {"filter": "lanczos3"}, {"filter": 14},
    {"chroma_format": "400"}, {"chroma_format": 444}, {"chroma_format": None}, {"chroma_loc": "top"}, {"chroma_loc": None},
    {"chroma_format": "422"}, {"frame_rate": 30}, {"frame_rate": [30]}, {"frame_rate": [30, 0]}, {"frame_rate": [30.0, 1]},
    {"frame_rate": "30:1"}, {"frame_rate": [True, 1]}, {"extra": 1}, {"filter": None, "drop": "filter"},
    {"frame_rate": None, "drop": "frame_rate"},
])
def test_source_format_refusals(tmp_path, change):
    import pmctf_chroma
    record = dict(GOOD, **change)
    if "drop" in record:
        del record[record.pop("drop")]
    with open(tmp_path / "source_format.json", "w") as f:
        json.dump(record, f)
    with pytest.raises(ValueError, match="source_format.json"):
        pmctf_chroma.read_source_format(str(tmp_path))


def test_source_format_malformed_files(tmp_path):
    import pmctf_chroma
    for text in ("", "{", "[1, 2]", "3", "\"444\""):
        (tmp_path / "source_format.json").write_text(text)
        with pytest.raises(ValueError, match="source_format.json"):
            pmctf_chroma.read_source_format(str(tmp_path))


# ------------------------------------------------------------------------------------------------- the public interface
def test_entry_points_and_keywords():
    import pmctf_chroma
    import pmctf_scale
    for name in ("encode_sequence", "encode_sequence_gops", "encode_sequence_rate"):
        p, base = inspect.signature(getattr(pmctf_chroma, name)).parameters, inspect.signature(getattr(pmctf_scale, name)).parameters
        assert p["coded_size"].default is None and p["chroma_loc"].default is None and p["chroma_format"].default is None
        assert list(p) == list(base)[:-1] + ["chroma_format", "kwargs"] and list(base)[-1] == "kwargs"
        lead = [k for k, v in p.items() if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
        assert lead == [k for k, v in base.items() if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD] and lead[-1] == "device"
    for name in ("decode_sequence_checked", "decode_sequence_layer"):
        p, base = inspect.signature(getattr(pmctf_chroma, name)).parameters, inspect.signature(getattr(pmctf_scale, name)).parameters
        assert list(p) == list(base) + ["coded_format_output"] and p["coded_format_output"].default is False
        assert all(p[k].default == base[k].default for k in base)


def test_refusals_before_any_gpu_work(tmp_path):
    import pmctf_chroma
    src = str(tmp_path / "a.y4m")
    cr.write_y4m(src, [np.zeros(cr.samples(100, 132, "422"), np.uint16)] * 4, 132, 100, "422p10")
    enc = lambda path, *a, **kw: pmctf_chroma.encode_sequence(None, path, *a, 4, 4, 3, str(tmp_path / "bins"), "cpu", **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        enc(src, 132, 100, bitdepth=10)
    with pytest.raises(RuntimeError, match="GPU"):
        enc("x.yuv", 132, 100, chroma_format="444")
    for args, kw, named in (((130, 100), dict(bitdepth=10), "width"), ((132, 98), dict(bitdepth=10), "height"),
                            ((132, 100), {}, "bitdepth"), ((132, 100), dict(bitdepth=10, chroma_format="444"), "chroma_format")):
        with pytest.raises(ValueError, match=named):
            enc(src, *args, **kw)
    with pytest.raises(ValueError, match="center"):
        enc(src, 132, 100, bitdepth=10, chroma_loc="center")
    with pytest.raises(ValueError, match="center"):
        enc("x.yuv", 132, 100, chroma_format="422", chroma_loc="center")
    with pytest.raises(ValueError, match="chroma_format"):
        enc("x.yuv", 132, 100, chroma_format="400")
    with pytest.raises(ValueError, match="src_format"):
        enc("x.yuv", 132, 100, chroma_format="444", src_format="png")
    with pytest.raises(ValueError, match="fps=None"):
        pmctf_chroma.encode_sequence_rate(None, "x.yuv", 132, 100, 4, 4, 60000, None, str(tmp_path / "bins"), "cpu")
    assert not os.path.exists(tmp_path / "bins")


def test_symbols_are_declared_bound_and_refuse_bad_arguments():
    from pMCTF.hip import lib, ops
    header = open(os.path.join(ROOT, "include", "pmctf_hip.h")).read()
    L = C.CDLL(lib.HIP_SO)
    for s in ("pmctf_convert_chroma_u8", "pmctf_convert_chroma_u16"):
        assert f"int {s}(" in header and s in lib.exported_symbols() and hasattr(L, s)
    assert list(inspect.signature(ops.convert_chroma).parameters) == ["frame", "h", "w", "fmt_in", "fmt_out", "tables", "taps",
                                                                     "bitdepth"]
    assert inspect.signature(ops.convert_chroma).parameters["bitdepth"].default == 8
    # refused before any launch (and so without a GPU): the pointers are never looked at
    H = lib.hip()
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)
    taps = (C.c_int * 2)(8, 8)
    ok = (p, p, 18, 34, 444, 420, p, p, taps)
    for fn, depth in ((H.pmctf_convert_chroma_u8, 8), (H.pmctf_convert_chroma_u16, 10)):
        for k in (0, 1, 6, 7, 8):
            bad = list(ok)
            bad[k] = None
            assert fn(*bad, depth, None) == -1, k
        for sizes in ((17, 34), (18, 33), (0, 34), (18, -34), (16386, 34), (18, 16386)):
            assert fn(p, p, *sizes, 444, 420, p, p, taps, depth, None) == -1, sizes
        for fmts in ((400, 420), (444, 411), (0, 444), (420, 4200), (-420, 420)):
            assert fn(p, p, 18, 34, *fmts, p, p, taps, depth, None) == -1, fmts
        for t in ((0, 4), (4, 18), (-1, 4), (4, 100)):
            assert fn(*ok[:8], (C.c_int * 2)(*t), depth, None) == -1, t
        odd = C.c_void_p(p.value + 2)
        assert fn(p, p, 18, 34, 444, 420, odd, p, taps, depth, None) == -1
        assert fn(p, p, 18, 34, 444, 420, p, odd, taps, depth, None) == -1
    for depth in (0, 7, 9, 16):
        assert H.pmctf_convert_chroma_u8(*ok, depth, None) == -1
    for depth in (8, 17, 0, -1):
        assert H.pmctf_convert_chroma_u16(*ok, depth, None) == -1
    assert H.pmctf_convert_chroma_u16(C.c_void_p(p.value + 1), p, *ok[2:], 10, None) == -1
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.convert_chroma(torch.zeros(18 * 34 * 3, dtype=torch.uint8), 18, 34, "444", "420", [None] * 2, [8] * 2)
    with pytest.raises(ValueError):
        ops.convert_chroma(torch.zeros(18 * 34 * 3, dtype=torch.uint8), 18, 34, "444", "411", [None] * 2, [8] * 2)
    with pytest.raises(ValueError):
        ops.convert_chroma(torch.zeros(18 * 34 * 2, dtype=torch.uint8), 18, 34, "444", "420", [None] * 2, [8] * 2)


# ------------------------------------------------------------------------------------------------------ the command line
def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_y4m_info(tmp_path, capsys):
    path = str(tmp_path / "a.y4m")
    cr.write_y4m(path, [np.zeros(cr.samples(12, 20, "422"), np.uint16)] * 5, 20, 12, "422p10", rate=(50, 1))
    _tool("y4m_info").main([path])
    out = json.loads(capsys.readouterr().out)
    assert out["frames"] == 5 and out["tag"] == "422p10" and out["frame_rate"] == [50, 1] and out["truncated"] is False
    assert (out["width"], out["height"], out["bitdepth"], out["chroma_format"], out["chroma_loc"]) == (20, 12, 10, "422", "left")
    open(path, "wb").write(b"YUV4MPEG2 W20 H12 C411\n")
    with pytest.raises(SystemExit) as e:
        _tool("y4m_info").main([path])
    assert "C411" in str(e.value.code)


@pytest.mark.parametrize("tag,extra,message", [
    ("444", ["--width", "130"], "--width 130"), ("444", ["--bitdepth", "10"], "--bitdepth 10"),
    ("422p10", ["--chroma-format", "444"], "--chroma-format 444"), ("422", ["--chroma-loc", "center"], "--chroma-loc"),
    ("444", ["--chroma-format", "400"], "invalid choice"), ("411", [], "C411"), ("420jpeg", ["--bitrate", "60000"], "--fps"),
])
def test_encode_cli_reads_the_header_and_refuses(tmp_path, capsys, tag, extra, message):
    src = str(tmp_path / "src.y4m")
    fmt, depth = ("420", 8) if tag in ("420jpeg", "411") else (tag[:3], 10 if tag.endswith("p10") else 8)
    cr.write_y4m(src, [np.zeros(cr.samples(100, 132, fmt), np.uint16 if depth > 8 else np.uint8)] * 4, 132, 100, tag,
                 rate=None)
    with pytest.raises(SystemExit) as e:
        _tool("encode_sequence").main(["--synth-seed", "0", "--gop", "4", *extra, src, str(tmp_path / "bins")])
    assert e.value.code == 2 and message in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "bins")


def test_decode_cli_has_the_option():
    text = open(os.path.join(ROOT, "tools", "decode_sequence.py")).read()
    assert "--coded-format-output" in text and "coded_format_output=a.coded_format_output" in text
