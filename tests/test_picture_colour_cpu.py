"""RGB pictures without a GPU: the product's coefficient tables against the restatement, the properties the
definition gives them, the fixed point against exact rational arithmetic, the round-trip error over every 8-bit triple, the
four entries of include/pmctf_colour.h (declared, exported, bound, refusing before any launch), colour_format.json, and every
refusal of the entry points and the command lines."""
import ctypes as C
import importlib.util
import inspect
import json
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import colour_restatement as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pmctf_rgb_to_ycc_u8", "pmctf_rgb_to_ycc_u16", "pmctf_ycc_to_rgb_u8", "pmctf_ycc_to_rgb_u16")
CASES = [(m, r) for m in ("bt601", "bt709", "bt2020") for r in ("full", "limited")]
DEPTHS = (8, 9, 10, 12, 16)
# the largest |RGB -> 4:4:4 -> RGB - RGB| over all 2^24 triples at 8 bits, measured on the restatement
ROUND_TRIP_8BIT = {("bt601", "full"): 1, ("bt601", "limited"): 2, ("bt709", "full"): 1, ("bt709", "limited"): 2,
                   ("bt2020", "full"): 1, ("bt2020", "limited"): 2}


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the codec was touched ({name}) before the arguments were checked")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ----------------------------------------------------------------------------------------------------- the arithmetic
@pytest.mark.parametrize("matrix,rng", CASES)
def test_coefficients_are_the_restatements_and_have_their_properties(matrix, rng):
    import pmctf_colour
    for b in DEPTHS:
        fwd, inv, off = pmctf_colour.coefficients(matrix, rng, b)
        kf, ki, o = cr.tables(matrix, rng, b)
        assert [list(r) for r in fwd] == kf and [list(r) for r in inv] == ki and tuple(off) == tuple(o), b
        assert all(isinstance(k, int) and abs(k) < 1 << 31 for row in fwd + inv for k in row), b
        sy, _, oy, oc = cr.scales(rng, b)
        assert [sum(r) for r in fwd] == [round(Fraction(sy, (1 << b) - 1) * 2 ** 29), 0, 0], b
        if rng == "full":
            assert sum(fwd[0]) == 1 << 29 and off == (0, 1 << (b - 1), 1 << (b - 1))
        assert inv[0][0] == inv[1][0] == inv[2][0] and inv[0][1] == 0 and inv[2][2] == 0
        # every coefficient but the forward G column is the rounding of its exact value; G is within a unit of it
        ef, ei = cr.exact_rows(matrix, rng, b)
        for row, exact in zip(fwd, ef):
            assert row[0] == round(exact[0] * 2 ** 29) and row[2] == round(exact[2] * 2 ** 29)
            assert abs(row[1] - exact[1] * 2 ** 29) <= Fraction(3, 2)
        assert all(k == round(c * 2 ** 29) for row, exact in zip(inv, ei) for k, c in zip(row, exact))
    assert max(abs(k) for m, r in CASES for b in (8, 10, 12, 16) for t in pmctf_colour.coefficients(m, r, b)[:2]
               for row in t for k in row) == 1154346882


@pytest.mark.parametrize("matrix,rng", CASES)
def test_greys_are_exact(matrix, rng):
    for b, values in ((8, np.arange(256)), (10, np.arange(1024)), (16, np.array([0, 1, 255, 256, 32767, 32768, 65534, 65535]))):
        y, cb, c = cr.forward(values, values, values, matrix, rng, b)
        assert (cb == 1 << (b - 1)).all() and (c == 1 << (b - 1)).all()
        if rng == "full":
            assert np.array_equal(y, values)
        else:
            sy, _, oy, _ = cr.scales(rng, b)
            k = round(Fraction(sy, (1 << b) - 1) * 2 ** 29)
            assert y.tolist() == [((k * int(v) + (oy << 29) + (1 << 28)) >> 29) for v in values]
            assert y[0] == oy and y[-1] == oy + sy                      # black and white land on 16 and 235 (scaled)
        r, g, bl = cr.inverse(y, cb, c, matrix, rng, b)
        assert np.array_equal(r, g) and np.array_equal(g, bl)
        if rng == "full":
            assert np.array_equal(r, values)


@pytest.mark.parametrize("matrix,rng", CASES)
def test_fixed_point_against_exact_rationals(matrix, rng):
    """|result - clamp(exact)| <= 1/2 + 2^-12 in both directions: four half-units of 2^-30 on samples below 2^16"""
    bound = Fraction(1, 2) + Fraction(1, 1 << 12)
    for b in (8, 10, 12, 16):
        rs = np.random.default_rng(1000 * b + len(matrix) + len(rng))
        top = (1 << b) - 1
        x = rs.integers(0, top + 1, (3, 1500))
        x[:, :8] = np.array([[0, 0, 0, 0, top, top, top, top], [0, 0, top, top, 0, 0, top, top], [0, top, 0, top, 0, top, 0, top]])
        fwd, inv = cr.forward(*x, matrix, rng, b), cr.inverse(*x, matrix, rng, b)
        for j in range(x.shape[1]):
            t = [int(v) for v in x[:, j]]
            for got, want in zip(fwd, cr.exact_forward(t, matrix, rng, b)):
                assert abs(int(got[j]) - want) <= bound, (b, t, "forward")
            for got, want in zip(inv, cr.exact_inverse(t, matrix, rng, b)):
                assert abs(int(got[j]) - want) <= bound, (b, t, "inverse")


@pytest.mark.parametrize("matrix,rng", CASES)
def test_round_trip_error_over_every_8_bit_triple(matrix, rng):
    g, b = (v.ravel() for v in np.meshgrid(np.arange(256), np.arange(256), indexing="ij"))
    G, B = np.tile(g, 16), np.tile(b, 16)
    worst = 0
    for r0 in range(0, 256, 16):
        R = np.repeat(np.arange(r0, r0 + 16), 65536)
        back = cr.inverse(*cr.forward(R, G, B, matrix, rng, 8), matrix, rng, 8)
        worst = max(worst, max(int(np.abs(x - y).max()) for x, y in zip(back, (R, G, B))))
    assert worst == ROUND_TRIP_8BIT[(matrix, rng)]


def test_layouts_by_hand():
    import pmctf_colour
    assert set(pmctf_colour.LAYOUTS) == set(cr.LAYOUTS)
    header = open(os.path.join(ROOT, "include", "pmctf_colour.h")).read()
    for name, (code, depth, comps) in pmctf_colour.LAYOUTS.items():
        assert re.search(rf"#define PMCTF_RGB_{name.upper()} {code}\b", header), name
        assert depth == cr.LAYOUTS[name][0] and comps == len(cr.LAYOUTS[name][2])
        for w, h in ((2, 2), (10, 6), (132, 100)):
            assert pmctf_colour.frame_bytes(name, w, h) == cr.frame_bytes(name, h, w)
    assert re.search(r"#define PMCTF_COLOUR_FIXED_POINT_BITS 29\b", header) and pmctf_colour.FIXED_POINT_BITS == 29
    r, g, b = np.array([1, 2, 3, 4]), np.array([11, 12, 13, 14]), np.array([21, 22, 23, 24])
    assert bytes(cr.pack_rgb(r, g, b, "rgb24", 2, 2)) == bytes([1, 11, 21, 2, 12, 22, 3, 13, 23, 4, 14, 24])
    assert bytes(cr.pack_rgb(r, g, b, "bgra", 2, 2))[:8] == bytes([21, 11, 1, 255, 22, 12, 2, 255])
    assert bytes(cr.pack_rgb(r, g, b, "gbrp", 2, 2)) == bytes([11, 12, 13, 14, 21, 22, 23, 24, 1, 2, 3, 4])
    assert bytes(cr.pack_rgb(r * 256, g, b, "rgb48", 2, 2))[:6] == bytes([0, 1, 11, 0, 21, 0])
    assert bytes(cr.pack_rgb(r, g, b * 40, "gbrp10", 2, 2))[8:12] == bytes([0x48, 3, 0x70, 3])
    for name in cr.LAYOUTS:
        top = (1 << cr.LAYOUTS[name][0]) - 1
        x = np.random.default_rng(5).integers(0, top + 1, (3, 60))
        assert all(np.array_equal(a, c) for a, c in zip(cr.unpack_rgb(cr.pack_rgb(*x, name, 6, 10), name, 6, 10), x)), name
    assert pmctf_colour.frame_bytes("rgb48", 16384, 16384) == 6 << 28
    for bad in ("rgb", "RGB24", None, 24):
        with pytest.raises(ValueError, match="rgb_layout"):
            pmctf_colour.check_rgb_layout(bad)


# --------------------------------------------------------------------------------------------------------- the entries
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(pmctf_\w+)\s*\(", text))


def test_entries_are_declared_in_their_own_header_exported_and_bound():
    import pmctf_colour
    from pMCTF.hip import lib
    assert _declared("pmctf_colour.h") == set(ENTRIES) == set(pmctf_colour.SIGS)
    assert not _declared("pmctf_hip.h") & set(ENTRIES) and not set(lib.exported_symbols()) & set(ENTRIES)
    H = C.CDLL(lib.HIP_SO)
    src = open(os.path.join(ROOT, "learned-pmctf_amd", "csrc", "picture_colour.hip")).read()
    for s in ENTRIES:
        assert hasattr(H, s), f"libpmctf_hip.so does not export {s}"
        assert re.search(r'extern "C" int ' + s + r"\(", src), s
    L = pmctf_colour.library()
    assert L is lib.hip() and all(getattr(L, s).argtypes == pmctf_colour.SIGS[s][1] for s in ENTRIES)
    assert "../include/pmctf_colour.h" in open(os.path.join(ROOT, "learned-pmctf_amd", "Makefile")).read()


def test_entries_refuse_bad_arguments_before_any_launch():
    import pmctf_colour
    L = pmctf_colour.library()
    one, odd = C.c_void_p(4096), C.c_void_p(4097)
    k, o = (C.c_int32 * 9)(*range(1, 10)), (C.c_int64 * 3)(16, 128, 128)
    u8 = [lambda a, b, lay, h, w, k_, o_, fn=fn: fn(a, b, lay, h, w, k_, o_, None)
          for fn in (L.pmctf_rgb_to_ycc_u8, L.pmctf_ycc_to_rgb_u8)]
    u16 = [lambda a, b, lay, h, w, k_, o_, depth=None, fn=fn: fn(a, b, lay, h, w, {4: 16, 6: 10, 7: 12, 8: 16}.get(lay, 10)
                                                                 if depth is None else depth, k_, o_, None)
           for fn in (L.pmctf_rgb_to_ycc_u16, L.pmctf_ycc_to_rgb_u16)]
    for fns, good, foreign in ((u8, (0, 1, 2, 3, 5), (4, 6, 7, 8)), (u16, (4, 6, 7, 8), (0, 1, 2, 3, 5))):
        for fn in fns:
            assert fn(None, None, good[0], 6, 10, None, None) == -1
            for j in range(4):                                           # each pointer on its own
                p = [one, one, k, o]
                p[j] = None
                assert fn(p[0], p[1], good[0], 6, 10, p[2], p[3]) == -1, j
            for lay in (-1, 9, 100) + foreign:                           # unknown, and of the other entry's container
                assert fn(one, one, lay, 6, 10, k, o) == -1, lay
            for lay in good:
                for h, w in ((5, 10), (6, 9), (0, 10), (6, 0), (-2, 10), (6, -2), (16386, 10), (6, 16386)):
                    assert fn(one, one, lay, h, w, k, o) == -1, (lay, h, w)
            for bad in ((-1, 128, 128), (16, 65536, 128), (16, 128, 1 << 40)):
                assert fn(one, one, good[0], 6, 10, k, (C.c_int64 * 3)(*bad)) == -1, bad
    for fn in u16:
        assert fn(odd, one, 6, 6, 10, k, o) == -1 and fn(one, odd, 6, 6, 10, k, o) == -1
        for lay, depth in ((6, 12), (6, 16), (6, 8), (7, 10), (8, 12), (4, 10), (4, 8), (6, 0), (6, 17)):
            assert fn(one, one, lay, 6, 10, k, o, depth) == -1, (lay, depth)


def test_wrappers_refuse_without_a_gpu():
    import torch
    import pmctf_colour
    surface = torch.zeros(180, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pmctf_colour.rgb_to_ycc(surface, "rgb24", 6, 10, ("bt709", "limited"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pmctf_colour.ycc_to_rgb(surface, "rgb24", 6, 10, ("bt709", "limited"))
    with pytest.raises(ValueError, match="rgb_layout"):
        pmctf_colour.rgb_to_ycc(surface, "rgb32", 6, 10, ("bt709", "limited"))
    with pytest.raises(ValueError, match="matrix"):
        pmctf_colour.rgb_to_ycc(surface, "rgb24", 6, 10, ("bt470", "limited"))
    with pytest.raises(ValueError, match="sides are even"):
        pmctf_colour.RgbUnpacker("rgb24", 9, 6, ("bt709", "limited"))
    u, p = pmctf_colour.RgbUnpacker("gbrp10", 10, 6, ("bt2020", "full")), pmctf_colour.RgbPacker("rgba", 10, 6, ("bt601", "full"))
    assert (u.layout, u.size, u.shape, u.bitdepth, u.chroma_format, u.frame_bytes) == ("gbrp10", (10, 6), (6, 10), 10, "444", 360)
    assert (p.layout, p.size, p.shape, p.bitdepth, p.chroma_format, p.frame_bytes) == ("rgba", (10, 6), (6, 10), 8, "444", 240)
    assert list(inspect.signature(u.__call__).parameters) == ["surface", "out"]
    assert list(inspect.signature(p.__call__).parameters) == ["frame", "out"]


# ------------------------------------------------------------------------------------------------- colour_format.json
def test_colour_format_round_trip_and_refusals(tmp_path):
    import pmctf_colour
    folder = str(tmp_path)
    assert pmctf_colour.read_colour_format(folder) is None
    path = pmctf_colour.write_colour_format(folder, ("bt2020", "limited"), "rgb")
    assert path == os.path.join(folder, "colour_format.json") and os.listdir(folder) == ["colour_format.json"]
    good = {"format_version": 1, "matrix": "bt2020", "range": "limited", "fixed_point_bits": 29, "source": "rgb"}
    assert json.load(open(path)) == good == pmctf_colour.read_colour_format(folder)
    assert pmctf_colour.read_colour_format(folder)["source"] == "rgb"
    pmctf_colour.write_colour_format(folder, ("bt601", "full"), "ycbcr")
    assert pmctf_colour.read_colour_format(folder) == dict(good, matrix="bt601", range="full", source="ycbcr")
    for colour, source, text in ((("bt470", "full"), "rgb", "matrix"), (("bt709", "video"), "rgb", "range"),
                                 (("bt709", "full"), "xyz", "source"), ("bt709", "rgb", "colour")):
        with pytest.raises(ValueError, match=text):
            pmctf_colour.write_colour_format(folder, colour, source)

    def refused(record, text):
        with open(path, "w") as f:
            f.write(record if isinstance(record, str) else json.dumps(record))
        with pytest.raises(ValueError, match=text) as e:
            pmctf_colour.read_colour_format(folder)
        assert "colour_format.json" in str(e.value)
    refused("{not json", "not a colour format file")
    refused([1, 2], "format version")
    refused(dict(good, format_version=2), "format version 2")
    refused(dict(good, fixed_point_bits=30), "fixed_point_bits 30")
    refused(dict(good, fixed_point_bits=29.0), "fixed_point_bits")
    refused(dict(good, matrix="bt2020c"), "matrix 'bt2020c'")
    refused(dict(good, matrix=["bt709"]), "matrix")
    refused(dict(good, range="pc"), "range 'pc'")
    refused(dict(good, source="png"), "source 'png'")
    refused(dict(good, transfer="pq"), "fields")
    refused({k: v for k, v in good.items() if k != "range"}, "fields")


# -------------------------------------------------------------------------------------------------------- the refusals
def _rgb_file(tmp_path, nbytes=3 * 10 * 6 * 5, name="src.rgb"):            # five rgb24 pictures of 10 x 6
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.truncate(nbytes)
    return p


def test_encoder_refusals_come_before_the_device(tmp_path):
    import pmctf_colour
    src, bins = _rgb_file(tmp_path), str(tmp_path / "bins")
    y4m = str(tmp_path / "src.y4m")
    calls = [lambda **kw: pmctf_colour.encode_sequence(_NoDevice(), kw.pop("src", src), 10, 6, 4, 4, 3, bins, "cpu", **kw),
             lambda **kw: pmctf_colour.encode_sequence_gops(_NoDevice(), kw.pop("src", src), 10, 6, 4, 4, 3, bins, "cpu", **kw),
             lambda **kw: pmctf_colour.encode_sequence_rate(_NoDevice(), kw.pop("src", src), 10, 6, 4, 4, 60000, (30, 1), bins,
                                                            "cpu", **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="rgb_layout 'rgb24' with a .y4m"):
            call(src=y4m, rgb_layout="rgb24")
        with pytest.raises(ValueError, match="rgb_layout 'rgb24' with pixel_layout 'nv12'"):
            call(rgb_layout="rgb24", pixel_layout="nv12")
        with pytest.raises(ValueError, match="rgb_layout 'rgb24' with pitch"):
            call(rgb_layout="rgb24", pitch=64)
        for fmt in ("420", "422"):
            with pytest.raises(ValueError, match=f"rgb_layout 'rgb24' with chroma_format '{fmt}'"):
                call(rgb_layout="rgb24", chroma_format=fmt)
        with pytest.raises(ValueError, match="bitdepth 10 contradicts rgb_layout 'rgb24'"):
            call(rgb_layout="rgb24", bitdepth=10)
        with pytest.raises(ValueError, match="bitdepth 8 contradicts rgb_layout 'gbrp10'"):
            call(rgb_layout="gbrp10", bitdepth=8)
        with pytest.raises(ValueError, match="rgb_layout is one of"):
            call(rgb_layout="rgb32")
        with pytest.raises(ValueError, match="rgb_layout 'rgb24' with src_format 'png'"):
            call(rgb_layout="rgb24", src_format="png")
        with pytest.raises(ValueError, match=r"not a whole number of rgba pictures of 10x6 \(240 bytes each; rgb_layout\)"):
            call(rgb_layout="rgba")
        for colour, text in ((("bt470", "full"), "matrix"), (("bt709", "tv"), "range"), ("bt709", "colour is")):
            with pytest.raises(ValueError, match=text):
                call(rgb_layout="rgb24", colour=colour)
            with pytest.raises(ValueError, match=text):                 # a YCbCr source: the description alone
                call(colour=colour)
            with pytest.raises(ValueError, match=text):
                call(src=str(tmp_path), src_format="png", colour=colour)
        with pytest.raises(ValueError, match="sides are even"):
            pmctf_colour.encode_sequence(_NoDevice(), src, 9, 6, 4, 4, 3, bins, "cpu", rgb_layout="rgb24")
        # what is not refused reaches the device question, which a CPU answers with RuntimeError
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(rgb_layout="rgb24", chroma_format="444", bitdepth=8, colour=("bt2020", "full"))
    with pytest.raises(ValueError, match="fps=None"):
        pmctf_colour.encode_sequence_rate(_NoDevice(), src, 10, 6, 4, 4, 60000, None, bins, "cpu", rgb_layout="rgb24")
    # the refusals of a PNG source stay, with or without a colour
    for kw in (dict(chroma_format="444"), dict(pixel_layout="nv12")):
        with pytest.raises(ValueError):
            calls[0](src=str(tmp_path), src_format="png", colour=("bt709", "limited"), **kw)
        with pytest.raises(ValueError):
            calls[0](src=str(tmp_path), src_format="png", **kw)
    assert not os.path.exists(bins)
    # the keywords are pmctf_layout's with the two new ones at the end
    import pmctf_layout
    for name in ("encode_sequence", "encode_sequence_gops", "encode_sequence_rate"):
        ours, theirs = (list(inspect.signature(getattr(m, name)).parameters) for m in (pmctf_colour, pmctf_layout))
        assert ours == theirs[:-1] + ["rgb_layout", "colour", "kwargs"], name
    for name in ("decode_sequence_checked", "decode_sequence_layer"):
        ours, theirs = (list(inspect.signature(getattr(m, name)).parameters) for m in (pmctf_colour, pmctf_layout))
        assert ours == theirs + ["rgb_out", "rgb_layout", "colour"], name


def _fake_folder(path, bitdepth=8, colour=None):
    import pmctf_colour
    import pmctf_gop
    os.makedirs(path)
    pmctf_gop.write_sequence_header(path, width=132, height=100, frame_num=4, gop=4, q_index=3, psize=128, me_downsample=1,
                                    ll_order="plane", num_me_stages=1, precision="f32", aten_threads=1)
    if bitdepth > 8:
        pmctf_gop.write_picture_format(path, bitdepth)
    if colour is not None:
        pmctf_colour.write_colour_format(path, colour, "rgb")
    return path


def test_decoder_refusals_come_before_the_codec(tmp_path):
    import pmctf_colour
    plain = _fake_folder(str(tmp_path / "plain"))
    known = _fake_folder(str(tmp_path / "known"), colour=("bt709", "limited"))
    deep = _fake_folder(str(tmp_path / "deep"), 10, ("bt2020", "limited"))
    out, yuv = str(tmp_path / "never.rgb"), str(tmp_path / "never.yuv")
    full = lambda folder, **kw: pmctf_colour.decode_sequence_checked(_NoDevice(), folder, kw.pop("yuv", None), **kw)
    layer = lambda folder, **kw: pmctf_colour.decode_sequence_layer(_NoDevice(), folder, kw.pop("yuv", None), 0, **kw)
    for call in (full, layer):
        with pytest.raises(ValueError, match="rgb_out and rgb_layout go together"):
            call(known, rgb_out=out)
        with pytest.raises(ValueError, match="rgb_out and rgb_layout go together"):
            call(known, rgb_layout="rgb24")
        with pytest.raises(ValueError, match="rgb_layout is one of"):
            call(known, rgb_out=out, rgb_layout="rgb32")
        for colour, text in ((("bt470", "full"), "matrix"), (("bt709", "tv"), "range")):
            with pytest.raises(ValueError, match=text):
                call(known, rgb_out=out, rgb_layout="rgb24", colour=colour)
        with pytest.raises(ValueError, match=r"plain.colour_format\.json: missing"):
            call(plain, rgb_out=out, rgb_layout="rgb24")
        with pytest.raises(ValueError, match=r"rgb_layout 'gbrp10' holds pictures of 10 bits; the pictures of .*known have 8 bits"):
            call(known, rgb_out=out, rgb_layout="gbrp10")
        with pytest.raises(ValueError, match=r"rgb_layout 'rgb24' holds pictures of 8 bits; the pictures of .*deep have 10 bits"):
            call(deep, rgb_out=out, rgb_layout="rgb24")
        with pytest.raises(ValueError, match="rgb_layout 'rgb48' holds pictures of 16 bits"):
            call(plain, rgb_out=out, rgb_layout="rgb48", colour=("bt601", "full"))
        with pytest.raises(ValueError, match="png_out writes 8-bit PNGs"):                 # with and without a description
            call(deep, png_out=str(tmp_path / "pngs"))
        with pytest.raises(ValueError, match="png_out writes 8-bit PNGs"):
            call(deep, png_out=str(tmp_path / "pngs"), rgb_out=out, rgb_layout="gbrp10")
        with pytest.raises(ValueError, match="verify is"):
            call(known, rgb_out=out, rgb_layout="rgb24", verify="maybe")
        with pytest.raises(ValueError, match="nothing to write"):
            call(known)
        with open(os.path.join(known, "colour_format.json")) as f:
            saved = f.read()
        with open(os.path.join(known, "colour_format.json"), "w") as f:
            f.write(saved.replace("29", "30"))
        with pytest.raises(ValueError, match="fixed_point_bits 30"):
            call(known, rgb_out=out, rgb_layout="rgb24")
        with open(os.path.join(known, "colour_format.json"), "w") as f:
            f.write(saved)
    assert not os.path.exists(out) and not os.path.exists(yuv) and not os.path.exists(str(tmp_path / "pngs"))


def test_convert_file_and_the_command_lines_refuse_without_a_gpu(tmp_path, capsys):
    import pmctf_colour
    src, dst = _rgb_file(tmp_path), str(tmp_path / "out.yuv")
    conv = lambda a, b, **kw: pmctf_colour.convert_file(kw.pop("src", src), dst, 10, 6, a, b, kw.pop("colour", ("bt709", "full")),
                                                         "cpu", **kw)
    for a, b in (("rgb24", "bgr24"), ("planar444", "planar444")):
        with pytest.raises(ValueError, match="one of from_layout and to_layout is 'planar444'"):
            conv(a, b)
    with pytest.raises(ValueError, match="from_layout is one of"):
        conv("rgb32", "planar444")
    with pytest.raises(ValueError, match="to_layout is one of"):
        conv("planar444", "planar")
    with pytest.raises(ValueError, match="bitdepth 10 contradicts 'rgb24'"):
        conv("rgb24", "planar444", bitdepth=10)
    with pytest.raises(ValueError, match="matrix"):
        conv("rgb24", "planar444", colour=("bt470", "full"))
    with pytest.raises(ValueError, match="not a whole number of rgba pictures"):
        conv("rgba", "planar444")
    with pytest.raises(ValueError, match="not a whole number of planar444 pictures"):
        conv("planar444", "rgb48")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv("rgb24", "planar444", bitdepth=8)
    assert not os.path.exists(dst)
    for argv, text in ((["--from", "rgb24", "--to", "bgr24"], "planar444"), (["--from", "rgb24", "--to", "planar444", "--matrix", "x"], "matrix")):
        with pytest.raises(SystemExit):
            _tool("convert_colour").main(["--width", "10", "--height", "6", *argv, src, dst])
        assert text in capsys.readouterr().err
    enc = _tool("encode_sequence")
    for argv, text in ((["--rgb-layout", "rgb32", "--width", "10", "--height", "6"], "--rgb-layout"),
                       (["--rgb-layout", "rgb24"], "--width and --height are required with --rgb-layout"),
                       (["--rgb-layout", "rgb24", "--pixel-layout", "nv12", "--width", "10", "--height", "6"], "--pixel-layout"),
                       (["--rgb-layout", "gbrp10", "--bitdepth", "8", "--width", "10", "--height", "6"], "--bitdepth 8"),
                       (["--rgb-layout", "rgb24", "--chroma-format", "420", "--width", "10", "--height", "6"], "--chroma-format 420"),
                       (["--rgb-layout", "rgba", "--width", "10", "--height", "6"], "not a whole number of rgba pictures"),
                       (["--colour-matrix", "bt470", "--width", "10", "--height", "6"], "--colour-matrix")):
        with pytest.raises(SystemExit):
            enc.main(["--synth-seed", "0", *argv, src, str(tmp_path / "bins")])
        assert text in capsys.readouterr().err, argv
    dec = _tool("decode_sequence")
    plain = _fake_folder(str(tmp_path / "plain"))
    for argv, text in ((["--rgb-output", dst], "--rgb-output and --rgb-layout go together"),
                       (["--rgb-layout", "rgb24"], "--rgb-output and --rgb-layout go together"),
                       (["--rgb-output", dst, "--rgb-layout", "rgb32"], "--rgb-layout is one of"),
                       (["--rgb-output", dst, "--rgb-layout", "rgb24", "--colour-matrix", "bt709"], "go together"),
                       (["--rgb-output", dst, "--rgb-layout", "rgb24"], "colour_format.json is missing")):
        with pytest.raises(SystemExit):
            dec.main(["--synth-seed", "0", *argv, plain])
        assert text in capsys.readouterr().err, argv
    assert not os.path.exists(dst) and not os.path.exists(str(tmp_path / "bins"))
