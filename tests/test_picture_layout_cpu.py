"""Pixel layouts without a GPU: the restatement against hand-written answers and against itself, the product's
table, sizes, refusals, readers, C entries and command lines."""
import ctypes as C
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest

import layout_restatement as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(2, 2), (6, 10), (100, 132)]                 # rows x columns
V210_WIDTHS = (2, 4, 6, 8, 10, 12, 46, 48, 50)


def _frame(layout, h, w, seed):
    depth = lr.TABLE[layout][1]
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << depth, lr.samples(layout, h, w)).astype(np.uint8 if depth == 8 else np.uint16)


# ------------------------------------------------------------------------------------------------- the known answers
def test_v210_word_zero_by_hand():
    # 2 x 2: Y = 2, Cb = 1, Cr = 3 everywhere; word 0 = Cb0 | Y0 << 10 | Cr0 << 20 = 0x00300801
    frame = np.array([2, 2, 2, 2, 1, 1, 3, 3], np.uint16)
    out = lr.pack(frame, "v210", 2, 2)
    assert out.size == 2 * 128
    assert bytes(out[:4]) == bytes([0x01, 0x08, 0x30, 0x00]) and int.from_bytes(bytes(out[:4]), "little") == 0x00300801
    # 8 bytes of each row carry data: word 0 whole and bits 0-9 of word 1 (Y1 = 2)
    for r in range(2):
        assert bytes(out[128 * r + 4:128 * r + 8]) == bytes([0x02, 0, 0, 0])
        assert not out[128 * r + 8:128 * (r + 1)].any()
    assert np.array_equal(lr.pack_v210_scalar(frame, 2, 2), out)


def test_p010_by_hand():
    frame = np.full(lr.samples("p010", 2, 2), 0x3FF, np.uint16)
    out = lr.pack(frame, "p010", 2, 2)
    assert out.size == 12 and bytes(out[:2]) == bytes([0xC0, 0xFF]) and bytes(out) == bytes([0xC0, 0xFF]) * 6
    assert np.array_equal(lr.unpack(np.full(12, 0xFF, np.uint8), "p010", 2, 2), frame)       # word 0xFFFF -> 0x3FF


def test_byte_orders_by_hand():
    # 2 x 2 picture: Y = 10 11 / 12 13, Cb = 20 (21 in row 1 of 4:2:2), Cr = 30 (31)
    f420 = np.array([10, 11, 12, 13, 20, 30], np.uint8)
    f422 = np.array([10, 11, 12, 13, 20, 21, 30, 31], np.uint8)
    assert bytes(lr.pack(f420, "nv12", 2, 2)) == bytes([10, 11, 12, 13, 20, 30])
    assert bytes(lr.pack(f420, "nv21", 2, 2)) == bytes([10, 11, 12, 13, 30, 20])
    assert bytes(lr.pack(f422, "nv16", 2, 2)) == bytes([10, 11, 12, 13, 20, 30, 21, 31])
    assert bytes(lr.pack(f422, "yuyv", 2, 2)) == bytes([10, 20, 11, 30, 12, 21, 13, 31])
    assert bytes(lr.pack(f422, "uyvy", 2, 2)) == bytes([20, 10, 30, 11, 21, 12, 31, 13])
    assert bytes(lr.pack(f422.astype(np.uint16), "y212", 2, 2)[:8]) == bytes([0xA0, 0, 0x40, 1, 0xB0, 0, 0xE0, 1])
    # pitch and luma_rows: nv12 with pitch 4 and 3 luma rows
    out = lr.pack(f420, "nv12", 2, 2, pitch=4, luma_rows=3, into=np.full(14, 0xEE, np.uint8))
    assert bytes(out) == bytes([10, 11, 0xEE, 0xEE, 12, 13, 0xEE, 0xEE, 0xEE, 0xEE, 0xEE, 0xEE, 20, 30])


# ------------------------------------------------------------------------------------------- the restatement on itself
@pytest.mark.parametrize("layout", sorted(lr.TABLE))
def test_restatement_round_trips(layout):
    container = lr.TABLE[layout][2]
    for h, w in SIZES:
        for pitch_extra, rows_extra in ((0, 0), (container, 2), (64, 0)):
            pitch = lr.row_bytes(layout, w) + pitch_extra
            frame = _frame(layout, h, w, h * w)
            surface = lr.pack(frame, layout, h, w, pitch, h + rows_extra)
            assert surface.size == lr.geometry(layout, h, w, pitch, h + rows_extra)[3]
            assert np.array_equal(lr.unpack(surface, layout, h, w, pitch, h + rows_extra), frame)
            assert np.array_equal(lr.pack(lr.unpack(surface, layout, h, w, pitch, h + rows_extra), layout, h, w, pitch,
                                          h + rows_extra), surface)
            # what unpacking ignores: every bit that pack leaves zero, set
            loud = surface | ~lr.pack(np.full(frame.size, 0xFFFF, np.uint16), layout, h, w, pitch, h + rows_extra)
            assert np.array_equal(lr.unpack(loud, layout, h, w, pitch, h + rows_extra), frame)


@pytest.mark.parametrize("w", V210_WIDTHS)
def test_v210_two_formulations_agree(w):
    for h in (2, 6):
        frame = _frame("v210", h, w, w)
        surface = lr.pack(frame, "v210", h, w)
        assert np.array_equal(surface, lr.pack_v210_scalar(frame, h, w))
        assert np.array_equal(lr.unpack_v210_scalar(surface, h, w), frame)
        assert np.array_equal(lr.unpack(surface, "v210", h, w), frame)
        assert np.array_equal(lr.unpack_v210_scalar(surface | np.tile(np.array([0, 0, 0, 0xC0], np.uint8), surface.size // 4),
                                                    h, w), frame)            # bits 30-31 set


# --------------------------------------------------------------------------------------------------- the product's table
def test_layouts_agree_with_the_restatement():
    import pmctf_layout
    assert set(pmctf_layout.LAYOUTS) == set(lr.TABLE)
    for name, (fmt, depth, container, family) in lr.TABLE.items():
        assert pmctf_layout.LAYOUTS[name] == {"chroma_format": fmt, "bitdepth": depth, "container": container,
                                              "family": family}
    header = open(os.path.join(ROOT, "include", "pmctf_hip.h")).read()
    from pMCTF.hip import ops
    for name, (code, *_rest) in ops.LAYOUTS.items():
        assert re.search(rf"#define PMCTF_LAYOUT_{name.upper()} {code}\b", header), name


def test_frame_bytes_and_default_pitch_by_hand():
    import pmctf_layout as pl
    assert pl.default_pitch("nv12", 132) == 132 and pl.default_pitch("p010", 132) == 264
    assert pl.default_pitch("yuyv", 132) == 264 and pl.default_pitch("y210", 132) == 528
    for w, want in zip(V210_WIDTHS, (128, 128, 128, 128, 128, 128, 128, 128, 256)):
        assert pl.default_pitch("v210", w) == want, w
        assert pl.frame_bytes("v210", w, 6) == 6 * want
    assert pl.default_pitch("v210", 1920) == 5120 and pl.frame_bytes("v210", 1920, 1080) == 5529600
    assert pl.frame_bytes("nv12", 132, 100) == 19800 and pl.frame_bytes("nv16", 132, 100) == 26400
    assert pl.frame_bytes("p010", 132, 100) == 39600 and pl.frame_bytes("uyvy", 132, 100) == 26400
    assert pl.frame_bytes("y216", 132, 100) == 52800
    # a 1920 x 1080 nv12 surface of pitch 2048 and 1088 luma rows: 2048 * (1088 + 539) + 1920
    assert pl.frame_bytes("nv12", 1920, 1080, 2048, 1088) == 3334016
    assert pl.frame_bytes("v210", 50, 2, 256 + 64) == 320 + 256
    for layout in lr.TABLE:
        for h, w in SIZES:
            assert pl.frame_bytes(layout, w, h) == lr.geometry(layout, h, w)[3]


def test_geometry_refusals_name_their_argument():
    import pmctf_layout as pl
    for bad in (131, (1 << 20) + 1, 1 << 21, 0, -132, True, 132.0):
        with pytest.raises(ValueError, match="pitch"):
            pl.frame_bytes("nv12", 132, 100, pitch=bad)
    for layout, bad in (("p010", 265), ("p010", 262), ("v210", 130), ("v210", 124), ("v210", 64), ("yuyv", 263)):
        with pytest.raises(ValueError, match="pitch"):
            pl.Unpacker(layout, 132 if layout != "v210" else 48, 100, pitch=bad)
    for bad in (99, 0, (1 << 17) + 1, 100.0):
        with pytest.raises(ValueError, match="luma_rows"):
            pl.frame_bytes("nv12", 132, 100, luma_rows=bad)
    assert pl.frame_bytes("nv12", 132, 100, 1 << 20, 1 << 17) > 1 << 36
    with pytest.raises(ValueError, match="pixel_layout"):
        pl.frame_bytes("nv24", 132, 100)
    with pytest.raises(ValueError, match="sides"):
        pl.frame_bytes("nv12", 131, 100)


class _NoCodec:
    pass


def _refused(match, tmp_path, name="src.raw", size=19800 * 8, entry="encode_sequence", **kw):
    import pmctf_layout as pl
    src = str(tmp_path / name)
    with open(src, "wb") as f:
        f.truncate(size)
    args = {"encode_sequence": (132, 100, 8, 4, 3), "encode_sequence_gops": (132, 100, 8, 4, 3),
            "encode_sequence_rate": (132, 100, 8, 4, 60000, kw.pop("fps", (30, 1)))}[entry]
    with pytest.raises(ValueError, match=match):
        getattr(pl, entry)(_NoCodec(), src, *args, str(tmp_path / "bins"), "cpu", **kw)
    assert not os.path.exists(tmp_path / "bins")


def test_encoder_refusals_name_their_argument(tmp_path):
    for entry in ("encode_sequence", "encode_sequence_gops", "encode_sequence_rate"):
        _refused("pixel_layout", tmp_path, entry=entry, pixel_layout="nv24")
        _refused("pixel_layout.*y4m", tmp_path, name="src.y4m", entry=entry, pixel_layout="nv12")
        _refused("src_format", tmp_path, entry=entry, pixel_layout="nv12", src_format="png")
        _refused("bitdepth 8", tmp_path, entry=entry, pixel_layout="p010", bitdepth=8)
        _refused("chroma_format '422'", tmp_path, entry=entry, pixel_layout="nv12", chroma_format="422")
        _refused("chroma_loc", tmp_path, entry=entry, pixel_layout="uyvy", chroma_loc="center")
        _refused("pitch", tmp_path, entry=entry, pixel_layout="nv12", pitch=130)
        _refused("luma_rows", tmp_path, entry=entry, pixel_layout="nv12", luma_rows=98)
        _refused("whole number", tmp_path, entry=entry, size=19800 * 8 - 1, pixel_layout="nv12")
        _refused("whole number", tmp_path, entry=entry, pixel_layout="nv12", pitch=136)
        _refused("pitch", tmp_path, entry=entry, pitch=132)                  # no layout to describe
        _refused("luma_rows", tmp_path, entry=entry, luma_rows=100)
    _refused("fps", tmp_path, entry="encode_sequence_rate", pixel_layout="nv12", fps=None)
    # everything in order: the refusal left is the missing GPU, and the depth was implied
    import pmctf_layout as pl
    src = str(tmp_path / "ok.p010")
    with open(src, "wb") as f:
        f.truncate(39600 * 8)
    with pytest.raises(RuntimeError, match="GPU"):
        pl.encode_sequence(_NoCodec(), src, 132, 100, 8, 4, 3, str(tmp_path / "bins"), "cpu", pixel_layout="p010")


def test_without_a_layout_the_pipeline_is_pmctf_chromas(tmp_path):
    import pmctf_chroma
    import pmctf_layout as pl
    src = str(tmp_path / "src.yuv")
    with open(src, "wb") as f:
        f.truncate(19800 * 8)
    none = pl._pipeline(src, 132, 100, "cpu", {}, None, None, None, None, None, None, "encode_sequence")
    assert none is None and pmctf_chroma._pipeline(src, 132, 100, "cpu", {}, None, None, None, "encode_sequence") is None
    # the state a pipeline holds, built directly (the device steps need a GPU): the layout is one more field, None without
    a = pmctf_chroma.SourcePipeline((132, 100), "422", "left")
    assert a.layout is None and a.planar
    b = pmctf_chroma.SourcePipeline((132, 100), "420", "center", layout=pl.Unpacker("nv12", 132, 100))
    assert not b.planar and b.write_header(str(tmp_path)) == [] and os.listdir(tmp_path) == ["src.yuv"]
    reader = b.open_reader(src, 132, 100)
    assert isinstance(reader, pl.PackedReader) and len(reader) == 8 and reader.unpack is b.layout
    for name in ("encode_sequence", "encode_sequence_gops", "encode_sequence_rate"):
        ours, theirs = (list(inspect.signature(getattr(m, name)).parameters) for m in (pl, pmctf_chroma))
        assert [p for p in ours if p not in ("pixel_layout", "pitch", "luma_rows")] == theirs
    for name in ("decode_sequence_checked", "decode_sequence_layer"):
        ours, theirs = (list(inspect.signature(getattr(m, name)).parameters) for m in (pl, pmctf_chroma))
        assert ours == theirs + ["output_layout"]


def test_decoder_refusals():
    import pmctf_layout as pl

    class Sink:
        shape, chroma_format = (100, 132), "422"

    with pytest.raises(ValueError, match="output_layout.*y4m"):
        pl.PackedSink(Sink(), "uyvy", "out.y4m", 8)
    with pytest.raises(ValueError, match="output_layout 'nv12'.*420.*8 bits.*422 of 8 bits"):
        pl.PackedSink(Sink(), "nv12", "out.raw", 8)
    with pytest.raises(ValueError, match="output_layout 'v210'.*10 bits.*422 of 8 bits"):
        pl.PackedSink(Sink(), "v210", "out.raw", 8)
    with pytest.raises(ValueError, match="output_layout"):
        pl.PackedSink(Sink(), "nv24", "out.raw", 8)
    sink = pl.PackedSink(Sink(), "v210", "out.v210", 10)
    assert sink.shape == (100, 132) and sink.pack.frame_bytes == 100 * 384 and sink.stream_header == b""


def test_convert_file_refusals(tmp_path):
    import pmctf_layout as pl
    src = str(tmp_path / "a.raw")
    with open(src, "wb") as f:
        f.truncate(19800 * 2)
    for kw, match in ((dict(from_layout="planar", to_layout="planar"), "both"), (dict(from_layout="nv12", to_layout="p010"), "to_layout"),
                      (dict(from_layout="nv24", to_layout="planar"), "from_layout"), (dict(from_layout="nv12", to_layout="nv42"), "to_layout"),
                      (dict(from_layout="nv16", to_layout="planar"), "whole number"),
                      (dict(from_layout="planar", to_layout="nv12", pitch=256), "pitch")):
        with pytest.raises(ValueError, match=match):
            pl.convert_file(src, str(tmp_path / "b.raw"), 132, 100, device="cpu", **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        pl.convert_file(src, str(tmp_path / "b.raw"), 132, 100, "nv12", "nv21", "cpu")
    assert not os.path.exists(tmp_path / "b.raw")


# ------------------------------------------------------------------------------------------------------------ readers
def test_packed_reader(tmp_path):
    import pmctf_layout as pl
    unpack = pl.Unpacker("v210", 10, 2)
    assert (unpack.frame_bytes, unpack.pitch, unpack.shape, unpack.bitdepth, unpack.chroma_format) == (256, 128, (2, 10), 10, "422")
    data = np.random.default_rng(0).integers(0, 256, 256 * 3 + 100, dtype=np.uint8)
    src = str(tmp_path / "a.v210")
    data.tofile(src)
    r = pl.PackedReader(src, unpack)
    assert len(r) == 3 and r.truncated and r.bitdepth == 10 and (r.width, r.height) == (10, 2)
    for k in range(3):
        got = r.read_one_frame()
        assert got.dtype == np.uint8 and np.array_equal(got, data[256 * k:256 * (k + 1)])
    with pytest.raises(AssertionError, match="ends inside a picture"):
        r.read_one_frame()
    r.close()
    assert np.array_equal(r.read_one_frame(), data[:256])
    r.close()
    data[:768].tofile(src)
    assert not pl.PackedReader(src, unpack).truncated
    with pytest.raises(AssertionError, match="no such sequence"):
        pl.PackedReader(str(tmp_path / "none"), unpack)


def test_surface_reader_without_a_device():
    import pmctf_layout as pl
    frames = [object(), object()]
    r = pl.SurfaceReader(frames, "nv12", 64, 2, pitch=65536, luma_rows=70000)
    assert len(r) == 2 and r.bitdepth == 8 and r.unpack.frame_bytes == 65536 * 70000 + 64
    assert r.read_one_frame() is frames[0] and r.read_one_frame() is frames[1] and r.read_one_frame() is None and r.eof
    r.close()
    assert r.read_one_frame() is frames[0]
    with pytest.raises(ValueError, match="pitch"):
        pl.SurfaceReader(frames, "nv12", 64, 2, pitch=63)


# ------------------------------------------------------------------------------------------------------- the C entries
ENTRIES = ("pmctf_unpack_layout_u8", "pmctf_unpack_layout_u16", "pmctf_pack_layout_u8", "pmctf_pack_layout_u16")


def test_the_four_symbols_are_declared_and_exported():
    from pMCTF.hip import lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pmctf_hip.h")).read(), flags=re.S)
    H = C.CDLL(lib.HIP_SO)
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", header) and name in lib.exported_symbols() and hasattr(H, name)


def test_the_entries_refuse_bad_arguments_before_any_launch():
    from pMCTF.hip import lib
    L = lib.hip()
    A, B = 0x10000, 0x20000                             # made-up pointers: nothing may be launched

    def call(kind, wide, layout, h=100, w=132, depth=10, pitch=None, luma_rows=None, a=A, b=B):
        names = {1: "nv12", 2: "nv21", 3: "nv16", 4: "p010", 6: "p016", 10: "yuyv", 11: "uyvy", 12: "y210", 15: "v210"}
        if pitch is None:
            pitch = lr.row_bytes(names.get(layout, "nv12"), max(w, 2)) if layout in names else 4 * w
        rows = h if luma_rows is None else luma_rows
        fn = getattr(L, f"pmctf_{kind}_layout_{'u16' if wide else 'u8'}")
        return fn(a, b, layout, h, w, depth, pitch, rows, None) if wide else fn(a, b, layout, h, w, pitch, rows, None)

    for kind in ("unpack", "pack"):
        for wide, layout in ((0, 1), (0, 11), (1, 4), (1, 12), (1, 15)):
            assert call(kind, wide, layout, a=None) == -1 and call(kind, wide, layout, b=None) == -1
            for h, w in ((99, 132), (100, 131), (0, 132), (100, -2), (16386, 132), (100, 16386)):
                assert call(kind, wide, layout, h=h, w=w, pitch=1 << 19) == -1
            assert call(kind, wide, layout, luma_rows=98) == -1 and call(kind, wide, layout, luma_rows=(1 << 17) + 1) == -1
            assert call(kind, wide, layout, pitch=(1 << 20) + 4) == -1 and call(kind, wide, layout, pitch=0) == -1
            assert call(kind, wide, layout, pitch=-528) == -1
            row = lr.row_bytes({1: "nv12", 11: "uyvy", 4: "p010", 12: "y210", 15: "v210"}[layout], 132)
            assert call(kind, wide, layout, pitch=row - (4 if layout == 15 else 2)) == -1      # below the row's bytes
        for layout in (0, 16, -1, 420):
            assert call(kind, 0, layout) == -1 and call(kind, 1, layout) == -1
        for layout in (4, 6, 12, 15):                                    # a layout of the other sample width
            assert call(kind, 0, layout) == -1
        for layout in (1, 2, 3, 10, 11):
            assert call(kind, 1, layout, depth=8) == -1 and call(kind, 1, layout, depth=10) == -1
        assert call(kind, 1, 4, depth=12) == -1 and call(kind, 1, 6, depth=10) == -1 and call(kind, 1, 15, depth=12) == -1
        assert call(kind, 1, 4, pitch=265) == -1 and call(kind, 1, 15, pitch=386) == -1        # no multiple of the container
        # a pointer not aligned to its container: the surface is the first argument of unpack, the second of pack
        odd = dict(a=A + 1) if kind == "unpack" else dict(b=B + 1)
        two = dict(a=A + 2) if kind == "unpack" else dict(b=B + 2)
        assert call(kind, 1, 4, **odd) == -1 and call(kind, 1, 15, **odd) == -1 and call(kind, 1, 15, **two) == -1
        planar_odd = dict(b=B + 1) if kind == "unpack" else dict(a=A + 1)
        assert call(kind, 1, 4, **planar_odd) == -1 and call(kind, 1, 15, **planar_odd) == -1


def test_the_bindings_refuse_host_tensors_and_bad_shapes():
    import torch
    from pMCTF.hip import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.unpack_layout(torch.zeros(19800, dtype=torch.uint8), "nv12", 100, 132)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pack_layout(torch.zeros(19800, dtype=torch.uint8), "nv12", 100, 132)
    with pytest.raises(ValueError, match="19799 bytes"):
        ops.unpack_layout(torch.zeros(19799, dtype=torch.uint8), "nv12", 100, 132)
    with pytest.raises(ValueError, match="uint16"):
        ops.pack_layout(torch.zeros(19800, dtype=torch.uint8), "p010", 100, 132)
    with pytest.raises(ValueError, match="bitdepth 8"):
        ops.unpack_layout(torch.zeros(39600, dtype=torch.uint8), "p010", 100, 132, bitdepth=8)


# ----------------------------------------------------------------------------------------------------- the command lines
def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("extra,message", [
    (["--pixel-layout", "nv24"], "--pixel-layout"), (["--pitch", "256"], "--pitch: only with --pixel-layout"),
    (["--luma-rows", "104"], "--luma-rows: only with --pixel-layout"), (["--pixel-layout", "p010", "--bitdepth", "8"], "--bitdepth 8"),
    (["--pixel-layout", "nv12", "--chroma-format", "422"], "--chroma-format 422"), (["--pixel-layout", "nv12", "--pitch", "130"], "pitch"),
    (["--pixel-layout", "nv12", "--luma-rows", "98"], "luma_rows"), (["--pixel-layout", "uyvy", "--chroma-loc", "center"], "--chroma-loc"),
    (["--pixel-layout", "nv16"], "whole number"), (["--pixel-layout", "nv12", "--pitch", "136"], "whole number"),
])
def test_encode_cli_parses_and_refuses(tmp_path, capsys, extra, message):
    src = str(tmp_path / "src.raw")
    with open(src, "wb") as f:
        f.truncate(19800 * 5)
    with pytest.raises(SystemExit) as e:
        _tool("encode_sequence").main(["--synth-seed", "0", "--gop", "4", "--width", "132", "--height", "100", *extra, src,
                                       str(tmp_path / "bins")])
    assert e.value.code == 2 and message in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "bins")


def test_encode_cli_refuses_a_layout_for_y4m_and_pngs(tmp_path, capsys):
    import chroma_restatement as cr
    src = str(tmp_path / "src.y4m")
    cr.write_y4m(src, [np.zeros(cr.samples(100, 132, "420"), np.uint8)] * 4, 132, 100, "420jpeg", rate=None)
    os.makedirs(tmp_path / "pngs")
    for source in (src, str(tmp_path / "pngs")):
        with pytest.raises(SystemExit) as e:
            _tool("encode_sequence").main(["--synth-seed", "0", "--pixel-layout", "nv12", source, str(tmp_path / "bins")])
        assert e.value.code == 2 and "--pixel-layout" in capsys.readouterr().err


@pytest.mark.parametrize("argv,message", [
    (["--output-layout", "nv24", "bins", "out.raw"], "--output-layout"), (["--output-layout", "nv12", "bins", "out.y4m"], "--output-layout"),
    (["--output-layout", "nv12", "--png", "dir", "bins"], "--output-layout"),
])
def test_decode_cli_parses_and_refuses(capsys, argv, message):
    with pytest.raises(SystemExit) as e:
        _tool("decode_sequence").main(["--synth-seed", "0", *argv])
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_convert_cli_parses_and_refuses(tmp_path, capsys):
    src = str(tmp_path / "a.raw")
    with open(src, "wb") as f:
        f.truncate(19800)
    for argv, message in ((["--from", "nv12", "--to", "p010"], "to_layout"), (["--from", "planar", "--to", "planar"], "both"),
                          (["--from", "v210", "--to", "planar"], "whole number"), (["--from", "nv12"], "--to")):
        with pytest.raises(SystemExit) as e:
            _tool("convert_layout").main(["--width", "132", "--height", "100", *argv, src, str(tmp_path / "b.raw")])
        assert e.value.code == 2 and message in capsys.readouterr().err
