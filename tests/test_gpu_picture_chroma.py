"""Chroma formats on the GPU: the kernel of csrc/picture_chroma.hip against tests/chroma_restatement.py, sample
for sample, and the drivers end to end on 132x100 sources of 8 pictures, GOP 4: .y4m files of 4:4:4, 4:2:2 (10 bit) and
4:2:0 in, .y4m and raw files out.  Everything is exact, byte for byte; there is no tolerance."""
import ctypes as C
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import chroma_restatement as cr
import scale_restatement as sr
from helpers import product_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64                                            # samples on either side of every output
# (fmt_in, fmt_out, chroma_loc)
CASES = [("444", "420", "center"), ("444", "420", "left"), ("422", "420", "left"), ("420", "444", "center"),
         ("420", "444", "left"), ("420", "422", "left"), ("444", "422", "left")]
# (h, w): chroma shrinks to one sample, every window clipped; Cr of the 4:2:0 picture starts on an odd byte; chroma 66 x 50:
# more than one 64-column and 16-row tile, ragged on both
SIZES = [(2, 2), (6, 10), (100, 132)]
DEPTHS = (8, 10, 16)
# (source offset, destination offset) in samples inside their buffers: every alignment of both, and every distance between
# them that the copy treats differently (a multiple of 16, 8, 4, 2 bytes, an odd one)
OFFSETS = [(0, 0), (1, 1), (2, 2), (3, 3), (0, 1), (1, 3), (2, 0), (3, 1), (0, 4), (0, 8)]


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _np_dtype(b):
    return np.uint8 if b == 8 else np.uint16


def _pictures(h, w, fmt, b, seed):
    """random with forced 0 / max samples, all max, and a 0 / max checkerboard (the filter's overshoot meets the clamp)"""
    top = (1 << b) - 1
    n = cr.samples(h, w, fmt)
    rng = np.random.default_rng(seed)
    rand = rng.integers(0, top + 1, n, dtype=np.uint16 if b > 8 else np.uint8).astype(_np_dtype(b))
    sat = rng.random(n)
    rand[sat < 0.1] = 0
    rand[sat > 0.9] = top
    rand[0], rand[1], rand[h * w], rand[-1] = 0, top, top, 0
    planes = [((np.add.outer(np.arange(r), np.arange(c)) & 1) * top).astype(_np_dtype(b)) for r, c in cr.plane_shapes(h, w, fmt)]
    return {"random": rand, "white": np.full(n, top, _np_dtype(b)), "checker": np.concatenate([p.reshape(-1) for p in planes])}


@functools.lru_cache(maxsize=None)
def _tables(h, w, fmt_in, fmt_out, loc):
    return [(start.astype("<i4").tobytes() + coef.astype("<i2").tobytes(), taps)
            for start, coef, taps in cr.axis_tables(h, w, fmt_in, fmt_out, loc)]


# ------------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("b", DEPTHS)
@pytest.mark.parametrize("fmt_in,fmt_out,loc", CASES)
def test_kernel_equals_the_restatement(cuda, fmt_in, fmt_out, loc, b):
    """the tables come from the restatement here (the product's are pinned to them in the CPU suite and used in the last
    assertion); luma must be the source's, the guards round the destination must survive"""
    import pmctf_chroma
    from pMCTF.hip import lib
    L = lib.hip()
    fn = L.pmctf_convert_chroma_u8 if b == 8 else L.pmctf_convert_chroma_u16
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    top = (1 << b) - 1
    fill = 0xA5 if b == 8 else 0xA5A5
    for h, w in SIZES:
        n_out = cr.samples(h, w, fmt_out)
        raw = _tables(h, w, fmt_in, fmt_out, loc)
        tabs = [torch.frombuffer(bytearray(r), dtype=torch.uint8).to(cuda) for r, _ in raw]
        ctaps = (C.c_int * 2)(*(t for _, t in raw))
        pictures = _pictures(h, w, fmt_in, b, seed=h * 1000 + w + b)
        for name, frame in pictures.items():
            want = cr.convert(frame, h, w, fmt_in, fmt_out, b, loc)
            assert np.array_equal(want[:h * w], frame[:h * w])
            if name == "white":
                assert (want == top).all()
            for off, doff in OFFSETS:
                src = torch.from_numpy(np.concatenate([np.zeros(off, frame.dtype), frame])).to(cuda)[off:]
                buf = torch.from_numpy(np.full(n_out + 2 * GUARD + doff, fill, _np_dtype(b))).to(cuda)
                dst = buf[GUARD + doff:GUARD + doff + n_out]
                assert src.data_ptr() % 8 == off * src.element_size() and buf.data_ptr() % 16 == 0
                rc = fn(_ptr(src), _ptr(dst), h, w, int(fmt_in), int(fmt_out), *(_ptr(t) for t in tabs), ctaps, b, stream)
                assert rc == 0
                host = buf.cpu().numpy()
                got = host[GUARD + doff:GUARD + doff + n_out]
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, (h, w, name, off, doff, bad[:5], got[bad[:5]], want[bad[:5]])
                assert np.array_equal(got[:h * w], frame[:h * w]), "luma is the source's"
                assert (host[:GUARD + doff] == fill).all() and (host[GUARD + doff + n_out:] == fill).all(), (h, w, name, off)
        # the product's own tables through the Converter
        conv = pmctf_chroma.Converter(w, h, fmt_in, fmt_out, cuda, b, loc)
        got = conv(torch.from_numpy(pictures["random"]).to(cuda)).cpu().numpy()
        assert np.array_equal(got, cr.convert(pictures["random"], h, w, fmt_in, fmt_out, b, loc))


def test_the_same_format_is_a_copy_and_refusals_leave_the_destination_untouched(cuda):
    import pmctf_chroma
    from pMCTF.hip import lib
    L = lib.hip()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for fmt in ("420", "422", "444"):
        frame = _pictures(100, 132, fmt, 10, 5)["random"]
        got = pmctf_chroma.Converter(132, 100, fmt, fmt, cuda, 10, "left")(torch.from_numpy(frame).to(cuda))
        assert np.array_equal(got.cpu().numpy(), frame)
    for b, fn in ((8, L.pmctf_convert_chroma_u8), (10, L.pmctf_convert_chroma_u16)):
        raw = _tables(36, 64, "444", "420", "center")
        tabs = [torch.frombuffer(bytearray(r), dtype=torch.uint8).to(cuda) for r, _ in raw]
        ctaps = (C.c_int * 2)(*(t for _, t in raw))
        src = torch.zeros(36 * 64 * 3, dtype=torch.uint8 if b == 8 else torch.uint16, device=cuda)
        fill = 0x5A if b == 8 else 0x5A5A
        dst = torch.from_numpy(np.full(36 * 64 * 3, fill, _np_dtype(b))).to(cuda)
        t = [_ptr(x) for x in tabs]
        calls = [(_ptr(src), _ptr(dst), 35, 64, 444, 420, *t, ctaps, b), (_ptr(src), _ptr(dst), 36, 63, 444, 420, *t, ctaps, b),
                 (_ptr(src), _ptr(dst), 36, 64, 400, 420, *t, ctaps, b), (_ptr(src), _ptr(dst), 36, 64, 444, 411, *t, ctaps, b),
                 (_ptr(src), _ptr(dst), 36, 64, 444, 420, *t, ctaps, 9 if b == 8 else 8),
                 (_ptr(src), _ptr(dst), 36, 64, 444, 420, *t, ctaps, 17), (None, _ptr(dst), 36, 64, 444, 420, *t, ctaps, b),
                 (_ptr(src), _ptr(dst), 36, 64, 444, 420, None, t[1], ctaps, b),
                 (_ptr(src), _ptr(dst), 36, 64, 444, 420, t[0], None, ctaps, b),
                 (_ptr(src), _ptr(dst), 36, 64, 444, 420, *t, None, b),
                 (_ptr(src), _ptr(dst), 36, 64, 444, 420, *t, (C.c_int * 2)(8, 18), b)]
        for k, args in enumerate(calls):
            assert fn(*args, stream) == -1, (b, k)
        assert fn(_ptr(src), None, 36, 64, 444, 420, *t, ctaps, b, stream) == -1
        torch.cuda.synchronize()
        assert bool((dst == fill).all())


# ------------------------------------------------------------------------------------------------------- 2. end to end
W, H, CW, CH, GOP, N, Q = 132, 100, 66, 50, 4, 8, 3


def _files(folder):
    out = {}
    for base, _, names in os.walk(folder):
        for n in names:
            p = os.path.join(base, n)
            out[os.path.relpath(p, folder)] = open(p, "rb").read()
    return out


def _raw_frames(path, n, b=8):
    data = np.fromfile(path, dtype=_np_dtype(b))
    assert data.size % n == 0
    return [data[i * n:(i + 1) * n] for i in range(data.size // n)]


def _write(path, frames):
    with open(path, "wb") as f:
        for fr in frames:
            f.write(fr.tobytes())


def _same_folder(new, plain, extra):
    fs, fp = _files(new), _files(plain)
    assert sorted(set(fs) - set(fp)) == sorted(extra) and set(fp) <= set(fs)
    for p in sorted(fp):
        assert fs[p] == fp[p], f"{p} differs from coding the converted pictures"


def _source(fmt, b=8):
    """N synthetic pictures of W x H in `fmt`, packed: luma of the 4:2:0 sequence, chroma planes of a sequence large enough
    to have them at this format's size; above 8 bits with random low bits"""
    import pmctf_synth
    sx, sy = cr.SUB[fmt]
    luma = pmctf_synth.synth_yuv420(W, H, N, seed=77)
    chroma = pmctf_synth.synth_yuv420(2 * W // sx, 2 * H // sy, N, seed=78)
    rng = np.random.default_rng(b)
    out = []
    for (y, _, _), (_, cb, cr_) in zip(luma, chroma):
        fr = np.concatenate([p.reshape(-1) for p in (y, cb, cr_)])
        if b > 8:
            fr = (fr.astype(np.uint16) << (b - 8)) + rng.integers(0, 1 << (b - 8), fr.size, dtype=np.uint16)
        out.append(fr)
    assert out[0].size == cr.samples(H, W, fmt)
    return out


@pytest.fixture(scope="module")
def seq(cuda, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("picture_chroma")
    out = {"tmp": tmp, "enc_net": product_model(1)[0], "dec_net": product_model(1)[0]}
    out["frames444"] = _source("444")
    out["src444"] = str(tmp / "src444.y4m")
    cr.write_y4m(out["src444"], out["frames444"], W, H, "444", rate=(30000, 1001))
    return out


def _bins(seq, name):
    p = str(seq["tmp"] / name)
    os.makedirs(p)
    return p


@pytest.fixture(scope="module")
def coded444(seq):
    """(a) the C444 .y4m coded with picture hashes, and the restatement's 4:2:0 .yuv of it coded without the feature"""
    import pmctf_chroma
    import pmctf_gop
    conv = str(seq["tmp"] / "conv444.yuv")
    _write(conv, [cr.convert(fr, H, W, "444", "420", 8, "center") for fr in seq["frames444"]])
    new, plain = _bins(seq, "new444"), _bins(seq, "plain444")
    r = pmctf_chroma.encode_sequence(seq["enc_net"], seq["src444"], W, H, N, GOP, Q, new, "cuda", keep_gops=True,
                                     picture_hash="u8")
    p = pmctf_gop.encode_sequence(seq["enc_net"], conv, W, H, N, GOP, Q, plain, "cuda", keep_gops=True, picture_hash="u8")
    return {"new": new, "plain": plain, "r": r, "p": p, "conv": conv}


def test_a_444_y4m_codes_to_the_files_of_its_converted_yuv(seq, coded444):
    import pmctf_chroma
    _same_folder(coded444["new"], coded444["plain"], ["source_format.json"])
    assert pmctf_chroma.read_source_format(coded444["new"]) == {
        "format_version": 1, "chroma_format": "444", "chroma_loc": "center", "filter": "catmull-rom-aa/14",
        "frame_rate": [30000, 1001]}
    for k in ("bits", "psnr", "frame_types"):
        assert coded444["r"][k] == coded444["p"][k]
    assert coded444["r"]["picture_hashes"] == coded444["p"]["picture_hashes"] and coded444["r"]["display_quality"] == []


def test_decode_to_the_source_format_and_to_y4m(seq, coded444):
    import pmctf_chroma
    import pmctf_gop
    plain, coded, out = (str(seq["tmp"] / n) for n in ("dec444_plain.yuv", "dec444_coded.yuv", "dec444_out.y4m"))
    pmctf_gop.decode_sequence(seq["dec_net"], coded444["plain"], plain, "cuda")
    a = pmctf_chroma.decode_sequence_checked(seq["dec_net"], coded444["new"], coded, "cuda", coded_format_output=True)
    b = pmctf_chroma.decode_sequence_checked(seq["dec_net"], coded444["new"], out, "cuda")
    assert a["verified"] == b["verified"] == N and a["frames"] == b["frames"] == [(H, W)] * N
    assert open(coded, "rb").read() == open(plain, "rb").read()
    assert pmctf_gop.check_yuv_hashes(coded444["new"], coded) == (N, [])
    assert open(out, "rb").read().startswith(b"YUV4MPEG2 W132 H100 F30000:1001 Ip A0:0 C444\nFRAME\n")
    info, got = cr.read_y4m(out)
    want = [cr.convert(fr, H, W, "420", "444", 8, "center") for fr in _raw_frames(plain, cr.samples(H, W, "420"))]
    assert len(got) == N and all(np.array_equal(g, w) for g, w in zip(got, want))
    # the old entry point honours the header too; a raw path gets the same planes without the markers
    raw = str(seq["tmp"] / "dec444_out.yuv")
    pmctf_gop.decode_sequence(seq["dec_net"], coded444["new"], raw, "cuda")
    assert open(raw, "rb").read() == b"".join(w.tobytes() for w in want)
    # a .y4m of the coded 4:2:0 pictures
    y420 = str(seq["tmp"] / "dec444_coded.y4m")
    pmctf_chroma.decode_sequence_checked(seq["dec_net"], coded444["new"], y420, "cuda", coded_format_output=True)
    info, got = cr.read_y4m(y420)
    assert info["C"] == "420jpeg" and b"".join(g.tobytes() for g in got) == open(plain, "rb").read()
    # PNGs keep coming from the 4:2:0 pictures
    png_new, png_plain = str(seq["tmp"] / "png_new"), str(seq["tmp"] / "png_plain")
    pmctf_chroma.decode_sequence_checked(seq["dec_net"], coded444["new"], None, "cuda", png_out=png_new)
    pmctf_gop.decode_sequence(seq["dec_net"], coded444["plain"], None, "cuda", png_out=png_plain)
    assert _files(png_new) == _files(png_plain) and len(_files(png_new)) == N


def test_a_422_ten_bit_y4m_left_siting(seq):
    import pmctf_chroma
    import pmctf_gop
    b = 10
    frames = _source("422", b)
    src, conv = str(seq["tmp"] / "src422.y4m"), str(seq["tmp"] / "conv422.yuv")
    cr.write_y4m(src, frames, W, H, "422p10", rate=None)
    _write(conv, [cr.convert(fr, H, W, "422", "420", b, "left") for fr in frames])
    new, plain = _bins(seq, "new422"), _bins(seq, "plain422")
    pmctf_chroma.encode_sequence(seq["enc_net"], src, W, H, N, GOP, Q, new, "cuda", keep_gops=True, bitdepth=b,
                                 picture_hash="u16", chroma_loc="left")
    pmctf_gop.encode_sequence(seq["enc_net"], conv, W, H, N, GOP, Q, plain, "cuda", keep_gops=True, bitdepth=b,
                              picture_hash="u16")
    _same_folder(new, plain, ["source_format.json"])
    assert pmctf_chroma.read_source_format(new) == {"format_version": 1, "chroma_format": "422", "chroma_loc": "left",
                                                    "filter": "catmull-rom-aa/14", "frame_rate": None}
    dec_plain, coded, out = (str(seq["tmp"] / n) for n in ("dec422_plain.yuv", "dec422_coded.yuv", "dec422_out.y4m"))
    pmctf_gop.decode_sequence(seq["dec_net"], plain, dec_plain, "cuda")
    pmctf_chroma.decode_sequence_checked(seq["dec_net"], new, coded, "cuda", coded_format_output=True)
    d = pmctf_chroma.decode_sequence_checked(seq["dec_net"], new, out, "cuda")
    assert d["bitdepth"] == b and d["verified"] == N
    assert open(coded, "rb").read() == open(dec_plain, "rb").read()
    assert open(out, "rb").read().startswith(b"YUV4MPEG2 W132 H100 F25:1 Ip A0:0 C422p10\nFRAME\n")
    _, got = cr.read_y4m(out)
    want = [cr.convert(fr, H, W, "420", "422", b, "left") for fr in _raw_frames(dec_plain, cr.samples(H, W, "420"), b)]
    assert len(got) == N and all(np.array_equal(g, w) for g, w in zip(got, want))


def test_a_420mpeg2_y4m_is_its_payload_and_gives_the_frame_rate(seq, capsys):
    import pmctf_chroma
    import pmctf_gop
    import pmctf_rate
    import pmctf_synth
    pictures = pmctf_synth.synth_yuv420(W, H, N, seed=77)
    frames = [np.concatenate([p.reshape(-1) for p in pic]) for pic in pictures]
    src, raw = str(seq["tmp"] / "src420.y4m"), str(seq["tmp"] / "src420.yuv")
    cr.write_y4m(src, frames, W, H, "420mpeg2", rate=(30, 1), frame_params="Ip")
    pmctf_gop.write_yuv(raw, pictures)
    new, plain = _bins(seq, "new420"), _bins(seq, "plain420")
    pmctf_chroma.encode_sequence(seq["enc_net"], src, W, H, N, GOP, Q, new, "cuda", keep_gops=True)
    pmctf_gop.encode_sequence(seq["enc_net"], raw, W, H, N, GOP, Q, plain, "cuda", keep_gops=True)
    _same_folder(new, plain, ["source_format.json"])
    assert pmctf_chroma.read_source_format(new) == {"format_version": 1, "chroma_format": "420", "chroma_loc": "left",
                                                    "filter": "catmull-rom-aa/14", "frame_rate": [30, 1]}
    out = str(seq["tmp"] / "dec420.y4m")
    pmctf_chroma.decode_sequence_checked(seq["dec_net"], new, out, "cuda")
    assert open(out, "rb").read().startswith(b"YUV4MPEG2 W132 H100 F30:1 Ip A0:0 C420mpeg2\nFRAME\n")
    # a bitrate without a frame rate: the header's, through the entry point and through the command line
    kw = dict(structure="fill", q_choices=range(0, 21, 5), max_trials=2)
    rate_new, rate_plain = _bins(seq, "rate_new"), _bins(seq, "rate_plain")
    r = pmctf_chroma.encode_sequence_rate(seq["enc_net"], src, W, H, GOP, GOP, 60000, None, rate_new, "cuda", **kw)
    p = pmctf_rate.encode_sequence_rate(seq["enc_net"], raw, W, H, GOP, GOP, 60000, (30, 1), rate_plain, "cuda", **kw)
    assert r["gops"] == p["gops"]
    _same_folder(rate_new, rate_plain, ["source_format.json"])
    assert json.load(open(os.path.join(rate_new, "rate_control.json")))["fps"] == [30, 1]
    spec = importlib.util.spec_from_file_location("encode_sequence", os.path.join(ROOT, "tools", "encode_sequence.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    cli = str(seq["tmp"] / "rate_cli")
    tool.main(["--synth-seed", "0", "--gop", str(GOP), "--frames", str(GOP), "--bitrate", "60000", "--max-trials", "2", src, cli])
    capsys.readouterr()
    record = json.load(open(os.path.join(cli, "rate_control.json")))
    assert record["fps"] == [30, 1] and pmctf_rate.verify_rate_record(cli)["header"]["width"] == W
    assert pmctf_chroma.read_source_format(cli)["frame_rate"] == [30, 1]


def test_a_444_source_at_a_coded_size(seq):
    """(e) format first, size second"""
    import pmctf_chroma
    import pmctf_gop
    import pmctf_scale
    small = str(seq["tmp"] / "conv444_small.yuv")
    _write(small, [sr.resize_yuv420(cr.convert(fr, H, W, "444", "420", 8, "center"), H, W, CH, CW, 8, "center")
                   for fr in seq["frames444"]])
    new, plain = _bins(seq, "new444s"), _bins(seq, "plain444s")
    r = pmctf_chroma.encode_sequence(seq["enc_net"], seq["src444"], W, H, N, GOP, Q, new, "cuda", keep_gops=True,
                                     coded_size=(CW, CH))
    pmctf_gop.encode_sequence(seq["enc_net"], small, CW, CH, N, GOP, Q, plain, "cuda", keep_gops=True)
    _same_folder(new, plain, ["display_format.json", "source_format.json"])
    assert pmctf_scale.read_display_format(new, CW, CH)["width"] == W and len(r["display_quality"]) == N
    dec_plain, out = str(seq["tmp"] / "dec444s_plain.yuv"), str(seq["tmp"] / "dec444s_out.y4m")
    pmctf_gop.decode_sequence(seq["dec_net"], plain, dec_plain, "cuda")
    d = pmctf_chroma.decode_sequence_checked(seq["dec_net"], new, out, "cuda")
    assert d["frames"] == [(H, W)] * N
    info, got = cr.read_y4m(out)
    want = [cr.convert(sr.resize_yuv420(fr, CH, CW, H, W, 8, "center"), H, W, "420", "444", 8, "center")
            for fr in _raw_frames(dec_plain, cr.samples(CH, CW, "420"))]
    assert (info["W"], info["H"], info["C"]) == ("132", "100", "444")
    assert len(got) == N and all(np.array_equal(g, w) for g, w in zip(got, want))
    # both headers ignored: the coded pictures
    coded = str(seq["tmp"] / "dec444s_coded.yuv")
    pmctf_chroma.decode_sequence_checked(seq["dec_net"], new, coded, "cuda", coded_size_output=True, coded_format_output=True)
    assert open(coded, "rb").read() == open(dec_plain, "rb").read()


def test_a_raw_420_source_goes_the_old_way(seq, coded444):
    """(f) the new entry points with nothing new asked for: pmctf_scale's folder, listing and bytes"""
    import pmctf_chroma
    import pmctf_scale
    new, old = _bins(seq, "raw_new"), _bins(seq, "raw_old")
    r = pmctf_chroma.encode_sequence(seq["enc_net"], coded444["conv"], W, H, N, GOP, Q, new, "cuda", keep_gops=True,
                                     picture_hash="u8")
    pmctf_scale.encode_sequence(seq["enc_net"], coded444["conv"], W, H, N, GOP, Q, old, "cuda", keep_gops=True,
                                picture_hash="u8")
    assert _files(new) == _files(old) == _files(coded444["plain"]) and "display_quality" not in r
    assert sorted(os.listdir(new)) == ["gop_00000", "gop_00001", "picture_hashes.json", "sequence.json"]
    outs = [str(seq["tmp"] / f"raw_{k}.yuv") for k in range(3)]
    pmctf_scale.decode_sequence_checked(seq["dec_net"], new, outs[0], "cuda")
    pmctf_chroma.decode_sequence_checked(seq["dec_net"], new, outs[1], "cuda")
    pmctf_chroma.decode_sequence_checked(seq["dec_net"], new, outs[2], "cuda", coded_format_output=True)
    data = [open(p, "rb").read() for p in outs]
    assert data[0] == data[1] == data[2] and len(data[0]) == N * W * H * 3 // 2


def test_an_extracted_layer_keeps_the_header(seq, coded444):
    import pmctf_chroma
    import pmctf_layers
    small = str(seq["tmp"] / "level1")
    written = pmctf_layers.extract_layer(coded444["new"], small, 1)
    assert "source_format.json" in written
    assert open(os.path.join(small, "source_format.json"), "rb").read() == \
        open(os.path.join(coded444["new"], "source_format.json"), "rb").read()
    out, coded = str(seq["tmp"] / "level1.y4m"), str(seq["tmp"] / "level1_coded.yuv")
    d = pmctf_chroma.decode_sequence_layer(seq["dec_net"], small, out, 1, "cuda")
    c = pmctf_chroma.decode_sequence_layer(seq["dec_net"], small, coded, 1, "cuda", coded_format_output=True)
    assert d["times"] == c["times"] == [0, 2, 4, 6]
    info, got = cr.read_y4m(out)
    want = [cr.convert(fr, H, W, "420", "444", 8, "center") for fr in _raw_frames(coded, cr.samples(H, W, "420"))]
    assert info["C"] == "444" and len(got) == 4 and all(np.array_equal(g, w) for g, w in zip(got, want))
