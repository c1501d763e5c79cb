"""Reduced-resolution coding on the GPU: the kernel of csrc/picture_scale.hip against tests/scale_restatement.py, bit for
bit, its refusals, and the drivers end to end on a 132x100 source of 8 frames coded at 66x50, GOP 4.

Everything is exact, byte for byte; the one tolerance is 1e-9 dB on a PSNR against its own formula (float64 log10)."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

import scale_restatement as sr
from helpers import product_model

pytestmark = pytest.mark.gpu

GUARD = 64                                            # samples on either side of every output
# (h_in, w_in, h_out, w_out): identity; 2:1; non-integer down; up; down in x and up in y; the two limits (the second has
# 3x5 chroma planes, Cr on an odd boundary); more than one tile with ragged edges on both axes
SHAPES = [(18, 34, 18, 34), (36, 64, 18, 32), (36, 64, 24, 44), (34, 50, 100, 132), (20, 96, 40, 24), (64, 64, 16, 16),
          (6, 10, 24, 40), (130, 258, 66, 130)]
DEPTHS = (8, 10, 16)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _np_dtype(b):
    return np.uint8 if b == 8 else np.uint16


def _pictures(h, w, b, seed):
    """random with forced 0 / max samples, all max, and a 0 / max checkerboard (the filter's overshoot meets the clamp)"""
    top = (1 << b) - 1
    n = h * w * 3 // 2
    rng = np.random.default_rng(seed)
    rand = rng.integers(0, top + 1, n, dtype=np.uint16 if b > 8 else np.uint8).astype(_np_dtype(b))
    sat = rng.random(n)
    rand[sat < 0.1] = 0
    rand[sat > 0.9] = top
    rand[0], rand[1], rand[h * w], rand[-1] = 0, top, top, 0
    white = np.full(n, top, _np_dtype(b))
    planes = [((np.add.outer(np.arange(r), np.arange(c)) & 1) * top).astype(_np_dtype(b)) for r, c in
              ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
    return {"random": rand, "white": white, "checker": np.concatenate([p.reshape(-1) for p in planes])}


@functools.lru_cache(maxsize=None)
def _tables(h_in, w_in, h_out, w_out, loc):
    px = sr.left_phase(w_in // 2, w_out // 2) if loc == "left" else 0
    out = []
    for n_in, n_out, phase in ((w_in, w_out, 0), (h_in, h_out, 0), (w_in // 2, w_out // 2, px), (h_in // 2, h_out // 2, 0)):
        start, coef, taps = sr.tables(n_in, n_out, phase)
        out.append((start.astype("<i4").tobytes() + coef.astype("<i2").tobytes(), taps))
    return out


def _device_tables(h_in, w_in, h_out, w_out, loc, dev):
    tabs = _tables(h_in, w_in, h_out, w_out, loc)
    return [torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev) for raw, _ in tabs], [t for _, t in tabs]


# ------------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("b", DEPTHS)
@pytest.mark.parametrize("h_in,w_in,h_out,w_out", SHAPES)
def test_kernel_equals_the_restatement(cuda, h_in, w_in, h_out, w_out, b):
    """both chroma sitings, every source byte alignment, guarded destinations at the same alignments; the tables come
    from the restatement here (the product's are pinned to them in the CPU suite and used in the last assertion)"""
    import pmctf_scale
    from pMCTF.hip import lib
    L = lib.hip()
    fn = L.pmctf_resize_yuv420_u8 if b == 8 else L.pmctf_resize_yuv420_u16
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tdt = torch.uint8 if b == 8 else torch.uint16
    top = (1 << b) - 1
    n_in, n_out = h_in * w_in * 3 // 2, h_out * w_out * 3 // 2
    fill = 0xA5 if b == 8 else 0xA5A5
    pictures = _pictures(h_in, w_in, b, seed=h_in * 1000 + w_out + b)
    for loc in ("center", "left"):
        tabs, taps = _device_tables(h_in, w_in, h_out, w_out, loc, cuda)
        ctaps = (C.c_int * 4)(*taps)
        for name, frame in pictures.items():
            want = sr.resize_yuv420(frame, h_in, w_in, h_out, w_out, b, loc)
            if name == "white":
                assert (want == top).all()
            if (h_in, w_in) == (h_out, w_out) and loc == "center":
                assert np.array_equal(want, frame), "identity"
            for off in range(4):                                     # samples at 8 bits: bytes 0..3; above: bytes 0, 2, 4, 6
                src = torch.from_numpy(np.concatenate([np.zeros(off, frame.dtype), frame])).to(cuda)[off:]
                buf = torch.from_numpy(np.full(n_out + 2 * GUARD + off, fill, _np_dtype(b))).to(cuda)
                dst = buf[GUARD + off:GUARD + off + n_out]
                assert src.data_ptr() % 8 == off * src.element_size() and src.dtype == tdt
                rc = fn(_ptr(src), _ptr(dst), h_in, w_in, h_out, w_out, *(_ptr(t) for t in tabs), ctaps, b, stream)
                assert rc == 0
                host = buf.cpu().numpy()
                got = host[GUARD + off:GUARD + off + n_out]
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, (loc, name, off, bad[:5], got[bad[:5]], want[bad[:5]])
                assert (host[:GUARD + off] == fill).all() and (host[GUARD + off + n_out:] == fill).all(), (loc, name, off)
        # the product's own tables through the Resampler
        r = pmctf_scale.Resampler(w_in, h_in, w_out, h_out, cuda, b, loc)
        got = r(torch.from_numpy(pictures["random"]).to(cuda)).cpu().numpy()
        assert np.array_equal(got, sr.resize_yuv420(pictures["random"], h_in, w_in, h_out, w_out, b, loc))


def test_rejected_arguments_leave_the_destination_untouched(cuda):
    from pMCTF.hip import lib
    L = lib.hip()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for b, fn in ((8, L.pmctf_resize_yuv420_u8), (10, L.pmctf_resize_yuv420_u16)):
        tabs, taps = _device_tables(36, 64, 18, 32, "center", cuda)
        ctaps = (C.c_int * 4)(*taps)
        src = torch.zeros(36 * 64 * 3 // 2, dtype=torch.uint8 if b == 8 else torch.uint16, device=cuda)
        fill = 0x5A if b == 8 else 0x5A5A
        dst = torch.from_numpy(np.full(64 * 64 * 3, fill, _np_dtype(b))).to(cuda)
        t = [_ptr(x) for x in tabs]
        calls = [(_ptr(src), _ptr(dst), 35, 64, 18, 32, *t, ctaps, b), (_ptr(src), _ptr(dst), 36, 64, 18, 31, *t, ctaps, b),
                 (_ptr(src), _ptr(dst), 36, 64, 8, 32, *t, ctaps, b), (_ptr(src), _ptr(dst), 36, 64, 18, 14, *t, ctaps, b),
                 (_ptr(src), _ptr(dst), 8, 64, 34, 32, *t, ctaps, b), (_ptr(src), _ptr(dst), 36, 12, 18, 50, *t, ctaps, b),
                 (_ptr(src), _ptr(dst), 36, 64, 18, 32, *t, ctaps, 9 if b == 8 else 8),
                 (_ptr(src), _ptr(dst), 36, 64, 18, 32, *t, ctaps, 17),
                 (None, _ptr(dst), 36, 64, 18, 32, *t, ctaps, b),
                 (_ptr(src), _ptr(dst), 36, 64, 18, 32, None, *t[1:], ctaps, b),
                 (_ptr(src), _ptr(dst), 36, 64, 18, 32, *t[:3], None, ctaps, b),
                 (_ptr(src), _ptr(dst), 36, 64, 18, 32, *t, None, b),
                 (_ptr(src), _ptr(dst), 36, 64, 18, 32, *t, (C.c_int * 4)(8, 8, 21, 8), b)]
        for k, args in enumerate(calls):
            assert fn(*args, stream) == -1, (b, k)
        assert fn(_ptr(src), None, 36, 64, 18, 32, *t, ctaps, b, stream) == -1
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


def _frames(path, w, h, b=8):
    data = np.fromfile(path, dtype=_np_dtype(b))
    n = w * h * 3 // 2
    assert data.size % n == 0
    return [data[i * n:(i + 1) * n] for i in range(data.size // n)]


def _write(path, frames):
    with open(path, "wb") as f:
        for fr in frames:
            f.write(fr.tobytes())


def _down(src_path, dst_path, b=8, loc="center"):
    _write(dst_path, [sr.resize_yuv420(fr, H, W, CH, CW, b, loc) for fr in _frames(src_path, W, H, b)])


def _same_folder(scaled, plain, extra=("display_format.json",)):
    fs, fp = _files(scaled), _files(plain)
    assert sorted(set(fs) - set(fp)) == sorted(extra) and set(fp) <= set(fs)
    for p in sorted(fp):
        assert fs[p] == fp[p], f"{p} differs from coding the resampled pictures"


@pytest.fixture(scope="module")
def seq(cuda, tmp_path_factory):
    import pmctf_gop
    import pmctf_synth
    tmp = tmp_path_factory.mktemp("picture_scale")
    out = {"tmp": tmp, "enc_net": product_model(1)[0], "dec_net": product_model(1)[0]}
    pictures = pmctf_synth.synth_yuv420(W, H, N, seed=77)
    out["src8"] = str(tmp / "src8.yuv")
    pmctf_gop.write_yuv(out["src8"], pictures)
    out["down8"] = str(tmp / "down8.yuv")
    _down(out["src8"], out["down8"])
    return out


def _bins(seq, name):
    p = str(seq["tmp"] / name)
    os.makedirs(p)
    return p


@pytest.fixture(scope="module")
def coded8(seq):
    """the 8-bit source coded at 66x50 with picture hashes, and the resampled .yuv coded without the feature"""
    import pmctf_gop
    import pmctf_scale
    scaled, plain = _bins(seq, "scaled8"), _bins(seq, "plain8")
    r = pmctf_scale.encode_sequence(seq["enc_net"], seq["src8"], W, H, N, GOP, Q, scaled, "cuda", keep_gops=True,
                                    picture_hash="u8", coded_size=(CW, CH))
    p = pmctf_gop.encode_sequence(seq["enc_net"], seq["down8"], CW, CH, N, GOP, Q, plain, "cuda", keep_gops=True,
                                  picture_hash="u8")
    return {"scaled": scaled, "plain": plain, "r": r, "p": p}


def test_files_are_those_of_the_resampled_source(seq, coded8):
    import pmctf_gop
    import pmctf_scale
    _same_folder(coded8["scaled"], coded8["plain"])
    assert pmctf_gop.read_sequence_header(coded8["scaled"])["width"] == CW
    assert pmctf_scale.read_display_format(coded8["scaled"], CW, CH) == {
        "format_version": 1, "width": W, "height": H, "filter": "catmull-rom-aa/14", "chroma_loc": "center"}
    for k in ("bits", "psnr", "frame_types"):
        assert coded8["r"][k] == coded8["p"][k]
    assert coded8["r"]["picture_hashes"] == coded8["p"]["picture_hashes"]


def test_decode_to_display_size_and_display_psnr(seq, coded8):
    import pmctf_gop
    import pmctf_scale
    small, big = str(seq["tmp"] / "dec8_coded.yuv"), str(seq["tmp"] / "dec8_display.yuv")
    a = pmctf_scale.decode_sequence_checked(seq["dec_net"], coded8["scaled"], small, "cuda", coded_size_output=True)
    b = pmctf_gop.decode_sequence(seq["dec_net"], coded8["scaled"], big, "cuda")
    assert a["frames"] == [(CH, CW)] * N and b["frames"] == [(H, W)] * N and a["verified"] == b["verified"] == N
    assert pmctf_gop.check_yuv_hashes(coded8["scaled"], small) == (N, [])
    plain = str(seq["tmp"] / "dec8_plain.yuv")
    pmctf_gop.decode_sequence(seq["dec_net"], coded8["plain"], plain, "cuda")
    assert open(plain, "rb").read() == open(small, "rb").read()
    want = [sr.resize_yuv420(fr, CH, CW, H, W, 8) for fr in _frames(small, CW, CH)]
    got = _frames(big, W, H)
    assert len(got) == N and all(np.array_equal(g, w) for g, w in zip(got, want))
    # (c) display PSNR: its formula on those pictures
    src = _frames(seq["src8"], W, H)
    assert len(coded8["r"]["display_quality"]) == N
    for q, rec, org in zip(coded8["r"]["display_quality"], want, src):
        psnr = []
        for pr, po in zip(sr.split(rec, H, W), sr.split(org, H, W)):
            d = pr.astype(np.int64) - po.astype(np.int64)
            sse = int((d * d).sum())
            psnr.append(math.inf if sse == 0 else 10.0 * math.log10(255.0 ** 2 * d.size / sse))
        expect = dict(zip(("y", "cb", "cr"), psnr), yuv=(6.0 * psnr[0] + psnr[1] + psnr[2]) / 8.0)
        assert sorted(q) == ["display_psnr_cb", "display_psnr_cr", "display_psnr_y", "display_psnr_yuv"]
        for k, v in expect.items():
            assert abs(q["display_psnr_" + k] - v) <= 1e-9, (k, q, v)
    # PNGs come at the display size too
    png = str(seq["tmp"] / "dec8_png")
    pmctf_gop.decode_sequence(seq["dec_net"], coded8["scaled"], None, "cuda", png_out=png)
    from PIL import Image
    assert sorted(os.listdir(png), key=lambda n: int(n[:-4])) == [f"{i}.png" for i in range(N)]
    assert Image.open(os.path.join(png, "0.png")).size == (W, H)


def test_ten_bit_and_left_siting(seq):
    import pmctf_gop
    import pmctf_scale
    b = 10
    rng = np.random.default_rng(10)
    src, down = str(seq["tmp"] / "src10.yuv"), str(seq["tmp"] / "down10.yuv")
    _write(src, [(fr.astype(np.uint16) << 2) + rng.integers(0, 4, fr.size, dtype=np.uint16)
                 for fr in _frames(seq["src8"], W, H)])
    _down(src, down, b, "left")
    scaled, plain = _bins(seq, "scaled10"), _bins(seq, "plain10")
    pmctf_scale.encode_sequence(seq["enc_net"], src, W, H, N, GOP, Q, scaled, "cuda", keep_gops=True, bitdepth=b,
                                picture_hash="u16", coded_size=(CW, CH), chroma_loc="left")
    pmctf_gop.encode_sequence(seq["enc_net"], down, CW, CH, N, GOP, Q, plain, "cuda", keep_gops=True, bitdepth=b,
                              picture_hash="u16")
    _same_folder(scaled, plain)
    assert pmctf_scale.read_display_format(scaled)["chroma_loc"] == "left"
    small, big = str(seq["tmp"] / "dec10_coded.yuv"), str(seq["tmp"] / "dec10_display.yuv")
    pmctf_scale.decode_sequence_checked(seq["dec_net"], scaled, small, "cuda", coded_size_output=True)
    d = pmctf_gop.decode_sequence(seq["dec_net"], scaled, big, "cuda")
    assert d["bitdepth"] == b and d["verified"] == N and d["frames"] == [(H, W)] * N
    want = [sr.resize_yuv420(fr, CH, CW, H, W, b, "left") for fr in _frames(small, CW, CH, b)]
    got = _frames(big, W, H, b)
    assert len(got) == N and all(np.array_equal(g, w) for g, w in zip(got, want))


def test_png_sources(seq, cuda):
    import pmctf_gop
    import pmctf_scale
    from PIL import Image
    pngs = str(seq["tmp"] / "src_png")
    os.makedirs(pngs)
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, (H // 4, W // 4, 3), dtype=np.uint8).repeat(4, axis=0).repeat(4, axis=1)
    for i in range(GOP):
        Image.fromarray(np.roll(base, 2 * i, axis=1)).save(os.path.join(pngs, f"{i}.png"))
    full, down = str(seq["tmp"] / "png_full.yuv"), str(seq["tmp"] / "png_down.yuv")
    assert pmctf_gop.pngs_to_yuv(pngs, full, cuda) == (W, H, GOP)
    _down(full, down)
    scaled, plain = _bins(seq, "scaled_png"), _bins(seq, "plain_png")
    pmctf_scale.encode_sequence(seq["enc_net"], pngs, W, H, GOP, GOP, Q, scaled, "cuda", keep_gops=True, src_format="png",
                                coded_size=(CW, CH))
    pmctf_gop.encode_sequence(seq["enc_net"], down, CW, CH, GOP, GOP, Q, plain, "cuda", keep_gops=True)
    _same_folder(scaled, plain)
    small, big = str(seq["tmp"] / "decpng_coded.yuv"), str(seq["tmp"] / "decpng_display.yuv")
    pmctf_scale.decode_sequence_checked(seq["dec_net"], scaled, small, "cuda", coded_size_output=True)
    pmctf_gop.decode_sequence(seq["dec_net"], scaled, big, "cuda")
    want = [sr.resize_yuv420(fr, CH, CW, H, W, 8) for fr in _frames(small, CW, CH)]
    got = _frames(big, W, H)
    assert len(got) == GOP and all(np.array_equal(g, w) for g, w in zip(got, want))


def test_bitrate_and_structure_fill(seq):
    import pmctf_rate
    import pmctf_scale
    frames = 7                                                       # fill: GOPs of 4, 2 and 1
    kw = dict(structure="fill", q_choices=range(0, 21, 5), max_trials=2, picture_hash="u8")
    scaled, plain = _bins(seq, "scaled_rate"), _bins(seq, "plain_rate")
    r = pmctf_scale.encode_sequence_rate(seq["enc_net"], seq["src8"], W, H, frames, GOP, 60000, 30, scaled, "cuda",
                                         coded_size=(CW, CH), **kw)
    p = pmctf_rate.encode_sequence_rate(seq["enc_net"], seq["down8"], CW, CH, frames, GOP, 60000, 30, plain, "cuda", **kw)
    assert [g["size"] for g in r["gops"]] == [4, 2, 1] and r["gops"] == p["gops"]
    _same_folder(scaled, plain)
    v = pmctf_rate.verify_rate_record(scaled)
    assert v["frame_num"] == frames and v["header"]["width"] == CW and v["header"]["height"] == CH
    assert len(r["display_quality"]) == frames
    big = str(seq["tmp"] / "rate_display.yuv")
    import pmctf_gop
    d = pmctf_gop.decode_sequence(seq["dec_net"], scaled, big, "cuda")
    assert d["frames"] == [(H, W)] * frames and d["verified"] == frames
    assert os.path.getsize(big) == frames * W * H * 3 // 2


def test_a_folder_without_the_header_decodes_as_before(seq, coded8):
    """the plain folder through the old and the new entry point, with and without coded_size_output: the same bytes, which
    are those of the encoder's own reconstruction (its u8 hashes)"""
    import pmctf_gop
    import pmctf_scale
    outs = [str(seq["tmp"] / f"plain_{k}.yuv") for k in range(3)]
    a = pmctf_gop.decode_sequence(seq["dec_net"], coded8["plain"], outs[0], "cuda")
    pmctf_scale.decode_sequence_checked(seq["dec_net"], coded8["plain"], outs[1], "cuda")
    pmctf_scale.decode_sequence_checked(seq["dec_net"], coded8["plain"], outs[2], "cuda", coded_size_output=True)
    data = [open(p, "rb").read() for p in outs]
    assert data[0] == data[1] == data[2] and len(data[0]) == N * CW * CH * 3 // 2
    assert a["frames"] == [(CH, CW)] * N and sorted(a) == ["bitdepth", "frames", "hash_mismatches", "header", "seconds",
                                                          "verified"]
    assert pmctf_gop.check_yuv_hashes(coded8["plain"], outs[0]) == (N, [])
    assert "display_quality" not in coded8["p"]
    assert sorted(os.listdir(coded8["plain"])) == ["gop_00000", "gop_00001", "picture_hashes.json", "sequence.json"]


def test_extracted_layer_decodes_at_the_display_size(seq, coded8):
    import pmctf_layers
    import pmctf_scale
    small = str(seq["tmp"] / "level1")
    written = pmctf_layers.extract_layer(coded8["scaled"], small, 1)
    assert "display_format.json" in written and os.path.exists(os.path.join(small, "display_format.json"))
    big, coded = str(seq["tmp"] / "level1_display.yuv"), str(seq["tmp"] / "level1_coded.yuv")
    d = pmctf_layers.decode_sequence_layer(seq["dec_net"], small, big, 1, "cuda")
    c = pmctf_scale.decode_sequence_layer(seq["dec_net"], small, coded, 1, "cuda", coded_size_output=True)
    assert d["times"] == c["times"] == [0, 2, 4, 6]
    assert d["frames"] == [(H, W)] * 4 and c["frames"] == [(CH, CW)] * 4
    want = [sr.resize_yuv420(fr, CH, CW, H, W, 8) for fr in _frames(coded, CW, CH)]
    got = _frames(big, W, H)
    assert len(got) == 4 and all(np.array_equal(g, w) for g, w in zip(got, want))
