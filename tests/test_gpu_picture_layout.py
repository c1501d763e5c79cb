"""Pixel layouts on the GPU: the pack / unpack kernels against the numpy restatement value for value, guarded
destinations, every alignment, offsets past 2^32, SurfaceReader, and sources / outputs in a layout end to end."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import layout_restatement as lr
from helpers import product_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(2, 2), (6, 10), (100, 132)]                 # rows x columns: one item, ragged items, more than one block
V210_SIZES = [(h, w) for h in (2, 6) for w in (2, 4, 6, 8, 10, 12, 46, 48, 50)]
GUARD, SENTINEL = 64, 0xA5
LAYOUTS = sorted(lr.TABLE)


def _dtype(layout):
    return np.uint8 if lr.TABLE[layout][1] == 8 else np.uint16


def _pictures(layout, h, w):
    """random, all-maximum, and a different value in every component position (Y, Cb, Cr by column and row)"""
    depth = lr.TABLE[layout][1]
    n, top = lr.samples(layout, h, w), (1 << depth) - 1
    rng = np.random.default_rng(h * 1000 + w)
    pattern = (np.arange(n, dtype=np.uint32) * 37 + 11) % (top + 1)
    return {"random": rng.integers(0, top + 1, n).astype(_dtype(layout)), "max": np.full(n, top, _dtype(layout)),
            "pattern": pattern.astype(_dtype(layout))}


def _geometries(layout, h, w):
    container, base = lr.TABLE[layout][2], lr.row_bytes(layout, w)
    return [(base + extra, h + rows) for extra in (0, container, 64) for rows in (0, 2)]


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_kernels_equal_the_restatement(cuda, layout):
    from pMCTF.hip import ops
    for h, w in SIZES + (V210_SIZES if layout == "v210" else []):
        for pitch, luma_rows in _geometries(layout, h, w):
            need = lr.geometry(layout, h, w, pitch, luma_rows)[3]
            ones = lr.pack(np.full(lr.samples(layout, h, w), 0xFFFF, np.uint16), layout, h, w, pitch, luma_rows)
            for name, frame in _pictures(layout, h, w).items():
                what = f"{layout} {h}x{w} pitch {pitch} luma_rows {luma_rows} {name}"
                # packing into a guarded, sentinel-filled destination: the whole buffer is the restatement's
                before = np.full(need + 2 * GUARD, SENTINEL, np.uint8)
                want = before.copy()
                want[GUARD:GUARD + need] = lr.pack(frame, layout, h, w, pitch, luma_rows, into=before[GUARD:GUARD + need])
                buf = _dev(before, cuda)
                got = ops.pack_layout(_dev(frame, cuda), layout, h, w, None, pitch, luma_rows, out=buf[GUARD:GUARD + need])
                assert got.data_ptr() == buf.data_ptr() + GUARD
                assert np.array_equal(buf.cpu().numpy(), want), what
                # unpacking it, and the same surface with every ignorable bit and all padding set
                surface = want[GUARD:GUARD + need]
                for loud in (surface, surface | ~ones):
                    out = _dev(np.full(frame.size + 2 * GUARD, 0x5A5A if frame.itemsize == 2 else 0x5A, frame.dtype), cuda)
                    ops.unpack_layout(_dev(loud, cuda), layout, h, w, None, pitch, luma_rows, out=out[GUARD:GUARD + frame.size])
                    host = out.cpu().numpy()
                    assert np.array_equal(host[GUARD:GUARD + frame.size], frame), what
                    assert (host[:GUARD] == host[0]).all() and (host[GUARD + frame.size:] == host[0]).all(), what
            # without `out` the surface comes back with zero padding, and samples above the depth are masked
            frame = _pictures(layout, h, w)["random"]
            wide = frame if frame.itemsize == 1 or lr.TABLE[layout][1] == 16 else frame | np.uint16(0xF000)
            got = ops.pack_layout(_dev(wide, cuda), layout, h, w, pitch=pitch, luma_rows=luma_rows).cpu().numpy()
            assert np.array_equal(got, lr.pack(frame, layout, h, w, pitch, luma_rows))


def _tt(layout):
    return torch.uint8 if lr.TABLE[layout][1] == 8 else torch.uint16


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_alignment_of_source_and_destination(cuda, layout):
    """offset views of larger buffers: the surface moves in steps of its container, the planar picture in steps of a
    sample, both up to 16 bytes, which covers every choice load4 / store4 / the 16-byte group access make"""
    from pMCTF.hip import ops
    h, w = 6, 10
    depth, container = lr.TABLE[layout][1], lr.TABLE[layout][2]
    word = 1 if depth == 8 else 2
    frame = _pictures(layout, h, w)["random"]
    pitch = lr.row_bytes(layout, w) + container                         # rows change their alignment too
    surface = lr.pack(frame, layout, h, w, pitch)
    need, n = surface.size, frame.size
    base = torch.empty(need + 64 + 16, dtype=torch.uint8, device=cuda)
    start = (-base.data_ptr()) % 16 + 16                                # a 16-byte aligned place inside, room in front
    fill = 0x5A if word == 1 else 0x5A5A
    planar, planar_fill = (_dev(np.full(n + 64, fill, frame.dtype), cuda) for _ in range(2))
    pstart = ((-planar.data_ptr()) % 16) // word + 16 // word
    for so in range(0, 17, container):
        for po in range(0, 16 // word + 1):
            s_view = base[start + so:start + so + need]
            p_view = planar[pstart + po:pstart + po + n]
            assert s_view.data_ptr() % 16 == so % 16 and p_view.data_ptr() % 16 == (po * word) % 16
            # unpack: surface at so -> planar at po
            base.fill_(SENTINEL)
            s_view.copy_(_dev(surface, cuda))
            planar.copy_(planar_fill)
            ops.unpack_layout(s_view, layout, h, w, pitch=pitch, out=p_view)
            host = planar.cpu().numpy()
            assert np.array_equal(host[pstart + po:pstart + po + n], frame), (layout, so, po)
            assert (np.delete(host, np.s_[pstart + po:pstart + po + n]) == fill).all(), (layout, so, po)
            # pack: planar at po -> surface at so, nothing around it touched
            base.fill_(SENTINEL)
            ops.pack_layout(p_view, layout, h, w, pitch=pitch, out=s_view)
            host = base.cpu().numpy()
            want = lr.pack(frame, layout, h, w, pitch, into=np.full(need, SENTINEL, np.uint8))
            assert np.array_equal(host[start + so:start + so + need], want), (layout, so, po)
            assert (np.delete(host, np.s_[start + so:start + so + need]) == SENTINEL).all(), (layout, so, po)


@pytest.mark.parametrize("luma_rows", [40000, 70000])
def test_offsets_beyond_32_bits(cuda, luma_rows):
    """nv12, 64 x 2, pitch 65536: the chroma plane starts past 2^31 and past 2^32 bytes; only the addressed rows are filled"""
    from pMCTF.hip import ops
    h, w, pitch = 2, 64, 65536
    need = lr.geometry("nv12", h, w, pitch, luma_rows)[3]
    assert need == pitch * luma_rows + w and pitch * luma_rows > (1 << 31) * (1 if luma_rows == 40000 else 2)
    try:
        a = torch.empty(need, dtype=torch.uint8, device=cuda)
        b = torch.empty(need, dtype=torch.uint8, device=cuda)
    except RuntimeError as e:
        pytest.skip(f"no room for two surfaces of {need} bytes: {e}")
    frame = _pictures("nv12", h, w)["random"]
    tight = lr.pack(frame, "nv12", h, w)                                # rows of 64 bytes: Y0, Y1, CbCr
    rows = [(0, tight[:64]), (pitch, tight[64:128]), (pitch * luma_rows, tight[128:192])]
    for at, data in rows:
        a[at:at + 64] = _dev(data, cuda)
        b[at:min(at + 128, need)] = SENTINEL                             # the row and, where there is any, padding behind it
    got = ops.unpack_layout(a, "nv12", h, w, pitch=pitch, luma_rows=luma_rows)
    assert np.array_equal(got.cpu().numpy(), frame)
    ops.pack_layout(got, "nv12", h, w, pitch=pitch, luma_rows=luma_rows, out=b)
    for at, data in rows:
        assert np.array_equal(b[at:at + 64].cpu().numpy(), data), at
        if at + 128 <= need:
            assert (b[at + 64:at + 128].cpu().numpy() == SENTINEL).all(), at
    del a, b
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------ through the layers
W, H, CW, CH, GOP, N, Q = 132, 100, 66, 50, 4, 8, 3


def _files(folder):
    out = {}
    for base, _, names in os.walk(folder):
        for n in names:
            p = os.path.join(base, n)
            out[os.path.relpath(p, folder)] = open(p, "rb").read()
    return out


def _same_folder(new, plain):
    fs, fp = _files(new), _files(plain)
    assert sorted(fs) == sorted(fp)
    for p in sorted(fp):
        assert fs[p] == fp[p], f"{p} differs from coding the planar pictures"


def _write(path, frames):
    with open(path, "wb") as f:
        for fr in frames:
            f.write(np.ascontiguousarray(fr).tobytes())


def _raw_frames(path, n, dtype):
    data = np.fromfile(path, dtype=dtype)
    assert data.size % n == 0
    return [data[i * n:(i + 1) * n] for i in range(data.size // n)]


def _source(fmt, b):
    """N synthetic pictures of W x H, packed planar in `fmt`; above 8 bits with random low bits"""
    import pmctf_synth
    luma = pmctf_synth.synth_yuv420(W, H, N, seed=77)
    chroma = luma if fmt == "420" else pmctf_synth.synth_yuv420(W, 2 * H, N, seed=78)
    rng = np.random.default_rng(b)
    out = []
    for (y, _, _), (_, cb, cr) in zip(luma, chroma):
        fr = np.concatenate([p.reshape(-1) for p in (y, cb, cr)])
        if b > 8:
            fr = (fr.astype(np.uint16) << (b - 8)) + rng.integers(0, 1 << (b - 8), fr.size, dtype=np.uint16)
        out.append(fr)
    return out


@pytest.fixture(scope="module")
def seq(cuda, tmp_path_factory):
    return {"tmp": tmp_path_factory.mktemp("picture_layout"), "enc_net": product_model(1)[0], "dec_net": product_model(1)[0]}


def _bins(seq, name):
    p = str(seq["tmp"] / name)
    os.makedirs(p)
    return p


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _same_state(a, b):
    """two objects built by the same steps: equal values, tensors equal element for element, nested objects likewise"""
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, (tuple, list)):
        return type(a) is type(b) and len(a) == len(b) and all(_same_state(x, y) for x, y in zip(a, b))
    if hasattr(a, "__dict__"):
        return type(a) is type(b) and sorted(vars(a)) == sorted(vars(b)) and \
            all(_same_state(v, vars(b)[k]) for k, v in vars(a).items())
    return a == b


def test_without_a_layout_the_pipeline_is_pmctf_chromas(cuda, tmp_path):
    import pmctf_chroma
    import pmctf_layout
    src = str(tmp_path / "src444.yuv")
    with open(src, "wb") as f:
        f.truncate(3 * W * H * N)
    ours = pmctf_layout._pipeline(src, W, H, cuda, {}, (CW, CH), "444", None, None, None, None, "encode_sequence")
    theirs = pmctf_chroma._pipeline(src, W, H, cuda, {}, (CW, CH), "444", None, "encode_sequence")
    assert ours.layout is None and ours.to420 is not None and ours.size is not None and _same_state(ours, theirs)
    assert not _same_state(ours, pmctf_chroma._pipeline(src, W, H, cuda, {}, (CW, CH), "444", "left", "encode_sequence"))
    assert pmctf_layout._pipeline(src, W, H, cuda, {}, None, None, None, None, None, None, "encode_sequence") is None


def test_surface_reader_gives_the_planar_readers_triple(cuda, tmp_path):
    import pmctf_gop
    import pmctf_layout
    from pMCTF.utils.yuv_reader import YUVReader
    frames = _source("420", 8)[:GOP]
    raw = str(tmp_path / "src.yuv")
    _write(raw, frames)
    pitch, luma_rows = 192, 112
    surfaces = [_dev(lr.pack(fr, "nv12", H, W, pitch, luma_rows, into=np.full(192 * (112 + 50), 0xEE, np.uint8)), cuda)
                for fr in frames]
    want = pmctf_gop.read_gop_device(YUVReader(raw, W, H), GOP, cuda, 64)
    got = pmctf_gop.read_gop_device(pmctf_layout.SurfaceReader(surfaces, "nv12", W, H, pitch, luma_rows), GOP, cuda, 64)
    assert got[2] == want[2] == (H, W)
    for g_list, w_list in zip(got[:2], want[:2]):
        assert len(g_list) == len(w_list) == GOP
        for g, w_ in zip(g_list, w_list):
            assert all(torch.equal(a, b) and a.dtype == b.dtype and a.is_cuda for a, b in zip(g, w_))


def test_an_nv12_file_codes_as_its_planar_pictures_and_decodes_to_nv12(seq, capsys):
    import pmctf_gop
    import pmctf_layout
    frames = _source("420", 8)
    raw, src = str(seq["tmp"] / "src420.yuv"), str(seq["tmp"] / "src.nv12")
    _write(raw, frames)
    _write(src, [lr.pack(fr, "nv12", H, W) for fr in frames])
    new, plain = _bins(seq, "new_nv12"), _bins(seq, "plain_nv12")
    r = pmctf_layout.encode_sequence(seq["enc_net"], src, W, H, N, GOP, Q, new, "cuda", keep_gops=True, picture_hash="u8",
                                     pixel_layout="nv12")
    p = pmctf_gop.encode_sequence(seq["enc_net"], raw, W, H, N, GOP, Q, plain, "cuda", keep_gops=True, picture_hash="u8")
    _same_folder(new, plain)
    assert r["bits"] == p["bits"] and r["psnr"] == p["psnr"] and r["picture_hashes"] == p["picture_hashes"]
    dec_plain, out = str(seq["tmp"] / "dec_nv12_plain.yuv"), str(seq["tmp"] / "dec.nv12")
    pmctf_gop.decode_sequence(seq["dec_net"], plain, dec_plain, "cuda")
    _tool("decode_sequence").main(["--synth-seed", "0", "--output-layout", "nv12", new, out])
    assert '"verified": 8' in capsys.readouterr().out
    want = [lr.pack(fr, "nv12", H, W) for fr in _raw_frames(dec_plain, lr.samples("nv12", H, W), np.uint8)]
    assert len(want) == N and open(out, "rb").read() == b"".join(w_.tobytes() for w_ in want)
    # a layout of another format or depth than the pictures, and a Y4M file, are refused
    for layout, path in (("nv16", out), ("p010", out), ("nv12", str(seq["tmp"] / "dec.y4m"))):
        with pytest.raises(ValueError, match="output_layout"):
            pmctf_layout.decode_sequence_checked(seq["dec_net"], new, path, "cuda", output_layout=layout)


def test_a_v210_file_codes_as_its_planar_422_pictures_and_decodes_to_v210(seq):
    import pmctf_chroma
    import pmctf_layout
    frames = _source("422", 10)
    src, raw = str(seq["tmp"] / "src.v210"), str(seq["tmp"] / "src422p10.yuv")
    _write(src, [lr.pack(fr, "v210", H, W) for fr in frames])
    planar = [lr.unpack(s, "v210", H, W) for s in _raw_frames(src, 100 * 384, np.uint8)]
    assert all(np.array_equal(a, b) for a, b in zip(planar, frames))
    _write(raw, [fr.astype("<u2") for fr in planar])
    new, plain = _bins(seq, "new_v210"), _bins(seq, "plain_v210")
    pmctf_layout.encode_sequence(seq["enc_net"], src, W, H, N, GOP, Q, new, "cuda", keep_gops=True, picture_hash="u16",
                                 pixel_layout="v210")
    pmctf_chroma.encode_sequence(seq["enc_net"], raw, W, H, N, GOP, Q, plain, "cuda", keep_gops=True, picture_hash="u16",
                                 chroma_format="422", bitdepth=10)
    _same_folder(new, plain)
    assert pmctf_chroma.read_source_format(new)["chroma_format"] == "422"
    dec_plain, out = str(seq["tmp"] / "dec422_plain.yuv"), str(seq["tmp"] / "dec.v210")
    pmctf_chroma.decode_sequence_checked(seq["dec_net"], plain, dec_plain, "cuda")
    d = pmctf_layout.decode_sequence_checked(seq["dec_net"], new, out, "cuda", output_layout="v210")
    assert d["verified"] == N and d["bitdepth"] == 10 and d["frames"] == [(H, W)] * N
    want = [lr.pack(fr, "v210", H, W) for fr in _raw_frames(dec_plain, lr.samples("v210", H, W), "<u2")]
    assert len(want) == N and open(out, "rb").read() == b"".join(w_.tobytes() for w_ in want)
    # the coded 4:2:0 pictures have another format than v210
    with pytest.raises(ValueError, match="output_layout 'v210'"):
        pmctf_layout.decode_sequence_checked(seq["dec_net"], new, out, "cuda", coded_format_output=True, output_layout="v210")


def test_a_p010_source_at_a_coded_size_under_rate_control(seq):
    import pmctf_chroma
    import pmctf_layout
    frames = _source("420", 10)[:GOP]
    raw, src = str(seq["tmp"] / "src420p10.yuv"), str(seq["tmp"] / "src.p010")
    _write(raw, [fr.astype("<u2") for fr in frames])
    _write(src, [lr.pack(fr, "p010", H, W) for fr in frames])
    kw = dict(structure="fill", q_choices=range(0, 21, 5), max_trials=2, coded_size=(CW, CH))
    new, plain = _bins(seq, "new_p010"), _bins(seq, "plain_p010")
    r = pmctf_layout.encode_sequence_rate(seq["enc_net"], src, W, H, GOP, GOP, 60000, (30, 1), new, "cuda", pixel_layout="p010",
                                          **kw)
    p = pmctf_chroma.encode_sequence_rate(seq["enc_net"], raw, W, H, GOP, GOP, 60000, (30, 1), plain, "cuda", bitdepth=10, **kw)
    _same_folder(new, plain)
    assert "rate_control.json" in _files(new) and "display_format.json" in _files(new)
    timeless = lambda rate: [{k: v for k, v in g.items() if k != "seconds"} for g in rate]     # wall-clock time per GOP
    assert r["gops"] == p["gops"] and timeless(r["rate"]) == timeless(p["rate"])
    assert r["display_quality"] == p["display_quality"] and len(r["display_quality"]) == GOP


def test_convert_file_between_layouts(cuda, tmp_path, capsys):
    frames = _source("422", 10)[:2]
    raw, v210, y210, back = (str(tmp_path / n) for n in ("a.yuv", "a.v210", "a.y210", "b.yuv"))
    _write(raw, [fr.astype("<u2") for fr in frames])
    tool = _tool("convert_layout")
    size = ["--width", str(W), "--height", str(H)]
    tool.main([*size, "--from", "planar", "--to", "v210", raw, v210])
    tool.main([*size, "--from", "v210", "--to", "y210", v210, y210])
    tool.main([*size, "--from", "y210", "--to", "planar", y210, back])
    assert capsys.readouterr().out.count('"frames": 2') == 3
    assert open(v210, "rb").read() == b"".join(lr.pack(fr, "v210", H, W).tobytes() for fr in frames)
    assert open(y210, "rb").read() == b"".join(lr.pack(fr, "y210", H, W).tobytes() for fr in frames)
    assert open(back, "rb").read() == open(raw, "rb").read()


def test_the_command_lines_take_a_v210_file_there_and_back(seq, capsys):
    """tools/encode_sequence.py --pixel-layout v210, then tools/decode_sequence.py --output-layout v210: no other program
    touches a sample, and the output is the packing of what the same folder decodes to as planar 4:2:2"""
    import pmctf_chroma
    import pmctf_gop
    src, cli = str(seq["tmp"] / "cli.v210"), str(seq["tmp"] / "cli_v210")
    _write(src, [lr.pack(fr, "v210", H, W) for fr in _source("422", 10)[:GOP]])
    _tool("encode_sequence").main(["--synth-seed", "0", "--gop", str(GOP), "--width", str(W), "--height", str(H),
                                   "--pixel-layout", "v210", "--picture-hash", "u16", src, cli])
    assert pmctf_chroma.read_source_format(cli)["chroma_format"] == "422" and pmctf_gop.read_picture_format(cli) == 10
    planar, out = str(seq["tmp"] / "cli_422.yuv"), str(seq["tmp"] / "cli_out.v210")
    pmctf_chroma.decode_sequence_checked(seq["dec_net"], cli, planar, "cuda")
    _tool("decode_sequence").main(["--synth-seed", "0", "--output-layout", "v210", cli, out])
    assert '"verified": 4' in capsys.readouterr().out
    want = [lr.pack(fr, "v210", H, W) for fr in _raw_frames(planar, lr.samples("v210", H, W), "<u2")]
    assert len(want) == GOP and open(out, "rb").read() == b"".join(w_.tobytes() for w_ in want)
