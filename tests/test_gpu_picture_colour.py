"""RGB pictures on the GPU: the two kernels of csrc/picture_colour.hip against the numpy restatement byte for
byte (every layout, matrix, range and depth, guarded destinations, every alignment, bits above the depth), and RGB sources
and outputs end to end.  No tolerance anywhere."""
import importlib.util
import os
import shutil

import numpy as np
import pytest
import torch

import colour_restatement as cr
from helpers import product_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(2, 2), (6, 10), (100, 132)]                 # rows x columns: one item, ragged, more than one block
CASES = [(m, r) for m in ("bt601", "bt709", "bt2020") for r in ("full", "limited")]
LAYOUTS = sorted(cr.LAYOUTS)
GUARD, SENTINEL = 64, 0xA5


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _word(layout):
    return 1 if cr.LAYOUTS[layout][0] == 8 else 2


def _planar_dtype(layout):
    return np.uint8 if cr.LAYOUTS[layout][0] == 8 else np.uint16


def _rgb_pictures(layout, h, w):
    """(R, G, B) triples: random, all zero, all maximum, the 256 (1024) greys, the eight cube corners repeated"""
    depth = cr.LAYOUTS[layout][0]
    n, top = h * w, (1 << cr.LAYOUTS[layout][0]) - 1
    rng = np.random.default_rng(h * 1000 + w + depth)
    i = np.arange(n)
    grey = i % 256 if depth == 8 else (i % 1024) * (top // 1023)
    return {"random": tuple(rng.integers(0, top + 1, (3, n))), "zero": (np.zeros(n, np.int64),) * 3,
            "max": (np.full(n, top),) * 3, "greys": (grey,) * 3,
            "corners": tuple(((i >> k) & 1) * top for k in range(3))}


def _ycc_pictures(layout, h, w, matrix, rng_name):
    """packed planar pictures: random over the whole code range (all three clamps act), all zero, all maximum, and the
    conversions of the greys and the corners"""
    depth = cr.LAYOUTS[layout][0]
    n, top = 3 * h * w, (1 << depth) - 1
    rng = np.random.default_rng(h * 1000 + w + depth + 1)
    dt = _planar_dtype(layout)
    rgb = _rgb_pictures(layout, h, w)
    out = {"random": rng.integers(0, top + 1, n).astype(dt), "zero": np.zeros(n, dt), "max": np.full(n, top, dt)}
    for name in ("greys", "corners"):
        out[name] = np.concatenate(cr.forward(*rgb[name], matrix, rng_name, depth)).astype(dt)
    return out


def _loud(a, layout):
    """16-bit samples with every bit above the depth set"""
    depth = cr.LAYOUTS[layout][0]
    return a if depth in (8, 16) else a | np.uint16((0xFFFF << depth) & 0xFFFF)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_kernels_equal_the_restatement(cuda, layout):
    import pmctf_colour
    word, dt = _word(layout), _planar_dtype(layout)
    for matrix, rng in CASES:
        colour = (matrix, rng)
        for h, w in SIZES:
            n, need = 3 * h * w, cr.frame_bytes(layout, h, w)
            for name, rgb in _rgb_pictures(layout, h, w).items():
                what = f"{layout} {matrix} {rng} {h}x{w} {name}"
                surface = cr.pack_rgb(*rgb, layout, h, w)
                want = cr.rgb_to_planar(surface, layout, h, w, matrix, rng)
                loud = surface if word == 1 else _loud(surface.view("<u2"), layout).view(np.uint8)
                if layout in ("rgba", "bgra"):                           # the fourth byte is ignored
                    loud = surface.copy()
                    loud[3::4] = np.arange(h * w) & 255
                for src in (surface, loud):
                    buf = _dev(np.full(n + 2 * GUARD, 0x5A5A if word == 2 else 0x5A, dt), cuda)
                    got = pmctf_colour.rgb_to_ycc(_dev(src, cuda), layout, h, w, colour, out=buf[GUARD:GUARD + n])
                    assert got.data_ptr() == buf.data_ptr() + GUARD * word
                    host = buf.cpu().numpy()
                    assert np.array_equal(host[GUARD:GUARD + n], want), what
                    assert (host[:GUARD] == host[0]).all() and (host[GUARD + n:] == host[0]).all(), what
            for name, frame in _ycc_pictures(layout, h, w, matrix, rng).items():
                what = f"{layout} {matrix} {rng} {h}x{w} inverse {name}"
                want = np.full(need + 2 * GUARD, SENTINEL, np.uint8)
                want[GUARD:GUARD + need] = cr.planar_to_rgb(frame, layout, h, w, matrix, rng)
                for src in (frame, _loud(frame, layout)):
                    buf = _dev(np.full(need + 2 * GUARD, SENTINEL, np.uint8), cuda)
                    pmctf_colour.ycc_to_rgb(_dev(src, cuda), layout, h, w, colour, out=buf[GUARD:GUARD + need])
                    assert np.array_equal(buf.cpu().numpy(), want), what
        # without `out`: fresh tensors of the stated type and size
        h, w = 6, 10
        surface = cr.pack_rgb(*_rgb_pictures(layout, h, w)["random"], layout, h, w)
        got = pmctf_colour.RgbUnpacker(layout, w, h, colour)(_dev(surface, cuda))
        assert got.dtype == (torch.uint8 if word == 1 else torch.uint16) and got.shape == (3 * h * w,)
        assert np.array_equal(got.cpu().numpy(), cr.rgb_to_planar(surface, layout, h, w, matrix, rng))
        back = pmctf_colour.RgbPacker(layout, w, h, colour)(got)
        assert back.dtype == torch.uint8 and back.shape == (cr.frame_bytes(layout, h, w),)
        assert np.array_equal(back.cpu().numpy(), cr.planar_to_rgb(got.cpu().numpy(), layout, h, w, matrix, rng))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_alignment_of_source_and_destination(cuda, layout):
    """offset views of larger buffers: surface and planar picture each at 0..3 containers past a 16-byte boundary, which
    covers every choice load4 / store4 and the 16-byte pixel-quad access make"""
    import pmctf_colour
    h, w = 6, 10
    matrix, rng = "bt709", "limited"
    word, dt = _word(layout), _planar_dtype(layout)
    need, n = cr.frame_bytes(layout, h, w), 3 * h * w
    surface = cr.pack_rgb(*_rgb_pictures(layout, h, w)["random"], layout, h, w)
    frame = cr.rgb_to_planar(surface, layout, h, w, matrix, rng)
    rgb_back = cr.planar_to_rgb(frame, layout, h, w, matrix, rng)
    base = torch.empty(need + 64, dtype=torch.uint8, device=cuda)
    start = (-base.data_ptr()) % 16 + 16
    fill = 0x5A if word == 1 else 0x5A5A
    planar = _dev(np.full(n + 64, fill, dt), cuda)
    pstart = ((-planar.data_ptr()) % 16) // word + 16 // word
    for so in range(4):
        for po in range(4):
            s_view = base[start + so * word:start + so * word + need]
            p_view = planar[pstart + po:pstart + po + n]
            assert s_view.data_ptr() % 16 == so * word and p_view.data_ptr() % 16 == po * word
            base.fill_(SENTINEL)
            s_view.copy_(_dev(surface, cuda))
            planar.fill_(fill)
            pmctf_colour.rgb_to_ycc(s_view, layout, h, w, (matrix, rng), out=p_view)
            host = planar.cpu().numpy()
            assert np.array_equal(host[pstart + po:pstart + po + n], frame), (layout, so, po)
            assert (np.delete(host, np.s_[pstart + po:pstart + po + n]) == fill).all(), (layout, so, po)
            base.fill_(SENTINEL)
            pmctf_colour.ycc_to_rgb(p_view, layout, h, w, (matrix, rng), out=s_view)
            host = base.cpu().numpy()
            at = start + so * word
            assert np.array_equal(host[at:at + need], rgb_back), (layout, so, po)
            assert (np.delete(host, np.s_[at:at + need]) == SENTINEL).all(), (layout, so, po)


# ------------------------------------------------------------------------------------------------------ through the layers
W, H, GOP, N, Q = 132, 100, 4, 8, 3
COLOUR = ("bt709", "limited")


def _files(folder, skip=()):
    out = {}
    for base, _, names in os.walk(folder):
        for n in names:
            p = os.path.join(base, n)
            if os.path.relpath(p, folder) not in skip:
                out[os.path.relpath(p, folder)] = open(p, "rb").read()
    return out


def _same_folder(new, plain, skip=("colour_format.json",)):
    fs, fp = _files(new, skip), _files(plain, skip)
    assert sorted(fs) == sorted(fp) and any(p.endswith(".bin") for p in fp)
    for p in sorted(fp):
        assert fs[p] == fp[p], f"{p} differs"


def _write(path, frames):
    with open(path, "wb") as f:
        for fr in frames:
            f.write(np.ascontiguousarray(fr).tobytes())


def _rgb_source(n, depth=8):
    """n synthetic RGB pictures of W x H as (R, G, B) flat arrays: moving, smooth, coloured; above 8 bits with low bits"""
    import pmctf_synth
    a = pmctf_synth.synth_yuv420(W, H, n, seed=91)
    b = pmctf_synth.synth_yuv420(W, H, n, seed=92)
    rng = np.random.default_rng(depth)
    out = []
    for (ya, _, _), (yb, _, _) in zip(a, b):
        planes = [ya.astype(np.int64), yb.astype(np.int64), 255 - (ya.astype(np.int64) + yb) // 2]
        if depth > 8:
            planes = [(p << (depth - 8)) + rng.integers(0, 1 << (depth - 8), p.shape) for p in planes]
        out.append(tuple(p.reshape(-1) for p in planes))
    return out


@pytest.fixture(scope="module")
def seq(cuda, tmp_path_factory):
    """the models, and the rgb24 source with the folder it codes to, made once"""
    import pmctf_colour
    tmp = tmp_path_factory.mktemp("picture_colour")
    s = {"tmp": tmp, "enc_net": product_model(1)[0], "dec_net": product_model(1)[0], "rgb": _rgb_source(N)}
    s["src"], s["new"] = str(tmp / "src.rgb"), str(tmp / "new_rgb24")
    _write(s["src"], [cr.pack_rgb(*p, "rgb24", H, W) for p in s["rgb"]])
    os.makedirs(s["new"])
    s["result"] = pmctf_colour.encode_sequence(s["enc_net"], s["src"], W, H, N, GOP, Q, s["new"], "cuda", keep_gops=True,
                                               picture_hash="u8", rgb_layout="rgb24", colour=COLOUR)
    return s


def _bins(seq, name):
    p = str(seq["tmp"] / name)
    os.makedirs(p)
    return p


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_an_rgb24_file_codes_as_the_planar_444_file_convert_file_makes(seq):
    import pmctf_chroma
    import pmctf_colour
    planar = str(seq["tmp"] / "src444.yuv")
    assert pmctf_colour.convert_file(seq["src"], planar, W, H, "rgb24", "planar444", COLOUR, "cuda") == N
    want = b"".join(cr.rgb_to_planar(cr.pack_rgb(*p, "rgb24", H, W), "rgb24", H, W, *COLOUR).tobytes() for p in seq["rgb"])
    assert open(planar, "rb").read() == want
    plain = _bins(seq, "plain_444")
    p = pmctf_chroma.encode_sequence(seq["enc_net"], planar, W, H, N, GOP, Q, plain, "cuda", keep_gops=True, picture_hash="u8",
                                     chroma_format="444")
    _same_folder(seq["new"], plain)
    r = seq["result"]
    assert r["bits"] == p["bits"] and r["psnr"] == p["psnr"] and r["picture_hashes"] == p["picture_hashes"]
    assert "colour_format.json" not in _files(plain) and pmctf_chroma.read_source_format(seq["new"])["chroma_format"] == "444"
    assert pmctf_colour.read_colour_format(seq["new"]) == {"format_version": 1, "matrix": "bt709", "range": "limited",
                                                           "fixed_point_bits": 29, "source": "rgb"}
    # and back through convert_file: the restatement's RGB of the planar file
    back = str(seq["tmp"] / "back.bgra")
    assert pmctf_colour.convert_file(planar, back, W, H, "planar444", "bgra", COLOUR, "cuda", bitdepth=8) == N
    frames = np.frombuffer(want, np.uint8).reshape(N, -1)
    assert open(back, "rb").read() == b"".join(cr.planar_to_rgb(f, "bgra", H, W, *COLOUR).tobytes() for f in frames)


def test_the_pngs_of_the_same_pixels_code_to_the_same_files(seq):
    from PIL import Image
    import pmctf_colour
    pngs = str(seq["tmp"] / "pngs_in")
    os.makedirs(pngs)
    for i, p in enumerate(seq["rgb"]):
        Image.fromarray(cr.pack_rgb(*p, "rgb24", H, W).reshape(H, W, 3)).save(os.path.join(pngs, f"{i}.png"))
    folder = _bins(seq, "new_png")
    r = pmctf_colour.encode_sequence(seq["enc_net"], pngs, W, H, N, GOP, Q, folder, "cuda", keep_gops=True, picture_hash="u8",
                                     src_format="png", colour=COLOUR)
    _same_folder(folder, seq["new"], skip=())
    assert r["bits"] == seq["result"]["bits"] and r["picture_hashes"] == seq["result"]["picture_hashes"]


def test_rgb_out_and_png_out_are_the_restatement_of_the_444_output(seq):
    from PIL import Image
    import pmctf_chroma
    import pmctf_colour
    import pmctf_gop
    out444, rgb, pngs, old = (str(seq["tmp"] / n) for n in ("dec444.yuv", "dec.rgb", "pngs_709", "pngs_601"))
    pmctf_chroma.decode_sequence_checked(seq["dec_net"], seq["new"], out444, "cuda")
    frames = np.fromfile(out444, np.uint8).reshape(N, 3 * H * W)
    d = pmctf_colour.decode_sequence_checked(seq["dec_net"], seq["new"], None, "cuda", png_out=pngs, rgb_out=rgb,
                                             rgb_layout="rgb24")
    assert d["verified"] == N and d["frames"] == [(H, W)] * N and d["hash_mismatches"] == []
    want = [cr.planar_to_rgb(f, "rgb24", H, W, *COLOUR) for f in frames]
    assert open(rgb, "rb").read() == b"".join(w_.tobytes() for w_ in want)
    pmctf_gop.decode_sequence(seq["dec_net"], seq["new"], None, "cuda", png_out=old)
    assert sorted(os.listdir(pngs)) == sorted(os.listdir(old)) == sorted(f"{i}.png" for i in range(N))
    for i in range(N):
        ours = np.array(Image.open(os.path.join(pngs, f"{i}.png")))
        assert ours.shape == (H, W, 3) and np.array_equal(ours.reshape(-1), want[i]), i
        assert not np.array_equal(ours, np.array(Image.open(os.path.join(old, f"{i}.png")))), i
    # another layout and an explicit description, with the planar file written beside it, at temporal level 1
    gbr, yuv, lvl = (str(seq["tmp"] / n) for n in ("dec.gbrp", "dec_l1.yuv", "dec444_l1.yuv"))
    pmctf_chroma.decode_sequence_layer(seq["dec_net"], seq["new"], lvl, 1, "cuda", verify=False)
    d = pmctf_colour.decode_sequence_layer(seq["dec_net"], seq["new"], yuv, 1, "cuda", verify=False, rgb_out=gbr,
                                           rgb_layout="gbrp", colour=("bt2020", "full"))
    assert open(yuv, "rb").read() == open(lvl, "rb").read() and len(d["frames"]) == N // 2
    half = np.fromfile(lvl, np.uint8).reshape(N // 2, 3 * H * W)
    assert open(gbr, "rb").read() == b"".join(cr.planar_to_rgb(f, "gbrp", H, W, "bt2020", "full").tobytes() for f in half)


def test_the_command_line_writes_chosen_pictures_as_bgra(seq, capsys):
    out444, out = str(seq["tmp"] / "cli444.yuv"), str(seq["tmp"] / "cli.bgra")
    dec = _tool("decode_sequence")
    dec.main(["--synth-seed", "0", "--frames", "1:3,6", seq["new"], out444])
    dec.main(["--synth-seed", "0", "--frames", "1:3,6", "--rgb-output", out, "--rgb-layout", "bgra", seq["new"]])
    assert capsys.readouterr().out.count('"verified": 3') == 2
    frames = np.fromfile(out444, np.uint8).reshape(3, 3 * H * W)
    assert open(out, "rb").read() == b"".join(cr.planar_to_rgb(f, "bgra", H, W, *COLOUR).tobytes() for f in frames)


def test_a_yuv_source_with_a_colour_is_only_described(seq):
    import pmctf_colour
    import pmctf_gop
    import pmctf_layout
    import pmctf_synth
    raw = str(seq["tmp"] / "src420.yuv")
    _write(raw, [np.concatenate([p.reshape(-1) for p in fr]) for fr in pmctf_synth.synth_yuv420(W, H, GOP, seed=77)])
    new, plain = _bins(seq, "new_420"), _bins(seq, "plain_420")
    r = pmctf_colour.encode_sequence(seq["enc_net"], raw, W, H, GOP, GOP, Q, new, "cuda", keep_gops=True, picture_hash="u8",
                                     colour=COLOUR)
    p = pmctf_gop.encode_sequence(seq["enc_net"], raw, W, H, GOP, GOP, Q, plain, "cuda", keep_gops=True, picture_hash="u8")
    _same_folder(new, plain)
    assert r["bits"] == p["bits"] and r["psnr"] == p["psnr"] and r["picture_hashes"] == p["picture_hashes"]
    assert sorted(set(_files(new)) - set(_files(plain))) == ["colour_format.json"]
    assert pmctf_colour.read_colour_format(new)["source"] == "ycbcr"
    # the existing decoder writes what it writes for the folder without the new file, for this folder and the RGB one
    for folder, name in ((new, "a"), (seq["new"], "b")):
        bare = str(seq["tmp"] / f"bare_{name}")
        shutil.copytree(folder, bare)
        os.remove(os.path.join(bare, "colour_format.json"))
        with_file, without = str(seq["tmp"] / f"with_{name}.yuv"), str(seq["tmp"] / f"without_{name}.yuv")
        pmctf_layout.decode_sequence_checked(seq["dec_net"], folder, with_file, "cuda")
        pmctf_layout.decode_sequence_checked(seq["dec_net"], bare, without, "cuda")
        assert open(with_file, "rb").read() == open(without, "rb").read() and os.path.getsize(without) > 0
    # the 4:2:0 pictures of the described folder as RGB: to 4:4:4 by the exact filter, then the restatement
    import pmctf_chroma
    rgb = str(seq["tmp"] / "dec420.rgb")
    pmctf_colour.decode_sequence_checked(seq["dec_net"], new, None, "cuda", rgb_out=rgb, rgb_layout="rgb24")
    to444 = pmctf_chroma.Converter(W, H, "420", "444", "cuda", 8, "center")
    frames = np.fromfile(str(seq["tmp"] / "with_a.yuv"), np.uint8).reshape(GOP, -1)
    want = [cr.planar_to_rgb(to444(_dev(f, "cuda")).cpu().numpy(), "rgb24", H, W, *COLOUR) for f in frames]
    assert open(rgb, "rb").read() == b"".join(w_.tobytes() for w_ in want)


def test_gbrp10_in_and_gbrp10_out(seq):
    import pmctf_chroma
    import pmctf_colour
    import pmctf_gop
    colour = ("bt2020", "limited")
    pictures = _rgb_source(GOP, 10)
    src, planar = str(seq["tmp"] / "src.gbrp10"), str(seq["tmp"] / "src444p10.yuv")
    surfaces = [cr.pack_rgb(*p, "gbrp10", H, W) for p in pictures]
    _write(src, surfaces)
    _write(planar, [cr.rgb_to_planar(s, "gbrp10", H, W, *colour).astype("<u2") for s in surfaces])
    new, plain = _bins(seq, "new_gbrp10"), _bins(seq, "plain_444p10")
    pmctf_colour.encode_sequence(seq["enc_net"], src, W, H, GOP, GOP, Q, new, "cuda", keep_gops=True, picture_hash="u16",
                                 rgb_layout="gbrp10", colour=colour)
    pmctf_chroma.encode_sequence(seq["enc_net"], planar, W, H, GOP, GOP, Q, plain, "cuda", keep_gops=True, picture_hash="u16",
                                 chroma_format="444", bitdepth=10)
    _same_folder(new, plain)
    assert pmctf_gop.read_picture_format(new) == 10 and pmctf_colour.read_colour_format(new)["matrix"] == "bt2020"
    out444, out = str(seq["tmp"] / "dec444p10.yuv"), str(seq["tmp"] / "dec.gbrp10")
    pmctf_chroma.decode_sequence_checked(seq["dec_net"], new, out444, "cuda")
    d = pmctf_colour.decode_sequence_checked(seq["dec_net"], new, None, "cuda", rgb_out=out, rgb_layout="gbrp10")
    assert d["verified"] == GOP and d["bitdepth"] == 10
    frames = np.fromfile(out444, "<u2").reshape(GOP, 3 * H * W)
    assert open(out, "rb").read() == b"".join(cr.planar_to_rgb(f, "gbrp10", H, W, *colour).tobytes() for f in frames)
    # a layout of another depth than the folder's
    for layout in ("rgb24", "rgb48", "gbrp12"):
        with pytest.raises(ValueError, match=f"rgb_layout '{layout}' holds pictures of"):
            pmctf_colour.decode_sequence_checked(seq["dec_net"], new, None, "cuda", rgb_out=out, rgb_layout=layout)
    with pytest.raises(ValueError, match="png_out writes 8-bit PNGs"):
        pmctf_colour.decode_sequence_checked(seq["dec_net"], new, None, "cuda", png_out=str(seq["tmp"] / "never"))


def test_rgb_out_needs_a_description_and_a_layout_of_the_folders_depth(seq):
    import pmctf_colour
    bare, out = str(seq["tmp"] / "bare_rgb"), str(seq["tmp"] / "never.rgb")
    shutil.copytree(seq["new"], bare)
    os.remove(os.path.join(bare, "colour_format.json"))
    with pytest.raises(ValueError, match=r"bare_rgb.colour_format\.json: missing"):
        pmctf_colour.decode_sequence_checked(seq["dec_net"], bare, None, "cuda", rgb_out=out, rgb_layout="rgb24")
    for layout in ("gbrp10", "rgb48"):
        with pytest.raises(ValueError, match=f"rgb_layout '{layout}' holds pictures of 1[06] bits; the pictures of .* have 8 bits"):
            pmctf_colour.decode_sequence_checked(seq["dec_net"], seq["new"], None, "cuda", rgb_out=out, rgb_layout=layout)
    assert not os.path.exists(out)
    # with a description given, the bare folder decodes, to the bytes of the described one
    a, b = str(seq["tmp"] / "a.bgr"), str(seq["tmp"] / "b.bgr")
    pmctf_colour.decode_sequence_checked(seq["dec_net"], bare, None, "cuda", rgb_out=a, rgb_layout="bgr24", colour=COLOUR)
    pmctf_colour.decode_sequence_checked(seq["dec_net"], seq["new"], None, "cuda", rgb_out=b, rgb_layout="bgr24")
    assert open(a, "rb").read() == open(b, "rb").read() and os.path.getsize(a) == 3 * W * H * N
