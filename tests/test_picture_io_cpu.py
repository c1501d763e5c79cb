"""Picture input / output without a GPU: the three entry points of csrc/picture_ops.hip are declared, bound and exported and
refuse bad arguments before anything is launched; the host-side pieces of the public interface (PNGReader, write_pngs,
the new parameters of encode_sequence / decode_sequence)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmctf_yuv420_to_rgb8_f32", "pmctf_yuv420_u8_to_planes_f32", "pmctf_rgb8_to_yuv420_u8")


def test_entry_points_are_declared_bound_and_exported():
    from pMCTF.hip import lib
    text = open(os.path.join(ROOT, "include", "pmctf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(pmctf_\w+)\s*\(", text))
    H = C.CDLL(lib.HIP_SO)
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/pmctf_hip.h"
        assert s in lib.exported_symbols(), f"{s} has no ctypes signature in pMCTF/hip/lib.py"
        assert hasattr(H, s), f"libpmctf_hip.so does not export {s}"
    src = open(os.path.join(ROOT, "learned-pmctf_amd", "csrc", "picture_ops.hip")).read()
    for s in SYMBOLS:                                # the kernels live in the new file, sharing one copy of the colour code
        assert re.search(r'extern "C" int ' + s + r"\(", src)
    assert '#include "picture_math.h"' in src
    quality = open(os.path.join(ROOT, "learned-pmctf_amd", "csrc", "quality_ops.hip")).read()
    assert '#include "picture_math.h"' in quality and "float round_u8(" not in quality and "void to_rgb(" not in quality


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from pMCTF.hip import lib
    L = lib.hip()
    one = C.c_void_p(4096)                           # non-null, aligned, never dereferenced: the checks come first
    to_rgb, to_planes, to_yuv = (getattr(L, s) for s in SYMBOLS)
    assert to_rgb(None, None, None, 128, 128, 100, 100, None) == -1
    for k in range(3):
        p = [one] * 3
        p[k] = None
        assert to_rgb(p[0], p[1], p[2], 128, 128, 100, 100, None) == -1, k
    assert to_planes(None, None, None, None, None, 128, 128, 100, 100, None) == -1
    for k in range(3):                               # the two originals may be null, the other three not
        p = [one] * 3
        p[k] = None
        assert to_planes(p[0], p[1], p[2], one, one, 128, 128, 100, 100, None) == -1, k
    assert to_yuv(None, None, 100, 100, None) == -1
    assert to_yuv(None, one, 100, 100, None) == -1 and to_yuv(one, None, 100, 100, None) == -1
    for h, w in ((99, 100), (100, 99), (1, 1), (0, 100), (100, 0), (-2, 100), (100, -2), (16386, 100)):
        assert to_rgb(one, one, one, 16384, 16384, h, w, None) == -1, (h, w)
        assert to_planes(one, one, one, one, one, 16384, 16384, h, w, None) == -1, (h, w)
        assert to_planes(one, one, one, None, None, 16384, 16384, h, w, None) == -1, (h, w)
        assert to_yuv(one, one, h, w, None) == -1, (h, w)
    for Hp, Wp in ((98, 128), (128, 98), (127, 128), (128, 127)):          # padded size smaller than the picture, or odd
        assert to_rgb(one, one, one, Hp, Wp, 100, 100, None) == -1, (Hp, Wp)
        assert to_planes(one, one, one, one, one, Hp, Wp, 100, 100, None) == -1, (Hp, Wp)


def test_wrappers_check_their_arguments_before_any_launch():
    import torch
    from pMCTF.hip import ops
    y, c = torch.zeros((1, 1, 128, 128)), torch.zeros((2, 1, 64, 64))
    for h, w in ((99, 100), (100, 99), (0, 100), (100, -2), (130, 100)):
        with pytest.raises(ValueError):
            ops.frame_to_rgb8(y, c, h, w)
    with pytest.raises(ValueError):
        ops.frame_to_rgb8(y, torch.zeros((2, 1, 64, 32)), 100, 100)
    with pytest.raises(ValueError):
        ops.frame_to_rgb8(y.double(), c, 100, 100)
    with pytest.raises(RuntimeError):                # no CPU fallback
        ops.frame_to_rgb8(y, c, 100, 100)
    frame = torch.zeros(100 * 100 * 3 // 2, dtype=torch.uint8)
    for h, w in ((99, 100), (100, 99), (0, 100), (100, 102)):
        with pytest.raises(ValueError):
            ops.planes_from_u8(frame, h, w)
    with pytest.raises(ValueError):
        ops.planes_from_u8(frame.float(), 100, 100)
    with pytest.raises(ValueError):
        ops.planes_from_u8(frame, 100, 100, psize=3)
    with pytest.raises(RuntimeError):
        ops.planes_from_u8(frame, 100, 100)
    for shape in ((99, 100, 3), (100, 99, 3), (100, 100), (100, 100, 4), (3, 100, 100)):
        with pytest.raises(ValueError):
            ops.rgb8_to_yuv420(torch.zeros(shape, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.rgb8_to_yuv420(torch.zeros((100, 100, 3)))
    with pytest.raises(RuntimeError):
        ops.rgb8_to_yuv420(torch.zeros((100, 100, 3), dtype=torch.uint8))


def test_public_signatures():
    import pmctf_gop
    sig = inspect.signature(pmctf_gop.encode_sequence)
    assert list(sig.parameters)[:11] == ["codec", "yuv_path", "width", "height", "frame_num", "gop", "q_index", "bin_folder",
                                         "device", "skip_decoding", "psize"]
    p = sig.parameters
    assert (p["src_format"].default, p["ingest"].default, p["decoded_frame_path"].default) == ("yuv", "host", None)
    assert (p["skip_decoding"].default, p["psize"].default, p["keep_gops"].default, p["msssim"].default) == \
        (True, 128, False, False)
    d = inspect.signature(pmctf_gop.decode_sequence).parameters
    assert list(d) == ["codec", "bin_folder", "yuv_out", "device", "png_out"] and d["png_out"].default is None
    assert list(inspect.signature(pmctf_gop.read_gop_device).parameters) == ["reader", "gop", "device", "psize"]
    assert list(inspect.signature(pmctf_gop.frames_to_rgb8).parameters) == ["frames_rec", "pic_height", "pic_width"]
    assert list(inspect.signature(pmctf_gop.write_pngs).parameters) == ["folder", "first_index", "pictures"]
    assert list(inspect.signature(pmctf_gop.pngs_to_yuv).parameters) == ["paths_or_folder", "yuv_out", "device"]


def test_device_paths_refuse_the_cpu(tmp_path):
    import pmctf_gop
    rng = np.random.default_rng(0)
    pmctf_gop.write_pngs(str(tmp_path / "png"), 0, [rng.integers(0, 256, (4, 6, 3), dtype=np.uint8) for _ in range(2)])
    for kw in ({"src_format": "png"}, {"ingest": "device"}):
        with pytest.raises(RuntimeError, match="GPU"):
            pmctf_gop.encode_sequence(None, str(tmp_path / "png"), 6, 4, 2, 2, 3, str(tmp_path), "cpu", **kw)
    with pytest.raises(ValueError):
        pmctf_gop.encode_sequence(None, str(tmp_path / "png"), 6, 4, 2, 2, 3, str(tmp_path), "cpu", src_format="jpeg")
    with pytest.raises(RuntimeError, match="GPU"):
        pmctf_gop.read_gop_device(pmctf_gop.PNGReader(str(tmp_path / "png")), 2, "cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        pmctf_gop.pngs_to_yuv(str(tmp_path / "png"), str(tmp_path / "o.yuv"), "cpu")


def _save(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(path)


def test_png_reader(tmp_path):
    from PIL import Image
    import pmctf_gop
    rng = np.random.default_rng(1)
    folder = tmp_path / "seq"
    folder.mkdir()
    pics = {n: rng.integers(0, 256, (6, 10, 3), dtype=np.uint8) for n in ("10.png", "2.png", "1.png", "b3.png", "b12.png")}
    for n, a in pics.items():
        _save(str(folder / n), a)
    (folder / "notes.txt").write_text("not a picture")
    r = pmctf_gop.PNGReader(str(folder))
    assert [os.path.basename(p) for p in r.paths] == ["1.png", "2.png", "10.png", "b3.png", "b12.png"]   # natural order
    assert (r.width, r.height, len(r)) == (10, 6, 5)
    for p in r.paths:
        got = r.read_one_frame()
        assert got.dtype == np.uint8 and got.shape == (6, 10, 3) and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got, np.asarray(Image.open(p).convert("RGB")))
        assert np.array_equal(got, pics[os.path.basename(p)])
    assert r.read_one_frame() is None
    r.close()
    assert np.array_equal(r.read_one_frame(), pics["1.png"])             # close() rewinds, as YUVReader's does
    # a list of paths is taken in the order given
    r = pmctf_gop.PNGReader([str(folder / "10.png"), str(folder / "1.png")])
    assert np.array_equal(r.read_one_frame(), pics["10.png"]) and np.array_equal(r.read_one_frame(), pics["1.png"])
    # grey and palette pictures come out as RGB, as convert("RGB") makes them
    grey = rng.integers(0, 256, (4, 4), dtype=np.uint8)
    _save(str(tmp_path / "grey.png"), grey)
    got = pmctf_gop.PNGReader([str(tmp_path / "grey.png")]).read_one_frame()
    assert np.array_equal(got, np.repeat(grey[:, :, None], 3, axis=2))

    other = tmp_path / "mixed"
    other.mkdir()
    _save(str(other / "0.png"), pics["1.png"])
    _save(str(other / "1.png"), rng.integers(0, 256, (6, 12, 3), dtype=np.uint8))
    r = pmctf_gop.PNGReader(str(other))
    r.read_one_frame()
    with pytest.raises(AssertionError, match="size"):
        r.read_one_frame()
    for shape in ((5, 10, 3), (6, 9, 3)):
        odd = tmp_path / f"odd{shape[0]}x{shape[1]}"
        odd.mkdir()
        _save(str(odd / "0.png"), rng.integers(0, 256, shape, dtype=np.uint8))
        with pytest.raises(ValueError, match="even"):
            pmctf_gop.PNGReader(str(odd))
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(AssertionError):
        pmctf_gop.PNGReader(str(empty))


def test_write_pngs(tmp_path):
    from PIL import Image
    import pmctf_gop
    rng = np.random.default_rng(2)
    pics = [rng.integers(0, 256, (18, 22, 3), dtype=np.uint8) for _ in range(3)]
    out = tmp_path / "new" / "frames"                # created on demand
    paths = pmctf_gop.write_pngs(str(out), 8, pics)
    assert sorted(os.listdir(out)) == ["10.png", "8.png", "9.png"]
    assert [os.path.basename(p) for p in paths] == ["8.png", "9.png", "10.png"]
    for p, a in zip(paths, pics):
        im = Image.open(p)
        assert im.mode == "RGB" and im.size == (22, 18)
        assert np.array_equal(np.asarray(im), a)
    assert [np.array_equal(a, b) for a, b in zip(pics, _all(pmctf_gop.PNGReader(str(out))))] == [True] * 3
    with pytest.raises(ValueError):
        pmctf_gop.write_pngs(str(out), 0, [pics[0].astype(np.float32)])


def _all(reader):
    return [reader.read_one_frame() for _ in range(len(reader))]
