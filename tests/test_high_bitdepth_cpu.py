"""High-bit-depth 4:2:0 sources, the parts that need no GPU: the 16-bit reader, read_gop's scaling and the parity anchor on
the host, the picture_format.json sidecar, the "u16" hash level and tools/check_picture_hashes.py on 16-bit files, the
public signatures, and the three entry points of csrc/picture_ops.hip / picture_hbd.hip (declared, bound, exported, refusing bad arguments
before anything is launched).  Everything is exact; the yardstick is tests/hbd_restatement.py and zlib.crc32."""
import ctypes as C
import importlib.util
import inspect
import json
import os
import re
import zlib

import numpy as np
import pytest
import torch

import hbd_restatement as hr
import pmctf_gop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmctf_yuv420_u16_to_planes_f32", "pmctf_planes_to_u16", "pmctf_frame_sse_u16_f32")


def _random_pictures(w, h, n, b, seed):
    rng = np.random.default_rng(seed)
    pics = []
    for _ in range(n):
        y = rng.integers(0, 1 << b, (h, w), dtype=np.uint16)
        c = rng.integers(0, 1 << b, (2, h // 2, w // 2), dtype=np.uint16)
        y[0, 0], y[-1, -1] = 0, (1 << b) - 1
        pics.append((y, c[0], c[1]))
    return pics


# ------------------------------------------------------------------------------------------------------------ reader
@pytest.mark.parametrize("b", [10, 16])
def test_reader_returns_the_samples_written(tmp_path, b):
    from pMCTF.utils.yuv_reader import YUVReader
    w, h, n = 10, 6, 3
    pics = _random_pictures(w, h, n, b, seed=b)
    path = str(tmp_path / "src.yuv")
    pmctf_gop.write_yuv(path, pics)
    assert os.path.getsize(path) == n * w * h * 3                     # two bytes per sample
    raw = np.fromfile(path, dtype="<u2")
    assert np.array_equal(raw[:w * h], pics[0][0].reshape(-1)), "little-endian words in file order"
    r = YUVReader(path, w, h, bitdepth=b)
    assert r.bitdepth == b
    for k in range(n):
        got = r.read_one_frame()
        for a, want in zip(got, pics[k]):
            assert a.dtype == np.uint16 and a.shape == want.shape and np.array_equal(a, want), k
    with pytest.raises(AssertionError):
        r.read_one_frame()                                            # past the end
    r.close()
    r = YUVReader(path, w, h, start_index=2, bitdepth=b)
    assert all(np.array_equal(a, want) for a, want in zip(r.read_one_frame(), pics[2]))
    r.close()
    for bad in (7, 17, 0):
        with pytest.raises(ValueError):
            YUVReader(path, w, h, bitdepth=bad)


def test_default_reader_is_unchanged(tmp_path):
    from pMCTF.utils.yuv_reader import YUVReader
    assert list(inspect.signature(YUVReader.__init__).parameters) == ["self", "src_file", "width", "height", "start_index",
                                                                      "bitdepth"]
    assert inspect.signature(YUVReader.__init__).parameters["bitdepth"].default == 8
    w, h = 10, 6
    data = np.random.default_rng(0).integers(0, 256, 2 * w * h * 3 // 2, dtype=np.uint8)
    path = str(tmp_path / "src8.yuv")
    data.tofile(path)
    r = YUVReader(path, w, h)
    assert r.bitdepth == 8
    for k in range(2):
        y, cb, cr = r.read_one_frame()
        assert y.dtype == np.uint8 and y.shape == (h, w) and cb.shape == cr.shape == (h // 2, w // 2)
        assert np.array_equal(np.concatenate([p.reshape(-1) for p in (y, cb, cr)]), data[k * 90:(k + 1) * 90])
    r.close()


# ---------------------------------------------------------------------------------------------------------- read_gop
@pytest.mark.parametrize("h,w,psize", [(6, 10, 2), (100, 132, 128)])
def test_read_gop_scales_on_the_host_as_the_restatement(tmp_path, h, w, psize):
    from pMCTF.utils.yuv_reader import YUVReader
    b, n = 10, 2
    pics = _random_pictures(w, h, n, b, seed=h)
    path = str(tmp_path / "src.yuv")
    pmctf_gop.write_yuv(path, pics)
    r = YUVReader(path, w, h, bitdepth=b)
    padded, orig, size = pmctf_gop.read_gop(r, n, "cpu", psize)
    r.close()
    assert size == (h, w)
    for k in range(n):
        want = hr.to_planes(hr.flat(pics[k]), h, w, b, psize)
        got = (padded[k][0], padded[k][1], orig[k][0], orig[k][1])
        for name, a, e in zip(("y_pad", "c_pad", "y_org", "c_org"), got, want):
            assert a.dtype == torch.float32 and tuple(a.shape) == e.shape, name
            assert np.array_equal(a.numpy(), e), (k, name)
        assert float(got[0].max()) <= 255.75 and bool((got[2] % 1.0 != 0).any()), "the low bits are fractions of the 8-bit range"


def test_parity_anchor_on_the_host(tmp_path):
    """a b-bit source of multiples of 2^(b-8) reaches the model as the tensors of the 8-bit source v >> (b-8)"""
    from pMCTF.utils.yuv_reader import YUVReader
    w, h, n = 132, 100, 2
    for b in (10, 12, 16):
        hbd = hr.synth_hbd(w, h, n, b, seed=5, low_bits=False)
        p16, p8 = str(tmp_path / f"src{b}.yuv"), str(tmp_path / f"src{b}_8.yuv")
        pmctf_gop.write_yuv(p16, hbd)
        pmctf_gop.write_yuv(p8, [tuple((p >> (b - 8)).astype(np.uint8) for p in pic) for pic in hbd])
        r16, r8 = YUVReader(p16, w, h, bitdepth=b), YUVReader(p8, w, h)
        a, b8 = pmctf_gop.read_gop(r16, n, "cpu"), pmctf_gop.read_gop(r8, n, "cpu")
        r16.close(), r8.close()
        assert a[2] == b8[2]
        for part in (0, 1):
            for k in range(n):
                for x, y in zip(a[part][k], b8[part][k]):
                    assert x.dtype == y.dtype and torch.equal(x, y), (b, part, k)
    low = hr.synth_hbd(w, h, 1, 10, seed=5, low_bits=True)
    assert any(bool((p & 3).any()) for p in low[0]) and all(int(p.max()) < 1024 for p in low[0])


# ----------------------------------------------------------------------------------------------------------- sidecar
def test_picture_format_round_trip_and_refusals(tmp_path):
    folder = str(tmp_path)
    path = os.path.join(folder, "picture_format.json")
    assert pmctf_gop.read_picture_format(folder) == 8                 # no file: an 8-bit folder
    for b in (9, 10, 16):
        assert pmctf_gop.write_picture_format(folder, b) == path
        assert json.load(open(path)) == {"format_version": 1, "bitdepth": b}
        assert pmctf_gop.read_picture_format(folder) == b
    os.remove(path)
    for b in (8, 17, 10.0, "10", True):
        with pytest.raises(ValueError) as e:
            pmctf_gop.write_picture_format(folder, b)
        assert path in str(e.value) and not os.path.exists(path)

    def refused(text):
        open(path, "w").write(text)
        with pytest.raises(ValueError) as e:
            pmctf_gop.read_picture_format(folder)
        assert path in str(e.value)
        return str(e.value)

    assert "version" in refused(json.dumps({"format_version": 2, "bitdepth": 10}))
    assert "version" in refused(json.dumps({"bitdepth": 10}))
    assert "fields" in refused(json.dumps({"format_version": 1, "bitdepth": 10, "chroma": "420"}))
    assert "fields" in refused(json.dumps({"format_version": 1}))
    for b in (8, 17, "10", 10.5):
        assert "bitdepth" in refused(json.dumps({"format_version": 1, "bitdepth": b}))
    assert "not a picture format file" in refused("{")
    assert "version" in refused("[1, 10]")


# ------------------------------------------------------------------------------------------------------------ hashes
W, H, N, GOP, B = 6, 10, 4, 2, 10                     # chroma planes of 5x3 samples: Cr starts at byte 150 of a picture
NY, NC = W * H * 2, (W // 2) * (H // 2) * 2           # bytes


def test_hash_level_u16():
    assert "u16" in pmctf_gop.HASH_LEVELS and pmctf_gop.HASH_KEYS["u16"] == pmctf_gop.HASH_KEYS["u8"]
    assert pmctf_gop.HASH_LEVELS[:2] == ("u8", "f32")
    assert list(inspect.signature(pmctf_gop.picture_hashes).parameters) == ["frames_rec", "pic_height", "pic_width", "level",
                                                                            "bitdepth"]
    assert inspect.signature(pmctf_gop.picture_hashes).parameters["bitdepth"].default == 8
    # refused before any tensor is looked at
    for level, b in (("u8", 10), ("u8", 16), ("u16", 8), ("md5", 8), ("md5", 10)):
        with pytest.raises(ValueError):
            pmctf_gop.picture_hashes([], H, W, level, b)
    with pytest.raises(ValueError):
        pmctf_gop.picture_hashes([], H, W, "u16")
    for b in (7, 17):
        with pytest.raises(ValueError):
            pmctf_gop.picture_hashes([], H, W, "f32", b)
    assert pmctf_gop.picture_hashes([], H, W, "u16", 10) == [] and pmctf_gop.picture_hashes([], H, W, "f32", 16) == []


def test_u16_hash_file_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    recs = [{k: int(rng.integers(0, 1 << 32)) for k in pmctf_gop.HASH_KEYS["u16"]} for _ in range(N)]
    pmctf_gop.write_picture_hashes(str(tmp_path), "u16", recs)
    got = pmctf_gop.read_picture_hashes(str(tmp_path), N)
    assert got == {"format_version": pmctf_gop.PICTURE_HASH_FORMAT_VERSION, "level": "u16", "frames": recs}
    assert pmctf_gop.PICTURE_HASH_FORMAT_VERSION == 1


def _tool():
    spec = importlib.util.spec_from_file_location("check_picture_hashes", os.path.join(ROOT, "tools", "check_picture_hashes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("level", ["u16", "f32"])
def test_check_tool_on_a_16_bit_sequence(tmp_path, capsys, level):
    rng = np.random.default_rng(7)
    data = rng.integers(0, 1 << B, N * (NY + 2 * NC) // 2, dtype=np.uint16).astype("<u2").tobytes()
    assert (NY + NC) % 4 == 2, "the Cr plane starts on a 2-byte boundary only"
    folder = str(tmp_path / "bins")
    os.makedirs(folder)
    pmctf_gop.write_sequence_header(folder, width=W, height=H, frame_num=N, gop=GOP, q_index=3, psize=128, me_downsample=1,
                                    num_me_stages=1, ll_order="plane", precision="exact", aten_threads=1)
    pmctf_gop.write_picture_format(folder, B)
    recs = []
    for i in range(N):
        f = data[i * (NY + 2 * NC):(i + 1) * (NY + 2 * NC)]
        rec = {"y": zlib.crc32(f[:NY]), "cb": zlib.crc32(f[NY:NY + NC]), "cr": zlib.crc32(f[NY + NC:]), "frame": zlib.crc32(f)}
        if level == "f32":
            rec.update(y_f32=i, c_f32=i + 1)
        recs.append(rec)
    pmctf_gop.write_picture_hashes(folder, level, recs)
    yuv = str(tmp_path / "dec.yuv")
    open(yuv, "wb").write(data)
    tool = _tool()
    assert tool.main([folder, yuv]) == 0
    assert f"all {N} frames match" in capsys.readouterr().out
    at = 2 * (NY + 2 * NC) + NY + NC + 7                              # frame 2, the high byte of a Cr sample
    bad = bytearray(data)
    bad[at] ^= 0x01
    open(yuv, "wb").write(bytes(bad))
    assert tool.main([folder, yuv]) == 1
    assert "frame 2, plane cr" in capsys.readouterr().out
    frames, mism = pmctf_gop.check_yuv_hashes(folder, yuv)
    assert frames == N and [(m["frame"], m["plane"]) for m in mism] == [(2, "cr"), (2, "frame")]
    # the same bytes read as an 8-bit folder have the wrong length: cannot be checked, not a pass
    os.remove(os.path.join(folder, "picture_format.json"))
    assert tool.main([folder, yuv]) == 2


# -------------------------------------------------------------------------------------------------------- signatures
def test_public_signatures():
    sig = inspect.signature(pmctf_gop.encode_sequence)
    p = sig.parameters
    assert p["bitdepth"].default == 8 and p["bitdepth"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    before = ["codec", "yuv_path", "width", "height", "frame_num", "gop", "q_index", "bin_folder", "device", "skip_decoding",
              "psize", "src_format", "ingest", "decoded_frame_path", "picture_hash", "keep_gops", "msssim"]
    assert [k for k in p if k != "bitdepth"] == before, "the existing parameters keep their order"
    assert list(p)[:15] == before[:15]
    for fn in (pmctf_gop.decode_sequence, ):
        assert list(inspect.signature(fn).parameters) == ["codec", "bin_folder", "yuv_out", "device", "png_out"]
    assert list(inspect.signature(pmctf_gop.decode_sequence_checked).parameters) == ["codec", "bin_folder", "yuv_out", "device",
                                                                                     "png_out", "verify"]
    q = inspect.signature(pmctf_gop.sequence_quality).parameters
    assert list(q) == ["src_yuv", "rec_yuv", "width", "height", "frame_num", "device", "gop", "msssim", "bitdepth"]
    assert q["bitdepth"].default == 8
    assert list(inspect.signature(pmctf_gop.frames_to_u16).parameters) == ["frames_rec", "pic_height", "pic_width", "bitdepth"]
    assert list(inspect.signature(pmctf_gop.gop_quality_hbd).parameters) == ["frames_rec", "frames_orig", "pic_height",
                                                                             "pic_width", "bitdepth"]
    from pMCTF.hip import ops
    assert list(inspect.signature(ops.planes_from_u16).parameters) == ["frame_u16", "h", "w", "bitdepth", "psize", "originals"]
    assert list(inspect.signature(ops.planes_to_u16).parameters) == ["x", "h", "w", "bitdepth"]
    assert list(inspect.signature(ops.frame_sse_hbd).parameters) == ["rec_y", "rec_c", "org_y", "org_c", "h", "w", "bitdepth"]


def test_encode_sequence_refusals_come_before_the_codec_is_touched(tmp_path):
    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError(f"the codec was touched ({name}) before the arguments were checked")

    args = (NoDevice(), str(tmp_path / "none.yuv"), W, H, N, GOP, 3, str(tmp_path), "cuda")
    for kw in ({"msssim": True}, {"decoded_frame_path": str(tmp_path / "png")}, {"src_format": "png"},
               {"picture_hash": "u8", "keep_gops": True}):
        with pytest.raises(ValueError, match="bitdepth 10"):
            pmctf_gop.encode_sequence(*args, bitdepth=10, **kw)
    with pytest.raises(ValueError, match="bitdepth 8"):
        pmctf_gop.encode_sequence(*args, picture_hash="u16", keep_gops=True)
    for b in (7, 17, "10"):
        with pytest.raises(ValueError, match="bitdepth"):
            pmctf_gop.encode_sequence(*args, bitdepth=b)
    assert os.listdir(tmp_path) == []
    y, c = torch.zeros((1, 1, 128, 128)), torch.zeros((2, 1, 64, 64))
    with pytest.raises(RuntimeError, match="GPU"):                    # no CPU fallback
        pmctf_gop.gop_quality_hbd([(y, c, None)], [(y, c)], 128, 128, 10)
    with pytest.raises(ValueError):
        pmctf_gop.gop_quality_hbd([(y, c, None)], [(y, c)], 128, 128, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        pmctf_gop.sequence_quality("a.yuv", "b.yuv", 128, 128, 1, "cpu", bitdepth=10)


# ---------------------------------------------------------------------------------------------------------- bindings
def test_entry_points_are_declared_bound_and_exported():
    from pMCTF.hip import lib
    text = open(os.path.join(ROOT, "include", "pmctf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(pmctf_\w+)\s*\(", text))
    L = C.CDLL(lib.HIP_SO)
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/pmctf_hip.h"
        assert s in lib.exported_symbols(), f"{s} has no ctypes signature in pMCTF/hip/lib.py"
        assert hasattr(L, s), f"libpmctf_hip.so does not export {s}"


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from pMCTF.hip import lib
    L = lib.hip()
    one = C.c_void_p(4096)                            # non-null, aligned, never dereferenced: the checks come first
    ingest, out, sse = (getattr(L, s) for s in SYMBOLS)
    # null pointers (the two originals of the ingest may be null, nothing else)
    for k in range(3):
        p = [one] * 3
        p[k] = None
        assert ingest(p[0], p[1], p[2], one, one, 128, 128, 100, 100, 10, None) == -1, k
    for k in range(2):
        p = [one] * 2
        p[k] = None
        assert out(p[0], p[1], 1, 128, 128, 100, 100, 10, None) == -1, k
    for k in range(5):
        p = [one] * 5
        p[k] = None
        assert sse(p[0], p[1], p[2], p[3], 128, 128, 100, 100, 10, p[4], None) == -1, k
    # sizes: the two that take whole 4:2:0 pictures want even ones; all three want positive ones up to 16384
    for h, w in ((99, 100), (100, 99), (1, 1)):
        assert ingest(one, one, one, one, one, 16384, 16384, h, w, 10, None) == -1, (h, w)
        assert ingest(one, one, one, None, None, 16384, 16384, h, w, 10, None) == -1, (h, w)
        assert sse(one, one, one, one, 16384, 16384, h, w, 10, one, None) == -1, (h, w)
    for h, w in ((0, 100), (100, 0), (-2, 100), (100, -2), (16386, 100), (100, 16386)):
        assert ingest(one, one, one, one, one, 16384, 16384, h, w, 10, None) == -1, (h, w)
        assert out(one, one, 1, 16384, 16384, h, w, 10, None) == -1, (h, w)
        assert sse(one, one, one, one, 16384, 16384, h, w, 10, one, None) == -1, (h, w)
    assert out(one, one, 0, 128, 128, 100, 100, 10, None) == -1
    for Hp, Wp in ((98, 128), (128, 98), (127, 128), (128, 127), (16386, 128)):          # smaller than the picture, odd, too large
        assert ingest(one, one, one, one, one, Hp, Wp, 100, 100, 10, None) == -1, (Hp, Wp)
        assert sse(one, one, one, one, Hp, Wp, 100, 100, 10, one, None) == -1, (Hp, Wp)
    for Hp, Wp in ((98, 128), (128, 98), (16386, 128)):
        assert out(one, one, 1, Hp, Wp, 100, 100, 10, None) == -1, (Hp, Wp)
    for b in (8, 17, 0, -1):
        assert ingest(one, one, one, one, one, 128, 128, 100, 100, b, None) == -1, b
        assert out(one, one, 1, 128, 128, 100, 100, b, None) == -1, b
        assert sse(one, one, one, one, 128, 128, 100, 100, b, one, None) == -1, b
    # a pointer less aligned than its element type (and the padded outputs' 16 bytes, as in the 8-bit ingest)
    odd = lambda n: C.c_void_p(4096 + n)
    assert ingest(odd(1), one, one, one, one, 128, 128, 100, 100, 10, None) == -1
    assert ingest(one, odd(4), one, one, one, 128, 128, 100, 100, 10, None) == -1
    assert ingest(one, one, odd(8), one, one, 128, 128, 100, 100, 10, None) == -1
    assert ingest(one, one, one, odd(2), one, 128, 128, 100, 100, 10, None) == -1
    assert ingest(one, one, one, one, odd(2), 128, 128, 100, 100, 10, None) == -1
    assert out(odd(2), one, 1, 128, 128, 100, 100, 10, None) == -1
    assert out(one, odd(1), 1, 128, 128, 100, 100, 10, None) == -1
    for k in range(4):
        p = [one] * 4
        p[k] = odd(2)
        assert sse(p[0], p[1], p[2], p[3], 128, 128, 100, 100, 10, one, None) == -1, k
    assert sse(one, one, one, one, 128, 128, 100, 100, 10, odd(4), None) == -1


def test_wrappers_check_their_arguments_before_any_launch():
    from pMCTF.hip import ops
    frame = torch.zeros(100 * 100 * 3 // 2, dtype=torch.uint16)
    for h, w in ((99, 100), (100, 99), (0, 100), (100, 102)):
        with pytest.raises(ValueError):
            ops.planes_from_u16(frame, h, w, 10)
    for b in (8, 17):
        with pytest.raises(ValueError):
            ops.planes_from_u16(frame, 100, 100, b)
    with pytest.raises(ValueError):
        ops.planes_from_u16(torch.zeros(15000, dtype=torch.uint8), 100, 100, 10)
    with pytest.raises(ValueError):
        ops.planes_from_u16(frame, 100, 100, 10, psize=3)
    with pytest.raises(RuntimeError):                 # no CPU fallback
        ops.planes_from_u16(frame, 100, 100, 10)
    y, c = torch.zeros((1, 1, 128, 128)), torch.zeros((2, 1, 64, 64))
    for h, w in ((0, 100), (100, -2), (130, 100), (100, 130)):
        with pytest.raises(ValueError):
            ops.planes_to_u16(y, h, w, 10)
    with pytest.raises(ValueError):
        ops.planes_to_u16(y, 100, 100, 8)
    with pytest.raises(ValueError):
        ops.planes_to_u16(y.double(), 100, 100, 10)
    with pytest.raises(RuntimeError):
        ops.planes_to_u16(y, 100, 100, 10)
    oy, oc = torch.zeros((1, 1, 100, 100)), torch.zeros((2, 1, 50, 50))
    for h, w in ((99, 100), (100, 99), (0, 100), (130, 100)):
        with pytest.raises(ValueError):
            ops.frame_sse_hbd(y, c, oy, oc, h, w, 10)
    with pytest.raises(ValueError):
        ops.frame_sse_hbd(y, c, oy, torch.zeros((2, 1, 50, 48)), 100, 100, 10)
    with pytest.raises(ValueError):
        ops.frame_sse_hbd(y, c, oy, oc, 100, 100, 17)
    with pytest.raises(RuntimeError):
        ops.frame_sse_hbd(y, c, oy, oc, 100, 100, 10)
    assert ops.psnr_from_sse_hbd(0, 100, 10) == float("inf")
    assert ops.psnr_from_sse_hbd(1023 ** 2 * 100, 100, 10) == 0.0
