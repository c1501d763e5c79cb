"""Picture hashes, the parts that need no GPU: crc32_combine against zlib, the strict reader and writer of
picture_hashes.json, tools/check_picture_hashes.py on a synthetic file, and the argument check of encode_sequence.  The
yardstick is zlib.crc32; everything is exact."""
import importlib.util
import json
import os
import zlib

import numpy as np
import pytest

import pmctf_gop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N, GOP = 6, 10, 4, 2                                # chroma planes of 5x3 = 15 bytes: Cr starts at an odd offset
NY, NC = W * H, (W // 2) * (H // 2)


def _tool():
    spec = importlib.util.spec_from_file_location("check_picture_hashes", os.path.join(ROOT, "tools", "check_picture_hashes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("len_b", [0, 1, 3, 4, 5, 4095, 4096, 4097, (1 << 20) + 3])
def test_crc32_combine_equals_zlib_of_the_concatenation(len_b):
    rng = np.random.default_rng(len_b)
    b = rng.integers(0, 256, len_b, dtype=np.uint8).tobytes()
    for len_a in (0, 1, 7, 1000):
        a = rng.integers(0, 256, len_a, dtype=np.uint8).tobytes()
        assert pmctf_gop.crc32_combine(zlib.crc32(a), zlib.crc32(b), len_b) == zlib.crc32(a + b)
    # three planes into a frame, as picture_hashes does it
    y = rng.integers(0, 256, 77, dtype=np.uint8).tobytes()
    frame = pmctf_gop.crc32_combine(pmctf_gop.crc32_combine(zlib.crc32(y), zlib.crc32(b), len_b), zlib.crc32(b[::-1]), len_b)
    assert frame == zlib.crc32(y + b + b[::-1])


def _records(level, n=N, seed=0):
    rng = np.random.default_rng(seed)
    return [{k: int(rng.integers(0, 1 << 32)) for k in pmctf_gop.HASH_KEYS[level]} for _ in range(n)]


@pytest.mark.parametrize("level", ["u8", "f32"])
def test_hash_file_round_trip(tmp_path, level):
    recs = _records(level)
    recs[0]["y"], recs[1]["frame"] = 0, 0xffffffff                    # the ends of the value range
    path = pmctf_gop.write_picture_hashes(str(tmp_path), level, recs)
    assert path == os.path.join(str(tmp_path), "picture_hashes.json") and os.listdir(tmp_path) == ["picture_hashes.json"]
    got = pmctf_gop.read_picture_hashes(str(tmp_path), N)
    assert got == {"format_version": pmctf_gop.PICTURE_HASH_FORMAT_VERSION, "level": level, "frames": recs}


def test_malformed_hash_files_are_refused_by_path(tmp_path):
    folder = str(tmp_path)
    path = os.path.join(folder, "picture_hashes.json")
    with pytest.raises(ValueError) as e:
        pmctf_gop.read_picture_hashes(folder, N)
    assert path in str(e.value) and "missing" in str(e.value)
    pmctf_gop.write_picture_hashes(folder, "u8", _records("u8"))
    good = json.load(open(path))

    def refused(record, n=N):
        json.dump(record, open(path, "w"))
        with pytest.raises(ValueError) as e:
            pmctf_gop.read_picture_hashes(folder, n)
        assert path in str(e.value)
        return str(e.value)

    assert "version" in refused(dict(good, format_version=good["format_version"] + 1))
    assert "version" in refused({k: v for k, v in good.items() if k != "format_version"})
    assert "frame records" in refused(dict(good, frames=good["frames"][:-1]))                 # short frame list
    assert "frame records" in refused(good, n=N + 1)
    assert "level" in refused(dict(good, level="md5"))
    assert "frame 1" in refused(dict(good, frames=[good["frames"][0], {"y": 1}] + good["frames"][2:]))
    assert "frame 0" in refused(dict(good, frames=[dict(good["frames"][0], y=1 << 32)] + good["frames"][1:]))
    assert "frame 0" in refused(dict(good, level="f32"))                                       # u8 records under level f32
    open(path, "w").write("{")
    with pytest.raises(ValueError, match="not a picture hash file"):
        pmctf_gop.read_picture_hashes(folder, N)
    # the writer holds its records to the same form
    with pytest.raises(ValueError, match="level"):
        pmctf_gop.write_picture_hashes(folder, "sha", _records("u8"))
    with pytest.raises(ValueError, match="frame 0"):
        pmctf_gop.write_picture_hashes(folder, "u8", _records("f32"))


def _synthetic_sequence(tmp_path, level="u8"):
    """a folder with a header and a hash file computed with zlib from a random .yuv -> (folder, yuv path, its bytes)"""
    rng = np.random.default_rng(7)
    data = rng.integers(0, 256, N * (NY + 2 * NC), dtype=np.uint8).tobytes()
    folder = str(tmp_path / "bins")
    os.makedirs(folder)
    pmctf_gop.write_sequence_header(folder, width=W, height=H, frame_num=N, gop=GOP, q_index=3, psize=128, me_downsample=1,
                                    num_me_stages=1, ll_order="plane", precision="exact", aten_threads=1)
    recs = []
    for i in range(N):
        f = data[i * (NY + 2 * NC):(i + 1) * (NY + 2 * NC)]
        rec = {"y": zlib.crc32(f[:NY]), "cb": zlib.crc32(f[NY:NY + NC]), "cr": zlib.crc32(f[NY + NC:]), "frame": zlib.crc32(f)}
        if level == "f32":
            rec.update(y_f32=i, c_f32=i + 1)                       # not checkable from a .yuv: the tool must not look
        recs.append(rec)
    pmctf_gop.write_picture_hashes(folder, level, recs)
    yuv = str(tmp_path / "dec.yuv")
    open(yuv, "wb").write(data)
    return folder, yuv, data


@pytest.mark.parametrize("level", ["u8", "f32"])
def test_check_tool_passes_and_names_a_flipped_byte(tmp_path, capsys, level):
    tool = _tool()
    folder, yuv, data = _synthetic_sequence(tmp_path, level)
    assert tool.main([folder, yuv]) == 0
    assert f"all {N} frames match" in capsys.readouterr().out
    at = 2 * (NY + 2 * NC) + NY + 11                                # frame 2, a byte of the Cb plane
    bad = bytearray(data)
    bad[at] ^= 0x10
    open(yuv, "wb").write(bytes(bad))
    assert tool.main([folder, yuv]) == 1
    out = capsys.readouterr().out
    assert "frame 2, plane cb" in out and f"{zlib.crc32(bytes(bad[at - 11:at - 11 + NC])):#010x}" in out
    frames, mism = pmctf_gop.check_yuv_hashes(folder, yuv)
    assert frames == N and [(m["frame"], m["plane"]) for m in mism] == [(2, "cb"), (2, "frame")]
    # a file of another length, or a folder without hashes, cannot be checked: status 2, not a pass
    open(yuv, "wb").write(data[:-1])
    assert tool.main([folder, yuv]) == 2
    os.remove(os.path.join(folder, "picture_hashes.json"))
    open(yuv, "wb").write(data)
    assert tool.main([folder, yuv]) == 2
    assert "picture_hashes.json" in capsys.readouterr().err


def test_encode_sequence_refuses_hashes_without_gop_folders(tmp_path):
    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError(f"the codec was touched ({name}) before the arguments were checked")

    args = (NoDevice(), str(tmp_path / "none.yuv"), W, H, N, GOP, 3, str(tmp_path), "cuda")
    with pytest.raises(ValueError, match="keep_gops"):
        pmctf_gop.encode_sequence(*args, picture_hash="u8", keep_gops=False)
    with pytest.raises(ValueError, match="picture_hash"):
        pmctf_gop.encode_sequence(*args, picture_hash="md5", keep_gops=True)
    assert os.listdir(tmp_path) == []


def test_decode_sequence_refuses_an_unknown_verify_mode(tmp_path):
    with pytest.raises(ValueError, match="verify"):
        pmctf_gop.decode_sequence_checked(None, str(tmp_path), str(tmp_path / "o.yuv"), verify="maybe")
    assert issubclass(pmctf_gop.PictureHashMismatch, ValueError)
    m = {"gop": 1, "folder": "bins/gop_00001", "frame": 5, "plane": "cr", "decoded": 0x1234, "recorded": 0xfedcba98}
    text = str(pmctf_gop.PictureHashMismatch(m))
    assert all(s in text for s in ("bins/gop_00001", "frame 5", "plane cr", "0x00001234", "0xfedcba98"))
