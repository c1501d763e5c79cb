"""Picture hashes on the GPU: pmctf_crc32_segments (csrc/picture_hash.hip) against zlib.crc32 of the same bytes copied to
the host, and the hashes through a sequence: written by encode_sequence, verified by decode_sequence / decode_sequence_checked in another model.
zlib.crc32 is exact, so every comparison is for equality."""
import ctypes as C
import importlib.util
import json
import os
import shutil
import zlib

import numpy as np
import pytest
import torch

from helpers import product_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096                                            # one workgroup tile: 256 threads x 16 bytes
LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 1, (1 << 20) + 3]
OFFSETS = list(range(18))                              # start of a range inside a 16-byte aligned buffer
CONTENTS = ["zeros", "ones", "random", "first_bit", "last_bit"]


def _layout():
    """(start, length) of every LENGTHS x OFFSETS range in one buffer: each in a 16-byte aligned region of its own"""
    at, ranges = 0, []
    for n in LENGTHS:
        for off in OFFSETS:
            ranges.append((at + off, n))
            at += (off + n + 15) // 16 * 16 + 16
    return ranges, at


@pytest.fixture(scope="module")
def buffers(cuda):
    """per content: (device buffer, ranges, zlib.crc32 of every range from the host copy).  The bytes between the ranges
    are random, so that a byte read from outside a range changes the value."""
    from pMCTF.hip import ops
    assert ops.CRC32_TILE_BYTES == TILE
    ranges, total = _layout()
    out = {}
    for ci, content in enumerate(CONTENTS):
        host = np.random.default_rng(ci).integers(0, 256, total, dtype=np.uint8)
        for start, n in ranges:
            if content == "zeros":
                host[start:start + n] = 0
            elif content == "ones":
                host[start:start + n] = 0xff
            elif content == "first_bit" and n:
                host[start:start + n] = 0
                host[start] = 0x01
            elif content == "last_bit" and n:
                host[start:start + n] = 0
                host[start + n - 1] = 0x80
        dev = torch.from_numpy(host).to(cuda)
        assert dev.data_ptr() % 16 == 0
        back = dev.cpu().numpy()
        want = [zlib.crc32(back[start:start + n].tobytes()) for start, n in ranges]
        out[content] = (dev, ranges, want)
    return out


def _report(ranges, got, want):
    bad = [(n, start % 16, f"{g:#010x}", f"{w:#010x}") for (start, n), g, w in zip(ranges, got, want) if g != w]
    return f"{len(bad)} of {len(want)} ranges differ; (length, offset, device, zlib) of the first: {bad[:5]}"


@pytest.mark.parametrize("content", CONTENTS)
def test_kernel_equals_zlib_over_lengths_offsets_and_contents(buffers, content):
    from pMCTF.hip import ops
    dev, ranges, want = buffers[content]
    got = ops.crc32([dev[start:start + n] for start, n in ranges])
    assert len(got) == len(LENGTHS) * len(OFFSETS) and all(isinstance(v, int) for v in got)
    assert got == want, _report(ranges, got, want)
    assert all(g == 0 for (_, n), g in zip(ranges, got) if n == 0)


@pytest.mark.parametrize("slices", [1, 2, 7, 64, 1024])
def test_launch_shape_does_not_change_the_values(buffers, slices):
    from pMCTF.hip import ops
    dev, ranges, want = buffers["random"]
    got = ops.crc32([dev[start:start + n] for start, n in ranges], slices=slices)
    assert got == want, _report(ranges, got, want)


def test_one_call_with_mixed_segments_dtypes_and_empty_ones(cuda):
    from pMCTF.hip import ops
    rng = np.random.default_rng(11)
    big = torch.from_numpy(rng.integers(0, 256, 1 << 20, dtype=np.uint8)).to(cuda)
    tensors, at = [], 0
    for i in range(44):
        n = [0, 1, 7, 31, 100, 4095, 4097, 9000, 20001][i % 9]
        off = int(rng.integers(0, 18))
        tensors.append(big[at + off:at + off + n])
        at += off + n + int(rng.integers(0, 40))
    assert at <= big.numel() and sum(t.numel() == 0 for t in tensors) >= 2
    tensors.append(torch.empty(0, dtype=torch.float32, device=cuda))                   # no storage at all
    tensors.append(torch.from_numpy(rng.standard_normal((3, 5, 7))).to(cuda))          # float64
    tensors.append(torch.from_numpy(rng.integers(-30000, 30000, 1001, dtype=np.int16)).to(cuda))
    tensors.append(torch.from_numpy(rng.integers(0, 256, (2, 5, 3), dtype=np.uint8)).to(cuda)[1])   # plane 1: an odd start
    assert tensors[-1].data_ptr() % 2 == 1
    want = [zlib.crc32(t.cpu().numpy().tobytes()) for t in tensors]
    got = ops.crc32(tensors)
    assert len(got) == 48 and got == want
    assert ops.crc32([]) == []


def test_float_tensor_is_hashed_as_stored_and_repeats(cuda):
    from pMCTF.hip import ops
    g = torch.Generator(device="cpu").manual_seed(3)
    t = (torch.rand((2, 1, 64, 128), generator=g) * 280.0 - 12.0).to(cuda)
    want = zlib.crc32(t.cpu().numpy().tobytes())
    first = ops.crc32([t, t[1], t[0, 0, 1:]])
    assert first[0] == want
    assert first[1:] == [zlib.crc32(t[1].cpu().numpy().tobytes()), zlib.crc32(t[0, 0, 1:].cpu().numpy().tobytes())]
    assert ops.crc32([t, t[1], t[0, 0, 1:]]) == first                                  # the same bits on every run


def test_output_guards_and_refused_arguments(buffers, cuda):
    from pMCTF.hip import lib, ops
    dev, ranges, want = buffers["random"]
    pick = list(range(0, len(ranges), 7))
    tensors = [dev[ranges[i][0]:ranges[i][0] + ranges[i][1]] for i in pick]
    S, guard = len(tensors), 5
    out = torch.full((S + 2 * guard,), 0x5a5a5a5a, dtype=torch.int32, device=cuda)
    got = ops.crc32(tensors, out=out[guard:guard + S])
    assert got == [want[i] for i in pick]
    host = out.cpu().numpy()
    assert (host[:guard] == 0x5a5a5a5a).all() and (host[guard + S:] == 0x5a5a5a5a).all()
    assert [int(v) & 0xffffffff for v in host[guard:guard + S]] == got
    # the wrapper's refusals
    with pytest.raises(ValueError, match="contiguous"):
        ops.crc32([torch.zeros((4, 4), device=cuda).t()])
    with pytest.raises(ValueError, match="device"):
        ops.crc32([torch.zeros(4)])
    # the library's, before any launch: the output stays as it was
    L = lib.hip()
    segs = torch.tensor([dev.data_ptr(), 16], dtype=torch.int64).to(cuda)
    o = C.c_void_p(out.data_ptr())
    s = C.c_void_p(segs.data_ptr())
    assert L.pmctf_crc32_segments(None, 1, 0, o, None) == -1
    assert L.pmctf_crc32_segments(s, 1, 0, None, None) == -1
    assert L.pmctf_crc32_segments(s, 1, 0, C.c_void_p(out.data_ptr() + 2), None) == -1
    assert L.pmctf_crc32_segments(C.c_void_p(segs.data_ptr() + 4), 1, 0, o, None) == -1
    assert L.pmctf_crc32_segments(s, -1, 0, o, None) == -1
    assert L.pmctf_crc32_segments(s, 65536, 0, o, None) == -1
    assert L.pmctf_crc32_segments(s, 1, 1025, o, None) == -1
    assert L.pmctf_crc32_segments(s, 1, -1, o, None) == -1
    assert L.pmctf_crc32_segments(None, 0, 0, None, None) == 0                         # nothing to do
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == host).all()


# ------------------------------------------------------------------------------------------------------------- sequence
W, H, GOP, N, Q = 132, 100, 4, 8, 3                     # the round trip's case: padded to 256x128, chroma rows of 66 bytes
FRAME_BYTES = W * H + 2 * (W // 2) * (H // 2)


def _listing(folder):
    return sorted(os.path.relpath(os.path.join(d, f), folder) for d, _, fs in os.walk(folder) for f in fs)


@pytest.fixture(scope="module")
def coded(cuda, tmp_path_factory):
    """the sequence coded twice by one model, with picture_hash="f32" and without, and a decoder model of its own"""
    import pmctf_gop
    import pmctf_synth
    tmp = tmp_path_factory.mktemp("picture_hash")
    src = str(tmp / "src.yuv")
    pmctf_gop.write_yuv(src, pmctf_synth.synth_yuv420(W, H, N, seed=5))
    enc_net, _ = product_model(1)
    out = {"tmp": tmp}
    for name, level in (("hashed", "f32"), ("plain", None)):
        bins = str(tmp / name)
        os.makedirs(bins)
        out[name + "_enc"] = pmctf_gop.encode_sequence(enc_net, src, W, H, N, GOP, Q, bins, "cuda", keep_gops=True,
                                                       picture_hash=level)
        out[name] = bins
    del enc_net
    out["dec_net"], _ = product_model(1)
    # both GOPs' files in each other's folder: every stream is intact and decodes, to the other GOP's pictures
    swapped = str(tmp / "swapped")
    shutil.copytree(out["hashed"], swapped)
    for a, b in (("gop_00000", "x"), ("gop_00001", "gop_00000"), ("x", "gop_00001")):
        os.rename(os.path.join(swapped, a), os.path.join(swapped, b))
    out["swapped"] = swapped
    return out


def test_hashed_sequence_verifies_in_another_model(coded):
    import pmctf_gop
    bins = coded["hashed"]
    assert sorted(os.listdir(bins)) == ["gop_00000", "gop_00001", "picture_hashes.json", "sequence.json"]
    recorded = pmctf_gop.read_picture_hashes(bins, N)
    assert recorded["level"] == "f32" and recorded["frames"] == coded["hashed_enc"]["picture_hashes"]
    assert all(set(r) == {"y", "cb", "cr", "frame", "y_f32", "c_f32"} for r in recorded["frames"])
    yuv = str(coded["tmp"] / "hashed.yuv")
    res = pmctf_gop.decode_sequence_checked(coded["dec_net"], bins, yuv, "cuda", verify=True)
    # a mismatch of y_f32 / c_f32 alone here would be a finding about the decoder's bit-exactness, not a test to loosen
    assert res["hash_mismatches"] == [] and res["verified"] == N and res["frames"] == [(H, W)] * N
    data = open(yuv, "rb").read()
    assert len(data) == N * FRAME_BYTES
    ny, nc = W * H, (W // 2) * (H // 2)
    for i, rec in enumerate(recorded["frames"]):
        f = data[i * FRAME_BYTES:(i + 1) * FRAME_BYTES]
        assert rec["frame"] == zlib.crc32(f), f"frame {i}"
        assert (rec["y"], rec["cb"], rec["cr"]) == (zlib.crc32(f[:ny]), zlib.crc32(f[ny:ny + nc]), zlib.crc32(f[ny + nc:]))
    spec = importlib.util.spec_from_file_location("check_picture_hashes", os.path.join(ROOT, "tools", "check_picture_hashes.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.main([bins, yuv]) == 0
    coded["hashed_yuv"] = data


def test_default_path_is_unchanged(coded):
    import pmctf_gop
    bins = coded["plain"]
    assert sorted(os.listdir(bins)) == ["gop_00000", "gop_00001", "sequence.json"]
    for k in range(N // GOP):
        assert sorted(os.listdir(os.path.join(bins, f"gop_{k:05d}"))) == sorted(pmctf_gop.gop_file_names(GOP))
    assert "picture_hashes" not in coded["plain_enc"]
    # hashing adds one file and changes no other
    assert [p for p in _listing(coded["hashed"]) if p != "picture_hashes.json"] == _listing(bins)
    for p in _listing(bins):
        if p != "sequence.json":
            assert open(os.path.join(bins, p), "rb").read() == open(os.path.join(coded["hashed"], p), "rb").read(), p
    assert pmctf_gop.read_sequence_header(bins) == pmctf_gop.read_sequence_header(coded["hashed"])
    yuv = str(coded["tmp"] / "plain.yuv")
    res = pmctf_gop.decode_sequence(coded["dec_net"], bins, yuv, "cuda")
    assert res["verified"] == 0 and res["hash_mismatches"] == [] and res["frames"] == [(H, W)] * N
    if "hashed_yuv" not in coded:
        hashed = str(coded["tmp"] / "hashed_again.yuv")
        pmctf_gop.decode_sequence_checked(coded["dec_net"], coded["hashed"], hashed, "cuda", verify=False)
        coded["hashed_yuv"] = open(hashed, "rb").read()
    assert open(yuv, "rb").read() == coded["hashed_yuv"]
    with pytest.raises(ValueError, match="picture_hashes.json"):
        pmctf_gop.decode_sequence_checked(coded["dec_net"], bins, str(coded["tmp"] / "no.yuv"), "cuda", verify=True)


def test_swapped_gops_are_caught_before_anything_of_the_gop_is_written(coded):
    import pmctf_gop
    yuv = str(coded["tmp"] / "swapped_default.yuv")
    with pytest.raises(pmctf_gop.PictureHashMismatch) as e:
        pmctf_gop.decode_sequence(coded["dec_net"], coded["swapped"], yuv, "cuda")
    m = e.value.mismatch
    assert isinstance(e.value, ValueError) and (m["gop"], m["frame"]) == (0, 0) and m["plane"] in ("y", "cb", "cr")
    text = str(e.value)
    assert os.path.join(coded["swapped"], "gop_00000") in text and "frame 0, plane " + m["plane"] in text
    assert f"{m['decoded']:#010x}" in text and f"{m['recorded']:#010x}" in text and m["decoded"] != m["recorded"]
    assert os.path.getsize(yuv) == 0


def test_swapped_gops_report_and_no_verify(coded):
    import pmctf_gop
    recorded = pmctf_gop.read_picture_hashes(coded["swapped"], N)["frames"]
    yuv = str(coded["tmp"] / "swapped_report.yuv")
    res = pmctf_gop.decode_sequence_checked(coded["dec_net"], coded["swapped"], yuv, "cuda", verify="report")
    assert res["verified"] == N and len(res["frames"]) == N and os.path.getsize(yuv) == N * FRAME_BYTES
    assert {m["gop"] for m in res["hash_mismatches"]} == {0, 1}
    assert {m["frame"] for m in res["hash_mismatches"]} == set(range(N))
    # what was written is the other GOP's pictures: frame i of the file hashes to the record of frame (i + GOP) % N
    data = open(yuv, "rb").read()
    for i in range(N):
        assert zlib.crc32(data[i * FRAME_BYTES:(i + 1) * FRAME_BYTES]) == recorded[(i + GOP) % N]["frame"]
    silent = str(coded["tmp"] / "swapped_silent.yuv")
    res = pmctf_gop.decode_sequence_checked(coded["dec_net"], coded["swapped"], silent, "cuda", verify=False)
    assert res["verified"] == 0 and res["hash_mismatches"] == [] and open(silent, "rb").read() == data


def test_one_altered_float_hash_is_named(coded):
    import pmctf_gop
    bins = str(coded["tmp"] / "altered")
    shutil.copytree(coded["hashed"], bins)
    path = os.path.join(bins, "picture_hashes.json")
    record = json.load(open(path))
    want = record["frames"][5]["y_f32"]
    record["frames"][5]["y_f32"] = want ^ 1
    json.dump(record, open(path, "w"))
    yuv = str(coded["tmp"] / "altered.yuv")
    with pytest.raises(pmctf_gop.PictureHashMismatch, match="frame 5, plane y_f32") as e:
        pmctf_gop.decode_sequence(coded["dec_net"], bins, yuv, "cuda")
    assert e.value.mismatch == {"gop": 1, "folder": os.path.join(bins, "gop_00001"), "frame": 5, "plane": "y_f32",
                                "decoded": want, "recorded": want ^ 1}
    assert os.path.getsize(yuv) == GOP * FRAME_BYTES                 # GOP 0 was written, nothing of GOP 1
    res = pmctf_gop.decode_sequence_checked(coded["dec_net"], bins, yuv, "cuda", verify="report")
    assert [(m["frame"], m["plane"]) for m in res["hash_mismatches"]] == [(5, "y_f32")]     # its u8 entries still match
