"""High-bit-depth 4:2:0 sources on the GPU: the uint16_t ingest and output of csrc/picture_ops.hip and the error sums of csrc/picture_hbd.hip against tests/hbd_restatement.py
(numpy), and the drivers end to end at 132x100 (padded to 256x128), GOP 4, 8 frames.

Everything is exact, bit for bit and byte for byte; the one tolerance is 1e-9 dB on a PSNR against its own formula, a
bound on float64 log10 differences between libraries.  The parity anchor ties the new path to the 8-bit one: a 10-bit source
whose samples are all multiples of 4 codes to exactly the files of the 8-bit source v >> 2."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import hbd_restatement as hr
from helpers import product_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTHS = (9, 10, 12, 16)
GUARD = 64                                            # floats / samples on either side of every output (256 / 128 bytes)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _guarded(numel, dtype, dev, fill, offset=0):
    """(whole buffer, the view of numel elements that starts GUARD + offset elements in)"""
    np_dtype = np.uint16 if dtype == torch.uint16 else np.float32
    buf = torch.from_numpy(np.full(numel + 2 * GUARD + offset, fill, dtype=np_dtype)).to(dev)
    return buf, buf[GUARD + offset:GUARD + offset + numel]


def _guards_untouched(buf, numel, fill, offset=0):
    host = buf.cpu().numpy()
    return bool((host[:GUARD + offset] == fill).all()) and bool((host[GUARD + offset + numel:] == fill).all())


def _picture(h, w, b, seed, above_max=False):
    rng = np.random.default_rng(seed)
    frame = rng.integers(0, 1 << (16 if above_max else b), h * w * 3 // 2, dtype=np.uint16)
    frame[0], frame[1], frame[h * w], frame[-1] = 0, (1 << b) - 1, (1 << b) - 1, 0
    return frame


# ------------------------------------------------------------------------------------------------------------ 1. ingest
SIZES = [(6, 10, 2), (10, 6, 2), (18, 34, 16), (100, 132, 128), (130, 258, 128)]


@pytest.mark.parametrize("b", DEPTHS)
@pytest.mark.parametrize("h,w,psize", SIZES)
def test_ingest_equals_the_restatement_at_every_source_alignment(cuda, tmp_path, h, w, psize, b):
    import pmctf_gop
    from pMCTF.hip import lib, ops
    from pMCTF.utils.yuv_reader import YUVReader
    frame = _picture(h, w, b, seed=h * 1000 + w + b)
    want = hr.to_planes(frame, h, w, b, psize)
    if (h, w) == (6, 10):
        assert (2 * (h * w + (h // 2) * (w // 2))) % 4 == 2, "the Cr plane starts on a 2-byte boundary only (byte 150)"
    # the host path gives the same tensors
    path = str(tmp_path / "one.yuv")
    frame.tofile(path)
    reader = YUVReader(path, w, h, bitdepth=b)
    padded, orig, _ = pmctf_gop.read_gop(reader, 1, "cpu", psize)
    reader.close()
    for a, e in zip((padded[0][0], padded[0][1], orig[0][0], orig[0][1]), want):
        assert np.array_equal(a.numpy(), e)
    Hp, Wp = want[0].shape[-2:]
    L = lib.hip()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = frame.size
    fill = -7.0
    for off in range(4):                              # the source starts 0, 2, 4 or 6 bytes past a multiple of 8
        big = torch.from_numpy(np.concatenate((np.zeros(off, np.uint16), frame, np.zeros(8 - off, np.uint16)))).to(cuda)
        assert big.data_ptr() % 8 == 0
        src = big[off:off + n]
        assert src.data_ptr() % 8 == 2 * off
        for with_org in (True, False):
            bufs = [_guarded(e.size, torch.float32, cuda, fill) for e in want]
            views = [v for _, v in bufs]
            assert all(v.data_ptr() % 16 == 0 for v in views[:2])
            rc = L.pmctf_yuv420_u16_to_planes_f32(_ptr(src), _ptr(views[0]), _ptr(views[1]),
                                                  _ptr(views[2]) if with_org else None,
                                                  _ptr(views[3]) if with_org else None, Hp, Wp, h, w, b, stream)
            assert rc == 0
            for k, ((buf, v), e) in enumerate(zip(bufs, want)):
                if k < 2 or with_org:
                    got = v.cpu().numpy().reshape(e.shape)
                    diff = np.argwhere(got != e)
                    assert diff.size == 0, (off, with_org, k, diff[0], got[tuple(diff[0])], e[tuple(diff[0])])
                else:
                    assert bool((v.cpu().numpy() == fill).all()), "null originals: nothing written"
                assert _guards_untouched(buf, e.size, fill), (off, with_org, k)
        got = ops.planes_from_u16(src, h, w, b, psize=psize)
        for a, e in zip(got, want):
            assert a.dtype == torch.float32 and a.is_cuda and tuple(a.shape) == e.shape and np.array_equal(a.cpu().numpy(), e)
    only = ops.planes_from_u16(torch.from_numpy(frame).to(cuda), h, w, b, psize=psize, originals=False)
    assert only[2] is None and only[3] is None and np.array_equal(only[0].cpu().numpy(), want[0])


def test_ingest_converts_samples_above_max_as_they_are(cuda):
    from pMCTF.hip import ops
    h, w, b = 18, 34, 10
    frame = _picture(h, w, b, seed=3, above_max=True)
    assert int(frame.max()) > 1023
    want = hr.to_planes(frame, h, w, b, 16)
    got = ops.planes_from_u16(torch.from_numpy(frame).to(cuda), h, w, b, psize=16)
    assert all(np.array_equal(a.cpu().numpy(), e) for a, e in zip(got, want))
    assert float(got[2].max()) > 255.75


def test_read_gop_device_equals_read_gop(cuda, tmp_path):
    import pmctf_gop
    from pMCTF.utils.yuv_reader import YUVReader
    w, h, n, b = 34, 18, 3, 12
    path = str(tmp_path / "src.yuv")
    pmctf_gop.write_yuv(path, hr.synth_hbd(w, h, n, b, seed=3))
    for psize in (128, 2):
        r = YUVReader(path, w, h, bitdepth=b)
        want = pmctf_gop.read_gop(r, n, "cpu", psize)
        r.close()
        r = YUVReader(path, w, h, bitdepth=b)
        got = pmctf_gop.read_gop_device(r, n, cuda, psize)
        r.close()
        assert got[2] == want[2] == (h, w)
        for k in range(n):
            for part in (0, 1):
                for a, e in zip(got[part][k], want[part][k]):
                    assert a.is_cuda and a.dtype == e.dtype and tuple(a.shape) == tuple(e.shape)
                    assert torch.equal(a.cpu(), e), (psize, k, part)


# ------------------------------------------------------------------------------------------------------------ 2. output
def _reconstruction(N, Hp, Wp, h, w, b):
    """uniform in [-40, 300]; inside the crop exact ties (k + 0.5) 2^-s and the special values"""
    s = b - 8
    g = torch.Generator().manual_seed(N * 11 + Hp * 7 + Wp * 5 + h * 3 + w + b)
    x = torch.rand((N, 1, Hp, Wp), generator=g) * 340.0 - 40.0
    top = float((1 << b) - 1) * 2.0 ** -s
    special = [float("nan"), float("inf"), float("-inf"), -0.0, top, float(np.nextafter(np.float32(top), np.float32(1e9))),
               top + 2.0 ** -s, (0.5) * 2.0 ** -s, (1.5) * 2.0 ** -s, (2.5) * 2.0 ** -s, -0.5 * 2.0 ** -s,
               (float((1 << b) - 2) + 0.5) * 2.0 ** -s, (float((1 << b) - 1) + 0.5) * 2.0 ** -s]
    ties = [(k + 0.5) * 2.0 ** -s for k in np.linspace(3, (1 << b) - 4, 40).astype(np.int64)]
    vals = torch.tensor(special + ties, dtype=torch.float32)
    for n in range(N):
        flat_idx = torch.randperm(h * w, generator=g)[:min(len(vals), h * w)]
        rows, cols = flat_idx // w, flat_idx % w
        x[n, 0, rows, cols] = vals[:len(flat_idx)]
    return x


@pytest.mark.parametrize("b", DEPTHS)
@pytest.mark.parametrize("N,Hp,Wp,h,w", [(1, 32, 48, 18, 34), (2, 32, 48, 18, 36), (2, 3, 5, 3, 5), (1, 128, 256, 100, 132),
                                         (2, 64, 128, 50, 66), (2, 66, 130, 65, 129)])
def test_output_equals_the_restatement(cuda, N, Hp, Wp, h, w, b):
    from pMCTF.hip import lib, ops
    x = _reconstruction(N, Hp, Wp, h, w, b)
    want = hr.to_u16(x.numpy(), h, w, b)
    crop = x[:, 0, :h, :w]
    if h * w > 60:
        assert bool(torch.isnan(crop).any()) and bool(torch.isinf(crop).any()), "the special values lie inside the crop"
        scaled = crop[torch.isfinite(crop)].double() * 2.0 ** (b - 8)
        assert bool(((scaled % 1.0) == 0.5).any()) and float(scaled.min()) < 0 and float(scaled.max()) > (1 << b) - 1
    xd = x.to(cuda)
    got = ops.planes_to_u16(xd, h, w, b)
    assert got.dtype == torch.uint16 and tuple(got.shape) == (N, h, w) and got.is_cuda and got.is_contiguous()
    diff = np.argwhere(got.cpu().numpy() != want)
    assert diff.size == 0, f"{len(diff)} samples differ, first at (n, y, x) {diff[0]}"
    # the output may start on any 2-byte boundary (plane 1 of a chroma tensor, a slice of a frame buffer): guards intact
    L = lib.hip()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for off in range(4):
        buf, view = _guarded(N * h * w, torch.uint16, cuda, 0xA5A5, offset=off)
        assert view.data_ptr() % 8 == (2 * off) % 8
        assert L.pmctf_planes_to_u16(_ptr(xd), _ptr(view), N, Hp, Wp, h, w, b, stream) == 0
        assert np.array_equal(view.cpu().numpy().reshape(N, h, w), want), off
        assert _guards_untouched(buf, N * h * w, 0xA5A5, offset=off), off


@pytest.mark.parametrize("b", [10, 16])
def test_out_of_in_is_the_identity_on_every_sample_value(cuda, b):
    from pMCTF.hip import ops
    h = w = 256
    v = np.arange(65536, dtype=np.uint16)
    rng = np.random.default_rng(b)
    frame = np.concatenate((v, rng.integers(0, 1 << b, h * w // 2, dtype=np.uint16)))
    y_pad, c_pad, _, _ = ops.planes_from_u16(torch.from_numpy(frame).to(cuda), h, w, b, psize=128, originals=False)
    assert tuple(y_pad.shape) == (1, 1, h, w)
    back = ops.planes_to_u16(y_pad, h, w, b).cpu().numpy().reshape(-1)
    top = (1 << b) - 1
    assert np.array_equal(back[:top + 1], v[:top + 1]), "out(in(v)) == v for every v <= max"
    assert bool((back[top + 1:] == top).all()), "samples above max come back clamped"
    cback = ops.planes_to_u16(c_pad, h // 2, w // 2, b).cpu().numpy().reshape(-1)
    assert np.array_equal(cback, frame[h * w:])


# -------------------------------------------------------------------------------------------------------- 3. error sums
@pytest.mark.parametrize("b", DEPTHS)
@pytest.mark.parametrize("h,w,psize", SIZES[:4])
def test_error_sums_equal_the_restatement(cuda, h, w, psize, b):
    from pMCTF.hip import ops
    frame = _picture(h, w, b, seed=h + w + b)
    _, _, org_y, org_c = hr.to_planes(frame, h, w, b, psize)
    Hp, Wp = hr.pad_size(h, w, psize)
    rec_y = _reconstruction(1, Hp, Wp, h, w, b)
    rec_c = _reconstruction(2, Hp // 2, Wp // 2, h // 2, w // 2, b)
    want = hr.sse(rec_y.numpy(), rec_c.numpy(), org_y, org_c, h, w, b)
    args = (rec_y.to(cuda), rec_c.to(cuda), torch.from_numpy(org_y).to(cuda), torch.from_numpy(org_c).to(cuda), h, w, b)
    got = ops.frame_sse_hbd(*args)
    assert got["sse"] == want and all(isinstance(v, int) for v in got["sse"])
    q = hr.yuv_psnr(want, h, w, b)
    for k in ("y", "cb", "cr", "yuv"):
        assert got[k] == pytest.approx(q[k], abs=1e-9), k
    assert ops.frame_sse_hbd(*args)["sse"] == got["sse"]
    # identical pictures: zero sums, infinite PSNR
    y_pad, c_pad = hr.to_planes(frame, h, w, b, psize)[:2]
    same = ops.frame_sse_hbd(torch.from_numpy(y_pad).to(cuda), torch.from_numpy(c_pad).to(cuda), args[2], args[3], h, w, b)
    assert same["sse"] == (0, 0, 0) and same["yuv"] == float("inf")


def test_error_sums_of_black_against_white_at_16_bits(cuda):
    from pMCTF.hip import ops
    h, w, b = 18, 34, 16
    Hp, Wp = hr.pad_size(h, w, 16)
    white = float(65535 * 2.0 ** -8)
    got = ops.frame_sse_hbd(torch.zeros((1, 1, Hp, Wp), device=cuda), torch.zeros((2, 1, Hp // 2, Wp // 2), device=cuda),
                            torch.full((1, 1, h, w), white, device=cuda), torch.full((2, 1, h // 2, w // 2), white, device=cuda),
                            h, w, b)
    assert got["sse"] == (65535 ** 2 * h * w, 65535 ** 2 * h * w // 4, 65535 ** 2 * h * w // 4)
    assert got["y"] == 0.0 and got["yuv"] == 0.0


def test_error_sums_past_2_to_the_53_stay_exact(cuda):
    """1536x2048 at 16 bits, nearly every term 65535^2, a sprinkling of small errors: the luma sum is odd (an even number of
    samples, all but one of their terms odd) and above 2^53, where a double stops counting in ones.  The expectation is made
    of Python integers."""
    from pMCTF.hip import ops
    h, w, b = 1536, 2048, 16
    white = np.float32(65535 * 2.0 ** -8)
    org_y = np.full((1, 1, h, w), white, np.float32)
    org_c = np.full((2, 1, h // 2, w // 2), white, np.float32)
    rec_y = np.zeros((1, 1, h, w), np.float32)
    rec_c = np.zeros((2, 1, h // 2, w // 2), np.float32)
    rng = np.random.default_rng(53)
    small = {}
    for plane, rec, n in (("y", rec_y[0, 0], 1001), ("cb", rec_c[0, 0], 300), ("cr", rec_c[1, 0], 301)):
        at = rng.choice(rec.size, n, replace=False)
        d = 2 * rng.integers(0, 50, n) + 1                          # odd errors 1..99 ...
        d[0] += 1                                                   # ... and one even one: every other term of the plane is odd
        rec.reshape(-1)[at] = ((65535 - d) * 2.0 ** -8).astype(np.float32)
        small[plane] = (n, sum(int(v) ** 2 for v in d))
    want = tuple((size - small[p][0]) * 65535 ** 2 + small[p][1]
                 for p, size in (("y", h * w), ("cb", h * w // 4), ("cr", h * w // 4)))
    assert want[0] > 2 ** 53 and want[0] % 2 == 1 and float(want[0]) != want[0], "not representable as a double"
    assert want == hr.sse(rec_y, rec_c, org_y, org_c, h, w, b)
    args = tuple(torch.from_numpy(a).to(cuda) for a in (rec_y, rec_c, org_y, org_c)) + (h, w, b)
    got = ops.frame_sse_hbd(*args)
    assert got["sse"] == want
    assert ops.frame_sse_hbd(*args)["sse"] == want


# ------------------------------------------------------------------------------------------------------- 4. end to end
W, H, GOP, N, Q, B = 132, 100, 4, 8, 3, 10              # the existing round trip's case: padded to 256x128
FRAME_SAMPLES = W * H * 3 // 2


def _files(folder):
    out = {}
    for base, _, names in os.walk(folder):
        for n in names:
            p = os.path.join(base, n)
            out[os.path.relpath(p, folder)] = open(p, "rb").read()
    return out


@pytest.fixture(scope="module")
def coded(cuda, tmp_path_factory):
    """three folders from one model: the multiples-of-4 source at 10 bits, its 8-bit form through the existing call, and a
    10-bit source with low bits coded with picture_hash="f32"; a decoder model of its own"""
    import pmctf_gop
    tmp = tmp_path_factory.mktemp("high_bitdepth")
    out = {"tmp": tmp}
    anchor = hr.synth_hbd(W, H, N, B, seed=5, low_bits=False)
    full = hr.synth_hbd(W, H, N, B, seed=5, low_bits=True)
    assert all(not (p & 3).any() for pic in anchor for p in pic) and any((p & 3).any() for pic in full for p in pic)
    out["full_src"] = full
    paths = {k: str(tmp / f"{k}.yuv") for k in ("anchor10", "anchor8", "full")}
    pmctf_gop.write_yuv(paths["anchor10"], anchor)
    pmctf_gop.write_yuv(paths["anchor8"], [tuple((p >> 2).astype(np.uint8) for p in pic) for pic in anchor])
    pmctf_gop.write_yuv(paths["full"], full)
    out["src"] = paths
    enc_net, _ = product_model(1)
    out["enc_net"] = enc_net
    for name, kw in (("anchor10", {"bitdepth": B}), ("anchor8", {}), ("full", {"bitdepth": B, "picture_hash": "f32"})):
        bins = str(tmp / f"{name}_bins")
        os.makedirs(bins)
        out[name + "_enc"] = pmctf_gop.encode_sequence(enc_net, paths[name], W, H, N, GOP, Q, bins, "cuda", keep_gops=True, **kw)
        out[name] = bins
    out["dec_net"], _ = product_model(1)
    return out


def test_parity_anchor(coded):
    """every sample a multiple of 4: the 10-bit path writes the files of the existing 8-bit path, byte for byte"""
    import pmctf_gop
    f10, f8 = _files(coded["anchor10"]), _files(coded["anchor8"])
    assert sorted(set(f10) - set(f8)) == ["picture_format.json"] and set(f8) <= set(f10)
    streams = [p for p in f8 if p.startswith("gop_")]
    assert len(streams) == (N // GOP) * len(pmctf_gop.gop_file_names(GOP))
    for p in sorted(f8):
        assert f10[p] == f8[p], f"{p} differs between the 10-bit folder and the 8-bit one"
    assert "sequence.json" in f8
    assert pmctf_gop.read_picture_format(coded["anchor10"]) == B and pmctf_gop.read_picture_format(coded["anchor8"]) == 8
    assert coded["anchor10_enc"]["bits"] == coded["anchor8_enc"]["bits"]


def test_eight_bit_folder_is_unchanged(coded):
    assert sorted(os.listdir(coded["anchor8"])) == ["gop_00000", "gop_00001", "sequence.json"]
    assert sorted(os.listdir(coded["anchor10"])) == ["gop_00000", "gop_00001", "picture_format.json", "sequence.json"]
    assert sorted(os.listdir(coded["full"])) == ["gop_00000", "gop_00001", "picture_format.json", "picture_hashes.json",
                                                 "sequence.json"]


def _decoded(coded):
    import pmctf_gop
    if "full_yuv" not in coded:
        yuv = str(coded["tmp"] / "full_dec.yuv")
        coded["full_res"] = pmctf_gop.decode_sequence(coded["dec_net"], coded["full"], yuv, "cuda")
        coded["full_yuv"] = yuv
    return coded["full_yuv"], coded["full_res"]


def test_round_trip_in_a_second_model(coded, cuda):
    import pmctf_gop
    from pMCTF.utils.yuv_reader import YUVReader
    yuv, res = _decoded(coded)
    assert res["verified"] == N and res["bitdepth"] == B and res["hash_mismatches"] == [] and res["frames"] == [(H, W)] * N
    data = np.fromfile(yuv, dtype="<u2")
    assert os.path.getsize(yuv) == 8 * 132 * 100 * 3 and data.size == N * FRAME_SAMPLES
    assert int(data.max()) <= 1023 and bool((data & 3).any()), "10-bit samples with live low bits"
    # the encoder's own reconstruction of the same pictures
    reader = YUVReader(coded["src"]["full"], W, H, bitdepth=B)
    scratch = str(coded["tmp"] / "own_reconstruction")
    os.makedirs(scratch)
    want = []
    with torch.no_grad():
        for k in range(N // GOP):
            padded, _, (h, w) = pmctf_gop.read_gop(reader, GOP, cuda)
            enc = pmctf_gop.encode_gop(coded["enc_net"], padded, h, w, Q, scratch, skip_decoding=True)
            rec = pmctf_gop.decode_gop(coded["enc_net"], enc["frames_coded"])
            want += pmctf_gop.frames_to_u16(rec, h, w, B)
    reader.close()
    for i, planes in enumerate(want):
        assert all(p.dtype == np.uint16 for p in planes)
        assert np.array_equal(data[i * FRAME_SAMPLES:(i + 1) * FRAME_SAMPLES], hr.flat(planes)), f"frame {i}"
    recorded = pmctf_gop.read_picture_hashes(coded["full"], N)
    assert recorded["level"] == "f32" and recorded["frames"] == coded["full_enc"]["picture_hashes"]
    spec = importlib.util.spec_from_file_location("check_picture_hashes", os.path.join(ROOT, "tools", "check_picture_hashes.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.main([coded["full"], yuv]) == 0
    bad = bytearray(open(yuv, "rb").read())
    bad[5 * FRAME_SAMPLES * 2 + 2 * W * H + 9] ^= 0x02               # frame 5, a byte of the Cb plane
    flipped = str(coded["tmp"] / "flipped.yuv")
    open(flipped, "wb").write(bytes(bad))
    assert tool.main([coded["full"], flipped]) == 1
    _, mism = pmctf_gop.check_yuv_hashes(coded["full"], flipped)
    assert [(m["frame"], m["plane"]) for m in mism] == [(5, "cb"), (5, "frame")]


def test_device_ingest_writes_the_same_files(coded):
    """the GOPs are closed units: the first GOP coded with ingest="device" is the first GOP of the host-ingest folder"""
    import pmctf_gop
    bins = str(coded["tmp"] / "device_bins")
    os.makedirs(bins)
    r = pmctf_gop.encode_sequence(coded["enc_net"], coded["src"]["full"], W, H, GOP, GOP, Q, bins, "cuda", keep_gops=True,
                                  ingest="device", bitdepth=B, picture_hash="u16")
    fd, fh = _files(bins), _files(coded["full"])
    names = [os.path.join("gop_00000", n) for n in pmctf_gop.gop_file_names(GOP)]
    assert sorted(p for p in fd if p.startswith("gop_")) == sorted(names)
    for p in names + ["picture_format.json"]:
        assert fd[p] == fh[p], p
    host = coded["full_enc"]
    assert r["bits"] == host["bits"][:GOP] and r["psnr"] == host["psnr"][:GOP]
    u16 = pmctf_gop.read_picture_hashes(bins, GOP)
    assert u16["level"] == "u16"
    assert u16["frames"] == [{k: rec[k] for k in pmctf_gop.HASH_KEYS["u16"]} for rec in host["picture_hashes"][:GOP]]


def test_quality_tables_are_the_psnr_of_the_decoded_file(coded, cuda):
    import pmctf_gop
    yuv, _ = _decoded(coded)
    data = np.fromfile(yuv, dtype="<u2").astype(np.int64)
    enc = coded["full_enc"]
    ny, nc = W * H, W * H // 4
    want_sse, want = [], []
    for i, pic in enumerate(coded["full_src"]):
        d = data[i * FRAME_SAMPLES:(i + 1) * FRAME_SAMPLES] - hr.flat(pic).astype(np.int64)
        sse3 = tuple(int((p * p).sum()) for p in (d[:ny], d[ny:ny + nc], d[ny + nc:]))
        want_sse.append(sse3)
        want.append(hr.yuv_psnr(sse3, H, W, B))
    assert all(s[0] > 0 for s in want_sse), "a lossy rate point"
    assert len(enc["psnr"]) == N
    for i in range(N):
        assert enc["psnr"][i] == pytest.approx(want[i]["yuv"], abs=1e-9), i
    assert enc["psnr_rgb"] == [0.0] * N and "msssim" not in enc
    q = pmctf_gop.sequence_quality(coded["src"]["full"], yuv, W, H, N, cuda, gop=GOP, bitdepth=B)
    assert [tuple(s) for s in q["sse"]] == want_sse
    for i in range(N):
        for k, name in (("yuv", "psnr"), ("y", "psnr_y"), ("cb", "psnr_cb"), ("cr", "psnr_cr")):
            assert q[name][i] == pytest.approx(want[i][k], abs=1e-9), (i, k)
        assert q["psnr"][i] == pytest.approx(enc["psnr"][i], abs=1e-9)
    assert q["psnr_rgb"] == [0.0] * N and q["msssim"] == [0.0] * N


def test_refusals(coded):
    import pmctf_gop
    src, net = coded["src"]["full"], coded["enc_net"]
    scratch = str(coded["tmp"] / "refused")
    os.makedirs(scratch)
    for kw in ({"msssim": True}, {"decoded_frame_path": str(coded["tmp"] / "png")}, {"src_format": "png"},
               {"picture_hash": "u8", "keep_gops": True}):
        with pytest.raises(ValueError):
            pmctf_gop.encode_sequence(net, src, W, H, N, GOP, Q, scratch, "cuda", bitdepth=B, **kw)
    assert os.listdir(scratch) == []
    with pytest.raises(ValueError, match="picture_format.json"):
        pmctf_gop.decode_sequence(coded["dec_net"], coded["full"], None, "cuda", png_out=str(coded["tmp"] / "png"))
    with pytest.raises(ValueError, match="picture_format.json"):
        pmctf_gop.decode_sequence(coded["dec_net"], coded["full"], str(coded["tmp"] / "x.yuv"), "cuda",
                                  png_out=str(coded["tmp"] / "png"))
    assert not os.path.exists(str(coded["tmp"] / "png")) and not os.path.exists(str(coded["tmp"] / "x.yuv"))
