"""Sequences as lists of GOPs on the GPU: pmctf_luma_activity_f32 against tests/structure_restatement.py, and
pmctf_seq.encode_sequence_gops end to end at 132x100 (padded to 256x128): the anchor to encode_sequence, any length with a
lone picture, the scene cut, ten bits, the rate-distortion search, each decoded and verified by a second model.
Everything is exact: integers, bytes and bits."""
import os

import numpy as np
import pytest
import torch

import structure_restatement as sr
from helpers import product_model

pytestmark = pytest.mark.gpu

W, H, Q = 132, 100, 3
GUARD = 64
FILL32, FILL64 = 0x5A5A5A5A, 0x123456789ABCDEF


# ------------------------------------------------------------------------------------------------------------ 1. kernel
def _run(cur, prev, b, cuda):
    """the kernel on outputs placed between guard words -> (hist list, sad or None)"""
    from pMCTF.hip import ops
    hbuf = torch.full((2 * GUARD + 256,), FILL32, dtype=torch.int32, device=cuda)
    sbuf = torch.full((3,), FILL64, dtype=torch.int64, device=cuda)
    c = torch.from_numpy(cur).to(cuda)
    p = None if prev is None else torch.from_numpy(prev).to(cuda)
    hist, sad = ops.luma_activity(c, p, b, hist=hbuf[GUARD:GUARD + 256], sad=None if p is None else sbuf[1:2])
    assert hist.data_ptr() == hbuf.data_ptr() + 4 * GUARD and (sad is None) == (p is None)
    hh, ss = hbuf.cpu(), sbuf.cpu().tolist()
    assert bool((hh[:GUARD] == FILL32).all()) and bool((hh[GUARD + 256:] == FILL32).all()), "guards of hist256"
    assert ss[0] == FILL64 and ss[2] == FILL64, "guards of sad"
    if p is None:
        assert ss[1] == FILL64, "no previous picture: sad is not touched"
    # the wrapper's own outputs give the same values
    h2, s2 = ops.luma_activity(c, p, b)
    assert h2.dtype == torch.int32 and h2.is_cuda and tuple(h2.shape) == (256,)
    assert h2.cpu().tolist() == hh[GUARD:GUARD + 256].tolist()
    assert (s2 is None) if p is None else (s2.dtype == torch.int64 and s2.cpu().tolist() == [ss[1]])
    return hh[GUARD:GUARD + 256].tolist(), None if p is None else ss[1] & 0xffffffffffffffff


def _random(h, w, b, seed, full_range=False):
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 1 << (16 if full_range else b), (1, 1, h, w), dtype=np.uint16)
    return v.astype(np.float32) * np.float32(2.0 ** -(b - 8))


@pytest.mark.parametrize("b", [8, 10, 16])
@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (6, 10), (18, 34), (100, 132), (300, 300)])
def test_kernel_equals_the_restatement(cuda, h, w, b):
    cur, prev = _random(h, w, b, seed=h * 1000 + w + b), _random(h, w, b, seed=h * 1000 + w + b + 1)
    want_hist, want_sad = sr.activity(cur, prev, b)
    assert sum(want_hist) == h * w
    if h * w >= 100 * 132:
        assert all(want_hist), "all 256 bins occupied"
    assert _run(cur, None, b, cuda) == (want_hist, None)
    got = _run(cur, prev, b, cuda)
    assert got == (want_hist, want_sad) and isinstance(got[1], int)
    assert _run(cur, prev, b, cuda) == got, "a second run gives the same bits"


def test_kernel_on_one_value(cuda):
    """every lane on one bin: 90 000 counts there, nothing anywhere else"""
    for b, v in ((8, 37), (10, 37 * 4 + 3), (16, 37 * 256 + 255)):
        cur = np.full((1, 1, 300, 300), v * 2.0 ** -(b - 8), np.float32)
        prev = np.full((1, 1, 300, 300), (v - 5) * 2.0 ** -(b - 8), np.float32)
        hist, sad = _run(cur, prev, b, cuda)
        assert hist[37] == 90000 and sum(hist) == 90000 and sad == 5 * 90000
        assert (hist, sad) == sr.activity(cur, prev, b)


def test_kernel_sad_above_2_to_the_32(cuda):
    cur = np.full((1, 1, 300, 300), 65535 * 2.0 ** -8, np.float32)
    prev = np.zeros((1, 1, 300, 300), np.float32)
    hist, sad = _run(cur, prev, 16, cuda)
    assert sad == 65535 * 90000 and sad > 2 ** 32 and hist[255] == 90000
    assert (hist, sad) == sr.activity(cur, prev, 16)
    assert _run(prev, cur, 16, cuda)[1] == sad


def test_kernel_on_samples_above_the_depth_and_special_values(cuda):
    """10-bit planes holding 16-bit values: everything from 1024 up lands in bin 255; NaN counts as 0"""
    cur, prev = _random(100, 132, 10, seed=1, full_range=True), _random(100, 132, 10, seed=2, full_range=True)
    assert float(cur.max()) * 4 > 1023
    want = sr.activity(cur, prev, 10)
    assert want[0][255] > 100 * 132 * 0.9
    assert _run(cur, prev, 10, cuda) == want
    odd = _random(18, 34, 8, seed=3)
    odd.reshape(-1)[:6] = [np.nan, np.inf, -np.inf, -3.0, 1e9, 255.0]
    ref = _random(18, 34, 8, seed=4)
    want = sr.activity(odd, ref, 8)
    assert _run(odd, ref, 8, cuda) == want


# -------------------------------------------------------------------------------------------------------- 2. end to end
def _files(folder):
    out = {}
    for base, _, names in os.walk(folder):
        for n in names:
            p = os.path.join(base, n)
            out[os.path.relpath(p, folder)] = open(p, "rb").read()
    return out


def _frame_bits(folder, size):
    """8 x the sizes of every frame's files in one GOP folder"""
    import pmctf_gop
    sz = lambda n: os.path.getsize(os.path.join(folder, n))
    bits = [8.0 * (sz("0_main.bin") + sz("0_C_main.bin"))] + [None] * (size - 1)
    if size > 1:
        for _, _, i in pmctf_gop.gop_pairs(size):
            bits[i] = 8.0 * (sz(f"{i}.bin") + sz(f"{i}_C_main.bin") + sz(f"{i}_mv.bin"))
    return bits


def _own_reconstruction(net, src, gops, scratch, bitdepth=8):
    """the pictures the encoder reconstructs, GOP by GOP, from this module's own pieces"""
    import pmctf_gop
    from pMCTF.utils.yuv_reader import YUVReader
    os.makedirs(scratch, exist_ok=True)
    reader = YUVReader(src, W, H, bitdepth=bitdepth)
    out = []
    with torch.no_grad():
        for g in gops:
            padded, _, (h, w) = pmctf_gop.read_gop(reader, g["size"], "cuda", g["psize"])
            if g["size"] == 1:
                r = net.encode_lone_picture(padded[0], scratch, w, h, psize=g["psize"], skip_decoding=True, q_index=Q)
                rec = [[r["L_t"], r["L_tc"], None]]
            else:
                enc = pmctf_gop.encode_gop(net, padded, h, w, Q, scratch, skip_decoding=True, psize=g["psize"],
                                           me_downsample=g["me_downsample"])
                rec = pmctf_gop.decode_gop(net, enc["frames_coded"])
            out += pmctf_gop.frames_to_samples(rec, h, w, bitdepth)
    reader.close()
    return out


@pytest.fixture(scope="module")
def seq(cuda, tmp_path_factory):
    """one encoder model, one decoder model (same weights), the sources"""
    import pmctf_gop
    import pmctf_synth
    tmp = tmp_path_factory.mktemp("sequence_structure")
    out = {"tmp": tmp, "enc_net": product_model(1)[0], "dec_net": product_model(1)[0]}
    out["src8"] = str(tmp / "src8.yuv")
    pmctf_gop.write_yuv(out["src8"], pmctf_synth.synth_yuv420(W, H, 8, seed=1234))
    out["cut"] = str(tmp / "cut.yuv")
    pmctf_gop.write_yuv(out["cut"], sr.cut_sequence())
    return out


def _bins(seq, name):
    p = str(seq["tmp"] / name)
    os.makedirs(p)
    return p


def test_anchor_whole_gops_are_the_files_of_encode_sequence(seq):
    import pmctf_gop
    import pmctf_seq
    old, new = _bins(seq, "anchor_old"), _bins(seq, "anchor_new")
    a = pmctf_gop.encode_sequence(seq["enc_net"], seq["src8"], W, H, 8, 4, Q, old, "cuda", keep_gops=True)
    b = pmctf_seq.encode_sequence_gops(seq["enc_net"], seq["src8"], W, H, 8, 4, Q, new, "cuda", structure="fill")
    fa, fb = _files(old), _files(new)
    names = [os.path.join(g, n) for g in ("gop_00000", "gop_00001") for n in pmctf_gop.gop_file_names(4)]
    assert sorted(p for p in fb if os.sep in p) == sorted(names) == sorted(p for p in fa if os.sep in p)
    for p in names:
        assert fa[p] == fb[p], f"{p} differs"
    assert sorted(set(fb) - set(names)) == ["gop_structure.json"] and sorted(set(fa) - set(names)) == ["sequence.json"]
    assert b["bits"] == a["bits"] and b["psnr"] == a["psnr"] and b["frame_types"] == a["frame_types"] == [0, 1, 1, 1] * 2
    assert b["bpp_mv"] == a["bpp_mv"] and b["psnr_rgb"] == a["psnr_rgb"]
    assert b["gops"] == [{"first": 0, "size": 4, "me_downsample": 1, "psize": 128},
                         {"first": 4, "size": 4, "me_downsample": 1, "psize": 128}]
    assert [ln.split(",")[0] for ln in b["lines"][-2:]] == [ln.split(",")[0] for ln in a["lines"][-2:]]
    assert "cuts" not in b and "activity" not in b


def test_any_length_with_a_lone_picture(seq, cuda):
    import pmctf_gop
    import pmctf_seq
    bins = _bins(seq, "seven")
    r = pmctf_seq.encode_sequence_gops(seq["enc_net"], seq["src8"], W, H, 7, 4, Q, bins, "cuda", picture_hash="f32")
    assert [g["size"] for g in r["gops"]] == [4, 2, 1] and [g["first"] for g in r["gops"]] == [0, 4, 6]
    assert r["frame_types"] == [0, 1, 1, 1, 0, 1, 0] and r["bpp_mv"][6] == 0.0 and len(r["psnr"]) == 7
    assert sorted(os.listdir(bins)) == ["gop_00000", "gop_00001", "gop_00002", "gop_structure.json", "picture_hashes.json"]
    for k, names in enumerate((pmctf_gop.gop_file_names(4), pmctf_gop.gop_file_names(2), ["0_main.bin", "0_C_main.bin"])):
        assert sorted(os.listdir(os.path.join(bins, pmctf_gop.gop_folder(k)))) == sorted(names), k
    want_bits = []
    for k, g in enumerate(r["gops"]):
        want_bits += _frame_bits(os.path.join(bins, pmctf_gop.gop_folder(k)), g["size"])
    assert r["bits"] == want_bits
    assert sum("P frames, average" in ln for ln in r["lines"]) == 2
    # a second model decodes and verifies
    yuv = str(seq["tmp"] / "seven.yuv")
    d = pmctf_gop.decode_sequence(seq["dec_net"], bins, yuv, "cuda")
    assert d["verified"] == 7 and d["hash_mismatches"] == [] and d["frames"] == [(H, W)] * 7 and d["bitdepth"] == 8
    assert d["header"] == pmctf_seq.read_gop_structure(bins) and d["header"]["gops"] == r["gops"]
    data = np.fromfile(yuv, dtype=np.uint8)
    n = W * H * 3 // 2
    assert data.size == 7 * n
    want = _own_reconstruction(seq["enc_net"], seq["src8"], r["gops"], str(seq["tmp"] / "seven_scratch"))
    for i, planes in enumerate(want):
        assert np.array_equal(data[i * n:(i + 1) * n], np.concatenate([p.reshape(-1) for p in planes])), f"frame {i}"
    assert pmctf_gop.check_yuv_hashes(bins, yuv) == (7, [])
    # the lone picture's luma through the L coder's own decompress, bit for bit
    lone = os.path.join(bins, "gop_00002")
    dec = pmctf_gop.decode_gop_files(seq["dec_net"], lone, 1, H, W, Q)
    assert len(dec["frames"]) == 1 and dec["stages"] == 0
    alone = seq["dec_net"].lp_coder.decompress(os.path.join(lone, "0_main.bin"), padding=128, q_index=Q)["x_hat"]
    assert alone.shape == dec["frames"][0][0].shape and torch.equal(alone, dec["frames"][0][0])
    # and its two files are the oracle's L coder on the same picture, byte for byte
    from helpers import synth_sd_cpu
    from pmctf_oracle.model import Oracle
    from pMCTF.utils.yuv_reader import YUVReader
    reader = YUVReader(seq["src8"], W, H, start_index=6)
    padded, _, _ = pmctf_gop.read_gop(reader, 1, "cpu", 128)
    reader.close()
    orc = Oracle(synth_sd_cpu(1), 1, "cdef")
    with torch.no_grad():
        y_hat, y_bytes, _ = orc.pwave_compress("lp_coder", padded[0][0], [1, 1, H, W], Q, None, True)
        c_hat, c_bytes, _ = orc.pwave_compress("lp_coder", padded[0][1], [1, 2, H // 2, W // 2], Q, None, True)
    assert open(os.path.join(lone, "0_main.bin"), "rb").read() == y_bytes
    assert open(os.path.join(lone, "0_C_main.bin"), "rb").read() == c_bytes
    assert torch.equal(dec["frames"][0][0].cpu(), y_hat) and torch.equal(dec["frames"][0][1].cpu(), c_hat)
    # a flipped recorded hash is found, in the lone picture's GOP
    import json
    path = os.path.join(bins, "picture_hashes.json")
    rec = json.load(open(path))
    rec["frames"][6]["y_f32"] ^= 1
    json.dump(rec, open(path, "w"))
    with pytest.raises(pmctf_gop.PictureHashMismatch) as e:
        pmctf_gop.decode_sequence(seq["dec_net"], bins, str(seq["tmp"] / "never.yuv"), "cuda")
    assert e.value.mismatch["frame"] == 6 and e.value.mismatch["gop"] == 2 and e.value.mismatch["plane"] == "y_f32"


def test_one_picture_and_decoder_order_files(seq, cuda):
    """frame_num 1 (no pair at all: no "average ms" lines), written in the sequential decoder's order"""
    import pmctf_gop
    import pmctf_seq
    bins = _bins(seq, "one")
    r = pmctf_seq.encode_sequence_gops(seq["enc_net"], seq["src8"], W, H, 1, 8, Q, bins, "cuda", skip_decoding=False,
                                       picture_hash="u8", ingest="device")
    assert r["gops"] == [{"first": 0, "size": 1, "me_downsample": 1, "psize": 128}] and r["frame_types"] == [0]
    assert not any("average" in ln for ln in r["lines"])
    assert pmctf_seq.read_gop_structure(bins)["ll_order"] == "position"
    d = pmctf_gop.decode_sequence(seq["dec_net"], bins, str(seq["tmp"] / "one.yuv"), "cuda")
    assert d["verified"] == 1 and d["hash_mismatches"] == []


def test_scene_cut_end_to_end(seq, cuda):
    import pmctf_gop
    import pmctf_seq
    bins = _bins(seq, "cut")
    r = pmctf_seq.encode_sequence_gops(seq["enc_net"], seq["cut"], W, H, 12, 8, Q, bins, "cuda", structure="scenecut",
                                       hd_min=0.3, mad_min=5, picture_hash="u8")
    want = sr.cut_figures()
    assert r["activity"]["sad"] == want["sad"] and r["activity"]["hist_l1"] == want["hist_l1"]
    assert r["activity"]["mad"] == want["mad"] and r["activity"]["hd"] == want["hd"]
    assert all(isinstance(v, int) for v in r["activity"]["sad"][1:] + r["activity"]["hist_l1"][1:])
    assert r["cuts"] == [6]
    assert [g["size"] for g in r["gops"]] == [4, 2, 4, 2] and r["frame_types"] == [0, 1, 1, 1, 0, 1] * 2
    d = pmctf_gop.decode_sequence(seq["dec_net"], bins, str(seq["tmp"] / "cut_dec.yuv"), "cuda")
    assert d["verified"] == 12 and d["hash_mismatches"] == []
    assert pmctf_gop.check_yuv_hashes(bins, str(seq["tmp"] / "cut_dec.yuv")) == (12, [])
    # the analysis alone, through the device ingest of a 10-bit reader: the same integers at the other depth
    from pMCTF.utils.yuv_reader import YUVReader
    hbd = str(seq["tmp"] / "cut10.yuv")
    pmctf_gop.write_yuv(hbd, [tuple((p.astype(np.uint16) << 2) + 1 for p in pic) for pic in sr.cut_sequence()])
    got = pmctf_seq.sequence_activity(lambda: YUVReader(hbd, W, H, bitdepth=10), 12, cuda, bitdepth=10)
    lumas = [((pic[0].astype(np.uint16) << 2) + 1).astype(np.float32) * np.float32(0.25) for pic in sr.cut_sequence()]
    assert got == sr.figures(lumas, 10)
    assert got["sad"][1:] == [4 * s for s in want["sad"][1:]] and got["hist_l1"] == want["hist_l1"]


def test_high_bit_depth(seq, cuda):
    import hbd_restatement as hr
    import pmctf_gop
    import pmctf_seq
    src = str(seq["tmp"] / "src10.yuv")
    pmctf_gop.write_yuv(src, hr.synth_hbd(W, H, 5, 10, seed=5))
    bins = _bins(seq, "ten_bits")
    r = pmctf_seq.encode_sequence_gops(seq["enc_net"], src, W, H, 5, 4, Q, bins, "cuda", bitdepth=10, picture_hash="u16")
    assert [g["size"] for g in r["gops"]] == [4, 1] and r["psnr_rgb"] == [0.0] * 5
    assert sorted(os.listdir(bins)) == ["gop_00000", "gop_00001", "gop_structure.json", "picture_format.json",
                                        "picture_hashes.json"]
    yuv = str(seq["tmp"] / "ten_bits.yuv")
    d = pmctf_gop.decode_sequence(seq["dec_net"], bins, yuv, "cuda")
    assert d["verified"] == 5 and d["bitdepth"] == 10 and d["hash_mismatches"] == []
    data = np.fromfile(yuv, dtype="<u2")
    n = W * H * 3 // 2
    assert data.size == 5 * n and int(data.max()) <= 1023
    want = _own_reconstruction(seq["enc_net"], src, r["gops"], str(seq["tmp"] / "ten_scratch"), bitdepth=10)
    for i, planes in enumerate(want):
        assert all(p.dtype == np.uint16 for p in planes)
        assert np.array_equal(data[i * n:(i + 1) * n], hr.flat(planes)), f"frame {i}"
    assert pmctf_gop.check_yuv_hashes(bins, yuv) == (5, [])


def test_search_structure(seq, cuda):
    import pmctf_ca
    import pmctf_gop
    import pmctf_seq
    import pmctf_synth
    from pMCTF.utils.yuv_reader import YUVReader
    w = h = 128
    src = str(seq["tmp"] / "src128.yuv")
    pmctf_gop.write_yuv(src, pmctf_synth.synth_yuv420(w, h, 9, seed=1234))
    bins = _bins(seq, "search")
    r = pmctf_seq.encode_sequence_gops(seq["enc_net"], src, w, h, 9, 8, Q, bins, "cuda", structure="search",
                                       picture_hash="f32")
    reader = YUVReader(src, w, h)
    _, orig, _ = pmctf_gop.read_gop(reader, 8, cuda, 128)
    reader.close()
    with torch.no_grad():
        s = pmctf_ca.search_gop(seq["enc_net"], orig, h, w, Q, None, write_stream=False)
    assert len(r["searches"]) == 1 and r["searches"][0]["first"] == 0
    assert (r["searches"][0]["gop_choice"], r["searches"][0]["ds_choice"]) == (s["gop_choice"], s["ds_choice"])
    assert [t[:2] for t in r["searches"][0]["trials"]] == [t[:2] for t in s["trials"]], "the same options were tried"
    size, ds = s["gop_choice"], s["ds_choice"]
    want = [{"first": f, "size": size, "me_downsample": ds, "psize": pmctf_gop.ca_psize(ds)} for f in range(0, 8, size)]
    want.append({"first": 8, "size": 1, "me_downsample": 1, "psize": 128})
    assert r["gops"] == want and pmctf_seq.read_gop_structure(bins)["gops"] == want
    assert sorted(os.listdir(os.path.join(bins, pmctf_gop.gop_folder(len(want) - 1)))) == ["0_C_main.bin", "0_main.bin"]
    d = pmctf_gop.decode_sequence(seq["dec_net"], bins, str(seq["tmp"] / "search.yuv"), "cuda")
    assert d["verified"] == 9 and d["hash_mismatches"] == [] and len(d["frames"]) == 9


def test_explicit_structure_and_refusals(seq, cuda):
    import pmctf_gop
    import pmctf_seq
    bins = _bins(seq, "explicit")
    r = pmctf_seq.encode_sequence_gops(seq["enc_net"], seq["src8"], W, H, 5, 4, Q, bins, "cuda",
                                       structure=[(1, 1), (2, 2), (2, 1)], picture_hash="f32")
    assert r["gops"] == [{"first": 0, "size": 1, "me_downsample": 1, "psize": 128},
                         {"first": 1, "size": 2, "me_downsample": 2, "psize": 128},
                         {"first": 3, "size": 2, "me_downsample": 1, "psize": 128}]
    assert r["frame_types"] == [0, 0, 1, 0, 1]
    d = pmctf_gop.decode_sequence(seq["dec_net"], bins, str(seq["tmp"] / "explicit.yuv"), "cuda")
    assert d["verified"] == 5 and d["hash_mismatches"] == []
    scratch = _bins(seq, "refused")
    call = lambda n, g, **kw: pmctf_seq.encode_sequence_gops(seq["enc_net"], seq["src8"], W, H, n, g, Q, scratch, "cuda", **kw)
    for n, g, kw in ((0, 4, {}), (-1, 4, {}), (7, 3, {}), (7, 1, {}), (7, 6, {}), (7, 2, {"structure": "search"}),
                     (7, 4, {"structure": [(4, 1), (2, 1)]}), (7, 4, {"structure": [(4, 1), (4, 1)]}),
                     (7, 4, {"structure": "adaptive"})):
        with pytest.raises(ValueError):
            call(n, g, **kw)
    assert os.listdir(scratch) == []
