"""Spatial layers on the GPU (pmctf_spatial) at 136x104, padded to 256x128, q 3, synthetic weights: the size
offers the levels 1 and 2 and refuses 3.  Seven pictures as GOPs of 4, 2, 1.  The yardstick is tests/spatial_restatement.py:
every file walked IN FULL with a HostDecoder, its level-k plane built from the engine's primitives, and decode_gop's loop on
those planes with the test's own nested reduction of the motion.  Everything is exact: torch.equal, bytes and integers.  No
bitstream file that is decoded is ever altered: the tampering is done on JSON records."""
import json
import os
import shutil
import struct
import zlib

import numpy as np
import pytest
import torch

import layers_restatement as lr
import spatial_restatement as sr
from helpers import frames, product_model

pytestmark = pytest.mark.gpu

W, H, Q, PSIZE = 136, 104, 3, 128
PW, PH = 256, 128


def _n(level, w=W, h=H):
    """samples of one 4:2:0 picture of the level"""
    return (w >> level) * (h >> level) * 3 // 2


@pytest.fixture(scope="module")
def seq(cuda, tmp_path_factory):
    """one encoder model, one decoder model (same weights), the folders coded once, and the caches of the restatement: a full
    walk per file, the full-size motion per GOP.  Tests copy a folder before they change anything in it."""
    import pmctf_gop
    import pmctf_seq
    import pmctf_synth
    tmp = tmp_path_factory.mktemp("spatial_layers")
    out = {"tmp": tmp, "enc_net": product_model(1)[0], "dec_net": product_model(1)[0], "walk": {}, "coded": {}}
    out["src"] = str(tmp / "src.yuv")
    pmctf_gop.write_yuv(out["src"], pmctf_synth.synth_yuv420(W, H, 7, seed=4321))
    out["seven"], out["pos"] = str(tmp / "seven"), str(tmp / "pos")
    os.makedirs(out["seven"])
    os.makedirs(out["pos"])
    r = pmctf_seq.encode_sequence_gops(out["enc_net"], out["src"], W, H, 7, 4, Q, out["seven"], "cuda", picture_hash="u8")
    assert [g["size"] for g in r["gops"]] == [4, 2, 1]
    r = pmctf_seq.encode_sequence_gops(out["enc_net"], out["src"], W, H, 2, 2, Q, out["pos"], "cuda", skip_decoding=False)
    assert pmctf_gop.sequence_layout(out["pos"])[0]["ll_order"] == "position"
    return out


# ------------------------------------------------------------------------------------------------ the restatement, cached
def _stage(i):
    return (i & -i).bit_length() - 1


def _job(net, path):
    """(coder, data, padding, q_index, qp_scale) of one picture file, as the decoder's jobs are, from the file's name"""
    from pMCTF.hip.engine import get_curr_q
    name = os.path.basename(path)
    chroma, low = name.endswith("_C_main.bin"), name.startswith("0_")
    qp = None
    if not low and net.quant_stage:
        me = min(net.num_me_stages - 1, _stage(int(name.split(".")[0].split("_")[0])))
        qp = get_curr_q(net.engine().sd[f"hp_q_scale.{me}"], Q)
    return ("lp_coder" if low else "hp_coder", open(path, "rb").read(), PSIZE // 2 if chroma else PSIZE, Q, qp)


def _walk(seq, path, ll_order="plane"):
    if path not in seq["walk"]:
        coder, data, pad, q, qp = _job(seq["dec_net"], path)
        with torch.no_grad():
            seq["walk"][path] = (coder,) + sr.full_walk(seq["dec_net"].engine(), coder, data, pad, q, qp, ll_order)
    return seq["walk"][path]


def _plane(seq, path, level, ll_order="plane"):
    coder, hat, q, _ = _walk(seq, path, ll_order)
    with torch.no_grad():
        return sr.plane_of_level(seq["dec_net"].engine(), coder, hat, q, level)


def _entries(seq, folder, g, size, level, ll_order="plane", me_downsample=1):
    """[[Y_k, UV_k, full-size mv_hat or None]] of one GOP: the restated planes, the motion of a full decode"""
    import pmctf_gop
    sub = os.path.join(folder, pmctf_gop.gop_folder(g))
    if sub not in seq["coded"]:
        seq["coded"][sub] = pmctf_gop.decode_gop_files(seq["dec_net"], sub, size, H, W, Q, me_downsample=me_downsample,
                                                       ll_order=ll_order)["frames_coded"]
    out = []
    for i, e in enumerate(seq["coded"][sub]):
        y, c = (f"{i}.bin", f"{i}_C_main.bin") if i else ("0_main.bin", "0_C_main.bin")
        out.append([_plane(seq, os.path.join(sub, y), level, ll_order), _plane(seq, os.path.join(sub, c), level, ll_order), e[2]])
    return out


def _expected(seq, folder, level, t=0, bitdepth=8):
    """the pictures of (spatial level, temporal level) of a whole folder as the decoder writes them"""
    import pmctf_gop
    header, gops = pmctf_gop.sequence_layout(folder)
    out = []
    for g, (first, size, psize, ds) in enumerate(gops):
        with torch.no_grad():
            rec = sr.synthesis(seq["dec_net"], _entries(seq, folder, g, size, level, header["ll_order"], ds), level, t)
        out += pmctf_gop.frames_to_samples([p + [None] for p in rec], H >> level, W >> level, bitdepth)
    return out


def _flat(planes):
    return np.concatenate([p.reshape(-1) for p in planes])


def _same_file(path, want, level, dtype=np.uint8):
    data = np.fromfile(path, dtype=dtype)
    assert data.size == len(want) * _n(level)
    for i, planes in enumerate(want):
        assert planes[0].shape == (H >> level, W >> level) and planes[1].shape == (H >> level + 1, W >> level + 1)
        assert np.array_equal(data[i * _n(level):(i + 1) * _n(level)], _flat(planes)), f"picture {i}"


def _same_pictures(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a[0].shape == b[0].shape and a[1].shape == b[1].shape, i
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), f"picture {i}"


def _copy(seq, name, to):
    dst = str(seq["tmp"] / to)
    shutil.copytree(seq[name], dst)
    return dst


# ------------------------------------------------------------------------------------------------------------ 1. per file
@pytest.mark.parametrize("name", ["0_main.bin", "0_C_main.bin", "2.bin", "1_C_main.bin"])
def test_one_file_at_every_level(seq, name):
    import pmctf_spatial
    net = seq["dec_net"]
    eng = net.engine()
    path = os.path.join(seq["seven"], "gop_00000", name)
    job = _job(net, path)
    N = 2 if name.endswith("_C_main.bin") else 1
    hp, wp = (PH // 2, PW // 2) if N == 2 else (PH, PW)
    assert struct.unpack(">III", job[1][:12]) == ((H // 2, W // 2, 2) if N == 2 else (H, W, 1))
    payload = _walk(seq, path)[3]
    used = []
    with torch.no_grad():
        today = eng.pwave_decompress_batch_end(eng.pwave_decompress_batch_begin([job], "plane"))[0]
        for k in range(5):
            begun = eng.pwave_decompress_batch_begin([job], "plane", k)
            assert begun[0]["level"] == k
            got = eng.pwave_decompress_batch_end(begun)[0]
            assert got.shape == (N, 1, hp >> k, wp >> k)
            if k:
                assert torch.equal(got, _plane(seq, path, k)), f"level {k}"
            else:
                assert torch.equal(got, today), "level 0 is the call without the keyword"
                hat, q = _walk(seq, path)[1:3]
                assert torch.equal(got, eng.pwave_synthesis(job[0], hat, *q)), "and the full walk's synthesis"
                if N == 1:
                    assert torch.equal(got, eng.pwave_decompress(*job))
            assert begun[0]["symbols_decoded"] == pmctf_spatial.level_symbol_count(N, hp, wp, k) == sr.symbols(N, hp, wp, k)
            used.append(begun[0]["payload_bytes_used"])
            # the same plane through the model's keyword, one file in a batch of its own
            files = [(job[1], N == 2, name.startswith("0_"), 0)]
            assert torch.equal(net.decompress_gop_files(files, PSIZE, Q, "plane", spatial_level=k)[0], got)
    assert used == sorted(used, reverse=True) and used[0] <= payload and used[4] >= 9, used
    assert used[1] < used[0], "the finest level holds bytes of its own"
    assert len(job[1]) == 16 + payload
    for level in (-1, 5, 1.0, None, True):
        with pytest.raises(ValueError, match="spatial level"):
            eng.pwave_decompress_batch_begin([job], "plane", level)


# ---------------------------------------------------------------------------------------------------- 2. the still coder
def test_still_image_coder(seq, tmp_path):
    coder = seq["dec_net"].lp_coder
    eng = coder.engine()
    fn = str(tmp_path / "img.bin")
    img = frames(256, 128, 1)[0][0].cuda()
    coder.compress(img, [1, 1, 128, 256], fn, q_index=Q, skip_decoding=False)
    data = open(fn, "rb").read()
    with torch.no_grad():
        hat, q, _ = sr.full_walk(eng, "coder", data, 64, Q)
        full = coder.decompress(fn, padding=64, q_index=Q)["x_hat"]
        for k in range(5):
            got = coder.decompress(fn, padding=64, q_index=Q, spatial_level=k)["x_hat"]
            assert got.shape == (1, 1, 128 >> k, 256 >> k)
            assert torch.equal(got, sr.plane_of_level(eng, "coder", hat, q, k) if k else full), f"level {k}"
    with pytest.raises(ValueError, match="spatial level"):
        coder.decompress(fn, padding=64, q_index=Q, spatial_level=5)


# --------------------------------------------------------------------------------------------------------- 3. per GOP
@pytest.mark.parametrize("level", [1, 2])
def test_gops_against_the_restated_loop(seq, level):
    import pmctf_spatial
    for folder, order, sizes in ((seq["seven"], "plane", [4, 2, 1]), (seq["pos"], "position", [2])):
        for g, size in enumerate(sizes):
            sub = os.path.join(folder, f"gop_{g:05d}")
            with torch.no_grad():
                want = sr.synthesis(seq["dec_net"], _entries(seq, folder, g, size, level, order), level)
            got = pmctf_spatial.decode_gop_files_layer(seq["dec_net"], sub, size, H, W, Q, 0, ll_order=order, spatial_level=level)
            assert got["times"] == list(range(size)) and got["spatial_level"] == level
            assert got["size"] == (H >> level, W >> level) and got["files"] == lr.file_names(size, 0)
            _same_pictures(got["frames"], want)
            assert got["frames"][0][0].shape == (1, 1, PH >> level, PW >> level)
            assert got["frames"][0][1].shape == (2, 1, PH >> level + 1, PW >> level + 1)
            pictures = [n for n in got["files"] if not n.endswith("_mv.bin")]
            assert sorted(got["symbols_decoded"]) == sorted(got["payload_bytes_used"]) == sorted(pictures)
            for n in pictures:
                N, hp, wp = (2, PH // 2, PW // 2) if n.endswith("_C_main.bin") else (1, PH, PW)
                assert got["symbols_decoded"][n] == sr.symbols(N, hp, wp, level)
                assert 9 <= got["payload_bytes_used"][n] <= os.path.getsize(os.path.join(sub, n)) - 16
            for i, e in enumerate(got["frames_coded"]):                          # the motion as the synthesis took it
                if e[2] is not None:
                    assert torch.equal(e[2], sr.reduced_motion(seq["coded"][sub][i][2], level))
                    assert e[2].shape == (1, 2, PH >> level, PW >> level)


# ----------------------------------------------------------------------------------------------------------- 4. level 0
def test_level_0_is_todays_decode(seq):
    import pmctf_gop
    import pmctf_layers
    import pmctf_spatial
    net, bins = seq["dec_net"], seq["seven"]
    old, new = str(seq["tmp"] / "old.yuv"), str(seq["tmp"] / "new.yuv")
    a = pmctf_gop.decode_sequence(net, bins, old, "cuda")
    b = pmctf_spatial.decode_sequence_layer(net, bins, new, 0, "cuda", spatial_level=0)
    assert open(old, "rb").read() == open(new, "rb").read() and os.path.getsize(new) == 7 * _n(0)
    assert a["verified"] == b["verified"] == 7 and b["spatial_level"] == 0 and b["size"] == (H, W) and b["frames"] == [(H, W)] * 7
    assert b["bytes_read"] == pmctf_layers.layer_bytes(bins, 0)
    for g, size in enumerate((4, 2, 1)):
        pictures = sorted(n for n in lr.file_names(size, 0) if not n.endswith("_mv.bin"))
        assert sorted(b["payload_bytes_used"][g]) == sorted(b["symbols_decoded"][g]) == pictures
        for n in pictures:
            N, hp, wp = (2, PH // 2, PW // 2) if n.endswith("_C_main.bin") else (1, PH, PW)
            assert b["symbols_decoded"][g][n] == sr.symbols(N, hp, wp, 0)
    sub = os.path.join(bins, "gop_00000")
    full = pmctf_gop.decode_gop_files(net, sub, 4, H, W, Q)
    for fn in (pmctf_spatial.decode_gop_files_layer, pmctf_layers.decode_gop_files_layer):
        _same_pictures(fn(net, sub, 4, H, W, Q, 0)["frames"], full["frames"])
    _same_pictures(pmctf_spatial.decode_gop_files_layer(net, sub, 4, H, W, Q, 0, spatial_level=0)["frames"], full["frames"])
    files = [(_job(net, os.path.join(sub, n))[1], c, n.startswith("0_"), 0) for n, c in (("0_main.bin", False), ("3_C_main.bin", True))]
    for x, y in zip(net.decompress_gop_files(files, PSIZE, Q, "plane"), net.decompress_gop_files(files, PSIZE, Q, "plane", spatial_level=0)):
        assert torch.equal(x, y)
    assert torch.equal(net.decompress_gop_files(files, PSIZE, Q, "plane")[0], full["frames_coded"][0][0])


# ------------------------------------------------------------------------------------------------ 5. temporal x spatial
def test_temporal_level_and_motion_fill_compose(seq):
    import pmctf_gop
    import pmctf_layers
    import pmctf_spatial
    net, bins = seq["dec_net"], seq["seven"]
    yuv = str(seq["tmp"] / "t1s1.yuv")
    d = pmctf_spatial.decode_sequence_layer(net, bins, yuv, 1, "cuda", spatial_level=1)
    assert d["times"] == [0, 2, 4, 6] and d["level"] == 1 and d["spatial_level"] == 1 and d["size"] == (H // 2, W // 2)
    assert d["frames"] == [(H // 2, W // 2)] * 4 and d["verified"] == 0 and d["bytes_read"] == pmctf_layers.layer_bytes(bins, 1)
    assert [sorted(g) for g in d["symbols_decoded"]] == [sorted(n for n in lr.file_names(s, 1) if not n.endswith("_mv.bin"))
                                                         for s in (4, 2, 1)]
    _same_file(yuv, _expected(seq, bins, 1, t=1), 1)
    # motion_fill at spatial level 1: decode_gop on the reduced planes with zeroed reduced high bands of stage 0
    sub = os.path.join(bins, "gop_00000")
    entries = _entries(seq, bins, 0, 4, 1)
    coded = [[e[0], e[1], None if e[2] is None else sr.reduced_motion(e[2], 1)] for e in entries]
    for i in (1, 3):
        coded[i][0], coded[i][1] = torch.zeros_like(coded[0][0]), torch.zeros_like(coded[0][1])
    with torch.no_grad():
        want = pmctf_gop.decode_gop(net, coded)
    got = pmctf_spatial.decode_gop_files_layer(net, sub, 4, H, W, Q, 1, motion_fill=True, spatial_level=1)
    assert got["times"] == [0, 1, 2, 3] and got["files"] == lr.file_names(4, 1, True)
    _same_pictures(got["frames"], want)
    assert got["frames_coded"][1][0].shape == (1, 1, PH // 2, PW // 2) and not bool(got["frames_coded"][1][0].any())
    assert bool(entries[1][0].any()), "the high band left out is not zero anyway"
    fill = str(seq["tmp"] / "fill_s1.yuv")
    d = pmctf_spatial.decode_sequence_layer(net, bins, fill, 1, motion_fill=True, spatial_level=1)
    assert d["times"] == list(range(7)) and d["verified"] == 0 and os.path.getsize(fill) == 7 * _n(1)
    data = np.fromfile(fill, dtype=np.uint8)
    for i, planes in enumerate(pmctf_gop.frames_to_u8(want, H // 2, W // 2)):
        assert np.array_equal(data[i * _n(1):(i + 1) * _n(1)], _flat(planes)), f"picture {i}"


# ------------------------------------------------------------------------------------------------- 6. hashes end to end
def test_spatial_hashes_end_to_end(seq):
    import pmctf_gop
    import pmctf_layers
    import pmctf_spatial
    bins = _copy(seq, "seven", "seven_hashed")
    yuv = str(seq["tmp"] / "hashed.yuv")
    with pytest.raises(ValueError, match=r"spatial_hashes\.json: missing"):
        pmctf_spatial.decode_sequence_layer(seq["dec_net"], bins, yuv, 0, "cuda", verify=True, spatial_level=1)
    assert not os.path.exists(yuv)
    path = pmctf_spatial.write_spatial_hashes(seq["enc_net"], bins)
    assert path == os.path.join(bins, "spatial_hashes.json")
    record = pmctf_spatial.read_spatial_hashes(bins)
    assert record["level"] == "u8" and record["size"] == [W, H] and sorted(record["layers"]) == ["1", "2"]
    assert all(sorted(record["layers"][k]) == ["0", "1", "2"] for k in ("1", "2"))
    assert [r["index"] for r in record["layers"]["1"]["1"]] == [0, 2, 4, 6]
    assert [r["index"] for r in record["layers"]["2"]["2"]] == [0, 4, 6]
    by = lambda k, t: {r["index"]: r for r in record["layers"][k][t]}
    assert by("1", "1")[6] == by("1", "0")[6] and by("1", "1")[4] == by("1", "2")[4] and by("1", "0")[0] != by("1", "1")[0]
    assert by("1", "0")[0] != by("2", "0")[0]
    for t, k, count in ((0, 1, 7), (1, 1, 4), (0, 2, 7)):
        d = pmctf_spatial.decode_sequence_layer(seq["dec_net"], bins, yuv, t, "cuda", verify=True, spatial_level=k)
        assert d["verified"] == count == len(d["frames"]) and d["hash_mismatches"] == [] and d["size"] == (H >> k, W >> k)
        _same_file(yuv, _expected(seq, seq["seven"], k, t=t), k)             # the same bitstream files
        data = open(yuv, "rb").read()
        assert [zlib.crc32(data[i * _n(k):(i + 1) * _n(k)]) for i in range(count)] == \
            [r["frame"] for r in record["layers"][str(k)][str(t)]], "a record's frame value is the CRC-32 of the picture's bytes"
    # through an extracted temporal folder: the record travels with it
    small = str(seq["tmp"] / "hashed_level1")
    pmctf_layers.extract_layer(bins, small, 1)
    d = pmctf_spatial.decode_sequence_layer(seq["dec_net"], small, yuv, 1, "cuda", verify=True, spatial_level=1)
    assert d["verified"] == 4 and d["hash_mismatches"] == []
    _same_file(yuv, _expected(seq, seq["seven"], 1, t=1), 1)
    with pytest.raises(ValueError, match="layer_extract.json"):
        pmctf_spatial.decode_sequence_layer(seq["dec_net"], small, yuv, 0, "cuda", spatial_level=1)
    # one recorded value changed, no bitstream touched: picture 4 (GOP 1) of (spatial 1, temporal 1)
    rec = json.load(open(path))
    assert rec["layers"]["1"]["1"][2]["index"] == 4
    rec["layers"]["1"]["1"][2]["cr"] ^= 1
    json.dump(rec, open(path, "w"))
    bad = str(seq["tmp"] / "tampered.yuv")
    with pytest.raises(pmctf_gop.PictureHashMismatch) as e:
        pmctf_spatial.decode_sequence_layer(seq["dec_net"], bins, bad, 1, "cuda", spatial_level=1)
    m = e.value.mismatch
    assert (m["frame"], m["plane"], m["gop"]) == (4, "cr", 1) and m["recorded"] == m["decoded"] ^ 1
    assert os.path.getsize(bad) == 2 * _n(1), "GOP 0 was written, nothing of GOP 1"
    d = pmctf_spatial.decode_sequence_layer(seq["dec_net"], bins, bad, 1, "cuda", verify="report", spatial_level=1)
    assert os.path.getsize(bad) == 4 * _n(1) and [(x["frame"], x["plane"]) for x in d["hash_mismatches"]] == [(4, "cr")]
    d = pmctf_spatial.decode_sequence_layer(seq["dec_net"], bins, bad, 0, "cuda", verify=True, spatial_level=1)   # intact
    assert d["verified"] == 7
    d = pmctf_spatial.decode_sequence_layer(seq["dec_net"], bins, bad, 1, "cuda", verify=False, spatial_level=1)
    assert d["verified"] == 0
    d = pmctf_spatial.decode_sequence_layer(seq["dec_net"], bins, bad, 1, verify="auto", motion_fill=True, spatial_level=1)
    assert d["verified"] == 0 and len(d["frames"]) == 7, "motion_fill output is never verified"
    # a picture_hashes.json with one altered value: the record is not written
    other = _copy(seq, "seven", "seven_bad_anchor")
    ppath = os.path.join(other, "picture_hashes.json")
    rec = json.load(open(ppath))
    rec["frames"][5]["y"] ^= 1
    json.dump(rec, open(ppath, "w"))
    with pytest.raises(pmctf_gop.PictureHashMismatch) as e:
        pmctf_spatial.write_spatial_hashes(seq["enc_net"], other)
    assert (e.value.mismatch["frame"], e.value.mismatch["plane"]) == (5, "y")
    assert not os.path.exists(os.path.join(other, "spatial_hashes.json"))


# ------------------------------------------------------------------------------------------------------ 7. other inputs
def test_ten_bits(seq):
    import hbd_restatement as hr
    import pmctf_gop
    import pmctf_seq
    import pmctf_spatial
    src = str(seq["tmp"] / "src10.yuv")
    pmctf_gop.write_yuv(src, hr.synth_hbd(W, H, 3, 10, seed=5))
    bins = str(seq["tmp"] / "ten_bits")
    os.makedirs(bins)
    r = pmctf_seq.encode_sequence_gops(seq["enc_net"], src, W, H, 3, 2, Q, bins, "cuda", bitdepth=10, picture_hash="u16")
    assert [g["size"] for g in r["gops"]] == [2, 1]
    pmctf_spatial.write_spatial_hashes(seq["enc_net"], bins)
    assert pmctf_spatial.read_spatial_hashes(bins)["level"] == "u16"
    yuv = str(seq["tmp"] / "ten_bits_s1.yuv")
    d = pmctf_spatial.decode_sequence_layer(seq["dec_net"], bins, yuv, 0, "cuda", verify=True, spatial_level=1)
    assert d["verified"] == 3 and d["bitdepth"] == 10 and d["frames"] == [(H // 2, W // 2)] * 3
    assert os.path.getsize(yuv) == 3 * _n(1) * 2
    want = _expected(seq, bins, 1, bitdepth=10)
    assert all(p.dtype == np.uint16 for planes in want for p in planes)
    _same_file(yuv, want, 1, dtype="<u2")
    assert int(np.fromfile(yuv, dtype="<u2").max()) <= 1023
    with pytest.raises(ValueError, match="picture_format.json"):
        pmctf_spatial.decode_sequence_layer(seq["dec_net"], bins, None, 0, png_out=str(seq["tmp"] / "ten_png"), spatial_level=1)


def test_reduced_resolution_motion_and_pngs(seq):
    import pmctf_gop
    import pmctf_seq
    import pmctf_spatial
    from PIL import Image
    bins = str(seq["tmp"] / "half_motion")
    os.makedirs(bins)
    r = pmctf_seq.encode_sequence_gops(seq["enc_net"], seq["src"], W, H, 4, 4, Q, bins, "cuda", structure=[(4, 2)])
    assert r["gops"] == [{"first": 0, "size": 4, "me_downsample": 2, "psize": 128}]
    yuv, png = str(seq["tmp"] / "half_motion_s1.yuv"), str(seq["tmp"] / "half_motion_png")
    d = pmctf_spatial.decode_sequence_layer(seq["dec_net"], bins, yuv, 0, "cuda", png_out=png, spatial_level=1)
    assert d["times"] == [0, 1, 2, 3] and d["size"] == (H // 2, W // 2)
    _same_file(yuv, _expected(seq, bins, 1), 1)
    assert sorted(os.listdir(png)) == ["0.png", "1.png", "2.png", "3.png"]
    with torch.no_grad():
        rec = sr.synthesis(seq["dec_net"], _entries(seq, bins, 0, 4, 1, me_downsample=2), 1)
    for i, rgb in enumerate(pmctf_gop.frames_to_rgb8([p + [None] for p in rec], H // 2, W // 2)):
        got = np.asarray(Image.open(os.path.join(png, f"{i}.png")))
        assert got.shape == (H // 2, W // 2, 3) and np.array_equal(got, rgb), f"picture {i}"
    # PNGs of a temporal level keep the source indices
    png = str(seq["tmp"] / "seven_png")
    pmctf_spatial.decode_sequence_layer(seq["dec_net"], seq["seven"], None, 1, png_out=png, spatial_level=2)
    assert sorted(os.listdir(png)) == ["0.png", "2.png", "4.png", "6.png"]
    assert Image.open(os.path.join(png, "6.png")).size == (W // 4, H // 4)


# ------------------------------------------------------------------------------------------------------------ 8. the tools
def _tool(name, argv, capsys):
    """main() of tools/{name}.py in this process with the given arguments -> the JSON object of its last output line"""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    capsys.readouterr()
    tool.main(argv)
    out = capsys.readouterr().out
    return json.loads(out[out.index("{"):]) if name == "encode_sequence" else json.loads(out.strip().splitlines()[-1])


def test_tools(seq, capsys):
    """encode --spatial-hashes, decode --spatial-level with --temporal-level, --motion-fill, --png and --output-layout"""
    import pmctf_layout
    import pmctf_spatial
    bins = str(seq["tmp"] / "tool_bins")
    _tool("encode_sequence", ["--synth-seed", "0", "--gop", "4", "--q-index", str(Q), "--structure", "fill", "--frames", "7",
                              "--width", str(W), "--height", str(H), "--picture-hash", "u8", "--spatial-hashes", seq["src"], bins],
          capsys)
    record = pmctf_spatial.read_spatial_hashes(bins)
    assert sorted(record["layers"]) == ["1", "2"] and record["level"] == "u8"
    for rel in lr.folder_files([(0, 4), (4, 2), (6, 1)], 0):             # the files of the fixture's folder, byte for byte
        assert open(os.path.join(bins, rel), "rb").read() == open(os.path.join(seq["seven"], rel), "rb").read(), rel
    nv12, png = str(seq["tmp"] / "tool_t1s1.nv12"), str(seq["tmp"] / "tool_png")
    out = _tool("decode_sequence", ["--synth-seed", "0", "--spatial-level", "1", "--temporal-level", "1", "--verify", "--png", png,
                                    "--output-layout", "nv12", bins, nv12], capsys)
    assert (out["frames"], out["verified"], out["hash_mismatches"], out["temporal_level"], out["spatial_level"]) == (4, 4, 0, 1, 1)
    assert (out["height"], out["width"]) == (H // 2, W // 2) and 0 < out["payload_bytes_used"] < out["bytes_read"]
    assert sorted(os.listdir(png)) == ["0.png", "2.png", "4.png", "6.png"]
    planar = str(seq["tmp"] / "tool_t1s1.yuv")
    assert pmctf_layout.convert_file(nv12, planar, W // 2, H // 2, "nv12", "planar", "cuda") == 4
    _same_file(planar, _expected(seq, seq["seven"], 1, t=1), 1)
    yuv = str(seq["tmp"] / "tool_fill.yuv")
    out = _tool("decode_sequence", ["--synth-seed", "0", "--spatial-level", "2", "--temporal-level", "1", "--motion-fill", bins, yuv],
                capsys)
    assert (out["frames"], out["verified"], out["motion_fill"], out["spatial_level"]) == (7, 0, True, 2)
    assert os.path.getsize(yuv) == 7 * _n(2)


# -------------------------------------------------------------------------------------------------------- 9. the refusal
def test_level_3_is_refused_before_any_file_is_opened(seq):
    import pmctf_spatial
    net = seq["dec_net"]
    yuv = str(seq["tmp"] / "never.yuv")
    for level in (3, 4):
        with pytest.raises(ValueError, match=r"136x104 offer the spatial levels 0\.\.2"):
            pmctf_spatial.decode_sequence_layer(net, seq["seven"], yuv, 0, "cuda", spatial_level=level)
        with pytest.raises(ValueError, match=r"136x104 offer the spatial levels 0\.\.2"):
            pmctf_spatial.decode_gop_files_layer(net, str(seq["tmp"] / "no_such_folder"), 4, H, W, Q, 0, spatial_level=level)
    assert not os.path.exists(yuv)
