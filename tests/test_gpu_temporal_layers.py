"""Temporal layers on the GPU (pmctf_layers) at 132x100, padded to 256x128, q 3: a decode at level k from the files of
that level alone against the full decode's synthesis stopped after stage k (tests/layers_restatement.py), the files that
are read and those that are not, motion_fill against decode_gop on zeroed high bands, a structured sequence of 7 pictures,
the layer hashes end to end with a second model and an extracted folder, ten bits, reduced-resolution motion, the tools.
Everything is exact: torch.equal, bytes and integers.  No bitstream file that is decoded is ever altered: the tampering
is done on JSON records and on files outside the set that is read."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import layers_restatement as lr
from helpers import product_model

pytestmark = pytest.mark.gpu

W, H, Q = 132, 100, 3
N8 = W * H * 3 // 2                                    # samples of one 4:2:0 picture


@pytest.fixture(scope="module")
def seq(cuda, tmp_path_factory):
    """one encoder model, one decoder model (same weights), the source, and the folders coded once: one GOP of 8, and 7
    pictures as GOPs of 4, 2, 1 with picture hashes.  Tests copy a folder before they change anything in it."""
    import pmctf_gop
    import pmctf_seq
    import pmctf_synth
    tmp = tmp_path_factory.mktemp("temporal_layers")
    out = {"tmp": tmp, "enc_net": product_model(1)[0], "dec_net": product_model(1)[0], "full": {}}
    out["src8"] = str(tmp / "src8.yuv")
    pmctf_gop.write_yuv(out["src8"], pmctf_synth.synth_yuv420(W, H, 8, seed=1234))
    out["eight"], out["seven"] = str(tmp / "eight"), str(tmp / "seven")
    for name in ("eight", "seven"):
        os.makedirs(out[name])
    r = pmctf_seq.encode_sequence_gops(out["enc_net"], out["src8"], W, H, 8, 8, Q, out["eight"], "cuda")
    assert [g["size"] for g in r["gops"]] == [8]
    r = pmctf_seq.encode_sequence_gops(out["enc_net"], out["src8"], W, H, 7, 4, Q, out["seven"], "cuda", picture_hash="u8")
    assert [g["size"] for g in r["gops"]] == [4, 2, 1]
    # the reference of the one GOP of 8, computed once and left alone: its full decode, and the synthesis stopped per level
    out["gop8"] = os.path.join(out["eight"], "gop_00000")
    out["full8"] = pmctf_gop.decode_gop_files(out["dec_net"], out["gop8"], 8, H, W, Q)
    with torch.no_grad():
        out["want8"] = {k: lr.truncated_synthesis(out["dec_net"], out["full8"]["frames_coded"], k) for k in (0, 1, 2, 3)}
    return out


def _same_pictures(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a[0].shape == b[0].shape and a[1].shape == b[1].shape, i
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), f"picture {i}"


def _copy(seq, name, to):
    dst = str(seq["tmp"] / to)
    shutil.copytree(seq[name], dst)
    return dst


def _expected(seq, folder, level, bitdepth=8):
    """the pictures of a level of a whole folder, GOP by GOP: the full decode of decode_gop_files, its synthesis stopped
    after the stage, converted as the decoder converts"""
    import pmctf_gop
    header, gops = pmctf_gop.sequence_layout(folder)
    if folder not in seq["full"]:                                        # every GOP's full decode, once per folder
        seq["full"][folder] = [pmctf_gop.decode_gop_files(seq["dec_net"], os.path.join(folder, pmctf_gop.gop_folder(k)), size,
                                                          H, W, Q, psize=psize, me_downsample=ds)["frames_coded"]
                               for k, (first, size, psize, ds) in enumerate(gops)]
    out = []
    for coded in seq["full"][folder]:
        with torch.no_grad():
            rec = [p + [None] for p in lr.truncated_synthesis(seq["dec_net"], coded, level)]
        out += pmctf_gop.frames_to_samples(rec, H, W, bitdepth)
    return out


def _flat(planes):
    return np.concatenate([p.reshape(-1) for p in planes])


# ------------------------------------------------------------------------------------------------------ 1. one GOP of 8
def test_one_gop_against_the_full_decode(seq):
    import pmctf_layers
    full, want = seq["full8"], seq["want8"]
    _same_pictures(want[0], full["frames"])                              # the restatement is decode_gop when it runs to the end
    for k in (0, 1, 2, 3, 5):
        got = pmctf_layers.decode_gop_files_layer(seq["dec_net"], seq["gop8"], 8, H, W, Q, k)
        kk = min(k, 3)
        assert got["times"] == list(range(0, 8, 2 ** kk)) and got["stages"] == 3
        assert got["files"] == lr.file_names(8, k)
        assert got["bytes_read"] == sum(os.path.getsize(os.path.join(seq["gop8"], n)) for n in got["files"])
        _same_pictures(got["frames"], want[kk])
        assert all(p[2] is None for p in got["frames"])
        if k == 0:
            _same_pictures(got["frames"], full["frames"])
        if kk == 3:                                                      # no synthesis: the decoded L planes as they are
            _same_pictures(got["frames"], [full["frames_coded"][0]])
    # the entries that were read are the full decode's, the others were never touched
    got = pmctf_layers.decode_gop_files_layer(seq["dec_net"], seq["gop8"], 8, H, W, Q, 2)
    for i, (a, b) in enumerate(zip(got["frames_coded"], full["frames_coded"])):
        if i in (0, 4):
            assert all(torch.equal(x, y) for x, y in zip(a, b) if y is not None) and (a[2] is None) == (b[2] is None)
        else:
            assert a == [None, None, None]


# ------------------------------------------------------------------------------------------- 2. only the needed files
def test_only_the_files_of_the_level_are_read(seq):
    import pmctf_gop
    import pmctf_layers
    folder = os.path.join(_copy(seq, "eight", "eight_level2"), "gop_00000")
    keep = pmctf_layers.layer_file_names(8, 2)
    others = [n for n in pmctf_gop.gop_file_names(8) if n not in keep]
    assert len(keep) == 5 and len(others) == 18
    for n in others:
        os.remove(os.path.join(folder, n))
    assert sorted(os.listdir(folder)) == sorted(keep)
    got = pmctf_layers.decode_gop_files_layer(seq["dec_net"], folder, 8, H, W, Q, 2)
    _same_pictures(got["frames"], seq["want8"][2])
    for n in others:                                                     # garbage too short for any header
        open(os.path.join(folder, n), "wb").write(b"abc")
    got = pmctf_layers.decode_gop_files_layer(seq["dec_net"], folder, 8, H, W, Q, 2)
    _same_pictures(got["frames"], seq["want8"][2])
    assert got["times"] == [0, 4] and got["files"] == keep
    os.remove(os.path.join(folder, "4_C_main.bin"))
    with pytest.raises(ValueError, match="4_C_main.bin: missing"):
        pmctf_layers.decode_gop_files_layer(seq["dec_net"], folder, 8, H, W, Q, 2)
    got = pmctf_layers.decode_gop_files_layer(seq["dec_net"], folder, 8, H, W, Q, 3)      # level 3 does not need it
    _same_pictures(got["frames"], seq["want8"][3])


# ------------------------------------------------------------------------------------------------------ 3. motion_fill
def test_motion_fill_is_decode_gop_on_zeroed_high_bands(seq):
    import pmctf_gop
    import pmctf_layers
    coded = [list(e) for e in seq["full8"]["frames_coded"]]
    low = [i for s, _, i in pmctf_gop.gop_pairs(8) if s < 2]
    assert low == [1, 3, 5, 7, 2, 6]
    for i in low:
        coded[i][0], coded[i][1] = torch.zeros_like(coded[i][0]), torch.zeros_like(coded[i][1])
    with torch.no_grad():
        want = pmctf_gop.decode_gop(seq["dec_net"], coded)
    got = pmctf_layers.decode_gop_files_layer(seq["dec_net"], seq["gop8"], 8, H, W, Q, 2, motion_fill=True)
    assert got["times"] == list(range(8)) and len(got["frames"]) == 8
    assert got["files"] == lr.file_names(8, 2, True)
    _same_pictures(got["frames"], want)
    assert any(bool(seq["full8"]["frames_coded"][i][0].any()) for i in low), "the high bands left out are not zero anyway"
    # with those stages' picture files gone
    folder = os.path.join(_copy(seq, "eight", "eight_fill"), "gop_00000")
    for i in low:
        os.remove(os.path.join(folder, f"{i}.bin"))
        os.remove(os.path.join(folder, f"{i}_C_main.bin"))
    again = pmctf_layers.decode_gop_files_layer(seq["dec_net"], folder, 8, H, W, Q, 2, motion_fill=True)
    _same_pictures(again["frames"], want)
    os.remove(os.path.join(folder, "3_mv.bin"))
    with pytest.raises(ValueError, match="3_mv.bin: missing"):
        pmctf_layers.decode_gop_files_layer(seq["dec_net"], folder, 8, H, W, Q, 2, motion_fill=True)
    got = pmctf_layers.decode_gop_files_layer(seq["dec_net"], folder, 8, H, W, Q, 2)          # level 2 itself does not read it
    _same_pictures(got["frames"], seq["want8"][2])


# ----------------------------------------------------------------------------------------------- 4. a structured sequence
def test_structured_sequence(seq):
    import pmctf_gop
    import pmctf_layers
    bins = seq["seven"]
    for level, times in ((1, [0, 2, 4, 6]), (2, [0, 4, 6]), (3, [0, 4, 6])):
        yuv = str(seq["tmp"] / f"seven_level{level}.yuv")
        d = pmctf_layers.decode_sequence_layer(seq["dec_net"], bins, yuv, level, "cuda")
        assert d["times"] == times and d["level"] == level and d["frames"] == [(H, W)] * len(times) and d["bitdepth"] == 8
        assert d["verified"] == 0 and d["hash_mismatches"] == [], "no layer_hashes.json here: nothing to check under auto"
        assert d["bytes_read"] == pmctf_layers.layer_bytes(bins, level)
        assert d["header"] == pmctf_gop.sequence_layout(bins)[0] and len(d["seconds"]) == 3
        data = np.fromfile(yuv, dtype=np.uint8)
        assert data.size == len(times) * N8
        want = _expected(seq, bins, level)
        assert len(want) == len(times)
        for i, planes in enumerate(want):
            assert np.array_equal(data[i * N8:(i + 1) * N8], _flat(planes)), f"level {level}, picture {i}"
    # level 0: the bytes of decode_sequence, verified against picture_hashes.json as it verifies
    old, new = str(seq["tmp"] / "seven_old.yuv"), str(seq["tmp"] / "seven_level0.yuv")
    a = pmctf_gop.decode_sequence(seq["dec_net"], bins, old, "cuda")
    b = pmctf_layers.decode_sequence_layer(seq["dec_net"], bins, new, 0, "cuda")
    assert open(old, "rb").read() == open(new, "rb").read() and os.path.getsize(new) == 7 * N8
    assert a["verified"] == b["verified"] == 7 and b["times"] == list(range(7)) and b["hash_mismatches"] == []
    assert b["bytes_read"] == pmctf_layers.layer_bytes(bins, 0)
    assert pmctf_layers.layer_bytes(bins, 2) < pmctf_layers.layer_bytes(bins, 1) < pmctf_layers.layer_bytes(bins, 0)
    # PNGs carry the source indices
    png = str(seq["tmp"] / "seven_png")
    pmctf_layers.decode_sequence_layer(seq["dec_net"], bins, None, 1, png_out=png)
    assert sorted(os.listdir(png)) == ["0.png", "2.png", "4.png", "6.png"]
    # every picture from the files of level 1 and the motion of stage 0; never verified
    fill = str(seq["tmp"] / "seven_fill.yuv")
    d = pmctf_layers.decode_sequence_layer(seq["dec_net"], bins, fill, 1, motion_fill=True)
    assert d["times"] == list(range(7)) and d["verified"] == 0 and os.path.getsize(fill) == 7 * N8
    assert d["bytes_read"] == pmctf_layers.layer_bytes(bins, 1, True)


# ------------------------------------------------------------------------------------------------- 5. hashes end to end
def test_layer_hashes_end_to_end(seq):
    import pmctf_gop
    import pmctf_layers
    bins = _copy(seq, "seven", "seven_hashed")
    path = pmctf_layers.write_layer_hashes(seq["enc_net"], bins)
    assert path == os.path.join(bins, "layer_hashes.json")
    record = pmctf_layers.read_layer_hashes(bins)
    assert record["level"] == "u8" and sorted(record["layers"]) == ["1", "2"]
    assert [r["index"] for r in record["layers"]["1"]] == [0, 2, 4, 6]
    assert [r["index"] for r in record["layers"]["2"]] == [0, 4, 6]
    # pictures that belong to both layers as the same picture have the same hashes: the lone picture, the GOP of 2's L
    by = lambda k: {r["index"]: r for r in record["layers"][k]}
    assert by("1")[6] == by("2")[6] and by("1")[4] == by("2")[4] and by("1")[0] != by("2")[0]
    full = pmctf_gop.read_picture_hashes(bins, 7)["frames"]
    assert {k: v for k, v in by("1")[6].items() if k != "index"} == full[6]
    small = str(seq["tmp"] / "seven_level1")
    pmctf_layers.extract_layer(bins, small, 1)
    assert not os.path.exists(os.path.join(small, "picture_hashes.json"))
    assert not os.path.exists(os.path.join(small, "gop_00000", "1.bin"))
    for level, count in ((1, 4), (2, 3)):
        yuv = str(seq["tmp"] / f"small_level{level}.yuv")
        d = pmctf_layers.decode_sequence_layer(seq["dec_net"], small, yuv, level, "cuda", verify=True)
        assert d["verified"] == count == len(d["frames"]) and d["hash_mismatches"] == []
        assert os.path.getsize(yuv) == count * N8
        want = _expected(seq, seq["seven"], level)                      # the same bitstream files
        data = np.fromfile(yuv, dtype=np.uint8)
        for i, planes in enumerate(want):
            assert np.array_equal(data[i * N8:(i + 1) * N8], _flat(planes)), f"level {level}, picture {i}"
    with pytest.raises(ValueError, match="layer_extract.json"):
        pmctf_layers.decode_sequence_layer(seq["dec_net"], small, str(seq["tmp"] / "never.yuv"), 0, "cuda")
    with pytest.raises(ValueError, match="layer_extract.json"):
        pmctf_layers.decode_sequence_layer(seq["dec_net"], small, str(seq["tmp"] / "never.yuv"), 1, motion_fill=True)
    assert not os.path.exists(str(seq["tmp"] / "never.yuv"))
    # one recorded value changed, no bitstream touched: picture 4 (GOP 1) of layer 1
    lpath = os.path.join(small, "layer_hashes.json")
    rec = json.load(open(lpath))
    assert rec["layers"]["1"][2]["index"] == 4
    rec["layers"]["1"][2]["cb"] ^= 1
    json.dump(rec, open(lpath, "w"))
    yuv = str(seq["tmp"] / "small_tampered.yuv")
    with pytest.raises(pmctf_gop.PictureHashMismatch) as e:
        pmctf_layers.decode_sequence_layer(seq["dec_net"], small, yuv, 1, "cuda")
    m = e.value.mismatch
    assert (m["frame"], m["plane"], m["gop"]) == (4, "cb", 1) and m["recorded"] == m["decoded"] ^ 1
    assert "frame 4, plane cb" in str(e.value) and "gop_00001" in str(e.value)
    assert os.path.getsize(yuv) == 2 * N8, "GOP 0 was written, nothing of GOP 1"
    d = pmctf_layers.decode_sequence_layer(seq["dec_net"], small, yuv, 1, "cuda", verify="report")
    assert os.path.getsize(yuv) == 4 * N8 and d["verified"] == 4
    assert [(x["frame"], x["plane"]) for x in d["hash_mismatches"]] == [(4, "cb")]
    d = pmctf_layers.decode_sequence_layer(seq["dec_net"], small, yuv, 2, "cuda", verify=True)      # layer 2's record is intact
    assert d["verified"] == 3 and d["hash_mismatches"] == []
    d = pmctf_layers.decode_sequence_layer(seq["dec_net"], small, yuv, 1, "cuda", verify=False)
    assert d["verified"] == 0 and os.path.getsize(yuv) == 4 * N8
    # a picture_hashes.json with one altered value: the layer record is not written
    other = _copy(seq, "seven", "seven_bad_anchor")
    ppath = os.path.join(other, "picture_hashes.json")
    rec = json.load(open(ppath))
    rec["frames"][5]["y"] ^= 1
    json.dump(rec, open(ppath, "w"))
    with pytest.raises(pmctf_gop.PictureHashMismatch) as e:
        pmctf_layers.write_layer_hashes(seq["enc_net"], other)
    assert (e.value.mismatch["frame"], e.value.mismatch["plane"]) == (5, "y")
    assert not os.path.exists(os.path.join(other, "layer_hashes.json"))
    with pytest.raises(ValueError, match="layer_hashes.json: missing"):
        pmctf_layers.decode_sequence_layer(seq["dec_net"], other, yuv, 1, "cuda", verify=True)


# ---------------------------------------------------------------------------------------------------------- 6. ten bits
def test_ten_bits(seq):
    import hbd_restatement as hr
    import pmctf_gop
    import pmctf_layers
    import pmctf_seq
    src = str(seq["tmp"] / "src10.yuv")
    pmctf_gop.write_yuv(src, hr.synth_hbd(W, H, 5, 10, seed=5))
    bins = str(seq["tmp"] / "ten_bits")
    os.makedirs(bins)
    r = pmctf_seq.encode_sequence_gops(seq["enc_net"], src, W, H, 5, 4, Q, bins, "cuda", bitdepth=10, picture_hash="u16")
    assert [g["size"] for g in r["gops"]] == [4, 1]
    pmctf_layers.write_layer_hashes(seq["enc_net"], bins, hash_level="u16")
    record = pmctf_layers.read_layer_hashes(bins)
    assert record["level"] == "u16" and [r["index"] for r in record["layers"]["1"]] == [0, 2, 4]
    yuv = str(seq["tmp"] / "ten_bits_level1.yuv")
    d = pmctf_layers.decode_sequence_layer(seq["dec_net"], bins, yuv, 1, "cuda", verify=True)
    assert d["times"] == [0, 2, 4] and d["verified"] == 3 and d["bitdepth"] == 10 and d["hash_mismatches"] == []
    data = np.fromfile(yuv, dtype="<u2")
    assert data.size == 3 * N8 and int(data.max()) <= 1023
    want = _expected(seq, bins, 1, bitdepth=10)
    assert len(want) == 3
    for i, planes in enumerate(want):
        assert all(p.dtype == np.uint16 for p in planes)
        assert np.array_equal(data[i * N8:(i + 1) * N8], hr.flat(planes)), f"picture {i}"
    with pytest.raises(ValueError, match="picture_format.json"):
        pmctf_layers.decode_sequence_layer(seq["dec_net"], bins, None, 1, png_out=str(seq["tmp"] / "ten_png"))


# --------------------------------------------------------------------------------------- 7. reduced-resolution motion
def test_reduced_resolution_motion(seq):
    import pmctf_gop
    import pmctf_layers
    import pmctf_seq
    bins = str(seq["tmp"] / "half_motion")
    os.makedirs(bins)
    r = pmctf_seq.encode_sequence_gops(seq["enc_net"], seq["src8"], W, H, 4, 4, Q, bins, "cuda", structure=[(4, 2)])
    assert r["gops"] == [{"first": 0, "size": 4, "me_downsample": 2, "psize": 128}]
    folder = os.path.join(bins, "gop_00000")
    full = pmctf_gop.decode_gop_files(seq["dec_net"], folder, 4, H, W, Q, psize=128, me_downsample=2)
    with torch.no_grad():
        want = lr.truncated_synthesis(seq["dec_net"], full["frames_coded"], 1)
    got = pmctf_layers.decode_gop_files_layer(seq["dec_net"], folder, 4, H, W, Q, 1, psize=128, me_downsample=2)
    assert got["times"] == [0, 2] and got["files"] == ["2.bin", "2_C_main.bin", "2_mv.bin", "0_main.bin", "0_C_main.bin"]
    _same_pictures(got["frames"], want)
    yuv = str(seq["tmp"] / "half_motion_level1.yuv")
    d = pmctf_layers.decode_sequence_layer(seq["dec_net"], bins, yuv, 1, "cuda")
    data = np.fromfile(yuv, dtype=np.uint8)
    assert d["times"] == [0, 2] and data.size == 2 * N8
    for i, planes in enumerate(pmctf_gop.frames_to_u8([p + [None] for p in want], H, W)):
        assert np.array_equal(data[i * N8:(i + 1) * N8], _flat(planes)), f"picture {i}"


# ------------------------------------------------------------------------------------------------------------ 8. the tools
def _tool(name, argv, monkeypatch, capsys):
    """main() of tools/{name}.py in this process with the given arguments -> the JSON object of its last output line"""
    import importlib.util
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.setattr(sys, "argv", [name + ".py"] + argv)
    capsys.readouterr()
    tool.main()
    out = capsys.readouterr().out
    return json.loads(out[out.index("{"):]) if name == "encode_sequence" else json.loads(out.strip().splitlines()[-1])


def test_tools(seq, monkeypatch, capsys):
    """encode --layer-hashes, extract, decode --temporal-level / --motion-fill: the options reach pmctf_layers"""
    import pmctf_layers
    bins, small = str(seq["tmp"] / "tool_bins"), str(seq["tmp"] / "tool_small")
    _tool("encode_sequence", ["--synth-seed", "0", "--gop", "4", "--q-index", str(Q), "--structure", "fill", "--frames", "7",
                              "--width", str(W), "--height", str(H), "--picture-hash", "u8", "--layer-hashes", seq["src8"], bins],
          monkeypatch, capsys)
    record = pmctf_layers.read_layer_hashes(bins)
    assert [r["index"] for r in record["layers"]["1"]] == [0, 2, 4, 6] and record["level"] == "u8"
    for rel in lr.folder_files([(0, 4), (4, 2), (6, 1)], 0):             # the files of the fixture's folder, byte for byte
        assert open(os.path.join(bins, rel), "rb").read() == open(os.path.join(seq["seven"], rel), "rb").read(), rel
    out = _tool("extract_temporal_layer", [bins, small, "1", "--motion"], monkeypatch, capsys)
    assert out["bytes"] == pmctf_layers.layer_bytes(bins, 1, True) and out["source_bytes"] == pmctf_layers.layer_bytes(bins, 0)
    yuv = str(seq["tmp"] / "tool_level1.yuv")
    out = _tool("decode_sequence", ["--synth-seed", "0", "--temporal-level", "1", "--verify", small, yuv], monkeypatch, capsys)
    assert (out["frames"], out["verified"], out["hash_mismatches"], out["temporal_level"]) == (4, 4, 0, 1)
    assert out["bytes_read"] == pmctf_layers.layer_bytes(bins, 1) and out["motion_fill"] is False
    data = np.fromfile(yuv, dtype=np.uint8)
    for i, planes in enumerate(_expected(seq, seq["seven"], 1)):
        assert np.array_equal(data[i * N8:(i + 1) * N8], _flat(planes)), f"picture {i}"
    out = _tool("decode_sequence", ["--synth-seed", "0", "--temporal-level", "1", "--motion-fill", small, yuv], monkeypatch, capsys)
    assert (out["frames"], out["verified"], out["motion_fill"]) == (7, 0, True) and os.path.getsize(yuv) == 7 * N8
    assert out["bytes_read"] == pmctf_layers.layer_bytes(bins, 1, True)
