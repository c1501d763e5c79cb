"""Spatial layers, the parts that need no GPU: the size rule and level_symbol_count against tests/spatial_restatement.py, the
spatial_hashes.json record (round trip and every refusal), the refusals of the decoders and of the tool, which come before
the codec is touched, and extract_layer carrying the record.  Everything is exact: integers, names and bytes."""
import ast
import importlib.util
import inspect
import json
import os

import pytest

import layers_restatement as lr
import pmctf_chroma
import pmctf_gop
import pmctf_layers
import pmctf_layout
import pmctf_scale
import pmctf_seq
import pmctf_spatial
import spatial_restatement as sr

W, H = 136, 104                                                          # offers the levels 1 and 2, refuses 3
GOPS = [{"first": 0, "size": 4, "me_downsample": 1, "psize": 128}, {"first": 4, "size": 2, "me_downsample": 1, "psize": 128},
        {"first": 6, "size": 1, "me_downsample": 1, "psize": 128}]
LAYOUT = [(0, 4), (4, 2), (6, 1)]
OTHERS = (2, 6, 8, 12, 16, 24, 32, 96, 136, 1080, 1920, 2160, 3840, 4400)


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the codec was touched ({name}) before the arguments were checked")


# ---------------------------------------------------------------------------------------------------------- the size rule
def test_size_rule_against_the_restatement():
    for a in range(2, 4401):
        for b in OTHERS:
            for h, w in ((a, b), (b, a)):
                top = pmctf_spatial.max_spatial_level(h, w)
                assert top == sr.top_level(h, w), (h, w)
                for level in range(6):
                    try:
                        got = pmctf_spatial.spatial_size(h, w, level)
                    except ValueError:
                        got = None
                    assert got == (sr.size(h, w, level) if sr.offered(h, w, level) else None), (h, w, level)
    assert pmctf_spatial.max_spatial_level(1080, 1920) == 2 and pmctf_spatial.max_spatial_level(2160, 3840) == 3
    assert pmctf_spatial.max_spatial_level(H, W) == 2 and pmctf_spatial.spatial_size(H, W, 2) == (26, 34)
    assert pmctf_spatial.spatial_size(1080, 1920, 2) == (270, 480) and pmctf_spatial.max_spatial_level(4096, 4096) == 4
    with pytest.raises(ValueError, match=r"136x104 offer the spatial levels 0\.\.2: level 3"):
        pmctf_spatial.spatial_size(H, W, 3)
    with pytest.raises(ValueError, match=r"1920x1080 offer the spatial levels 0\.\.2"):
        pmctf_spatial.spatial_size(1080, 1920, 3)
    for level in (-1, 5, 1.0, "1", None, True):
        with pytest.raises(ValueError, match="spatial_level"):
            pmctf_spatial.spatial_size(4096, 4096, level)
    for h, w in ((0, 8), (8, -8), (8.0, 8), (True, 8)):
        with pytest.raises(ValueError, match="picture size"):
            pmctf_spatial.max_spatial_level(h, w)


def test_level_symbol_count_against_the_restatement():
    for N in (1, 2, 3):
        for Hp in range(64, 4417, 64):
            for Wp in (64, 128, 256, 1920, 3840, 4416):
                for a, b in ((Hp, Wp), (Wp, Hp)):
                    counts = [pmctf_spatial.level_symbol_count(N, a, b, level) for level in range(5)]
                    assert counts == [sr.symbols(N, a, b, level) for level in range(5)], (N, a, b)
                    assert counts == sorted(counts, reverse=True) and counts[4] == N * (a >> 4) * (b >> 4)
                    assert counts[0] - counts[1] == 3 * N * a * b, "the finest level: three subbands, four steps each"
                    with pytest.raises(ValueError, match="spatial_level"):
                        pmctf_spatial.level_symbol_count(N, a, b, 5)
    # three quarters of a file's symbols belong to the finest level
    full, one = pmctf_spatial.level_symbol_count(1, 1152, 1920, 0), pmctf_spatial.level_symbol_count(1, 1152, 1920, 1)
    assert full - one == 3 * 1152 * 1920 and 0.75 < (full - one) / full < 0.76
    from pMCTF.hip.engine import HipEngine                                  # level 0 is the encoder's count

    class _Four:
        L = 4
    assert all(HipEngine.pwave_symbol_count(_Four, n, 128, 256) == pmctf_spatial.level_symbol_count(n, 128, 256, 0) for n in (1, 2))


def test_module_needs_no_torch_at_import_and_its_forms_extend_the_layered_ones():
    for module in (pmctf_spatial, importlib.import_module("pmctf_records")):
        tree = ast.parse(open(module.__file__).read())
        top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
        names = {a.name for n in top if isinstance(n, ast.Import) for a in n.names} | \
                {n.module for n in top if isinstance(n, ast.ImportFrom)}
        assert names <= {"os", "json", "pmctf_records"}, names
    p = inspect.signature(pmctf_spatial.decode_gop_files_layer).parameters
    assert list(p) == list(inspect.signature(pmctf_layers.decode_gop_files_layer).parameters) + ["spatial_level"]
    q = inspect.signature(pmctf_spatial.decode_sequence_layer).parameters
    assert list(q) == list(inspect.signature(pmctf_layout.decode_sequence_layer).parameters) + ["spatial_level"]
    assert p["spatial_level"].default == 0 and q["spatial_level"].default == 0
    assert list(inspect.signature(pmctf_spatial.write_spatial_hashes).parameters) == ["codec", "bin_folder", "hash_level"]
    assert list(inspect.signature(pmctf_spatial.level_symbol_count).parameters) == ["N", "Hp", "Wp", "level", "decomp_levels"]
    from pMCTF.hip.engine import HipEngine
    from pMCTF.models.pWave import pWave
    from pMCTF.models.video.pMCTF_L import pMCTF
    for fn, name in ((HipEngine.pwave_walk, "stop_level"), (HipEngine.pwave_synthesis, "level"), (HipEngine._open_file, "level"),
                     (HipEngine.pwave_decompress, "level"), (HipEngine.pwave_decompress_begin, "level"),
                     (HipEngine.pwave_decompress_many, "level"), (HipEngine.pwave_decompress_many_begin, "level"),
                     (HipEngine.pwave_decompress_batch_begin, "level"), (pWave.decompress, "spatial_level"),
                     (pMCTF.decompress_gop_files, "spatial_level"), (pMCTF._decompress_gop_files_begin, "spatial_level"),
                     (pMCTF.decompress_one_stage, "spatial_level")):
        assert inspect.signature(fn).parameters[name].default == 0, fn


# ------------------------------------------------------------------------------------------------------ a folder of dummies
def _fake_folder(path, width=W, height=H, bitdepth=8):
    """a real header over dummy bitstream files"""
    os.makedirs(path)
    pmctf_seq.write_gop_structure(path, width=width, height=height, frame_num=7, max_gop=4, q_index=3, num_me_stages=1,
                                  ll_order="plane", precision="f32", aten_threads=1, gops=GOPS)
    for rel in lr.folder_files(LAYOUT, 0):
        os.makedirs(os.path.dirname(os.path.join(path, rel)), exist_ok=True)
        open(os.path.join(path, rel), "wb").write(b"x" * 9)
    if bitdepth > 8:
        pmctf_gop.write_picture_format(path, bitdepth)
    return path


def _record(level="u8", spatial=(1, 2), temporal=(0, 1, 2)):
    keys = pmctf_gop.HASH_KEYS[level]
    return {"format_version": 1, "level": level, "size": [W, H],
            "layers": {str(k): {str(t): [dict({key: 1000 * k + 100 * t + i for i, key in enumerate(keys)}, index=index)
                                         for _, index in lr.times(LAYOUT, t)] for t in temporal} for k in spatial}}


def _put(folder, record):
    path = os.path.join(folder, "spatial_hashes.json")
    with open(path, "w") as f:
        f.write(record if isinstance(record, str) else json.dumps(record))
    return path


# ------------------------------------------------------------------------------------------------------------ the record
def test_spatial_hash_record_round_trip_and_refusals(tmp_path):
    folder = _fake_folder(str(tmp_path / "bins"))
    with pytest.raises(ValueError, match=r"spatial_hashes\.json: missing \(write_spatial_hashes was not run"):
        pmctf_spatial.read_spatial_hashes(folder)
    for level in ("u8", "f32"):
        good = _record(level)
        path = _put(folder, good)
        assert pmctf_spatial.read_spatial_hashes(folder) == good
        assert [r["index"] for r in good["layers"]["2"]["1"]] == [0, 2, 4, 6] and len(good["layers"]["1"]["0"]) == 7
    good = _record()

    def refused(record, match):
        _put(folder, record)
        with pytest.raises(ValueError, match=match) as e:
            pmctf_spatial.read_spatial_hashes(folder)
        assert path in str(e.value), "the refusal names the file"

    def changed(fn):
        rec = json.loads(json.dumps(good))
        fn(rec)
        return rec

    refused("{not json", "not a spatial hash file")
    refused("[1, 2]", "format version None")
    refused(changed(lambda r: r.update(format_version=2)), "format version 2, this decoder reads version 1")
    refused(changed(lambda r: r.update(extra=1)), r"unknown \['extra'\]")
    refused(changed(lambda r: r.pop("size")), r"missing \['size'\]")
    refused(changed(lambda r: r.update(level="u4")), "level 'u4'")
    refused(changed(lambda r: r.update(size=[H, W])), "size")
    refused(changed(lambda r: r.update(size=[W // 2, H // 2])), "size")
    refused(changed(lambda r: r["layers"].update({"3": r["layers"]["2"]})), r"offer the spatial levels \['1', '2'\]")
    refused(changed(lambda r: r["layers"].pop("2")), r"offer the spatial levels \['1', '2'\]")
    refused(changed(lambda r: r["layers"].update({"0": r["layers"]["1"]})), "offer the spatial levels")
    refused(changed(lambda r: r.update(layers=[])), "offer the spatial levels")
    refused(changed(lambda r: r["layers"]["1"].pop("0")), "spatial level 1: temporal levels")
    refused(changed(lambda r: r["layers"]["2"].update({"3": []})), "spatial level 2: temporal levels")
    refused(changed(lambda r: r["layers"].update({"1": []})), "spatial level 1: temporal levels")
    refused(changed(lambda r: r["layers"]["1"]["1"].pop()), "spatial level 1, temporal level 1: source indices")
    refused(changed(lambda r: r["layers"]["2"]["2"][1].update(index=5)), "spatial level 2, temporal level 2: source indices")
    refused(changed(lambda r: r["layers"]["1"]["0"][3].pop("cb")), "a list of records that hold exactly")
    refused(changed(lambda r: r["layers"]["1"]["0"][3].update(y_f32=1)), "a list of records that hold exactly")
    refused(changed(lambda r: r["layers"]["1"]["0"][3].update(y=-1)), "picture 3: y is not a 32-bit value")
    refused(changed(lambda r: r["layers"]["1"]["0"][3].update(y=2 ** 32)), "picture 3: y is not a 32-bit value")
    refused(changed(lambda r: r["layers"]["1"]["0"][3].update(y=1.5)), "picture 3: y is not a 32-bit value")
    # a record of levels the folder's size does not offer: the same file under a header of 132x100 (level 1 alone)
    other = _fake_folder(str(tmp_path / "narrow"), width=132, height=100)
    _put(other, changed(lambda r: r.update(size=[132, 100])))
    with pytest.raises(ValueError, match=r"narrow.spatial_hashes\.json.*132x100 offer the spatial levels \['1'\]"):
        pmctf_spatial.read_spatial_hashes(other)


# -------------------------------------------------------------------------------------------------------- the refusals
def test_decoders_refuse_before_the_codec_is_touched(tmp_path):
    folder = _fake_folder(str(tmp_path / "bins"))
    yuv = str(tmp_path / "never.yuv")
    sub = os.path.join(folder, "gop_00000")
    for level in (-1, 5, 1.0, "1", None, True):
        with pytest.raises(ValueError, match="spatial_level"):
            pmctf_spatial.decode_sequence_layer(_NoDevice(), folder, yuv, 0, spatial_level=level)
        with pytest.raises(ValueError, match="spatial_level"):
            pmctf_spatial.decode_gop_files_layer(_NoDevice(), sub, 4, H, W, 3, 0, spatial_level=level)
        with pytest.raises(ValueError, match="spatial_level"):
            pmctf_layers.LayerDecode(0, False, level)
    # a level the size does not offer, naming the size and the largest level; no file is opened ("nowhere" does not exist)
    for level in (3, 4):
        with pytest.raises(ValueError, match=r"136x104 offer the spatial levels 0\.\.2"):
            pmctf_spatial.decode_sequence_layer(_NoDevice(), folder, yuv, 0, spatial_level=level)
        with pytest.raises(ValueError, match=r"136x104 offer the spatial levels 0\.\.2"):
            pmctf_spatial.decode_gop_files_layer(_NoDevice(), "nowhere", 4, H, W, 3, 1, spatial_level=level)
    with pytest.raises(ValueError, match=r"132x100 offer the spatial levels 0\.\.1: level 2"):
        pmctf_spatial.decode_gop_files_layer(_NoDevice(), "nowhere", 4, 100, 132, 3, 0, spatial_level=2)
    # the temporal arguments are checked as before
    with pytest.raises(ValueError, match="level"):
        pmctf_spatial.decode_sequence_layer(_NoDevice(), folder, yuv, -1, spatial_level=1)
    with pytest.raises(ValueError, match="motion_fill"):
        pmctf_spatial.decode_sequence_layer(_NoDevice(), folder, yuv, 1, motion_fill=1, spatial_level=1)
    with pytest.raises(ValueError, match="motion_fill output is never verified"):
        pmctf_spatial.decode_sequence_layer(_NoDevice(), folder, yuv, 1, verify=True, motion_fill=True, spatial_level=1)
    with pytest.raises(ValueError, match="verify is"):
        pmctf_spatial.decode_sequence_layer(_NoDevice(), folder, yuv, 1, verify="yes", spatial_level=1)
    with pytest.raises(ValueError, match="nothing to write"):
        pmctf_spatial.decode_sequence_layer(_NoDevice(), folder, None, 1, spatial_level=1)
    # verify=True without the record
    with pytest.raises(ValueError, match=r"spatial_hashes\.json: missing"):
        pmctf_spatial.decode_sequence_layer(_NoDevice(), folder, yuv, 0, verify=True, spatial_level=1)
    # a display form that is not the coded form: only with the coded-form output the caller asks for
    shown = _fake_folder(str(tmp_path / "shown"))
    pmctf_scale.write_display_format(shown, 2 * W, 2 * H)
    for kwargs in ({}, {"coded_format_output": True}):
        with pytest.raises(ValueError, match=r"shown.display_format\.json.*spatial level 1"):
            pmctf_spatial.decode_sequence_layer(_NoDevice(), shown, yuv, 0, spatial_level=1, **kwargs)
    with pytest.raises(ValueError, match=r"spatial_hashes\.json: missing"):     # accepted up to the next refusal
        pmctf_spatial.decode_sequence_layer(_NoDevice(), shown, yuv, 0, verify=True, spatial_level=1, coded_size_output=True)
    other = _fake_folder(str(tmp_path / "other_format"))
    pmctf_chroma.write_source_format(other, "422", "left")
    for kwargs in ({}, {"coded_size_output": True}):
        with pytest.raises(ValueError, match=r"other_format.source_format\.json.*spatial level 2"):
            pmctf_spatial.decode_sequence_layer(_NoDevice(), other, yuv, 1, spatial_level=2, **kwargs)
    with pytest.raises(ValueError, match=r"spatial_hashes\.json: missing"):
        pmctf_spatial.decode_sequence_layer(_NoDevice(), other, yuv, 1, verify=True, spatial_level=2, coded_format_output=True)
    same = _fake_folder(str(tmp_path / "y4m_420"))                             # a 4:2:0 .y4m source: coded form = display form
    pmctf_chroma.write_source_format(same, "420", "left", (30, 1))
    with pytest.raises(ValueError, match=r"spatial_hashes\.json: missing"):
        pmctf_spatial.decode_sequence_layer(_NoDevice(), same, yuv, 0, verify=True, spatial_level=1)
    # an extracted folder refuses as before, and write_spatial_hashes refuses it
    small = str(tmp_path / "level1")
    pmctf_layers.extract_layer(folder, small, 1)
    with pytest.raises(ValueError, match="layer_extract.json.*level 1 and above"):
        pmctf_spatial.decode_sequence_layer(_NoDevice(), small, yuv, 0, spatial_level=1)
    with pytest.raises(ValueError, match="layer_extract.json"):
        pmctf_spatial.write_spatial_hashes(_NoDevice(), small)
    hbd = _fake_folder(str(tmp_path / "hbd"), bitdepth=10)
    with pytest.raises(ValueError, match="does not go with bitdepth 10"):
        pmctf_spatial.write_spatial_hashes(_NoDevice(), hbd, hash_level="u8")
    with pytest.raises(ValueError, match="picture_format.json"):
        pmctf_spatial.decode_sequence_layer(_NoDevice(), hbd, yuv, 0, png_out=str(tmp_path / "png"), spatial_level=1)
    assert not os.path.exists(yuv) and not os.path.exists(str(tmp_path / "png"))


def test_tool_refuses_before_the_weights_are_loaded(tmp_path, capsys):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("decode_sequence", os.path.join(root, "tools", "decode_sequence.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    folder = _fake_folder(str(tmp_path / "bins"))
    shown = _fake_folder(str(tmp_path / "shown"))
    pmctf_scale.write_display_format(shown, 2 * W, 2 * H)
    yuv = str(tmp_path / "never.yuv")
    base = ["--synth-seed", "0", "--device", "no-such-device"]
    for argv, text in ((["--spatial-level", "3", folder, yuv], "136x104 offer the spatial levels 0..2"),
                       (["--spatial-level", "5", folder, yuv], "--spatial-level is 0 to 4"),
                       (["--spatial-level", "-1", folder, yuv], "--spatial-level is 0 to 4"),
                       (["--spatial-level", "1", "--verify", folder, yuv], "spatial_hashes.json: missing"),
                       (["--spatial-level", "1", "--temporal-level", "1", "--motion-fill", "--verify", folder, yuv], "--motion-fill"),
                       (["--spatial-level", "1", shown, yuv], "display_format.json"),
                       (["--spatial-level", "2", "--coded-size-output", "--verify", shown, yuv], "spatial_hashes.json: missing")):
        with pytest.raises(SystemExit) as e:
            tool.main(base + argv)
        assert e.value.code == 2 and text in capsys.readouterr().err, argv
    assert not os.path.exists(yuv)


# ------------------------------------------------------------------------------------------------------ extracted folders
def test_extract_layer_carries_the_record(tmp_path):
    src = _fake_folder(str(tmp_path / "src"))
    record = _record()
    _put(src, record)
    for level in (0, 1, 2):
        dst = str(tmp_path / f"dst{level}")
        written = pmctf_layers.extract_layer(src, dst, level)
        assert "spatial_hashes.json" in written
        assert open(os.path.join(dst, "spatial_hashes.json"), "rb").read() == open(os.path.join(src, "spatial_hashes.json"), "rb").read()
        assert pmctf_spatial.read_spatial_hashes(dst) == record, "the layout of an extracted folder is the source's"
    os.remove(os.path.join(src, "spatial_hashes.json"))
    assert "spatial_hashes.json" not in pmctf_layers.extract_layer(src, str(tmp_path / "without"), 1)
