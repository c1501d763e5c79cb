"""Temporal layers, the parts that need no GPU: the plan (layer_times, layer_file_names, layer_bytes) exhaustively against
tests/layers_restatement.py, extract_layer on a folder of dummy files under a real header, the layer_hashes.json record
(round trip and every refusal) and the argument refusals of the decoders, which come before the codec is touched.
Everything is exact: names, integers and bytes."""
import inspect
import json
import os

import pytest

import layers_restatement as lr
import pmctf_gop
import pmctf_layers
import pmctf_seq

SIZES = (1, 2, 4, 8, 16)
LEVELS = range(6)


# ------------------------------------------------------------------------------------------------------------- the plan
def test_layer_file_names_exhaustively():
    for gop in SIZES:
        S = lr.log2(gop)
        full = pmctf_gop.gop_file_names(gop) if gop > 1 else ["0_main.bin", "0_C_main.bin"]
        for fill in (False, True):
            assert pmctf_layers.layer_file_names(gop, 0, fill) == full, "level 0 is gop_file_names"
            for level in LEVELS:
                got = pmctf_layers.layer_file_names(gop, level, fill)
                assert got == lr.file_names(gop, level, fill), (gop, level, fill)
                assert len(set(got)) == len(got)
                assert [n for n in full if n in got] == got, "a subsequence of gop_file_names: the same order"
                if level:
                    assert set(got) <= set(pmctf_layers.layer_file_names(gop, level - 1, fill)), "files(k) within files(k-1)"
                if level >= S:
                    assert got == pmctf_layers.layer_file_names(gop, S, fill), "saturation"
                pictures = 2 * (gop >> min(level, S))                        # luma and chroma file per picture that is read
                assert sum(not n.endswith("_mv.bin") for n in got) == pictures
                assert sum(n.endswith("_mv.bin") for n in got) == (gop - 1 if fill else (gop >> min(level, S)) - 1)
        assert pmctf_layers.layer_file_names(gop, S, False) == ["0_main.bin", "0_C_main.bin"], "all high bands left out"
    assert pmctf_layers.layer_file_names(8, 2) == ["4.bin", "4_C_main.bin", "4_mv.bin", "0_main.bin", "0_C_main.bin"]
    assert pmctf_layers.layer_file_names(8, 2, True) == ["1_mv.bin", "3_mv.bin", "5_mv.bin", "7_mv.bin", "2_mv.bin", "6_mv.bin",
                                                         "4.bin", "4_C_main.bin", "4_mv.bin", "0_main.bin", "0_C_main.bin"]
    assert pmctf_layers.layer_file_names(8, 9) == ["0_main.bin", "0_C_main.bin"]
    for gop in (0, 3, 6, -4, 4.0, True):
        with pytest.raises(ValueError):
            pmctf_layers.layer_file_names(gop, 1)


def test_layer_times_exhaustively():
    for gop in SIZES:
        for level in LEVELS:
            for first in (0, 5):
                got = pmctf_layers.layer_times([(first, gop, 128, 1)], level)
                assert got == lr.times([(first, gop)], level), (gop, level)
                assert len(got) == max(1, gop >> level) and got[0] == (0, first)
        assert pmctf_layers.layer_times([(3, gop, 128, 1)], 0) == [(0, 3 + j) for j in range(gop)], "level 0: every picture"
        assert pmctf_layers.layer_times([(3, gop, 128, 1)], 5) == [(0, 3)], "saturation: the one low-band picture"
    assert pmctf_layers.layer_times([(0, 4), (4, 2), (6, 1)], 1) == [(0, 0), (0, 2), (1, 4), (2, 6)]
    assert pmctf_layers.layer_times([(0, 4), (4, 2), (6, 1)], 2) == [(0, 0), (1, 4), (2, 6)]
    assert pmctf_layers.layer_times([(0, 4), (4, 2), (6, 1)], 3) == [(0, 0), (1, 4), (2, 6)]


def test_layer_times_over_planned_sequences():
    for max_gop in (2, 4, 8, 16):
        for n in range(1, 41):
            gops = pmctf_seq.plan_gops(n, max_gop)
            previous = None
            for level in LEVELS:
                got = pmctf_layers.layer_times(gops, level)
                assert got == lr.times(gops, level), (n, max_gop, level)
                ts = [t for _, t in got]
                assert ts == sorted(set(ts)) and [k for k, _ in got] == sorted(k for k, _ in got)
                assert {k for k, _ in got} == set(range(len(gops))), "every GOP gives at least one picture"
                assert all(first in ts for first, _ in gops), "the first picture of every GOP is in every layer"
                assert previous is None or set(ts) <= previous, "the pictures of a level are among those of the level below"
                previous = set(ts)
            assert [t for _, t in pmctf_layers.layer_times(gops, 0)] == list(range(n))


def test_level_refusals_of_the_plan():
    for level in (-1, 1.0, "1", None, True):
        with pytest.raises(ValueError, match="level"):
            pmctf_layers.layer_times([(0, 4)], level)
        with pytest.raises(ValueError, match="level"):
            pmctf_layers.layer_file_names(4, level)
        with pytest.raises(ValueError, match="level"):
            pmctf_layers.layer_bytes("nowhere", level)


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the codec was touched ({name}) before the arguments were checked")


class _Stages:
    """a codec that is asked for nothing but its number of motion stages"""
    num_me_stages = 1


# ------------------------------------------------------------------------------------------------------ a folder of dummies
GOPS = [{"first": 0, "size": 4, "me_downsample": 1, "psize": 128}, {"first": 4, "size": 2, "me_downsample": 1, "psize": 128},
        {"first": 6, "size": 1, "me_downsample": 1, "psize": 128}]
LAYOUT = [(0, 4), (4, 2), (6, 1)]


def _fake_folder(path, structured=True, picture_hashes=True, bitdepth=8):
    """a real header over dummy files whose sizes are all different -> {relative path: size}"""
    os.makedirs(path)
    if structured:
        pmctf_seq.write_gop_structure(path, width=132, height=100, frame_num=7, max_gop=4, q_index=3, num_me_stages=1,
                                      ll_order="plane", precision="f32", aten_threads=1, gops=GOPS)
        layout = LAYOUT
    else:
        pmctf_gop.write_sequence_header(path, width=132, height=100, frame_num=8, gop=4, q_index=3, psize=128, me_downsample=1,
                                        num_me_stages=1, ll_order="plane", precision="f32", aten_threads=1)
        layout = [(0, 4), (4, 4)]
    sizes = {}
    for rel in lr.folder_files(layout, 0):
        os.makedirs(os.path.dirname(os.path.join(path, rel)), exist_ok=True)
        sizes[rel] = 2 ** len(sizes) + 3                                  # any subset has its own sum
        open(os.path.join(path, rel), "wb").write(b"x" * sizes[rel])
    if picture_hashes:
        pmctf_gop.write_picture_hashes(path, "u8", [{"y": i, "cb": 1, "cr": 2, "frame": 3} for i in range(7 if structured else 8)])
    if bitdepth > 8:
        pmctf_gop.write_picture_format(path, bitdepth)
    return sizes


def _tree(path):
    return sorted(os.path.relpath(os.path.join(base, n), path) for base, _, names in os.walk(path) for n in names)


def test_layer_bytes_is_the_sum_of_the_sizes(tmp_path):
    for structured, layout in ((True, LAYOUT), (False, [(0, 4), (4, 4)])):
        folder = str(tmp_path / f"bins{structured}")
        sizes = _fake_folder(folder, structured)
        for level in LEVELS:
            for fill in (False, True):
                want = sum(sizes[rel] for rel in lr.folder_files(layout, level, fill))
                assert pmctf_layers.layer_bytes(folder, level, fill) == want, (level, fill)
        assert pmctf_layers.layer_bytes(folder, 0) == sum(sizes.values())
        assert pmctf_layers.layer_bytes(folder, 1) < pmctf_layers.layer_bytes(folder, 1, True) < pmctf_layers.layer_bytes(folder, 0)
    os.remove(os.path.join(folder, "gop_00001", "2_mv.bin"))
    with pytest.raises(ValueError, match="2_mv.bin"):
        pmctf_layers.layer_bytes(folder, 1)
    assert pmctf_layers.layer_bytes(folder, 2) > 0                        # that file is not part of level 2


def test_extract_layer_copies_exactly_the_files_of_the_level(tmp_path):
    src = str(tmp_path / "src")
    sizes = _fake_folder(src, bitdepth=10)
    open(os.path.join(src, "layer_hashes.json"), "w").write("{}")        # copied as it is, not read
    for level in (0, 1, 2, 3):
        for fill in (False, True):
            dst = str(tmp_path / f"dst_{level}_{fill}")
            written = pmctf_layers.extract_layer(src, dst, level, motion_fill=fill)
            want = sorted(lr.folder_files(LAYOUT, level, fill) +
                          ["gop_structure.json", "picture_format.json", "layer_hashes.json", "layer_extract.json"])
            assert _tree(dst) == want == written, (level, fill)
            assert "picture_hashes.json" not in _tree(dst)
            for rel in (r for r in want if r != "layer_extract.json"):
                assert open(os.path.join(dst, rel), "rb").read() == open(os.path.join(src, rel), "rb").read(), rel
            marker = json.load(open(os.path.join(dst, "layer_extract.json")))
            assert marker == {"format_version": 1, "min_level": level, "motion": fill}
            assert pmctf_layers.read_layer_extract(dst) == marker
            assert pmctf_layers.layer_bytes(dst, level, fill) == sum(sizes[r] for r in lr.folder_files(LAYOUT, level, fill))
            assert pmctf_gop.sequence_layout(dst) == pmctf_gop.sequence_layout(src)
    assert pmctf_layers.read_layer_extract(src) is None
    # the old decoder on such a folder: its own missing-file error, before the codec is touched
    with pytest.raises(ValueError, match="1.bin: missing"):
        pmctf_gop.decode_gop_files(_Stages(), str(tmp_path / "dst_1_False" / "gop_00000"), 4, 100, 132, 3)


def test_extract_layer_refusals(tmp_path):
    src = str(tmp_path / "src")
    _fake_folder(src, structured=False)
    dst = str(tmp_path / "dst")
    os.makedirs(dst)
    open(os.path.join(dst, "note.txt"), "w").write("mine")
    with pytest.raises(ValueError, match="not an empty folder"):
        pmctf_layers.extract_layer(src, dst, 1)
    assert _tree(dst) == ["note.txt"]
    with pytest.raises(ValueError, match="not an empty folder"):
        pmctf_layers.extract_layer(src, os.path.join(dst, "note.txt"), 1)
    for level in (-1, 1.5, None):
        with pytest.raises(ValueError, match="level"):
            pmctf_layers.extract_layer(src, str(tmp_path / "never"), level)
    with pytest.raises(ValueError, match="motion_fill"):
        pmctf_layers.extract_layer(src, str(tmp_path / "never"), 1, motion_fill=1)
    with pytest.raises(ValueError, match="sequence.json: missing"):
        pmctf_layers.extract_layer(str(tmp_path / "nothing"), str(tmp_path / "never"), 1)
    os.remove(os.path.join(src, "gop_00001", "2.bin"))
    with pytest.raises(ValueError, match="2.bin: missing"):
        pmctf_layers.extract_layer(src, str(tmp_path / "never"), 1)
    assert not os.path.exists(str(tmp_path / "never"))
    # an empty destination that exists is taken; a sequence.json folder is copied with its header
    os.remove(os.path.join(dst, "note.txt"))
    pmctf_layers.extract_layer(src, dst, 2)
    assert _tree(dst) == sorted(lr.folder_files([(0, 4), (4, 4)], 2) + ["sequence.json", "layer_extract.json"])
    # a folder that was extracted gives its own level and above, and motion_fill only with its motion files
    with pytest.raises(ValueError, match="layer_extract.json"):
        pmctf_layers.extract_layer(dst, str(tmp_path / "never"), 1)
    with pytest.raises(ValueError, match="layer_extract.json"):
        pmctf_layers.extract_layer(dst, str(tmp_path / "never"), 2, motion_fill=True)
    for bad in ("{", "[1]", json.dumps({"format_version": 2, "min_level": 2, "motion": False}),
                json.dumps({"format_version": 1, "min_level": 2}), json.dumps({"format_version": 1, "min_level": -1, "motion": False}),
                json.dumps({"format_version": 1, "min_level": 2, "motion": 0}),
                json.dumps({"format_version": 1, "min_level": 2, "motion": False, "more": 1})):
        open(os.path.join(dst, "layer_extract.json"), "w").write(bad)
        with pytest.raises(ValueError, match="layer_extract.json"):
            pmctf_layers.read_layer_extract(dst)


def test_extract_tool(tmp_path, capsys):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("extract_temporal_layer", os.path.join(root, "tools", "extract_temporal_layer.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    src, dst = str(tmp_path / "src"), str(tmp_path / "dst")
    sizes = _fake_folder(src)
    assert tool.main([src, dst, "1", "--motion"]) == 0
    out = json.loads(capsys.readouterr().out)
    assert out["bytes"] == sum(sizes[r] for r in lr.folder_files(LAYOUT, 1, True)) and out["source_bytes"] == sum(sizes.values())
    assert out["level"] == 1 and out["motion"] is True and out["source_level"] == 0
    with pytest.raises(SystemExit) as e:
        tool.main([src, dst, "1"])
    assert "not an empty folder" in str(e.value)


# --------------------------------------------------------------------------------------------------------- the hash record
def _layer_record(level="u8", **over):
    rec = lambda t: dict({k: (7 * t + i) for i, k in enumerate(pmctf_gop.HASH_KEYS[level])}, index=t)
    record = {"format_version": 1, "level": level, "layers": {"1": [rec(t) for t in (0, 2, 4, 6)], "2": [rec(t) for t in (0, 4, 6)]}}
    record.update(over)
    return record


def test_layer_hashes_round_trip(tmp_path):
    folder = str(tmp_path / "bins")
    _fake_folder(folder)
    path = os.path.join(folder, "layer_hashes.json")
    assert path == os.path.join(folder, pmctf_layers.LAYER_HASHES)
    with pytest.raises(ValueError, match="layer_hashes.json: missing"):
        pmctf_layers.read_layer_hashes(folder)
    for level in ("u8", "f32", "u16"):
        json.dump(_layer_record(level), open(path, "w"))
        got = pmctf_layers.read_layer_hashes(folder)
        assert got == _layer_record(level)
        for k in ("1", "2"):
            assert [r["index"] for r in got["layers"][k]] == [t for _, t in lr.times(LAYOUT, int(k))]
            assert all(set(r) == set(pmctf_gop.HASH_KEYS[level]) | {"index"} for r in got["layers"][k])


def test_layer_hashes_refusals(tmp_path):
    folder = str(tmp_path / "bins")
    _fake_folder(folder)
    path = os.path.join(folder, "layer_hashes.json")

    def refused(record):
        open(path, "w").write(record if isinstance(record, str) else json.dumps(record))
        with pytest.raises(ValueError) as e:
            pmctf_layers.read_layer_hashes(folder)
        assert path in str(e.value)
        return str(e.value)

    good = _layer_record()
    layers = lambda **over: dict(good, layers=dict(good["layers"], **over))
    assert "not a layer hash file" in refused("{")
    assert "version" in refused(dict(good, format_version=2))
    assert "version" in refused({k: v for k, v in good.items() if k != "format_version"})
    assert "version" in refused("[1]")
    assert "unknown" in refused(dict(good, frames=[]))
    assert "missing" in refused({k: v for k, v in good.items() if k != "level"})
    assert "missing" in refused({k: v for k, v in good.items() if k != "layers"})
    assert "level" in refused(dict(good, level="u4"))
    assert "layers" in refused(dict(good, layers=[]))
    assert "layers" in refused(dict(good, layers={"1": good["layers"]["1"]}))                  # layer 2 is missing
    assert "layers" in refused(layers(**{"3": good["layers"]["2"]}))                           # the largest GOP has 4 pictures
    assert "layers" in refused(layers(**{"0": []}))
    # source indices that are not layer_times of the layout
    assert "source indices" in refused(layers(**{"1": good["layers"]["1"][:3]}))
    assert "source indices" in refused(layers(**{"2": good["layers"]["1"]}))
    assert "source indices" in refused(layers(**{"1": [dict(r, index=r["index"] + 1) for r in good["layers"]["1"]]}))
    assert "source indices" in refused(layers(**{"2": list(reversed(good["layers"]["2"]))}))
    # the records themselves
    first = good["layers"]["1"][0]
    rest = good["layers"]["1"][1:]
    assert "hold exactly" in refused(layers(**{"1": [{k: v for k, v in first.items() if k != "cb"}] + rest}))
    assert "hold exactly" in refused(layers(**{"1": [dict(first, y_f32=1)] + rest}))
    assert "hold exactly" in refused(layers(**{"1": [{k: v for k, v in first.items() if k != "index"}] + rest}))
    assert "hold exactly" in refused(layers(**{"1": [list(first)] + rest}))
    assert "hold exactly" in refused(layers(**{"1": "0246"}))
    for v in (-1, 2 ** 32, 1.0, "1", None, True):
        assert "32-bit" in refused(layers(**{"1": [dict(first, frame=v)] + rest}))
    # the level's keys: a u8 record under f32 lacks the float hashes
    assert "hold exactly" in refused(dict(good, level="f32"))
    # a folder without a readable header
    os.remove(os.path.join(folder, "gop_structure.json"))
    with pytest.raises(ValueError, match="sequence.json: missing"):
        pmctf_layers.read_layer_hashes(folder)


# ------------------------------------------------------------------------------------------------------------ the decoders
def test_decoder_refusals_come_before_the_codec_is_touched(tmp_path):
    folder = str(tmp_path / "bins")
    _fake_folder(folder)
    sub = os.path.join(folder, "gop_00000")
    yuv = str(tmp_path / "out.yuv")
    for level in (-1, -7, 1.0, "2", None, True):
        with pytest.raises(ValueError, match="level"):
            pmctf_layers.decode_gop_files_layer(_NoDevice(), sub, 4, 100, 132, 3, level)
        with pytest.raises(ValueError, match="level"):
            pmctf_layers.decode_sequence_layer(_NoDevice(), folder, yuv, level)
    with pytest.raises(ValueError, match="never verified"):
        pmctf_layers.decode_sequence_layer(_NoDevice(), folder, yuv, 1, verify=True, motion_fill=True)
    with pytest.raises(ValueError, match="verify"):
        pmctf_layers.decode_sequence_layer(_NoDevice(), folder, yuv, 1, verify="yes")
    with pytest.raises(ValueError, match="motion_fill"):
        pmctf_layers.decode_sequence_layer(_NoDevice(), folder, yuv, 1, motion_fill="yes")
    with pytest.raises(ValueError, match="nothing to write"):
        pmctf_layers.decode_sequence_layer(_NoDevice(), folder, None, 1)
    with pytest.raises(ValueError, match="ll_order"):
        pmctf_layers.decode_gop_files_layer(_NoDevice(), sub, 4, 100, 132, 3, 1, ll_order="raster")
    with pytest.raises(ValueError, match="power of two"):
        pmctf_layers.decode_gop_files_layer(_NoDevice(), sub, 6, 100, 132, 3, 1)
    # what an extracted folder cannot give, naming its marker file
    dst = str(tmp_path / "level2")
    pmctf_layers.extract_layer(folder, dst, 2)
    for level in (0, 1):
        with pytest.raises(ValueError, match="layer_extract.json.*level 2 and above"):
            pmctf_layers.decode_sequence_layer(_NoDevice(), dst, yuv, level)
    with pytest.raises(ValueError, match="layer_extract.json.*motion"):
        pmctf_layers.decode_sequence_layer(_NoDevice(), dst, yuv, 2, motion_fill=True)
    with pytest.raises(ValueError, match="layer_extract.json"):
        pmctf_layers.write_layer_hashes(_NoDevice(), dst)
    # png_out above 8 bits, as decode_sequence refuses it
    hbd = str(tmp_path / "hbd")
    _fake_folder(hbd, bitdepth=10, picture_hashes=False)
    with pytest.raises(ValueError, match="picture_format.json"):
        pmctf_layers.decode_sequence_layer(_NoDevice(), hbd, yuv, 1, png_out=str(tmp_path / "png"))
    with pytest.raises(ValueError, match="does not go with bitdepth 10"):
        pmctf_layers.write_layer_hashes(_NoDevice(), hbd, hash_level="u8")
    assert not os.path.exists(yuv) and not os.path.exists(str(tmp_path / "png"))
    # a missing file of the set is named before anything is decoded
    os.remove(os.path.join(sub, "2.bin"))
    with pytest.raises(ValueError, match="2.bin: missing"):
        pmctf_layers.decode_gop_files_layer(_Stages(), sub, 4, 100, 132, 3, 1)


def test_public_signatures():
    p = inspect.signature(pmctf_layers.decode_gop_files_layer).parameters
    assert list(p) == ["codec", "bin_folder", "gop", "pic_height", "pic_width", "q_index", "level", "psize", "me_downsample",
                       "ll_order", "motion_fill"]
    assert (p["psize"].default, p["me_downsample"].default, p["ll_order"].default, p["motion_fill"].default) == \
        (128, 1, "plane", False)
    p = inspect.signature(pmctf_layers.decode_sequence_layer).parameters
    assert list(p) == ["codec", "bin_folder", "yuv_out", "level", "device", "png_out", "verify", "motion_fill"]
    assert (p["device"].default, p["png_out"].default, p["verify"].default, p["motion_fill"].default) == \
        (None, None, "auto", False)
    assert list(inspect.signature(pmctf_layers.layer_times).parameters) == ["gops", "level"]
    for fn, names in ((pmctf_layers.layer_file_names, ["gop", "level", "motion_fill"]),
                      (pmctf_layers.layer_bytes, ["bin_folder", "level", "motion_fill"]),
                      (pmctf_layers.extract_layer, ["src_folder", "dst_folder", "level", "motion_fill"])):
        q = inspect.signature(fn).parameters
        assert list(q) == names and q["motion_fill"].default is False
    q = inspect.signature(pmctf_layers.write_layer_hashes).parameters
    assert list(q) == ["codec", "bin_folder", "hash_level"] and q["hash_level"].default is None
    assert list(inspect.signature(pmctf_layers.read_layer_hashes).parameters) == ["bin_folder"]
