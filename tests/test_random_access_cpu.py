"""Random access, the parts that need no GPU: the plan of pmctf_access against the dependency closure restated in
tests/access_restatement.py, the worked example, the counts, check_frames, access_plan, access_bytes on a folder of dummies,
the tool's argument errors (raised before any weights are loaded) and the parameter lists.  Everything is exact."""
import ast
import importlib.util
import inspect
import itertools
import os

import pytest

import access_restatement as ar
import layers_restatement as lr
import pmctf_access
import pmctf_gop
import pmctf_layers
import pmctf_seq

SIZES = (1, 2, 4, 8, 16)
GOPS = [{"first": 0, "size": 4, "me_downsample": 1, "psize": 128}, {"first": 4, "size": 2, "me_downsample": 1, "psize": 128},
        {"first": 6, "size": 1, "me_downsample": 1, "psize": 128}]
LAYOUT = [(0, 4), (4, 2), (6, 1)]


def _names(size):
    return pmctf_gop.gop_file_names(size) if size != 1 else ["0_main.bin", "0_C_main.bin"]


def _in_order(files, size):
    names = _names(size)
    return [names.index(n) for n in files] == sorted(names.index(n) for n in files) and len(set(files)) == len(files)


# --------------------------------------------------------------------------------------------------------------- the plan
def test_files_are_the_restated_closure():
    for size in SIZES:
        assert ar.all_files(size) == _names(size)
        for n in range(size):
            files = pmctf_access.access_file_names(size, [n])
            assert files == ar.closure(size, [n]), (size, n)
            assert _in_order(files, size), (size, n)
    for k in range(1, 9):
        for wanted in itertools.combinations(range(8), k):
            files = pmctf_access.access_file_names(8, list(wanted))
            assert files == ar.closure(8, wanted), wanted
            assert _in_order(files, 8), wanted
    assert sum(1 for k in range(1, 9) for _ in itertools.combinations(range(8), k)) == 255


def test_worked_example():
    plan = pmctf_access.gop_plan(8, [5])
    assert plan["needed"] == {0: [5], 1: [4], 2: [4], 3: [0]}
    assert plan["pairs"] == [(2, 0, 4, True), (1, 4, 6, False), (0, 4, 5, True)]
    assert plan["files"] == ["1_mv.bin", "3_mv.bin", "5.bin", "5_C_main.bin", "5_mv.bin", "2_mv.bin", "6.bin", "6_C_main.bin",
                             "6_mv.bin", "4.bin", "4_C_main.bin", "4_mv.bin", "0_main.bin", "0_C_main.bin"]
    assert len(plan["files"]) == 14 and len(pmctf_gop.gop_file_names(8)) == 23
    assert len(plan["picture_files"]) == 8 and sum(not n.endswith("_mv.bin") for n in pmctf_gop.gop_file_names(8)) == 16
    assert plan["picture_files"] == ["4.bin", "4_C_main.bin", "6.bin", "6_C_main.bin", "5.bin", "5_C_main.bin", "0_main.bin",
                                     "0_C_main.bin"]
    assert plan["motion_files"] == ["1_mv.bin", "3_mv.bin", "5_mv.bin", "2_mv.bin", "6_mv.bin", "4_mv.bin"]
    assert "needed = {0: [5], 1: [4], 2: [4], 3: [0]}" in pmctf_access.__doc__
    assert "pairs = [(2, 0, 4, True), (1, 4, 6, False), (0, 4, 5, True)]" in pmctf_access.__doc__
    lone = pmctf_access.gop_plan(1, [0])
    assert lone == {"needed": {0: [0]}, "pairs": [], "picture_files": ["0_main.bin", "0_C_main.bin"], "motion_files": [],
                    "files": ["0_main.bin", "0_C_main.bin"]}


def test_counts_of_a_gop_of_16():
    for n in range(16):
        plan = pmctf_access.gop_plan(16, [n])
        assert len(plan["picture_files"]) == 10 and len(plan["pairs"]) == 4, n
        assert len(plan["motion_files"]) == sum((n >> (s + 1)) + 1 for s in range(4)), n
        assert sorted(plan["files"]) == sorted(plan["picture_files"] + plan["motion_files"])
        assert plan["needed"][4] == [0] and plan["needed"][0] == [n]
        # a pair computes `cur` exactly where the picture's bit of that stage is set
        assert [(s, want) for s, _, _, want in plan["pairs"]] == [(s, bool(n >> s & 1)) for s in (3, 2, 1, 0)]
    assert len(pmctf_access.gop_plan(16, [0])["motion_files"]) == 4
    assert len(pmctf_access.gop_plan(16, [15])["motion_files"]) == 15


def test_whole_gop_monotony_and_motion_prefix():
    for size in SIZES:
        plan = pmctf_access.gop_plan(size, list(range(size)))
        assert plan["files"] == _names(size)
        assert all(want for _, _, _, want in plan["pairs"])
        assert [(s, r, c) for s, r, c, _ in plan["pairs"]] == \
            ([p for s in reversed(range(size.bit_length() - 1)) for p in reversed([q for q in pmctf_gop.gop_pairs(size) if q[0] == s])]
             if size > 1 else [])
    subsets = [list(w) for k in range(1, 9) for w in itertools.combinations(range(8), k)]
    files = {tuple(w): set(pmctf_access.access_file_names(8, w)) for w in subsets}
    for a in subsets:
        for b in subsets:
            if set(a) <= set(b):
                assert files[tuple(a)] <= files[tuple(b)], (a, b)
    for size in SIZES[1:]:
        for n in range(size):
            motion = pmctf_access.gop_plan(size, [n])["motion_files"]
            for s in range(size.bit_length() - 1):
                coded = [f"{c}_mv.bin" for stage, _, c in pmctf_gop.gop_pairs(size) if stage == s]
                mine = [m for m in motion if m in coded]
                assert mine and mine == coded[:len(mine)], (size, n, s)
            assert motion == [m for m in pmctf_gop.gop_file_names(size) if m in motion], "coding order"


def test_gop_plan_refusals():
    for size in (0, 3, 6, -4, 2.0, "8"):
        with pytest.raises(ValueError, match="power of two"):
            pmctf_access.gop_plan(size, [0])
    for wanted in ([], [8], [-1], [3, 2], [2, 2], [1.0], [True]):
        with pytest.raises(ValueError, match="wanted"):
            pmctf_access.gop_plan(8, wanted)


# ----------------------------------------------------------------------------------------------------------- check_frames
def test_check_frames():
    assert pmctf_access.check_frames(range(2, 6), 7) == [2, 3, 4, 5]
    assert pmctf_access.check_frames([5, 0, 3], 7) == [0, 3, 5]
    assert pmctf_access.check_frames((2, 6), 7) == [2, 3, 4, 5]
    assert pmctf_access.check_frames(iter([6]), 7) == [6]
    assert pmctf_access.check_frames(range(7), 7) == list(range(7))
    for frames, text in (([], r"\[\] selects no picture"), (range(3, 3), r"range\(3, 3\) selects no picture"),
                         ((4, 2), r"\(4, 2\) selects no picture"), ([1, 2.0], "2.0 is not an integer"),
                         ([True], "True is not an integer"), (["3"], "'3' is not an integer"), ((1, 2.5), "2.5 is not an integer"),
                         ([0, 7], "7 is outside 0..6"), ([-1], "-1 is outside 0..6"), ((5, 9), "7 is outside 0..6"),
                         ([3, 1, 3], "3 is given twice"), (5, "5 is not a range")):
        with pytest.raises(ValueError, match=text):
            pmctf_access.check_frames(frames, 7)


# ------------------------------------------------------------------------------------------------------------ access_plan
def test_access_plan():
    gops = [(0, 4, 128, 1), (4, 2, 128, 1), (6, 1, 128, 1)]
    assert pmctf_access.access_plan(gops, list(range(7))) == [(0, [0, 1, 2, 3]), (1, [0, 1]), (2, [0])]
    assert pmctf_access.access_plan(gops, [2, 3, 4, 5]) == [(0, [2, 3]), (1, [0, 1])]
    assert pmctf_access.access_plan(gops, [1, 6]) == [(0, [1]), (2, [0])]             # skips the GOP of 2
    assert pmctf_access.access_plan(gops, [5]) == [(1, [1])]
    eights = [(0, 8, 128, 1), (8, 8, 128, 1), (16, 8, 128, 1)]
    assert pmctf_access.access_plan(eights, [7, 8]) == [(0, [7]), (1, [0])]
    assert pmctf_access.access_plan(eights, [0, 23]) == [(0, [0]), (2, [7])]
    assert pmctf_access.access_plan(eights, [9, 10, 15]) == [(1, [1, 2, 7])]
    assert pmctf_access.access_plan(eights, list(range(24))) == [(k, list(range(8))) for k in range(3)]


# ------------------------------------------------------------------------------------------------------ a folder of dummies
def _fake_folder(path):
    """a real header over dummy bitstream files, each of a size of its own"""
    os.makedirs(path)
    pmctf_seq.write_gop_structure(path, width=136, height=104, frame_num=7, max_gop=4, q_index=3, num_me_stages=1,
                                  ll_order="plane", precision="f32", aten_threads=1, gops=GOPS)
    for i, rel in enumerate(lr.folder_files(LAYOUT, 0)):
        os.makedirs(os.path.dirname(os.path.join(path, rel)), exist_ok=True)
        open(os.path.join(path, rel), "wb").write(b"x" * (1 << i))
    return path


def test_access_bytes(tmp_path):
    folder = _fake_folder(str(tmp_path / "bins"))
    size = lambda k, names: sum(os.path.getsize(os.path.join(folder, pmctf_gop.gop_folder(k), n)) for n in names)
    assert pmctf_access.access_bytes(folder, range(7)) == pmctf_layers.layer_bytes(folder, 0)
    # pictures 2 and 3 hang on the pair (2, 3) of stage 0, whose motion follows that of the pair (0, 1): all but 1's pictures
    late = ["1_mv.bin", "3.bin", "3_C_main.bin", "3_mv.bin", "2.bin", "2_C_main.bin", "2_mv.bin", "0_main.bin", "0_C_main.bin"]
    assert pmctf_access.access_bytes(folder, [2]) == pmctf_access.access_bytes(folder, [3]) == size(0, late)
    assert pmctf_access.access_bytes(folder, [0]) == size(0, ["1.bin", "1_C_main.bin", "1_mv.bin", "2.bin", "2_C_main.bin",
                                                              "2_mv.bin", "0_main.bin", "0_C_main.bin"])
    assert pmctf_access.access_bytes(folder, (1, 7)) == size(0, ar.closure(4, [1, 2, 3])) + size(1, ar.closure(2, [0, 1])) + \
        size(2, ["0_main.bin", "0_C_main.bin"])
    assert pmctf_access.access_bytes(folder, [0, 6]) == size(0, ar.closure(4, [0])) + size(2, ar.closure(1, [0]))
    os.remove(os.path.join(folder, "gop_00001", "1_mv.bin"))
    assert pmctf_access.access_bytes(folder, [0, 6]) == size(0, ar.closure(4, [0])) + size(2, ar.closure(1, [0]))
    with pytest.raises(ValueError, match="gop_00001.1_mv.bin: missing"):
        pmctf_access.access_bytes(folder, [4])
    with pytest.raises(ValueError, match="7 is outside 0..6"):
        pmctf_access.access_bytes(folder, [7])


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the codec was touched ({name}) before the arguments were checked")


def test_decoder_refusals_come_before_the_codec(tmp_path):
    folder = _fake_folder(str(tmp_path / "bins"))
    yuv = str(tmp_path / "never.yuv")
    for frames, text in (([7], "7 is outside 0..6"), ([], "selects no picture"), ([1, 1], "1 is given twice")):
        with pytest.raises(ValueError, match=text):
            pmctf_access.decode_frames(_NoDevice(), folder, yuv, frames)
        with pytest.raises(ValueError, match=text):
            pmctf_access.read_frames(_NoDevice(), folder, frames)
    with pytest.raises(ValueError, match=r"136x104 offer the spatial levels 0\.\.2"):
        pmctf_access.decode_frames(_NoDevice(), folder, yuv, [1], spatial_level=3)
    with pytest.raises(ValueError, match="spatial_hashes.json: missing"):
        pmctf_access.decode_frames(_NoDevice(), folder, yuv, [1], verify=True, spatial_level=1)
    with pytest.raises(ValueError, match="nothing to write"):
        pmctf_access.decode_frames(_NoDevice(), folder, None, [1])
    small = str(tmp_path / "small")
    pmctf_layers.extract_layer(folder, small, 1)
    with pytest.raises(ValueError, match="layer_extract.json"):
        pmctf_access.decode_frames(_NoDevice(), small, yuv, [0])
    assert not os.path.exists(yuv)


# ---------------------------------------------------------------------------------------------------------------- the tool
def _decode_tool():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("decode_sequence", os.path.join(root, "tools", "decode_sequence.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_tool_parses_and_refuses_before_the_weights_are_loaded(tmp_path, capsys):
    tool = _decode_tool()
    assert tool.parse_frames("37") == [37] and tool.parse_frames("2:6") == [2, 3, 4, 5]
    assert tool.parse_frames("0,8:12,40") == [0, 8, 9, 10, 11, 40]
    for spec in ("", "a", "1:2:3", "3:", ":3", "-1", "1,,2", "4:4", "5:2", "1.5"):
        with pytest.raises(ValueError):
            tool.parse_frames(spec)
    folder = _fake_folder(str(tmp_path / "bins"))
    small = str(tmp_path / "small")
    pmctf_layers.extract_layer(folder, small, 1)
    yuv = str(tmp_path / "never.yuv")
    base = ["--synth-seed", "0", "--device", "no-such-device"]
    for argv, text in ((["--frames", "2", "--temporal-level", "1", folder, yuv], "--frames: cannot be combined with --temporal-level"),
                       (["--frames", "2", "--temporal-level", "0", folder, yuv], "--frames: cannot be combined with --temporal-level"),
                       (["--frames", "2", "--motion-fill", folder, yuv], "--frames: cannot be combined with --motion-fill"),
                       (["--frames", "2", "--compare", os.path.join(folder, "gop_structure.json"), folder, yuv], "--frames: cannot be combined with --compare"),
                       (["--frames", "2:x", folder, yuv], "--frames: '2:x' is neither N nor A:B"),
                       (["--frames", "1,,2", folder, yuv], "--frames: '' is neither N nor A:B"),
                       (["--frames", "4:4", folder, yuv], "--frames: '4:4' selects no picture"),
                       (["--frames", "5:8", folder, yuv], "--frames: frames: 7 is outside 0..6"),
                       (["--frames", "1,0:2", folder, yuv], "--frames: frames: 1 is given twice"),
                       (["--frames", "1", "--spatial-level", "3", folder, yuv], "136x104 offer the spatial levels 0..2"),
                       (["--frames", "1", "--spatial-level", "1", "--verify", folder, yuv], "spatial_hashes.json: missing"),
                       (["--frames", "1", small, yuv], "layer_extract.json")):
        with pytest.raises(SystemExit) as e:
            tool.main(base + argv)
        assert e.value.code == 2 and text in capsys.readouterr().err, argv
    assert not os.path.exists(yuv)


# ---------------------------------------------------------------------------------------------------------- parameter lists
def test_parameter_lists():
    def params(fn):
        return [(p.name, p.default, p.kind == p.KEYWORD_ONLY) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert params(pmctf_access.check_frames) == [("frames", E, False), ("frame_num", E, False)]
    assert params(pmctf_access.gop_plan) == [("size", E, False), ("wanted", E, False)]
    assert params(pmctf_access.access_plan) == [("gops", E, False), ("frames", E, False)]
    assert params(pmctf_access.access_file_names) == [("size", E, False), ("wanted", E, False)]
    assert params(pmctf_access.access_bytes) == [("bin_folder", E, False), ("frames", E, False)]
    assert params(pmctf_access.decode_gop_files_frames) == \
        [(n, E, False) for n in ("codec", "bin_folder", "gop", "pic_height", "pic_width", "q_index", "wanted")] + \
        [("psize", 128, False), ("me_downsample", 1, False), ("ll_order", "plane", False), ("spatial_level", 0, False),
         ("one_sided", True, False)]
    assert params(pmctf_access.decode_frames) == \
        [("codec", E, False), ("bin_folder", E, False), ("yuv_out", E, False), ("frames", E, False), ("device", None, False),
         ("png_out", None, False), ("verify", "auto", False), ("spatial_level", 0, True), ("coded_size_output", False, True),
         ("coded_format_output", False, True), ("output_layout", None, True)]
    assert params(pmctf_access.read_frames) == [("codec", E, False), ("bin_folder", E, False), ("frames", E, False),
                                                ("device", None, False), ("verify", "auto", False)]
    assert issubclass(pmctf_access.FrameDecode, pmctf_gop.FullDecode)
    # what was there keeps its parameters
    assert params(pmctf_gop.decode_sequence_with) == \
        [("mode", E, False), ("codec", E, False), ("bin_folder", E, False), ("yuv_out", E, False), ("device", None, False),
         ("png_out", None, False), ("verify", "auto", False), ("coded_size_output", False, True),
         ("coded_format_output", False, True), ("output_layout", None, True)]
    from pMCTF.hip.engine import HipEngine
    from pMCTF.models.video.pMCTF_L import pMCTF
    lifting = [("self", E, False), ("L_t", E, False), ("H_t", E, False), ("mv_hat", E, False), ("downscale", False, False),
               ("stage_idx", 0, False)]
    for fn in (HipEngine.inverse_MCTF, HipEngine.inverse_MCTF_ref, pMCTF.inverse_MCTF, pMCTF.inverse_MCTF_ref):
        assert params(fn) == lifting, fn
    assert params(pmctf_layers.decode_gop_files_layer) == \
        [(n, E, False) for n in ("codec", "bin_folder", "gop", "pic_height", "pic_width", "q_index", "level")] + \
        [("psize", 128, False), ("me_downsample", 1, False), ("ll_order", "plane", False), ("motion_fill", False, False)]


def test_module_imports_no_torch_itself():
    tree = ast.parse(open(pmctf_access.__file__).read())
    top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
    names = {a.name for n in top if isinstance(n, ast.Import) for a in n.names} | \
            {n.module for n in top if isinstance(n, ast.ImportFrom)}
    assert names == {"os", "pmctf_gop", "pmctf_layers", "pmctf_spatial", "pmctf_records"}
