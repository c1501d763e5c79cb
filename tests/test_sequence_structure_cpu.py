"""Sequences as lists of GOPs, the parts that need no GPU: plan_gops exhaustively, scene_cuts on the restatement's figures
of a sequence with one scene change, the gop_structure.json header (round trip and every refusal), the public signatures,
and the entry point of csrc/scene_ops.hip (declared, bound, exported, refusing bad arguments before anything is enqueued).
Everything is exact; the yardstick is tests/structure_restatement.py."""
import ctypes as C
import inspect
import json
import os
import random
import re

import pytest

import pmctf_gop
import pmctf_seq
import structure_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "pmctf_luma_activity_f32"


# ---------------------------------------------------------------------------------------------------------- plan_gops
def _check_plan(plan, frame_num, max_gop, cuts):
    at = 0
    bounds = sorted(set(cuts)) + [frame_num]
    for first, size in plan:
        assert first == at, "contiguous"
        assert size >= 1 and size & (size - 1) == 0 and size <= max_gop
        assert not any(first < c < first + size for c in cuts), "no cut inside a GOP"
        left = min(b for b in bounds if b > first) - first         # what is left of the segment
        assert size <= left and (size == max_gop or 2 * size > left), "the largest power of two that fits"
        at += size
    assert at == frame_num


def test_plan_gops_exhaustively():
    rng = random.Random(5)
    for max_gop in (2, 4, 8, 16):
        for n in range(1, 71):
            plan = pmctf_seq.plan_gops(n, max_gop)
            _check_plan(plan, n, max_gop, [])
            if n % max_gop == 0:
                assert plan == [(k * max_gop, max_gop) for k in range(n // max_gop)]
            for _ in range(4):
                if n < 2:
                    break
                cuts = rng.sample(range(1, n), rng.randint(1, min(5, n - 1)))
                plan = pmctf_seq.plan_gops(n, max_gop, cuts)
                _check_plan(plan, n, max_gop, cuts)
                assert all(any(first == c for first, _ in plan) for c in cuts), "every cut starts a GOP"


def test_plan_gops_example_and_refusals():
    assert [s for _, s in pmctf_seq.plan_gops(21, 8, [5])] == [4, 1, 8, 8]
    assert pmctf_seq.plan_gops(21, 8, (5,)) == [(0, 4), (4, 1), (5, 8), (13, 8)]
    assert [s for _, s in pmctf_seq.plan_gops(7, 4)] == [4, 2, 1]
    assert pmctf_seq.plan_gops(1, 2) == [(0, 1)]
    assert pmctf_seq.plan_gops(9, 8, [3, 3]) == pmctf_seq.plan_gops(9, 8, [3])
    for n, g, cuts in ((0, 8, ()), (-1, 8, ()), (8.0, 8, ()), (8, 1, ()), (8, 6, ()), (8, 0, ()), (8, 8.0, ()), (8, True, ()),
                       (8, 8, (0,)), (8, 8, (8,)), (8, 8, (2.5,)), (8, 8, (-1,))):
        with pytest.raises(ValueError):
            pmctf_seq.plan_gops(n, g, cuts)


# --------------------------------------------------------------------------------------------------------- scene_cuts
def test_scene_cuts_on_the_restatement_of_a_scene_change():
    f = sr.cut_figures()
    assert len(f["hd"]) == 12 and f["hd"][0] is None and f["mad"][0] is None and f["sad"][0] is None
    assert all(isinstance(v, int) for v in f["sad"][1:] + f["hist_l1"][1:])
    assert pmctf_seq.scene_cuts(f["mad"], f["hd"], hd_min=0.3, mad_min=5) == [sr.CUT_AT]
    # the thresholds sit far from both sides (figures computed once with this restatement: hd 0.635 at the cut and at
    # most 0.077 elsewhere, mad 58.0 and at most 14.9)
    others = [t for t in range(1, 12) if t != sr.CUT_AT]
    assert f["hd"][sr.CUT_AT] > 0.6 and max(f["hd"][t] for t in others) < 0.1
    assert f["mad"][sr.CUT_AT] > 50 and max(f["mad"][t] for t in others) < 20
    # either threshold alone decides differently: both are needed
    assert pmctf_seq.scene_cuts(f["mad"], f["hd"], hd_min=0.0, mad_min=5) != [sr.CUT_AT]
    assert pmctf_seq.scene_cuts(f["mad"], f["hd"], hd_min=0.3, mad_min=100) == []
    assert pmctf_seq.scene_cuts([None, 9.0, 1.0, 9.0], [None, 0.5, 0.5, 0.1], 0.3, 5) == [1]
    with pytest.raises(ValueError):
        pmctf_seq.scene_cuts([None, 1.0], [None], 0.3, 5)
    assert 0.25 <= pmctf_seq.HD_MIN <= 0.5 and pmctf_seq.MAD_MIN > 0


# -------------------------------------------------------------------------------------------------------------- header
def _fields(**over):
    gops = [{"first": 0, "size": 4, "me_downsample": 1, "psize": 128}, {"first": 4, "size": 2, "me_downsample": 4, "psize": 256},
            {"first": 6, "size": 1, "me_downsample": 1, "psize": 128}]
    f = dict(width=132, height=100, frame_num=7, max_gop=4, q_index=3, num_me_stages=1, ll_order="plane", precision="f32",
             aten_threads=1, gops=gops)
    f.update(over)
    return f


def test_gop_structure_round_trip(tmp_path):
    folder = str(tmp_path)
    path = pmctf_seq.write_gop_structure(folder, **_fields())
    assert path == os.path.join(folder, "gop_structure.json") == os.path.join(folder, pmctf_gop.GOP_STRUCTURE)
    want = dict(_fields(), format_version=1)
    assert json.load(open(path)) == want and pmctf_seq.read_gop_structure(folder) == want
    header, layout = pmctf_gop.sequence_layout(folder)
    assert header == want and layout == [(0, 4, 128, 1), (4, 2, 256, 4), (6, 1, 128, 1)]
    # an older decoder refuses the folder cleanly
    with pytest.raises(ValueError, match="sequence.json: missing"):
        pmctf_gop.read_sequence_header(folder)
    # a sequence.json folder is laid out as before
    old = str(tmp_path / "old")
    os.makedirs(old)
    pmctf_gop.write_sequence_header(old, width=132, height=100, frame_num=8, gop=4, q_index=3, psize=128, me_downsample=1,
                                    num_me_stages=1, ll_order="plane", precision="f32", aten_threads=1)
    assert pmctf_gop.sequence_layout(old)[1] == [(0, 4, 128, 1), (4, 4, 128, 1)]
    with pytest.raises(ValueError, match="gop_structure.json: missing"):
        pmctf_seq.read_gop_structure(old)


def test_gop_structure_refusals(tmp_path):
    folder = str(tmp_path)
    path = os.path.join(folder, "gop_structure.json")

    def refused(record):
        open(path, "w").write(record if isinstance(record, str) else json.dumps(record))
        with pytest.raises(ValueError) as e:
            pmctf_seq.read_gop_structure(folder)
        assert path in str(e.value)
        with pytest.raises(ValueError):
            pmctf_gop.sequence_layout(folder)
        return str(e.value)

    good = dict(_fields(), format_version=1)
    gops = lambda *triples: [{"first": f, "size": s, "me_downsample": d, "psize": p} for f, s, d, p in triples]
    assert "not a GOP structure file" in refused("{")
    assert "version" in refused(dict(good, format_version=2))
    assert "version" in refused({k: v for k, v in good.items() if k != "format_version"})
    assert "version" in refused("[1]")
    assert "unknown" in refused(dict(good, gop=4))
    for k in pmctf_seq.STRUCTURE_FIELDS:
        assert "missing" in refused({x: v for x, v in good.items() if x != k}), k
    assert "power of two" in refused(dict(good, gops=gops((0, 3, 1, 128), (3, 4, 1, 128))))
    assert "power of two" in refused(dict(good, frame_num=8, gops=gops((0, 8, 1, 128))))           # above max_gop 4
    assert "power of two" in refused(dict(good, gops=gops((0, 0, 1, 128), (0, 4, 1, 128))))
    assert "first" in refused(dict(good, gops=gops((0, 4, 1, 128), (5, 2, 1, 128), (7, 1, 1, 128))))
    assert "first" in refused(dict(good, gops=gops((1, 4, 1, 128), (5, 2, 1, 128))))
    assert "cover" in refused(dict(good, gops=gops((0, 4, 1, 128), (4, 2, 1, 128))))
    assert "cover" in refused(dict(good, gops=gops((0, 4, 1, 128), (4, 4, 1, 128))))
    assert "me_downsample" in refused(dict(good, gops=gops((0, 4, 3, 128), (4, 2, 1, 128), (6, 1, 1, 128))))
    assert "me_downsample" in refused(dict(good, gops=gops((0, 4, 16, 512), (4, 2, 1, 128), (6, 1, 1, 128))))
    # ca_psize(8) is 512 and ca_psize(1) 128: 64 may be the sequence's own, 64 and 32 cannot both be
    own = dict(good, gops=gops((0, 4, 8, 512), (4, 2, 1, 64), (6, 1, 2, 64)))
    open(path, "w").write(json.dumps(own))
    assert pmctf_seq.read_gop_structure(folder) == own
    assert "psize" in refused(dict(good, gops=gops((0, 4, 1, 64), (4, 2, 1, 32), (6, 1, 1, 128))))
    assert "psize" in refused(dict(good, gops=gops((0, 4, 1, 127), (4, 2, 1, 128), (6, 1, 1, 128))))
    assert "holds exactly" in refused(dict(good, gops=[{"first": 0, "size": 4, "me_downsample": 1}]))
    assert "holds exactly" in refused(dict(good, gops=gops((0, 4, 1, 128))[:1] + [[4, 2, 1, 128]]))
    assert "integer" in refused(dict(good, gops=gops((0, 4.0, 1, 128), (4, 2, 1, 128), (6, 1, 1, 128))))
    assert "non-empty list" in refused(dict(good, gops=[]))
    assert "max_gop" in refused(dict(good, max_gop=6))
    assert "ll_order" in refused(dict(good, ll_order="raster"))
    assert "integer" in refused(dict(good, width="132"))
    # both headers in one folder
    open(path, "w").write(json.dumps(good))
    assert pmctf_seq.read_gop_structure(folder) == good
    pmctf_gop.write_sequence_header(folder, width=132, height=100, frame_num=8, gop=4, q_index=3, psize=128, me_downsample=1,
                                    num_me_stages=1, ll_order="plane", precision="f32", aten_threads=1)
    with pytest.raises(ValueError, match="sequence.json"):
        pmctf_seq.read_gop_structure(folder)
    with pytest.raises(ValueError, match="one header"):
        pmctf_gop.sequence_layout(folder)
    with pytest.raises(ValueError, match="one header"):
        pmctf_gop.decode_sequence(None, folder, str(tmp_path / "out.yuv"))
    with pytest.raises(ValueError, match="one header"):
        pmctf_gop.check_yuv_hashes(folder, str(tmp_path / "out.yuv"))
    # the writer refuses what the reader would
    os.remove(path)
    for bad in (dict(frame_num=8), dict(max_gop=2), dict(ll_order="raster")):
        with pytest.raises(ValueError):
            pmctf_seq.write_gop_structure(folder, **_fields(**bad))
    with pytest.raises(ValueError):
        pmctf_seq.write_gop_structure(folder, **{k: v for k, v in _fields().items() if k != "q_index"})
    with pytest.raises(ValueError):
        pmctf_seq.write_gop_structure(folder, psize=128, **_fields())
    assert not os.path.exists(path)


def test_check_tool_reads_a_structured_folder(tmp_path, capsys):
    """tools/check_picture_hashes.py on a folder with gop_structure.json: zlib alone, no GPU"""
    import importlib.util
    import zlib
    import numpy as np
    w, h, n = 6, 10, 3
    ny, nc = w * h, (w // 2) * (h // 2)
    data = np.random.default_rng(1).integers(0, 256, n * (ny + 2 * nc), dtype=np.uint8).tobytes()
    folder = str(tmp_path / "bins")
    os.makedirs(folder)
    pmctf_seq.write_gop_structure(folder, **_fields(width=w, height=h, frame_num=n, max_gop=2, gops=[
        {"first": 0, "size": 2, "me_downsample": 1, "psize": 128}, {"first": 2, "size": 1, "me_downsample": 1, "psize": 128}]))
    recs = []
    for i in range(n):
        f = data[i * (ny + 2 * nc):(i + 1) * (ny + 2 * nc)]
        recs.append({"y": zlib.crc32(f[:ny]), "cb": zlib.crc32(f[ny:ny + nc]), "cr": zlib.crc32(f[ny + nc:]),
                     "frame": zlib.crc32(f)})
    pmctf_gop.write_picture_hashes(folder, "u8", recs)
    yuv = str(tmp_path / "dec.yuv")
    open(yuv, "wb").write(data)
    spec = importlib.util.spec_from_file_location("check_picture_hashes", os.path.join(ROOT, "tools", "check_picture_hashes.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.main([folder, yuv]) == 0
    assert f"all {n} frames match" in capsys.readouterr().out
    bad = bytearray(data)
    bad[2 * (ny + 2 * nc) + 3] ^= 0x10                                # the lone picture's luma
    open(yuv, "wb").write(bytes(bad))
    assert tool.main([folder, yuv]) == 1
    assert "frame 2, plane y" in capsys.readouterr().out


# ---------------------------------------------------------------------------------------------------------- signatures
def test_public_signatures():
    p = inspect.signature(pmctf_seq.encode_sequence_gops).parameters
    assert list(p) == ["codec", "source", "width", "height", "frame_num", "max_gop", "q_index", "bin_folder", "device",
                       "structure", "hd_min", "mad_min", "ds_factors", "skip_decoding", "psize", "src_format", "ingest",
                       "decoded_frame_path", "picture_hash", "bitdepth", "msssim"]
    assert p["structure"].default == "fill" and p["ds_factors"].default == (1, 2, 4, 8)
    assert p["hd_min"].default == pmctf_seq.HD_MIN and p["mad_min"].default == pmctf_seq.MAD_MIN
    old = inspect.signature(pmctf_gop.encode_sequence).parameters
    for k in ("skip_decoding", "psize", "src_format", "ingest", "decoded_frame_path", "picture_hash", "bitdepth", "msssim"):
        assert p[k].default == old[k].default, k
    assert list(inspect.signature(pmctf_seq.plan_gops).parameters) == ["frame_num", "max_gop", "cuts"]
    assert inspect.signature(pmctf_seq.plan_gops).parameters["cuts"].default == ()
    assert list(inspect.signature(pmctf_seq.scene_cuts).parameters) == ["mad", "hd", "hd_min", "mad_min"]
    q = inspect.signature(pmctf_seq.sequence_activity).parameters
    assert list(q) == ["reader_factory", "frame_num", "device", "bitdepth"] and q["bitdepth"].default == 8
    assert list(inspect.signature(pmctf_seq.read_gop_structure).parameters) == ["bin_folder"]
    from pMCTF.hip import ops
    o = inspect.signature(ops.luma_activity).parameters
    assert list(o) == ["cur", "prev", "bitdepth", "hist", "sad"]
    assert (o["bitdepth"].default, o["hist"].default, o["sad"].default) == (8, None, None)
    # the decoder's entry points keep their parameters
    assert list(inspect.signature(pmctf_gop.decode_gop_files).parameters) == [
        "codec", "bin_folder", "gop", "pic_height", "pic_width", "q_index", "psize", "me_downsample", "ll_order", "luma_stage0"]
    assert list(inspect.signature(pmctf_gop.read_sequence_header).parameters) == ["bin_folder"]
    with pytest.raises(ValueError):
        pmctf_gop.gop_pairs(1)                                        # a lone picture has no pairs, as before


def test_encode_refusals_come_before_the_codec_is_touched(tmp_path):
    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError(f"the codec was touched ({name}) before the arguments were checked")

    def call(frame_num=7, max_gop=4, **kw):
        return pmctf_seq.encode_sequence_gops(NoDevice(), str(tmp_path / "none.yuv"), 132, 100, frame_num, max_gop, 3,
                                              str(tmp_path), "cuda", **kw)
    for n in (0, -3, 7.0):
        with pytest.raises(ValueError, match="frame_num"):
            call(frame_num=n)
    for g in (1, 3, 6, 0, 8.0):
        with pytest.raises(ValueError, match="max_gop"):
            call(max_gop=g)
    with pytest.raises(ValueError, match="max_gop >= 4"):
        call(max_gop=2, structure="search")
    with pytest.raises(ValueError, match="structure"):
        call(structure="adaptive")
    with pytest.raises(ValueError, match="structure"):
        call(structure=5)
    for listed in ([(4, 1), (2, 1)], [(4, 1), (4, 1)], [(4, 1), (3, 1)], [(8, 1)], [(4, 1), (2, 3), (1, 1)], []):
        with pytest.raises(ValueError):
            call(structure=listed)
    for kw in ({"msssim": True}, {"decoded_frame_path": str(tmp_path / "png")}, {"src_format": "png"}, {"picture_hash": "u8"}):
        with pytest.raises(ValueError, match="bitdepth 10"):
            call(bitdepth=10, **kw)
    with pytest.raises(ValueError, match="bitdepth 8"):
        call(picture_hash="u16")
    with pytest.raises(ValueError):
        call(ingest="gpu")
    with pytest.raises(ValueError):
        call(structure="search", max_gop=8, ds_factors=(1, 3))
    assert os.listdir(tmp_path) == []
    with pytest.raises(RuntimeError, match="GPU"):                    # no CPU fallback
        pmctf_seq.sequence_activity(lambda: None, 4, "cpu")


# ------------------------------------------------------------------------------------------------------- C entry point
def test_entry_point_is_declared_bound_and_exported():
    from pMCTF.hip import lib
    text = open(os.path.join(ROOT, "include", "pmctf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert SYMBOL in set(re.findall(r"\b(pmctf_\w+)\s*\(", text)), "not declared in include/pmctf_hip.h"
    assert SYMBOL in lib.exported_symbols(), "no ctypes signature in pMCTF/hip/lib.py"
    assert hasattr(C.CDLL(lib.HIP_SO), SYMBOL), "libpmctf_hip.so does not export it"


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    from pMCTF.hip import lib
    fn = getattr(lib.hip(), SYMBOL)
    one = C.c_void_p(4096)                            # non-null, aligned, never dereferenced: the checks come first
    odd = lambda n: C.c_void_p(4096 + n)
    assert fn(None, one, 100, 132, 8, one, one, None) == -1
    assert fn(one, one, 100, 132, 8, None, one, None) == -1
    assert fn(None, None, 100, 132, 8, one, None, None) == -1
    assert fn(one, one, 100, 132, 8, one, None, None) == -1          # a previous picture needs somewhere to put the sum
    for b in (7, 17, 0, -1):
        assert fn(one, one, 100, 132, b, one, one, None) == -1, b
        assert fn(one, None, 100, 132, b, one, None, None) == -1, b
    for h, w in ((0, 132), (100, 0), (-2, 132), (100, -2), (16385, 132), (100, 16385)):
        assert fn(one, one, h, w, 8, one, one, None) == -1, (h, w)
        assert fn(one, None, h, w, 8, one, None, None) == -1, (h, w)
    for n in (4, 8, 12, 1):
        assert fn(odd(n), one, 100, 132, 8, one, one, None) == -1, n
        assert fn(one, odd(n), 100, 132, 8, one, one, None) == -1, n
        assert fn(odd(n), None, 100, 132, 8, one, None, None) == -1, n
    for n in (1, 2, 3):
        assert fn(one, one, 100, 132, 8, odd(n), one, None) == -1, n
    for n in (1, 2, 4, 6):
        assert fn(one, one, 100, 132, 8, one, odd(n), None) == -1, n


def test_wrapper_checks_its_arguments_before_any_launch():
    import torch
    from pMCTF.hip import ops
    y = torch.zeros((1, 1, 100, 132))
    for b in (7, 17):
        with pytest.raises(ValueError):
            ops.luma_activity(y, None, b)
    with pytest.raises(ValueError):
        ops.luma_activity(y.double(), None)
    with pytest.raises(ValueError):
        ops.luma_activity(y, torch.zeros((1, 1, 100, 130)))
    with pytest.raises(ValueError):
        ops.luma_activity(torch.zeros((2, 1, 100, 132)), None)
    with pytest.raises(RuntimeError):                 # no CPU fallback
        ops.luma_activity(y, None)
    with pytest.raises(RuntimeError):
        ops.luma_activity(y, y, 10)
