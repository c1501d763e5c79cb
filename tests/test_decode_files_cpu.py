"""The parts of the standalone decoder (pmctf_gop.decode_gop_files / decode_sequence) that need no GPU: the sequence
header, the enumeration of a GOP's files, the Python mirror of the batched LL decode's applicability, and the unchanged
default of encode_sequence."""
import inspect
import json
import os
import re

import pytest

import pmctf_gop
from helpers import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = dict(width=448, height=256, frame_num=16, gop=8, q_index=3, psize=128, me_downsample=1, num_me_stages=2,
              ll_order="plane", precision="f32", aten_threads=8)


def test_sequence_header_round_trip(tmp_path):
    path = pmctf_gop.write_sequence_header(str(tmp_path), **FIELDS)
    assert os.path.basename(path) == "sequence.json"
    got = pmctf_gop.read_sequence_header(str(tmp_path))
    assert got == dict(FIELDS, format_version=1)
    assert set(pmctf_gop.SEQUENCE_FIELDS) == set(FIELDS)


def test_sequence_header_refuses_what_it_does_not_know(tmp_path):
    d = str(tmp_path)
    with pytest.raises(ValueError, match="sequence.json"):
        pmctf_gop.read_sequence_header(d)                                   # no header at all
    with pytest.raises(ValueError, match="missing"):
        pmctf_gop.write_sequence_header(d, **{k: v for k, v in FIELDS.items() if k != "gop"})
    with pytest.raises(ValueError, match="unknown"):
        pmctf_gop.write_sequence_header(d, **FIELDS, colour="bt709")
    with pytest.raises(ValueError, match="ll_order"):
        pmctf_gop.write_sequence_header(d, **dict(FIELDS, ll_order="raster"))
    path = pmctf_gop.write_sequence_header(d, **FIELDS)
    record = json.load(open(path))
    for bad, what in ((dict(record, format_version=2), "format version"), (dict(record, format_version="1"), "format version"),
                      ({k: v for k, v in record.items() if k != "aten_threads"}, "aten_threads"),
                      (dict(record, ll_order="raster"), "ll_order"), (dict(record, frame_num=12), "multiple")):
        json.dump(bad, open(path, "w"))
        with pytest.raises(ValueError, match=what):
            pmctf_gop.read_sequence_header(d)
    open(path, "w").write("{not json")
    with pytest.raises(ValueError, match="not a sequence header"):
        pmctf_gop.read_sequence_header(d)


def test_codec_configuration_must_equal_the_headers():
    header = dict(FIELDS, format_version=1)
    same = {"num_me_stages": 2, "precision": "f32", "aten_threads": 8}
    pmctf_gop.check_sequence_header(header, same)
    for k, v in (("num_me_stages", 1), ("precision", "f32-chain"), ("aten_threads", 16)):
        with pytest.raises(ValueError, match=k):
            pmctf_gop.check_sequence_header(header, dict(same, **{k: v}))


def test_gop_file_names_are_what_encode_gop_writes():
    """GOP 4: the names the real reference's run left behind (the keys of the fixture's per-pair file listings; later
    pairs' listings repeat earlier files).  Other GOP lengths: the schedule of encode_gop restated here."""
    g = golden()
    written = {m.group(1) for m in (re.fullmatch(r"gop\.pair\d+\.file\.(.+)", k) for k in g.files) if m}
    assert len(written) == 11
    names = pmctf_gop.gop_file_names(4)
    assert len(names) == len(set(names)) and set(names) == written
    for gop in (2, 4, 8, 16):
        want, step = [], 1
        while step < gop:
            for i_ref in range(0, gop, 2 * step):
                want += [f"{i_ref + step}.bin", f"{i_ref + step}_C_main.bin", f"{i_ref + step}_mv.bin"]
            step *= 2
        want += ["0_main.bin", "0_C_main.bin"]
        assert pmctf_gop.gop_file_names(gop) == want
        assert len(want) == 3 * (gop - 1) + 2
        pairs = pmctf_gop.gop_pairs(gop)
        assert [p[0] for p in pairs] == sorted(p[0] for p in pairs) and len(pairs) == gop - 1
    for bad in (0, 1, 3, 12):
        with pytest.raises(ValueError):
            pmctf_gop.gop_file_names(bad)


def test_damaged_files_are_named(tmp_path):
    import struct
    p = str(tmp_path / "3.bin")
    with pytest.raises(ValueError, match="3.bin: missing"):
        pmctf_gop._read_framed(p, 16)
    body = struct.pack(">IIII", 128, 128, 1, 10) + bytes(10)
    open(p, "wb").write(body)
    assert pmctf_gop._read_framed(p, 16) == body
    open(p, "wb").write(body[:20])
    with pytest.raises(ValueError, match="3.bin: truncated"):
        pmctf_gop._read_framed(p, 16)
    open(p, "wb").write(body[:9])
    with pytest.raises(ValueError, match="3.bin: truncated"):
        pmctf_gop._read_framed(p, 16)
    open(p, "wb").write(body + b"\0")
    with pytest.raises(ValueError, match="3.bin: 1 surplus"):
        pmctf_gop._read_framed(p, 16)
    mv = struct.pack(">HI", 0, 4) + bytes(4)
    open(p, "wb").write(mv)
    assert pmctf_gop._read_framed(p, 6) == mv


def test_batched_ll_applicability_mirror_tracks_the_source():
    """HipEngine.ll_batch_form restates pmctf_ll_ar_batch_form (decode_ops.hip) so that tests can tell which path a case
    took.  Read the constants, the LDS estimate and the conditions from the source and hold the restatement to them; the
    estimate itself must be the one of the single-job entry (ll_decode_helper.lds_bytes, held to the source by
    test_product_cpu)."""
    import ll_decode_helper as hp
    from pMCTF.hip.engine import HipEngine
    src = open(os.path.join(ROOT, "learned-pmctf_amd", "csrc", "decode_ops.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "pmctf_hip.h")).read()
    const = {n: int(re.search(rf"constexpr int {n} = (\d+);", src).group(1)) for n in ("NF", "TB", "LL_BATCH_MAX_PLANES")}
    lim = re.search(r"constexpr int LL_BATCH_LDS_LIMIT = (\d+) \* (\d+);", src)
    limit = int(lim.group(1)) * int(lim.group(2))
    assert const["LL_BATCH_MAX_PLANES"] == HipEngine.LL_BATCH_MAX_PLANES and limit == HipEngine.LL_BATCH_LDS_LIMIT
    max_jobs = int(re.search(r"#define PMCTF_LL_BATCH_MAX_JOBS (\d+)", hdr).group(1))
    assert max_jobs == HipEngine.LL_BATCH_MAX_JOBS == 32
    for name, val in HipEngine.LL_ORDERS.items():
        assert int(re.search(rf"#define PMCTF_LL_ORDER_{name.upper()} (\d+)", hdr).group(1)) == val
    c_expr = lambda e: e.replace("(size_t)", "").replace("sizeof(int32_t)", "4").replace("sizeof(float)", "4")
    fn = src[src.index("inline size_t ll_batch_lds("):]
    fn = " ".join(fn[:fn.index("\n}\n")].split())
    lds = c_expr(re.search(r"const size_t lds = (.*?);", fn).group(1))
    extra = c_expr(re.search(r"return two_half \? lds \+ (.*?) : lds;", fn).group(1))
    body = src[src.index('extern "C" int pmctf_ll_ar_batch_form('):]
    body = " ".join(body[:body.index("\n}\n")].split())
    for cond in ("if (P < 1 || P > LL_BATCH_MAX_PLANES || W < 1 || cdf_cols < 3) return 0;",
                 "const int N = plane_order == PMCTF_LL_ORDER_PLANE ? 1 : P;",
                 "if (ll_batch_lds(N, W, cdf_cols, false) > LL_BATCH_LDS_LIMIT) return 0;",
                 "return ll_batch_lds(N, W, cdf_cols, true) > LL_BATCH_LDS_LIMIT ? 1 : 2;"):
        assert cond in body, cond
    assert ctypes_sizeof_job() == HipEngine.LL_JOB.itemsize == 64
    cols = 103
    for order in ("position", "plane"):
        for P in (1, 2, 3, 4):
            for W in (1, 7, 88, 89, 344, 345, 2676, 2677, 2932, 2933):
                N = 1 if order == "plane" else P
                env = dict(const, N=N, W=W, cdf_cols=cols)
                one = eval(lds, {}, env)
                two = one + eval(extra, {}, env)
                assert (one, two) == hp.lds_bytes(N, W, cols)
                want = 0 if (P > const["LL_BATCH_MAX_PLANES"] or one > limit) else (1 if two > limit else 2)
                assert HipEngine.ll_batch_form(P, W, cols, order) == want, (order, P, W)
                assert HipEngine.ll_batch_form(P, W, cols, order, hp.CHAIN) == 0
    # where the thresholds fall: position order follows the single-job entry's, plane order decodes single planes
    assert [HipEngine.ll_batch_form(2, w, cols, "position") for w in (88, 89, 344, 345)] == [2, 1, 1, 0]
    assert [HipEngine.ll_batch_form(2, w, cols, "plane") for w in (88, 89, 344, 345, 2676, 2677, 2933)] == [2, 2, 2, 2, 2, 1, 0]
    assert HipEngine.ll_batch_form(2, 8, cols, "raster") == 0


def ctypes_sizeof_job():
    """sizeof(pmctf_ll_job) as the header declares it: six 8-byte members and four int32"""
    hdr = open(os.path.join(ROOT, "include", "pmctf_hip.h")).read()
    body = re.search(r"typedef struct pmctf_ll_job \{(.*?)\} pmctf_ll_job;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = 0
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        if "*" in decl or decl.startswith(("int64_t", "uint64_t")):
            size += 8 * len(decl.split(","))
        else:
            assert decl.startswith("int32_t"), decl
            size += 4 * len(decl.split(","))
    return size


def test_batched_symbols_are_bound_with_their_signatures():
    from pMCTF.hip import lib
    L = lib.hip()
    for name in ("pmctf_ll_ar_batch_form", "pmctf_ll_ar_decode_batch_f32", "pmctf_planes_to_u8"):
        assert name in lib.exported_symbols() and hasattr(L, name)
    cols = 103
    from pMCTF.hip.engine import HipEngine
    for order, code in HipEngine.LL_ORDERS.items():
        for P in (1, 2, 3):
            for W in (1, 88, 89, 344, 345, 2677, 2933):
                assert L.pmctf_ll_ar_batch_form(P, W, cols, code) == HipEngine.ll_batch_form(P, W, cols, order)
    assert L.pmctf_ll_ar_batch_form(1, 8, cols, 2) == 0
    # invalid arguments are refused before anything is launched
    assert L.pmctf_ll_ar_decode_batch_f32(None, 1, None, None, None, cols, 0.0, 1.0, 1, 4, 4, 0, None) == -1
    assert L.pmctf_planes_to_u8(None, None, 1, 8, 8, 8, 8, None) == -1


def test_encode_sequence_keeps_its_default():
    sig = inspect.signature(pmctf_gop.encode_sequence)
    assert sig.parameters["keep_gops"].default is False
    assert list(sig.parameters)[:11] == ["codec", "yuv_path", "width", "height", "frame_num", "gop", "q_index", "bin_folder",
                                         "device", "skip_decoding", "psize"]
    assert sig.parameters["skip_decoding"].default is True and sig.parameters["psize"].default == 128
    d = inspect.signature(pmctf_gop.decode_gop_files).parameters
    assert (d["psize"].default, d["me_downsample"].default, d["ll_order"].default, d["luma_stage0"].default) == \
        (128, 1, "plane", False)
