"""Rate control on the GPU: pmctf_rate.encode_sequence_rate at 132x100 (padded to 256x128), 7 pictures as GOPs of 4, 2 and
1, q_choices (0, 7, 14, 20).  Every GOP is first coded at every choice with the fixed-q path (encode_sequence_gops); the
controller's run on that table of sizes is then predicted by tests/rate_restatement.py, and the encoder has to make exactly
those trials, in that order, and leave exactly the fixed-q path's files.  A second model decodes the folder with every
GOP's own q_index, fully and by temporal layer.  Everything is exact: integers and bytes."""
import os

import numpy as np
import pytest

import rate_restatement as rr
from helpers import product_model

pytestmark = pytest.mark.gpu

W, H, FRAMES, MAX_GOP = 132, 100, 7, 4
SIZES = (4, 2, 1)
CHOICES = (0, 7, 14, 20)
TOP_FILES = ["gop_00000", "gop_00001", "gop_00002", "gop_structure.json", "rate_control.json"]


def _gop_files(folder):
    return {n: open(os.path.join(folder, n), "rb").read() for n in sorted(os.listdir(folder))}


@pytest.fixture(scope="module")
def seq(cuda, tmp_path_factory):
    """one encoder model, one decoder model (same weights), the source, and every GOP coded at every choice by the
    fixed-q path: 12 tiny encodes, their files and sizes"""
    import pmctf_gop
    import pmctf_seq
    import pmctf_synth
    tmp = tmp_path_factory.mktemp("rate_control")
    out = {"tmp": tmp, "enc_net": product_model(1)[0], "dec_net": product_model(1)[0]}
    out["src8"] = str(tmp / "src8.yuv")
    pictures = pmctf_synth.synth_yuv420(W, H, FRAMES, seed=1234)
    pmctf_gop.write_yuv(out["src8"], pictures)
    out["src10"] = str(tmp / "src10.yuv")                    # the same pictures at ten bits: every sample times four
    pmctf_gop.write_yuv(out["src10"], [tuple(p.astype(np.uint16) << 2 for p in pic) for pic in pictures])
    out["files"], out["fixed"], out["bits"] = {}, {}, [[None] * len(CHOICES) for _ in SIZES]
    for i, q in enumerate(CHOICES):
        bins = str(tmp / f"fixed_q{q:02d}")
        os.makedirs(bins)
        r = pmctf_seq.encode_sequence_gops(out["enc_net"], out["src8"], W, H, FRAMES, MAX_GOP, q, bins, "cuda")
        assert [g["size"] for g in r["gops"]] == list(SIZES)
        out["fixed"][q] = r
        for k, size in enumerate(SIZES):
            files = _gop_files(os.path.join(bins, pmctf_gop.gop_folder(k)))
            names = pmctf_gop.gop_file_names(size) if size > 1 else ["0_main.bin", "0_C_main.bin"]
            assert sorted(files) == sorted(names)
            out["files"][k, q] = files
            out["bits"][k][i] = 8 * sum(len(files[n]) for n in names)
    print("sizes in bits, per GOP and choice:", out["bits"])
    for k, row in enumerate(out["bits"]):
        assert len(set(row)) == len(CHOICES), f"GOP {k}: the four sizes {row} are not distinct"
    out["sets"] = _parameter_sets(out["bits"])
    return out


# ------------------------------------------------------------------------------------------------ the three parameter sets
def _predict(table, p):
    return rr.run(SIZES, lambda k, q: table[k][CHOICES.index(q)], p["bitrate"], p["fps"], CHOICES, p["q_start"],
                  p["bucket_ms"], p["max_trials"], p["slack"])


def _parameter_sets(table):
    """Three sets derived from the table, at one picture per second (alloc = size x bitrate).
    generous: twice the dearest picture of any GOP at any choice, so everything fits; from the lowest choice with two
      trials per GOP, every GOP climbs one step and runs out of trials.
    starved: bucket 0 (no credit is ever carried) and a bitrate below the lone picture's smallest size: GOP 2 cannot fit.
    middle: the first bitrate, among those that give a picture one of the per-picture costs in the table, and q_start at
      which the credit that the bucket carries changes a later GOP's choice against the same run without a bucket, while
      every GOP fits; at 30000/1001 pictures per second and slack 0.05."""
    per_picture = sorted({-(-b // s) for row, s in zip(table, SIZES) for b in row})
    sets = {"generous": dict(bitrate=2 * per_picture[-1], fps=1, q_start=CHOICES[0], bucket_ms=1000, max_trials=2, slack=0.0),
            "starved": dict(bitrate=min(table[2]) - 8, fps=1, q_start=CHOICES[-1], bucket_ms=0, max_trials=4, slack=0.0)}
    for cost in per_picture:
        for q_start in CHOICES:
            # a fractional frame rate; the bitrate gives every picture `cost` bits, or one more
            p = dict(bitrate=cost * 30000 // 1001 + 1, fps=(30000, 1001), q_start=q_start, bucket_ms=10 ** 6, max_trials=4,
                     slack=0.05)
            with_bucket, without = _predict(table, p), _predict(table, dict(p, bucket_ms=0))
            changed = [k for k in range(1, len(SIZES)) if with_bucket[k]["q_index"] != without[k]["q_index"]
                       and with_bucket[k - 1]["credit"] > 0]
            if changed and all(r["fits"] for r in with_bucket) and "middle" not in sets:
                sets["middle"] = p
    return sets


def test_the_parameter_sets_cover_the_controller(seq):
    table, sets = seq["bits"], seq["sets"]
    assert sorted(sets) == ["generous", "middle", "starved"], "no bitrate at which a carried credit changes a choice"
    runs = {name: _predict(table, p) for name, p in sets.items()}
    for name, run in runs.items():
        print(name, sets[name], [(r["q_index"], r["fits"], r["bits"], r["budget"], r["credit"], r["trials"]) for r in run])
    records = [(sets[name], r) for name, run in runs.items() for r in run]
    step = lambda r, sign: any((b[0] - a[0]) * sign > 0 for a, b in zip(r["trials"], r["trials"][1:]))
    assert any(step(r, +1) for _, r in records), "an upward step"
    assert any(step(r, -1) for _, r in records), "a downward step"
    assert any(len(r["trials"]) == p["max_trials"] and r["q_index"] not in (CHOICES[0], CHOICES[-1]) for p, r in records), \
        "max_trials exhausted before the end of the choices"
    assert any(not r["fits"] for _, r in records), "a GOP that does not fit"
    assert all(r["fits"] for r in runs["generous"]) and not runs["starved"][2]["fits"]
    assert runs["starved"][2]["budget"] < min(table[2])
    # a positive carried credit that changes a later choice
    p = sets["middle"]
    without = _predict(table, dict(p, bucket_ms=0))
    assert any(a["credit"] > 0 and b["q_index"] != c["q_index"]
               for a, b, c in zip(runs["middle"], runs["middle"][1:], without[1:]))
    assert len({r["q_index"] for r in runs["middle"]} | {r["q_index"] for r in runs["starved"]}) > 1


# ------------------------------------------------------------------------------------------------------------- the encoder
def _encode(seq, name, folder, **kw):
    import pmctf_rate
    p = seq["sets"][name]
    bins = str(seq["tmp"] / folder)
    os.makedirs(bins)
    src = kw.pop("source", seq["src8"])
    r = pmctf_rate.encode_sequence_rate(seq["enc_net"], src, W, H, FRAMES, MAX_GOP, p["bitrate"], p["fps"], bins, "cuda",
                                        q_choices=CHOICES, q_start=p["q_start"], bucket_ms=p["bucket_ms"],
                                        max_trials=p["max_trials"], slack=p["slack"], **kw)
    return bins, r


def _check_against_the_table(seq, name, bins, r, extra=()):
    import pmctf_gop
    import pmctf_rate
    import pmctf_seq
    want = _predict(seq["bits"], seq["sets"][name])
    # the restatement, exactly: trials in order, choices, fits, credits
    assert [{f: rec[f] for f in pmctf_rate.RECORD_FIELDS} for rec in r["rate"]] == want
    assert all(set(rec) == set(pmctf_rate.RECORD_FIELDS) | {"seconds"} and rec["seconds"] > 0 for rec in r["rate"])
    # no trial folder is left, and every file is the fixed-q path's file of that GOP at the chosen q
    assert sorted(os.listdir(bins)) == sorted(TOP_FILES + list(extra))
    for k, rec in enumerate(want):
        got = _gop_files(os.path.join(bins, pmctf_gop.gop_folder(k)))
        fixed = seq["files"][k, rec["q_index"]]
        assert sorted(got) == sorted(fixed), k
        for n in fixed:
            assert got[n] == fixed[n], f"GOP {k}, {n}: not the file of q_index {rec['q_index']}"
    # the header, the record, the returned tables
    header = pmctf_seq.read_gop_structure(bins)
    assert header["format_version"] == 2 and header["gops"] == r["gops"] and header["q_index"] == want[0]["q_index"]
    assert [g["q_index"] for g in r["gops"]] == [rec["q_index"] for rec in want]
    assert [(g["first"], g["size"]) for g in r["gops"]] == [(0, 4), (4, 2), (6, 1)]
    v = pmctf_rate.verify_rate_record(bins)
    assert v["total_bits"] == sum(rec["bits"] for rec in want) == int(sum(r["bits"])) and v["frame_num"] == FRAMES
    assert v["record"]["gops"] == [dict(rec, trials=[list(t) for t in rec["trials"]]) for rec in want]
    assert r["frame_types"] == [0, 1, 1, 1, 0, 1, 0] and len(r["psnr"]) == FRAMES
    # report_gop ran once per GOP, on the accepted trial's reconstruction: the rows of the fixed-q coding at the chosen q
    for rec, first, size in zip(want, (0, 4, 6), SIZES):
        for table in ("bits", "bpp_mv") + (() if "picture_format.json" in extra else ("psnr", "psnr_rgb")):
            assert r[table][first:first + size] == seq["fixed"][rec["q_index"]][table][first:first + size], (table, first)
    # the "average ms" lines count the pairs of the accepted trials: 3 + 1
    assert [ln.split(",")[0] for ln in r["lines"][-2:]] == ["encoding 4 P frames", "decoding 4 P frames"]
    return want


@pytest.mark.parametrize("name", ["generous", "middle", "starved"])
def test_encoder_equals_the_restatement_and_the_fixed_q_files(seq, name):
    bins, r = _encode(seq, name, f"rate_{name}")
    _check_against_the_table(seq, name, bins, r)


def test_decoders_use_every_gops_own_q_index(seq, cuda):
    import pmctf_gop
    import pmctf_layers
    name = "middle" if len({r["q_index"] for r in _predict(seq["bits"], seq["sets"]["middle"])}) > 1 else "starved"
    bins, r = _encode(seq, name, "rate_hashed", picture_hash="u8")
    want = _check_against_the_table(seq, name, bins, r, extra=["picture_hashes.json"])
    assert len({rec["q_index"] for rec in want}) > 1, "the GOPs were coded at different q_index values"
    yuv = str(seq["tmp"] / "rate_hashed.yuv")
    d = pmctf_gop.decode_sequence_checked(seq["dec_net"], bins, yuv, "cuda", verify=True)
    assert d["verified"] == FRAMES and d["hash_mismatches"] == [] and d["header"]["format_version"] == 2
    assert pmctf_gop.check_yuv_hashes(bins, yuv) == (FRAMES, [])
    assert r["picture_hashes"] == pmctf_gop.read_picture_hashes(bins, FRAMES)["frames"]
    # temporal layers: the record from a full decode by the second model, then level 1 from the folder and from an extract
    pmctf_layers.write_layer_hashes(seq["dec_net"], bins)
    times = [0, 2, 4, 6]
    for folder in (bins, str(seq["tmp"] / "rate_hashed_level1")):
        if folder != bins:
            pmctf_layers.extract_layer(bins, folder, 1)
            assert open(os.path.join(folder, "gop_structure.json")).read() == open(os.path.join(bins, "gop_structure.json")).read()
        d = pmctf_layers.decode_sequence_layer(seq["dec_net"], folder, str(seq["tmp"] / "rate_level1.yuv"), 1, "cuda",
                                               verify=True)
        assert d["verified"] == len(times) and d["times"] == times and d["hash_mismatches"] == []


def test_ten_bits(seq, cuda):
    """the ten-bit source whose samples are four times the 8-bit ones codes to the 8-bit files, so the table holds"""
    import pmctf_gop
    bins, r = _encode(seq, "middle", "rate_ten_bits", source=seq["src10"], bitdepth=10, picture_hash="u16")
    _check_against_the_table(seq, "middle", bins, r, extra=["picture_format.json", "picture_hashes.json"])
    assert r["psnr_rgb"] == [0.0] * FRAMES
    yuv = str(seq["tmp"] / "rate_ten_bits.yuv")
    d = pmctf_gop.decode_sequence_checked(seq["dec_net"], bins, yuv, "cuda", verify=True)
    assert d["verified"] == FRAMES and d["bitdepth"] == 10 and d["hash_mismatches"] == []
    assert os.path.getsize(yuv) == FRAMES * W * H * 3 and pmctf_gop.check_yuv_hashes(bins, yuv) == (FRAMES, [])
