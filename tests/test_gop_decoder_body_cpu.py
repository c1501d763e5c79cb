"""The GOP decoders on a stand-in codec, no GPU: the full decode (pmctf_gop.decode_gop_files), the temporal levels and
motion_fill (pmctf_layers.decode_gop_files_layer) and random access (pmctf_access.decode_gop_files_frames) read the same
files, make the same codec calls in the same order and give the same pictures wherever they overlap.  The stand-in records
every call and computes exact float64 combinations, so every comparison is for equality.  The yardsticks are
tests/layers_restatement.py and tests/access_restatement.py, which know nothing of the product."""
import itertools
import os
import struct

import pytest
import torch

import access_restatement as ar
import layers_restatement as lr
import pmctf_access
import pmctf_gop
import pmctf_layers

H, W = 100, 132
SIZES = (1, 2, 4, 8, 16)
Q = 3


class Lifting:
    """what pmctf_gop.decode_gop needs of a codec, and no more: the oracle model and the reference network have no
    inverse_MCTF_ref.  Small integers in float64: every result is exact, whatever the order of the pairs."""
    num_me_stages = 2

    def __init__(self):
        self.log = []

    @staticmethod
    def _ref(L_t, H_t, mv_hat, downscale, stage_idx):
        return 3 * L_t - 2 * H_t + mv_hat + (stage_idx + 1) + (7 if downscale else 0)

    def inverse_MCTF(self, L_t, H_t, mv_hat, downscale=False, stage_idx=0):
        self.log.append(("inverse_MCTF", stage_idx, downscale))
        return self._ref(L_t, H_t, mv_hat, downscale, stage_idx), L_t + 4 * H_t - 2 * mv_hat + 11 * stage_idx


class Codec(Lifting):
    """the stand-in: one tiny CPU tensor per file, derived from the file's payload byte"""

    def __init__(self, fail_mv=None):
        super().__init__()
        self.fail_mv = fail_mv

    def inverse_MCTF_ref(self, L_t, H_t, mv_hat, downscale=False, stage_idx=0):
        self.log.append(("inverse_MCTF_ref", stage_idx, downscale))
        return self._ref(L_t, H_t, mv_hat, downscale, stage_idx)

    def _decompress_gop_files_begin(self, files, psize, q_index, ll_order, names=None, spatial_level=0):
        self.log.append(("begin", tuple((data[16], chroma, low, me_num) for data, chroma, low, me_num in files), psize, q_index,
                         ll_order, tuple(os.path.basename(n) for n in names), spatial_level))
        return [{"byte": data[16], "chroma": chroma} for data, chroma, _, _ in files], names

    def _decompress_gop_files_end(self, begun):
        jobs, _ = begun
        self.log.append(("end", tuple(job["byte"] for job in jobs)))
        for job in jobs:
            job.update(symbols_decoded=10 * job["byte"], payload_bytes_used=1)
        return [torch.tensor([job["byte"], -job["byte"]] if job["chroma"] else [job["byte"]], dtype=torch.float64)
                for job in jobs]

    def decompress_mv(self, string, dtype, height, width, dpb, stage_idx=0, q_index=0, me_downsample=1):
        self.log.append(("decompress_mv", string[0], dpb["mv_feature"], dpb["ref_mv_y"], stage_idx, height, width, q_index,
                         me_downsample))
        if string[0] == self.fail_mv:
            raise RuntimeError("the stream ends early")
        return {"mv_hat": torch.tensor([string[0]], dtype=torch.float64), "mv_feature": string[0], "mv_y_hat": 1000 + string[0]}


def _names(gop):
    return pmctf_gop.gop_file_names(gop) if gop != 1 else ["0_main.bin", "0_C_main.bin"]


def write_gop(folder, gop, h=H, w=W):
    """framed dummy files with correct headers: 16 bytes for a picture file, 6 for a motion file, one payload byte each, the
    file's place in the GOP's list plus one"""
    os.makedirs(folder, exist_ok=True)
    for at, name in enumerate(_names(gop)):
        payload = bytes([at + 1])
        if name.endswith("_mv.bin"):
            head = b"\x00\x00" + struct.pack(">I", len(payload))
        elif "_C_main" in name:
            head = struct.pack(">IIII", h // 2, w // 2, 2, len(payload))
        else:
            head = struct.pack(">IIII", h, w, 1, len(payload))
        with open(os.path.join(folder, name), "wb") as f:
            f.write(head + payload)
    return folder


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    root = tmp_path_factory.mktemp("gops")
    return {gop: write_gop(str(root / f"gop{gop}"), gop) for gop in SIZES}


@pytest.fixture(scope="module")
def full(folders):
    """the full decode of every size, computed once and left as it is"""
    out = {}
    for gop, folder in folders.items():
        codec = Codec()
        out[gop] = dict(pmctf_gop.decode_gop_files(codec, folder, gop, H, W, Q), log=codec.log)
    return out


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))


def call_logs(folders):
    """{name: the codec's call log} of the three decoders over the grid, for a diff between two commits"""
    logs = {}
    for gop, folder in folders.items():
        runs = {"full": lambda c: pmctf_gop.decode_gop_files(c, folder, gop, H, W, Q),
                "ca": lambda c: pmctf_gop.decode_gop_files(c, folder, gop, H, W, Q, me_downsample=2, luma_stage0=True)}
        for level in range(pmctf_layers.gop_stages(gop) + 2):
            for fill in (False, True):
                runs[f"level{level}{'_fill' if fill else ''}"] = \
                    lambda c, level=level, fill=fill: pmctf_layers.decode_gop_files_layer(c, folder, gop, H, W, Q, level,
                                                                                          motion_fill=fill)
        for n in range(gop):
            runs[f"frame{n}"] = lambda c, n=n: pmctf_access.decode_gop_files_frames(c, folder, gop, H, W, Q, [n])
        runs["frames_all"] = lambda c: pmctf_access.decode_gop_files_frames(c, folder, gop, H, W, Q, list(range(gop)))
        runs["frames_all_two_sided"] = lambda c: pmctf_access.decode_gop_files_frames(c, folder, gop, H, W, Q, list(range(gop)),
                                                                                      one_sided=False)
        for name, run in runs.items():
            codec = Codec()
            run(codec)
            logs[f"gop{gop}/{name}"] = [list(entry) for entry in codec.log]
    return logs


# ------------------------------------------------------------------------------------------------------------ one call log
def test_three_decoders_make_the_same_calls(folders, full):
    for gop, folder in folders.items():
        layer, frames = Codec(), Codec()
        a = pmctf_layers.decode_gop_files_layer(layer, folder, gop, H, W, Q, 0)
        b = pmctf_access.decode_gop_files_frames(frames, folder, gop, H, W, Q, list(range(gop)))
        assert full[gop]["log"] == layer.log == frames.log, gop
        assert [e[0] for e in layer.log[:1]] == ["begin"] and layer.log[0][5] == tuple(n for n in _names(gop)
                                                                                         if not n.endswith("_mv.bin"))
        assert a["files"] == b["files"] == _names(gop)
        assert a["bytes_read"] == b["bytes_read"] == sum(os.path.getsize(os.path.join(folder, n)) for n in _names(gop))
        assert _same(a["frames"], full[gop]["frames"]) and _same(b["frames"], full[gop]["frames"])
        assert a["symbols_decoded"] == b["symbols_decoded"] == {n: 10 * (_names(gop).index(n) + 1) for n in _names(gop)
                                                                if not n.endswith("_mv.bin")}
        assert set(a["payload_bytes_used"].values()) == {1} and a["payload_bytes_used"] == b["payload_bytes_used"]
        assert full[gop]["stages"] == a["stages"] == b["stages"] == lr.log2(gop)
        assert b["half_pairs"] == 0 and a["size"] == b["size"] == (H, W)


def test_full_decode_is_the_restated_synthesis(full):
    for gop, out in full.items():
        assert _same(out["frames"], lr.truncated_synthesis(Lifting(), out["frames_coded"], 0)), gop
        luma = [e for e in out["log"] if e[0] == "inverse_MCTF" and not e[2]]
        assert [e[1] for e in luma] == [min(1, s) for s in reversed(range(lr.log2(gop))) for _ in range(gop >> (s + 1))]


def test_luma_stage0_and_reduced_motion(folders):
    codec = Codec()
    pmctf_gop.decode_gop_files(codec, folders[8], 8, H, W, Q, me_downsample=2, luma_stage0=True)
    calls = [e for e in codec.log if e[0] == "inverse_MCTF"]
    assert {e[1] for e in calls if not e[2]} == {0} and [e[1] for e in calls if e[2]] == [1, 1, 1, 0, 0, 0, 0]
    motion = [e for e in codec.log if e[0] == "decompress_mv"]
    assert len(motion) == 7 and {e[5:] for e in motion} == {(64, 128, Q, 2)}, "the halved padded size, 128 x 256 at psize 128"
    for decode in (lambda c: pmctf_layers.decode_gop_files_layer(c, folders[8], 8, H, W, Q, 1, me_downsample=2),
                   lambda c: pmctf_access.decode_gop_files_frames(c, folders[8], 8, H, W, Q, [5], me_downsample=2)):
        other = Codec()
        decode(other)
        assert {e[5:] for e in other.log if e[0] == "decompress_mv"} == {(64, 128, Q, 2)}


def test_motion_context_restarts_at_each_stage(full):
    for gop, out in full.items():
        motion = [e for e in out["log"] if e[0] == "decompress_mv"]
        coding = ar.coding_order(gop)
        assert len(motion) == len(coding) == gop - 1
        before = None
        for (stage, _, i_cur), e in zip(coding, motion):
            byte = _names(gop).index(f"{i_cur}_mv.bin") + 1
            first = before is None or before[0] != stage
            assert e[1:5] == (byte, None if first else before[1], None if first else 1000 + before[1], min(1, stage))
            before = (stage, byte)
        # all files are read and handed over before the first motion file is decoded, and finished after the last
        assert [e[0] for e in out["log"]][:gop + 1] == ["begin"] + ["decompress_mv"] * (gop - 1) + ["end"]


# ------------------------------------------------------------------------------------------------------- temporal levels
def test_levels_read_the_restated_files_and_give_the_restated_pictures(folders, full):
    for gop, folder in folders.items():
        S = lr.log2(gop)
        for level in range(S + 2):
            codec = Codec()
            out = pmctf_layers.decode_gop_files_layer(codec, folder, gop, H, W, Q, level)
            assert out["files"] == lr.file_names(gop, level), (gop, level)
            assert out["times"] == list(range(0, gop, 2 ** min(level, S)))
            assert _same(out["frames"], lr.truncated_synthesis(Lifting(), full[gop]["frames_coded"], level)), (gop, level)
            assert not [e for e in codec.log if e[0] == "inverse_MCTF_ref"]
            assert len([e for e in codec.log if e[0] == "inverse_MCTF"]) == 2 * (gop - 1 - (gop - (gop >> min(level, S))))
            assert codec.log[0][5] == tuple(n for n in out["files"] if not n.endswith("_mv.bin"))


def test_a_level_is_the_full_plan_of_a_shorter_gop(folders):
    for size in range(1, 17):
        if size & (size - 1):
            continue
        for level in range(lr.log2(size) + 2):
            kk = min(level, lr.log2(size))
            plan = pmctf_access.gop_plan(size >> kk, range(size >> kk))
            shifted = sorted((s + kk, i_cur << kk) for s, _, i_cur, _ in plan["pairs"])
            names = [n for _, i in shifted for n in (f"{i}.bin", f"{i}_C_main.bin", f"{i}_mv.bin")]
            assert names + ["0_main.bin", "0_C_main.bin"] == pmctf_layers.layer_file_names(size, level) == \
                lr.file_names(size, level)
            assert all(want for _, _, _, want in plan["pairs"])


def test_motion_fill_is_decode_gop_of_the_zero_filled_entries(folders, full):
    for gop, folder in folders.items():
        S = lr.log2(gop)
        for level in range(S + 2):
            kk = min(level, S)
            codec = Codec()
            out = pmctf_layers.decode_gop_files_layer(codec, folder, gop, H, W, Q, level, motion_fill=True)
            assert out["files"] == lr.file_names(gop, level, True) and out["times"] == list(range(gop))
            entries = [list(e) for e in full[gop]["frames_coded"]]
            for stage, _, i_cur in ar.coding_order(gop):
                if stage < kk:
                    entries[i_cur][:2] = [torch.zeros(1, dtype=torch.float64), torch.zeros(2, dtype=torch.float64)]
            assert _same(out["frames_coded"], entries)
            assert all((a[2] is None) == (b[2] is None) and (a[2] is None or torch.equal(a[2], b[2]))
                       for a, b in zip(out["frames_coded"], entries))
            assert _same(out["frames"], pmctf_gop.decode_gop(Lifting(), entries)), (gop, level)
            assert [e for e in codec.log if e[0].startswith("inverse")] == \
                [e for e in full[gop]["log"] if e[0].startswith("inverse")]


# --------------------------------------------------------------------------------------------------------- random access
def _frames(folder, gop, wanted, **kw):
    codec = Codec()
    out = pmctf_access.decode_gop_files_frames(codec, folder, gop, H, W, Q, list(wanted), **kw)
    return out, codec.log


def _check_selection(folder, gop, wanted, full):
    out, log = _frames(folder, gop, wanted)
    assert _same(out["frames"], [full["frames"][t] for t in wanted]), (gop, wanted)
    assert out["times"] == list(wanted) and out["files"] == ar.closure(gop, wanted), (gop, wanted)
    refs = [e for e in log if e[0] == "inverse_MCTF_ref"]
    assert out["half_pairs"] == len([e for e in refs if not e[2]]) == len([e for e in refs if e[2]]), (gop, wanted)
    assert out["half_pairs"] == sum(not want for _, _, _, want in out["pairs"])
    assert log[0][5] == tuple(n for n in out["files"] if not n.endswith("_mv.bin"))
    return out


def test_every_single_picture_is_the_full_decode_s(folders, full):
    for gop, folder in folders.items():
        for n in range(gop):
            out = _check_selection(folder, gop, [n], full[gop])
            assert out["half_pairs"] == sum(not n >> s & 1 for s in range(lr.log2(gop)))


def test_every_subset_of_a_gop_of_8_is_the_full_decode_s(folders, full):
    count = 0
    for k in range(1, 9):
        for wanted in itertools.combinations(range(8), k):
            _check_selection(folders[8], 8, wanted, full[8])
            count += 1
    assert count == 255


def test_two_sided_runs_no_half_pair(folders, full):
    for gop, folder in folders.items():
        for wanted in ([0], [gop - 1], [gop // 2]):
            one, _ = _frames(folder, gop, wanted)
            two, log = _frames(folder, gop, wanted, one_sided=False)
            assert not [e for e in log if e[0] == "inverse_MCTF_ref"] and two["half_pairs"] == 0
            assert _same(two["frames"], one["frames"]) and two["files"] == one["files"] and two["pairs"] == one["pairs"]
            assert len([e for e in log if e[0] == "inverse_MCTF"]) == 2 * len(two["pairs"])


# ---------------------------------------------------------------------------------------------------------------- errors
def _copy_without(folders, tmp_path, gop, *left_out, to="copy"):
    import shutil
    dst = str(tmp_path / to)
    shutil.copytree(folders[gop], dst)
    for name in left_out:
        os.remove(os.path.join(dst, name))
    return dst


def test_a_missing_file_of_the_plan_raises_before_any_codec_call(folders, tmp_path):
    folder = _copy_without(folders, tmp_path, 8, "6_mv.bin")
    for decode in (lambda c: pmctf_gop.decode_gop_files(c, folder, 8, H, W, Q),
                   lambda c: pmctf_layers.decode_gop_files_layer(c, folder, 8, H, W, Q, 1),
                   lambda c: pmctf_layers.decode_gop_files_layer(c, folder, 8, H, W, Q, 2, motion_fill=True),
                   lambda c: pmctf_access.decode_gop_files_frames(c, folder, 8, H, W, Q, [5])):
        codec = Codec()
        with pytest.raises(ValueError, match="6_mv.bin: missing") as e:
            decode(codec)
        assert os.path.join(folder, "6_mv.bin") in str(e.value) and codec.log == []


def test_a_file_outside_the_plan_may_be_missing(folders, full, tmp_path):
    folder = _copy_without(folders, tmp_path, 8, "1.bin", "1_C_main.bin", "1_mv.bin", "3.bin", "7_mv.bin")
    out = pmctf_layers.decode_gop_files_layer(Codec(), folder, 8, H, W, Q, 1)
    assert _same(out["frames"], lr.truncated_synthesis(Lifting(), full[8]["frames_coded"], 1))
    with pytest.raises(ValueError, match="missing"):
        pmctf_gop.decode_gop_files(Codec(), folder, 8, H, W, Q)
    # picture 4 hangs on the motion of the pairs before its own, not on their pictures, and on nothing behind
    folder = _copy_without(folders, tmp_path, 8, "1.bin", "3_C_main.bin", "7.bin", "7_C_main.bin", "7_mv.bin", "2.bin",
                           to="selection")
    out = pmctf_access.decode_gop_files_frames(Codec(), folder, 8, H, W, Q, [4])
    assert _same(out["frames"], [full[8]["frames"][4]]) and "7_mv.bin" not in out["files"] and "1_mv.bin" in out["files"]


def test_a_header_of_another_size_names_the_file(folders, tmp_path):
    folder = write_gop(str(tmp_path / "other"), 4, H, W + 2)
    for decode in (lambda c: pmctf_gop.decode_gop_files(c, folder, 4, H, W, Q),
                   lambda c: pmctf_layers.decode_gop_files_layer(c, folder, 4, H, W, Q, 0),
                   lambda c: pmctf_access.decode_gop_files_frames(c, folder, 4, H, W, Q, [1])):
        codec = Codec()
        with pytest.raises(ValueError, match=rf"1\.bin: header says 1 plane\(s\) of {H}x{W + 2}, expected 1 of {H}x{W}"):
            decode(codec)
        assert codec.log == []


def test_a_failing_motion_file_is_named_and_the_batch_still_drained(folders):
    byte = _names(8).index("6_mv.bin") + 1
    for decode in (lambda c: pmctf_gop.decode_gop_files(c, folders[8], 8, H, W, Q),
                   lambda c: pmctf_layers.decode_gop_files_layer(c, folders[8], 8, H, W, Q, 1),
                   lambda c: pmctf_access.decode_gop_files_frames(c, folders[8], 8, H, W, Q, [5])):
        codec = Codec(fail_mv=byte)
        with pytest.raises(ValueError, match="the stream ends early") as e:
            decode(codec)
        assert str(e.value).startswith(os.path.join(folders[8], "6_mv.bin") + ": ")
        assert [x[0] for x in codec.log][-2:] == ["decompress_mv", "end"] and codec.log[-2][1] == byte
        assert not [x for x in codec.log if x[0].startswith("inverse")]


def test_decode_gop_needs_no_inverse_MCTF_ref(full):
    assert not hasattr(Lifting(), "inverse_MCTF_ref")
    for gop, out in full.items():
        for luma_stage0 in (False, True):
            codec = Lifting()
            entries = [list(e) for e in out["frames_coded"]]
            rec = pmctf_gop.decode_gop(codec, entries, luma_stage0=luma_stage0)
            assert rec is entries and len(codec.log) == 2 * (gop - 1)
            assert luma_stage0 or _same(rec, out["frames"])
            assert {e[1] for e in codec.log if not e[2]} <= ({0} if luma_stage0 else {0, 1})
