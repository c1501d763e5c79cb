"""Random access on the GPU (pmctf_access) at 132x100, padded to 256x128, q 3: chosen pictures decoded from the files they
depend on against the same pictures of the full decode, the one-sided lifting against the two-sided one, the files that are
read and those that are not, a structured sequence of 7 pictures through decode_frames with its hashes, a spatial level, ten
bits, reduced-resolution motion, the sinks, read_frames and the tool.  Everything is exact: torch.equal, bytes and integers.
No bitstream file that is decoded is ever altered: the tampering is done on JSON records, and files outside the set that is
read are removed."""
import importlib.util
import json
import os
import shutil

import numpy as np
import pytest
import torch

from helpers import product_model

pytestmark = pytest.mark.gpu

W, H, Q = 132, 100, 3
N8 = W * H * 3 // 2                                    # samples of one 4:2:0 picture


@pytest.fixture(scope="module")
def seq(cuda, tmp_path_factory):
    """one encoder model, one decoder model (same weights), the source, the folders coded once with f32 picture hashes (one
    GOP of 8; 7 pictures as GOPs of 4, 2, 1) and their full decodes, computed once and left alone.  Tests copy a folder
    before they change anything in it."""
    import pmctf_gop
    import pmctf_seq
    import pmctf_synth
    tmp = tmp_path_factory.mktemp("random_access")
    out = {"tmp": tmp, "enc_net": product_model(1)[0], "dec_net": product_model(1)[0]}
    out["src8"] = str(tmp / "src8.yuv")
    pmctf_gop.write_yuv(out["src8"], pmctf_synth.synth_yuv420(W, H, 8, seed=1234))
    out["eight"], out["seven"] = str(tmp / "eight"), str(tmp / "seven")
    for name in ("eight", "seven"):
        os.makedirs(out[name])
    r = pmctf_seq.encode_sequence_gops(out["enc_net"], out["src8"], W, H, 8, 8, Q, out["eight"], "cuda", picture_hash="f32")
    assert [g["size"] for g in r["gops"]] == [8]
    r = pmctf_seq.encode_sequence_gops(out["enc_net"], out["src8"], W, H, 7, 4, Q, out["seven"], "cuda", picture_hash="f32")
    assert [g["size"] for g in r["gops"]] == [4, 2, 1]
    out["gop8"] = os.path.join(out["eight"], "gop_00000")
    out["full8"] = pmctf_gop.decode_gop_files(out["dec_net"], out["gop8"], 8, H, W, Q)
    out["yuv7"] = str(tmp / "seven_full.yuv")
    d = pmctf_gop.decode_sequence_checked(out["dec_net"], out["seven"], out["yuv7"], "cuda")
    assert d["verified"] == 7 and os.path.getsize(out["yuv7"]) == 7 * N8
    return out


def _same_picture(a, b, what=""):
    assert a[0].shape == b[0].shape and a[1].shape == b[1].shape, what
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), what
    assert a[2] is None


def _copy(seq, name, to):
    dst = str(seq["tmp"] / to)
    shutil.copytree(seq[name], dst)
    return dst


def _pictures(path, indices, size=N8, dtype=np.uint8):
    data = np.fromfile(path, dtype=dtype)
    return np.concatenate([data[i * size:(i + 1) * size] for i in indices])


# --------------------------------------------------------------------------------------------------- 1. single pictures
def test_every_single_picture_of_a_gop_of_8(seq):
    import pmctf_access
    full = seq["full8"]["frames"]
    for n in range(8):
        plan = pmctf_access.gop_plan(8, [n])
        got = pmctf_access.decode_gop_files_frames(seq["dec_net"], seq["gop8"], 8, H, W, Q, [n])
        assert len(got["frames"]) == 1 and got["times"] == [n] and got["stages"] == 3
        _same_picture(got["frames"][0], full[n], f"picture {n}")
        assert got["files"] == plan["files"] and got["pairs"] == plan["pairs"]
        assert got["bytes_read"] == sum(os.path.getsize(os.path.join(seq["gop8"], f)) for f in plan["files"])
        assert got["half_pairs"] == sum(not want for _, _, _, want in plan["pairs"]) == 3 - bin(n).count("1")
        assert got["spatial_level"] == 0 and got["size"] == (H, W)
        pictures = [f for f in plan["files"] if not f.endswith("_mv.bin")]
        assert sorted(got["symbols_decoded"]) == sorted(got["payload_bytes_used"]) == sorted(pictures) and len(pictures) == 8


# ------------------------------------------------------------------------------------------------------------ 2. subsets
def test_subsets_one_sided_and_two_sided(seq):
    import pmctf_access
    full, halves = seq["full8"]["frames"], {}
    for wanted in ([0], [7], [2, 3], [1, 6], list(range(8))):
        one = pmctf_access.decode_gop_files_frames(seq["dec_net"], seq["gop8"], 8, H, W, Q, wanted, one_sided=True)
        two = pmctf_access.decode_gop_files_frames(seq["dec_net"], seq["gop8"], 8, H, W, Q, wanted, one_sided=False)
        assert one["times"] == two["times"] == wanted and one["files"] == two["files"] and two["half_pairs"] == 0
        assert len(one["frames"]) == len(two["frames"]) == len(wanted)
        for t, a, b in zip(wanted, one["frames"], two["frames"]):
            _same_picture(a, b, f"{wanted}: picture {t}, one-sided against two-sided")
            _same_picture(a, full[t], f"{wanted}: picture {t}")
        halves[tuple(wanted)] = one["half_pairs"]
        if len(wanted) == 8:
            assert one["half_pairs"] == 0 and one["files"] == pmctf_access.pmctf_gop.gop_file_names(8)
    # [0]: `ref` alone at every stage; [7]: `cur` at every stage; [2, 3]: (2, 3) and (0, 2) whole, (0, 4) `ref` alone;
    # [1, 6]: (0, 1) whole, (6, 7) `ref` alone, (0, 2) `ref` alone, (4, 6) and (0, 4) whole
    assert halves == {(0,): 3, (7,): 0, (2, 3): 1, (1, 6): 2, tuple(range(8)): 0}


# -------------------------------------------------------------------------------------------------- 3. inverse_MCTF_ref
def test_inverse_mctf_ref_is_the_first_result_of_inverse_mctf(seq):
    net, coded = seq["dec_net"], seq["full8"]["frames_coded"]
    for i_cur in (4, 3):                               # decoded entries: the low band, a high band of the last or the first stage
        (L_t, L_tc, _), (H_t, H_tc, mv_hat) = coded[0], coded[i_cur]
        ref, cur = net.inverse_MCTF(L_t, H_t, mv_hat)
        only = net.inverse_MCTF_ref(L_t, H_t, mv_hat)
        assert only.shape == ref.shape and torch.equal(only, ref) and not torch.equal(ref, L_t)
        ref_c, cur_c = net.inverse_MCTF(L_tc, H_tc, mv_hat, stage_idx=0, downscale=True)
        only_c = net.inverse_MCTF_ref(L_tc, H_tc, mv_hat, stage_idx=0, downscale=True)
        assert only_c.shape == ref_c.shape and torch.equal(only_c, ref_c) and not torch.equal(ref_c, L_tc)
        eng = net.engine()                                               # and the engine's own, which inverse_MCTF calls
        c = lambda t: t.contiguous()
        assert torch.equal(eng.inverse_MCTF_ref(c(L_t), c(H_t), c(mv_hat)), ref)
        assert torch.equal(eng.inverse_MCTF_ref(c(L_tc), c(H_tc), c(mv_hat), downscale=True), ref_c)


# ---------------------------------------------------------------------------------------- 4. only the planned files
def test_only_the_planned_files_are_read(seq):
    import pmctf_access
    import pmctf_gop
    folder = os.path.join(_copy(seq, "eight", "eight_picture5"), "gop_00000")
    keep = pmctf_access.access_file_names(8, [5])
    others = [n for n in pmctf_gop.gop_file_names(8) if n not in keep]
    assert len(keep) == 14 and len(others) == 9
    for n in others:
        os.remove(os.path.join(folder, n))
    assert sorted(os.listdir(folder)) == sorted(keep)
    got = pmctf_access.decode_gop_files_frames(seq["dec_net"], folder, 8, H, W, Q, [5])
    _same_picture(got["frames"][0], seq["full8"]["frames"][5])
    assert got["files"] == keep
    for n in others:                                                     # garbage too short for any header
        open(os.path.join(folder, n), "wb").write(b"abc")
    got = pmctf_access.decode_gop_files_frames(seq["dec_net"], folder, 8, H, W, Q, [5])
    _same_picture(got["frames"][0], seq["full8"]["frames"][5])
    os.remove(os.path.join(folder, "6_C_main.bin"))                      # the high band of the pair that runs `ref` alone
    with pytest.raises(ValueError, match="6_C_main.bin: missing"):
        pmctf_access.decode_gop_files_frames(seq["dec_net"], folder, 8, H, W, Q, [5])
    os.remove(os.path.join(folder, "3_mv.bin"))                          # of the motion prefix of stage 0, read before
    with pytest.raises(ValueError, match="3_mv.bin: missing"):
        pmctf_access.decode_gop_files_frames(seq["dec_net"], folder, 8, H, W, Q, [5])
    got = pmctf_access.decode_gop_files_frames(seq["dec_net"], seq["gop8"], 8, H, W, Q, [0])    # picture 0 needs 1, 2, 4 alone
    assert got["files"] == ["1.bin", "1_C_main.bin", "1_mv.bin", "2.bin", "2_C_main.bin", "2_mv.bin", "4.bin",
                            "4_C_main.bin", "4_mv.bin", "0_main.bin", "0_C_main.bin"]


# ------------------------------------------------------------------------------------------ 5. a window of a sequence
def test_decode_frames_on_the_structured_sequence(seq):
    import pmctf_access
    import pmctf_gop
    net, bins = seq["dec_net"], _copy(seq, "seven", "seven_window")
    want = _pictures(seq["yuv7"], [2, 3, 4, 5])
    yuv = str(seq["tmp"] / "window.yuv")
    d = pmctf_access.decode_frames(net, bins, yuv, range(2, 6), "cuda")
    assert np.array_equal(np.fromfile(yuv, dtype=np.uint8), want)
    assert d["verified"] == 4 and d["times"] == [2, 3, 4, 5] and d["hash_mismatches"] == [] and d["gops_opened"] == 2
    assert d["frames"] == [(H, W)] * 4 and d["bitdepth"] == 8 and d["spatial_level"] == 0 and d["size"] == (H, W)
    assert d["bytes_read"] == pmctf_access.access_bytes(bins, range(2, 6)) and len(d["seconds"]) == 3
    assert d["half_pairs"] == 0, "pictures 2, 3 of the GOP of 4 need `cur` of (0, 2) and of (2, 3); 4, 5 are a whole GOP"
    assert pmctf_access.decode_frames(net, bins, yuv, [2], "cuda")["half_pairs"] == 1
    assert np.array_equal(np.fromfile(yuv, dtype=np.uint8), want[:N8])
    # the lone picture's GOP is not touched: its folder may be gone
    shutil.rmtree(os.path.join(bins, "gop_00002"))
    again = pmctf_access.decode_frames(net, bins, yuv, (2, 6), "cuda")
    assert np.array_equal(np.fromfile(yuv, dtype=np.uint8), want)
    assert {k: v for k, v in again.items() if k != "seconds"} == {k: v for k, v in d.items() if k != "seconds"}
    with pytest.raises(ValueError, match="gop_00002.0_main.bin: missing"):
        pmctf_access.decode_frames(net, bins, yuv, [6], "cuda")
    # every picture: the bytes of decode_sequence_checked
    everything = str(seq["tmp"] / "window_all.yuv")
    d = pmctf_access.decode_frames(net, seq["seven"], everything, range(7), "cuda", verify=True)
    assert open(everything, "rb").read() == open(seq["yuv7"], "rb").read()
    assert d["verified"] == 7 and d["times"] == list(range(7)) and d["gops_opened"] == 3 and d["half_pairs"] == 0
    assert d["bytes_read"] == pmctf_access.pmctf_layers.layer_bytes(seq["seven"], 0)
    # one recorded value of a wanted frame changed, no bitstream touched: picture 4 (GOP 1)
    path = os.path.join(bins, "picture_hashes.json")
    intact = json.load(open(path))
    rec = json.loads(json.dumps(intact))
    rec["frames"][4]["c_f32"] ^= 1
    json.dump(rec, open(path, "w"))
    with pytest.raises(pmctf_gop.PictureHashMismatch) as e:
        pmctf_access.decode_frames(net, bins, yuv, range(2, 6), "cuda")
    m = e.value.mismatch
    assert (m["frame"], m["plane"], m["gop"]) == (4, "c_f32", 1) and m["recorded"] == m["decoded"] ^ 1
    assert "frame 4, plane c_f32" in str(e.value) and "gop_00001" in str(e.value)
    assert os.path.getsize(yuv) == 2 * N8, "GOP 0 was written, nothing of GOP 1"
    d = pmctf_access.decode_frames(net, bins, yuv, range(2, 6), "cuda", verify="report")
    assert [(x["frame"], x["plane"]) for x in d["hash_mismatches"]] == [(4, "c_f32")] and d["verified"] == 4
    assert np.array_equal(np.fromfile(yuv, dtype=np.uint8), want)
    d = pmctf_access.decode_frames(net, bins, yuv, range(2, 6), "cuda", verify=False)
    assert d["verified"] == 0 and np.array_equal(np.fromfile(yuv, dtype=np.uint8), want)
    # the record of a frame that is not wanted does not matter
    d = pmctf_access.decode_frames(net, bins, yuv, [2, 3, 5], "cuda", verify=True)
    assert d["verified"] == 3 and d["hash_mismatches"] == [] and d["times"] == [2, 3, 5]
    assert np.array_equal(np.fromfile(yuv, dtype=np.uint8), _pictures(seq["yuv7"], [2, 3, 5]))
    os.remove(path)
    with pytest.raises(ValueError, match="picture_hashes.json"):
        pmctf_access.decode_frames(net, bins, yuv, [2], "cuda", verify=True)
    assert pmctf_access.decode_frames(net, bins, yuv, [2], "cuda")["verified"] == 0


# ------------------------------------------------------------------------------------------------------ 6. spatial level
def test_spatial_level_1(seq):
    import pmctf_access
    import pmctf_gop
    import pmctf_spatial
    net, bins = seq["dec_net"], _copy(seq, "seven", "seven_spatial")
    pmctf_spatial.write_spatial_hashes(seq["enc_net"], bins)
    n = N8 // 4                                                          # 66 x 50
    full = str(seq["tmp"] / "spatial_full.yuv")
    d = pmctf_spatial.decode_sequence_layer(net, bins, full, 0, "cuda", verify=True, spatial_level=1)
    assert d["verified"] == 7 and os.path.getsize(full) == 7 * n
    yuv = str(seq["tmp"] / "spatial_1_5.yuv")
    d = pmctf_access.decode_frames(net, bins, yuv, [1, 5], "cuda", verify=True, spatial_level=1)
    assert np.array_equal(np.fromfile(yuv, dtype=np.uint8), _pictures(full, [1, 5], n))
    assert d["verified"] == 2 and d["hash_mismatches"] == [] and d["times"] == [1, 5] and d["gops_opened"] == 2
    assert d["spatial_level"] == 1 and d["size"] == (H // 2, W // 2) and d["frames"] == [(H // 2, W // 2)] * 2
    assert d["bytes_read"] == pmctf_access.access_bytes(bins, [1, 5])
    # the record that is checked is that of (spatial level 1, temporal level 0) of the wanted index
    path = os.path.join(bins, "spatial_hashes.json")
    rec = json.load(open(path))
    assert rec["layers"]["1"]["0"][5]["index"] == 5
    rec["layers"]["1"]["0"][5]["y"] ^= 1
    rec["layers"]["1"]["0"][4]["y"] ^= 1                                 # not wanted
    rec["layers"]["1"]["1"][0]["y"] ^= 1                                 # another temporal level
    json.dump(rec, open(path, "w"))
    with pytest.raises(pmctf_gop.PictureHashMismatch) as e:
        pmctf_access.decode_frames(net, bins, yuv, [1, 5], "cuda", spatial_level=1)
    assert (e.value.mismatch["frame"], e.value.mismatch["plane"], e.value.mismatch["gop"]) == (5, "y", 1)
    assert os.path.getsize(yuv) == n, "picture 1 was written, nothing of GOP 1"
    os.remove(path)
    with pytest.raises(ValueError, match="spatial_hashes.json: missing"):
        pmctf_access.decode_frames(net, bins, yuv, [1, 5], "cuda", verify=True, spatial_level=1)
    with pytest.raises(ValueError, match=r"132x100 offer the spatial levels 0\.\.1"):
        pmctf_access.decode_frames(net, bins, yuv, [1], "cuda", spatial_level=2)


# --------------------------------------------------------------------------------- 7. ten bits, reduced-resolution motion
def test_ten_bits_and_reduced_resolution_motion(seq):
    import hbd_restatement as hr
    import pmctf_access
    import pmctf_gop
    import pmctf_seq
    net = seq["dec_net"]
    src = str(seq["tmp"] / "src10.yuv")
    pmctf_gop.write_yuv(src, hr.synth_hbd(W, H, 5, 10, seed=5))
    bins = str(seq["tmp"] / "ten_bits")
    os.makedirs(bins)
    r = pmctf_seq.encode_sequence_gops(seq["enc_net"], src, W, H, 5, 4, Q, bins, "cuda", bitdepth=10, picture_hash="u16")
    assert [g["size"] for g in r["gops"]] == [4, 1]
    full, yuv = str(seq["tmp"] / "ten_bits_full.yuv"), str(seq["tmp"] / "ten_bits_3.yuv")
    pmctf_gop.decode_sequence_checked(net, bins, full, "cuda")
    d = pmctf_access.decode_frames(net, bins, yuv, [3], "cuda", verify=True)
    assert d["verified"] == 1 and d["bitdepth"] == 10 and d["times"] == [3] and d["gops_opened"] == 1
    got = np.fromfile(yuv, dtype="<u2")
    assert got.size == N8 and int(got.max()) <= 1023 and np.array_equal(got, _pictures(full, [3], dtype="<u2"))
    with pytest.raises(ValueError, match="picture_format.json"):
        pmctf_access.decode_frames(net, bins, None, [3], png_out=str(seq["tmp"] / "ten_png"))
    # motion coded at half the resolution
    bins = str(seq["tmp"] / "half_motion")
    os.makedirs(bins)
    r = pmctf_seq.encode_sequence_gops(seq["enc_net"], seq["src8"], W, H, 4, 4, Q, bins, "cuda", structure=[(4, 2)])
    assert r["gops"] == [{"first": 0, "size": 4, "me_downsample": 2, "psize": 128}]
    folder = os.path.join(bins, "gop_00000")
    whole = pmctf_gop.decode_gop_files(net, folder, 4, H, W, Q, psize=128, me_downsample=2)
    got = pmctf_access.decode_gop_files_frames(net, folder, 4, H, W, Q, [3], psize=128, me_downsample=2)
    _same_picture(got["frames"][0], whole["frames"][3])
    assert got["files"] == ["1_mv.bin", "3.bin", "3_C_main.bin", "3_mv.bin", "2.bin", "2_C_main.bin", "2_mv.bin", "0_main.bin",
                            "0_C_main.bin"] and got["half_pairs"] == 0
    yuv, full = str(seq["tmp"] / "half_motion_3.yuv"), str(seq["tmp"] / "half_motion_full.yuv")
    pmctf_gop.decode_sequence_checked(net, bins, full, "cuda")
    assert pmctf_access.decode_frames(net, bins, yuv, [3], "cuda")["times"] == [3]
    assert np.array_equal(np.fromfile(yuv, dtype=np.uint8), _pictures(full, [3]))


# ----------------------------------------------------------------------------------------------------------- 8. the sinks
def test_sinks(seq):
    import pmctf_access
    import pmctf_chroma
    import pmctf_layout
    net, bins = seq["dec_net"], seq["seven"]
    # Y4M: the header, then FRAME and the planes per picture
    full, part = str(seq["tmp"] / "sink_full.y4m"), str(seq["tmp"] / "sink_3_5.y4m")
    pmctf_chroma.decode_sequence_checked(net, bins, full, "cuda")
    d = pmctf_access.decode_frames(net, bins, part, range(3, 6), "cuda")
    assert d["times"] == [3, 4, 5] and d["verified"] == 3
    whole, got = open(full, "rb").read(), open(part, "rb").read()
    head, step = whole.index(b"FRAME\n"), len(b"FRAME\n") + N8
    assert len(whole) == head + 7 * step and whole[head + N8 + 6:head + N8 + 12] == b"FRAME\n"
    assert got == whole[:head] + whole[head + 3 * step:head + 6 * step]
    # NV12: packed on the device after the pictures are chosen
    full, part = str(seq["tmp"] / "sink_full.nv12"), str(seq["tmp"] / "sink_3_5.nv12")
    pmctf_layout.decode_sequence_checked(net, bins, full, "cuda", output_layout="nv12")
    d = pmctf_access.decode_frames(net, bins, part, range(3, 6), "cuda", output_layout="nv12")
    assert d["times"] == [3, 4, 5] and os.path.getsize(full) == 7 * N8
    assert open(part, "rb").read() == open(full, "rb").read()[3 * N8:6 * N8]
    assert open(part, "rb").read() != open(seq["yuv7"], "rb").read()[3 * N8:6 * N8], "NV12 interleaves the chroma"
    # PNGs carry the source indices and are those of the full decode
    all_png, png = str(seq["tmp"] / "sink_png_all"), str(seq["tmp"] / "sink_png")
    pmctf_access.pmctf_gop.decode_sequence_checked(net, bins, None, "cuda", png_out=all_png)
    d = pmctf_access.decode_frames(net, bins, None, [1, 6], png_out=png)
    assert sorted(os.listdir(png)) == ["1.png", "6.png"] and d["times"] == [1, 6] and d["gops_opened"] == 2
    for name in ("1.png", "6.png"):
        assert open(os.path.join(png, name), "rb").read() == open(os.path.join(all_png, name), "rb").read()


# --------------------------------------------------------------------------------------------------------- 9. read_frames
def test_read_frames_stay_on_the_device(seq):
    import pmctf_access
    import pmctf_gop
    net = seq["dec_net"]
    got = pmctf_access.read_frames(net, seq["eight"], [1, 6], "cuda", verify=True)
    assert [t for t, _ in got] == [1, 6]
    want = pmctf_gop.PlainSink(H, W, 8).frames([seq["full8"]["frames"][t] for t in (1, 6)])
    for (t, a), b in zip(got, want):
        assert a.is_cuda and a.dtype == torch.uint8 and a.shape == (N8,), t
        assert torch.equal(a, b), t
    full = np.fromfile(seq["yuv7"], dtype=np.uint8)
    got = pmctf_access.read_frames(net, seq["seven"], (3, 7))
    assert [t for t, _ in got] == [3, 4, 5, 6]
    for t, a in got:
        assert a.is_cuda and np.array_equal(a.cpu().numpy(), full[t * N8:(t + 1) * N8]), t
    assert not [n for n in os.listdir(seq["seven"]) if n.endswith((".yuv", ".png"))], "nothing is written"


# --------------------------------------------------------------------------------------------------------- 10. the tool
def test_tool(seq, capsys):
    import pmctf_access
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("decode_sequence", os.path.join(root, "tools", "decode_sequence.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    yuv = str(seq["tmp"] / "tool_2_6.yuv")
    capsys.readouterr()
    tool.main(["--synth-seed", "0", "--frames", "2:6", "--verify", seq["seven"], yuv])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert np.array_equal(np.fromfile(yuv, dtype=np.uint8), _pictures(seq["yuv7"], [2, 3, 4, 5]))
    assert (out["frames"], out["verified"], out["hash_mismatches"], out["gops_opened"]) == (4, 4, 0, 2)
    assert out["frames_wanted"] == [2, 3, 4, 5] and out["bytes_read"] == pmctf_access.access_bytes(seq["seven"], range(2, 6))
    assert (out["height"], out["width"], out["bitdepth"], out["spatial_level"]) == (H, W, 8, 0)
    png = str(seq["tmp"] / "tool_png")
    tool.main(["--synth-seed", "0", "--frames", "6,0", "--png", png, seq["seven"]])
    assert sorted(os.listdir(png)) == ["0.png", "6.png"]
