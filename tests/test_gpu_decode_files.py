"""The standalone decoder on the GPU: the batched sequential LL decode (pmctf_ll_ar_decode_batch_f32) against the CPU, the
output conversion kernel (pmctf_planes_to_u8), and pmctf_gop.decode_gop_files / decode_sequence on files of the fast
path (skip_decoding=True: chroma's LL symbols plane after plane), on decoder-order files and on files the real reference
wrote.  Expectations come from the oracle, the host range coder, the encoder's own returned tensors or the reference's
fixtures — never from the decoder alone.  Bit-exact unless a bound is stated."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest
import torch

import ll_decode_helper as hp
from helpers import assert_same, frames, golden, golden_448, product_model
from ll_decode_helper import BLOCKS, CHAIN

pytestmark = pytest.mark.gpu

WSETS = ["s0", "s1", "lo", "hi", "m+", "m-"]        # s0 / s1: two coders' weights (an H file's and an L file's) in one batch
HEADS = [CHAIN, 16, 32, 48, 64, 80, 96, 112]
OUTS = [CHAIN, 16, 64, 112]
# (order, P, H, W, jobs, index of the job whose stream is cut in half or None).  With the gauss table's 103 CDF columns the
# two-plane kernels are the two-half form up to W = 88, one thread per channel for 89..344 and do not fit LDS from 345
# (test_gpu_ll_decode.py); in plane order the single-plane kernels decode two-plane streams of any of these widths.
BATCHES = [("position", 1, 1, 9, 1, None), ("position", 1, 3, 7, 2, None), ("position", 1, 4, 8, 5, 3),
           ("position", 1, 6, 13, 16, None),
           ("position", 2, 2, 88, 2, None), ("position", 2, 2, 89, 5, None), ("position", 2, 2, 344, 1, None),
           ("position", 2, 3, 9, 16, 7),
           ("plane", 2, 2, 88, 2, None), ("plane", 2, 2, 89, 1, None), ("plane", 2, 2, 344, 2, None),
           ("plane", 2, 2, 345, 5, 1), ("plane", 2, 3, 9, 16, None), ("plane", 1, 4, 8, 2, None)]


def _plane_major(c, P, tables, lead, trail):
    """the same oracle symbols and CDF rows pushed plane after plane through the host coder (what the one-shot order of
    pwave_compress(ar_order=False) writes), and what a host decoder reports around them"""
    from pMCTF.hip.engine import HostDecoder
    s = np.ascontiguousarray(c["sym"].reshape(-1, P).T).reshape(-1)
    i = np.ascontiguousarray(c["idx"].reshape(-1, P).T).reshape(-1)
    stream = hp.encode(tables, [lead, (s, i), trail])
    dec = HostDecoder({"gauss": tables}, stream)
    assert np.array_equal(dec.decode(lead[1], "gauss"), lead[0])
    x0, pos0 = dec.get_state()
    assert np.array_equal(dec.decode(i, "gauss"), s)
    x1, pos1 = dec.get_state()
    assert np.array_equal(dec.decode(trail[1], "gauss"), trail[0])
    return dict(c, stream=stream, words=dec.words.copy(), x0=x0, pos0=pos0, x1=x1, pos1=pos1)


@pytest.fixture(scope="module")
def batches():
    """every batch's jobs, built on the CPU: oracle parameters under the job's rules, host coder, host decoder"""
    sets = hp.weight_sets()
    planes = hp.ll_planes()
    tabs = tuple(np.ascontiguousarray(a, dtype=np.int32) for a in sets["s0"].tables.cdf_info())
    g = sets["s0"].tables
    packed = {k: hp.pack_weights(o.sd) for k, o in sets.items()}
    out = []
    for b, (order, P, H, W, J, cut) in enumerate(BATCHES):
        jobs = []
        for j in range(J):
            ws = WSETS[(b + j) % len(WSETS)]
            rules = (BLOCKS, HEADS[(b + 3 * j) % 8], OUTS[(b + j) % 4])
            ll = hp.ll_for(planes, P, H, W, 1000 + 37 * b + j)
            lead = hp.side_symbols(3000 + 100 * b + j, 4 + 7 * ((j * 5 + b) % 9), tabs)     # entry states differ per job
            trail = hp.side_symbols(5000 + 100 * b + j, 24 + 5 * (j % 4), tabs)
            c = hp.make_case(sets[ws], rules, ll, lead, trail)
            if order == "plane" and P > 1:
                c = _plane_major(c, P, tabs, lead, trail)
            n_words = c["words"].size
            if j == cut:
                n_words = (c["pos0"] + c["pos1"]) // 2
                assert c["pos1"] - n_words >= 2, "the cut must fall inside the LL"
            c.update(ws=ws, rules=rules, trail=trail, n_words=n_words, trunc=j == cut)
            jobs.append(c)
        out.append({"order": order, "P": P, "H": H, "W": W, "jobs": jobs})
    return {"batches": out, "tabs": tabs, "packed": packed, "lmin": float(g.log_scale_min), "lstep": float(g.log_scale_step)}


def _run_batch(dev, b, tabs_dev, wdev, lmin, lstep):
    """one call of pmctf_ll_ar_decode_batch_f32 with a hand-built job table; -> (rc, ll [J][P][H][W], state [J][3])"""
    from pMCTF.hip import lib
    from pMCTF.hip.engine import HipEngine
    L = lib.hip()
    P, H, W, jobs = b["P"], b["H"], b["W"], b["jobs"]
    J = len(jobs)
    cdf, sizes, offs = tabs_dev
    ll = torch.full((J, P, H, W), float("nan"), dtype=torch.float32, device=dev)            # every position must be written
    scratch = torch.zeros((J, L.pmctf_ll_ar_scratch_floats(P, H, W)), dtype=torch.float32, device=dev)
    host_state = np.array([[c["x0"], c["pos0"], 0] for c in jobs], dtype=np.uint64)
    state = torch.from_numpy(host_state.view(np.int64)).to(dev)
    words = [torch.from_numpy(np.ascontiguousarray(c["words"][:max(c["n_words"], 1)])).to(dev) for c in jobs]
    table = np.zeros(J, HipEngine.LL_JOB)
    for j, c in enumerate(jobs):
        table[j] = (wdev[c["ws"]].data_ptr(), words[j].data_ptr(), c["n_words"], state[j].data_ptr(), ll[j].data_ptr(),
                    scratch[j].data_ptr(), c["rules"], 0)
    tdev = torch.from_numpy(table.view(np.uint8)).to(dev)
    vp = lambda t: C.c_void_p(t.data_ptr())
    st = torch.cuda.current_stream(dev)
    rc = L.pmctf_ll_ar_decode_batch_f32(vp(tdev), J, vp(cdf), vp(sizes), vp(offs), cdf.shape[1], lmin, lstep, P, H, W,
                                        HipEngine.LL_ORDERS[b["order"]], C.c_void_p(st.cuda_stream))
    st.synchronize()
    return rc, ll.cpu().numpy(), state.cpu().numpy().view(np.uint64)


def test_batched_ll_decode_against_the_cpu(cuda, batches):
    """per job of every batch: ll_out = the oracle's ll_hat, exit state = the host decoder's, and a host decoder restarted
    from it decodes the trailing run; a job whose stream is cut in half raises its own flag only"""
    from pMCTF.hip.engine import HipEngine, HostDecoder
    tabs = batches["tabs"]
    cols = tabs[0].shape[1]
    tabs_dev = tuple(torch.from_numpy(a).to(cuda) for a in tabs)
    wdev = {k: torch.from_numpy(v).to(cuda) for k, v in batches["packed"].items()}
    bad, forms, sizes, cuts = [], set(), set(), 0
    for b in batches["batches"]:
        form = HipEngine.ll_batch_form(b["P"], b["W"], cols, b["order"], BLOCKS)
        assert form in (1, 2), f"{b['order']} P={b['P']} W={b['W']}: the batched form must cover this case"
        forms.add((b["order"], b["P"], form))
        sizes.add(len(b["jobs"]))
        assert len({(c["x0"], c["pos0"]) for c in b["jobs"]}) == len(b["jobs"]), "entry states must differ"
        rc, ll, st = _run_batch(cuda, b, tabs_dev, wdev, batches["lmin"], batches["lstep"])
        assert rc == 0, f"batch {b['order']} P={b['P']} H={b['H']} W={b['W']}: status {rc}"
        for j, c in enumerate(b["jobs"]):
            what = f"{b['order']} P={b['P']} H={b['H']} W={b['W']} J={len(b['jobs'])} job {j} ({c['ws']}, {c['rules']})"
            if c["trunc"]:
                cuts += 1
                if int(st[j][2]) != 1 or not np.isfinite(ll[j]).all():
                    bad.append(f"{what}: truncated, flag {int(st[j][2])}, finite {bool(np.isfinite(ll[j]).all())}")
                continue
            if not np.array_equal(ll[j], c["ll_hat"]):
                neq = np.argwhere(~(ll[j] == c["ll_hat"]))
                f = tuple(neq[0])
                bad.append(f"{what}: {len(neq)} of {ll[j].size} values differ, first at {f}: {ll[j][f]!r} vs {c['ll_hat'][f]!r}")
                continue
            if (int(st[j][0]), int(st[j][1]), int(st[j][2])) != (c["x1"], c["pos1"], 0):
                bad.append(f"{what}: state {[int(v) for v in st[j]]} vs host decoder {[c['x1'], c['pos1'], 0]}")
                continue
            dec = HostDecoder({"gauss": tabs}, c["stream"])
            dec.set_state(int(st[j][0]), int(st[j][1]))
            if not np.array_equal(dec.decode(c["trail"][1], "gauss"), c["trail"][0]):
                bad.append(f"{what}: the symbols after the LL do not decode from the kernel's state")
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:20])
    assert sizes >= {1, 2, 5, 16} and cuts == 3
    assert forms >= {("position", 1, 2), ("position", 2, 2), ("position", 2, 1), ("plane", 2, 2)}, forms
    # outside the batched form the entry refuses (two planes in position order too wide for LDS; three planes; 33 jobs)
    from pMCTF.hip import lib
    L = lib.hip()
    assert HipEngine.ll_batch_form(2, 345, cols, "position") == 0 and HipEngine.ll_batch_form(3, 8, cols, "plane") == 0
    vp = lambda t: C.c_void_p(t.data_ptr())
    dummy = torch.zeros(64 * 33, dtype=torch.uint8, device=cuda)
    args = (vp(tabs_dev[0]), vp(tabs_dev[1]), vp(tabs_dev[2]), cols, batches["lmin"], batches["lstep"])
    assert L.pmctf_ll_ar_decode_batch_f32(vp(dummy), 1, *args, 2, 2, 345, 0, None) == -1
    assert L.pmctf_ll_ar_decode_batch_f32(vp(dummy), 1, *args, 3, 2, 8, 1, None) == -1
    assert L.pmctf_ll_ar_decode_batch_f32(vp(dummy), 33, *args, 1, 2, 8, 0, None) == -1


def test_single_job_entry_equals_a_batch_of_one(cuda, batches):
    from pMCTF.hip import lib
    L = lib.hip()
    tabs_dev = tuple(torch.from_numpy(a).to(cuda) for a in batches["tabs"])
    wdev = {k: torch.from_numpy(v).to(cuda) for k, v in batches["packed"].items()}
    n = 0
    for b in batches["batches"]:
        if b["P"] != 1:
            continue
        for c in b["jobs"][:3]:
            one = dict(b, jobs=[c])
            rc, ll_b, st_b = _run_batch(cuda, one, tabs_dev, wdev, batches["lmin"], batches["lstep"])
            assert rc == 0
            ll_s, st_s = hp.run_case(L, lib, wdev[c["ws"]], c["words"], c["n_words"], c["x0"], c["pos0"], tabs_dev,
                                     batches["lmin"], batches["lstep"], 1, b["H"], b["W"], c["rules"])
            assert np.array_equal(ll_b[0], ll_s, equal_nan=True) and np.array_equal(st_b[0], st_s), (b["H"], b["W"], c["ws"])
            assert int(st_s[2]) == int(c["trunc"])
            n += 1
    assert n >= 6


# ------------------------------------------------------------------------------------------------ files of a GOP
def _compare_with_encoder(gop, enc, out, what):
    import pmctf_gop
    coded = out["frames_coded"]
    pairs = pmctf_gop.gop_pairs(gop)
    assert len(pairs) == len(enc["results"])
    for (stage, i_ref, i_cur), r in zip(pairs, enc["results"]):
        for k, got in (("H_t", coded[i_cur][0]), ("H_tc", coded[i_cur][1]), ("mv_hat", coded[i_cur][2])):
            assert_same(got, r[k], f"{what}: pair ({i_ref}, {i_cur}) stage {stage} {k}")
    last = enc["results"][-1]
    assert_same(coded[0][0], last["L_t"], f"{what}: L_t")
    assert_same(coded[0][1], last["L_tc"], f"{what}: L_tc")
    assert coded[0][2] is None


@pytest.mark.parametrize("w,h,gop,stages", [(128, 128, 4, 1), (448, 256, 8, 2)])
@pytest.mark.parametrize("skip_decoding,ll_order", [(True, "plane"), (False, "position")])
def test_gop_files_decode_in_a_fresh_model(cuda, tmp_path, w, h, gop, stages, skip_decoding, ll_order):
    """encode_gop writes a folder; a NEW model object with the same weights decodes it with nothing else from the encoder.
    skip_decoding=True files carry chroma's LL plane after plane: no decoder could read them before."""
    import pmctf_gop
    enc_net, _ = product_model(stages)
    fr = frames(w, h, gop, device="cuda")
    enc = pmctf_gop.encode_gop(enc_net, fr, h, w, 3, str(tmp_path), skip_decoding=skip_decoding)
    assert sorted(os.listdir(tmp_path)) == sorted(pmctf_gop.gop_file_names(gop))
    dec_net, _ = product_model(stages)
    assert dec_net is not enc_net and dec_net.engine() is not enc_net.engine()
    out = pmctf_gop.decode_gop_files(dec_net, str(tmp_path), gop, h, w, 3, ll_order=ll_order)
    _compare_with_encoder(gop, enc, out, f"{w}x{h} GOP {gop} {ll_order}")
    rec = pmctf_gop.decode_gop(enc_net, enc["frames_coded"])
    for i in range(gop):
        assert_same(out["frames"][i][0], rec[i][0], f"frame {i} luma")
        assert_same(out["frames"][i][1], rec[i][1], f"frame {i} chroma")
    # every picture file of this GOP went through the batched launches
    eng = dec_net.engine()
    cols = eng.tables["gauss"][0].shape[1]
    pad_h, pad_w = -(-h // 128) * 128, -(-w // 128) * 128
    for P, sw in ((1, pad_w >> 4), (2, pad_w >> 5)):
        assert eng.ll_batch_form(P, sw, cols, ll_order) in (1, 2)


def test_gop_decode_reports_the_path_and_damaged_files(cuda, tmp_path):
    import pmctf_gop
    net, _ = product_model(1)
    fr = frames(128, 128, 2, device="cuda")
    pmctf_gop.encode_gop(net, fr, 128, 128, 3, str(tmp_path))
    dec, _ = product_model(1)
    files = []
    for name, chroma, low in (("1.bin", False, False), ("1_C_main.bin", True, False), ("0_main.bin", False, True),
                              ("0_C_main.bin", True, True)):
        files.append((open(tmp_path / name, "rb").read(), chroma, low, 0))
    begun, _ = dec._decompress_gop_files_begin(files, 128, 3, "plane")
    assert [b["ticket"]["path"] for b in begun] == ["batched"] * 4
    assert len({id(b["ticket"]["stream"]) for b in begun}) == 2           # one stream per geometry
    dec._decompress_gop_files_end((begun, None))
    good = open(tmp_path / "1_C_main.bin", "rb").read()
    for damage, what in ((good[:len(good) // 2], "truncated"), (good + b"\0\0", "surplus"), (None, "missing")):
        if damage is None:
            os.remove(tmp_path / "1_C_main.bin")
        else:
            open(tmp_path / "1_C_main.bin", "wb").write(damage)
        with pytest.raises(ValueError, match=rf"1_C_main\.bin: .*{what}"):
            pmctf_gop.decode_gop_files(dec, str(tmp_path), 2, 128, 128, 3)
    open(tmp_path / "1_C_main.bin", "wb").write(good)
    ref = pmctf_gop.decode_gop_files(dec, str(tmp_path), 2, 128, 128, 3)    # and the decoder still works afterwards
    # a stream cut short behind a header that was adjusted to it: as for every corrupt stream here
    # (test_corrupt_streams_fail_cleanly) an exception — which names the file — or finite, wrong pixels, never the intact
    # picture; the host range decoder stops refilling at the end of its words and does not report it
    n = struct.unpack(">I", good[12:16])[0]
    keep = n // 2 // 4 * 4 + 1
    open(tmp_path / "1_C_main.bin", "wb").write(good[:12] + struct.pack(">I", keep) + good[16:16 + keep])
    try:
        out = pmctf_gop.decode_gop_files(dec, str(tmp_path), 2, 128, 128, 3)
        got, want = out["frames_coded"][1][1], ref["frames_coded"][1][1]
        assert torch.isfinite(got).all() and not torch.equal(got, want)
    except ValueError as e:
        assert "1_C_main.bin" in str(e)


def _write_file_set(g, prefix, folder):
    names = {}
    for k in g.files:
        m = re.fullmatch(rf"{re.escape(prefix)}(?:pair\d+\.)?file\.(.+)", k)
        if m:
            data = g[k].tobytes()
            assert names.setdefault(m.group(1), data) == data, f"{m.group(1)}: listings of later pairs repeat earlier files"
    for name, data in names.items():
        open(os.path.join(folder, name), "wb").write(data)
    return sorted(names)


@pytest.mark.parametrize("w,h", [(128, 128), (448, 256)])
def test_gop4_files_of_the_reference_decode(cuda, tmp_path, w, h):
    """The GOP-4 file sets the real reference wrote with skip_decoding=True (chroma LL plane-major: nothing could decode
    them so far): per-frame PSNR of the decoded pictures against the reference's own figures within 1e-4 dB; at 128x128
    (where the product's files are asserted byte-identical to these) every decoded tensor equals the product encoder's."""
    import pmctf_gop
    g = golden() if w == 128 else golden_448()
    assert _write_file_set(g, "gop.", str(tmp_path)) == sorted(pmctf_gop.gop_file_names(4))
    net, _ = product_model(1)
    fr = frames(w, h, 4, device="cuda")
    out = pmctf_gop.decode_gop_files(net, str(tmp_path), 4, h, w, 3, ll_order="plane")
    ps = pmctf_gop.gop_psnr(out["frames"], fr, h, w)
    err = np.abs(np.array([p["yuv"] for p in ps]) - g["gop.psnr_yuv"])
    print(f"\n{w}x{h}: per-frame |PSNR - reference's| = {err.tolist()}")
    assert err.max() < 1e-4
    if w == 128:
        enc_net, _ = product_model(1)
        own = tmp_path / "own"
        own.mkdir()
        enc = pmctf_gop.encode_gop(enc_net, fr, h, w, 3, str(own))
        _compare_with_encoder(4, enc, out, "reference files 128x128")


def test_decoder_order_files_of_the_reference_decode(cuda, tmp_path):
    """dec.file.*: one pair the reference wrote with skip_decoding=False (position-major), against the tensors its own
    decoder returned, at the 2e-3 absolute test_decoder_round_trip_and_oracle uses"""
    import pmctf_gop
    g = golden()
    assert _write_file_set(g, "dec.", str(tmp_path)) == sorted(pmctf_gop.gop_file_names(2))
    net, _ = product_model(1)
    out = pmctf_gop.decode_gop_files(net, str(tmp_path), 2, 128, 128, 3, ll_order="position")
    coded = out["frames_coded"]
    for k, got in (("H_t", coded[1][0]), ("H_tc", coded[1][1]), ("mv_hat", coded[1][2]), ("L_t", coded[0][0]),
                   ("L_tc", coded[0][1])):
        want = g[f"dec.{k}"]
        assert tuple(got.shape) == want.shape, k
        d = np.abs(got.cpu().numpy() - want).max()
        print(f"dec.{k}: max abs difference {d:.3e}")
        assert d < 2e-3, k


def test_the_order_argument_is_live_on_chroma(cuda, tmp_path):
    """a plane-major chroma file read position-major must not silently give the right planes"""
    net, _ = product_model(1)
    net.engine().keep_streams = True
    fr = frames(128, 128, 2, device="cuda")
    r = net.encode_one_stage(fr[0], fr[1], True, {"mv_feature": None, "ref_mv_y": None},
                             output_path=str(tmp_path / "1.bin"), pic_width=128, pic_height=128, skip_decoding=True,
                             stage_idx=0, q_index=3)
    data = open(tmp_path / "1_C_main.bin", "rb").read()
    assert data == r["files"]["Hc"] == golden()["gop.pair0.file.1_C_main.bin"].tobytes()
    sym = np.asarray(r["traces"]["Hc"][0])
    n = (128 // 2 // 16) ** 2                      # chroma's LL plane: 64x64 four levels down
    assert not np.array_equal(sym[:n], sym[n:2 * n]), "premise: Cb's and Cr's LL symbols differ (host check)"
    dec, _ = product_model(1)
    right = dec.decompress_gop_files([(data, True, False, 0)], 128, 3, "plane")[0]
    assert_same(right, r["H_tc"], "plane order")
    try:
        wrong = dec.decompress_gop_files([(data, True, False, 0)], 128, 3, "position")[0]
    except ValueError:
        return
    assert not torch.equal(wrong, right)


# ------------------------------------------------------------------------------------------------ output stage
@pytest.mark.parametrize("N,Hp,Wp,h,w", [(1, 1088, 1920, 1080, 1920), (2, 544, 960, 540, 959), (1, 128, 256, 100, 134),
                                         (2, 64, 128, 50, 67), (3, 8, 8, 5, 1), (1, 4, 4, 4, 4)])
def test_planes_to_u8(cuda, N, Hp, Wp, h, w):
    from pMCTF.hip import ops
    g = torch.Generator().manual_seed(N * 1000 + w)
    x = (torch.rand((N, 1, Hp, Wp), generator=g) * 300.0 - 20.0)
    special = torch.cat([torch.arange(256, dtype=torch.float32) + 0.5, torch.tensor([-0.0, 0.0, -0.5, -1e-30, -3.0, -1e9,
                        255.0, 255.4999, 255.5, 256.0, 1e9, 0.49999997, 1.5, 2.5, 254.5, float("inf"), -float("inf")])])
    k = min(special.numel(), w)                    # the constructed values go where the crop keeps them: the first rows
    for i in range(0, special.numel(), k):
        row = i // k
        if row < h:
            x[0, 0, row, :min(k, special.numel() - i)] = special[i:i + k]
    want = torch.round(x.clamp(0, 255))[..., :h, :w].to(torch.uint8)[:, 0]
    got = ops.planes_to_u8(x.to(cuda), h, w)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (N, h, w)
    assert torch.equal(got.cpu(), want)
    if w >= 256:
        assert {0, 2, 4, 254, 255} <= set(want[0, 0, :256].tolist()) and 1 not in want[0, 0, :2].tolist()   # ties to even


# ------------------------------------------------------------------------------------------------ sequence
def test_sequence_round_trip(cuda, tmp_path):
    import json
    import pmctf_gop
    import pmctf_synth
    from pMCTF.utils.yuv_reader import YUVReader
    w, h, gop, n = 132, 100, 4, 8                    # padded to 256x128; chroma rows of 66 bytes (w % 4 = 2)
    src = str(tmp_path / "src.yuv")
    pmctf_gop.write_yuv(src, pmctf_synth.synth_yuv420(w, h, n, seed=5))
    bins = str(tmp_path / "bins")
    os.makedirs(bins)
    enc_net, _ = product_model(1)
    enc = pmctf_gop.encode_sequence(enc_net, src, w, h, n, gop, 3, bins, "cuda", keep_gops=True)
    assert sorted(os.listdir(bins)) == ["gop_00000", "gop_00001", "sequence.json"]
    for k in range(2):
        assert sorted(os.listdir(os.path.join(bins, f"gop_{k:05d}"))) == sorted(pmctf_gop.gop_file_names(gop))
    header = pmctf_gop.read_sequence_header(bins)
    assert (header["ll_order"], header["gop"], header["frame_num"], header["width"], header["height"]) == ("plane", gop, n, w, h)

    # what the encoder side reconstructs, rounded and cropped with torch
    want = b""
    reader = YUVReader(src, w, h)
    with torch.no_grad():
        for k in range(n // gop):
            padded, orig, _ = pmctf_gop.read_gop(reader, gop, "cuda")
            e = pmctf_gop.encode_gop(enc_net, padded, h, w, 3, os.path.join(bins, f"gop_{k:05d}"))
            for ry, rc, _ in pmctf_gop.decode_gop(enc_net, e["frames_coded"]):
                y8 = torch.round(ry.clamp(0, 255))[..., :h, :w].to(torch.uint8).cpu().numpy()
                c8 = torch.round(rc.clamp(0, 255))[..., :h // 2, :w // 2].to(torch.uint8).cpu().numpy()
                want += y8[0, 0].tobytes() + c8[0, 0].tobytes() + c8[1, 0].tobytes()
    reader.close()

    dec_net, _ = product_model(1)
    out_yuv = str(tmp_path / "dec.yuv")
    res = pmctf_gop.decode_sequence(dec_net, bins, out_yuv, "cuda")
    assert res["frames"] == [(h, w)] * n and len(res["seconds"]) == n // gop
    got = open(out_yuv, "rb").read()
    assert len(got) == n * (w * h + 2 * (w // 2) * (h // 2))
    assert got == want, "decoded .yuv differs from the encoder side's rounded reconstruction"

    # PSNR recomputed from the decoded file equals encode_sequence's table
    ro, rd = YUVReader(src, w, h), YUVReader(out_yuv, w, h)
    psnr = []
    for k in range(n // gop):
        _, orig, _ = pmctf_gop.read_gop(ro, gop, "cuda")
        _, dec, _ = pmctf_gop.read_gop(rd, gop, "cuda")
        psnr += [p["yuv"] for p in pmctf_gop.gop_psnr([(y, c, None) for y, c in dec], orig, h, w)]
    ro.close(); rd.close()
    assert np.abs(np.array(psnr) - np.array(enc["psnr"])).max() <= 1e-9

    # a header that names another thread setting or profile is refused
    path = os.path.join(bins, "sequence.json")
    good = json.load(open(path))
    for k, v in (("aten_threads", good["aten_threads"] + 1), ("precision", "f32-chain"), ("num_me_stages", 2)):
        json.dump(dict(good, **{k: v}), open(path, "w"))
        with pytest.raises(ValueError, match=k):
            pmctf_gop.decode_sequence(dec_net, bins, str(tmp_path / "no.yuv"), "cuda")


# ------------------------------------------------------------------------------------------------ fallback
def test_three_planes_take_the_per_file_path(cuda, tmp_path):
    """an RGB still (three planes in one stream) is outside the batched form: per-file launches, today's result — in the
    decoder's order and, plane after plane with the state read back in between, in the one-shot order"""
    net, _ = product_model(1)
    coder = net.lp_coder
    img = frames(128, 128, 1)[0][0]
    rgb = torch.cat([img, img.flip(2), img.flip(3)], dim=1).cuda()
    fn = str(tmp_path / "img.bin")
    eng = coder.engine()
    for skip, order in ((False, "position"), (True, "plane")):
        x3 = coder.compress(rgb, [1, 3, 128, 128], fn, q_index=7, skip_decoding=skip)
        data = open(fn, "rb").read()
        assert eng.ll_batch_form(3, 8, eng.tables["gauss"][0].shape[1], order) == 0
        begun = eng.pwave_decompress_batch_begin([("coder", data, 64, 7, None)], order)
        assert begun[0]["ticket"]["path"] == "per-file"
        got = eng.pwave_decompress_batch_end(begun)[0]
        assert_same(torch.cat([got[c:c + 1] for c in range(3)], dim=1), x3, f"RGB still, {order} order")
        if not skip:
            assert_same(coder.decompress(fn, padding=64, q_index=7)["x_hat"], x3, "pWave.decompress")
