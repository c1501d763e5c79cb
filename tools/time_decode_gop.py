#!/usr/bin/env python3
"""Times the decode of one GOP from its files two ways, in one process after warm-up, and writes
profiles/decode_gop_files.json:

  (a) the per-pair schedule that existed before decode_gop_files: per pair in coding order the picture files through
      _decompress_files_begin / _decompress_files_end (per-file LL launches on side streams) with decompress_mv under
      them, then the temporal synthesis;
  (b) pmctf_gop.decode_gop_files: every picture file of the GOP in one batch.

Both read the SAME folder, written once with skip_decoding=False (decoder order, ll_order="position"): the only kind of
chroma file (a) can read.  (b) is timed again on the skip_decoding=True files in "plane" order (no figure of (a) exists
for those) and with other numbers of finishing threads (--workers), and the batched LL series is timed alone.  Medians of --reps timed
repetitions after --warmup untimed ones; min and max are the run-to-run spread.

    python tools/time_decode_gop.py [--width 1920 --height 1080 --gop 16 --q_index 3 --reps 5 --warmup 2]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learned-pmctf_amd"))
import torch  # noqa: E402

import pmctf_gop  # noqa: E402
import pmctf_synth  # noqa: E402
from pMCTF.models.video.pMCTF_L import pMCTF  # noqa: E402
from pMCTF.utils.stream_helper import decode_p  # noqa: E402


def model(stages):
    net = pMCTF(num_me_stages=stages).eval()
    net.load_state_dict(pmctf_synth.synth_state_dict(net.state_dict(), seed=0), strict=True)
    net = net.cuda()
    net.update(force=True)
    net.lazy_stages = False
    return net


def per_pair_schedule(net, folder, gop, h, w, q_index, psize=128):
    """schedule (a): what encode_one_stage(skip_decoding=False) does after writing a pair's files, pair after pair"""
    pad_h, pad_w = -(-h // psize) * psize, -(-w // psize) * psize
    coded = [[None, None, None] for _ in range(gop)]
    pairs = pmctf_gop.gop_pairs(gop)
    stages = pairs[-1][0] + 1
    dpb, at = None, None
    for stage, i_ref, i_cur in pairs:
        if stage != at:
            dpb, at = {"mv_feature": None, "ref_mv_y": None}, stage
        me_num = min(net.num_me_stages - 1, stage)
        code_lt = stage + 1 == stages
        path = os.path.join(folder, f"{i_cur}.bin")
        _, string = decode_p(path.replace(".bin", "_mv.bin"))
        begun = net._decompress_files_begin([(path, False), (path.replace(".bin", "_C_main.bin"), True)], code_lt, psize,
                                            q_index, me_num)
        d = net.decompress_mv(string, torch.float32, pad_h, pad_w, dpb, stage_idx=me_num, q_index=q_index)
        dpb = {"mv_feature": d["mv_feature"], "ref_mv_y": d["mv_y_hat"]}
        luma, chroma = net._decompress_files_end(begun)
        coded[i_cur] = [luma["H_t"]["x_hat"], chroma["H_t"]["x_hat"], d["mv_hat"]]
        if code_lt:
            coded[i_ref] = [luma["L_t"]["x_hat"], chroma["L_t"]["x_hat"], None]
    return pmctf_gop.decode_gop(net, coded)


def timed(fn, reps, warmup):
    out = None
    for _ in range(warmup):
        out = fn()
        torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return out, {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "reps": ts}


def ll_series(net, folder, names, coder, psize, q_index, order, reps, warmup):
    """the batched LL launches of the named files alone (upload of the words and the job table included)"""
    eng = net.engine()
    jobs = [(coder, open(os.path.join(folder, n), "rb").read(), psize, q_index, None) for n in names]

    def run():
        begun = eng.pwave_decompress_batch_begin(jobs, order)
        assert all(b["ticket"]["path"] == "batched" for b in begun)
        return begun
    begun, t = timed(run, reps, warmup)
    P = begun[0]["N"]
    sh, sw = begun[0]["shape"][2:]
    t.update(jobs=len(jobs), planes=P, ll_h=sh, ll_w=sw,
             us_per_position=t["median_s"] * 1e6 / (sh * sw * (P if order == "plane" else 1)))
    del t["reps"]
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--gop", type=int, default=16)
    ap.add_argument("--q_index", type=int, default=3)
    ap.add_argument("--stages", type=int, default=4, help="num_me_stages of the model")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workers", type=lambda v: [int(x) for x in v.split(",")], default=[2, 4, 8, 16],
                    help="finishing-thread counts (b) is timed with besides the engine's default")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_gop_files.json"))
    a = ap.parse_args()
    assert a.reps >= 5 and a.warmup >= 2, "at least 5 timed repetitions after 2 warm-ups"
    W, H, G, q = a.width, a.height, a.gop, a.q_index
    frames = [list(pmctf_synth.frames_to_tensors(f, device="cuda")) for f in pmctf_synth.synth_yuv420(W, H, G)]
    enc = model(a.stages)
    pos_dir, plane_dir = tempfile.mkdtemp(prefix="pos_"), tempfile.mkdtemp(prefix="plane_")
    with torch.no_grad():
        pmctf_gop.encode_gop(enc, frames, H, W, q, pos_dir, skip_decoding=False)
        e = pmctf_gop.encode_gop(enc, frames, H, W, q, plane_dir, skip_decoding=True)
        want = pmctf_gop.decode_gop(enc, e["frames_coded"])
        want = [(y.clone(), c.clone()) for y, c, _ in want]
    del enc, e, frames
    torch.cuda.empty_cache()
    dec = model(a.stages)
    eng = dec.engine()
    rec = {"what": "decode of one GOP from files, seconds", "width": W, "height": H, "gop": G, "q_index": q,
           "num_me_stages": a.stages, "timed_reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        ra, rec["a_per_pair"] = timed(lambda: per_pair_schedule(dec, pos_dir, G, H, W, q), a.reps, a.warmup)
        rb, rec["b_gop_files"] = timed(lambda: pmctf_gop.decode_gop_files(dec, pos_dir, G, H, W, q, ll_order="position")["frames"],
                                       a.reps, a.warmup)
        rp, rec["b_gop_files_plane_order"] = timed(
            lambda: pmctf_gop.decode_gop_files(dec, plane_dir, G, H, W, q, ll_order="plane")["frames"], a.reps, a.warmup)
        default_workers = eng.decode_workers
        rec["decode_workers"] = default_workers
        rec["b_gop_files_by_threads"] = {}
        for n in a.workers:
            eng.decode_workers = n
            _, rec["b_gop_files_by_threads"][str(n)] = timed(
                lambda: pmctf_gop.decode_gop_files(dec, pos_dir, G, H, W, q, ll_order="position")["frames"], a.reps, 1)
        eng.decode_workers = default_workers
        same = all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(ra, rb))
        same_plane = all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(rp, want))
        rec["a_equals_b"] = bool(same)
        rec["plane_order_equals_encoder_side"] = bool(same_plane)
        pairs = pmctf_gop.gop_pairs(G)
        luma = [f"{c}.bin" for _, _, c in pairs]
        chroma = [f"{c}_C_main.bin" for _, _, c in pairs]
        rec["ll_series"] = {
            "luma_1_job": ll_series(dec, pos_dir, luma[:1], "hp_coder", 128, q, "position", a.reps, a.warmup),
            f"luma_{len(luma)}_jobs": ll_series(dec, pos_dir, luma, "hp_coder", 128, q, "position", a.reps, a.warmup),
            f"chroma_{len(chroma)}_jobs_position": ll_series(dec, pos_dir, chroma, "hp_coder", 64, q, "position", a.reps, a.warmup),
            f"chroma_{len(chroma)}_jobs_plane": ll_series(dec, plane_dir, chroma, "hp_coder", 64, q, "plane", a.reps, a.warmup),
        }
    rec["ratio_a_over_b"] = rec["a_per_pair"]["median_s"] / rec["b_gop_files"]["median_s"]
    rec["b_not_slower_beyond_spread"] = bool(rec["b_gop_files"]["median_s"] <= rec["a_per_pair"]["max_s"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=2)
        f.write("\n")
    print(json.dumps({k: (v if not isinstance(v, dict) or "reps" not in v else {x: y for x, y in v.items() if x != "reps"})
                      for k, v in rec.items()}, indent=1))
    if not (same and same_plane):
        sys.exit("the schedules do not reconstruct the same pictures")


if __name__ == "__main__":
    main()
