#!/usr/bin/env python3
"""Times the decode of a sequence at its temporal levels (pmctf_layers.decode_sequence_layer) and writes
profiles/temporal_layers.json: a 1920x1080 folder of one GOP of 16 at q_index 3, synthetic weights; for the levels 0..4
and for level 1 with motion_fill the bytes read and the wall time of the decode to a .yuv file (the host clock between
two device synchronisations: file reads, entropy decode, synthesis, conversion and the write), the median of --reps runs
after one warm-up.

Every GPU step is a process of its own under `timeout`: the encode of the folder, then one process per row.  The first
step that fails ends the run; nothing is started after it.  No figure is a pass criterion.

    python tools/time_temporal_layers.py [--reps 5 --step-seconds 240]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learned-pmctf_amd"))

W, H, GOP, Q, STAGES = 1920, 1080, 16, 3, 4
ROWS = [(0, False), (1, False), (2, False), (3, False), (4, False), (1, True)]


def model():
    import pmctf_synth
    from pMCTF.models.video.pMCTF_L import pMCTF
    net = pMCTF(num_me_stages=STAGES).eval()
    net.load_state_dict(pmctf_synth.synth_state_dict(net.state_dict(), seed=0), strict=True)
    net = net.cuda()
    net.update(force=True)
    net.lazy_stages = False
    return net


def encode(folder):
    import torch
    import pmctf_gop
    import pmctf_synth
    net = model()
    frames = [list(pmctf_synth.frames_to_tensors(f, device="cuda")) for f in pmctf_synth.synth_yuv420(W, H, GOP)]
    sub = os.path.join(folder, pmctf_gop.gop_folder(0))
    os.makedirs(sub)
    with torch.no_grad():
        pmctf_gop.encode_gop(net, frames, H, W, Q, sub, skip_decoding=True)
    pmctf_gop.write_sequence_header(folder, width=W, height=H, frame_num=GOP, gop=GOP, q_index=Q, psize=128, me_downsample=1,
                                    ll_order="plane", **pmctf_gop.codec_header_fields(net))
    torch.cuda.synchronize()


def decode(folder, level, motion_fill, reps):
    import time
    import torch
    import pmctf_layers
    net = model()
    yuv = os.path.join(folder, f"level{level}{'m' if motion_fill else ''}.yuv")
    ts, out = [], None
    with torch.no_grad():
        for k in range(1 + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pmctf_layers.decode_sequence_layer(net, folder, yuv, level, verify=False, motion_fill=motion_fill)
            torch.cuda.synchronize()
            if k:
                ts.append(time.perf_counter() - t0)
    assert out["bytes_read"] == pmctf_layers.layer_bytes(folder, level, motion_fill)
    print(json.dumps({"level": level, "motion_fill": motion_fill, "pictures": len(out["frames"]),
                      "bytes_read": out["bytes_read"], "median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts),
                      "reps": ts, "device": torch.cuda.get_device_name(0)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-seconds", type=int, default=240, help="time limit of every GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_layers.json"))
    ap.add_argument("--step", nargs="+", help=argparse.SUPPRESS)                # a child: encode FOLDER | decode FOLDER K M
    a = ap.parse_args()
    if a.step:
        if a.step[0] == "encode":
            return encode(a.step[1])
        return decode(a.step[1], int(a.step[2]), a.step[3] == "1", a.reps)
    assert a.reps >= 5, "at least 5 timed repetitions after the warm-up"

    def step(*args):
        cmd = ["timeout", "-k", "10", str(a.step_seconds), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps),
               "--step", *args]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode:
            sys.exit(f"step {' '.join(args[:1] + args[2:])} ended with status {r.returncode}: nothing more is started")
        return r.stdout

    rec = {"what": "decode of one GOP at its temporal levels, wall seconds to a .yuv file", "width": W, "height": H,
           "gop": GOP, "q_index": Q, "num_me_stages": STAGES, "timed_reps": a.reps, "warmup": 1, "rows": []}
    with tempfile.TemporaryDirectory() as folder:
        step("encode", folder)
        for level, motion_fill in ROWS:
            row = json.loads(step("decode", folder, str(level), "01"[motion_fill]).strip().splitlines()[-1])
            rec["device"] = row.pop("device")
            rec["rows"].append(row)
            print(f"level {level}{' motion_fill' if motion_fill else ''}: {row['pictures']} pictures, {row['bytes_read']} bytes, "
                  f"{row['median_s']:.3f} s ({row['min_s']:.3f}-{row['max_s']:.3f})", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=2)
        f.write("\n")


if __name__ == "__main__":
    main()
