#!/usr/bin/env python3
"""Times the decode of chosen pictures of a sequence (pmctf_access.decode_frames) and writes profiles/random_access.json: a
1920x1080 folder of GOPs of 16 at q_index 3, synthetic weights; one picture at each of the 16 positions of the second GOP,
a window of 4 pictures and the full GOP.  Per row: the files and bytes read, the pairs that ran their `ref` half alone, and
the wall time of the decode to a .yuv file (the host clock between two device synchronisations: file reads, entropy decode,
synthesis, conversion and the write), one-sided as decode_frames runs it and with one_sided=False (both halves of every
pair), each the median of --reps runs after one warm-up.  The first GOP is never wanted: it is never opened.

Every GPU step is a process of its own under `timeout`: the encode of the folder, then one process per group of rows.  The
first step that fails ends the run; nothing is started after it.  No figure is a pass criterion.

    python tools/time_random_access.py [--reps 5 --step-seconds 400]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_temporal_layers import GOP, H, Q, STAGES, W, model  # noqa: E402 - the same model and pictures

GOPS = 2
ROWS = [[GOP + n] for n in range(GOP)] + [list(range(GOP + 6, GOP + 10)), list(range(GOP, 2 * GOP))]
GROUP = 6                                                 # rows per process


def encode(folder):
    """the second GOP is coded; the first is a folder that does not exist, which a selection inside the second never opens"""
    import torch
    import pmctf_gop
    import pmctf_synth
    net = model()
    frames = [list(pmctf_synth.frames_to_tensors(f, device="cuda")) for f in pmctf_synth.synth_yuv420(W, H, GOP)]
    sub = os.path.join(folder, pmctf_gop.gop_folder(GOPS - 1))
    os.makedirs(sub)
    with torch.no_grad():
        pmctf_gop.encode_gop(net, frames, H, W, Q, sub, skip_decoding=True)
    pmctf_gop.write_sequence_header(folder, width=W, height=H, frame_num=GOPS * GOP, gop=GOP, q_index=Q, psize=128,
                                    me_downsample=1, ll_order="plane", **pmctf_gop.codec_header_fields(net))
    torch.cuda.synchronize()


def decode(folder, rows, reps):
    import time
    import torch
    import pmctf_access
    import pmctf_gop
    net = model()
    yuv = os.path.join(folder, "frames.yuv")
    for frames in rows:
        row = {"frames": frames}
        for key, one_sided in (("one_sided", True), ("two_sided", False)):
            ts, out = [], None
            with torch.no_grad():
                for k in range(1 + reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = pmctf_gop.decode_sequence_with(pmctf_access.FrameDecode(frames, one_sided=one_sided), net, folder,
                                                         yuv, verify=False)
                    torch.cuda.synchronize()
                    if k:
                        ts.append(time.perf_counter() - t0)
            assert out["times"] == frames and out["gops_opened"] == 1
            assert out["bytes_read"] == pmctf_access.access_bytes(folder, frames)
            row[key] = {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "reps": ts,
                        "half_pairs": out["half_pairs"]}
        local = [t - (GOPS - 1) * GOP for t in frames]
        plan = pmctf_access.gop_plan(GOP, local)
        row.update({"local": local, "files": len(plan["files"]), "picture_files": len(plan["picture_files"]),
                    "motion_files": len(plan["motion_files"]), "bytes_read": out["bytes_read"],
                    "device": torch.cuda.get_device_name(0)})
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-seconds", type=int, default=400, help="time limit of every GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "random_access.json"))
    ap.add_argument("--step", nargs="+", help=argparse.SUPPRESS)                # a child: encode FOLDER | decode FOLDER ROWS
    a = ap.parse_args()
    if a.step:
        if a.step[0] == "encode":
            return encode(a.step[1])
        return decode(a.step[1], json.loads(a.step[2]), a.reps)
    assert a.reps >= 5, "at least 5 timed repetitions after the warm-up"

    def step(*args):
        cmd = ["timeout", "-k", "10", str(a.step_seconds), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps),
               "--step", *args]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode:
            sys.exit(f"step {' '.join(args[:1] + args[2:])} ended with status {r.returncode}: nothing more is started")
        return r.stdout

    rec = {"what": "decode of chosen pictures of one GOP of 16, wall seconds to a .yuv file; two_sided: one_sided=False",
           "width": W, "height": H, "gop": GOP, "q_index": Q, "num_me_stages": STAGES, "timed_reps": a.reps, "warmup": 1,
           "rows": []}
    with tempfile.TemporaryDirectory() as folder:
        step("encode", folder)
        for at in range(0, len(ROWS), GROUP):
            for line in step("decode", folder, json.dumps(ROWS[at:at + GROUP])).strip().splitlines():
                if not line.startswith("{"):
                    continue
                row = json.loads(line)
                rec["device"] = row.pop("device")
                rec["rows"].append(row)
                print(f"pictures {row['local']}: {row['files']} files ({row['picture_files']} picture, {row['motion_files']} "
                      f"motion), {row['bytes_read']} bytes, {row['one_sided']['half_pairs']} half pairs, "
                      f"{row['one_sided']['median_s']:.3f} s one-sided, {row['two_sided']['median_s']:.3f} s two-sided",
                      flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=2)
        f.write("\n")


if __name__ == "__main__":
    main()
