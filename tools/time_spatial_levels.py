#!/usr/bin/env python3
"""Times the decode of a sequence at its spatial levels (pmctf_spatial.decode_sequence_layer) and writes
profiles/spatial_levels.json: a 1920x1080 folder of one GOP of 16 at q_index 3, 4 motion stages, synthetic weights; for the
spatial levels 0, 1 and 2 and for temporal level 1 at spatial level 1 the wall time of the decode to a .yuv file (the host
clock between two device synchronisations: file reads, entropy decode, synthesis, conversion and the write), the median of
--reps runs after one warm-up, the bytes of the payloads the decoder read (payload_bytes_used, summed over the GOP) and
their share of level 0's.  Level 0 is the baseline: it must give the bytes of pmctf_gop.decode_sequence.
Every reduced output is also described by its YUV-PSNR ((6 Y + Cb + Cr) / 8) against the full-size output of the same
temporal level resampled to its size by pmctf_scale's filter: what the preview looks like with these weights, not a bar.

Every GPU step is a process of its own under `timeout`: the encode of the folder, then one process per row.  The first
step that fails ends the run; nothing is started after it.  No figure is a pass criterion.

    python tools/time_spatial_levels.py [--reps 5 --step-seconds 300]
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

from time_temporal_layers import GOP, H, Q, STAGES, W, encode, model  # noqa: E402 - the same folder, coded the same way

ROWS = [(0, 0), (0, 1), (0, 2), (1, 1)]                                   # (temporal level, spatial level)


def psnr_yuv(a, b, h, w):
    import numpy as np
    n, out = h * w, []
    for lo, hi in ((0, n), (n, n + n // 4), (n + n // 4, n + n // 2)):
        mse = float(np.mean((a[lo:hi].astype(np.float64) - b[lo:hi].astype(np.float64)) ** 2))
        out.append(99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse))
    return (6 * out[0] + out[1] + out[2]) / 8


def decode(folder, t, k, reps):
    import time
    import numpy as np
    import torch
    import pmctf_gop
    import pmctf_layers
    import pmctf_scale
    import pmctf_spatial
    net = model()
    yuv = os.path.join(folder, f"t{t}s{k}.yuv")
    ts, out = [], None
    with torch.no_grad():
        for i in range(1 + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pmctf_spatial.decode_sequence_layer(net, folder, yuv, t, verify=False, spatial_level=k)
            torch.cuda.synchronize()
            if i:
                ts.append(time.perf_counter() - t0)
        ref = os.path.join(folder, f"t{t}_reference.yuv")
        if t == 0:
            pmctf_gop.decode_sequence_checked(net, folder, ref, verify=False)
        else:
            pmctf_layers.decode_sequence_layer(net, folder, ref, t, verify=False)
        row = {"temporal_level": t, "spatial_level": k, "pictures": len(out["frames"]), "size": list(out["size"][::-1]),
               "bytes_read": out["bytes_read"], "payload_bytes_used": sum(sum(g.values()) for g in out["payload_bytes_used"]),
               "symbols_decoded": sum(sum(g.values()) for g in out["symbols_decoded"]),
               "median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "reps": ts,
               "device": torch.cuda.get_device_name(0)}
        if k == 0:
            assert open(yuv, "rb").read() == open(ref, "rb").read(), "spatial level 0 does not give the baseline's bytes"
            row["equals_baseline"] = True
        else:
            h, w = out["size"]
            down = pmctf_scale.Resampler(W, H, w, h, torch.device("cuda"))
            full, small = np.fromfile(ref, dtype=np.uint8), np.fromfile(yuv, dtype=np.uint8)
            n0, n1 = W * H * 3 // 2, w * h * 3 // 2
            values = [psnr_yuv(down(torch.from_numpy(full[i * n0:(i + 1) * n0]).cuda()).cpu().numpy(),
                               small[i * n1:(i + 1) * n1], h, w) for i in range(len(out["frames"]))]
            row["psnr_yuv_vs_resampled"] = {"mean": statistics.mean(values), "min": min(values), "max": max(values)}
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-seconds", type=int, default=300, help="time limit of every GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spatial_levels.json"))
    ap.add_argument("--step", nargs="+", help=argparse.SUPPRESS)                # a child: encode FOLDER | decode FOLDER T K
    a = ap.parse_args()
    if a.step:
        if a.step[0] == "encode":
            return encode(a.step[1])
        return decode(a.step[1], int(a.step[2]), int(a.step[3]), a.reps)
    assert a.reps >= 5, "at least 5 timed repetitions after the warm-up"

    def step(*args):
        cmd = ["timeout", "-k", "10", str(a.step_seconds), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps),
               "--step", *args]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode:
            sys.exit(f"step {' '.join(args[:1] + args[2:])} ended with status {r.returncode}: nothing more is started")
        return r.stdout

    rec = {"what": "decode of one GOP at its spatial levels, wall seconds to a .yuv file", "width": W, "height": H,
           "gop": GOP, "q_index": Q, "num_me_stages": STAGES, "timed_reps": a.reps, "warmup": 1, "rows": []}
    with tempfile.TemporaryDirectory() as folder:
        step("encode", folder)
        for t, k in ROWS:
            row = json.loads(step("decode", folder, str(t), str(k)).strip().splitlines()[-1])
            rec["device"] = row.pop("device")
            row["payload_share_of_level_0"] = row["payload_bytes_used"] / rec["rows"][0]["payload_bytes_used"] if rec["rows"] else 1.0
            rec["rows"].append(row)
            print(f"temporal {t}, spatial {k}: {row['pictures']} pictures of {row['size'][0]}x{row['size'][1]}, "
                  f"{row['payload_bytes_used']} payload bytes ({100 * row['payload_share_of_level_0']:.1f} %), "
                  f"{row['median_s']:.3f} s ({row['min_s']:.3f}-{row['max_s']:.3f})"
                  + (f", PSNR {row['psnr_yuv_vs_resampled']['mean']:.2f} dB" if k else ""), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=2)
        f.write("\n")


if __name__ == "__main__":
    main()
