#!/usr/bin/env python3
"""Measures what rate control (pmctf_rate.encode_sequence_rate) costs at 1920x1080 and writes profiles/rate_control.json:
trials per GOP, wall time against coding the same sequence once at a fixed q_index, the device memory the process holds
afterwards (torch.cuda.memory_reserved) and the number of launch plans the engine holds (plans are keyed by q_index and
never dropped, so every q_index visited records more).

    python tools/time_rate_control.py [--frames 32 --gop 16 --slack 0 0.1]

Synthetic weights with four motion stages, synthetic pictures, all 21 choices.  Every row is a process of its own under
`timeout`, so that a row starts with no plans: first the sequence at the middle q_index, whose size sets the bitrate; then
one row per --slack value; then the sequence at the q_index the controller chose most often (the baseline of the wall
times; the first row serves when that is the middle one).  A row that cannot be made is recorded as "not measured", and
after a row that crashed or ran into its time limit no further row is started."""
import argparse
import collections
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learned-pmctf_amd"))
FPS = 30
MARK = "ROW "


def child(a):
    """one row, in this process: code the sequence, print what was measured"""
    import torch
    import pmctf_rate
    import pmctf_seq
    import pmctf_synth
    from pMCTF.models.video.pMCTF_L import pMCTF
    net = pMCTF(num_me_stages=a.num_me_stages).eval()
    net.load_state_dict(pmctf_synth.synth_state_dict(net.state_dict(), seed=0), strict=True)
    net = net.to("cuda:0")
    net.update(force=True)
    w, h = (int(v) for v in a.size.split("x"))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        if a.bitrate is None:
            out = pmctf_seq.encode_sequence_gops(net, a.source, w, h, a.frames, a.gop, a.q_index, a.bins, "cuda:0")
        else:
            out = pmctf_rate.encode_sequence_rate(net, a.source, w, h, a.frames, a.gop, a.bitrate, FPS, a.bins, "cuda:0",
                                                  slack=a.slack[0], max_trials=a.max_trials)
    torch.cuda.synchronize()
    row = {"wall_s": time.perf_counter() - t0, "total_bits": int(sum(out["bits"])),
           "memory_reserved_MiB": torch.cuda.memory_reserved() / 2 ** 20, "launch_plans": len(net.engine().pair_plans),
           "psnr_yuv_mean": sum(out["psnr"]) / len(out["psnr"])}
    if a.bitrate is None:
        row.update(q_index=a.q_index)
    else:
        v = pmctf_rate.verify_rate_record(a.bins)
        row.update(slack=a.slack[0], bitrate=a.bitrate, bits_per_second=v["bits_per_second"],
                   q_indexes=[r["q_index"] for r in out["rate"]], fits=[r["fits"] for r in out["rate"]],
                   trials_per_gop=[len(r["trials"]) for r in out["rate"]], trial_seconds=sum(r["seconds"] for r in out["rate"]),
                   q_visited=sorted({q for r in out["rate"] for q, _ in r["trials"]}))
    print(MARK + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--gop", type=int, default=16)
    ap.add_argument("--num-me-stages", type=int, default=4)
    ap.add_argument("--slack", type=float, nargs="+", default=[0.0, 0.1])
    ap.add_argument("--max-trials", type=int, default=4)
    ap.add_argument("--row-timeout", type=int, default=300, help="seconds a row may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_control.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--source", help=argparse.SUPPRESS)
    ap.add_argument("--bins", help=argparse.SUPPRESS)
    ap.add_argument("--q-index", type=int, help=argparse.SUPPRESS)
    ap.add_argument("--bitrate", type=int, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    import pmctf_gop
    import pmctf_synth
    w, h = (int(v) for v in a.size.split("x"))
    rows, stopped = [], None

    def row(name, folder, *args):
        nonlocal stopped
        if stopped is not None:
            rows.append({"row": name, "not measured": f"not started: {stopped}"})
            return None
        os.makedirs(folder)
        cmd = ["timeout", "-k", "10", str(a.row_timeout), sys.executable, os.path.abspath(__file__), "--child", "--size", a.size,
               "--frames", str(a.frames), "--gop", str(a.gop), "--num-me-stages", str(a.num_me_stages), "--max-trials",
               str(a.max_trials), "--source", src, "--bins", folder] + [str(v) for v in args]
        print(f"row '{name}' ...", flush=True)
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        found = [ln[len(MARK):] for ln in p.stdout.splitlines() if ln.startswith(MARK)]
        if p.returncode != 0 or not found:
            stopped = f"row '{name}' ended with status {p.returncode}"
            rows.append({"row": name, "not measured": f"status {p.returncode}", "output_tail": p.stdout[-2000:]})
            return None
        rows.append(dict(json.loads(found[-1]), row=name))
        print(f"  {rows[-1]}", flush=True)
        return rows[-1]

    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "src.yuv")
        pmctf_gop.write_yuv(src, pmctf_synth.synth_yuv420(w, h, a.frames, seed=1234))
        middle = 10
        probe = row(f"fixed q_index {middle}", os.path.join(td, "probe"), "--q-index", middle)
        rate_rows = []
        if probe is not None:
            bitrate = probe["total_bits"] * FPS // a.frames
            for s in a.slack:
                rate_rows.append(row(f"bitrate, slack {s:g}", os.path.join(td, f"slack{s:g}"), "--bitrate", bitrate, "--slack", s))
        chosen = collections.Counter(q for r in rate_rows if r is not None for q in r["q_indexes"])
        base = probe
        if chosen and chosen.most_common(1)[0][0] != middle:
            q = chosen.most_common(1)[0][0]
            base = row(f"fixed q_index {q}", os.path.join(td, "baseline"), "--q-index", q)
    for r in rows:
        if base is not None and "wall_s" in r:
            r["wall_vs_baseline"] = r["wall_s"] / base["wall_s"]
    out = {"what": "rate control against one coding at a fixed q_index, one process per row", "picture": [h, w],
           "frames": a.frames, "max_gop": a.gop, "fps": FPS, "num_me_stages": a.num_me_stages, "q_choices": "0..20",
           "max_trials": a.max_trials, "baseline": None if base is None else base["row"], "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=2)
        f.write("\n")
    print("| row | q_index per GOP | trials per GOP | wall, s | vs baseline | reserved, MiB | launch plans |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        if "not measured" in r:
            print(f"| {r['row']} | not measured ({r['not measured']}) | | | | | |")
        else:
            print(f"| {r['row']} | {r.get('q_indexes', r.get('q_index'))} | {r.get('trials_per_gop', 1)} | {r['wall_s']:.1f} | "
                  f"{r.get('wall_vs_baseline', float('nan')):.2f} | {r['memory_reserved_MiB']:.0f} | {r['launch_plans']} |")
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
