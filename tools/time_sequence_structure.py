#!/usr/bin/env python3
"""Times the sequence-structure pre-analysis (csrc/scene_ops.hip, pmctf_seq.sequence_activity) at 1920x1080 and writes
profiles/sequence_structure.json:

  kernel  GPU time per launch of pmctf_luma_activity_f32 with its two clears, with a previous picture: a batch of launches
          captured into one HIP graph, HIP events around each replay (the host's enqueue rate is not in the figure), and
          the algorithmic bytes per second that time means (two float32 luma planes read, 8.3 MB each at 1080p);
  pass    wall time per picture of sequence_activity over a .yuv file of --frames pictures, host clock: reading the file,
          the copy of the bytes to the device, the ingest kernel, the activity kernel, one copy back per 16 pictures.

    python tools/time_sequence_structure.py [--reps 30 --warmup 5 --batch 50 --frames 32]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learned-pmctf_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pmctf_seq  # noqa: E402
from pMCTF.hip import lib  # noqa: E402
from pMCTF.utils.yuv_reader import YUVReader  # noqa: E402

RUNTIME_COPY_TBS = 5.5          # the runtime's own device copy on this part (docs/history.md, section 5)


def stats(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "n": len(ts)}


def gpu_time(fn, reps, warmup, batch):
    """seconds per call of fn on the device: `batch` calls are captured into one HIP graph (a chain, no branches) and each
    replay is bracketed by events, so that a launch of a few microseconds is not measured at the host's enqueue rate"""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(batch):
            fn()
    ts = []
    for k in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        if k >= warmup:
            ts.append(e0.elapsed_time(e1) * 1e-3 / batch)
    return stats(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--bitdepth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--frames", type=int, default=32, help="pictures of the analysis pass")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sequence_structure.json"))
    a = ap.parse_args()
    assert a.reps >= 20 and a.warmup >= 2, "at least 20 timed repetitions after warm-up"
    w, h = (int(v) for v in a.size.split("x"))
    b, dev = a.bitdepth, torch.device("cuda:0")
    rng = np.random.default_rng(0)
    dtype = np.uint16 if b > 8 else np.uint8
    lumas = [torch.from_numpy(rng.integers(0, 1 << b, (1, 1, h, w), dtype=dtype).astype(np.float32) * 2.0 ** -(b - 8)).to(dev)
             for _ in range(2)]
    hist = torch.empty(256, dtype=torch.int32, device=dev)
    sad = torch.empty(1, dtype=torch.int64, device=dev)
    L = lib.hip()
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def launch():
        rc = L.pmctf_luma_activity_f32(ptr(lumas[0]), ptr(lumas[1]), h, w, b, ptr(hist), ptr(sad),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0

    nbytes = 2 * 4 * h * w
    kernel = gpu_time(launch, a.reps, a.warmup, a.batch)
    kernel.update(algorithmic_bytes=nbytes, algorithmic_TBps=nbytes / kernel["median"] / 1e12)
    first = (hist.cpu().tolist(), sad.cpu().tolist())
    launch()
    same = first == (hist.cpu().tolist(), sad.cpu().tolist()) and sum(first[0]) == h * w

    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "src.yuv")
        with open(path, "wb") as f:
            for _ in range(a.frames):
                f.write(rng.integers(0, 1 << b, h * w * 3 // 2, dtype=dtype).tobytes())
        ts = []
        for k in range(2 + 5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pmctf_seq.sequence_activity(lambda: YUVReader(path, w, h, bitdepth=b), a.frames, dev, bitdepth=b)
            torch.cuda.synchronize()
            if k >= 2:
                ts.append((time.perf_counter() - t0) / a.frames)
    out = {"device": torch.cuda.get_device_name(0), "picture": [h, w], "bitdepth": b, "reps": a.reps, "warmup": a.warmup,
           "batch": a.batch, "runtime_copy_TBps": RUNTIME_COPY_TBS, "kernel": kernel, "runs_agree": bool(same),
           "analysis_pass": dict(stats(ts), frames=a.frames, unit="seconds per picture, host clock")}
    us = lambda t: f"{t['median'] * 1e6:.1f} ({t['min'] * 1e6:.1f}-{t['max'] * 1e6:.1f})"
    print(f"{w}x{h}, {b} bits, {out['device']}; median (min-max)")
    print("| | time, us | algorithmic bytes, MB | TB/s (runtime copy: %.1f) |" % RUNTIME_COPY_TBS)
    print("|---|---|---|---|")
    print(f"| luma_activity with its clears, GPU time per launch ({a.reps} replays of {a.batch}) | {us(kernel)} | "
          f"{nbytes / 1e6:.1f} | {kernel['algorithmic_TBps']:.2f} |")
    print(f"| analysis pass per picture, wall ({a.frames} pictures, 5 passes) | {us(out['analysis_pass'])} | | |")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=2)
        f.write("\n")
    if not same:
        sys.exit("two runs of the kernel must give the same integers")


if __name__ == "__main__":
    main()
