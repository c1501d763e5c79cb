#!/usr/bin/env python3
"""Times the per-plane quality record of one picture (pmctf_quality.frame_quality_planar) against the same
figures from torch on the same GPU, in one process, and writes profiles/planar_quality.json.

Cases: 1920x1080 at 8-bit 4:2:0, 10-bit 4:2:0 and 10-bit 4:4:4, each with and without MS-SSIM.
  hip     pmctf_quality.frame_quality_planar: host clock around work that ends in the picture's one copy to the host
  torch   the yardstick: per-plane int64 error sums and the float32 restatement of MS-SSIM (tests/quality_restatement.py,
          one channel, data range 2^b - 1) in torch on the GPU, from int32 copies of the pictures made outside the timing
          (torch has no arithmetic on uint16 tensors; the conversion is not charged to it)
  kernels events on the stream around the entries of include/pmctf_quality.h alone, no copy
  context ops.frame_quality at 8 bits on the same pictures: three RGB channels plus the RGB front end
The two paths are warmed and alternated picture by picture; medians and ranges of the repetitions are written down, with
the ratio torch / hip per case.  Exit status 1 when a case is slower than the torch path.

    python tools/time_planar_quality.py [--width 1920 --height 1080 --frames 30 --warmup 5]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learned-pmctf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import planar_quality_restatement as pq  # noqa: E402
import pmctf_quality  # noqa: E402
import quality_restatement as qr  # noqa: E402
from pMCTF.hip import ops  # noqa: E402

CASES = ((8, "420"), (10, "420"), (10, "444"))


def torch_path(a32, b32, shapes, depth, msssim):
    """a32, b32: the packed pictures as int32 device tensors"""
    out, at, sums = {}, 0, []
    planes = []
    for rows, cols in shapes:
        planes.append((a32[at:at + rows * cols].view(rows, cols), b32[at:at + rows * cols].view(rows, cols)))
        at += rows * cols
    for pa, pb in planes:
        d = (pa - pb).long()
        sums.append((d * d).sum())
    out["sse"] = tuple(torch.stack(sums).tolist())
    for name, (pa, pb), (rows, cols) in zip("y cb cr".split(), planes, shapes):
        out["msssim_" + name] = qr.ms_ssim(pa.float()[None], pb.float()[None], torch.float32,
                                           data_range=float((1 << depth) - 1), device=pa.device)[0] \
            if msssim and min(rows, cols) > qr.MIN_SIDE else None
    return out


def stats(ts):
    return {"median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3}


def kernel_time(a, b, h, w, fmt, depth, msssim, frames, warmup):
    """events around the entries alone: the sums, then the planes that have five scales"""
    L = pmctf_quality.library()
    shapes = pmctf_quality.plane_shapes(h, w, fmt)
    out = torch.empty(3 + 30, dtype=torch.int64, device=a.device)
    scratch = torch.empty(L.pmctf_plane_msssim_scratch_floats(h, w), dtype=torch.float32, device=a.device)
    st = torch.cuda.current_stream()
    ts = []
    for k in range(warmup + frames):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        pmctf_quality._enqueue_sse(L, a, b, h, w, fmt, depth, C.c_void_p(out.data_ptr()))
        off = 0
        for p, (rows, cols) in enumerate(shapes):
            if msssim and pmctf_quality.has_msssim(rows, cols):
                pmctf_quality._enqueue_msssim(L, a.data_ptr() + off * a.element_size(), b.data_ptr() + off * a.element_size(),
                                              rows, cols, depth, scratch, C.c_void_p(out.data_ptr() + 8 * (3 + 10 * p)))
            off += rows * cols
        e1.record(st)
        e1.synchronize()
        if k >= warmup:
            ts.append(e0.elapsed_time(e1) * 1e-3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planar_quality.json"))
    a = ap.parse_args()
    assert a.frames >= 20 and a.warmup >= 2, "at least 20 timed pictures each after warm-up"
    h, w = a.height, a.width
    dev = torch.device("cuda:0")
    record = {"device": torch.cuda.get_device_name(0), "width": w, "height": h, "frames": a.frames, "warmup": a.warmup,
              "method": "hip and torch alternated picture by picture in one process, host clock around work that ends in "
                        "the copy to the host; kernels: events on the stream around the entries alone", "cases": []}
    slower = []
    for depth, fmt in CASES:
        shapes = pmctf_quality.plane_shapes(h, w, fmt)
        pairs = []
        for k in range(4):
            src = pq.synth_frames(h, w, fmt, depth, 1, seed=k)[0]
            r = np.random.default_rng(k)
            rec = np.clip(src.astype(np.int64) + np.rint(0.01 * (1 << depth) * r.standard_normal(src.size)).astype(np.int64),
                          0, (1 << depth) - 1).astype(src.dtype)
            ta, tb = torch.from_numpy(src).to(dev), torch.from_numpy(rec).to(dev)
            pairs.append((ta, tb, torch.from_numpy(src.astype(np.int32)).to(dev), torch.from_numpy(rec.astype(np.int32)).to(dev)))
        for msssim in (True, False):
            t_hip, t_torch, last = [], [], None
            for k in range(a.warmup + a.frames):
                ta, tb, a32, b32 = pairs[k % len(pairs)]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ref = torch_path(a32, b32, shapes, depth, msssim)
                t1 = time.perf_counter()
                got = pmctf_quality.frame_quality_planar(ta, tb, h, w, fmt, depth, msssim=msssim)
                t2 = time.perf_counter()
                assert got["sse"] == ref["sse"], (got["sse"], ref["sse"])
                if k >= a.warmup:
                    t_torch.append(t1 - t0)
                    t_hip.append(t2 - t1)
                last = (got, ref)
            kern = kernel_time(pairs[0][0], pairs[0][1], h, w, fmt, depth, msssim, a.frames, a.warmup)
            case = {"bitdepth": depth, "chroma_format": fmt, "msssim": msssim, "hip": stats(t_hip), "torch": stats(t_torch),
                    "kernels": stats(kern), "ratio_torch_over_hip": statistics.median(t_torch) / statistics.median(t_hip),
                    "last": {"hip": {k: v for k, v in last[0].items()}, "torch_float32": last[1]}}
            record["cases"].append(case)
            print(f"{depth}-bit {fmt} msssim={msssim}: hip {case['hip']['median_ms']:.3f} ms "
                  f"[{case['hip']['min_ms']:.3f} .. {case['hip']['max_ms']:.3f}], torch {case['torch']['median_ms']:.3f} ms "
                  f"[{case['torch']['min_ms']:.3f} .. {case['torch']['max_ms']:.3f}], ratio "
                  f"{case['ratio_torch_over_hip']:.2f}, kernels {case['kernels']['median_ms'] * 1e3:.1f} us", flush=True)
            if not statistics.median(t_hip) < statistics.median(t_torch):
                slower.append((depth, fmt, msssim))
    # context: the 8-bit RGB path on a picture of the same size
    ta, tb = pairs_8 = [torch.from_numpy(f).to(dev) for f in pq.synth_frames(h, w, "420", 8, 2, seed=9)]
    oy, oc = ops.planes_from(ta, h, w, 8, psize=2)[2:]
    ry, rc = ops.planes_from(tb, h, w, 8, psize=2)[:2]
    ts = []
    for k in range(a.warmup + a.frames):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.frame_quality(ry, rc, oy, oc, h, w)
        if k >= a.warmup:
            ts.append(time.perf_counter() - t0)
    record["context_frame_quality_8bit_rgb"] = stats(ts)
    print(f"context, ops.frame_quality (8-bit, RGB front end + three channels): {record['context_frame_quality_8bit_rgb']}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=2)
        f.write("\n")
    if slower:
        sys.exit(f"slower than the torch path: {slower}")


if __name__ == "__main__":
    main()
