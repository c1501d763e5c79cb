#!/usr/bin/env python3
"""Times the picture resampling kernel (csrc/picture_scale.hip, pmctf_scale.Resampler) per picture, next to torch's own
antialiased bicubic on the three float planes, and writes profiles/picture_scale.json:

  kernel    one launch per packed 4:2:0 picture, HIP events around `--iters` launches in a row on the stream, after a
            warm-up, repeated `--repeats` times: median and spread of the per-picture time; and the time of one launch
            alone between two events (what a caller that waits for every picture sees);
  torch     F.interpolate(mode="bicubic", antialias=True, align_corners=False) on Y, Cb and Cr as float32 planes already
            on the device (no conversion from or to integers counted), timed the same way;
  bytes     source read once plus destination written once, over the kernel time, against the HBM figures of
            tools/bench_hbm.py (8 TB/s specification) and the measured device copy.

    python tools/time_picture_scale.py [--iters 200 --repeats 7 --out profiles/picture_scale.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learned-pmctf_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import pmctf_scale  # noqa: E402

HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.29         # MI355X: specification, measured device copy (tools/time_quality.py)
CASES = [(3840, 2160, 1920, 1080), (960, 540, 1920, 1080)]


def timed(fn, iters, repeats, warmup=20):
    """-> per-call microseconds of `repeats` runs of `iters` calls between two events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / iters)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "picture_scale.json"))
    a = ap.parse_args()
    dev = torch.device(a.device)
    rows = []
    for w_in, h_in, w_out, h_out in CASES:
        for b in (8, 10):
            dtype, size = (torch.uint8, 1) if b == 8 else (torch.uint16, 2)
            n_in, n_out = w_in * h_in * 3 // 2, w_out * h_out * 3 // 2
            g = torch.Generator().manual_seed(b)
            frame = torch.randint(0, 1 << b, (n_in,), generator=g, dtype=torch.int32).to(dtype).to(dev)
            r = pmctf_scale.Resampler(w_in, h_in, w_out, h_out, dev, b)
            kernel = timed(lambda: r(frame), a.iters, a.repeats)
            alone = timed(lambda: r(frame), 1, 25)
            planes = [frame[:h_in * w_in].float().reshape(1, 1, h_in, w_in),
                      frame[h_in * w_in:].float().reshape(2, 1, h_in // 2, w_in // 2)]
            sizes = [(h_out, w_out), (h_out // 2, w_out // 2)]
            ref = timed(lambda: [F.interpolate(p, size=s, mode="bicubic", antialias=True, align_corners=False)
                                 for p, s in zip(planes, sizes)], max(a.iters // 4, 1), a.repeats)
            moved = (n_in + n_out) * size
            med = statistics.median(kernel)
            row = {"case": f"{w_in}x{h_in}->{w_out}x{h_out}", "bitdepth": b, "taps": [t for _, t in r.tables],
                   "kernel_us": {"median": med, "min": min(kernel), "max": max(kernel)},
                   "kernel_alone_us": {"median": statistics.median(alone), "min": min(alone), "max": max(alone)},
                   "torch_float_planes_us": {"median": statistics.median(ref), "min": min(ref), "max": max(ref)},
                   "bytes_moved": moved, "achieved_TBs": moved / med / 1e6,
                   "fraction_of_hbm_spec": moved / med / 1e6 / HBM_SPEC_TBS,
                   "fraction_of_hbm_copy": moved / med / 1e6 / HBM_COPY_TBS,
                   "time_at_hbm_copy_us": moved / HBM_COPY_TBS / 1e6}
            rows.append(row)
            print(f"{row['case']:24s} {b:2d} bit  kernel {med:8.1f} us (alone {row['kernel_alone_us']['median']:7.1f})  "
                  f"torch {row['torch_float_planes_us']['median']:8.1f} us  {moved / 1e6:6.1f} MB  "
                  f"{row['achieved_TBs']:5.2f} TB/s ({100 * row['fraction_of_hbm_copy']:4.1f} % of the device copy)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(dev), "iters": a.iters, "repeats": a.repeats, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
