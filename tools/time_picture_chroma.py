#!/usr/bin/env python3
"""Times the chroma format conversion kernel (csrc/picture_chroma.hip, pmctf_chroma.Converter) per picture, next to the
device copy and to torch's own antialiased bicubic on the two float chroma planes, writes profiles/picture_chroma.json and
prints the table of DESIGN 5m:

  kernel    one launch per packed picture, HIP events around `--iters` launches in a row on the stream, after a warm-up,
            repeated `--repeats` times: median and spread of the per-picture time; and one launch alone between two events;
  copy_path the same kernel with the same format on both sides: the whole picture goes through the copy blocks alone, which
            is how the luma copy inside a conversion is judged;
  copy      Tensor.copy_ of a 256 MiB device buffer, timed the same way in the same process: the device copy's rate;
  torch     F.interpolate(mode="bicubic", antialias=True, align_corners=False) on Cb and Cr as float32 planes already on the
            device (no conversion from or to integers, no luma copy counted), timed the same way;
  bytes     source read once plus destination written once, over the kernel time.

Every case runs in a child process of its own under a time limit (`--limit` seconds); the first one that fails or runs out
of time ends the run, and the cases measured so far are written.

    python tools/time_picture_chroma.py [--iters 200 --repeats 7 --out profiles/picture_chroma.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learned-pmctf_amd"))

CASES = [(w, h, fi, fo, b) for w, h in ((3840, 2160), (1920, 1080)) for fi, fo in (("444", "420"), ("420", "444"))
         for b in (8, 10)]
COPY_BYTES = 256 << 20


def timed(fn, iters, repeats, warmup=20):
    """-> per-call microseconds of `repeats` runs of `iters` calls between two events"""
    import torch
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


def spread(us):
    return {"median": statistics.median(us), "min": min(us), "max": max(us)}


def one_case(index, iters, repeats, device):
    import torch
    import torch.nn.functional as F
    import pmctf_chroma
    w, h, fmt_in, fmt_out, b = CASES[index]
    dev = torch.device(device)
    dtype, size = (torch.uint8, 1) if b == 8 else (torch.uint16, 2)
    n_in, n_out = pmctf_chroma.frame_samples(w, h, fmt_in), pmctf_chroma.frame_samples(w, h, fmt_out)
    g = torch.Generator().manual_seed(b)
    frame = torch.randint(0, 1 << b, (n_in,), generator=g, dtype=torch.int32).to(dtype).to(dev)
    conv = pmctf_chroma.Converter(w, h, fmt_in, fmt_out, dev, b, "center")
    same = pmctf_chroma.Converter(w, h, fmt_in, fmt_in, dev, b, "center")
    kernel = timed(lambda: conv(frame), iters, repeats)
    alone = timed(lambda: conv(frame), 1, 25)
    copy_path = timed(lambda: same(frame), iters, repeats)
    big, dst = torch.empty(COPY_BYTES, dtype=torch.uint8, device=dev), torch.empty(COPY_BYTES, dtype=torch.uint8, device=dev)
    copy = timed(lambda: dst.copy_(big), max(iters // 4, 1), repeats)
    (sxi, syi), (sxo, syo) = pmctf_chroma.SUBSAMPLING[fmt_in], pmctf_chroma.SUBSAMPLING[fmt_out]
    planes = frame[h * w:].float().reshape(2, 1, h // syi, w // sxi)
    ref = timed(lambda: F.interpolate(planes, size=(h // syo, w // sxo), mode="bicubic", antialias=True, align_corners=False),
                max(iters // 4, 1), repeats)
    moved = (n_in + n_out) * size
    med, copy_tbs = statistics.median(kernel), 2 * COPY_BYTES / statistics.median(copy) / 1e6
    return {"case": f"{w}x{h} {fmt_in}->{fmt_out}", "bitdepth": b, "taps": [t for _, t in conv.tables],
            "device": torch.cuda.get_device_name(dev), "kernel_us": spread(kernel), "kernel_alone_us": spread(alone),
            "copy_path_us": spread(copy_path), "copy_path_TBs": 2 * n_in * size / statistics.median(copy_path) / 1e6,
            "device_copy_TBs": copy_tbs, "torch_float_chroma_planes_us": spread(ref), "bytes_moved": moved,
            "luma_fraction_of_bytes": 2 * h * w * size / moved, "achieved_TBs": moved / med / 1e6,
            "fraction_of_device_copy": moved / med / 1e6 / copy_tbs, "time_at_device_copy_us": moved / copy_tbs / 1e6}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--limit", type=int, default=120, help="seconds a case may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "picture_chroma.json"))
    ap.add_argument("--case", type=int, help="measure this case alone and print its row as JSON (what the children run)")
    a = ap.parse_args()
    if a.case is not None:
        print(json.dumps(one_case(a.case, a.iters, a.repeats, a.device)))
        return 0
    rows, status = [], 0
    for k in range(len(CASES)):
        cmd = [sys.executable, os.path.abspath(__file__), "--case", str(k), "--iters", str(a.iters), "--repeats",
               str(a.repeats), "--device", a.device]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"case {k} {CASES[k]}: no result within {a.limit} s; stopping", file=sys.stderr)
            status = 124
            break
        if done.returncode != 0:
            print(f"case {k} {CASES[k]}: exit status {done.returncode}; stopping\n{done.stderr[-2000:]}", file=sys.stderr)
            status = done.returncode
            break
        row = json.loads(done.stdout.strip().splitlines()[-1])
        rows.append(row)
        print(f"{row['case']:24s} {row['bitdepth']:2d} bit  kernel {row['kernel_us']['median']:7.1f} us (alone "
              f"{row['kernel_alone_us']['median']:6.1f})  copy path {row['copy_path_us']['median']:6.1f} us "
              f"{row['copy_path_TBs']:5.2f} TB/s  torch {row['torch_float_chroma_planes_us']['median']:7.1f} us  "
              f"{row['bytes_moved'] / 1e6:6.1f} MB  {row['achieved_TBs']:5.2f} TB/s of {row['device_copy_TBs']:5.2f} "
              f"({100 * row['fraction_of_device_copy']:4.1f} %)", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": rows[0]["device"] if rows else None, "iters": a.iters, "repeats": a.repeats, "rows": rows}, f,
                  indent=1)
        f.write("\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
