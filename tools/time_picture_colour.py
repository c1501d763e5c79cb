#!/usr/bin/env python3
"""Times the RGB kernels (csrc/picture_colour.hip, pmctf_colour.RgbUnpacker / RgbPacker) per picture, next to the device
copy and to the torch expression a user would otherwise write, writes profiles/picture_colour.json and prints the table of
DESIGN 5s:

  kernel    one launch per picture into a destination allocated once, HIP events around `--iters` launches in a row on the
            stream, after a warm-up, repeated `--repeats` times: median and spread of the per-picture time; and one launch
            alone between two events (median of 25);
  copy      Tensor.copy_ of a 256 MiB device buffer, timed the same way in the same process: the device copy's rate;
  torch     the same conversion written as float32 statements on the device (exact rational coefficients rounded to float,
            round, clamp, cast, torch.cat / stack), timed the same way; its result is checked once against the kernel's:
            within one code value everywhere;
  bytes     surface plus planar picture, each touched once, over the kernel time.

Every case runs in a child process of its own under a time limit (`--limit` seconds); the first one that fails or runs out
of time ends the run, and the cases measured so far are written.

    python tools/time_picture_colour.py [--iters 200 --repeats 7 --out profiles/picture_colour.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learned-pmctf_amd"))

CASES = [(w, h, layout, kind) for w, h in ((1920, 1080), (3840, 2160)) for layout in ("rgb24", "rgb48", "gbrp10")
         for kind in ("to_ycc", "to_rgb")]
COLOUR = ("bt709", "limited")
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


def _samples(t, depth):
    """a uint8 tensor holding bytes (depth 8) or little-endian words -> float32 sample values"""
    import torch
    if depth == 8:
        return t.float()
    return (t.view(torch.int16).to(torch.int32) & 0xFFFF).float()


def _store(v, depth):
    """rounded, clamped float32 values -> the bytes they are stored as (uint8 tensor)"""
    import torch
    v = torch.clamp(torch.round(v), 0, (1 << depth) - 1)
    return v.to(torch.uint8) if depth == 8 else v.to(torch.int32).to(torch.int16).view(torch.uint8)


def torch_expression(layout, w, h, forward):
    """the conversion as torch float statements: surface bytes -> planar bytes (forward), planar bytes -> surface bytes"""
    import torch
    import pmctf_colour
    depth = pmctf_colour.LAYOUTS[layout][1]
    fwd, inv = pmctf_colour.exact_rows(COLOUR[0], COLOUR[1], depth)
    _, _, oy, oc = pmctf_colour.scales(COLOUR[1], depth)
    rows = [[float(c) for c in row] for row in (fwd if forward else inv)]
    n = h * w
    planar = layout.startswith("gbrp")

    def to_ycc(s):
        v = _samples(s, depth)
        if planar:
            g, b, r = v[:n], v[n:2 * n], v[2 * n:]
        else:
            t = v.view(n, 3)
            r, g, b = t[:, 0], t[:, 1], t[:, 2]
        out = [row[0] * r + row[1] * g + row[2] * b + o for row, o in zip(rows, (oy, oc, oc))]
        return _store(torch.cat(out), depth)

    def to_rgb(s):
        v = _samples(s, depth)
        y, cb, cr = v[:n] - oy, v[n:2 * n] - oc, v[2 * n:] - oc
        r, g, b = (row[0] * y + row[1] * cb + row[2] * cr for row in rows)
        return _store(torch.cat([g, b, r]) if planar else torch.stack([r, g, b], dim=1).reshape(-1), depth)
    return to_ycc if forward else to_rgb


def one_case(index, iters, repeats, device):
    import torch
    import pmctf_colour
    w, h, layout, kind = CASES[index]
    dev = torch.device(device)
    depth = pmctf_colour.LAYOUTS[layout][1]
    dtype, word = (torch.uint8, 1) if depth == 8 else (torch.uint16, 2)
    n = 3 * h * w
    g = torch.Generator().manual_seed(depth)
    values = torch.randint(0, 1 << depth, (n,), generator=g, dtype=torch.int32).to(dtype).to(dev)
    unpack, pack = pmctf_colour.RgbUnpacker(layout, w, h, COLOUR), pmctf_colour.RgbPacker(layout, w, h, COLOUR)
    forward = kind == "to_ycc"
    if forward:
        src = values.view(torch.uint8)                                   # a surface of random samples
        out = torch.empty(n, dtype=dtype, device=dev)
        fn = lambda: unpack(src, out=out)
    else:
        src = values                                                     # a planar picture over the whole code range
        out = torch.empty(n * word, dtype=torch.uint8, device=dev)
        fn = lambda: pack(src, out=out)
    expr = torch_expression(layout, w, h, forward)
    as_int = lambda t: t.view(torch.uint8).to(torch.int32) if depth == 8 else t.view(torch.int16).to(torch.int32) & 0xFFFF
    got, ref = as_int(fn()), as_int(expr(src.view(torch.uint8)))
    worst = int((got - ref).abs().max())
    assert worst <= 1, f"the torch expression differs from the kernel by {worst} code values"
    ref_us = timed(lambda: expr(src.view(torch.uint8)), max(iters // 4, 1), repeats)
    kernel = timed(fn, iters, repeats)
    alone = timed(fn, 1, 25)
    big, dst = torch.empty(COPY_BYTES, dtype=torch.uint8, device=dev), torch.empty(COPY_BYTES, dtype=torch.uint8, device=dev)
    copy = timed(lambda: dst.copy_(big), max(iters // 4, 1), repeats)
    moved = 2 * n * word
    med, copy_tbs = statistics.median(kernel), 2 * COPY_BYTES / statistics.median(copy) / 1e6
    return {"case": f"{w}x{h} {layout} {kind}", "bitdepth": depth, "colour": list(COLOUR),
            "device": torch.cuda.get_device_name(dev), "kernel_us": spread(kernel), "kernel_alone_us": spread(alone),
            "device_copy_TBs": copy_tbs, "torch_expression_us": spread(ref_us), "torch_differs_by_at_most": worst,
            "bytes_moved": moved, "achieved_TBs": moved / med / 1e6, "fraction_of_device_copy": moved / med / 1e6 / copy_tbs,
            "time_at_device_copy_us": moved / copy_tbs / 1e6,
            "slower_than_torch": statistics.median(kernel) > statistics.median(ref_us)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--limit", type=int, default=120, help="seconds a case may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "picture_colour.json"))
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
        ref = row["torch_expression_us"]
        print(f"{row['case']:26s} kernel {row['kernel_us']['median']:7.1f} us [{row['kernel_us']['min']:.1f}..."
              f"{row['kernel_us']['max']:.1f}] (alone {row['kernel_alone_us']['median']:6.1f})  torch "
              f"{ref['median']:7.1f} us{' SLOWER' if row['slower_than_torch'] else ''}  {row['bytes_moved'] / 1e6:6.1f} MB  "
              f"{row['achieved_TBs']:5.2f} TB/s of {row['device_copy_TBs']:5.2f} ({100 * row['fraction_of_device_copy']:4.1f} %)",
              flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": rows[0]["device"] if rows else None, "iters": a.iters, "repeats": a.repeats, "rows": rows}, f,
                  indent=1)
        f.write("\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
