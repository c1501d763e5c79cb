#!/usr/bin/env python3
"""Times the pixel-layout kernels (csrc/picture_layout.hip, pmctf_layout.Unpacker / Packer) per picture, next to the device
copy and to the torch expression a user would otherwise write, writes profiles/picture_layout.json and prints the table of
DESIGN 5n:

  kernel    one launch per picture into a destination allocated once, HIP events around `--iters` launches in a row on the
            stream, after a warm-up, repeated `--repeats` times: median and spread of the per-picture time; and one launch
            alone between two events (median of 25);
  copy      Tensor.copy_ of a 256 MiB device buffer, timed the same way in the same process: the device copy's rate;
  torch     for the unpack cases, the same unpacking written with strided slices, shifts and torch.cat on the device (its
            result is checked against the kernel's once), timed the same way;
  bytes     surface plus planar picture, each touched once, over the kernel time.

Every case runs in a child process of its own under a time limit (`--limit` seconds); the first one that fails or runs out
of time ends the run, and the cases measured so far are written.

    python tools/time_picture_layout.py [--iters 200 --repeats 7 --out profiles/picture_layout.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learned-pmctf_amd"))

CASES = [(w, h, layout, kind) for w, h in ((1920, 1080), (3840, 2160)) for layout in ("nv12", "p010", "uyvy", "v210")
         for kind in ("unpack", "pack")]
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


def torch_unpack(layout, w, h):
    """surface (uint8 device tensor) -> the planar picture as torch ops; 16-bit results as int16 bit patterns"""
    import torch
    n = h * w
    if layout == "nv12":
        def f(s):
            c = s[n:].view(h // 2, w // 2, 2)
            return torch.cat([s[:n], c[..., 0].reshape(-1), c[..., 1].reshape(-1)])
    elif layout == "p010":
        def f(s):
            v = ((s.view(torch.int16).to(torch.int32) & 0xFFFF) >> 6).to(torch.int16)
            c = v[n:].view(h // 2, w // 2, 2)
            return torch.cat([v[:n], c[..., 0].reshape(-1), c[..., 1].reshape(-1)])
    elif layout == "uyvy":
        def f(s):
            t = s.view(h, w // 2, 4)
            return torch.cat([t[..., 1::2].reshape(-1), t[..., 0].reshape(-1), t[..., 2].reshape(-1)])
    else:
        groups = (w + 5) // 6

        def f(s):
            q = s.view(torch.int32).view(h, -1)[:, :4 * groups].reshape(h, groups, 4)
            a, b, c = q & 1023, (q >> 10) & 1023, (q >> 20) & 1023
            y = torch.stack([b[..., 0], a[..., 1], c[..., 1], b[..., 2], a[..., 3], c[..., 3]], dim=2).reshape(h, -1)[:, :w]
            cb = torch.stack([a[..., 0], b[..., 1], c[..., 2]], dim=2).reshape(h, -1)[:, :w // 2]
            cr = torch.stack([c[..., 0], a[..., 2], b[..., 3]], dim=2).reshape(h, -1)[:, :w // 2]
            return torch.cat([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)]).to(torch.int16)
    return f


def one_case(index, iters, repeats, device):
    import torch
    import pmctf_chroma
    import pmctf_layout
    w, h, layout, kind = CASES[index]
    dev = torch.device(device)
    info = pmctf_layout.LAYOUTS[layout]
    b = info["bitdepth"]
    dtype, word = (torch.uint8, 1) if b == 8 else (torch.uint16, 2)
    n = pmctf_chroma.frame_samples(w, h, info["chroma_format"])
    g = torch.Generator().manual_seed(b)
    frame = torch.randint(0, 1 << b, (n,), generator=g, dtype=torch.int32).to(dtype).to(dev)
    unpack, pack = pmctf_layout.Unpacker(layout, w, h), pmctf_layout.Packer(layout, w, h)
    surface = pack(frame)
    assert torch.equal(unpack(surface).view(torch.uint8), frame.view(torch.uint8)), "unpack(pack(p)) != p"
    ref = None
    if kind == "unpack":
        out = torch.empty_like(frame)
        fn = lambda: unpack(surface, out=out)
        expr = torch_unpack(layout, w, h)
        assert torch.equal(expr(surface).view(torch.uint8), frame.view(torch.uint8)), "the torch expression disagrees"
        ref = timed(lambda: expr(surface), max(iters // 4, 1), repeats)
    else:
        out = torch.empty_like(surface)
        fn = lambda: pack(frame, out=out)
    kernel = timed(fn, iters, repeats)
    alone = timed(fn, 1, 25)
    big, dst = torch.empty(COPY_BYTES, dtype=torch.uint8, device=dev), torch.empty(COPY_BYTES, dtype=torch.uint8, device=dev)
    copy = timed(lambda: dst.copy_(big), max(iters // 4, 1), repeats)
    moved = surface.numel() + n * word
    med, copy_tbs = statistics.median(kernel), 2 * COPY_BYTES / statistics.median(copy) / 1e6
    return {"case": f"{w}x{h} {layout} {kind}", "bitdepth": b, "device": torch.cuda.get_device_name(dev),
            "kernel_us": spread(kernel), "kernel_alone_us": spread(alone), "device_copy_TBs": copy_tbs,
            "torch_expression_us": None if ref is None else spread(ref), "bytes_moved": moved,
            "achieved_TBs": moved / med / 1e6, "fraction_of_device_copy": moved / med / 1e6 / copy_tbs,
            "time_at_device_copy_us": moved / copy_tbs / 1e6,
            "slower_than_torch_beyond_spread": ref is not None and min(kernel) > statistics.median(ref)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--limit", type=int, default=120, help="seconds a case may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "picture_layout.json"))
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
              f"{'      -' if ref is None else format(ref['median'], '7.1f')} us  {row['bytes_moved'] / 1e6:6.1f} MB  "
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
