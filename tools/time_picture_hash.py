#!/usr/bin/env python3
"""Times the picture hash (csrc/picture_hash.hip) on one 1920x1080 picture padded to 1920x1152, at both levels, next to the
path it replaces, in one process, and writes profiles/picture_hash.json:

  kernels  GPU time of pmctf_crc32_segments (both launches) per picture: the u8 level (the three cropped 8-bit planes,
           3.1 MB), the f32 level's additional tensors (padded float32 luma and chroma, 13.3 MB), and a GOP of eight
           pictures at the f32 level in one call (40 ranges), per picture.  A batch of calls is captured into one HIP graph
           (a chain, no branches) and each replay is bracketed by events, as tools/time_picture_io.py does; the bytes per
           second that time means are given next to it;
  paths    per picture, host clock, synchronised: ops.crc32 as picture_hashes calls it (table to the device, two launches,
           4 bytes per range back) against the copy of the same tensors to the host followed by zlib.crc32.

    python tools/time_picture_hash.py [--reps 30 --warmup 5 --batch 20]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learned-pmctf_amd"))
import torch  # noqa: E402

from pMCTF.hip import lib, ops  # noqa: E402
from pMCTF.utils.stream_helper import get_padding_size  # noqa: E402


def stats(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "n": len(ts)}


def gpu_time(fn, reps, warmup, batch):
    """seconds per call of fn on the device: `batch` calls in one captured graph, events around each replay"""
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


def wall_time(fn, reps, warmup):
    ts = []
    for k in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            ts.append(time.perf_counter() - t0)
    return stats(ts)


def launcher(tensors):
    """the library call alone on prepared device arguments (nothing a graph capture refuses) -> (fn, out, slices)"""
    dev = tensors[0].device
    lengths = [t.numel() * t.element_size() for t in tensors]
    table = []
    for t, n in zip(tensors, lengths):
        table += [t.data_ptr(), n]
    segs = torch.tensor(table, dtype=torch.int64).to(dev)
    out = torch.empty(len(tensors), dtype=torch.int32, device=dev)
    slices = max(1, min(128, -(-max(lengths) // (8 * ops.CRC32_TILE_BYTES))))          # ops.crc32's default

    def fn():
        lib.check(lib.hip().pmctf_crc32_segments(C.c_void_p(segs.data_ptr()), len(tensors), slices,
                                                 C.c_void_p(out.data_ptr()), ops._stream()), "crc32")
    fn.keep = (segs, tensors)
    return fn, out, slices


def host_crc(tensors):
    return [zlib.crc32(memoryview(t.cpu().numpy()).cast("B")) for t in tensors]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "picture_hash.json"))
    a = ap.parse_args()
    assert a.reps >= 20 and a.warmup >= 2, "at least 20 timed repetitions after warm-up"
    h, w, psize, gop = a.height, a.width, 128, 8
    dev = torch.device("cuda:0")
    _, right, _, bottom = get_padding_size(h, w, p=psize)
    Hp, Wp = h + bottom, w + right
    g = torch.Generator(device="cpu").manual_seed(0)

    def picture():
        rec_y = (torch.rand((1, 1, Hp, Wp), generator=g) * 280.0 - 12.0).to(dev)
        rec_c = (torch.rand((2, 1, Hp // 2, Wp // 2), generator=g) * 280.0 - 12.0).to(dev)
        c8 = ops.planes_to_u8(rec_c, h // 2, w // 2)
        return {"u8": [ops.planes_to_u8(rec_y, h, w), c8[0], c8[1]], "f32": [rec_y, rec_c]}

    pics = [picture() for _ in range(gop)]
    cases = {"u8 level: 3 ranges": pics[0]["u8"],
             "f32 level's float tensors: 2 ranges": pics[0]["f32"],
             "f32 level, one picture: 5 ranges": pics[0]["u8"] + pics[0]["f32"],
             f"f32 level, GOP of {gop} in one call: {5 * gop} ranges, per picture": sum((p["u8"] + p["f32"] for p in pics), [])}
    out = {"device": torch.cuda.get_device_name(0), "picture": [h, w], "padded": [Hp, Wp], "reps": a.reps, "warmup": a.warmup,
           "batch": a.batch, "kernels": {}, "paths": {}}
    agree = True
    for name, tensors in cases.items():
        pictures = gop if "GOP" in name else 1
        nbytes = sum(t.numel() * t.element_size() for t in tensors) // pictures
        fn, res, slices = launcher(tensors)
        s = gpu_time(fn, a.reps, a.warmup, a.batch)
        s = {k: (v / pictures if k != "n" else v) for k, v in s.items()}
        s.update(bytes=int(nbytes), slices=slices, TBps=nbytes / s["median"] / 1e12)
        out["kernels"][name] = s
        agree &= [v & 0xffffffff for v in res.cpu().tolist()] == host_crc(tensors)

    for level, tensors in (("u8", pics[0]["u8"]), ("f32", pics[0]["u8"] + pics[0]["f32"])):
        agree &= ops.crc32(tensors) == host_crc(tensors)
        out["paths"][f"{level} level, ops.crc32 on the device"] = wall_time(lambda: ops.crc32(tensors), a.reps, a.warmup)
        out["paths"][f"{level} level, copy to the host + zlib.crc32"] = wall_time(lambda: host_crc(tensors), a.reps, a.warmup)
    out["device_and_host_agree"] = bool(agree)

    us = lambda s: f"{s['median'] * 1e6:.1f} ({s['min'] * 1e6:.1f}-{s['max'] * 1e6:.1f})"
    print(f"{w}x{h} padded to {Wp}x{Hp}, {out['device']}; median (min-max) of {a.reps} repetitions after {a.warmup} warm-up")
    print("| pmctf_crc32_segments | GPU time per picture, us | MB per picture | TB/s |")
    print("|---|---|---|---|")
    for name, s in out["kernels"].items():
        print(f"| {name} | {us(s)} | {s['bytes'] / 1e6:.1f} | {s['TBps']:.2f} |")
    print("| path | wall time per picture, us |")
    print("|---|---|")
    for name, s in out["paths"].items():
        print(f"| {name} | {us(s)} |")
    print(f"device and host values agree: {out['device_and_host_agree']}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=2)
        f.write("\n")
    if not out["device_and_host_agree"]:
        sys.exit("the timed paths must compute the same values")


if __name__ == "__main__":
    main()
