#!/usr/bin/env python3
"""Times the picture input / output kernels (csrc/picture_ops.hip) on one 1920x1080 picture padded to 1920x1152, next to
the code paths they replace, in one process, and writes profiles/picture_io.json:

  kernels  GPU time per launch of each of the four kernels: a batch of launches captured into one HIP graph, HIP events
           around each replay (the host's enqueue rate is not in the figure), and the algorithmic bytes per second that
           time means;
  ingest   bytes of one picture in host memory -> padded tensors and originals on the device, synchronised, host clock:
           read_gop's per-picture statements (host uint8 -> float32, three float copies, stack, two pads) against one copy
           of bytes + pmctf_yuv420_u8_to_planes_f32;
  rgb out  reconstruction on the device -> (h, w, 3) uint8 array on the host, host clock: the harness's torch statements
           (round(clamp), crop, yuv_420_to_444, ycbcr2rgb, round, clip, cast, permute) on the GPU followed by .cpu()
           against pmctf_yuv420_to_rgb8_f32 + the copy of its bytes.

    python tools/time_picture_io.py [--reps 30 --warmup 5 --batch 50]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learned-pmctf_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from pMCTF.hip import ops  # noqa: E402
from pMCTF.utils.stream_helper import get_padding_size  # noqa: E402
from pMCTF.utils.util import ycbcr2rgb, yuv_420_to_444  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "picture_io.json"))
    a = ap.parse_args()
    assert a.reps >= 20 and a.warmup >= 2, "at least 20 timed repetitions after warm-up"
    h, w, psize = a.height, a.width, 128
    dev = torch.device("cuda:0")
    left, right, top, bottom = get_padding_size(h, w, p=psize)
    Hp, Wp = h + bottom, w + right
    rng = np.random.default_rng(0)
    frame = rng.integers(0, 256, h * w * 3 // 2, dtype=np.uint8)
    y8 = frame[:h * w].reshape(h, w)
    cb8 = frame[h * w:h * w + h * w // 4].reshape(h // 2, w // 2)
    cr8 = frame[h * w + h * w // 4:].reshape(h // 2, w // 2)
    rgb_host = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)

    # ---- the kernels alone
    frame_dev, rgb_dev = torch.from_numpy(frame).to(dev), torch.from_numpy(rgb_host).to(dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    rec_y = (torch.rand((1, 1, Hp, Wp), generator=g) * 280.0 - 12.0).to(dev)
    rec_c = (torch.rand((2, 1, Hp // 2, Wp // 2), generator=g) * 280.0 - 12.0).to(dev)
    n, npad = h * w, Hp * Wp
    kernels = {
        "yuv420_to_rgb8 (a)": (lambda: ops.frame_to_rgb8(rec_y, rec_c, h, w), 4 * 1.5 * n + 3 * n),
        "yuv420_u8_to_planes (b)": (lambda: ops.planes_from_u8(frame_dev, h, w, psize), 1.5 * n + 4 * 1.5 * (npad + n)),
        "rgb8_to_yuv420 (c)": (lambda: ops.rgb8_to_yuv420(rgb_dev), 3 * n + 1.5 * n),
        "planes_to_u8 (luma)": (lambda: ops.planes_to_u8(rec_y, h, w), 4 * n + n),
    }
    out = {"device": torch.cuda.get_device_name(0), "picture": [h, w], "padded": [Hp, Wp], "reps": a.reps,
           "warmup": a.warmup, "batch": a.batch, "runtime_copy_TBps": RUNTIME_COPY_TBS, "kernels": {}, "paths": {}}
    for name, (fn, nbytes) in kernels.items():
        s = gpu_time(fn, a.reps, a.warmup, a.batch)
        s.update(algorithmic_bytes=int(nbytes), algorithmic_TBps=nbytes / s["median"] / 1e12)
        out["kernels"][name] = s

    # ---- ingest: what read_gop did per picture before, against the copy of bytes and one launch
    def ingest_host():
        y, cb, cr = (torch.from_numpy(p).float() for p in (y8, cb8, cr8))
        luma = y[None, None].to(dev)
        chroma = torch.stack((cb, cr))[:, None].to(dev)
        return (F.pad(luma, (left, right, top, bottom)),
                F.pad(chroma, (left // 2, right // 2, top // 2, bottom // 2)), luma, chroma)

    def ingest_device():
        return ops.planes_from_u8(torch.from_numpy(frame).to(dev), h, w, psize)

    def ingest_copy_only():
        return torch.from_numpy(frame).to(dev)

    same = all(torch.equal(p, q) for p, q in zip(ingest_host(), ingest_device()))
    out["paths"]["ingest, read_gop's host statements"] = wall_time(ingest_host, a.reps, a.warmup)
    out["paths"]["ingest, bytes + kernel (b)"] = wall_time(ingest_device, a.reps, a.warmup)
    out["paths"]["ingest, the copy of bytes alone"] = wall_time(ingest_copy_only, a.reps, a.warmup)
    out["ingest_paths_agree"] = bool(same)

    # ---- RGB out: the harness's statements in torch on the GPU + .cpu(), against kernel (a) + the copy of its bytes
    def rgb_torch():
        ry = torch.round(rec_y.clamp(0, 255.0))[:, :, :h, :w]
        rc = torch.round(rec_c.clamp(0, 255.0))[:, :, :h // 2, :w // 2]
        rgb = torch.round(ycbcr2rgb(yuv_420_to_444((ry, rc[0:1], rc[1:2]))))
        return rgb.clamp(0, 255).to(torch.uint8)[0].permute(1, 2, 0).contiguous().cpu().numpy()

    def rgb_kernel():
        return ops.frame_to_rgb8(rec_y, rec_c, h, w).cpu().numpy()

    out["rgb_paths_agree"] = bool(np.array_equal(rgb_torch(), rgb_kernel()))
    out["paths"]["rgb out, torch statements on the GPU + .cpu()"] = wall_time(rgb_torch, a.reps, a.warmup)
    out["paths"]["rgb out, kernel (a) + copy"] = wall_time(rgb_kernel, a.reps, a.warmup)

    us = lambda s: f"{s['median'] * 1e6:.1f} ({s['min'] * 1e6:.1f}-{s['max'] * 1e6:.1f})"
    print(f"{w}x{h} padded to {Wp}x{Hp}, {out['device']}; median (min-max) of {a.reps} repetitions after {a.warmup} warm-up")
    print("| kernel | GPU time per launch, us | algorithmic bytes, MB | TB/s (runtime copy: %.1f) |" % RUNTIME_COPY_TBS)
    print("|---|---|---|---|")
    for name, s in out["kernels"].items():
        print(f"| {name} | {us(s)} | {s['algorithmic_bytes'] / 1e6:.1f} | {s['algorithmic_TBps']:.2f} |")
    print("| path | wall time per picture, us |")
    print("|---|---|")
    for name, s in out["paths"].items():
        print(f"| {name} | {us(s)} |")
    print(f"ingest paths agree bit for bit: {out['ingest_paths_agree']}; RGB paths agree byte for byte: {out['rgb_paths_agree']}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=2)
        f.write("\n")
    if not (out["ingest_paths_agree"] and out["rgb_paths_agree"]):
        sys.exit("the timed paths must compute the same pictures")


if __name__ == "__main__":
    main()
