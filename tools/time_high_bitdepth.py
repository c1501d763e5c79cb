#!/usr/bin/env python3
"""Times the high-bit-depth picture kernels (csrc/picture_ops.hip at uint16_t, csrc/picture_hbd.hip) at 1920x1080 and
3840x2160, 10 bits, next to the code paths they stand beside, in one process, and writes profiles/high_bitdepth_io.json:

  kernels  GPU time per launch of each of the three kernels: a batch of launches captured into one HIP graph, HIP events
           around each replay (the host's enqueue rate is not in the figure), and the algorithmic bytes per second that
           time means;
  ingest   samples of one picture in host memory -> padded tensors and originals on the device, synchronised, host clock:
           read_gop's per-picture statements (host uint16 -> float32, scale, three float copies, stack, two pads) against
           one copy of the 16-bit samples + pmctf_yuv420_u16_to_planes_f32;
  sse      the three error sums on the host as integers, host clock: ops.frame_sse_hbd (one launch, 24 bytes copied)
           against the same sums as torch statements on the GPU (scale, clamp, round, crop, subtract in int64, square, sum).

    python tools/time_high_bitdepth.py [--reps 30 --warmup 5 --batch 50]
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
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from pMCTF.hip import lib, ops  # noqa: E402
from pMCTF.utils.stream_helper import get_padding_size  # noqa: E402

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


def one_size(h, w, b, a, dev):
    psize, s = 128, b - 8
    left, right, top, bottom = get_padding_size(h, w, p=psize)
    Hp, Wp = h + bottom, w + right
    rng = np.random.default_rng(0)
    frame = rng.integers(0, 1 << b, h * w * 3 // 2, dtype=np.uint16)
    y16 = frame[:h * w].reshape(h, w)
    cb16 = frame[h * w:h * w + h * w // 4].reshape(h // 2, w // 2)
    cr16 = frame[h * w + h * w // 4:].reshape(h // 2, w // 2)
    frame_dev = torch.from_numpy(frame).to(dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    rec_y = (torch.rand((1, 1, Hp, Wp), generator=g) * 280.0 - 12.0).to(dev)
    rec_c = (torch.rand((2, 1, Hp // 2, Wp // 2), generator=g) * 280.0 - 12.0).to(dev)
    _, _, org_y, org_c = ops.planes_from_u16(frame_dev, h, w, b, psize)
    sse_out = torch.empty(3, dtype=torch.int64, device=dev)
    L = lib.hip()
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def sse_launch():                                  # ops.frame_sse_hbd without its copy to the host
        rc = L.pmctf_frame_sse_u16_f32(ptr(rec_y), ptr(rec_c), ptr(org_y), ptr(org_c), Hp, Wp, h, w, b, ptr(sse_out),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0

    n, npad = h * w, Hp * Wp
    kernels = {
        "yuv420_u16_to_planes": (lambda: ops.planes_from_u16(frame_dev, h, w, b, psize), 2 * 1.5 * n + 4 * 1.5 * (npad + n)),
        "planes_to_u16 (luma)": (lambda: ops.planes_to_u16(rec_y, h, w, b), 4 * n + 2 * n),
        "frame_sse_u16 (+ its clear)": (sse_launch, 2 * 4 * 1.5 * n),
    }
    out = {"picture": [h, w], "padded": [Hp, Wp], "bitdepth": b, "kernels": {}, "paths": {}}
    for name, (fn, nbytes) in kernels.items():
        t = gpu_time(fn, a.reps, a.warmup, a.batch)
        t.update(algorithmic_bytes=int(nbytes), algorithmic_TBps=nbytes / t["median"] / 1e12)
        out["kernels"][name] = t

    def ingest_host():
        y, cb, cr = (torch.from_numpy(p.astype(np.float32)) * 2.0 ** -s for p in (y16, cb16, cr16))
        luma = y[None, None].to(dev)
        chroma = torch.stack((cb, cr))[:, None].to(dev)
        return (F.pad(luma, (left, right, top, bottom)),
                F.pad(chroma, (left // 2, right // 2, top // 2, bottom // 2)), luma, chroma)

    def ingest_device():
        return ops.planes_from_u16(torch.from_numpy(frame).to(dev), h, w, b, psize)

    out["ingest_paths_agree"] = bool(all(torch.equal(p, q) for p, q in zip(ingest_host(), ingest_device())))
    out["paths"]["ingest, read_gop's host statements"] = wall_time(ingest_host, a.reps, a.warmup)
    out["paths"]["ingest, 16-bit samples + kernel"] = wall_time(ingest_device, a.reps, a.warmup)

    up, top_v = float(1 << s), float((1 << b) - 1)

    def sse_torch():
        sums = []
        for rec, org, hh, ww in ((rec_y, org_y, h, w), (rec_c[0:1], org_c[0:1], h // 2, w // 2),
                                 (rec_c[1:2], org_c[1:2], h // 2, w // 2)):
            v = torch.round((rec * up).clamp(0.0, top_v))[:, :, :hh, :ww].to(torch.int64)
            d = v - (org * up).to(torch.int64)
            sums.append((d * d).sum())
        return tuple(int(x) for x in torch.stack(sums).cpu().tolist())

    def sse_kernel():
        return ops.frame_sse_hbd(rec_y, rec_c, org_y, org_c, h, w, b)["sse"]

    out["sse_paths_agree"] = bool(sse_torch() == sse_kernel())
    out["paths"]["sse, torch statements on the GPU + .cpu()"] = wall_time(sse_torch, a.reps, a.warmup)
    out["paths"]["sse, frame_sse_hbd"] = wall_time(sse_kernel, a.reps, a.warmup)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--bitdepth", type=int, default=10)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "high_bitdepth_io.json"))
    a = ap.parse_args()
    assert a.reps >= 20 and a.warmup >= 2, "at least 20 timed repetitions after warm-up"
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "batch": a.batch,
           "runtime_copy_TBps": RUNTIME_COPY_TBS, "sizes": []}
    us = lambda t: f"{t['median'] * 1e6:.1f} ({t['min'] * 1e6:.1f}-{t['max'] * 1e6:.1f})"
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        r = one_size(h, w, a.bitdepth, a, dev)
        out["sizes"].append(r)
        print(f"{w}x{h} padded to {r['padded'][1]}x{r['padded'][0]}, {a.bitdepth} bits, {out['device']}; median (min-max) of "
              f"{a.reps} repetitions after {a.warmup} warm-up")
        print("| kernel | GPU time per launch, us | algorithmic bytes, MB | TB/s (runtime copy: %.1f) |" % RUNTIME_COPY_TBS)
        print("|---|---|---|---|")
        for name, t in r["kernels"].items():
            print(f"| {name} | {us(t)} | {t['algorithmic_bytes'] / 1e6:.1f} | {t['algorithmic_TBps']:.2f} |")
        print("| path | wall time per picture, us |")
        print("|---|---|")
        for name, t in r["paths"].items():
            print(f"| {name} | {us(t)} |")
        print(f"ingest paths agree bit for bit: {r['ingest_paths_agree']}; error sums agree: {r['sse_paths_agree']}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=2)
        f.write("\n")
    if not all(r["ingest_paths_agree"] and r["sse_paths_agree"] for r in out["sizes"]):
        sys.exit("the timed paths must compute the same values")


if __name__ == "__main__":
    main()
