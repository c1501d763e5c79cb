#!/usr/bin/env python3
"""Times the per-frame quality record (Y/Cb/Cr/YUV/RGB-PSNR + MS-SSIM) two ways in one process and writes
profiles/quality_metrics_1080p.txt:

  (i)  the path that existed before the quality kernels: pmctf_gop.gop_psnr + rgb_psnr on the GPU, plus the float32
       restatement of MS-SSIM (tests/quality_restatement.py) on the GPU as the stand-in for the third-party package;
  (ii) pMCTF.hip.ops.frame_quality.

Both warmed, alternated frame by frame, timed with a host clock around work that ends in the copy to the host.  Launches
and host synchronisations per frame are counted on one frame (torch profiler / wrapped Tensor methods).  For (ii) the
kernels alone are timed with events on the stream, next to the bytes the algorithm must move.

    python tools/time_quality.py [--width 1920 --height 1080 --frames 50 --warmup 5]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learned-pmctf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import pmctf_gop  # noqa: E402
import quality_restatement as qr  # noqa: E402
from pMCTF.hip import lib, ops  # noqa: E402

HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.29         # MI355X: specification, measured device copy


def algorithmic_bytes(h, w, msssim=True):
    """what the algorithm must move: the front end reads 2 x 1.5 float planes and writes 2 x 3; scale i reads 6 planes of
    its size and writes 6 of the next one's (the last writes none)"""
    sizes = qr.scale_sizes(h, w)
    total = 4 * (2 * 1.5 + (2 * 3 if msssim else 0)) * h * w
    if msssim:
        for i, (a, b) in enumerate(sizes):
            total += 4 * 6 * a * b
            if i + 1 < len(sizes):
                total += 4 * 6 * sizes[i + 1][0] * sizes[i + 1][1]
    return int(total)


def torch_path(rec_y, rec_c, org_y, org_c, h, w):
    p = pmctf_gop.gop_psnr([(rec_y, rec_c, None)], [(org_y, org_c)], h, w)[0]
    ry = torch.round(rec_y.clamp(0, 255.0))[:, :, :h, :w]
    rc = torch.round(rec_c.clamp(0, 255.0))[:, :, :h // 2, :w // 2]
    p["rgb"] = pmctf_gop.rgb_psnr(ry, rc, org_y, org_c)
    from pMCTF.utils.util import ycbcr2rgb, yuv_420_to_444
    rgb = lambda y, c: torch.round(ycbcr2rgb(yuv_420_to_444((y, c[0:1], c[1:2]))))
    p["msssim"], _ = qr.ms_ssim(rgb(ry, rc), rgb(org_y, org_c), dtype=torch.float32, device=rec_y.device)
    return p


class SyncCounter:
    """counts the Tensor methods that wait for the device"""
    NAMES = ("item", "tolist", "cpu")

    def __enter__(self):
        self.n = 0
        self.saved = {k: getattr(torch.Tensor, k) for k in self.NAMES}
        for k, fn in self.saved.items():
            def wrapped(t, *a, _fn=fn, **kw):
                if t.is_cuda:
                    self.n += 1
                return _fn(t, *a, **kw)
            setattr(torch.Tensor, k, wrapped)
        return self

    def __exit__(self, *exc):
        for k, fn in self.saved.items():
            setattr(torch.Tensor, k, fn)


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev = getattr(torch.autograd.DeviceType, "CUDA")
        n = sum(1 for e in prof.events() if e.device_type == dev and "copy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n if n else None
    except Exception as e:          # the profiler is a convenience here, not part of the measurement
        print(f"(launch count unavailable: {e})")
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quality_metrics_1080p.txt"))
    a = ap.parse_args()
    assert a.frames >= 50 and a.warmup >= 2, "at least 50 timed frames each after warm-up"
    h, w = a.height, a.width
    Hp, Wp = -(-h // 128) * 128, -(-w // 128) * 128
    dev = torch.device("cuda:0")
    pics = [tuple(t.to(dev) for t in qr.quality_case(Hp, Wp, h, w, 3.0, seed=k)) for k in range(4)]
    t_i, t_ii = [], []
    last = None
    for k in range(a.warmup + a.frames):
        p = pics[k % len(pics)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ri = torch_path(*p, h, w)
        t1 = time.perf_counter()
        rii = ops.frame_quality(*p, h, w)
        t2 = time.perf_counter()
        if k >= a.warmup:
            t_i.append(t1 - t0)
            t_ii.append(t2 - t1)
        last = (ri, rii)
    with SyncCounter() as si:
        torch_path(*pics[0], h, w)
    with SyncCounter() as sii:
        ops.frame_quality(*pics[0], h, w)
    li = count_launches(lambda: torch_path(*pics[0], h, w))
    lii = count_launches(lambda: ops.frame_quality(*pics[0], h, w))

    # the kernels of (ii) alone: events on the stream around the C entry point
    L = lib.hip()
    scratch = torch.empty(L.pmctf_msssim_scratch_floats(h, w), dtype=torch.float32, device=dev)
    out = torch.empty(ops.QUALITY_OUT_DOUBLES, dtype=torch.float64, device=dev)
    vp = lambda t: C.c_void_p(t.data_ptr())
    st = torch.cuda.current_stream()
    kern = {}
    for ms in (1, 0):
        ts = []
        for k in range(a.warmup + a.frames):
            p = pics[k % len(pics)]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            rc = L.pmctf_frame_quality_f32(vp(p[0]), vp(p[1]), vp(p[2]), vp(p[3]), Hp, Wp, h, w, ms, vp(scratch), vp(out),
                                           C.c_void_p(st.cuda_stream))
            e1.record(st)
            assert rc == 0
            e1.synchronize()
            if k >= a.warmup:
                ts.append(e0.elapsed_time(e1) * 1e-3)
        kern[ms] = ts

    med = statistics.median
    lines = [
        f"quality record of one {w}x{h} frame (padded {Wp}x{Hp}), {torch.cuda.get_device_name(0)}",
        f"{a.frames} timed frames each after {a.warmup} warm-up frames, the two paths alternated frame by frame in one process;",
        "host clock around work that ends in the copy to the host; median [min .. max] ms per frame",
        f"(i)  gop_psnr + rgb_psnr + float32 MS-SSIM restatement in torch on the GPU: {med(t_i) * 1e3:.3f} "
        f"[{min(t_i) * 1e3:.3f} .. {max(t_i) * 1e3:.3f}] ms, launches per frame {li}, host synchronisations per frame {si.n}",
        f"(ii) ops.frame_quality (HIP kernels):                                    {med(t_ii) * 1e3:.3f} "
        f"[{min(t_ii) * 1e3:.3f} .. {max(t_ii) * 1e3:.3f}] ms, launches per frame {lii} (the library's 7: front end, 5 "
        f"scales, final sums; the profiler also counts the runtime's kernel behind the copy to the host), host synchronisations "
        f"per frame {sii.n}",
        f"ratio (i) / (ii) of the medians: {med(t_i) / med(t_ii):.2f}",
        f"last frame, (i): {last[0]}",
        f"last frame, (ii): { {k: v for k, v in last[1].items() if k != 'sse'} }",
        "",
        "kernels of (ii) alone (events on the stream around pmctf_frame_quality_f32, no copy):",
    ]
    for ms, name in ((1, "PSNR + MS-SSIM"), (0, "PSNR only")):
        b = algorithmic_bytes(h, w, bool(ms))
        t = med(kern[ms])
        lines.append(f"  {name}: {t * 1e6:.1f} us [{min(kern[ms]) * 1e6:.1f} .. {max(kern[ms]) * 1e6:.1f}], algorithmic bytes "
                     f"{b / 1e6:.1f} MB -> {b / t / 1e12:.3f} TB/s algorithmic bytes per second "
                     f"(HBM: {HBM_SPEC_TBS} TB/s specification, {HBM_COPY_TBS} TB/s measured copy)")
    lines += [
        "The working set of a 1080p frame (about 75 MB) fits the 256 MiB Infinity Cache: the figure above is algorithmic bytes",
        "per second, not HBM utilisation.",
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    if not (med(t_ii) < med(t_i) and sii.n == 1):
        sys.exit("the quality kernels must be faster than the torch path, with one host synchronisation per frame")


if __name__ == "__main__":
    main()
