#!/usr/bin/env python3
"""Runs pm_flow_warp, the CPU twin of flow_warp_kernel, under the address and undefined-behaviour sanitizers on every
flow_warp case of tests/edge_values.py — both images x the flow kinds (normal, integer, half-integer, +0, -0, +-1e30, +-inf,
NaN) x shared / per-plane fields x both signs, on the four planes of the GPU test and the 1x7 and 7x1 planes the GPU entry
refuses: 224 cases.  A stand-alone program (tools/flow_warp_sanitize.c, with the build line), nothing loaded into python.
CPU only; DESIGN.md section 6e quotes its result.  Usage: python tools/flow_warp_sanitize.py"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import edge_values as ev  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as td:
        path, exe, n = os.path.join(td, "cases.bin"), os.path.join(td, "flow_warp_sanitize"), 0
        with open(path, "wb") as f:
            for shape in ev.WARP_PLANES + ev.WARP_DEGENERATE:
                N, C, H, W = shape
                lx, ly = ev.lin_tables(H, W)
                for image in ev.IMAGES.values():
                    im = image(shape)
                    for kind in ev.FLOWS:
                        for fn in sorted({1, N}):
                            for sign in (1.0, -1.0):
                                fl = ev.flow(kind, fn, H, W) * np.float32(sign)
                                f.write(np.array([N, C, H, W, fn], np.int32).tobytes())
                                for a in (im, fl, lx, ly):
                                    f.write(np.ascontiguousarray(a, np.float32).tobytes())
                                n += 1
        subprocess.check_call([os.environ.get("CC", "gcc"), "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-march=x86-64-v3",
                               "-pthread", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                               os.path.join(ROOT, "tools", "flow_warp_sanitize.c"), os.path.join(ROOT, "oracle", "c", "pm_ops.c"),
                               "-lm", "-o", exe])
        out = subprocess.run([exe, path], capture_output=True, text=True)
        print(out.stdout + out.stderr, end="")
        assert out.returncode == 0 and out.stdout.startswith(f"{n} cases"), "the sanitizers reported, or a case was not read"


if __name__ == "__main__":
    main()
