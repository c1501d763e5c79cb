#!/usr/bin/env python3
"""python tools/math_sweep.py --host [function ...]

All 2^32 float32 bit patterns through learned-pmctf_amd/csrc/pm_device_math.h compiled for the HOST (tests/math_sweep.py
HostBuild: g++ behind a stub hip/hip_runtime.h), against the oracle map of every function — for whoever regenerates a
table or a generated header.  Not part of the suite, which runs the same comparison on the stratified set S without a GPU
(tests/test_math_sweep_cpu.py) and on all 2^32 inputs on the GPU (tests/test_gpu_math_sweep.py).
Measured: 73-105 s per function on 8 CPU threads with the oracle's maps single-threaded and fanned out from Python; the
maps now run on PM_ORACLE_THREADS threads themselves.  Subnormal and NaN inputs run at about 5 M/s per thread, the rest
at 80-200 M/s.  Exit status 1 on any mismatch."""
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, p))

import numpy as np  # noqa: E402

import math_sweep as ms  # noqa: E402


def main(argv):
    if "--host" not in argv:
        print(__doc__)
        return 2
    names = [a for a in argv if not a.startswith("--")] or [n for n, _, _ in ms.FUNCTIONS]
    bad = 0
    with tempfile.TemporaryDirectory() as td:
        host = ms.HostBuild(td)
        for name in names:
            t0, count, exempt, first_bad = time.time(), 0, 0, None
            for first, n in ms.chunks():
                x = ms.chunk_bits(first, n).view(np.float32)
                got, want = host.probe(name, None, first, n).view(np.uint32), ms.SPEC[name](x).view(np.uint32)
                c, i, e = ms.compare(got, want)
                if c and first_bad is None:
                    first_bad = f"first at input {first + i:#010x}: host build {int(got[i]):#010x}, oracle {int(want[i]):#010x}"
                count, exempt = count + c, exempt + e
            print(f"{name}: {count} mismatches on 2^32 inputs, {exempt} both-NaN payload differences, "
                  f"{time.time() - t0:.0f} s" + (f"; {first_bad}" if first_bad else ""), flush=True)
            bad += count
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
