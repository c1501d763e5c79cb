#!/usr/bin/env python3
"""Writes tests/golden/reference_scale_index_boundaries.npz: scales and the CDF rows the reference's
GaussianEncoder.build_indexes gives them (entropy_models.py:269-273: trunc(clamp((log(max(s, 1e-5)) - lmin) / step,
0, 255)) in torch's CPU arithmetic, GaussianTables.build_indexes_torch) — the known answers that pin every copy of the
row selection (ew_ops.hip / decode_ops.hip scale_index, the LL decode kernels, GaussianTables.build_indexes_cdef) where
they can disagree: one ulp either side of a row boundary.

Contents: for every boundary exp(lmin + k * step), k = 1 .. 255, the f32 values from 64 ulps below to 64 ulps above;
0, -0, negatives, -inf and denormals; 1e-5 +- 4 ulps; scale_max +- 4 ulps, values above exp(lmax), 1e10 and +inf.  NaN
stays out: the reference's .int() of NaN is undefined (the kernels map it to row 0, which the GPU test asserts on its
own).  torch.log runs over whole vectors inside one thread's slice (chunks of a multiple of 64 elements, well below
ATen's grain size), so that no element goes through the scalar tail.  Build-container tool; needs only torch and the
oracle package."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from pmctf_oracle.entropy import GaussianTables  # noqa: E402

ULPS = 64
CHUNK = 4096                          # a multiple of 64 and far below ATen's grain size (32768)


def around(v, n):
    """the f32 values from n ulps below to n ulps above the f32 nearest v (v > 0)"""
    b = np.array([v], np.float32).view(np.int32)[0]
    return (b + np.arange(-n, n + 1, dtype=np.int32)).view(np.float32)


def rows_torch(g, x):
    pad = (-x.size) % 64
    xp = np.concatenate([x, np.full(pad, x[0], np.float32)])
    out = [g.build_indexes_torch(torch.from_numpy(xp[i:i + CHUNK].copy())).numpy() for i in range(0, xp.size, CHUNK)]
    return np.concatenate(out)[:x.size]


def main():
    torch.set_num_threads(1)
    g = GaussianTables()
    bounds = [np.exp(g.log_scale_min + k * g.log_scale_step) for k in range(1, g.scale_level)]
    parts = [around(b, ULPS) for b in bounds]
    specials = np.array([0.0, -0.0, -1e-30, -1.0, -64.0, -1e10, -np.inf, 1e-45, 1e-42, 1e-40, 1.1754942e-38,
                         1.1754944e-38, 1e-30, 1e-10, 1e-6, 2e-3, 100.0, 1000.0, 1e6, 1e10, 3.4028235e38, np.inf],
                        np.float32)
    parts += [specials, around(1e-5, 4), around(g.scale_max, 4), around(np.exp(g.log_scale_max), 4)]
    x = np.concatenate(parts).astype(np.float32)
    assert not np.isnan(x).any()
    rows = rows_torch(g, x)
    assert rows.min() == 0 and rows.max() == g.scale_level - 1
    out = os.path.join(ROOT, "tests", "golden", "reference_scale_index_boundaries.npz")
    np.savez_compressed(out, scale_x=x, scale_row=rows.astype(np.int16))
    print(out, x.size, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
