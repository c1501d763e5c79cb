"""Helper of test_math_sweep_cpu.py, test_gpu_math_sweep.py and tools/math_sweep.py (not collected by pytest): the scalar
functions of learned-pmctf_amd/csrc/pm_device_math.h against the oracle's maps, input by input.

  FUNCTIONS        probe code of pmctf_math_probe_f32 <-> the oracle map that specifies it
  chunks()         all 2^32 float32 bit patterns, 2^26 per chunk
  stratified()     the fixed set S of ~48 M patterns the CPU test and the in-situ GPU tests use
  HostBuild        pm_device_math.h compiled for the host behind a stub hip/hip_runtime.h
  compare()        bits equal; where both results are NaN the payload is exempt, but counted
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "learned-pmctf_amd", "csrc")

CHUNK = 1 << 26
LEAKY_SLOPE = 0.1           # slope of the apply_act(leaky) sweep: the slope of ConvFFN3's first gate

# the two inputs (of 2^32) on which pm_glibc_expf was one ulp off the expf of glibc 2.35 (x86-64, FMA build) while its
# remainder r = z - kd was left uncontracted; part of S so that the suite keeps them
EXPF_DEVIATIONS = (0x4202422f, 0xc27c65d9)
LIBM_FMA_PROBE = (0x4202422f, 0x56fc9f1c)        # input, what the FMA build of glibc's expf returns for it


def _f(bits):
    return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)


def _relu(x):
    """torch.relu itself (F.relu of the oracle, oracle/pmctf_oracle/model.py): a NaN and -0 come back unchanged"""
    import torch
    return torch.relu(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))).numpy()


def _leaky(x):
    with np.errstate(all="ignore"):
        return np.where(x > 0, x, x * np.float32(LEAKY_SLOPE)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _clib(name):
    """one object per oracle map, so that callers can compute a map once and reuse it for every probe code it specifies"""
    def call(x):
        from pmctf_oracle import clib
        return getattr(clib, name)(x)
    call.__name__ = name
    return call


# name, probe code (PMCTF_PROBE_* of include/pmctf_hip.h), specification: float32 array -> float32 array
FUNCTIONS = [
    ("tanh", 0, _clib("tanh")),                       # tanhf_, table in global memory
    ("tanh_lds", 1, _clib("tanh")),                   # tanhf_rows on the table tanh_rows_to_lds copied
    ("sigmoid", 2, _clib("sigmoid")),                 # sigmoidf_ (SLEEF transcription)
    ("sigmoid_scalar", 3, _clib("sigmoid_scalar")),   # pm_aten_sigmoidf_scalar (glibc expf transcription)
    ("log", 4, _clib("log")),                         # logf_
    ("log_poly", 5, _clib("log_poly")),               # logf_poly_
    ("exp", 6, _clib("exp")),                         # expf_
    ("glibc_exp", 7, _clib("glibc_exp")),             # pm_glibc_expf
    ("act_relu", 8 + 1, _relu),                       # apply_act; specification: torch.relu
    ("act_leaky", 8 + 2, _leaky),                     # numpy; equals F.leaky_relu on every input
    ("act_tanh", 8 + 3, _clib("tanh")),
    ("act_sigmoid", 8 + 4, _clib("sigmoid")),
]
SPEC = {name: spec for name, _, spec in FUNCTIONS}
CODE = {name: code for name, code, _ in FUNCTIONS}


def chunks(first=0, total=1 << 32, chunk=CHUNK):
    """(first pattern, count) of every chunk of the patterns first .. first + total - 1"""
    for b in range(first, first + total, chunk):
        yield b, min(chunk, first + total - b)


def chunk_bits(first, n):
    return np.arange(n, dtype=np.uint32) + np.uint32(first)                  # wraps past 2^32


def _fbits(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


def special_patterns():
    """+-0, +-inf, the smallest and largest subnormal and normal of both signs; the thresholds the sources name (tanh:
    0.046875, 9, 2^127 * 1.25; exp: -87, 87, 88; log: 2^-100, 2^100) of both signs with their two neighbours; the two
    inputs on which pm_glibc_expf was once one ulp off libm"""
    s = [0x00000000, 0x80000000, 0x7f800000, 0xff800000]
    for u in (0x00000001, 0x007fffff, 0x00800000, 0x7f7fffff):
        s += [u, u | 0x80000000]
    thresholds = [_fbits(0.046875), _fbits(9.0), 0x7f200000, _fbits(87.0), _fbits(-87.0), _fbits(88.0),
                  _fbits(2.0 ** 100), _fbits(2.0 ** -100)]
    assert thresholds[2] == _fbits(np.float32(2.0 ** 127) * np.float32(1.25))
    for u in thresholds:
        for d in (-1, 0, 1):
            s += [u + d, (u + d) ^ 0x80000000]
    s += list(EXPF_DEVIATIONS)
    return np.array(sorted(set(s)), np.uint32)


FULL_BINADES = (0x3f000000, 0x3f800000, 0x40000000, 0x41000000, 0xbf800000)     # [0.5,1) [1,2) [2,4) [8,16) -[1,2)


def stratified():
    """The set S, fixed by construction, as (label, uint32 patterns) pieces of at most 2^23 + a few:
    for each of the 512 sign x exponent values the first and last 4096 mantissas and 4096 evenly spaced ones (with the
    special patterns appended to the first piece); all 2^23 mantissas of [0.5, 1), [1, 2), [2, 4), [8, 16) and -[1, 2)."""
    m = np.concatenate([np.arange(4096), (1 << 23) - 4096 + np.arange(4096), np.arange(4096) * 2048 + 1024]).astype(np.uint32)
    se = (np.arange(512, dtype=np.uint32) << np.uint32(23))
    strata = (se[:, None] | m[None, :]).reshape(-1)
    yield "strata+specials", np.concatenate([strata, special_patterns()])
    for base in FULL_BINADES:
        yield f"binade {base:#010x}", np.uint32(base) + np.arange(1 << 23, dtype=np.uint32)


def compare(got_bits, want_bits):
    """-> (mismatches, index of the first or -1, elements where both are NaN with different payloads: exempt, counted)"""
    got_bits, want_bits = np.asarray(got_bits).view(np.uint32), np.asarray(want_bits).view(np.uint32)
    neq = np.flatnonzero(got_bits != want_bits)
    if neq.size == 0:
        return 0, -1, 0
    both_nan = np.isnan(got_bits[neq].view(np.float32)) & np.isnan(want_bits[neq].view(np.float32))
    bad = neq[~both_nan]
    return int(bad.size), (int(bad[0]) if bad.size else -1), int(both_nan.sum())


def describe(name, inputs, got_bits, want_bits, count, first):
    got_bits, want_bits = np.asarray(got_bits).view(np.uint32), np.asarray(want_bits).view(np.uint32)
    return (f"{name}: {count} mismatches; first at input {int(inputs[first]):#010x}: "
            f"got {int(got_bits[first]):#010x}, specification {int(want_bits[first]):#010x}")


# ---- pm_device_math.h compiled for the host ------------------------------------------------------------------------------
_STUB = r"""
#pragma once
#include <stdint.h>
#include <string.h>
#define __device__
#define __host__
#define __forceinline__ inline
struct alignas(16) uint4 { unsigned x, y, z, w; };
static inline float __uint_as_float(unsigned u) { float f; memcpy(&f, &u, 4); return f; }
static inline unsigned __float_as_uint(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
"""

_DRIVER = r"""
#include "pm_device_math.h"
#include <thread>
#include <vector>
static float eval(int fn, float x, float slope, const uint4 *lds) {
    switch (fn) {
    case 0: return pm::tanhf_(x);
    case 1: return pm::tanhf_rows(x, lds);
    case 2: return pm::sigmoidf_(x);
    case 3: return pm_aten_sigmoidf_scalar(x);
    case 4: return pm::logf_(x);
    case 5: return pm::logf_poly_(x);
    case 6: return pm::expf_(x);
    case 7: return pm_glibc_expf(x);
    default: return pm::apply_act(x, fn - 8, slope);
    }
}
extern "C" int host_probe(int fn, const uint32_t *bits, uint32_t first_bits, long n, float *y, float slope, int threads) {
    if (fn < 0 || fn > 12 || fn == 8 || !y || n <= 0) return -1;
    static uint4 lds[pm::TANH_LDS_UINT4];
    pm::tanh_rows_to_lds(lds, 0, 1);
    if (threads < 1) threads = 1;
    std::vector<std::thread> pool;
    const long per = (n + threads - 1) / threads;
    for (int t = 0; t < threads; ++t)
        pool.emplace_back([=] {
            const long b = t * per, e = b + per < n ? b + per : n;
            for (long i = b; i < e; ++i)
                y[i] = eval(fn, __uint_as_float(bits ? bits[i] : first_bits + (uint32_t)i), slope, lds);
        });
    for (auto &th : pool) th.join();
    return 0;
}
"""

HOST_FLAGS = ["-O2", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-shared", "-fPIC", "-pthread"]


class HostBuild:
    """g++ build of the device header in `workdir` (a temporary directory of the caller): probe(name, bits) evaluates the
    function the way pmctf_math_probe_f32 does on the GPU.  csrc: another copy of the sources (mutation checks)."""

    def __init__(self, workdir, csrc=CSRC):
        os.makedirs(os.path.join(workdir, "stub", "hip"), exist_ok=True)
        with open(os.path.join(workdir, "stub", "hip", "hip_runtime.h"), "w") as f:
            f.write(_STUB)
        src = os.path.join(workdir, "host_probe.cpp")
        with open(src, "w") as f:
            f.write(_DRIVER)
        so = os.path.join(workdir, "libhost_probe.so")
        subprocess.check_call([os.environ.get("CXX", "g++")] + HOST_FLAGS +
                              ["-I", os.path.join(workdir, "stub"), "-I", csrc, src, "-o", so])
        self.lib = C.CDLL(so)
        self.lib.host_probe.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_long, C.c_void_p, C.c_float, C.c_int]
        self.threads = int(os.environ.get("PM_ORACLE_THREADS", "0")) or min(16, len(os.sched_getaffinity(0)))

    def probe(self, name, bits=None, first=0, n=None):
        if bits is not None:
            bits = np.ascontiguousarray(bits, dtype=np.uint32)
            n = bits.size
        y = np.empty(n, np.float32)
        rc = self.lib.host_probe(CODE[name], None if bits is None else bits.ctypes.data, first, n, y.ctypes.data,
                                 LEAKY_SLOPE, self.threads)
        assert rc == 0, (name, rc)
        return y


def libm_is_fma_build():
    """glibc selects its expf by CPU; the transcription follows the FMA build, which this input tells from the other"""
    from pmctf_oracle import clib
    x, want = LIBM_FMA_PROBE
    return int(clib.libm_exp(_f([x])).view(np.uint32)[0]) == want
