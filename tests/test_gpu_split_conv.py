"""The bf16-split 3x3 convolution (csrc/conv_split.hip: pmctf_conv3x3_split_f32 behind ops.Conv2d(split=ns),
pmctf_conv3x3_split_geom_f32 behind ops.conv_at_class) held to its written arithmetic, restated in float64 by
tests/split_restatement.py.

Exact data (split_restatement.exact_case): every kept partial product is a multiple of 2^-18 and every partial sum stays
below 16, so an f32 accumulation gives the float64 sum S whatever its order, and the kernel's output must equal
epilogue(f32(S)) BIT FOR BIT, for 1, 2 and 3 planes, every activation the kernel has and 0 / 1 / 2 residuals.  A dropped
or swapped partial product, a split that truncates, a wrong tap or channel half, a stale LDS stage: each changes more
than half of the expected values (tests/test_split_restatement_cpu.py checks that on the CPU).

Dense data (dense_case): |y - S| <= T = n 2^-23 A elementwise, n = 9 Cin len(TERMS[ns]) + 1 additions: Higham's bound
for a sum of n terms in any order with the unit round-off of a truncating f32 adder; and |y - conv64| <= T + EPS[ns]
sum |x||w|, the accuracy the header promises, end to end.

The cases (split_conv_helper.STRIDE1 / STRIDE2) are the smallest that reach every tile boundary.  They run in this process
on the kernel the dispatcher picks, and the stride-1 ones again in one child process per PMCTF_SPLIT_VARIANT (0, 1, 2:
the variable is latched at first use), so that all eighteen stride-1 instantiations and the three stride-2 ones run."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import split_conv_helper as hp
import split_restatement as sr
from helpers import assert_same

pytestmark = pytest.mark.gpu

# one child: interpreter and torch start-up, GPU initialisation, 6 cases x (27 exact + 3 dense launch pairs) and the
# copies back.  Measured on the first GPU visit: see the figure next to the constant's use in the log of
# test_every_variant_of_the_stride1_kernels; the limit is several times that.
CHILD_TIMEOUT = 120
IDS = [c.name for c in hp.CASES]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def reference():
    """expected values of every case, computed once on the CPU and left unchanged"""
    t0 = time.time()
    ref = {c.name: (hp.expected_exact(c), hp.expected_dense(c)) for c in hp.CASES}
    print(f"\nsplit conv: expected values of {len(hp.CASES)} cases on the CPU in {time.time() - t0:.1f} s")
    return ref


@pytest.fixture(scope="module")
def in_process(cuda):
    """every case on the kernels the dispatcher picks (stride 1) and on the stride-2 entry"""
    t0 = time.time()
    out, same = hp.run(hp.CASES, log=lambda s: print("  " + s))
    print(f"split conv: {len(out)} outputs of {len(hp.CASES)} cases in process in {time.time() - t0:.1f} s")
    return out, same


def exact_failures(c, out, ref, label):
    """the exact-data outputs of case c against the expected bits"""
    want, _ = ref[c.name][0]
    bad = []
    for tag, _, _ in hp.geometries(c):
        for ns in hp.NSPLITS:
            for epi in hp.EPILOGUES:
                k = hp.key(c, "exact", tag, ns, epi)
                got = out[k]
                if got.shape != want[k].shape:
                    bad.append(f"{label} {k}: shape {got.shape} vs {want[k].shape}")
                    continue
                neq = got != want[k]
                if neq.any():
                    i = tuple(int(v) for v in np.argwhere(neq)[0])
                    d = np.abs(got.astype(np.float64) - want[k])
                    bad.append(f"{label} {k}: {int(neq.sum())} of {neq.size} values differ; first at {i}: {got[i]!r} vs "
                               f"{want[k][i]!r}; largest difference {d.max() / sr.Q:.3g} x 2^-18")
        plain = [out[hp.key(c, "exact", tag, ns)] for ns in hp.NSPLITS]
        for a, b in ((0, 1), (0, 2), (1, 2)):
            if np.array_equal(plain[a], plain[b]):
                bad.append(f"{label} {c.name} {tag}: {hp.NSPLITS[a]} and {hp.NSPLITS[b]} planes give the same output")
    return bad


def dense_failures(c, out, ref, label, worst):
    """the dense outputs of case c against the accumulation bound T and the end-to-end promise; worst[ns] collects the
    largest |y - S| / T"""
    bad = []
    for tag, _, _ in hp.geometries(c):
        for ns in hp.NSPLITS:
            k = hp.key(c, "dense", tag, ns)
            S, T, C64, E = ref[c.name][1][k]
            y = out[k].astype(np.float64)
            if y.shape != S.shape or not np.isfinite(y).all():
                bad.append(f"{label} {k}: shape {y.shape} vs {S.shape}, or values that are not finite")
                continue
            r = np.abs(y - S) / T
            worst[ns] = max(worst.get(ns, 0.0), float(r.max()))
            if (r > 1).any():
                i = tuple(int(v) for v in np.argwhere(r > 1)[0])
                bad.append(f"{label} {k}: |y - S| > T at {int((r > 1).sum())} of {r.size} values, first at {i}: y {y[i]!r}, "
                           f"S {S[i]!r}, T {T[i]:.3e}; largest |y - S| / T = {r.max():.3g}")
            e = np.abs(y - C64) / (T + E)
            if (e > 1).any():
                bad.append(f"{label} {k}: |y - conv64| > T + eps sum|x||w| at {int((e > 1).sum())} values, largest ratio "
                           f"{e.max():.3g}")
    return bad


@pytest.mark.parametrize("case", hp.CASES, ids=IDS)
def test_exact_data_bit_for_bit(case, in_process, reference):
    """y == epilogue(f32(S)) for 1 / 2 / 3 planes x {none, relu, leaky 0.2} x {0, 1, 2 residuals}; the three plane counts
    give three different outputs"""
    bad = exact_failures(case, in_process[0], reference, "in process")
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:12])


@pytest.mark.parametrize("case", hp.CASES, ids=IDS)
def test_dense_data_within_the_accumulation_bound(case, in_process, reference):
    """|y - S| <= T and |y - conv64| <= T + EPS[ns] sum |x||w|, elementwise"""
    worst = {}
    bad = dense_failures(case, in_process[0], reference, "in process", worst)
    print(f"\n{case.name}: largest |y - S| / T for 1 / 2 / 3 planes: " + " / ".join(f"{worst[ns]:.4f}" for ns in hp.NSPLITS))
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:12])


def test_every_launch_twice_gives_equal_bits(in_process):
    out, same = in_process
    assert set(same) == set(out) and len(out) == sum(len(hp.geometries(c)) for c in hp.CASES) * 3 * (len(hp.EPILOGUES) + 1)
    assert all(same.values()), [k for k, v in same.items() if not v][:10]
    launched = {hp.instantiation(None, c.Cout, ns, c.stride) for c in hp.CASES for ns in hp.NSPLITS}
    assert len(launched) == 6 + 3               # the dispatcher's six stride-1 choices and the three stride-2 kernels


def test_every_variant_of_the_stride1_kernels(cuda, in_process, reference, tmp_path):
    """PMCTF_SPLIT_VARIANT = 0, 1, 2 in a fresh child each (tests/split_conv_helper.py), one after another; a child that
    fails or runs out of time ends the test before the next starts.  Exact data: the expected bits, hence identical
    across variants and equal to the dispatcher's choice.  Dense data: each variant within T (the order of accumulation
    may differ between the workgroup and the wave kernel)."""
    results, seconds = {}, {}
    for v in hp.VARIANTS:
        path = str(tmp_path / f"variant{v}.npz")
        env = dict(os.environ)
        env[hp.SWITCH] = str(v)
        t0 = time.time()
        try:
            p = subprocess.run([sys.executable, hp.__file__, str(v), path], env=env, timeout=CHILD_TIMEOUT,
                               capture_output=True, text=True)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"variant {v}: no exit within {CHILD_TIMEOUT} s\n{(e.stderr or '')[-3000:]}")
        if p.returncode != 0:
            pytest.fail(f"variant {v}: exit status {p.returncode}\n{p.stderr[-3000:]}")
        seconds[v] = time.time() - t0
        d = np.load(path)
        results[v] = {k: d[k] for k in d.files}
    print("\nsplit conv: child processes took " + ", ".join(f"variant {v}: {s:.1f} s" for v, s in seconds.items()))

    bad, ran = [], set()
    for v, out in results.items():
        worst = {}
        for c in hp.STRIDE1_CASES:
            bad += exact_failures(c, out, reference, f"variant {v}")
            bad += dense_failures(c, out, reference, f"variant {v}", worst)
            ran |= {hp.instantiation(v, c.Cout, ns) for ns in hp.NSPLITS}
        bad += [f"variant {v} {k[6:]}: two launches, different bits" for k in out if k.startswith("same__") and not out[k]]
        print(f"  variant {v}: largest |y - S| / T for 1 / 2 / 3 planes: " + " / ".join(f"{worst[ns]:.4f}" for ns in hp.NSPLITS))
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:20])
    assert len(ran) == 18, sorted(ran)
    for c in hp.STRIDE1_CASES:                  # identical bits across the variants and the dispatcher's choice
        for ns in hp.NSPLITS:
            for epi in hp.EPILOGUES:
                k = hp.key(c, "exact", "full", ns, epi)
                for v in hp.VARIANTS:
                    assert np.array_equal(_bits(results[v][k]), _bits(in_process[0][k])), (v, k)


def test_tanh_keeps_the_exact_kernel(cuda):
    """the split kernels have no tanh / sigmoid epilogue: ops.Conv2d(split=3) called with one returns the exact kernel's
    bits (use_split stays false above leaky), while the same layer with leaky does take the split kernel"""
    import torch
    from pMCTF.hip import ops
    c = hp.STRIDE1_CASES[2]
    x, w, b = hp.inputs(c, "dense")
    xt = torch.from_numpy(x).cuda()
    wt, bt = torch.from_numpy(w), torch.from_numpy(b)
    exact = ops.Conv2d(wt, bt, 1, (1, 1))
    old = ops.SPLIT_MIN_PX
    ops.SPLIT_MIN_PX = 0
    try:
        conv = ops.Conv2d(wt, bt, 1, (1, 1), split=3)
        assert conv.split == 3
        for act in (ops.ACT_TANH, ops.ACT_SIGMOID):
            assert_same(conv(xt, act=act), exact(xt, act=act), f"split=3 with activation {act}")
        assert not torch.equal(conv(xt, act=ops.ACT_LEAKY, slope=0.2), exact(xt, act=ops.ACT_LEAKY, slope=0.2))
        c2 = hp.CASES[-2]
        x2, w2, b2 = hp.inputs(c2, "dense")
        x2t = torch.from_numpy(x2).cuda()
        exact2 = ops.Conv2d(torch.from_numpy(w2), torch.from_numpy(b2), 1, (1, 1))
        conv2 = ops.Conv2d(torch.from_numpy(w2), torch.from_numpy(b2), 1, (1, 1), split=3)
        assert_same(ops.conv_at_class(conv2, x2t, 3, act=ops.ACT_TANH), ops.conv_at_class(exact2, x2t, 3, act=ops.ACT_TANH),
                    "conv_at_class, split=3 with tanh")
        assert not torch.equal(ops.conv_at_class(conv2, x2t, 3), ops.conv_at_class(exact2, x2t, 3))
    finally:
        ops.SPLIT_MIN_PX = old
