"""Every kernel the convolution dispatcher (csrc/conv_mfma.hip) can launch, reached by name and bit for bit: each row of
conv_census.CENSUS sets its knobs, runs ops.Conv2d with the row's activation and residual adds, asserts WHICH kernels
ran (pmctf_conv2d_last_launch against the row's expected keys) and compares the output with the oracle's C convolution
under the row's summation rule as uint32 bit patterns (-0.0 is not +0.0 here).  The rows on zero and subnormal data
(conv_census.DATA) have their own preconditions, asserted without a GPU in test_conv_census_cpu.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import conv_census as cc

pytestmark = pytest.mark.gpu

MIN_RULE_SHARE = 0.5       # a row under rule R is only a test of R if the oracle's other rules give other bits in half the elements


def _nhwc(x):
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 1))).cuda()


def _nchw(t):
    return np.ascontiguousarray(t.cpu().numpy().transpose(0, 3, 1, 2))


def reference(r, x, w, b, res):
    """clib.conv2d under the row's rule, then the activation, then + res1 + res2; for rule != 0 first the precondition that
    the data tells the row's rule from the other rules (CPU only: the reference alone holds it)"""
    from pmctf_oracle import clib
    rid, (N, Cin, H, W, Cout, K, S, pad), rule, act, slope, nres, knobs, expected = r
    ref = clib.conv2d(x, w, b, S, (pad, pad), rule)
    # The rows on zero and subnormal data do not test rule selection (on zeros the rules part in the sign of a zero only;
    # the ordinary rows of the same expression and rule hold it); a no-bias row does, unless its input is one 16-channel
    # chunk: without a bias that is one chain from +0 under both rules.
    kind = cc.DATA.get(rid)
    tells = rule and (kind is None or (kind == "nobias" and Cin > 16))
    for other in {0, 1} - {rule} if tells else ():
        share = float((ref != clib.conv2d(x, w, b, S, (pad, pad), other)).mean())
        print(f"{rid}: rule {rule} differs from rule {other} in {share:.3f} of the elements")
        assert share >= MIN_RULE_SHARE, f"{rid}: the data does not tell rule {rule} from rule {other} ({share:.3f}): change the row's data"
    if act == 1:
        ref = np.where(ref < 0, np.float32(0), ref)          # max(0, v) as ATen takes it: -0 and NaN stay (pm::relu_)
    elif act == 2:
        ref = np.where(ref > 0, ref, ref * np.float32(slope)).astype(np.float32)
    elif act == 3:
        ref = clib.tanh(ref)
    elif act == 4:
        ref = clib.sigmoid(ref)
    for q in res:
        ref = ref + q
    return ref


def assert_same_bits(got, want, what):
    got, want = (np.ascontiguousarray(a, dtype=np.float32) for a in (got, want))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    neq = got.view(np.uint32) != want.view(np.uint32)
    if neq.any():
        i = tuple(np.argwhere(neq)[0])
        raise AssertionError(f"{what}: {int(neq.sum())}/{got.size} bit patterns differ; first at (n, c, y, x) = {i}: "
                             f"{got[i]!r} ({got.view(np.uint32)[i]:#010x}) vs {want[i]!r} ({want.view(np.uint32)[i]:#010x}); "
                             f"differing couts {sorted(set(np.argwhere(neq)[:, 1].tolist()))[:20]}, "
                             f"rows {sorted(set(np.argwhere(neq)[:, 2].tolist()))[:20]}")


def _last_launch(L):
    buf = C.create_string_buffer(512)
    assert L.pmctf_conv2d_last_launch(buf, 512) == 0
    return buf.value.decode()


def run_row(r, x, w, b, res):
    """the row's convolution under the row's knobs: (output NCHW, launch string); every knob restored afterwards"""
    from pMCTF.hip import lib, ops
    rid, (N, Cin, H, W, Cout, K, S, pad), rule, act, slope, nres, knobs, expected = r
    L = lib.hip()
    conv = ops.Conv2d(torch.from_numpy(w), None if b is None else torch.from_numpy(b), S, (pad, pad), rule=rule)
    assert not conv.small and not conv.few and not conv.split
    xd, rd = _nhwc(x), [_nhwc(q) for q in res]
    saved = {k: L.pmctf_conv2d_get_option(k.encode()) for k in cc.KNOBS}
    try:
        for k, v in {**cc.KNOBS, **knobs}.items():
            assert L.pmctf_conv2d_set_option(k.encode(), v) == 0, k
        y = conv(xd, act=act, slope=slope, res1=rd[0] if nres > 0 else None, res2=rd[1] if nres > 1 else None)
        launched = _last_launch(L)
        torch.cuda.synchronize()
        return _nchw(y), launched
    finally:
        for k, v in saved.items():
            L.pmctf_conv2d_set_option(k.encode(), v)


@pytest.mark.parametrize("rid", [r[0] for r in cc.CENSUS])
def test_census_row(cuda, rid):
    r = cc.row(rid)
    x, w, b, res = cc.case_data(r)
    ref = reference(r, x, w, b, res)
    got, launched = run_row(r, x, w, b, res)
    keys = cc.parse_launch(launched)
    assert keys == r[7], f"{rid}: expected {r[7]}, launched {keys} ({launched})"
    assert_same_bits(got, ref, f"{rid} {launched}")


def test_knobs_are_back_at_their_defaults(cuda):
    """what the rows set must not leak into later tests (the rows restore what they read)"""
    from pMCTF.hip import lib
    L = lib.hip()
    for k, v in cc.KNOBS.items():
        if f"PMCTF_CONV_{k}" not in os.environ:
            assert L.pmctf_conv2d_get_option(k.encode()) == v, k
