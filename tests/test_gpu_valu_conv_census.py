"""Every vector-ALU convolution kernel of csrc/basic_ops.hip, reached by name and bit for bit: each row of
valu_conv_census.CENSUS runs through ops.Conv2d, ops.conv3x3_cin1_dual or ops.DepthwiseConv2d (the C entry where the
wrapper cannot express the row), asserts WHICH kernel ran (ops.valu_conv_last_launch() against the row's expected
expression) and compares the output, written between sentinels, with the oracle's convolution under the row's rule,
the oracle's activation and the residual adds, as uint32 patterns: -0.0 is not +0.0 here.

The rows behind PMCTF_FEWCOUT_LDS=0 and PMCTF_DWCONV_COLUMN=0 (read once per process) run in one fresh child process
per switch (valu_conv_census.py is its own __main__), one after the other, each under its own time limit; a child that
ends abnormally ends the test before the next one starts.  A child writes its outputs to a file; they are compared here."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import valu_conv_census as vc

pytestmark = pytest.mark.gpu

# one child: interpreter and torch start-up, GPU initialisation, at most 60 tiny launches, one 95 MB plane, the file
CHILD_TIMEOUT = 120


def compare(r, outs, launched, intact):
    """the failures of one row: kernel name first (both names), then guards, then bit patterns"""
    rid, expected = r[0], r[9]
    want, ok, text = vc.reference(r)
    print(text)
    assert ok, f"precondition: {text}: change the row's data"
    expr, grid = vc.parse_launch(launched)
    assert expr == expected, f"{rid}: expected {expected}, launched {expr} ({launched})"
    assert intact, f"{rid} ({launched}): a store outside the output (the sentinels around it changed)"
    assert len(outs) == len(want), (rid, len(outs), len(want))
    for i, (got, ref) in enumerate(zip(outs, want)):
        assert got.shape == ref.shape, (rid, i, got.shape, ref.shape)
        neq = vc.bits(got) != vc.bits(ref)
        if neq.any():
            at = tuple(int(v) for v in np.argwhere(neq)[0])
            where = np.argwhere(neq)
            raise AssertionError(
                f"{rid} ({launched}) output {i}: {int(neq.sum())}/{got.size} bit patterns differ; first at (n, c, y, x) = {at}: "
                f"{got[at]!r} ({vc.bits(got)[at]:#010x}) vs {ref[at]!r} ({vc.bits(ref)[at]:#010x}); "
                f"couts {sorted(set(where[:, 1].tolist()))[:12]}, rows {sorted(set(where[:, 2].tolist()))[:12]}, "
                f"columns {sorted(set(where[:, 3].tolist()))[:12]}; unwritten (sentinel) {int((vc.bits(got) == vc.SENTINEL).sum())}")


@pytest.mark.parametrize("rid", [r[0] for r in vc.rows_for(None)])
def test_census_row(cuda, rid):
    from pMCTF.hip import ops
    r = vc.row(rid)
    outs, launched, intact = vc.run_row(r)
    assert launched == ops.valu_conv_last_launch()           # the record stays until the next convolution of this thread
    compare(r, outs, launched, intact)


def test_a_refused_call_clears_the_record(cuda):
    import torch
    from pMCTF.hip import lib, ops
    vc.run_row(vc.row("dw_k3_c6"))
    assert ops.valu_conv_last_launch().startswith("dwconv_kernel grid ")
    x = torch.zeros(16, device="cuda")
    assert lib.hip().pmctf_dwconv2d_nhwc_f32(ops._p(x), ops._p(x), None, ops._p(x), 1, 2, 2, 4, 2, None) == -1     # even K
    assert ops.valu_conv_last_launch() == ""


def test_rows_behind_the_environment_switches(cuda, tmp_path):
    """PMCTF_FEWCOUT_LDS=0, then PMCTF_DWCONV_COLUMN=0, in a fresh child each; never more than one child at a time"""
    results, seconds = {}, {}
    for switch in vc.SWITCHES:
        assert vc.rows_for(switch), switch
        path = str(tmp_path / f"{switch}.npz")
        env = dict(os.environ)
        env[switch] = "0"
        t0 = time.time()
        try:
            p = subprocess.run([sys.executable, vc.__file__, switch, path], env=env, timeout=CHILD_TIMEOUT,
                               capture_output=True, text=True)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"{switch}=0: no exit within {CHILD_TIMEOUT} s\n{(e.stderr or '')[-3000:]}")
        if p.returncode != 0:
            pytest.fail(f"{switch}=0: exit status {p.returncode}\n{p.stderr[-3000:]}")
        seconds[switch] = time.time() - t0
        with np.load(path) as d:
            results[switch] = {k: d[k] for k in d.files}
    print("\nchild processes took " + ", ".join(f"{k}=0: {s:.1f} s" for k, s in seconds.items()))
    bad = []
    for switch, out in results.items():
        for r in vc.rows_for(switch):
            n = sum(1 for k in out if k.startswith(r[0] + "__y"))
            try:
                compare(r, [out[f"{r[0]}__y{i}"] for i in range(n)], str(out[r[0] + "__launch"]), bool(out[r[0] + "__intact"]))
            except AssertionError as e:
                bad.append(str(e))
    assert not bad, f"{len(bad)} rows failed:\n" + "\n".join(bad[:20])
