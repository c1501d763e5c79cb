"""CPU half of the direct tests of csrc/conv_split.hip: the restatement (tests/split_restatement.py) and the inputs are
checked here, so that what tests/test_gpu_split_conv.py holds the kernels to is itself pinned.

  * bf16_rne against torch's bfloat16 cast;
  * the exact data of every GPU case really is order-independent in f32 (conditions on the INPUTS: if one fails, the
    inputs change, not the test);
  * every wrong-on-purpose restatement (MUTANTS) changes the expected output, so a kernel with that error cannot pass;
  * the truncation bounds EPS[ns] hold on the dense data;
  * pmctf_conv3x3_split_pack_weights (host code) against planes(), and the refusals of the two launch entry points;
  * every extern "C" of conv_split.hip is named in the GPU test or its helper."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import split_conv_helper as hp
import split_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERIFIED = (2, 32, 64, 9, 19, 7)                # N, Cin, Cout, H, W, seed: the data set the figures in the comments are from


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_bf16_rne_is_torchs_cast():
    """10^5 values over 40 binades, both signs; a third of them exact ties (low half 0x8000), on even and odd neighbours"""
    r = np.random.default_rng(5)
    n = 100000
    u = (r.integers(0, 2, n).astype(np.uint32) << 31) | (r.integers(107, 147, n).astype(np.uint32) << 23) \
        | r.integers(0, 1 << 23, n).astype(np.uint32)
    u[::3] = (u[::3] & np.uint32(0xFFFF0000)) | np.uint32(0x8000)
    u[:8] = [0, 0x80000000, 0x3F800000, 0x3F808000, 0x3F818000, 0x7F7FFFFF, 0x00000001, 0x7F800000]
    x = u.view(np.float32)
    assert len(np.unique(u >> 23 & 0xFF)) >= 40 and ((u & 0xFFFF) == 0x8000).sum() > n // 3
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    got = sr.bf16_rne(x)
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:5]
    ties = (u & 0xFFFF) == 0x8000
    assert (_bits(got)[ties] >> 16 & 1 == 0).all(), "a tie went to the odd neighbour"
    assert (_bits(sr.bf16_trunc(x)) == (u & 0xFFFF0000)).all()
    for ns in (1, 2, 3):            # the planes add up to x again, to what ns planes of 8 bits can hold
        p = sr.planes(x[8:], ns)
        rest = x[8:].astype(np.float64) - sum(q.astype(np.float64) for q in p)
        assert (np.abs(rest) <= 2.0 ** (-8 * ns) * np.abs(x[8:])).all()


def test_planes_of_the_exact_values():
    x, w, b = sr.exact_case(*VERIFIED)
    for v in (x[x != 0], w.reshape(-1)):
        p = sr.planes(v, 3)
        s = np.sign(v)
        assert (np.abs(p[0]) == 1).all() and (p[0] == s).all()
        assert (p[1] == s * 2.0 ** -9).all()
        assert (np.abs(p[2]) == 2.0 ** -18).all()
        assert (p[0].astype(np.float64) + p[1] + p[2] == v).all()
        assert {-1.0, 1.0} == set(np.unique(p[2] * s * 2.0 ** 18))              # both signs of t occur
    assert (np.count_nonzero(x, axis=-1) == 1).all()
    assert (b / sr.Q == np.rint(b / sr.Q)).all() and np.abs(b).max() <= 2 and np.abs(b).max() > 1


@pytest.mark.parametrize("case", hp.CASES, ids=[c.name for c in hp.CASES])
def test_exact_data_is_order_independent_in_f32(case):
    """the conditions under which the kernel's f32 sums must equal the float64 S bit for bit, for every case, geometry
    and plane count the GPU test uses"""
    x, w, b = hp.inputs(case, "exact")
    assert (np.count_nonzero(x, axis=-1) == 1).all()
    for tag, _, g in hp.geometries(case):
        outs = {}
        for ns in hp.NSPLITS:
            S, A = sr.conv_ref(x, w, b, ns, **g)
            assert S.shape == (case.N,) + g["out_hw"] + (case.Cout,)
            assert A.max() < 16 and A.max() <= 11.04, (tag, ns, A.max())
            assert (S / sr.Q == np.rint(S / sr.Q)).all(), "S is not a multiple of 2^-18"
            assert (S.astype(np.float32).astype(np.float64) == S).all(), "S is not an f32 number"
            for rev in (False, True):
                got = sr.sequential_f32(x, w, b, ns, reverse=rev, **g)
                assert np.array_equal(got.astype(np.float64), S), (tag, ns, "reverse" if rev else "forward")
            outs[ns] = S
        if case.N * case.H * case.W > 100:
            for a, c in ((1, 2), (1, 3), (2, 3)):       # a launch that used fewer planes gives another result
                assert (outs[a] != outs[c]).mean() > 0.5, (tag, a, c, (outs[a] != outs[c]).mean())
        else:
            for a, c in ((1, 2), (1, 3), (2, 3)):
                assert (outs[a] != outs[c]).any()


def test_every_mutant_changes_the_expected_output():
    """verified case: each dropped term changes 90-91 % of the outputs, the truncating split 89 % (two planes) and 94 %
    (three), the column shift 81-97 %, one negated weight exactly the outputs that read it"""
    x, w, b = sr.exact_case(*VERIFIED)
    co, ci, ky, kx = sr.NEGATED
    for ns in (1, 2, 3):
        S, _ = sr.conv_ref(x, w, b, ns)
        assert set(sr.MUTANTS[ns]) == {f"drop {t}" for t in sr.TERMS[ns]} | {"truncate", "shift", "negate"}
        for name, f in sr.MUTANTS[ns].items():
            changed = f(x, w, b, ns) != S
            print(f"ns {ns}, {name}: {changed.mean():.3f} of the outputs change")
            if name == "negate":
                reads = np.zeros(S.shape, bool)
                tap_x = dict(sr.windows(x))[3 * ky + kx][..., ci]
                reads[..., co] = tap_x != 0
                assert np.array_equal(changed, reads) and reads.sum() > 0
            elif name == "truncate" and ns == 1:
                assert not changed.any()        # the first plane of these values is the same either way: nothing to see
            else:
                assert changed.mean() > 0.5, (ns, name, changed.mean())


def test_mutants_change_the_stride2_output_too():
    x, w, b = sr.exact_case(1, 16, 112, 10, 12, 9)
    for cls in range(4):
        g = dict(stride=2, pad=(1 - (cls >> 1), 1 - (cls & 1)), out_hw=(5, 6))
        full = sr.conv_ref(x, w, b, 3)[0]
        S = sr.conv_ref(x, w, b, 3, **g)[0]
        assert np.array_equal(S, full[:, cls >> 1::2, cls & 1::2]), "a parity class is the full convolution sampled"
        for name, f in sr.MUTANTS[3].items():
            if name != "negate":
                assert (f(x, w, b, 3, **g) != S).mean() > 0.5, (cls, name)


@pytest.mark.parametrize("case", hp.CASES, ids=[c.name for c in hp.CASES])
def test_truncation_bounds_on_the_dense_data(case):
    """|S - conv64| <= EPS[ns] sum |x||w|: the header's "~2^-8 / ~2^-16 / ~2^-22 per product" as an assertion.  Verified
    data set: the largest error is 0.62 / 0.52 / 0.11 of the bound."""
    x, w, b = hp.inputs(case, "dense")
    scales = np.log2(np.abs(x).reshape(-1, case.Cin).max(axis=0))
    assert scales.max() - scales.min() >= 6 or case.Cin == 16, "the channels should differ in scale"
    for tag, _, g in hp.geometries(case):
        C64, B = sr.conv64(x, w, b, **g)
        for ns in hp.NSPLITS:
            S, A = sr.conv_ref(x, w, b, ns, **g)
            ratio = (np.abs(S - C64) / (sr.EPS[ns] * B)).max()
            print(f"{case.name} {tag} ns {ns}: max |S - conv64| / (eps sum|x||w|) = {ratio:.3f}")
            assert ratio <= 1, (tag, ns, ratio)


def _pack(L, w, b, ns):
    cout, cin = w.shape[:2]
    n = L.pmctf_conv3x3_split_packed_size(cout, cin, ns)
    assert n == (cin // 16) * 5 * (cout // 16) * ns * 512
    wp = np.full(n + 64, 0xDEAD, np.uint16)             # canaries behind the buffer
    bp = np.full(cout + 8, np.float32(7), np.float32)
    rc = L.pmctf_conv3x3_split_pack_weights(w.ctypes.data, None if b is None else b.ctypes.data, cout, cin, ns,
                                            wp.ctypes.data, bp.ctypes.data)
    assert rc == 0
    assert (wp[n:] == 0xDEAD).all() and (bp[cout:] == 7).all(), "the packer wrote past its buffers"
    return wp[:n], bp[:cout]


@pytest.mark.parametrize("shape", [(64, 16), (112, 32), (112, 112)])
def test_pack_weights_bit_for_bit(shape):
    """layout [mb][cb][kb][mt][plane][lane][j], lane = (g, p): cout (mb*MT + mt)*16 + p, tap 2 kb + (g >> 1), channel
    cb*16 + 8 (g & 1) + j; the tenth half-block (tap 9) holds zeros"""
    from pMCTF.hip import lib
    L = lib.hip()
    cout, cin = shape
    assert L.pmctf_conv3x3_split_supported(cin, cout) == 1
    r = np.random.default_rng(cout + cin)
    w = (r.standard_normal((cout, cin, 3, 3)) * 2.0 ** r.integers(-20, 20, (cout, cin, 3, 3))).astype(np.float32)
    w[0, 0, 0, :2] = np.array([0x3F808000, 0x3F818000], np.uint32).view(np.float32)     # ties, to even both ways
    b = r.standard_normal(cout).astype(np.float32)
    mt = cout // 16
    for ns in (1, 2, 3):
        wp, bp = _pack(L, w, b, ns)
        assert np.array_equal(_bits(bp), _bits(b)), "bias_packed is the bias"
        # [cb][kb][mt][plane][g >> 1][g & 1][p][j] -> [plane][mt][p][cb][g & 1][j][kb][g >> 1] = [plane][cout][cin][tap]
        got = wp.reshape(cin // 16, 5, mt, ns, 2, 2, 16, 8).transpose(3, 2, 6, 0, 5, 7, 1, 4).reshape(ns, cout, cin, 10)
        assert (got[..., 9] == 0).all(), "tap 9 must hold zero weights"
        want = np.stack([(_bits(p) >> 16).astype(np.uint16) for p in sr.planes(w, ns)]).reshape(ns, cout, cin, 9)
        assert (_bits(np.stack(sr.planes(w, ns))) & 0xFFFF == 0).all()
        assert np.array_equal(got[..., :9], want), (ns, np.argwhere(got[..., :9] != want)[:4])
        _, bp0 = _pack(L, w, None, ns)
        assert (bp0 == 0).all(), "no bias: zeros"
    assert L.pmctf_conv3x3_split_packed_size(cout, cin, 0) == -1 and L.pmctf_conv3x3_split_packed_size(cout, cin, 4) == -1
    assert L.pmctf_conv3x3_split_packed_size(cout, cin + 8, 2) == -1 and L.pmctf_conv3x3_split_packed_size(128, cin, 2) == -1
    wp = np.zeros(16, np.uint16)
    for bad in ((128, cin, 2), (cout, cin + 8, 2), (cout, cin, 0), (cout, cin, 4)):
        assert L.pmctf_conv3x3_split_pack_weights(w.ctypes.data, None, *bad, wp.ctypes.data, b.ctypes.data) == -1
    assert L.pmctf_conv3x3_split_supported(cin + 8, cout) == 0 and L.pmctf_conv3x3_split_supported(cin, 128) == 0
    assert L.pmctf_conv3x3_split_supported(0, cout) == 0


def test_launch_entry_points_refuse_without_a_launch():
    """every refusal of the guards of pmctf_conv3x3_split_f32 / _geom_f32 returns PMCTF_EINVAL; the pointers are made up
    and only ever passed together with a refused argument"""
    from pMCTF.hip import lib
    L = lib.hip()
    p = 0x1000
    ok1 = dict(N=1, H=8, W=8, Cin=16, Cout=112, nsplit=2, act=0)

    def s1(**kw):
        a = {**ok1, **kw}
        return L.pmctf_conv3x3_split_f32(a.get("x", p), p, p, None, None, a.get("y", p), a["N"], a["H"], a["W"], a["Cin"],
                                         a["Cout"], a["nsplit"], a["act"], 0.0, None)

    ok2 = dict(ok1, stride=2, pad_h=1, pad_w=0, Ho=4, Wo=4)

    def s2(**kw):
        a = {**ok2, **kw}
        return L.pmctf_conv3x3_split_geom_f32(a.get("x", p), p, p, None, None, a.get("y", p), a["N"], a["H"], a["W"],
                                              a["Cin"], a["Cout"], a["nsplit"], a["stride"], a["pad_h"], a["pad_w"],
                                              a["Ho"], a["Wo"], a["act"], 0.0, None)

    common = [dict(Cin=24), dict(Cin=8), dict(Cin=0), dict(Cout=128), dict(Cout=96), dict(Cout=16), dict(nsplit=0),
              dict(nsplit=4), dict(act=3), dict(act=4), dict(act=-1), dict(N=65536), dict(N=0), dict(H=0), dict(W=0),
              dict(x=None), dict(y=None)]
    for kw in common:
        assert s1(**kw) == -1, ("pmctf_conv3x3_split_f32", kw)
        assert s2(**kw) == -1, ("pmctf_conv3x3_split_geom_f32", kw)
    assert s1(Cout=64, nsplit=0) == -1 and s1(Cout=64, nsplit=4) == -1
    geom = [dict(Cout=64), dict(stride=1), dict(stride=3), dict(pad_h=2), dict(pad_w=2), dict(pad_h=-1), dict(Ho=0),
            dict(Wo=0),
            dict(Ho=6, pad_h=1),            # last window starts at row 2*5 - 1 = 9 >= H = 8
            dict(Ho=5, pad_h=0),            # ... at row 8
            dict(Wo=5, pad_w=0), dict(Wo=6, pad_w=1)]
    for kw in geom:
        assert s2(**kw) == -1, ("pmctf_conv3x3_split_geom_f32", kw)


def test_every_entry_point_of_conv_split_is_named_by_the_gpu_test():
    src = open(os.path.join(ROOT, "learned-pmctf_amd", "csrc", "conv_split.hip")).read()
    entries = set(re.findall(r'extern "C" \w+ (pmctf_\w+)\(', src))
    assert len(entries) == 5, entries
    text = open(os.path.join(ROOT, "tests", "test_gpu_split_conv.py")).read() + open(hp.__file__).read()
    for e in entries:
        assert re.search(rf"\b{e}\b", text), f"{e} is not named in tests/test_gpu_split_conv.py or its helper"
    ops_text = open(os.path.join(ROOT, "learned-pmctf_amd", "pMCTF", "hip", "ops.py")).read()
    for e in entries:
        assert e in ops_text, f"pMCTF.hip.ops never calls {e}"
    assert "ops.Conv2d(" in open(hp.__file__).read() and "ops.conv_at_class(" in open(hp.__file__).read()


def test_the_instantiation_mirror_counts_eighteen_and_three():
    s1 = {hp.instantiation(v, cout, ns) for v in hp.VARIANTS for cout in (64, 112) for ns in hp.NSPLITS}
    assert len(s1) == 18
    assert {hp.instantiation(v, c.Cout, ns) for v in hp.VARIANTS for c in hp.STRIDE1_CASES for ns in hp.NSPLITS} == s1
    assert {hp.instantiation(None, cout, ns) for cout in (64, 112) for ns in hp.NSPLITS} < s1
    s2 = {hp.instantiation(None, c.Cout, ns, 2) for c in hp.CASES if c.stride == 2 for ns in hp.NSPLITS}
    assert len(s2) == 3 and not (s1 & s2)
    src = open(os.path.join(ROOT, "learned-pmctf_amd", "csrc", "conv_split.hip")).read()
    assert src.count("return launch_split<MT, ") == 3 and src.count("return launch_split_wave<MT, ") == 6
    assert src.count("return launch_split_wave<7, ") == 3
