"""Precondition of test_gpu_pu_fused.py, on the oracle alone: the references of the (rule, skip_rule) pairs are told
apart by the test's data, and the large weights saturate most tanh values."""
import itertools

import pytest

import numpy as np

from pu_fused_reference import MODE0_C, RULES, SCALES, ZERO_SHAPES, reference, zero_inputs, zero_reference


@pytest.mark.parametrize("scale", list(SCALES), ids=list(SCALES))
def test_references_tell_the_rules_apart(scale):
    """Precondition, on the CPU: on 37x53 the references of any two (rule, skip_rule) pairs differ in at least half of the
    elements (mode 0: of the two rules), or a kernel that ran the wrong rule would pass; and under the large weights most
    tanh values are saturated."""
    shape, s = (1, 37, 53), SCALES[scale]
    a, b = (reference(shape, s, rule, 0, 0) for rule in (0, 1))
    for c in MODE0_C:
        share = float((a[0][c] != b[0][c]).mean())
        print(f"mode 0 c {c} scale {s}: chain vs blocks {share:.3f}")
        assert share >= 0.5, (c, share)
    for p, q in itertools.combinations(RULES, 2):
        for sign in (1.0, -1.0):
            share = float((reference(shape, s, *p, 1)[0][sign] != reference(shape, s, *q, 1)[0][sign]).mean())
            print(f"mode 1 sign {sign} scale {s}: {p} vs {q} {share:.3f}")
            assert share >= 0.5, (p, q, sign, share)
    if scale == "saturating":
        for mode in (0, 1):
            sat = reference(shape, s, 0, 0, mode)[1]
            print(f"mode {mode}: saturated tanh values {sat:.3f}")
            assert sat > 0.5, (mode, sat)


@pytest.mark.parametrize("shape", ZERO_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_zero_references_hold_both_signs_of_zero(shape):
    """Precondition of the zero cases, on the CPU, per output: every output holds +0; which hold -0 follows from the
    arithmetic and is asserted as such.  A chain that starts at the bias (-0) keeps a -0 through all four layers, a chain
    that starts at +0 ends at +0 on zeros.  So mode 0 (x + pu * 0.1) shows -0 under rule chain only; mode 1 with sign +1
    (other + branch) only where the four layers AND the lifting filter run the chain; mode 1 with sign -1
    (other - branch: -0 - +0) under every pair.  Every (rule, skip_rule) pair therefore has an output with both signs;
    mode 0 under rule blocks has none, and checks there that nothing but +0 comes out of a zero patch."""
    u = zero_inputs(shape)[0].view(np.uint32)
    assert (u[..., 0:10] == 0x80000000).all() and (u[..., 10:20] == 0).all() and (u[..., 20:30] == 0x80000001).all()
    for rule, skip_rule in RULES:
        cases = [((1, sign), out, sign == -1.0 or (rule == 0 and skip_rule == 0))
                 for sign, out in zero_reference(shape, "neg0", rule, skip_rule, 1).items()]
        if skip_rule == 0:
            cases += [((0, c), out, rule == 0) for c, out in zero_reference(shape, "neg0", rule, 0, 0).items()]
        for key, out, shows_minus_zero in cases:
            o = np.ascontiguousarray(out).view(np.uint32)
            assert (o == 0).any(), (rule, skip_rule, key)
            assert bool((o == 0x80000000).any()) == shows_minus_zero, (rule, skip_rule, key)
        assert any(c[2] for c in cases if c[0][0] == 1), (rule, skip_rule)
