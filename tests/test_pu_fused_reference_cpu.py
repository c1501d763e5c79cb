"""Precondition of test_gpu_pu_fused.py, on the oracle alone: the references of the (rule, skip_rule) pairs are told
apart by the test's data, and the large weights saturate most tanh values."""
import itertools

import pytest

from pu_fused_reference import MODE0_C, RULES, SCALES, reference


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
