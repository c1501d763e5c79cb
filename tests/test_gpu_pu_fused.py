"""The fused PredictUpdate kernel (csrc/pu_fused.hip) through its own entry, ops.predict_update_fused, bit for bit
against pu_fused_reference.py (the oracle's C primitives composed in the kernel's written order): both weight scales,
every (rule, skip_rule) pair, both modes and five plane shapes.  That the data tells the rule pairs apart is checked
without a GPU in test_pu_fused_reference_cpu.py."""
import numpy as np
import pytest
import torch

from pu_fused_reference import (F, MODE0_C, RULES, SCALES, SHAPES, ZERO_BIASES, ZERO_SHAPES, inputs, reference, weights,
                                zero_inputs, zero_reference, zero_weights)

pytestmark = pytest.mark.gpu


def assert_same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    neq = got.view(np.uint32) != want.view(np.uint32)
    if neq.any():
        i = tuple(np.argwhere(neq)[0])
        raise AssertionError(f"{what}: {int(neq.sum())}/{got.size} bit patterns differ; first at {i}: {got[i]!r} vs {want[i]!r}")


@pytest.fixture(scope="module")
def layers_on_device(cuda):
    from pMCTF.hip import ops
    made = {}

    def get(scale, rule):
        if (scale, rule) not in made:
            made[scale, rule] = tuple(ops.Conv2d(torch.from_numpy(w), torch.from_numpy(b), 1, (1, 1), rule=rule)
                                      for w, b in weights(scale)[0])
        return made[scale, rule]
    return get


@pytest.mark.parametrize("rule,skip_rule", RULES, ids=[f"rule{r}_skip{s}" for r, s in RULES])
@pytest.mark.parametrize("scale", list(SCALES), ids=list(SCALES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_predict_update_fused_bitexact(cuda, layers_on_device, shape, scale, rule, skip_rule):
    from pMCTF.hip import ops
    s = SCALES[scale]
    pu = layers_on_device(s, rule)
    lift = weights(s)[1]
    x0, x1, other = (torch.from_numpy(a).cuda() for a in inputs(shape, s))
    if skip_rule == 0:                                  # mode 0 has no lifting filter: once per rule
        want = reference(shape, s, rule, 0, 0)[0]
        for c in MODE0_C:
            got = ops.predict_update_fused(x0, None, pu, 0, c=c)
            assert_same_bits(got.cpu().numpy(), want[c], f"mode 0 {shape} scale {s} rule {rule} c {c}")
    want = reference(shape, s, rule, skip_rule, 1)[0]
    for sign in (1.0, -1.0):
        got = ops.predict_update_fused(x1, other, pu, 1, sign=sign, lift=lift, skip_rule=skip_rule)
        assert_same_bits(got.cpu().numpy(), want[sign], f"mode 1 {shape} scale {s} rule {rule} skip rule {skip_rule} sign {sign}")


@pytest.mark.parametrize("rule,skip_rule", RULES, ids=[f"rule{r}_skip{s}" for r, s in RULES])
@pytest.mark.parametrize("biases", ZERO_BIASES)
@pytest.mark.parametrize("shape", ZERO_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_predict_update_fused_on_zeros_of_both_signs(cuda, shape, biases, rule, skip_rule):
    """the zero data of the convolution censuses through all four layers and the lifting arithmetic: -0 biases (the lifting
    filter's too) and the biases of the other cases; both modes, every (rule, skip_rule) pair.  That the reference holds
    both signs of zero is asserted in test_pu_fused_reference_cpu.py."""
    from pMCTF.hip import ops
    layers, lift = zero_weights(biases)
    pu = tuple(ops.Conv2d(torch.from_numpy(w), torch.from_numpy(b), 1, (1, 1), rule=rule) for w, b in layers)
    x0, x1, other = (torch.from_numpy(a).cuda() for a in zero_inputs(shape))
    if skip_rule == 0:
        want = zero_reference(shape, biases, rule, 0, 0)
        for c in MODE0_C:
            got = ops.predict_update_fused(x0, None, pu, 0, c=c)
            assert_same_bits(got.cpu().numpy(), want[c], f"zeros, mode 0 {shape} biases {biases} rule {rule} c {c}")
    want = zero_reference(shape, biases, rule, skip_rule, 1)
    for sign in (1.0, -1.0):
        got = ops.predict_update_fused(x1, other, pu, 1, sign=sign, lift=lift, skip_rule=skip_rule)
        assert_same_bits(got.cpu().numpy(), want[sign],
                         f"zeros, mode 1 {shape} biases {biases} rule {rule} skip rule {skip_rule} sign {sign}")
