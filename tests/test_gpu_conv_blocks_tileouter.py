"""Rule-"blocks" 3x3 convolution with 7 cout tiles in one launch (conv3x3s1_blocks_tileouter_kernel, cout tile as the
outer loop of a 16-channel chunk): bit for bit the oracle's C convolution AND the 4 + 3 two-launch path it replaces
(knob BSUM_TILEOUTER = 0), on the shapes at which its staging, its row range and its partial tiles can go wrong."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import assert_same

pytestmark = pytest.mark.gpu

NEW = "conv3x3s1_blocks_tileouter_kernel"
OLD = ("conv3x3s1_wave_kernel<4, 2, true, 0>", "conv3x3s1_wave_kernel<3, 2, true, 4>")
REMAINDER = "conv3x3s1_pipe_kernel<MT, 1, true>"
DEFAULTS = {"NT": 0, "MSPLIT_PX": 70000, "BSUM_TILEOUTER": 1}
FORCE_8X32 = {"NT": 4, "MSPLIT_PX": 0}

CASES = {
    # (N, Cin, H, W, Cout), act, slope, residual adds, knobs
    "seven_chunks_ragged": ((1, 112, 20, 36, 112), 2, 0.2, 0, FORCE_8X32),     # waves whose tile lies outside the plane
    "one_chunk_one_tile": ((1, 16, 8, 32, 112), 0, 0.0, 0, FORCE_8X32),       # no next-patch fetch or stash
    "two_planes_two_chunks": ((2, 32, 9, 17, 112), 1, 0.0, 1, FORCE_8X32),    # one row and one column past a tile
    "below_a_wave_tile": ((1, 112, 5, 3, 112), 0, 0.0, 2, FORCE_8X32),        # every halo slot zero
    "partial_last_cout_tile": ((1, 112, 24, 33, 100), 0, 0.0, 1, FORCE_8X32),
    "two_m_blocks": ((1, 48, 24, 40, 224), 2, 0.2, 1, FORCE_8X32),            # 224 couts = two packed 7-tile blocks in grid.z
    "rounds_plus_remainder": ((1, 16, 264, 520, 112), 0, 0.0, 0, {}),         # row range oy_end < Ho, then 4x16 tiles
}


def _nhwc(x):
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 1))).cuda()


def _nchw(t):
    return t.cpu().numpy().transpose(0, 3, 1, 2)


def _last_launch(L):
    buf = C.create_string_buffer(512)
    assert L.pmctf_conv2d_last_launch(buf, 512) == 0
    return buf.value.decode()


def _run_both_arms(x, w, b, act, slope, res, knobs):
    """The convolution with BSUM_TILEOUTER = 1 and = 0 under `knobs`: ((y, launch string) per arm)."""
    from pMCTF.hip import lib, ops
    L = lib.hip()
    conv = ops.Conv2d(torch.from_numpy(w), torch.from_numpy(b), 1, (1, 1), rule=ops.SUM_BLOCKS)
    xd = _nhwc(x)
    rd = [_nhwc(q) for q in res]
    out = []
    try:
        for arm in (1, 0):
            for k, v in {**DEFAULTS, **knobs, "BSUM_TILEOUTER": arm}.items():
                assert L.pmctf_conv2d_set_option(k.encode(), v) == 0
            y = conv(xd, act=act, slope=slope, res1=rd[0] if len(rd) > 0 else None, res2=rd[1] if len(rd) > 1 else None)
            launched = _last_launch(L)
            torch.cuda.synchronize()
            out.append((_nchw(y), launched))
    finally:
        for k, v in DEFAULTS.items():
            L.pmctf_conv2d_set_option(k.encode(), v)
    return out


def _check_arms(arms, ref, what, remainder):
    (y1, l1), (y0, l0) = arms
    assert NEW in l1 and not any(o in l1 for o in OLD), l1
    assert all(o in l0 for o in OLD) and NEW not in l0, l0
    assert (REMAINDER in l1) == remainder and (REMAINDER in l0) == remainder, (l1, l0)
    assert_same(y1, ref, f"{what}: tile-outer kernel vs oracle")
    assert_same(y0, ref, f"{what}: 4 + 3 launches vs oracle")
    assert_same(y1, y0, f"{what}: tile-outer kernel vs 4 + 3 launches")


@pytest.mark.parametrize("name", list(CASES))
def test_tileouter_bitexact(cuda, name):
    from pmctf_oracle import clib
    (N, Cin, H, W, Cout), act, slope, nres, knobs = CASES[name]
    r = np.random.default_rng(4100 + Cin * 7 + Cout + H)
    x = r.standard_normal((N, Cin, H, W), dtype=np.float32) * 3
    w = (r.standard_normal((Cout, Cin, 3, 3), dtype=np.float32) * 0.05).astype(np.float32)
    b = r.standard_normal(Cout, dtype=np.float32)
    ref = clib.conv2d(x, w, b, 1, (1, 1), 1)
    if act == 1:
        ref = np.maximum(ref, 0)
    elif act == 2:
        ref = np.where(ref > 0, ref, ref * np.float32(slope)).astype(np.float32)
    res = [r.standard_normal(ref.shape, dtype=np.float32) for _ in range(nres)]
    for q in res:
        ref = ref + q
    _check_arms(_run_both_arms(x, w, b, act, slope, res, knobs), ref, f"conv {name}", remainder=not knobs)


def scaled_chunks_case():
    """(1, 112, 16, 32, 112): the input channels of chunk c scaled by 10^(c-3) and half the weights negated, so that the
    chunk sums differ by orders of magnitude and cancel inside a chunk: a fold in the wrong order, or a chain continued
    across chunks, changes bits."""
    r = np.random.default_rng(4242)
    x = r.standard_normal((1, 112, 16, 32), dtype=np.float32)
    x *= np.repeat(np.float32(10.0) ** np.arange(-3, 4, dtype=np.float32), 16)[None, :, None, None]
    w = np.abs(r.standard_normal((112, 112, 3, 3), dtype=np.float32) * 0.05).astype(np.float32)
    w = np.where(r.random(w.shape) < 0.5, -w, w).astype(np.float32)
    b = r.standard_normal(112, dtype=np.float32)
    return x, w, b


def test_tileouter_fold_order(cuda):
    from pmctf_oracle import clib
    x, w, b = scaled_chunks_case()
    ref = clib.conv2d(x, w, b, 1, (1, 1), 1)
    chain = clib.conv2d(x, w, b, 1, (1, 1), 0)
    assert (ref != chain).mean() > 0.5, "the input does not tell rule blocks from rule chain"
    _check_arms(_run_both_arms(x, w, b, 0, 0.0, [], FORCE_8X32), ref, "conv scaled chunks", remainder=False)
