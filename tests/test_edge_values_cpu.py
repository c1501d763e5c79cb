"""Preconditions of test_gpu_edge_values.py, asserted without a GPU: the data of edge_values.py reach every edge class they
are there for.  If one of these fails the GPU file still passes, but no longer tests what it says."""
import numpy as np
import pytest
import torch

import edge_values as ev


@pytest.mark.parametrize("shape", ev.WARP_PLANES + ev.WARP_DEGENERATE, ids=lambda s: "x".join(map(str, s)))
def test_flow_fields_reach_every_class_of_flow_warp(shape):
    """over the flow kinds of one plane: a zero weight (exact grid hit), a right and a lower neighbour outside the image
    (x1ok / y1ok false), the clamp at either end; and every position inside the image after the clamp, whatever the flow —
    warp_classes asserts that, NaN and infinite flows included"""
    N, _, H, W = shape
    reached = {}
    for kind in ev.FLOWS:
        for fn in sorted({1, N}):
            reached[kind] = ev.warp_classes(ev.flow(kind, fn, H, W), H, W) | reached.get(kind, set())
    assert set().union(*reached.values()) == ev.WARP_CLASSES
    assert {"w==0", "x1ok false", "y1ok false"} <= reached["integer"]
    assert {"clamp low", "clamp high"} <= reached["big"] and {"clamp low", "clamp high"} <= reached["inf"]
    assert "clamp low" in reached["nan"]                              # fmaxf(NaN, 0) = 0
    assert "w==0" in reached["pzero"] and "w==0" in reached["nzero"]


@pytest.mark.parametrize("shape", [s for s in ev.WARP_PLANES if min(s[2:]) >= 7], ids=lambda s: "x".join(map(str, s)))
def test_warped_quantised_image_has_zeros_of_both_signs(shape):
    from pmctf_oracle import clib
    N, _, H, W = shape
    lx, ly = ev.lin_tables(H, W)
    im = ev.quantised(shape)
    for kind in ("integer", "pzero", "normal"):
        out = clib.flow_warp(im, ev.flow(kind, 1, H, W), lx, ly)
        assert all(ev.zero_signs(out)) or kind == "normal", kind
    assert ev.zero_signs(clib.flow_warp(ev.pixel(shape), ev.flow("normal", 1, H, W), lx, ly)) == (False, False)


@pytest.mark.parametrize("shape", ev.RESAMPLE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_resampling_planes_hold_what_they_are_named_for(shape):
    q = ev.quantised(shape).view(np.uint32)
    assert (q[..., 0:2, 0:2] == 0x80000000).all(), "no all -0 window"
    if shape[3] >= 4:
        win = q[0, 0, 0:2, 2:4].reshape(-1).tolist()
        assert sorted(win) == [0, 0, 0x80000000, 0x80000000], "no window that mixes the signs of zero"
    if shape[2] * shape[3] >= 1000:
        assert 0.5 < (ev.quantised(shape) == 0).mean() < 0.7          # P(|N(0, 0.6)| < 0.5) = 0.595
    s = ev.subnormal(shape)
    assert (np.abs(s) < np.finfo(np.float32).tiny).all()
    if s.size >= 63:
        assert all(ev.zero_signs(s)) and (s > 0).any() and (s < 0).any()
    i = ev.islands(shape)
    assert np.isnan(i).any()
    if shape[2] >= 8 and shape[3] >= 8:
        assert np.isposinf(i).any() and np.isneginf(i).any()


@pytest.mark.parametrize("shape", ev.LSTM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_lstm_data_hold_the_special_set(shape):
    xh, cell = ev.lstm_data(shape)
    assert set(ev.SPECIALS.view(np.uint32).tolist()) <= set(xh.view(np.uint32).reshape(-1).tolist())
    assert all(ev.zero_signs(cell)) and np.isposinf(cell).any() and np.isneginf(cell).any()


def test_u8_patterns_are_round_of_clamp():
    """the documented byte of each pattern is torch's: clamp(x, 0, 255).round() (ties to even), NaN to 0"""
    vals = torch.tensor([v for v, _ in ev.U8_PATTERNS], dtype=torch.float32)
    want = torch.nan_to_num(vals, nan=0.0, posinf=float("inf"), neginf=float("-inf")).clamp(0, 255).round().to(torch.uint8)
    assert want.tolist() == [b for _, b in ev.U8_PATTERNS]
    assert {0.5, 1.5, 254.5, 255.5, -0.5} <= {v for v, _ in ev.U8_PATTERNS}
