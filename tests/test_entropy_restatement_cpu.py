"""What can be said about the entropy-stage element kernels without a GPU: tests/entropy_restatement.py agrees with the
oracle's functions that describe the same thing (so the plain reference of tests/test_gpu_entropy_kernels.py is pinned to
the one the byte-identical files vouch for), the estimate edge grid tests the definition and not an accident of it, every
totals case satisfies the condition its summation bound needs, and every entry point refuses the arguments its guard
lists."""
import os
import re

import numpy as np
import pytest
import torch

import entropy_restatement as er
from helpers import assert_same, synth_sd_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("fourstep_quant", "ll_quant", "z_symbols", "mv_fourpart_step", "mv_dequant", "fourstep_dequant",
                "mv_fourpart_dequant", "sym_to_nhwc", "fourstep_estimate", "ll_estimate", "z_estimate",
                "mv_fourpart_estimate", "sqdiff_sum")


@pytest.fixture(scope="module")
def orc():
    from pmctf_oracle.model import Oracle
    return Oracle(synth_sd_cpu(1), 1, "torch")


def _record(o, name):
    """calls of the oracle's method `name`: [(args, result)]"""
    calls, real = [], getattr(o, name)

    def wrapper(*a, **kw):
        out = real(*a, **kw)
        calls.append((a, out))
        return out
    setattr(o, name, wrapper)
    return calls


def _mixed(shape, seed, scale):
    """random values with ties, +-0 and symbols past the int16 clamp among them"""
    r = np.random.default_rng(seed)
    v = (r.standard_normal(shape) * scale).astype(np.float32)
    f = v.reshape(-1)
    f[::2] = er.EDGE_RES[np.arange(f[::2].size) % er.EDGE_RES.size]
    return torch.from_numpy(v)


@pytest.mark.parametrize("H,W", [(6, 10), (5, 7)])
def test_fourstep_agrees_with_fusion_compress(orc, H, W):
    """each step restated alone, fed the oracle's own per-step (scales, means), chained through so_far: the oracle's final
    so_far, its symbols and its CDF rows.  (5, 7): odd sizes, the masks cut from a repeat of (H+1)/2 x (W+1)/2 tiles."""
    p = "hp_coder.context_fusion.3.lh"
    cin = orc.sd[p + ".conv1_context.weight"].shape[1]
    x = _mixed((2, 1, H, W), 3, 4.0)
    ctx = torch.from_numpy(np.random.default_rng(4).standard_normal((2, cin, H, W)).astype(np.float32))
    calls = _record(orc, "process_with_mask")
    try:
        qs, ss, so_far = orc.fusion_compress(p, x, ctx, None)
    finally:
        del orc.process_with_mask
    assert len(calls) == 4
    prev, back = None, None
    for k, ((xk, scales, means, _), _) in enumerate(calls):
        assert xk is x
        prev, sym, idx = er.fourstep_quant(x, scales, means, prev, k)
        assert_same(sym, er.sym16(qs[k]).reshape(-1), f"symbols of step {k}")
        assert_same(idx, er.rows(ss[k]).reshape(-1), f"rows of step {k}")
        est, bits = er.fourstep_estimate(x, scales, means, None if k == 0 else est, k)
        back = er.fourstep_dequant(sym, means, back, k)
        assert_same(est, prev, f"estimate so_far of step {k}")
        live = er.Oracle.masks4(H, W)[k][0, 0] > 0
        want = er.K.laplace_bits(qs[k], ss[k])
        for n in range(2):
            assert_same(bits[n], want[n, 0][live], f"bits of step {k}, plane {n}")
    assert_same(prev, so_far, "so_far after four steps")
    clamped = (qs[0] + qs[1] + qs[2] + qs[3]).abs() > 30000
    assert clamped.any() and not clamped.all()
    assert_same(torch.where(clamped, prev, back), so_far, "decoder's so_far where the symbol was not clamped")


def test_mv_fourpart_agrees_with_compress_four_part_prior(orc):
    H, W = 4, 6
    r = np.random.default_rng(5)
    y = _mixed((1, 64, H, W), 6, 3.0)
    common = torch.from_numpy(r.standard_normal((1, 192, H, W)).astype(np.float32))
    common[:, :64] = torch.from_numpy(er.MV_QSTEPS[r.integers(0, er.MV_QSTEPS.size, (1, 64, H, W))])
    calls = _record(orc, "process_with_mask")
    try:
        y_q, y_hat, scales_hat = orc.compress_four_part_prior(0, y, common, full=True)
        n_full = len(calls)
        qw, sw, y_hat_w = orc.compress_four_part_prior(0, y, common)
    finally:
        del orc.process_with_mask
    assert n_full == 16 and len(calls) == 32
    assert_same(y_hat_w, y_hat, "the oracle's two forms")
    prev = back = None
    m = er.Oracle.masks4(H, W)
    y_q_mine = torch.zeros(1, 64, H, W)
    for t in range(4):
        step = calls[4 * t:4 * t + 4]                   # groups 0..3 of step t: (y_g, scales_g, means_g, mask)
        sp = None if t == 0 else torch.cat([c[0][1] for c in step] + [c[0][2] for c in step], 1)
        if t == 0:
            assert_same(torch.cat([c[0][1] for c in step], 1), common[:, 64:128], "step 0 takes the common scales")
        for g in range(4):
            assert torch.equal(step[g][0][3], m[er.MV_PERMS[t][g]]), (t, g)
        prev, sym, idx = er.mv_fourpart_step(y, common, sp, prev, t)
        assert_same(sym, er.sym16(qw[t]).reshape(-1), f"symbols of step {t}")
        assert_same(idx, er.rows(sw[t]).reshape(-1), f"rows of step {t}")
        est, bits = er.mv_fourpart_step(y, common, sp, None if t == 0 else est, t, estimate=True)
        assert_same(est, prev, f"estimate so_far of step {t}")
        back = er.mv_fourpart_dequant(sym, common, sp, back, t)
        for g in range(4):
            y_q_mine[:, 16 * g:16 * g + 16] += sym.reshape(1, 16, H, W).float() * m[er.MV_PERMS[t][g]]
    assert_same(er.mv_dequant(prev, common), y_hat, "y_hat")
    assert_same(y_q_mine, y_q.clamp(-30000, 30000), "y_q from the four pushes")
    assert_same(er.mv_dequant(back, common), torch.where(y_q.abs() > 30000, er.mv_dequant(back, common), y_hat),
                "decoder's y_hat where the symbol was not clamped")
    assert (y_q.abs() > 30000).any()
    want_bits = er.K.laplace_bits(y_q, scales_hat)
    got = torch.zeros(1, 64, H, W)
    est = None
    for t in range(4):
        step = calls[4 * t:4 * t + 4]
        sp = None if t == 0 else torch.cat([c[0][1] for c in step] + [c[0][2] for c in step], 1)
        est, bits = er.mv_fourpart_step(y, common, sp, est, t, estimate=True)
        got[torch.cat([m[er.MV_PERMS[t][g]].expand(1, 16, H, W) for g in range(4)], 1) > 0] = bits
    assert_same(got, want_bits, "per-element bits")


@pytest.mark.parametrize("N,skip_decoding", [(1, True), (2, True), (2, False)])
def test_ll_agrees_with_pwave_compress(orc, N, skip_decoding):
    """the LL lines of pwave_compress on a 64x64 picture (4x4 LL): ll_hat, the pushed symbols and rows in both orders"""
    x = torch.from_numpy((np.random.default_rng(8).standard_normal((N, 1, 64, 64)) * 900 + 128).astype(np.float32))
    net = _record(orc, "context_fusion_ll")
    push = _record(orc, "gaussian_encode")
    ctxs = _record(orc, "ctx_forward_one_subband")
    try:
        orc.pwave_compress("lp_coder", x, [1, N, 64, 64], 0, skip_decoding=skip_decoding)
    finally:
        del orc.context_fusion_ll, orc.gaussian_encode, orc.ctx_forward_one_subband
    (_, ll), params = net[0]
    scales, means = params.chunk(2, dim=1)
    ll_hat, sym, idx = er.ll_quant(ll, scales, means, ar_order=not skip_decoding)
    assert_same(ll_hat, ctxs[0][0][1], "ll_hat")
    q, sc = push[0][0]
    assert_same(sym, er.sym16(q).reshape(-1), "symbols")
    assert_same(idx, er.rows(sc).reshape(-1), "rows")
    assert (means != means.round()).any() and sym.abs().max() > 0
    if N > 1 and not skip_decoding:
        assert not torch.equal(sym, er.ll_quant(ll, scales, means, False)[1])


def _laplace_bits_clamped(y, sigma, lo, hi=1e10):
    """CdefK.laplace_bits line by line with another sigma clamp: what a kernel with the wrong clamp would compute"""
    from pmctf_oracle import clib
    sigma = sigma.clamp(lo, hi)

    def cdf(v):
        e = torch.from_numpy(clib.exp((-v.abs() / sigma).numpy())) - 1.0
        return 0.5 - 0.5 * v.sign() * e
    return er.K._neglog2(cdf(y + 0.5) - cdf(y - 0.5))


def test_edge_grid_tests_the_definition():
    """18 y x 15 sigma: finite, between 0 and the cap -log2(1e-5), both ends reached, 47 different values; the PM-F32
    definition stays within 3e-4 bits of the reference's own expressions on it (seen: 1.7e-4).  The grid itself, not
    random data, tells the lower sigma clamp from a smaller one: with 1e-6 in place of 1e-5 the twelve elements (y one ulp
    off +-0.5) x (sigma <= 1e-5) change.  It cannot tell sgn(0) = 0 from sgn(0) = 1 in the cdf, and nothing can: the
    factor the sign scales is pm_exp(-0) - 1, and pm_exp(-0.0) is exactly 1."""
    from pmctf_oracle import clib
    from pmctf_oracle.kernels import TorchK
    y, s = er.edge_grid()
    assert y.numel() == 270 and len(set(er.EDGE_Y.view(np.int32).tolist())) == 18
    b = er.K.laplace_bits(y, s)
    assert torch.isfinite(b).all()
    assert float(b.min()) == 0.0 and f"{float(b.max()):.8f}" == "16.60964012"
    assert int((b == 0).sum()) == 12 and int((b == b.max()).sum()) == 140 and len(set(b.tolist())) == 47
    assert float((b - TorchK().laplace_bits(y, s)).abs().max()) <= 3e-4
    assert_same(_laplace_bits_clamped(y, s, 1e-5), b, "the line-by-line copy used below")
    moved = _laplace_bits_clamped(y, s, 1e-6) != b
    assert int(moved.sum()) == 12
    assert (s[moved] <= 1.0000001e-5).all() and ((y[moved].abs() - 0.5).abs() < 1e-6).all() and (y[moved].abs() != 0.5).all()
    assert clib.exp(np.array([-0.0, 0.0], np.float32)).tolist() == [1.0, 1.0]
    yr, sr = er.random_pairs(100000, 1)
    br = er.K.laplace_bits(yr, sr)
    assert torch.isfinite(br).all() and float(br.min()) >= 0.0 and float(br.max()) <= float(b.max())


def test_totals_cases_satisfy_the_condition_of_their_bound():
    """|got - sum64 v| <= n * 2^-53 * sum |v| can only catch a dropped or doubled element if that bound is below half the
    smallest nonzero v: for the reference alone, in every totals case of the GPU file"""
    cases = er.totals_cases()
    assert len(cases) > 40
    for name, vs in cases.items():
        for v in vs:
            assert v.dtype == torch.float32 and v.numel() > 0 and torch.isfinite(v).all(), name
            assert (v != 0).any() or v.numel() == 1, name
            bound, half = er.summation_bound(v), er.half_smallest(v)
            assert bound < half, (name, v.numel(), bound, half)
            if v.numel() <= 4096 and (v != 0).any():   # as sharp as a per-element check: below one float32 ulp of the values
                assert bound < float(np.spacing(np.float32(v.abs().max()))), (name, bound)
    big = cases["ll 1x1088x1920"][0]
    assert big.numel() == 1088 * 1920 and er.summation_bound(big) < 0.005


def test_every_parity_class_meets_every_edge():
    """the inputs of the GPU file: each class k of the four-step cases, and each step of the MV cases, sees all 28 edge
    residuals (x - mean in float32 returns them) and all 15 edge scales"""
    for (N, H, W) in ((2, 36, 60), (2, 37, 53), (6, 68, 120)):
        for k, (x, sc, mu) in enumerate(er.fourstep_inputs(N, H, W)):
            on = er.Oracle.masks4(H, W)[k].expand(N, 1, H, W) > 0
            res = set((x - mu)[on].numpy().view(np.int32).tolist())
            assert set(er.EDGE_RES.view(np.int32).tolist()) <= res, (N, H, W, k)
            assert set(er.EDGE_SCALES.view(np.int32).tolist()) <= set(sc[on].numpy().view(np.int32).tolist()), (N, H, W, k)
            assert (x[~on] == er.GARBAGE).all() and (sc[~on] == er.GARBAGE).all() and (mu[~on] == er.GARBAGE).all()
    ll, sc, mu = er.ll_inputs(2, 17, 30)
    assert set(er.EDGE_SCALES.view(np.int32).tolist()) <= set(sc.numpy().view(np.int32).reshape(-1).tolist())
    assert ((ll - ll.round()).abs() == 0.5).any() and ((mu - mu.round()).abs() == 0.5).any()
    y, common, sps = er.mv_inputs(18, 30)
    q = common[:, :64]
    assert (q < 0.5).any() and (q == 0.5).any() and (q > 0.5).any()


P = 0x1000       # a made-up pointer: passed only together with an argument that must be refused


def _calls():
    """entry point -> (valid argument list with made-up pointers, pointer positions that must not be null,
    [(position, refused value)])"""
    lm, ls = 0.0, 1.0
    return {
        "pmctf_fourstep_quant_f32": ([P, P, P, P, P, 2, 4, 6, 0, 0, lm, ls, None], [0, 1, 2, 3, 4],
                                     [(8, -1), (8, 4), (5, 0), (6, 0), (7, 0)]),
        "pmctf_ll_quant_f32": ([P, P, P, P, P, 12, 0, lm, ls, None], [0, 1, 2, 3, 4], [(5, 0), (6, -1), (6, 5)]),
        "pmctf_z_symbols_f32": ([P, P, P, P, 6, 64, None], [0, 1, 2, 3], [(4, 0), (5, 0)]),
        "pmctf_mv_fourpart_step_f32": ([P, P, P, P, P, P, 4, 6, 1, lm, ls, None], [0, 1, 3, 4, 5],
                                       [(8, -1), (8, 4), (6, 0), (7, 0), (2, None)]),
        "pmctf_mv_dequant_f32": ([P, P, P, 24, None], [0, 1, 2], [(3, 0)]),
        "pmctf_fourstep_dequant_f32": ([P, P, P, 2, 4, 6, 0, 0, None], [0, 1, 2], [(6, -1), (6, 4), (3, 0), (4, 0), (5, 0)]),
        "pmctf_mv_fourpart_dequant_f32": ([P, P, P, P, 4, 6, 1, None], [0, 1, 3], [(6, -1), (6, 4), (4, 0), (5, 0), (2, None)]),
        "pmctf_sym_to_nhwc_f32": ([P, P, 6, 64, None], [0, 1], [(2, 0), (3, 0)]),
        "pmctf_fourstep_estimate_f32": ([P, P, P, 2, 4, 6, 0, 0, P, None], [0, 1, 2, 8],
                                        [(6, -1), (6, 4), (3, 0), (3, 65536), (4, 0), (5, 0)]),
        "pmctf_ll_estimate_f32": ([P, P, 2, 24, P, None], [0, 1, 4], [(2, 0), (2, 65536), (3, 0)]),
        "pmctf_z_estimate_f32": ([P, P, P, 6, 64, P, None], [0, 1, 2, 5], [(3, 0), (4, 0)]),
        "pmctf_mv_fourpart_estimate_f32": ([P, P, P, P, 4, 6, 1, P, None], [0, 1, 3, 7],
                                           [(6, -1), (6, 4), (4, 0), (5, 0), (2, None)]),
        "pmctf_sqdiff_sum_f32": ([P, P, 24, P, None], [0, 1, 3], [(2, 0)]),
    }


def test_every_entry_point_refuses_what_its_guard_lists():
    """PMCTF_EINVAL before any launch: null pointers, k / t outside 0..3, empty shapes, N > 65535, t > 0 without sp, and
    the quarter-size parameter layout on an odd plane"""
    from pMCTF.hip import lib
    L = lib.hip()
    calls = _calls()
    assert sorted(calls) == sorted(f"pmctf_{n}_f32" for n in ENTRY_POINTS)
    for name, (args, ptrs, refused) in calls.items():
        fn = getattr(L, name)
        for i in ptrs:
            a = list(args)
            a[i] = None
            assert fn(*a) == -1, (name, "null pointer", i)
        for i, v in refused:
            a = list(args)
            a[i] = v
            assert fn(*a) == -1, (name, i, v)
    for name, (hpos, wpos, spos) in {"pmctf_fourstep_quant_f32": (6, 7, 9), "pmctf_fourstep_dequant_f32": (4, 5, 7),
                                     "pmctf_fourstep_estimate_f32": (4, 5, 7)}.items():
        for pos in (hpos, wpos):
            a = list(calls[name][0])
            a[spos] = 1
            a[pos] = 5
            assert getattr(L, name)(*a) == -1, (name, "params_sub on an odd plane")


# what else csrc/ew_ops.hip and csrc/decode_ops.hip export: layout / network kernels, each reached by name through its ops
# wrapper in a tests/test_gpu_*.py (test_math_sweep_cpu.py::test_every_layout_and_network_kernel_has_a_direct_gpu_test
# keeps that true), the sequential LL decoder (test_gpu_ll_decode.py), and the two CDF-row kernels of the decoder
# (test_scale_index_rows_at_every_gpu_site, test_gpu_math_sweep.py::test_cdf_row_of_every_scale)
OTHER_EXPORTS = {
    "ew_ops": {"pmctf_ew_f32", "pmctf_spynet_pack8_f32", "pmctf_lift_skip3_f32", "pmctf_nearest_up2_nhwc_f32",
               "pmctf_pixel_shuffle2_nhwc_f32", "pmctf_ffn3_mix_f32", "pmctf_lstm_gates_f32", "pmctf_lstm_gates_aten_f32",
               "pmctf_ew_last_launch"},
    "decode_ops": {"pmctf_ll_ar_packed_size", "pmctf_ll_ar_pack_weights", "pmctf_ll_ar_scratch_floats",
                   "pmctf_ll_ar_decode_f32", "pmctf_ll_ar_decode_rules_f32", "pmctf_ll_ar_batch_form",
                   "pmctf_ll_ar_decode_batch_f32", "pmctf_fourstep_indexes_f32", "pmctf_mv_fourpart_indexes_f32"},
    "estimate_ops": set(),
}


def test_gpu_file_calls_every_entry_point_by_name():
    """the GPU file names each of the thirteen entry points, and the three sources export these thirteen plus the listed
    others and nothing else: an entry point added to one of them shows up here until it is given a test or listed"""
    text = open(os.path.join(ROOT, "tests", "test_gpu_entropy_kernels.py")).read()
    for name in ENTRY_POINTS:
        assert re.search(rf"\bops\.{name}\(", text), f"tests/test_gpu_entropy_kernels.py never calls ops.{name}"
    exported = set()
    for f, others in OTHER_EXPORTS.items():
        src = open(os.path.join(ROOT, "learned-pmctf_amd", "csrc", f + ".hip")).read()
        found = set(re.findall(r'extern "C" \w+ (pmctf_\w+)\(', src))
        assert others <= found, (f, others - found)
        exported |= found - others
    assert exported == {f"pmctf_{n}_f32" for n in ENTRY_POINTS}, exported ^ {f"pmctf_{n}_f32" for n in ENTRY_POINTS}
