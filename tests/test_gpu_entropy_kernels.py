"""The thirteen element kernels between the networks and the range coder, each called alone through pMCTF.hip.ops and
compared with tests/entropy_restatement.py: every float tensor and every int16 buffer bit for bit, every bit total within
the worst-case error of its float64 summation.

  encode    fourstep_quant, ll_quant, z_symbols, mv_fourpart_step, mv_dequant            (csrc/ew_ops.hip)
  decode    fourstep_dequant, mv_fourpart_dequant, sym_to_nhwc                           (csrc/decode_ops.hip)
  estimate  fourstep_estimate, ll_estimate, z_estimate, mv_fourpart_estimate, sqdiff_sum (csrc/estimate_ops.hip)

Inputs mix, at known positions, residuals on +-0.5 / 1.5 / 2.5 and one ulp either side, +-0.0, means that are not
integers, |q| of 29999 / 30000 / 30001 / 40000 (the symbol clamps, so_far does not), the scales 0, -1, 1e-6 ... 1e10,
3e10, +inf, MV quant_step below, at and above 0.5, and 1e30 wherever a step must not read.  Outputs are cut from the
middle of sentinel-filled buffers (int16: at an odd offset) and the sentinels are looked at afterwards.

The only tolerance in this file is n * 2^-53 * sum|v| on a total of n float32 values v: the worst-case error of any
order of float64 additions, which is what "block tree + one f64 atomic per wave" promises.  tests/
test_entropy_restatement_cpu.py asserts for each of these cases that the bound is below half the smallest nonzero v, so a
dropped or doubled element cannot hide in it.  Per-element bits are checked with == through launches that leave one
live element per accumulated double.

Out of scope: NaN anywhere, +-inf in x or mean.  (The kernels' sigma clamp maps a NaN scale to 1e-5 where torch
propagates it; nothing here asserts either.)

What each of these one-line changes to the kernels turns red (each keeps every index in range, or inside the guard
band of this file's buffers; applied one at a time to a scratch copy, this file run once on an MI355X):

  laplace_bits: lower sigma clamp 1e-5f -> 1e-6f            test_bits_per_element_ll
  fourstep_estimate_kernel: no `so_far = 0` for k == 0      test_fourstep (all 10), test_bits_per_element_fourstep (both)
  MV_PERM: {3,2,1,0} -> {2,3,1,0}                           test_mv_fourpart (all 4)
  MVE_PERM: the same                                        test_mv_fourpart (all 4)
  MVD_PERM: the same                                        test_mv_fourpart (all 4)
  fourstep_quant_kernel: grid-stride for -> if              test_fourstep_three_full_size_planes
  fourstep_estimate_kernel: grid-stride for -> if           test_fourstep[1-1088-1920-False], [1-1088-1920-True]
  sym16: clamp removed                                      test_fourstep (9), test_ll (13), test_z (4), test_mv_fourpart (4)
  ll_quant_kernel: pm_mod / pm_div exchanged (ar_order)     test_ll, the six cases with N > 1 and ar_order
  fourstep_quant_kernel: __builtin_rintf -> roundf          test_fourstep (all 10), test_fourstep_three_full_size_planes
  ll_quant_kernel: outer __builtin_rintf of ll_hat dropped  test_ll (all 19)
  lap_cdf: v > 0.0f -> v >= 0.0f                            nothing, and nothing can: at v = 0 the factor it scales is
                                                            pm_exp(-0 / sigma) - 1 = 0, so cdf(0) = 0.5 whatever sgn is;
                                                            the two kernels compute the same function of every input
                                                            (pm_exp(-0.0) == 1 exactly: asserted in the CPU test file)
"""
import contextlib

import numpy as np
import pytest
import torch

import entropy_restatement as er
from helpers import assert_same

pytestmark = pytest.mark.gpu

SENT_F = -7.25e33            # float sentinel: nothing a kernel computes here
SENT_I = -21846              # 0xAAAA
SENT_D = -1.5e300
G = 64                       # guard band, elements (a multiple of 4 floats: the cut keeps 16-byte alignment)
OFF = 37                     # odd, > 0: where a push starts in the int16 stream buffers


def _np(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t))


def assert_bits(got, want, what):
    """same shape, same dtype, same bits (float32: -0.0 is not +0.0)"""
    g, w = _np(got), _np(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    gi, wi = (a.view(np.int32) if a.dtype == np.float32 else a for a in (g, w))
    neq = gi != wi
    if neq.any():
        i = tuple(int(j) for j in np.argwhere(neq)[0])
        raise AssertionError(f"{what}: {int(neq.sum())}/{g.size} elements differ; first at {i}: {g[i]!r} vs {w[i]!r}")


class Guarded:
    """a contiguous tensor cut from the middle of a sentinel-filled 1-D buffer"""

    def __init__(self, shape, dtype=torch.float32, lead=G, init=None):
        self.n = int(np.prod(shape))
        self.lead = lead
        self.sent = {torch.float32: SENT_F, torch.int16: SENT_I, torch.float64: SENT_D}[dtype]
        self.buf = torch.full((lead + self.n + G,), self.sent, dtype=dtype, device="cuda")
        self.t = self.buf[lead:lead + self.n].view(shape)
        if init is not None:
            self.t.copy_(init)

    def check(self, what):
        edge = torch.cat([self.buf[:self.lead], self.buf[self.lead + self.n:]])
        assert_bits(edge, torch.full_like(edge, self.sent), f"{what}: written outside its output")


class _TorchWithGuardedOutputs:
    """stands in for the `torch` of pMCTF.hip.ops: what an op allocates for its result is a Guarded cut.  This leans on
    ops spelling its allocations torch.empty / torch.empty_like; guarded_results fails if an op allocated another way."""

    def __init__(self, made):
        self._made = made

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty_like(self, t):
        g = Guarded(tuple(t.shape), t.dtype)
        self._made.append(g)
        return g.t

    def empty(self, shape, dtype=torch.float32, device=None):
        g = Guarded(tuple(shape), dtype)
        self._made.append(g)
        return g.t


@contextlib.contextmanager
def guarded_results(what):
    from pMCTF.hip import ops
    made = []
    ops.torch = _TorchWithGuardedOutputs(made)
    try:
        yield made
    finally:
        ops.torch = torch
    torch.cuda.synchronize()
    assert made, what
    for g in made:
        g.check(what)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def params_dev(sc, mu, k, sub):
    """(N,H,W,2) = (scale, mean), or the quarter-size layout that holds only the class-k positions"""
    if sub:
        sc, mu = (v[:, :, (k >> 1)::2, (k & 1)::2] for v in (sc, mu))
    return torch.stack([sc[:, 0], mu[:, 0]], -1).contiguous().cuda()


def check_total(got, v, what, start=0.0, launches=1):
    """|got - (start + launches * sum64 v)| within the worst-case error of any order of float64 additions of those values"""
    n = launches * v.numel() + (1 if start else 0)
    mag = launches * float(v.double().abs().sum()) + abs(start)
    want = start + launches * er.total64(v)
    bound = n * 2.0 ** -53 * mag
    if start == 0.0 and launches == 1:
        assert bound == er.summation_bound(v) and bound < er.half_smallest(v), (what, bound)
    assert abs(got - want) <= bound, (what, got, want, got - want, bound)


def _fourstep(N, H, W, sub, estimate=True):
    from pMCTF.hip import ops
    lmin, lstep = er.lmin_lstep()
    steps = er.fourstep_inputs(N, H, W)
    n = N * H * W
    what0 = f"fourstep {N}x{H}x{W} sub={int(sub)}"
    so_q, so_e, so_d = (Guarded((N, 1, H, W)) for _ in range(3))      # step 0 finds sentinels, not zeros
    want_so = want_d = None
    any_clamped = False
    for k in range(4):
        what = f"{what0} k={k}"
        xk, sc, mu = steps[k]
        want_so, want_sym, want_idx = er.fourstep_quant(xk, sc, mu, want_so, k)
        want_d = er.fourstep_dequant(want_sym, mu, want_d, k)
        xd, pd = xk.cuda(), params_dev(sc, mu, k, sub)
        sym, idx = Guarded((n,), torch.int16, OFF), Guarded((n,), torch.int16, OFF)
        ops.fourstep_quant(xd, pd, so_q.t, sym.buf, idx.buf, OFF, k, lmin, lstep)
        assert_bits(so_q.t, want_so, what + " so_far")
        assert_bits(sym.t, want_sym, what + " sym")
        assert_bits(idx.t, want_idx, what + " idx")
        for g, name in ((so_q, "so_far"), (sym, "sym"), (idx, "idx")):
            g.check(f"{what} {name}")
        # decoder: the encoder's symbols back through the dequant kernel
        ops.fourstep_dequant(sym.t.clone(), pd, so_d.t, k)
        assert_bits(so_d.t, want_d, what + " dequant so_far")
        so_d.check(what + " dequant")
        if estimate:
            bits = Guarded((N,), torch.float64)
            bits.t.zero_()
            ops.fourstep_estimate(xd, pd, so_e.t, k, bits.t)
            assert_bits(so_e.t, so_q.t, what + " estimate so_far against quant so_far")
            so_e.check(what + " estimate so_far")
            bits.check(what + " bits")
            _, v = er.fourstep_estimate(xk, sc, mu, None, k)
            got = bits.t.cpu().tolist()
            for p in range(N):
                check_total(got[p], v[p], f"{what} plane {p}")
            start = 2048.0                               # onto what the doubles hold, twice (so_far: the same values again)
            bits.t.fill_(start)
            for _ in range(2):
                ops.fourstep_estimate(xd, pd, so_e.t, k, bits.t)
            got = bits.t.cpu().tolist()
            for p in range(N):
                check_total(got[p], v[p], f"{what} plane {p}, twice onto {start}", start=start, launches=2)
            assert_bits(so_e.t, so_q.t, what + " estimate so_far after three launches")
            bits.check(what + " bits")
    unclamped = (want_so - want_d) == 0
    any_clamped = bool((~unclamped).any())
    assert_bits(torch.where(unclamped.cuda(), so_d.t, so_q.t), so_q.t, what0 + ": decoder against encoder where |q| <= 30000")
    assert any_clamped or n < 28, what0


@pytest.mark.parametrize("N,H,W,sub", er.FOURSTEP_SHAPES + [(1,) + er.BIG_PLANE + (False,), (1,) + er.BIG_PLANE + (True,)],
                         ids=lambda v: str(v))
def test_fourstep(cuda, N, H, W, sub):
    """values, nothing else written, decoder = encoder, estimate = quantise, totals per plane; 1088x1920: the estimate
    kernel's grid-stride loop runs twice per plane"""
    _fourstep(N, H, W, sub)


def test_fourstep_three_full_size_planes(cuda):
    """6 266 880 elements: the second pass of the grid-stride loops of fourstep_quant / fourstep_dequant (16 384 blocks)"""
    _fourstep(3, *er.BIG_PLANE, False, estimate=False)


@pytest.mark.parametrize("N,H,W,ar", er.LL_SHAPES + [(1,) + er.BIG_PLANE + (False,)], ids=lambda v: str(v))
def test_ll(cuda, N, H, W, ar):
    from pMCTF.hip import ops
    lmin, lstep = er.lmin_lstep()
    ll, sc, mu = er.ll_inputs(N, H, W)
    what = f"ll {N}x{H}x{W} ar={int(ar)}"
    n = N * H * W
    want_hat, want_sym, want_idx = er.ll_quant(ll, sc, mu, ar)
    pd = params_dev(sc, mu, 0, False)
    sym, idx = Guarded((n,), torch.int16, OFF), Guarded((n,), torch.int16, OFF)
    with guarded_results(what + " ll_hat"):
        ll_hat = ops.ll_quant(ll.cuda(), pd, sym.buf, idx.buf, OFF, lmin, lstep, ar_order=ar)
    assert_bits(ll_hat, want_hat, what + " ll_hat")
    assert_bits(sym.t, want_sym, what + " sym")
    assert_bits(idx.t, want_idx, what + " idx")
    sym.check(what + " sym")
    idx.check(what + " idx")
    # estimate: bits of the UNROUNDED residual round(ll) - mean, per plane, into doubles that already hold something
    llr = torch.round(ll)
    v = er.ll_estimate(llr, sc, mu)
    bits = Guarded((N,), torch.float64)
    bits.t.zero_()
    ops.ll_estimate(llr.cuda(), pd, bits.t)
    got = bits.t.cpu().tolist()
    for p in range(N):
        check_total(got[p], v[p], f"{what} plane {p}")
    start = 4096.0
    bits.t.fill_(start)
    ops.ll_estimate(llr.cuda(), pd, bits.t)
    ops.ll_estimate(llr.cuda(), pd, bits.t)
    got = bits.t.cpu().tolist()
    for p in range(N):
        check_total(got[p], v[p], f"{what} plane {p}, twice onto {start}", start=start, launches=2)
    bits.check(what + " bits")


@pytest.mark.parametrize("C,H,W", er.Z_SHAPES, ids=lambda v: str(v))
def test_z(cuda, C, H, W):
    from pMCTF.hip import ops
    z, consts = er.z_inputs(C, H, W)
    what = f"z {C}x{H}x{W}"
    n = C * H * W
    want_hat, want_sym, want_idx = er.z_symbols(z)
    sym, idx = Guarded((n,), torch.int16, OFF), Guarded((n,), torch.int16, OFF)
    zd = nhwc(z)
    with guarded_results(what + " z_hat"):
        z_hat = ops.z_symbols(zd, sym.buf, idx.buf, OFF)
    assert_bits(z_hat, nhwc(want_hat), what + " z_hat")
    assert_bits(sym.t, want_sym, what + " sym")
    assert_bits(idx.t, want_idx, what + " idx")
    sym.check(what + " sym")
    idx.check(what + " idx")
    with guarded_results(what + " sym_to_nhwc"):
        back = ops.sym_to_nhwc(sym.t.clone(), H, W, C)
    assert_bits(back, nhwc(er.sym_to_nhwc(want_sym, C, H, W)), what + " sym_to_nhwc")
    clamped = nhwc(want_hat.abs() > 30000)
    assert bool(clamped.any()) or n < 56
    # numerically: int16 has no -0.0, round(-0.3) comes back as +0.0
    assert_same(torch.where(clamped, z_hat, back), z_hat, what + ": sym_to_nhwc reproduces z_hat where |z_hat| <= 30000")
    # estimate
    want_hat_e, vb = er.z_estimate(z, consts)
    v = vb.reshape(-1)
    bits = Guarded((1,), torch.float64)
    bits.t.zero_()
    with guarded_results(what + " z_estimate z_hat"):
        z_hat_e = ops.z_estimate(zd, consts.cuda(), bits.t)
    assert_bits(z_hat_e, z_hat, what + " estimate z_hat against z_symbols z_hat")
    check_total(float(bits.t.cpu()[0]), v, what)
    start = 1024.0
    bits.t.fill_(start)
    for _ in range(2):
        ops.z_estimate(zd, consts.cuda(), bits.t)
    check_total(float(bits.t.cpu()[0]), v, f"{what} twice onto {start}", start=start, launches=2)
    bits.check(what + " bits")


@pytest.mark.parametrize("H,W", er.MV_SHAPES, ids=lambda v: str(v))
def test_mv_fourpart(cuda, H, W):
    """the four steps in turn, each fed the so_far of the step before as the engine does, then mv_dequant"""
    from pMCTF.hip import ops
    lmin, lstep = er.lmin_lstep()
    y, common, sps = er.mv_inputs(H, W)
    what0 = f"mv {H}x{W}"
    n = 16 * H * W
    yd, cd = nhwc(y), nhwc(common)
    so_q, so_e, so_d = (Guarded((1, H, W, 64)) for _ in range(3))
    bits = Guarded((1,), torch.float64)
    want_so = want_d = None
    for t in range(4):
        what = f"{what0} t={t}"
        sp = sps[t]
        spd = None if sp is None else nhwc(sp)
        want_so, want_sym, want_idx = er.mv_fourpart_step(y, common, sp, want_so, t)
        want_d = er.mv_fourpart_dequant(want_sym, common, sp, want_d, t)
        sym, idx = Guarded((n,), torch.int16, OFF), Guarded((n,), torch.int16, OFF)
        ops.mv_fourpart_step(yd, cd, spd, so_q.t, sym.buf, idx.buf, OFF, t, lmin, lstep)
        assert_bits(so_q.t, nhwc(want_so), what + " so_far")
        assert_bits(sym.t, want_sym, what + " sym")
        assert_bits(idx.t, want_idx, what + " idx")
        for g, name in ((so_q, "so_far"), (sym, "sym"), (idx, "idx")):
            g.check(f"{what} {name}")
        ops.mv_fourpart_dequant(sym.t.clone(), cd, spd, so_d.t, t)
        assert_bits(so_d.t, nhwc(want_d), what + " dequant so_far")
        so_d.check(what + " dequant")
        _, v = er.mv_fourpart_step(y, common, sp, None, t, estimate=True)
        bits.t.zero_()
        ops.mv_fourpart_estimate(yd, cd, spd, so_e.t, t, bits.t)
        assert_bits(so_e.t, so_q.t, what + " estimate so_far against step so_far")
        so_e.check(what + " estimate so_far")
        check_total(float(bits.t.cpu()[0]), v, what)
        start = 512.0
        bits.t.fill_(start)
        for _ in range(2):                               # rewrites the same so_far values
            ops.mv_fourpart_estimate(yd, cd, spd, so_e.t, t, bits.t)
        check_total(float(bits.t.cpu()[0]), v, f"{what} twice onto {start}", start=start, launches=2)
        bits.check(what + " bits")
    with guarded_results(what0 + " y_hat"):
        y_hat = ops.mv_dequant(so_q.t, cd)
    assert_bits(y_hat, nhwc(er.mv_dequant(want_so, common)), what0 + " y_hat")
    unclamped = nhwc((want_so - want_d) == 0)
    assert not bool(unclamped.all())
    assert_bits(torch.where(unclamped, so_d.t, so_q.t), so_q.t, what0 + ": decoder against encoder where |q| <= 30000")


@pytest.mark.parametrize("n", er.SQDIFF_N)
def test_sqdiff_sum(cuda, n):
    from pMCTF.hip import ops
    a, b = er.sqdiff_case(n, n)
    v = er.sqdiff(a, b)
    acc = Guarded((1,), torch.float64)
    acc.t.zero_()
    ad, bd = a.cuda(), b.cuda()
    ops.sqdiff_sum(ad, bd, acc.t)
    check_total(float(acc.t.cpu()[0]), v, f"sqdiff {n}")
    start = 65536.0
    acc.t.fill_(start)
    ops.sqdiff_sum(ad, bd, acc.t)
    ops.sqdiff_sum(ad, bd, acc.t)
    check_total(float(acc.t.cpu()[0]), v, f"sqdiff {n} twice onto {start}", start=start, launches=2)
    acc.check(f"sqdiff {n}")


# ---------------------------------------------------------------------------------------------------------------------
# per-element bits: launches that leave one live element per accumulated double.  One float32 value plus zeros in
# float64 is exact: ==, no tolerance.
def _pairs():
    y, s = er.edge_grid()
    yr, sr = er.random_pairs(100000, 1)
    return torch.cat([y, yr]), torch.cat([s, sr])


def test_bits_per_element_ll(cuda):
    """ll_estimate with HW = 1: one plane per (y, sigma) pair, up to 65 535 planes a launch; y = ll_hat - mean with both
    a zero and a non-integer mean"""
    from pMCTF.hip import ops
    y, s = _pairs()
    for mean in (0.0, 0.375):
        ll_hat = (y + mean).to(torch.float32)
        mu = torch.full_like(y, mean)
        want = er.K.laplace_bits(ll_hat - mu, s).double()
        got = []
        for a in range(0, y.numel(), 65535):
            sl = slice(a, min(a + 65535, y.numel()))
            N = sl.stop - sl.start
            bits = Guarded((N,), torch.float64)
            bits.t.zero_()
            ops.ll_estimate(ll_hat[sl].reshape(N, 1, 1, 1).cuda(),
                            torch.stack([s[sl], mu[sl]], -1).reshape(N, 1, 1, 2).contiguous().cuda(), bits.t)
            got.append(bits.t.cpu())
            bits.check("ll_estimate, one element per plane")
        assert_bits(torch.cat(got), want, f"ll_estimate per element, mean {mean}")


@pytest.mark.parametrize("sub", [False, True])
def test_bits_per_element_fourstep(cuda, sub):
    """fourstep_estimate on 2x2 planes: one element of class k per plane, thousands of planes"""
    from pMCTF.hip import ops
    y, s = _pairs()
    y, s = y[:270 + 8192], s[:270 + 8192]
    N = y.numel()
    for k in range(4):
        mean = torch.full((N, 1, 1, 1), 0.25 * k)
        x = er.place_class((y.reshape(N, 1, 1, 1) + mean).to(torch.float32), k, 2, 2, float(er.GARBAGE))
        sc = er.place_class(s.reshape(N, 1, 1, 1), k, 2, 2, float(er.GARBAGE))
        mu = er.place_class(mean, k, 2, 2, float(er.GARBAGE))
        want_so, v = er.fourstep_estimate(x, sc, mu, None, k)
        so = Guarded((N, 1, 2, 2))
        bits = Guarded((N,), torch.float64)
        bits.t.zero_()
        ops.fourstep_estimate(x.cuda(), params_dev(sc, mu, k, sub), so.t, k, bits.t)
        if k == 0:
            assert_bits(so.t, want_so, "so_far")
        assert_bits(bits.t, torch.cat(v).double(), f"fourstep_estimate per element, k={k}")
        bits.check("bits")
        so.check("so_far")


def test_bits_per_element_z(cuda):
    """z_estimate with HW = 1 and C = 1: one element per launch, each into its own double"""
    from pMCTF.hip import ops
    consts = er.z_consts(64, 5)
    z = torch.cat([torch.from_numpy(er.EDGE_RES), torch.from_numpy(np.random.default_rng(3).laplace(0, 4, 100).astype(np.float32))])
    bits = Guarded((z.numel(),), torch.float64)
    bits.t.zero_()
    want = []
    for i in range(z.numel()):
        c = consts[:, i % 64:i % 64 + 1].contiguous()
        zi = z[i].reshape(1, 1, 1, 1)
        want.append(er.z_estimate(zi, c)[1].reshape(1))
        ops.z_estimate(zi.cuda(), c.cuda(), bits.t[i:i + 1])
    assert_bits(bits.t, torch.cat(want).double(), "z_estimate per element")
    bits.check("bits")


def test_bits_per_element_mv(cuda):
    """mv_fourpart_estimate on a 1x1 picture: step t codes the 16 channels of one group; fifteen of them contribute an
    exact zero (y = 0, sigma = 1e-3: p = 1), the sixteenth is the pair under test"""
    from pMCTF.hip import ops
    y, s = _pairs()
    y, s = torch.cat([y[:270:5], y[270:280]]), torch.cat([s[:270:5], s[270:280]])
    for t in range(4):
        bits = Guarded((y.numel(),), torch.float64)
        bits.t.zero_()
        want = []
        for i in range(y.numel()):
            ch = 16 * er.MV_PERMS[t].index(0) + i % 16
            yy = torch.zeros(1, 64, 1, 1)
            sc = torch.full((1, 64, 1, 1), 1e-3)
            mu = torch.zeros(1, 64, 1, 1)
            yy[0, ch], sc[0, ch] = y[i], s[i]
            common = torch.cat([torch.ones(1, 64, 1, 1), sc if t == 0 else torch.full_like(sc, float(er.GARBAGE)),
                                mu if t == 0 else torch.full_like(mu, float(er.GARBAGE))], 1)
            sp = None if t == 0 else torch.cat([sc, mu], 1)
            v = er.mv_fourpart_step(yy, common, sp, None, t, estimate=True)[1]
            assert v.numel() == 16 and int((v != 0).sum()) <= 1
            want.append(v.double().sum().reshape(1))
            so = torch.empty(1, 1, 1, 64, device="cuda")
            ops.mv_fourpart_estimate(nhwc(yy), nhwc(common), None if sp is None else nhwc(sp), so, t, bits.t[i:i + 1])
        assert_bits(bits.t, torch.cat(want), f"mv_fourpart_estimate per element, t={t}")
        bits.check("bits")
