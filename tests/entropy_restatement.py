"""Plain reference of the entropy-stage element kernels (csrc/ew_ops.hip, decode_ops.hip, estimate_ops.hip), and the
inputs the tests feed them.  No GPU import: torch-CPU float32 on NCHW tensors, one IEEE operation per written operation,
so that every expected tensor is exact and needs no tolerance.

Written from the reference's formulation, not from the kernels' index arithmetic: the four parity masks of
Oracle.masks4, Oracle.process_with_mask for residual / round / add-back, the channel groups and their masks per step as
compress_four_part_prior / decompress_four_part_prior assign them, torch.max(quant_step, 0.5) and `1. / quant_step`,
symbols.clamp(-30000, 30000).to(int16), and the symbol orders the range coder consumes (NCHW for the four-step coder and
z, [16][HW] per MV step, position-major over the planes for the sequential LL coder).  Per-element bits are
CdefK.laplace_bits / CdefK.z_bits unchanged; totals are float64 sums of those float32 values.

One thing is the kernels' contract and not the reference's: a step writes ONLY the positions of its mask.  The
reference adds a masked tensor (`so_far + x_hat`, x_hat = +-0 off the mask), which gives the same numbers and may turn
a -0.0 into +0.0; here the positions off the mask keep the bits they had (+0.0 after step 0).  The CPU tests compare
with the oracle's functions numerically (-0.0 == +0.0), the GPU tests compare with this file bit for bit.
"""
import numpy as np
import torch

from pmctf_oracle import entropy
from pmctf_oracle.kernels import CdefK
from pmctf_oracle.model import Oracle

K = CdefK()
MV_PERMS = ((0, 1, 2, 3), (3, 2, 1, 0), (2, 3, 0, 1), (1, 0, 3, 2))   # mask of channel group g in step t (four_part_prior.py)
_tables = None


def tables():
    global _tables
    if _tables is None:
        _tables = entropy.GaussianTables()
    return _tables


def lmin_lstep():
    return tables().log_scale_min, tables().log_scale_step


def rows(scales):
    """GaussianEncoder.build_indexes in PM-F32 -> int16"""
    return tables().build_indexes_cdef(scales.contiguous()).to(torch.int16)


def sym16(q):
    return q.clamp(-30000, 30000).to(torch.int16)


def _keep(mask, new, prev):
    """the step's values on its mask, what was there before elsewhere (+0.0 when nothing was)"""
    return torch.where(mask.expand_as(new) > 0, new, torch.zeros_like(new) if prev is None else prev)


def place_class(sub, k, H, W, fill):
    """parameters known only at the class-k positions (N,1,H/2,W/2) -> full size, `fill` elsewhere"""
    full = torch.full((sub.shape[0], 1, H, W), fill, dtype=sub.dtype)
    full[:, :, (k >> 1)::2, (k & 1)::2] = sub
    return full


# ------------------------------------------------------------------------------------------------ four-step coder
def fourstep_quant(x, scales, means, prev, k):
    """-> so_far (N,1,H,W), sym (N*H*W,), idx (N*H*W,)"""
    mask = Oracle.masks4(x.shape[2], x.shape[3])[k]
    _, q, x_hat, sh = Oracle.process_with_mask(x, scales, means, mask)
    return _keep(mask, x_hat, prev), sym16(q).reshape(-1), rows(sh).reshape(-1)


def fourstep_dequant(sym, means, prev, k):
    N, _, H, W = means.shape
    mask = Oracle.masks4(H, W)[k]
    q = sym.reshape(N, 1, H, W).to(torch.float32)
    return _keep(mask, (q + means) * mask, prev)


def fourstep_estimate(x, scales, means, prev, k):
    """-> so_far, [per plane: float32 bits of the class-k elements]"""
    mask = Oracle.masks4(x.shape[2], x.shape[3])[k]
    _, q, x_hat, sh = Oracle.process_with_mask(x, scales, means, mask)
    bits = K.laplace_bits(q, sh)
    live = mask[0, 0] > 0
    return _keep(mask, x_hat, prev), [bits[n, 0][live] for n in range(x.shape[0])]


# ------------------------------------------------------------------------------------------------ LL subband
def ll_quant(ll, scales, means, ar_order):
    """the LL lines of pWave.compress -> ll_hat, sym, idx"""
    y_q = torch.round(ll)
    ll_res = y_q - means
    ll_hat = (ll_res.round() + means).round()
    q = ll_res.round()
    if ar_order:
        q, scales = q.permute(2, 3, 0, 1), scales.permute(2, 3, 0, 1)
    return ll_hat, sym16(q).reshape(-1), rows(scales).reshape(-1)


def ll_estimate(ll_hat, scales, means):
    """-> [per plane: float32 bits]"""
    bits = K.laplace_bits(ll_hat - means, scales)
    return [bits[n].reshape(-1) for n in range(ll_hat.shape[0])]


# ------------------------------------------------------------------------------------------------ MV hyper latent
def z_symbols(z):
    """z (1,C,H,W) -> z_hat, sym, idx in NCHW order"""
    z_hat = torch.round(z)
    idx = entropy.BitEstimatorTables.build_indexes(z.size()).to(torch.int16)
    return z_hat, sym16(z_hat).reshape(-1), idx.reshape(-1)


def sym_to_nhwc(sym, C, H, W):
    """-> z_hat as the NCHW tensor whose NHWC form the kernel writes"""
    return sym.reshape(1, C, H, W).to(torch.float32)


def bitparm_params(consts):
    """[11][C] rows softplus(h) f1..4, b f1..4, tanh(a) f1..3 -> the (softplus(h), b, tanh(a)) tuples of CdefK.bitparm_cdf"""
    r = [c.reshape(1, -1, 1, 1) for c in consts]
    return [(r[0], r[4], r[8]), (r[1], r[5], r[9]), (r[2], r[6], r[10]), (r[3], r[7], None)]


def z_estimate(z, consts):
    """-> z_hat, float32 bits (1,C,H,W)"""
    z_hat = torch.round(z)
    return z_hat, K.z_bits(z_hat, bitparm_params(consts))


# ------------------------------------------------------------------------------------------------ MV four-part coder
def _mv_step_params(common, sp, t):
    quant_step, scales, means = common.chunk(3, 1)
    quant_step = torch.max(quant_step, torch.ones_like(quant_step) * 0.5)
    if t == 0:
        return quant_step, scales.chunk(4, 1), means.chunk(4, 1)
    ch = sp.chunk(8, 1)
    return quant_step, ch[:4], ch[4:]


def mv_fourpart_step(y, common, sp, prev, t, estimate=False):
    """y (1,64,H,W), common (1,192,H,W), sp (1,128,H,W) or None -> so_far, sym [16][HW], idx [16][HW];
    estimate=True: -> so_far, float32 bits of the live elements"""
    quant_step, sc, mu = _mv_step_params(common, sp, t)
    q_enc = 1. / quant_step
    m = Oracle.masks4(y.shape[2], y.shape[3])
    ys = (y * q_enc).chunk(4, 1)
    qs, hs, shs, ms = [], [], [], []
    for g in range(4):
        mask = m[MV_PERMS[t][g]]
        _, q, h, sh = Oracle.process_with_mask(ys[g], sc[g], mu[g], mask)
        qs.append(q); hs.append(h); shs.append(sh); ms.append(mask.expand_as(q))
    mask64 = torch.cat(ms, 1)
    so_far = _keep(mask64, torch.cat(hs, 1), prev)
    if estimate:
        bits = K.laplace_bits(torch.cat(qs, 1), torch.cat(shs, 1))
        return so_far, bits[mask64 > 0]
    return so_far, sym16(qs[0] + qs[1] + qs[2] + qs[3]).reshape(-1), rows(shs[0] + shs[1] + shs[2] + shs[3]).reshape(-1)


def mv_dequant(so_far, common):
    quant_step = common.chunk(3, 1)[0]
    quant_step = torch.max(quant_step, torch.ones_like(quant_step) * 0.5)
    return so_far * quant_step


def mv_fourpart_dequant(sym, common, sp, prev, t):
    _, _, H, W = common.shape
    _, _, mu = _mv_step_params(common, sp, t)
    m = Oracle.masks4(H, W)
    y_q_r = sym.reshape(1, 16, H, W).to(torch.float32)
    cur = torch.cat([(y_q_r + mu[g]) * m[MV_PERMS[t][g]] for g in range(4)], 1)
    mask64 = torch.cat([m[MV_PERMS[t][g]].expand(1, 16, H, W) for g in range(4)], 1)
    return _keep(mask64, cur, prev)


def sqdiff(a, b):
    """-> float32 squared differences"""
    d = a - b
    return (d * d).reshape(-1)


# ------------------------------------------------------------------------------------------------ totals
def total64(v):
    return float(v.double().sum())


def summation_bound(v):
    """worst-case error of ANY order of float64 additions of the n values v: n * 2^-53 * sum |v|"""
    return v.numel() * 2.0 ** -53 * float(v.double().abs().sum())


def half_smallest(v):
    nz = v[v != 0]
    return float("inf") if nz.numel() == 0 else 0.5 * float(nz.abs().min())


# ------------------------------------------------------------------------------------------------ inputs
F32 = np.float32
EDGE_SCALES = np.array([0, -1, 1e-6, 1e-5, np.nextafter(F32(1e-5), F32(1)), 1e-3, 0.11, 0.5, 1, 7.3, 64, 1e3, 1e10, 3e10,
                        np.inf], F32)
# no mean of -0.0: with a residual in [-0.5, -0.0) the encoder's so_far is -0.0 + -0.0 = -0.0 and the decoder's
# (float)0 + -0.0 = +0.0, in the reference as in the kernels; equal numbers, and no network output is an exact -0.0
EDGE_MEANS = np.array([0.25, -3.75, 17.125, 0.5, -0.625, -1.5, 0.0, 2.3], F32)
GARBAGE = F32(1e30)
# estimate edge grid: y x sigma.  +-0 (p = 1 under a small sigma: exact zeros), the ties +-0.5 where one of the two cdf
# arguments is 0, one ulp either side of them (the only y whose bits tell a lower sigma clamp of 1e-5 from a smaller one:
# exp(-ulp / sigma) is neither 0 nor 1 there), +-1.5 / +-2.5 with a neighbour each, and four symbols about the int16 clamp
_U = lambda v, d: np.nextafter(np.float32(v), np.float32(d * np.inf))
EDGE_Y = np.array([0.0, -0.0, _U(0.5, -1), 0.5, _U(0.5, 1), _U(-0.5, -1), -0.5, _U(-0.5, 1), _U(1.5, -1), 1.5, _U(1.5, 1),
                   -1.5, 2.5, _U(-2.5, 1), 30000, -30001, 40000, -29999], np.float32)


def _edge_residuals():
    r = []
    for t in (0.5, 1.5, 2.5):
        for s in (1, -1):
            v = F32(s * t)
            r += [np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf))]
    r += [F32(0.0), F32(-0.0)]
    for big in (29999, 30000, 30001, 40000):
        r += [F32(big), F32(-big)]
    return np.array(r, F32)


EDGE_RES = _edge_residuals()       # 28 residuals x - mean: ties and one ulp either side, +-0, the int16 clamp


def edge_grid():
    """(y, sigma) of the 18 x 15 grid, flat"""
    y, s = np.meshgrid(EDGE_Y, EDGE_SCALES, indexing="ij")
    return torch.from_numpy(y.reshape(-1).copy()), torch.from_numpy(s.reshape(-1).copy())


def random_pairs(n, seed):
    """residuals Laplace(0, 2) scaled by sigma's magnitude, sigma log-uniform in [1e-6, 1e3]"""
    r = np.random.default_rng(seed)
    s = np.exp(r.uniform(np.log(1e-6), np.log(1e3), n)).astype(F32)
    y = (r.laplace(0, 2, n) * np.where(r.random(n) < 0.5, 1.0, s)).astype(F32)
    return torch.from_numpy(y), torch.from_numpy(s)


def element_inputs(n, seed, stride, edge_scales=True, smin=0.05, smax=30.0):
    """n elements (x, scale, mean): Laplace(0, 2) residuals about N(0, 3) means with log-uniform scales, and at every
    `stride`-th element one combination of EDGE_RES x EDGE_MEANS x EDGE_SCALES (x is the float32 sum mean + residual, so
    that x - mean lands on the residual or next to it); the CPU tests check that every parity class of a plane meets every
    residual and every scale"""
    r = np.random.default_rng(seed)
    mean = (r.standard_normal(n) * 3).astype(F32)
    x = (mean + r.laplace(0, 2, n).astype(F32)).astype(F32)
    scale = np.exp(r.uniform(np.log(smin), np.log(smax), n)).astype(F32)
    pos = np.arange(0, n, stride)
    e = np.arange(pos.size)
    mean[pos] = EDGE_MEANS[(e // 56) % EDGE_MEANS.size]
    res = EDGE_RES[(e + e // 2) % EDGE_RES.size]                  # e + e/2: both parities of e meet every residual
    x[pos] = np.where(mean[pos] == 0, res, (mean[pos] + res).astype(F32))      # about a zero mean: the residual itself, -0.0 too
    if edge_scales:
        scale[pos] = EDGE_SCALES[e % EDGE_SCALES.size]
    return torch.from_numpy(x), torch.from_numpy(scale), torch.from_numpy(mean)


def fourstep_case(N, H, W, seed, edge_scales=True, smin=0.05, smax=30.0):
    """x (N,1,H,W) and, per step k, (x_k, scales_k, means_k): the step's own parameters on its mask and GARBAGE off it, in
    x as well, so that a kernel that reads a position of another class shows"""
    n = N * H * W
    stride = 1 if n <= 65536 else 3
    steps = []
    masks = Oracle.masks4(H, W)
    for k in range(4):
        xk, sc, mu = element_inputs(n, seed + 1 + k, stride, edge_scales, smin, smax)
        on = masks[k].expand(N, 1, H, W) > 0
        g = torch.full((N, 1, H, W), float(GARBAGE))
        steps.append((torch.where(on, xk.reshape(N, 1, H, W), g), torch.where(on, sc.reshape(N, 1, H, W), g),
                      torch.where(on, mu.reshape(N, 1, H, W), g)))
    return steps


def ll_case(N, H, W, seed, edge_scales=True, smin=0.05, smax=30.0):
    n = N * H * W
    ll, sc, mu = element_inputs(n, seed, 1 if n <= 4096 else 3, edge_scales, smin, smax)
    return ll.reshape(N, 1, H, W), sc.reshape(N, 1, H, W), mu.reshape(N, 1, H, W)


def z_case(C, H, W, seed):
    """z with ties, +-0 and values past the int16 clamp; consts of a plausible factorized prior"""
    r = np.random.default_rng(seed)
    n = C * H * W
    z = (r.laplace(0, 3, n)).astype(F32)
    pos = np.arange(0, n, 2)
    z[pos] = EDGE_RES[np.arange(pos.size) % EDGE_RES.size]
    return torch.from_numpy(z).reshape(1, C, H, W)


def z_consts(C, seed):
    r = np.random.default_rng(seed)
    h = torch.from_numpy(r.uniform(-1.0, 2.0, (4, C)).astype(F32))
    b = torch.from_numpy(r.uniform(-1.0, 1.0, (4, C)).astype(F32))
    a = torch.from_numpy(r.uniform(-1.0, 1.0, (3, C)).astype(F32))
    return torch.cat([torch.nn.functional.softplus(h), b, torch.tanh(a)], 0).contiguous()


MV_QSTEPS = np.array([0.0, 0.25, np.nextafter(F32(0.5), F32(0)), 0.5, np.nextafter(F32(0.5), F32(1)), 0.75, 1.0, 1.7, 3.0],
                     F32)


def mv_case(H, W, seed, edge_scales=True):
    """y (1,64,H,W), common (1,192,H,W) = (quant_step | scales | means), sp[t] (1,128,H,W) for t = 1..3.  quant_step runs
    below, at and above 0.5; y is (mean + residual) * max(quant_step, 0.5), so that y / quant_step lands on or next to the
    edge residuals; every parameter is GARBAGE wherever its step does not code the element."""
    n = 64 * H * W
    r = np.random.default_rng(seed)
    qs = MV_QSTEPS[r.integers(0, MV_QSTEPS.size, n)]
    m = Oracle.masks4(H, W)
    y = np.zeros(n, F32)
    par = []
    for t in range(4):
        xk, sc, mu = element_inputs(n, seed + 10 + t, 1 if n <= 4096 else 3, edge_scales)
        on = torch.cat([m[MV_PERMS[t][g]].expand(1, 16, H, W) for g in range(4)], 1).reshape(-1) > 0
        y = np.where(on.numpy(), (xk.numpy() * np.maximum(qs, F32(0.5))).astype(F32), y)
        g = torch.full((n,), float(GARBAGE))
        par.append((torch.where(on, sc, g).reshape(1, 64, H, W), torch.where(on, mu, g).reshape(1, 64, H, W)))
    qs = torch.from_numpy(qs).reshape(1, 64, H, W)
    common = torch.cat([qs, par[0][0], par[0][1]], 1)
    sps = [None] + [torch.cat([par[t][0], par[t][1]], 1) for t in (1, 2, 3)]
    return torch.from_numpy(y).reshape(1, 64, H, W), common, sps


# shapes of the issue
FOURSTEP_SHAPES = [(1, 2, 2, False), (3, 5, 7, False), (2, 37, 53, False), (2, 36, 60, False), (2, 36, 60, True),
                   (6, 68, 120, False), (6, 68, 120, True), (1, 2, 2, True)]           # (N, H, W, params_sub)
BIG_PLANE = (1088, 1920)
LL_SHAPES = [(n, h, w, ar) for n in (1, 2, 3) for (h, w) in ((1, 1), (17, 30), (68, 120)) for ar in (False, True)]
Z_SHAPES = [(64, 1, 1), (64, 4, 7), (64, 17, 30), (24, 9, 13), (3, 1, 5)]              # (C, H, W)
MV_SHAPES = [(2, 2), (4, 6), (18, 30), (68, 120)]
SQDIFF_N = [1, 63, 65, 255, 257, 1000, 65537, 2 ** 20 + 1, 2 ** 21 + 3]


def sqdiff_case(n, seed):
    """differences of magnitude 1..3 (squares 1..9) and exact zeros: the smallest nonzero term stays far above the
    summation bound of the largest n (n^2 * 2^-53 * mean = 5e-4 * mean at n = 2^21 + 3)"""
    r = np.random.default_rng(seed)
    a = (r.standard_normal(n) * 40 + 128).astype(F32)
    d = (r.uniform(1.0, 3.0, n) * np.where(r.random(n) < 0.5, -1.0, 1.0)).astype(F32)
    b = (a + d).astype(F32)
    b[:: 7] = a[:: 7]                                   # exact zeros among the terms
    return torch.from_numpy(a), torch.from_numpy(b)


def fourstep_inputs(N, H, W):
    if (H, W) == BIG_PLANE:      # moderate scales: the smallest contribution stays far above the bound of 522 240 values
        return fourstep_case(N, H, W, 7, edge_scales=False, smin=0.5)
    return fourstep_case(N, H, W, 100 + H)


def ll_inputs(N, H, W):
    if (H, W) == BIG_PLANE:
        return ll_case(N, H, W, 9, edge_scales=False, smin=0.5)
    return ll_case(N, H, W, 200 + H)


def z_inputs(C, H, W):
    return z_case(C, H, W, 300 + H), z_consts(C, 5)


def mv_inputs(H, W):
    return mv_case(H, W, 400 + H, edge_scales=H * W <= 1000)


def totals_cases():
    """name -> list of float32 value vectors, one per accumulated double: every total the GPU file checks against
    summation_bound.  The CPU file asserts bound < half_smallest for each; inputs whose smallest contribution would be too
    small for their size (scales that push p + 1e-5 next to 1 on a full-size plane) are kept out by smin."""
    out = {}
    for (N, H, W) in sorted(set(s[:3] for s in FOURSTEP_SHAPES)) + [(1,) + BIG_PLANE]:
        steps = fourstep_inputs(N, H, W)
        for k in range(4):
            out[f"fourstep {N}x{H}x{W} k={k}"] = fourstep_estimate(*steps[k], None, k)[1]
    for (N, h, w) in sorted(set(s[:3] for s in LL_SHAPES)) + [(1,) + BIG_PLANE]:
        ll, sc, mu = ll_inputs(N, h, w)
        out[f"ll {N}x{h}x{w}"] = ll_estimate(torch.round(ll), sc, mu)
    for (C, h, w) in Z_SHAPES:
        out[f"z {C}x{h}x{w}"] = [z_estimate(*z_inputs(C, h, w))[1].reshape(-1)]
    for (h, w) in MV_SHAPES:
        y, common, sps = mv_inputs(h, w)
        for t in range(4):
            out[f"mv {h}x{w} t={t}"] = [mv_fourpart_step(y, common, sps[t], None, t, estimate=True)[1]]
    for n in SQDIFF_N:
        out[f"sqdiff {n}"] = [sqdiff(*sqdiff_case(n, n))]
    return out
