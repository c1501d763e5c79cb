"""The arithmetic of csrc/conv_split.hip (the bf16-split 3x3 convolution) restated from its header comment, in numpy and
float64, without the product and without a GPU.

    operands   x = x0 + x1 + x2 + ...: plane k is the round-to-nearest-even bf16 of what planes 0..k-1 leave, the
               subtraction in f32 (exact): split4<NS> for the activations, the loop of pmctf_conv3x3_split_pack_weights
               for the weights
    products   the NS(NS+1)/2 largest partial products, TERMS[NS] = (plane of the weights, plane of the activations),
               term_a / term_b of the kernel
    sum        f32, starting from the bias; taps outside the picture contribute zero
    epilogue   conv_mfma.hip's: max(v, 0) or (v > 0 ? v : v * slope), then + res1, then + res2, one f32 rounding each

conv_ref returns the sum S of the kept products in float64 (every product of two bf16 values is exact there) and
A = |b| + sum |w_i| |x_j| over the same products, the quantity every bound on the f32 accumulation is stated in.
Tensors are NHWC (N, H, W, C), weights OIHW (Cout, Cin, 3, 3), as the product's ops.Conv2d takes them.

Two seeded input generators: exact_case makes data on which S is the same in every order of summation, so that the
kernel's f32 result must equal S bit for bit; dense_case is ordinary data, for the bounds.  MUTANTS are restatements that
are wrong on purpose: tests/test_split_restatement_cpu.py checks that each of them changes the expected output, i.e.
that a kernel with that error could not pass the bit-for-bit test."""
import numpy as np

TERMS = {3: [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)], 2: [(1, 0), (0, 1), (0, 0)], 1: [(0, 0)]}
# |S - conv64| <= EPS[ns] * sum |x||w|: with |x - x0| <= 2^-9 |x| per plane (so plane k is at most 2^-9k of the value,
# and what NS planes leave at most 2^-9NS) the products that TERMS[ns] drops add up to
#   ns = 1: w rx + rw x + rw rx                      2 * 2^-9 + 2^-18
#   ns = 2: w1 x1 + w rx + rw x + ...                3 * 2^-18 + 2^-26
#   ns = 3: w1 x2 + w2 x1 + w rx + rw x + ...        4 * 2^-27 + ... < 2^-24
# 2^-9 |x| is half an ulp of bf16 for a value at the top of its binade; just above a power of two half an ulp is 2^-8 |x|,
# so a single product can exceed these figures (by up to 2x for ns = 1, 4x for ns = 2 and 3).  They are the figures the
# header's "~2^-8 / ~2^-16 / ~2^-22 per product" is held to over the 144..1008 products of an output of dense_case, where
# the roundings of the products are independent; the CPU test asserts that they hold there.
EPS = {1: 2.0 ** -8 + 2.0 ** -18, 2: 3 * 2.0 ** -18 + 2.0 ** -26, 3: 2.0 ** -24}
Q = 2.0 ** -18                                  # every kept product of exact_case is a multiple of it


def bf16_rne(x):
    """float32 -> the nearest bf16 (ties to even), returned as float32.  Bit level: add 0x7fff plus the lowest kept bit,
    drop the low half; NaN stays NaN."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = np.where(nan, (u | 0x400000) & 0xFFFF0000, r)
    return r.astype(np.uint32).view(np.float32)


def bf16_trunc(x):
    """the wrong split: the low half of the word dropped (round toward zero)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return (u & np.uint32(0xFFFF0000)).view(np.float32)


def planes(x, ns, cast=bf16_rne):
    """[x0, x1, ...]: x0 = bf16(x), x1 = bf16(x - x0), ... in float32"""
    r = np.asarray(x, dtype=np.float32)
    out = []
    for _ in range(ns):
        h = cast(r)
        out.append(h)
        r = (r - h).astype(np.float32)
    return out


def windows(x, stride=1, pad=(1, 1), out_hw=None):
    """yields (tap, v): v[n, oy, ox, :] = x[n, stride*oy - pad[0] + ky, stride*ox - pad[1] + kx, :], zero outside; tap =
    3 ky + kx"""
    N, H, W, C = x.shape
    Ho, Wo = out_hw if out_hw is not None else ((H + 2 * pad[0] - 3) // stride + 1, (W + 2 * pad[1] - 3) // stride + 1)
    bot = max(0, stride * (Ho - 1) - pad[0] + 2 - (H - 1))
    right = max(0, stride * (Wo - 1) - pad[1] + 2 - (W - 1))
    xp = np.pad(x, ((0, 0), (pad[0], bot), (pad[1], right), (0, 0)))
    for ky in range(3):
        for kx in range(3):
            yield 3 * ky + kx, xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride, :]


def conv_terms(xs, ws, b, terms, stride=1, pad=(1, 1), out_hw=None):
    """(S, A) in float64 for planes xs (NHWC) and ws (OIHW): S = b + sum over taps, channels and terms (i, j) of
    ws[i] * xs[j], A the same with absolute values"""
    bias = np.asarray(b, dtype=np.float64)
    cout, cin = ws[0].shape[:2]
    # [tap][cin] x [cout] matrices, and per activation plane the windows of every output side by side: [pixel] x [tap][cin]
    wm = [np.asarray(v, dtype=np.float64).reshape(cout, cin, 9).transpose(2, 1, 0).reshape(9 * cin, cout) for v in ws]
    S = A = None
    for j in sorted({j for _, j in terms} | {0}):
        win = [v for _, v in windows(np.asarray(xs[j], dtype=np.float64), stride, pad, out_hw)]
        vm = np.stack(win, axis=3).reshape(-1, 9 * cin)
        if S is None:
            S = np.zeros(win[0].shape[:3] + (cout,)) + bias
            A = np.zeros_like(S) + np.abs(bias)
        for i in (i for i, jj in terms if jj == j):
            S += (vm @ wm[i]).reshape(S.shape)
            A += (np.abs(vm) @ np.abs(wm[i])).reshape(S.shape)
    return S, A


def conv_ref(x, w, b, ns, stride=1, pad=(1, 1), out_hw=None, terms=None, cast=bf16_rne):
    """what the kernel computes before its epilogue, up to the rounding of its f32 additions: (S, A) in float64"""
    return conv_terms(planes(x, ns, cast), planes(w, ns, cast), b, TERMS[ns] if terms is None else terms, stride, pad,
                      out_hw)


def conv64(x, w, b, stride=1, pad=(1, 1), out_hw=None):
    """the convolution the split approximates, on the unsplit f32 operands in float64: (sum, sum |x||w| without the bias)"""
    S, A = conv_terms([x], [w], b, [(0, 0)], stride, pad, out_hw)
    return S, A - np.abs(np.asarray(b, dtype=np.float64))


def accumulation_bound(A, cin, ns):
    """T = n 2^-23 A, n = 9 Cin len(TERMS[ns]) + 1: Higham's bound for n f32 additions in any order (gamma_n <= n u to
    first order), with the unit round-off 2^-23 of an adder that truncates"""
    return (9 * cin * len(TERMS[ns]) + 1) * 2.0 ** -23 * A


def epilogue(v, act=0, slope=0.0, res=()):
    """f32, one rounding per written operation; act 0 none, 1 relu, 2 leaky"""
    v = np.asarray(v, dtype=np.float32)
    if act == 1:
        v = np.maximum(v, np.float32(0))
    elif act == 2:
        v = np.where(v > 0, v, v * np.float32(slope)).astype(np.float32)
    for r in res:
        v = (v + np.asarray(r, dtype=np.float32)).astype(np.float32)
    return v


def sequential_f32(x, w, b, ns, stride=1, pad=(1, 1), out_hw=None, reverse=False):
    """The kept products of a ONE-HOT x (at most one non-zero channel per pixel, as exact_case makes) added one at a time
    in float32, from the bias: tap by tap, the terms in written order, or all of it backwards.  The channels that hold
    zero would add an exact zero each and are left out."""
    assert (np.count_nonzero(x, axis=-1) <= 1).all()
    g = dict(stride=stride, pad=pad, out_hw=out_hw)
    ci = np.abs(x).argmax(axis=-1)[..., None]                                # the live channel of every pixel
    live = [v[..., 0].astype(np.int64) for _, v in windows(ci.astype(np.float64), **g)]
    vals = [[v for _, v in windows(np.take_along_axis(p, ci, -1), **g)] for p in planes(x, ns)]   # [plane][tap]: (N, Ho, Wo, 1)
    ws = [p.reshape(p.shape[0], p.shape[1], 9) for p in planes(w, ns)]
    steps = [(tap, i, j) for tap in range(9) for i, j in TERMS[ns]]
    acc = np.zeros(live[0].shape + (w.shape[0],), np.float32) + np.asarray(b, np.float32)
    for tap, i, j in (reversed(steps) if reverse else steps):
        prod = (vals[j][tap] * ws[i][:, :, tap].T[live[tap]]).astype(np.float32)      # bf16 x bf16 is exact in f32
        acc = (acc + prod).astype(np.float32)
    return acc


# --------------------------------------------------------------------------------------------------------- inputs
def exact_case(N, Cin, Cout, H, W, seed):
    """(x, w, b): every pixel of x has exactly one non-zero channel; every non-zero activation and every weight is
    s (1 + 2^-9 + t 2^-18) with independent signs s, t; the bias a multiple of 2^-18 with |b| <= 2.  The planes of such a
    value are s, s 2^-9, s t 2^-18 (2^-9 - 2^-18 is a tie that round-to-nearest-even sends UP to 2^-9 and truncation
    down), every kept product is a multiple of 2^-18, and A <= 2 + 9 (1 + 2^-8 + 3 2^-18) < 11.04: every partial sum in
    every order fits in 22 bits, so an f32 accumulation is exact whatever its order."""
    r = np.random.default_rng(seed)

    def values(shape):
        s = r.integers(0, 2, shape) * 2.0 - 1.0
        t = r.integers(0, 2, shape) * 2.0 - 1.0
        return (s * (1 + 2.0 ** -9 + t * 2.0 ** -18)).astype(np.float32)

    x = np.zeros((N, H, W, Cin), np.float32)
    ch = r.integers(0, Cin, (N, H, W, 1))
    np.put_along_axis(x, ch, values((N, H, W, 1)), -1)
    w = values((Cout, Cin, 3, 3))
    b = (r.integers(-2 ** 19, 2 ** 19 + 1, Cout) * Q).astype(np.float32)
    return x, w, b


def dense_case(N, Cin, Cout, H, W, seed):
    """(x, w, b): x standard normal times a power of two per channel from 2^-6 .. 2^6, w normal x 0.05, b normal"""
    r = np.random.default_rng(seed)
    x = (r.standard_normal((N, H, W, Cin)) * 2.0 ** r.integers(-6, 7, Cin)).astype(np.float32)
    w = (r.standard_normal((Cout, Cin, 3, 3)) * 0.05).astype(np.float32)
    b = r.standard_normal(Cout).astype(np.float32)
    return x, w, b


def residuals(shape, seed):
    """two ordinary f32 normal tensors of the output's shape"""
    r = np.random.default_rng(seed)
    return r.standard_normal(shape).astype(np.float32), r.standard_normal(shape).astype(np.float32)


# -------------------------------------------------------------------------------------------------------- mutants
NEGATED = (5, 3, 1, 2)                          # (cout, cin, ky, kx) of the weight the last mutant negates


def _drop(t):
    return lambda x, w, b, ns, **g: conv_ref(x, w, b, ns, terms=TERMS[ns][:t] + TERMS[ns][t + 1:], **g)[0]


def _truncating(x, w, b, ns, **g):
    return conv_ref(x, w, b, ns, cast=bf16_trunc, **g)[0]


def _shifted(x, w, b, ns, **g):
    return conv_ref(np.roll(x, 1, axis=2), w, b, ns, **g)[0]


def _negated(x, w, b, ns, **g):
    w = w.copy()
    w[NEGATED] = -w[NEGATED]
    return conv_ref(x, w, b, ns, **g)[0]


def mutants(ns):
    """{name: f(x, w, b, ns, **geometry) -> S}: each single term of TERMS[ns] dropped, a truncating split, the input
    shifted by one column, one weight negated"""
    m = {f"drop {TERMS[ns][t]}": _drop(t) for t in range(len(TERMS[ns]))}
    m.update({"truncate": _truncating, "shift": _shifted, "negate": _negated})
    return m


MUTANTS = {ns: mutants(ns) for ns in (1, 2, 3)}
