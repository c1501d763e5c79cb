"""Cases for the direct tests of the sequential LL decode (pmctf_ll_ar_decode_rules_f32, decode_ops.hip) and the code
that runs them.  Used by tests/test_gpu_ll_decode.py in process (default kernel choice) and as a child process for the
variants that the environment switches PMCTF_LL_AR_V1 / _V2 / _ROW1 select (they are read once per process):

    python ll_decode_helper.py <variant> cases.npz out.npz

Building a case is CPU only (oracle + the product's host range coder): weights, an LL plane, a rule triple, the
expected ll_hat from the oracle's one-shot network under those rules, and a stream with symbols before and after the LL.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "learned-pmctf_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

CODER = "lp_coder"
LL = f"{CODER}.context_fusion.3.ll"
NF = 128
CHAIN, BLOCKS = 0, 1                            # PMCTF_SUM_CHAIN / PMCTF_SUM_BLOCKS; B >= 16: reduce-B of a 1x1 layer
VARIANTS = {"default": None, "v2": "PMCTF_LL_AR_V2", "row1": "PMCTF_LL_AR_ROW1", "v1": "PMCTF_LL_AR_V1"}
SWITCHES = tuple(v for v in VARIANTS.values() if v)


# ---------------------------------------------------------------------------------------------------- kernel choice
def lds_bytes(N, W, cols):
    """the LDS estimate of pmctf_ll_ar_decode_rules_f32 (decode_ops.hip), and the two-half row kernel's (+ N*4*NF floats)"""
    smem = (256 * cols + 512) * 4 + (2 * N * 5 * NF + 5 * N * NF + 5 * N * 4 * NF + 7 * NF + 2 * NF + 2 + 2 * N
                                     + N * 2 * (W + 2)) * 4 + 64
    return smem, smem + N * 4 * NF * 4


def kernel_for(variant, rule3, N, W, cols):
    """the kernel pmctf_ll_ar_decode_rules_f32 sends a case to under a variant (mirror of its selection)"""
    smem, smem2 = lds_bytes(N, W, cols)
    lim = 150 * 1024
    if variant not in ("v1", "v2") and rule3 == BLOCKS and N <= 2 and smem <= lim:
        return f"row<{N}>" if (variant == "row1" or smem2 > lim) else f"row2<{N}>"
    if variant != "v1" and N <= 2 and smem <= lim:
        return f"stream<{N}>"
    return f"v1 N={N}"


# ---------------------------------------------------------------------------------------------------- running
def run_case(L, lib, w_dev, words, n_words, x0, pos0, tabs, lmin, lstep, N, H, W, rules):
    """one call of pmctf_ll_ar_decode_rules_f32 on the current stream; returns (ll_out [N][H][W], state [3])"""
    import torch
    dev = w_dev.device
    wd = torch.from_numpy(np.ascontiguousarray(words[:max(n_words, 1)])).to(dev)   # n_words of them are valid
    ll = torch.full((N, H, W), float("nan"), dtype=torch.float32, device=dev)          # every position must be written
    scratch = torch.zeros(L.pmctf_ll_ar_scratch_floats(N, H, W), dtype=torch.float32, device=dev)
    state = torch.full((3,), -1, dtype=torch.int64, device=dev)
    cdf, sizes, offs = tabs
    vp = lambda t: C.c_void_p(t.data_ptr())
    st = torch.cuda.current_stream(dev)
    lib.check(L.pmctf_ll_ar_decode_rules_f32(vp(w_dev), vp(wd), int(n_words), C.c_uint64(int(x0)), int(pos0), vp(cdf),
                                             vp(sizes), vp(offs), cdf.shape[1], float(lmin), float(lstep), vp(ll),
                                             vp(scratch), N, H, W, vp(state), int(rules[0]), int(rules[1]),
                                             int(rules[2]), C.c_void_p(st.cuda_stream)), "ll_ar_decode_rules")
    st.synchronize()
    return ll.cpu().numpy(), state.cpu().numpy().view(np.uint64)


def run_all(cases_npz, out_npz=None):
    """decode every case of cases_npz (what make_cases wrote) on cuda:0; returns {case: (ll, state)}"""
    import torch
    from pMCTF.hip import lib
    L = lib.hip()
    d = np.load(cases_npz)
    dev = torch.device("cuda:0")
    tabs = tuple(torch.from_numpy(np.ascontiguousarray(d[k], dtype=np.int32)).to(dev) for k in ("cdf", "sizes", "offsets"))
    lmin, lstep = float(d["lmin"]), float(d["lstep"])
    wdev = {}
    out = {}
    for i in range(int(d["n_cases"])):
        m = d[f"c{i}_meta"]
        N, H, W, r3, rh, ro, pos0, n_words, wi = (int(v) for v in m[:9])
        x0 = int(d[f"c{i}_x0"][0])
        if wi not in wdev:
            wdev[wi] = torch.from_numpy(d[f"w{wi}"]).to(dev)
        out[i] = run_case(L, lib, wdev[wi], d[f"c{i}_words"], n_words, x0, pos0, tabs, lmin, lstep, N, H, W,
                          (r3, rh, ro))
    if out_npz is not None:
        np.savez(out_npz, **{f"c{i}_ll": v[0] for i, v in out.items()}, **{f"c{i}_state": v[1] for i, v in out.items()})
    return out


# ---------------------------------------------------------------------------------------------------- building cases
def forced_rules(rule3, rule_head, rule_out):
    """a replacement for Oracle.sum_rule: the 3x3 rule for the masked layers, the head rule for convs.0/1, the out
    rule for convs.2 (only the LL network is evaluated with it)"""
    def sum_rule(p, x, w, groups=1, stride=1):
        if p.endswith(".convs.2"):
            return rule_out
        if p.endswith(".convs.0") or p.endswith(".convs.1"):
            return rule_head
        return rule3
    return sum_rule


def pack_weights(sd):
    """pmctf_ll_ar_pack_weights of the (masked) LL network, as HipEngine._ll_weights does"""
    from pMCTF.hip import lib
    g = lambda k: np.ascontiguousarray(sd[LL + k].numpy(), dtype=np.float32)
    names = [".residualBlocks.0.conv1", ".residualBlocks.0.conv2", ".residualBlocks.1.conv1", ".residualBlocks.1.conv2",
             ".maskedConv2"]
    wb = [g(n + ".weight") for n in names]
    bb = [g(n + ".bias") for n in names]
    wb_p = (C.c_void_p * 5)(*[a.ctypes.data for a in wb])
    bb_p = (C.c_void_p * 5)(*[a.ctypes.data for a in bb])
    L = lib.hip()
    out = np.empty(L.pmctf_ll_ar_packed_size(), np.float32)
    keep = [g(".maskedConv1.weight"), g(".maskedConv1.bias"), g(".convs.0.weight"), g(".convs.0.bias"),
            g(".convs.1.weight"), g(".convs.1.bias"), g(".convs.2.weight"), g(".convs.2.bias")]
    lib.check(L.pmctf_ll_ar_pack_weights(keep[0].ctypes.data, keep[1].ctypes.data, C.addressof(wb_p), C.addressof(bb_p),
                                         keep[2].ctypes.data, keep[3].ctypes.data, keep[4].ctypes.data,
                                         keep[5].ctypes.data, keep[6].ctypes.data, keep[7].ctypes.data,
                                         out.ctypes.data), "ll_ar_pack_weights")
    return out


@functools.lru_cache(maxsize=None)
def synth_sd(seed):
    import pmctf_synth
    from pMCTF.models.video.pMCTF_L import pMCTF
    return pmctf_synth.synth_state_dict(pMCTF(num_me_stages=1).state_dict(), seed=seed)


def weight_sets(names=None):
    """name -> Oracle.  Seeds 0 and 1, and seed 0 with the convs.2 bias shifted: scale far down (most positions at row
    0, the smallest support: almost every residual escapes), far up (row 255), mean +-2000 (escapes of 3 and 4 bypass
    nibbles of both signs)."""
    import torch
    from pmctf_oracle.model import Oracle
    sets = {}
    base = synth_sd(0)
    for name, seed, shift in (("s0", 0, None), ("s1", 1, None), ("lo", 0, (-2.995, 0.0)), ("hi", 0, (100.0, 0.0)),
                              ("m+", 0, (0.0, 2000.0)), ("m-", 0, (0.0, -2000.0))):
        if names is not None and name not in names:
            continue
        sd = base if seed == 0 else synth_sd(seed)
        if shift is not None:
            sd = dict(sd)
            sd[LL + ".convs.2.bias"] = sd[LL + ".convs.2.bias"] + torch.tensor(shift, dtype=torch.float32)
        sets[name] = Oracle(sd, 1, "cdef")
    return sets


MASKED = [".maskedConv1", ".residualBlocks.0.conv1", ".residualBlocks.0.conv2", ".residualBlocks.1.conv1",
          ".residualBlocks.1.conv2", ".maskedConv2"]
TYPE_B = MASKED[1:]


def big_bias_set(seed=5):
    """seed 0 with biases of O(1) (std 1) in the six masked 3x3 layers instead of the synthetic ~0.01, and the mean's
    head weights x100, so that a bias counted twice, or not at all, moves the parameters far past rounding"""
    import torch
    from pmctf_oracle.model import Oracle
    sd = dict(synth_sd(0))
    g = torch.Generator().manual_seed(seed)
    for n in MASKED:
        sd[LL + n + ".bias"] = torch.randn(sd[LL + n + ".bias"].shape, generator=g)
    w = sd[LL + ".convs.2.weight"].clone()
    w[1] *= 100.0                                  # means of O(10): a shifted activation moves rint(symbol + mean)
    sd[LL + ".convs.2.weight"] = w
    return Oracle(sd, 1, "cdef")


def with_doubled_type_b_bias(orc):
    """orc with the bias of the five type-B layers counted twice: what a kernel that starts the first chunk's sum of
    rule "blocks" from the bias (and then adds the bias) computes, up to rounding"""
    o = Oracle_with_rules(orc, None)
    o.sd = dict(orc.sd)
    for n in TYPE_B:
        o.sd[LL + n + ".bias"] = 2 * orc.sd[LL + n + ".bias"]
    return o


def decoded_by(enc, enc_rules, dec, dec_rules, ll):
    """ll_hat and rows of a decoder (dec, dec_rules) that decodes the symbols the encoder (enc, enc_rules) wrote, both
    evaluated one-shot on ll (the decoder's parameters at a position see the encoder's ll: exact up to the first
    difference, which is all a test needs)"""
    pe = Oracle_with_rules(enc, enc_rules).context_fusion_ll(CODER, ll)
    pd = Oracle_with_rules(dec, dec_rules).context_fusion_ll(CODER, ll)
    sym = (ll.round() - pe[:, 1:2]).round()
    idx_e = enc.K.build_indexes(enc.tables, pe[:, 0:1])
    idx_d = dec.K.build_indexes(dec.tables, pd[:, 0:1])
    return (sym + pe[:, 1:2]).round(), (sym + pd[:, 1:2]).round(), idx_e, idx_d


def head_rule_sensitive_set(orc, rules, ll, gain=100.0, tries=200):
    """orc with convs.2's mean weights scaled by `gain` and its mean bias tuned until, on ll, the decoded plane under
    the head rule of `rules` differs from the one under a head summed as one chain (rules[1] -> CHAIN): at some
    position sym + mean sits on a rounding edge of rint() between the two means.  Returns (Oracle, positions that
    differ).  A head reduction at rounding level is otherwise invisible in the decoded values."""
    import torch
    o = Oracle_with_rules(orc, None)
    o.sd = dict(orc.sd)
    w = o.sd[LL + ".convs.2.weight"].clone()
    w[1] *= gain
    o.sd[LL + ".convs.2.weight"] = w
    chain = (rules[0], CHAIN, rules[2])
    tried = set()
    for _ in range(tries):
        he, hd, ie, idd = decoded_by(o, rules, o, chain, ll)
        if torch.equal(he, ll) and (not torch.equal(he, hd) or not torch.equal(ie, idd)):
            return o, int(((he != hd) | (ie != idd)).sum())
        pe = Oracle_with_rules(o, rules).context_fusion_ll(CODER, ll)[:, 1]
        pc = Oracle_with_rules(o, chain).context_fusion_ll(CODER, ll)[:, 1]
        diff = (pe - pc).abs().flatten()
        order = [int(i) for i in torch.argsort(diff, descending=True) if diff[i] > 0]
        cand = [i for i in order if i not in tried]
        if not cand:
            break
        p = cand[0]
        tried.add(p)
        mid = (float(pe.flatten()[p]) + float(pc.flatten()[p])) / 2
        b = o.sd[LL + ".convs.2.bias"].clone()
        b[1] = float(np.float32(float(b[1]) + (np.floor(mid) + 0.5 - mid)))
        o.sd[LL + ".convs.2.bias"] = b
    raise AssertionError("no bias found that makes the head rule visible in the decoded plane")


def boundary_weight_set(orc, rules):
    """orc with the convs.2 scale bias moved so that the scale of the first position (its causal inputs are all zero:
    a function of the biases alone) lands on the boundary of row k.  Returns
    (Oracle, k, ulps off the boundary).  The target is the smallest f32 whose row (the oracle's, equal to the reference
    formula's at every boundary: tests/golden/reference_scale_index_boundaries.npz) is k: the scale where the row
    actually changes, which need not be the f32 nearest exp(lmin + k * step)."""
    import torch
    g = orc.tables
    o = Oracle_with_rules(orc, rules)
    o.sd = dict(orc.sd)
    z = torch.zeros(1, 1, 1, 1)
    scale0 = lambda: np.float32(o.context_fusion_ll(CODER, z)[0, 0, 0, 0])
    bits = lambda v: int(np.array([v], np.float32).view(np.int32)[0])
    row = lambda v: int(g.build_indexes_cdef(torch.tensor([v], dtype=torch.float32))[0])
    k = int((np.log(scale0()) - g.log_scale_min) / g.log_scale_step) + 1
    target = np.float32(np.exp(g.log_scale_min + k * g.log_scale_step))
    while row(np.nextafter(target, np.float32(0))) >= k:
        target = np.nextafter(target, np.float32(0))
    while row(target) < k:
        target = np.nextafter(target, np.float32(np.inf))
    bias, best = o.sd[LL + ".convs.2.bias"].clone(), None
    for _ in range(40):
        o.sd[LL + ".convs.2.bias"] = bias
        s = scale0()
        off = bits(s) - bits(target)
        if best is None or abs(off) < abs(best[1]):
            best = (bias, off)
        if off == 0:
            break
        b0 = np.float32(bias[0])
        nb = np.float32(b0 + (target - s))
        if nb == b0:                                   # below the bias's ulp: one ulp towards the target
            nb = np.nextafter(b0, np.float32(np.inf if off < 0 else -np.inf))
        bias = bias.clone()
        bias[0] = float(nb)
    o.sd[LL + ".convs.2.bias"] = best[0]
    return o, k, best[1]


@functools.lru_cache(maxsize=None)
def ll_planes():
    """real LL planes: the oracle's 4-level lifting of a synthetic luma frame, scaled by QP_ll (q_index 3), clamped to
    +-8192 and rounded, with its mean taken out (so that residuals of every size occur, not only DC-sized ones): a 16x16
    one, and a wide one for widths up to 352."""
    import torch
    import pmctf_synth
    from pmctf_oracle.model import Oracle, get_curr_q
    orc = Oracle(synth_sd(0), 1, "cdef")
    out = []
    for (w, h) in ((256, 256), (5632, 64)):
        f = pmctf_synth.synth_yuv420(w, h, 1, seed=77)
        y = pmctf_synth.frames_to_tensors(f[0])[0]
        ll = y
        for _ in range(4):
            ll = orc.forward_lift_2d(CODER, ll)["ll"]
        q = get_curr_q(orc.sd[f"{CODER}.QP_ll"], 3)
        ll = (ll * q).clamp(-8192, 8192).round()
        out.append((ll - ll.mean().round())[0, 0])
    return out


def ll_for(planes, N, H, W, salt):
    """N planes of H x W cropped from the real LL planes (different windows per plane), outliers +-8192 planted at the
    first position, at row starts and in the last column"""
    import torch
    src = planes[0] if H <= 16 and W <= 16 else planes[1]
    r = np.random.default_rng(salt)
    ll = torch.zeros(N, 1, H, W)
    for n in range(N):
        y0 = int(r.integers(0, src.shape[0] - H + 1))
        x0 = int(r.integers(0, src.shape[1] - W + 1))
        ll[n, 0] = src[y0:y0 + H, x0:x0 + W]
    sgn = 1.0 if salt % 2 else -1.0
    ll[0, 0, 0, 0] = 8192 * sgn
    for h in range(1, H, 2):
        ll[h % N, 0, h, 0] = -8192 * sgn
    for h in range(0, H, 3):
        ll[(h + 1) % N, 0, h, W - 1] = 8192 * sgn * (-1) ** h
    return ll


def escape_nibbles(sym, idx, sizes, offsets):
    """per symbol: -1 if coded directly, else the number of bypass nibbles of its escape (0 when raw == 0), signed by
    the direction of the escape (negative: below the table)"""
    value = sym.astype(np.int64) - offsets[idx]
    mx = sizes[idx].astype(np.int64) - 2
    esc = (value < 0) | (value >= mx)
    raw = np.where(value < 0, -2 * value - 1, 2 * (value - mx))
    n = np.zeros(sym.shape, np.int64)
    for j in range(8):
        n += (raw >> (4 * j)) != 0
    return np.where(esc, n, -1), np.where(value < 0, -1, 1)


def encode(tables, parts):
    """one stream (the product's host range coder) with the (symbols, indexes) parts in order"""
    from pMCTF.entropy_models.entropy_models import EntropyCoder
    ec = EntropyCoder()
    ec.reset()
    for s, i in parts:
        ec.encode_with_indexes(s, i, *tables)
    ec.flush()
    return ec.get_encoded_stream()


def make_case(orc, rules, ll, lead, trail):
    """-> dict: the oracle's one-shot parameters under `rules`, ll_hat, symbols and CDF rows in decode order (position-
    major, planes inner), the stream, and what a host decoder reports around the LL."""
    import torch
    from pMCTF.hip.engine import HostDecoder
    o = Oracle_with_rules(orc, rules)
    params = o.context_fusion_ll(CODER, ll)
    scales, means = params.chunk(2, dim=1)
    res = ll.round() - means
    sym = res.round()
    ll_hat = (sym + means).round()
    assert torch.equal(ll_hat, ll), "premise: ll_hat = ll, so the one-shot parameters are the decoder's"
    idx = o.K.build_indexes(o.tables, scales)
    order = lambda t: t.permute(2, 3, 0, 1).reshape(-1)
    s_ll = order(sym).clamp(-30000, 30000).to(torch.int16).numpy()
    i_ll = order(idx).to(torch.int16).numpy()
    cdf, sizes, offs = (np.ascontiguousarray(a, dtype=np.int32) for a in o.tables.cdf_info())
    tables = (cdf, sizes, offs)
    stream = encode(tables, [lead, (s_ll, i_ll), trail])
    dec = HostDecoder({"gauss": tables}, stream)
    assert np.array_equal(dec.decode(lead[1], "gauss"), lead[0])
    x0, pos0 = dec.get_state()
    assert np.array_equal(dec.decode(i_ll, "gauss"), s_ll)
    x1, pos1 = dec.get_state()
    assert np.array_equal(dec.decode(trail[1], "gauss"), trail[0])
    return {"ll_hat": ll_hat[:, 0].numpy(), "sym": s_ll, "idx": i_ll, "stream": stream, "words": dec.words.copy(),
            "x0": x0, "pos0": pos0, "x1": x1, "pos1": pos1, "scales": scales}


def Oracle_with_rules(orc, rules):
    """a shallow copy of orc whose sum_rule is forced to the rule triple (None: orc's own)"""
    from pmctf_oracle.model import Oracle
    o = Oracle.__new__(Oracle)
    o.__dict__.update(orc.__dict__)
    if rules is not None:
        o.sum_rule = forced_rules(*rules)
    return o


def side_symbols(salt, n, tables):
    """a run of symbols with mixed CDF rows (0, 255 and in between), escapes of both signs among them"""
    r = np.random.default_rng(salt)
    idx = r.integers(0, 256, n).astype(np.int16)
    idx[:4] = (0, 255, 0, 255)
    sizes, offs = tables[1], tables[2]
    lo, hi = offs[idx], offs[idx] + sizes[idx] - 3            # the directly coded range of each row
    sym = r.integers(lo, hi + 1).astype(np.int64)
    sym[1::7] = hi[1::7] + r.integers(1, 300, sym[1::7].size)
    sym[3::7] = lo[3::7] - r.integers(1, 300, sym[3::7].size)
    return sym.astype(np.int16), idx


def main():
    variant, cases, out = sys.argv[1:4]
    want = VARIANTS[variant]
    got = [k for k in SWITCHES if k in os.environ]
    assert got == ([want] if want else []), f"variant {variant} but switches {got} set"
    run_all(cases, out)


if __name__ == "__main__":
    main()
