"""The sequential LL decode (pmctf_ll_ar_decode_rules_f32, decode_ops.hip) driven directly, kernel by kernel, against the
oracle: the test chooses weights, LL planes, shapes and summation rules itself, instead of reaching the kernels through
pWave.decompress at the few LL shapes that padded frames produce.

For every case the expected values come from the CPU: the oracle's one-shot LL network under the forced rule triple
(ll_hat, the CDF rows), the product's host range coder (the stream, with symbols before the LL so that the entry state
is not the stream's first, and a known run after it), and a host decoder (the state after the LL).  Every case runs
under every kernel choice: the default, and the three environment switches (read once per process, so each of those
runs in a fresh child process, tests/ll_decode_helper.py).  Per case and variant: ll_out equal to ll_hat bit for bit,
the state equal to the host decoder's with the error flag clear, and a host decoder restarted from the kernel's state
decodes the trailing run.  A few cases have their stream cut in half: every variant must flag the error, return, and
leave finite values.

The decoded values depend on the parameters only through the CDF row and rint(symbol + mean), so with the synthetic
weights a kernel whose parameters are off by a little (a 1x1 head summed as one chain instead of reduce-B, a 3x3 bias
counted twice) flips nothing.  Two kinds of cases are there for such kernels, each checked on the CPU to be able to
see the error: "bb" has masked-layer biases of O(1), and the oracle with the type-B biases doubled decodes them
differently; "hs" has the mean's head amplified and its bias tuned until the oracle decodes differently under a head
summed as one chain than under the case's reduce-B head."""
import os
import subprocess
import sys
import time
from collections import Counter

import numpy as np
import pytest

import ll_decode_helper as hp
from ll_decode_helper import BLOCKS, CHAIN

pytestmark = pytest.mark.gpu

HEADS = [CHAIN, 16, 32, 48, 64, 80, 96, 112]       # convs.0 / convs.1: one chain or reduce-B
OUTS = [CHAIN, 16, 64, 112]                        # convs.2
# Kernel thresholds, from the LDS estimate of pmctf_ll_ar_decode_rules_f32 (hp.lds_bytes) with the gauss table's 103
# CDF columns: 112200 + 17944 N + 8 N W bytes against 150 KB (153600), the two-half row kernel 2048 N bytes more.
#   N = 2, rule "blocks": row2 up to W = 88, the one-thread row kernel for 89..344, v1 from 345
#   N = 2, rule "chain":  stream up to W = 344, v1 from 345
#   N = 1: row2 up to W = 2676, row up to 2932 (stream for "chain" up to 2932)
#   N = 3, 4: v1 always
# The widths 88 / 89 and 344 / 345 below straddle the N = 2 thresholds; test_thresholds_are_where_the_comment_says
# keeps this comment honest.
SHAPES = [(1, 1, 1), (1, 1, 9), (1, 5, 1), (1, 3, 7), (1, 4, 8), (1, 6, 13), (1, 16, 16), (2, 3, 9), (2, 4, 17),
          (2, 8, 60), (2, 2, 88), (2, 2, 89), (2, 2, 344), (2, 2, 345)]
WSETS = ["s0", "lo", "hi", "m+", "m-", "s1"]
CHILD_TIMEOUT = 600


def _case_list():
    """(weight set, N, H, W, (rule 3x3, rule head, rule out), truncated)"""
    out = []
    for j, (N, H, W) in enumerate(SHAPES):
        out.append((WSETS[len(out) % 6], N, H, W, (BLOCKS, HEADS[j % 8], OUTS[j % 4]), False))
        out.append((WSETS[len(out) % 6], N, H, W, (CHAIN, HEADS[(j + 3) % 8], OUTS[(j + 1) % 4]), False))
    # three and four planes (RGB stills): v1 under every variant.  (3, 16, 16) with head 80 is the product's 256x256 RGB
    # still: conv1x1_sum_rule gives B = 80 for convs.0/1 at an LL height of 11..27.
    out += [("s1", 3, 4, 6, (BLOCKS, 32, 16), False), ("lo", 3, 4, 6, (CHAIN, 112, CHAIN), False),
            ("s0", 3, 16, 16, (BLOCKS, 80, CHAIN), False), ("m-", 3, 16, 16, (CHAIN, 80, 64), False),
            ("hi", 4, 3, 5, (BLOCKS, 48, 112), False), ("m+", 4, 3, 5, (CHAIN, CHAIN, 16), False)]
    # O(1) masked-layer biases: a 3x3 bias counted twice or dropped changes the decoded plane (stream under "blocks"
    # with PMCTF_LL_AR_V2, row / row2 by default, v1)
    out += [("bb", 1, 4, 8, (BLOCKS, 32, 16), False), ("bb", 2, 8, 60, (BLOCKS, 112, CHAIN), False),
            ("bb", 1, 6, 13, (CHAIN, 64, 112), False), ("bb", 3, 4, 6, (BLOCKS, 96, CHAIN), False)]
    # a reduce-B head that decodes differently from one chain (weights tuned per case); v1 at N = 3
    out += [("hs", 3, 16, 16, (BLOCKS, 80, CHAIN), False), ("hs", 3, 16, 16, (CHAIN, 80, 64), False),
            ("hs", 2, 4, 17, (BLOCKS, 48, CHAIN), False)]
    # the scale of the first position exactly on a row boundary (weights tuned per rule triple)
    out += [("bd-blocks", 1, 2, 9, (BLOCKS, 64, CHAIN), False), ("bd-chain", 1, 2, 9, (CHAIN, 16, 64), False)]
    # truncated streams: escape-heavy cases, one per kind of kernel
    out += [("lo", 1, 4, 8, (BLOCKS, 96, 16), True), ("m-", 2, 3, 9, (CHAIN, 48, CHAIN), True),
            ("lo", 3, 4, 6, (CHAIN, 16, 112), True)]
    return out


@pytest.fixture(scope="module")
def ll_cases(tmp_path_factory):
    """build every case on the CPU once; write them for the child processes"""
    t0 = time.time()
    sets = hp.weight_sets()
    sets["bb"] = hp.big_bias_set()
    planes = hp.ll_planes()
    g = sets["s0"].tables
    tabs = tuple(np.ascontiguousarray(a, dtype=np.int32) for a in g.cdf_info())
    cases, blobs, wid = [], {}, {}
    for i, (ws, N, H, W, rules, trunc) in enumerate(_case_list()):
        ll = hp.ll_for(planes, N, H, W, i)
        k = off = teeth = None
        key = ws
        if ws.startswith("bd-"):
            orc, k, off = hp.boundary_weight_set(sets["s0"], rules)
            assert off == 0, f"{ws}: first scale {off} ulps off the boundary of row {k}"
        elif ws == "hs":
            orc, teeth = hp.head_rule_sensitive_set(sets["s0"], rules, ll)
            key = f"hs{i}"
        else:
            orc = sets[ws]
        if ws == "bb":
            he, hd, ie, idd = hp.decoded_by(orc, rules, hp.with_doubled_type_b_bias(orc), rules, ll)
            teeth = int(((he != hd) | (ie != idd)).sum())
            assert teeth > 0, f"case {i}: a doubled type-B bias would decode the same"
        if key not in wid:
            wid[key] = len(wid)
            blobs[f"w{wid[key]}"] = hp.pack_weights(orc.sd)
        lead = hp.side_symbols(100 + i, 5 + 3 * i, tabs)
        trail = hp.side_symbols(200 + i, 48, tabs)
        c = hp.make_case(orc, rules, ll, lead, trail)
        n_words = c["words"].size
        if trunc:
            n_words = (c["pos0"] + c["pos1"]) // 2
            assert c["pos1"] - n_words >= 4, "the cut must fall inside the LL"
        c.update(ws=ws, key=key, N=N, H=H, W=W, rules=rules, trunc=trunc, n_words=n_words, trail=trail,
                 boundary=(k, off), teeth=teeth)
        cases.append(c)
    path = str(tmp_path_factory.mktemp("ll_decode") / "cases.npz")
    arrays = {"cdf": tabs[0], "sizes": tabs[1], "offsets": tabs[2], "lmin": np.float64(g.log_scale_min),
              "lstep": np.float64(g.log_scale_step), "n_cases": np.int64(len(cases)), **blobs}
    for i, c in enumerate(cases):
        r3, rh, ro = c["rules"]
        arrays[f"c{i}_meta"] = np.array([c["N"], c["H"], c["W"], r3, rh, ro, c["pos0"], c["n_words"], wid[c["key"]]],
                                        np.int64)
        arrays[f"c{i}_x0"] = np.array([c["x0"]], np.uint64)
        arrays[f"c{i}_words"] = c["words"]
    np.savez(path, **arrays)
    print(f"\n{len(cases)} LL decode cases built on the CPU in {time.time() - t0:.1f} s")
    return {"path": path, "cases": cases, "tabs": tabs, "cols": tabs[0].shape[1]}


def _coverage(cases, tabs):
    """what the cases exercise, counted on the host from CDF rows and symbols"""
    nib, rows = Counter(), Counter()
    for c in cases:
        if c["trunc"]:
            continue
        n, sg = hp.escape_nibbles(c["sym"].astype(np.int64), c["idx"].astype(np.int64), tabs[1], tabs[2])
        for a, s in zip(n[n > 0].tolist(), sg[n > 0].tolist()):
            nib[(a, "+" if s > 0 else "-")] += 1
        rows["row 0"] += int((c["idx"] == 0).sum())
        rows["row 255"] += int((c["idx"] == 255).sum())
    return nib, rows


def test_thresholds_are_where_the_comment_says():
    cols, lim = 103, 150 * 1024
    for N, W in ((1, 1), (2, 1), (2, 300), (4, 7)):
        assert hp.lds_bytes(N, W, cols)[0] == 112200 + 17944 * N + 8 * N * W
    assert hp.lds_bytes(2, 88, cols)[1] <= lim < hp.lds_bytes(2, 89, cols)[1]
    assert hp.lds_bytes(2, 344, cols)[0] <= lim < hp.lds_bytes(2, 345, cols)[0]
    assert hp.lds_bytes(1, 2676, cols)[1] <= lim < hp.lds_bytes(1, 2677, cols)[1]
    assert hp.lds_bytes(1, 2932, cols)[0] <= lim < hp.lds_bytes(1, 2933, cols)[0]
    for N, W, want in ((2, 88, "row2<2>"), (2, 89, "row<2>"), (2, 344, "row<2>"), (2, 345, "v1 N=2")):
        assert hp.kernel_for("default", BLOCKS, N, W, cols) == want
    assert hp.kernel_for("default", CHAIN, 2, 344, cols) == "stream<2>"
    assert hp.kernel_for("default", CHAIN, 2, 345, cols) == "v1 N=2"


def test_every_ll_kernel_against_the_oracle(cuda, ll_cases, tmp_path):
    from pMCTF.hip.engine import HostDecoder
    cases, tabs, cols = ll_cases["cases"], ll_cases["tabs"], ll_cases["cols"]
    t0 = time.time()
    results = {}
    for variant, switch in hp.VARIANTS.items():
        if switch is None and not any(k in os.environ for k in hp.SWITCHES):
            results[variant] = hp.run_all(ll_cases["path"])
            continue
        env = {k: v for k, v in os.environ.items() if k not in hp.SWITCHES}
        if switch:
            env[switch] = "1"
        out = str(tmp_path / f"{variant}.npz")
        cmd = [sys.executable, hp.__file__, variant, ll_cases["path"], out]
        try:
            p = subprocess.run(cmd, env=env, timeout=CHILD_TIMEOUT, capture_output=True, text=True)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"variant {variant}: no exit within {CHILD_TIMEOUT} s\n{(e.stderr or '')[-3000:]}")
        if p.returncode != 0:
            pytest.fail(f"variant {variant}: exit status {p.returncode}\n{p.stderr[-3000:]}")
        d = np.load(out)
        results[variant] = {i: (d[f"c{i}_ll"], d[f"c{i}_state"]) for i in range(len(cases))}
    elapsed = time.time() - t0

    bad = []
    ran = Counter()
    for variant, res in results.items():
        for i, c in enumerate(cases):
            kern = hp.kernel_for(variant, c["rules"][0], c["N"], c["W"], cols)
            what = (f"{variant} / {kern}: case {i} {c['ws']} N={c['N']} H={c['H']} W={c['W']} rules={c['rules']}"
                    + (" truncated" if c["trunc"] else ""))
            ll, st = res[i]
            if c["trunc"]:
                if int(st[2]) != 1 or not np.isfinite(ll).all():
                    bad.append(f"{what}: error flag {int(st[2])}, finite {bool(np.isfinite(ll).all())}")
                ran[("truncated", kern)] += 1
                continue
            ran[(variant, kern, "blocks" if c["rules"][0] == BLOCKS else "chain", c["N"])] += 1
            if c["rules"][1] != CHAIN and c["N"] >= 3:
                ran[("reduce-B head", kern)] += 1
            if c["ws"] in ("bb", "hs"):
                ran[(c["ws"], kern, c["rules"][0])] += 1
            if not np.array_equal(ll, c["ll_hat"]):
                neq = np.argwhere(~(ll == c["ll_hat"]))
                first = tuple(neq[0])
                bad.append(f"{what}: {len(neq)} of {ll.size} values differ, first at {first}: {ll[first]!r} vs "
                           f"{c['ll_hat'][first]!r}")
                continue
            if (int(st[0]), int(st[1]), int(st[2])) != (c["x1"], c["pos1"], 0):
                bad.append(f"{what}: state {[int(v) for v in st]} vs host decoder {[c['x1'], c['pos1'], 0]}")
                continue
            dec = HostDecoder({"gauss": tabs}, c["stream"])
            dec.set_state(int(st[0]), int(st[1]))
            if not np.array_equal(dec.decode(c["trail"][1], "gauss"), c["trail"][0]):
                bad.append(f"{what}: the symbols after the LL do not decode from the kernel's state")
    nib, rows = _coverage(cases, tabs)
    print(f"\nLL decode: {len(cases)} cases x {len(results)} variants in {elapsed:.1f} s")
    for variant in hp.VARIANTS:
        print(f"  {variant}: " + ", ".join(f"{k[1]} {k[2]}: {n}" for k, n in sorted(ran.items(), key=str)
                                          if k[0] == variant))
    print("  truncated: " + ", ".join(f"{k[1]}: {n}" for k, n in sorted(ran.items(), key=str) if k[0] == "truncated"))
    print("  escapes by bypass nibbles and sign: " + ", ".join(f"{k[0]}{k[1]}: {n}" for k, n in sorted(nib.items())))
    print(f"  CDF rows: {dict(rows)}; boundary cases (k, ulps off): "
          f"{[c['boundary'] for c in cases if c['ws'].startswith('bd-')]}")
    print("  positions where the oracle decodes differently with a doubled type-B bias (bb) / a one-chain head (hs): "
          + ", ".join(f"{c['ws']} N={c['N']} {c['rules']}: {c['teeth']}" for c in cases if c["teeth"] is not None))
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:20])

    # the matrix did exercise what it is there for
    for n in (1, 2, 3, 4):
        for s in "+-":
            assert nib[(n, s)] > 0, f"no escape with {n} bypass nibbles, sign {s}"
    assert rows["row 0"] > 0 and rows["row 255"] > 0
    for variant in hp.VARIANTS:
        for N in (1, 2):
            for r3 in ("blocks", "chain"):
                assert any(k[0] == variant and k[2] == r3 and k[3] == N for k in ran), (variant, N, r3)
    kernels = {k[1] for k in ran if k[0] in hp.VARIANTS}
    assert kernels >= {"row2<1>", "row2<2>", "row<1>", "row<2>", "stream<1>", "stream<2>", "v1 N=1", "v1 N=2",
                       "v1 N=3", "v1 N=4"}, kernels
    assert ("v2", "stream<1>", "blocks", 1) in ran and ("v2", "stream<2>", "blocks", 2) in ran
    assert ("v1", "v1 N=1", "blocks", 1) in ran and ("v1", "v1 N=2", "blocks", 2) in ran
    assert ran[("reduce-B head", "v1 N=3")] > 0
    # the cases that see small parameter errors reached the kernels they are there for
    assert ("bb", "stream<1>", BLOCKS) in ran and ("bb", "stream<2>", BLOCKS) in ran
    assert ("hs", "v1 N=3", BLOCKS) in ran and ("hs", "v1 N=3", CHAIN) in ran
    assert {k[1] for k in ran if k[0] == "truncated"} >= {"row2<1>", "row<1>", "stream<1>", "stream<2>", "v1 N=1",
                                                         "v1 N=2", "v1 N=3"}
