"""The large-plane table (large_planes.py) without a GPU: every row's byte counts lie on the side of the boundary it claims,
the expected launch keys are kernels the sources launch, every size guard of the dispatchers has its rows or a named
exemption (a new guard fails here), window_reference equals the full-plane oracle on a small plane for every (kernel size,
stride, rule, padding) of the table, and a read that wrapped at 2^32 bytes would be caught by the table's data."""
import os
import re

import numpy as np
import pytest

import conv_census as cc
import ew_census as ec
import large_planes as lp
from test_conv_census_cpu import launched_expressions

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "learned-pmctf_amd", "csrc")
AUDITED = ("conv_mfma.hip", "basic_ops.hip", "ew_ops.hip", "conv_epilogue.h", "pu_fused.hip", "conv_split.hip", "estimate_ops.hip",
           "decode_ops.hip", "picture_ops.hip")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


IDS = [r[0] for r in lp.ROWS]


def test_rows_are_well_formed():
    assert len(set(IDS)) == len(IDS)
    for r in lp.ROWS:
        rid, entry, g, rule, act, nres, knobs, expected, boundary, side = r
        assert entry in ("conv", "conv_geom", "smallcin", "fewcout", "dw", "nearest_up2", "pixel_shuffle2", "ffn3_mix", "lstm_gates", "ew") + lp.FOURSTEP, rid
        assert len(g) == (9 if entry == "ew" or entry in lp.FOURSTEP else 8) and rule in (0, 1) and act in range(5) and nres in (0, 1, 2), rid
        assert side in ("under", "over") and boundary[1] in (lp.G31, lp.G31 - 1, lp.G32) and boundary[2] in ("bytes", "elements"), rid
        assert set(knobs) <= set(cc.KNOBS), rid
        assert rid.endswith("__" + side) or "__" not in rid, rid
        assert g[3] % 16 and g[3] % 32 or entry == "ew" or rid.startswith("batch_") or g[3] == 8200, f"{rid}: the width is a multiple of the tile"
    pairs = {rid[:-7] for rid in IDS if rid.endswith("__under")}
    assert pairs == {rid[:-6] for rid in IDS if rid.endswith("__over")}
    for p in pairs:                             # a pair differs in the height alone (and in what it launches)
        u, o = lp.row(p + "__under"), lp.row(p + "__over")
        assert u[1] == o[1] and u[2][:2] == o[2][:2] and u[2][3:] == o[2][3:] and u[6] == o[6] and u[7] != o[7], p
        assert 0 < o[2][2] - u[2][2] <= 2, p


@pytest.mark.parametrize("rid", IDS)
def test_row_lies_on_the_side_it_claims(rid):
    r = lp.row(rid)
    (operand, limit, unit), side = r[8], r[9]
    value, pitch = lp.boundary_value(r)
    if side == "under":
        assert value < limit and value + pitch >= limit, f"{rid}: {value} is not within one row ({pitch}) below {limit}"
        if limit == lp.G32:
            assert value > lp.G31                # the specialised kernel still meets offsets past 2^31
    else:
        assert value >= limit, f"{rid}: {value} < {limit}"
    assert lp.need_bytes(r) <= lp.MEMORY_CAP, f"{rid}: needs {lp.need_bytes(r) / 2 ** 30:.1f} GiB"
    for n, o0, o1, i0, i1 in lp.bands(r):        # every band is the regime the other censuses verify
        N, Cin, H, W = r[2][:4]
        Ho, Wo, Co = lp.out_dims(r)
        assert 4 * (i1 - i0) * W * Cin < lp.G31 and 4 * (o1 - o0 + 4) * Wo * Co < lp.G31 and 0 <= i0 < i1 <= H, rid
    covered = sorted((n, o0, o1) for n, o0, o1, i0, i1 in lp.bands(r))
    assert [c[1] for c in covered if c[0] == 0][0] == 0 and covered[-1][2] == lp.out_dims(r)[0]
    for a, b in zip(covered, covered[1:]):
        assert (a[0] == b[0] and a[2] == b[1]) or (a[0] + 1 == b[0] and b[1] == 0), rid


def test_windows_sit_on_the_boundaries():
    """per row: the corners, a window that holds the pixel at every 2^31 / k * 2^32 byte offset of either operand, the last
    pixel; at most 16 x 96; origins off the tile grid"""
    for r in lp.ROWS:
        N, Cin, H, W, Cout, K, S, pad = r[2][:8]
        Ho, Wo, Co = lp.out_dims(r)
        wins = lp.windows(r)
        assert len(wins) >= 4 + 1 + lp.N_RANDOM and all(w[4] <= lp.WIN_H and w[5] <= lp.WIN_W for w in wins), r[0]
        for what, n, oy0, ox0, h, w in wins:
            assert 0 <= n < N and 0 <= oy0 and oy0 + h <= Ho and 0 <= ox0 and ox0 + w <= Wo, (r[0], what)
        names = [w[0] for w in wins]
        for total, word, px in ((4 * N * H * W * Cin, "input", 4 * Cin), (4 * N * Ho * Wo * Co, "output", 4 * Co)):
            for b in [lp.G31] + list(range(lp.G32, total, lp.G32)):
                if b < total:
                    assert f"{word} byte {b:#x}" in names, (r[0], word, b)
                    if word == "output":
                        what, n, oy0, ox0, h, w = wins[names.index(f"output byte {b:#x}")]
                        p = b // px
                        nn, rem = divmod(p, Ho * Wo)
                        assert nn == n and oy0 <= rem // Wo < oy0 + h and ox0 <= rem % Wo < ox0 + w, (r[0], what)
        interior = [w for w in wins if 0 < w[2] and w[2] + w[4] < Ho and 0 < w[3] and w[3] + w[5] < Wo]
        assert interior and all(w[2] % 2 == 1 and w[3] % 2 == 1 for w in interior), r[0]


def test_expected_keys_are_kernels_the_sources_launch():
    conv = launched_expressions(_source("conv_mfma.hip"))
    valu = _source("basic_ops.hip")
    ew = _source("ew_ops.hip")
    for r in lp.ROWS:
        if r[1] in ("conv", "conv_geom"):
            assert r[7] and {e[0] for e in r[7]} <= conv, r[0]
        elif r[7] is not None:
            name = r[7].split("<")[0].split(" ")[0]
            assert re.search(r"__global__[^;{]*\bvoid %s\(" % name, valu if r[1] in ("smallcin", "fewcout", "dw") else ew), r[0]
    # the kernels the issue of this census names, by launch expression
    keys = {e[0] for r in lp.ROWS if r[1] in ("conv", "conv_geom") for e in r[7]} | {r[7] for r in lp.ROWS if isinstance(r[7], str)}
    for k in ("conv3x3s1_wave_kernel<MT, 2>", "conv3x3s1_wave_kernel<MT, 1>", "conv3x3s1_pipe_kernel<MT>", "conv3x3s1_pipe_kernel<MT, 2>",
              "conv7x7s1_pipe_kernel<MT, NT>", "conv7x7s1_pipe_kernel<MT, NT, true>", "conv3x3s1_blocks_tileouter_kernel",
              "conv3x3s1_wave_kernel<MT, NB, true>", "conv3x3s1_pipe_kernel<MT, 1, true>", "conv3x3s1_pipe_kernel<MT, 2, true>",
              "conv_mfma_kernel<MT, NT, TW16>", "conv_mfma_wave_kernel<MT, 7>", "conv_mfma_wave_kernel<MT, 7, 1>",
              "conv_mfma_pipe_kernel<MT, NT, TW16, 6>", "conv_mfma_pipe_kernel<MT, NT, TW16, 9>", "conv_mfma_bsum_kernel<MT, NT, TW16>",
              "conv1x1_kernel<MTW, NT>", "conv16_band_kernel", "conv16_persistent_kernel", "conv3x3_smallcin_strip_kernel<1>",
              "conv_smallcin_reg_kernel<1, 2>", "conv_fewcout_lds_kernel<3, 64, 1>", "conv_fewcout_pix_kernel<3, 64, 1>",
              "dwconv3_column_kernel<4, 8>", "nearest_up2_vec4_kernel", "pixel_shuffle2_vec4_kernel", "ew_flat_kernel<true>",
              "ew_c4_kernel<long> channels", "ew_kernel<true, long>", "ew_kernel<false, long>"):
        assert k in keys, k
    assert {r[1] for r in lp.ROWS} >= {"ffn3_mix", "lstm_gates"}
    # the long forms of the elementwise census are rows here, and its int forms run next to them
    assert {ec_long for ec_long in lp.EW_LONG_FORMS} == {k.split(" ")[0] if k.endswith(("channels", "rows")) else k for k in keys if "long" in k}
    assert {ec.C4_CH, ec.GEN_C, ec.GEN_P} <= keys


def guards_in(text):
    """the size guards of a source: every comparison against 2^30, 2^31, 2^31 - 1 or 2^32, as the source words it"""
    flat = " ".join(re.sub(r"//[^\n]*", "", text).replace("\\\n", " ").split())
    found = []
    for m in re.finditer(r"1ull << 32|1L << 3[01]|0x7fffffffL", flat):
        start = max(flat.rfind(tok, 0, m.start()) + len(tok) for tok in ("&& ", "|| ", "if (", " = ", "; ", "{ "))
        end = m.end() + (1 if flat[m.end():m.end() + 1] == ")" and flat[m.start() - 1] == "(" else 0)
        found.append(flat[start:end].strip())
    return found


def test_every_size_guard_has_its_rows_or_an_exemption():
    seen = set()
    for name in AUDITED:
        found = guards_in(_source(name))
        for text in set(found):
            assert (name, text) in lp.GUARDS, f"{name}: a size guard without rows or an exemption: {text!r}"
            want = len(lp.GUARDS[(name, text)])
            assert found.count(text) == want, f"{name}: {text!r} occurs {found.count(text)} times, the table has {want}"
            seen.add((name, text))
    assert seen == set(lp.GUARDS), sorted(set(lp.GUARDS) - seen)
    product = _source_of_test("test_product_cpu.py")
    assert "for name, (entry, args) in lp.REFUSALS.items():" in product       # the product test makes exactly these calls
    assert {site[1] for sites in lp.GUARDS.values() for site in sites if site[0] == "refusal"} == set(lp.REFUSALS)
    for (name, text), sites in lp.GUARDS.items():
        for site in sites:
            if site[0] == "rows":
                for p in site[1:]:
                    u, o = lp.row(p + "__under"), lp.row(p + "__over")
                    assert u[7] != o[7], p
            elif site[0] == "refusal":
                assert site[1] in lp.REFUSALS, f"{text}: no refusal call for {site[1]} in large_planes.REFUSALS"
            else:
                assert site[0] == "exempt" and len(site[1]) > 20
    assert all(size <= lp.MEMORY_CAP or "cap" in why for _, size, why in lp.EXEMPT_ROWS)


def _source_of_test(name):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), name)) as f:
        return f.read()


def test_the_goff_product_is_taken_unsigned():
    """the per-lane byte offset of the four specialised kernel bodies must not go back to a signed product that is cast
    afterwards (undefined between 2^31 and 2^32); any defined wording passes, the `__under` rows on the GPU hold the values"""
    lines = [l for l in _source("conv_mfma.hip").splitlines() if re.search(r"\bgoff\[j\] = ", l)]
    assert len(lines) == 4
    for l in lines:
        assert not re.search(r"\(unsigned\)\(\(\(gy \* a\.W \+ gx\) \* a\.Cin", l), l


def test_each_site_of_the_2_32_guard_launches_what_its_rows_expect():
    """the six occurrences of the 4 GiB guard in source order: the code between one occurrence and the next launches the
    specialised kernels that the under rows of THAT site expect — the rows of one site cannot stand in for another's"""
    flat = " ".join(_source("conv_mfma.hip").split())
    sites = lp.GUARDS[("conv_mfma.hip", lp.SIX)]
    at = [m.start() for m in re.finditer(re.escape(lp.SIX), flat)]
    assert len(at) == len(sites) == 6
    ends = at[1:] + [at[-1] + 400]
    seen = []
    for site, a, b in zip(sites, at, ends):
        launched = {cc.strip_parens(m) for m in re.findall(r"CONV_LAUNCH\((\([^()]*\)|[^,()]*),", flat[a:b])}
        expected = {e[0] for p in site[1:] for e in lp.row(p + "__under")[7]}
        assert expected <= launched, f"site {site[1:]}: the rows expect {sorted(expected - launched)}, the site launches {sorted(launched)}"
        seen.append(expected)
    assert len({frozenset(e) for e in seen}) == 6              # no two sites are covered by the same kernels


# ---- window_reference against the full-plane oracle -------------------------------------------------------------------------------
def _small(r, H=23, W=41, N=2):
    """the row on a small plane: same entry, channels (at most 32 in), kernel size, stride, padding, rule, activation"""
    g = r[2]
    cin = g[1] if g[1] <= 4 or r[1] not in ("conv", "conv_geom") else 32
    if r[1] in ("dw",):
        cin = 8
    cout = cin if r[1] == "dw" else min(g[4], 24)
    if r[1] == "fewcout":
        cin, cout = 64, 1
    if r[1] == "conv_geom":
        H, W = 24, 42
    return (r[0],) + (r[1], (N, cin, H, W, cout) + tuple(g[5:8])) + r[3:]


def _full_plane(r, x, w, b, res):
    """the oracle on the whole small plane with the layer's own padding: (N, Ho, Wo, Cout)"""
    from pmctf_oracle import clib
    N, Cin, H, W, Cout, K, S, pad = r[2][:8]
    xc = np.ascontiguousarray(x.transpose(0, 3, 1, 2))
    if r[1] == "dw":
        return clib.dwconv2d(xc, w, b).transpose(0, 2, 3, 1)
    if r[1] == "conv_geom":                      # stride 2, padding `pad` above / left: the class positions of the 'same' conv
        full = clib.conv2d(xc, w, b, 1, (1, 1), r[3])
        y = full[:, :, 1 - pad::2, 1 - pad::2]
    else:
        y = clib.conv2d(xc, w, b, S, (pad, pad), r[3])
    y = lp._act(np.ascontiguousarray(y.transpose(0, 2, 3, 1)), r[4], lp.SLOPE)
    for q in res:
        y = y + q
    return y


CONV_KINDS = sorted({(r[1], r[2][5], r[2][6], r[2][7], r[3]): r[0] for r in lp.ROWS
                     if r[1] in ("conv", "conv_geom", "smallcin", "fewcout", "dw")}.items())


@pytest.mark.parametrize("kind,rid", CONV_KINDS, ids=[f"{k[0]}-k{k[1]}s{k[2]}p{k[3]}r{k[4]}" for k, _ in CONV_KINDS])
def test_window_reference_is_the_full_plane_oracle(kind, rid):
    """every (entry, kernel size, stride, padding, rule) of the table: the windows of the small plane (corners, edges,
    interior, random) equal the full-plane oracle bit for bit — and a window shifted by one pixel does not"""
    r = _small(lp.row(rid))
    N, Cin, H, W, Cout, K, S, pad = r[2][:8]
    Ho, Wo, Co = lp.out_dims(r)
    g = np.random.default_rng(lp.seed(rid))
    x = g.standard_normal((N, H, W, Cin), dtype=np.float32) * np.float32(3)
    w, b = lp.weights(r)
    res = [g.standard_normal((N, Ho, Wo, Co), dtype=np.float32) for _ in range(r[5])]
    full = _full_plane(r, x, w, b, res)
    assert full.shape == (N, Ho, Wo, Co)
    wins = lp.windows(r) + [("interior", 1, 3, 5, 7, 13), ("left edge", 0, 5, 0, 4, 9), ("bottom edge", 1, Ho - 3, 7, 3, 11)]
    interior = 0
    for win in wins:
        what, n, oy0, ox0, h, wd = win
        iy0, ix0, ih, iw = lp.input_window(r, win)
        xw = lp.crop_zero_extended(x[n], iy0, ix0, ih, iw)
        got = lp.window_reference(r, win, xw, w, b, [q[n, oy0:oy0 + h, ox0:ox0 + wd] for q in res])
        want = np.ascontiguousarray(full[n, oy0:oy0 + h, ox0:ox0 + wd])
        assert got.shape == want.shape and (got.view(np.uint32) == want.view(np.uint32)).all(), (rid, what)
        interior += 0 < oy0 and oy0 + h < Ho and 0 < ox0 and ox0 + wd < Wo
    assert interior >= 1
    other = np.ascontiguousarray(full[1, 4:11, 5:18])
    assert (other.view(np.uint32) != np.ascontiguousarray(full[1, 3:10, 5:18]).view(np.uint32)).mean() > 0.5


@pytest.mark.parametrize("entry", ["nearest_up2", "pixel_shuffle2", "ffn3_mix", "lstm_gates"])
def test_element_window_reference(entry):
    """the element kernels' window reference against the torch expression each replaces, on a small plane"""
    import torch
    import torch.nn.functional as F
    big = next(r for r in lp.ROWS if r[1] == entry)
    cin = {"nearest_up2": 8, "pixel_shuffle2": 32, "ffn3_mix": 16, "lstm_gates": 8}[entry]
    r = (big[0], entry, (2, cin, 9, 21, 8, 1, 1, 0)) + big[3:]
    g = np.random.default_rng(7)
    x = g.standard_normal((2, 9, 21, cin), dtype=np.float32) * np.float32(3)
    cell = g.standard_normal((2, 9, 21, 8), dtype=np.float32)
    xt = torch.from_numpy(x).permute(0, 3, 1, 2)
    if entry == "nearest_up2":
        full = F.interpolate(xt, scale_factor=2, mode="nearest")
    elif entry == "pixel_shuffle2":
        full = F.pixel_shuffle(xt, 2)
    elif entry == "ffn3_mix":
        full = F.leaky_relu(xt[:, :8], 0.1) + F.leaky_relu(xt[:, 8:], 0.01)
    else:
        full = None
    for win in lp.windows(r):
        what, n, oy0, ox0, h, wd = win
        iy0, ix0, ih, iw = lp.input_window(r, win)
        xw = lp.crop_zero_extended(x[n], iy0, ix0, ih, iw)
        got = lp.window_reference(r, win, xw, extra=cell[n, oy0:oy0 + h, ox0:ox0 + wd])
        if full is not None:
            want = np.ascontiguousarray(full[n].permute(1, 2, 0).numpy()[oy0:oy0 + h, ox0:ox0 + wd])
            assert got.shape == want.shape and (got.view(np.uint32) == want.view(np.uint32)).all(), (entry, what)
        else:                                    # PM-F32 sigmoid / tanh: the oracle's own functions, element by element
            from pmctf_oracle import clib
            v = x[n, oy0:oy0 + h, ox0:ox0 + wd]
            f, c = clib.sigmoid(v), cell[n, oy0:oy0 + h, ox0:ox0 + wd]
            cn = f * c + f * clib.tanh(v)
            assert got.shape == (2, h, wd, 8) and (got[1] == cn).all() and (got[0] == f * clib.tanh(cn)).all()


def test_a_wrapped_read_is_caught():
    """a kernel whose input offset wrapped at 2^32 bytes reads the pixel 2^30 elements earlier: on a mock plane whose input
    is rotated by that many elements (mod the plane), at least half of every window's bit patterns change — the table's
    data (independent normal values) cannot hide a wrong offset"""
    for rid in ("wave33_mt7__under", "k77_32_64__under", "pipe33_s2_mt7__under", "dw_column_112", "ffn3_mix_112"):
        r = _small(lp.row(rid)) if lp.row(rid)[1] != "ffn3_mix" else (rid, "ffn3_mix", (2, 16, 9, 21, 8, 1, 1, 0)) + lp.row(rid)[3:]
        N, Cin, H, W, Cout, K, S, pad = r[2][:8]
        g = np.random.default_rng(lp.seed(rid))
        x = g.standard_normal((N, H, W, Cin), dtype=np.float32) * np.float32(3)
        shift = (lp.G32 // 4) % (H * W * Cin)
        assert shift % (H * W * Cin) != 0
        wrapped = np.roll(x.reshape(N, -1), shift, axis=1).reshape(x.shape)
        w, b = lp.weights(r)
        for win in lp.windows(r)[:6]:
            what, n, oy0, ox0, h, wd = win
            iy0, ix0, ih, iw = lp.input_window(r, win)
            a = lp.window_reference(r, win, lp.crop_zero_extended(x[n], iy0, ix0, ih, iw), w, b)
            c = lp.window_reference(r, win, lp.crop_zero_extended(wrapped[n], iy0, ix0, ih, iw), w, b)
            assert (a.view(np.uint32) != c.view(np.uint32)).mean() >= 0.5, (rid, what)


def test_first_difference_names_the_element():
    r = lp.row("wave33_mt7__under")
    Ho, Wo, Co = lp.out_dims(r)
    assert lp.first_difference(((5 * Wo) + 7) * Co + 3, r) == ((0, 5, 7, 3), 4 * (((5 * Wo) + 7) * Co + 3))



@pytest.mark.parametrize("rid", [r[0] for r in lp.ROWS if r[1] in lp.FOURSTEP])
def test_fourstep_window_reference_is_the_full_plane_restatement(rid):
    """the four-step rows on a small plane: every window (odd origins, corners, edges) of window_reference equals the
    entropy tests' restatement of the whole plane, for the full-size parameters and for those at the class positions"""
    import torch
    import entropy_restatement as er
    big = lp.row(rid)
    r = (rid, big[1], (2, 2, 11, 23, 1, 1, 1, 0, big[2][8])) + big[3:]
    N, _, Hp, Wp = r[2][:4]
    H, W, _ = lp.out_dims(r)
    assert (H, W) == ((22, 46) if big[2][8] == "psub" else (11, 23))
    if big[2][8] == "full":                                      # even planes: the windows' even alignment needs them
        r = (rid, big[1], (2, 2, 12, 24, 1, 1, 1, 0, "full")) + big[3:]
        N, _, Hp, Wp = r[2][:4]
        H, W, _ = lp.out_dims(r)
    g = np.random.default_rng(lp.seed(rid))
    params = g.standard_normal((N, Hp, Wp, 2), dtype=np.float32)
    params[..., 0] = np.abs(params[..., 0]) * 3 + np.float32(0.01)
    quant = big[1] == "fourstep_quant"
    planes = (g.standard_normal((N, H, W), dtype=np.float32) * 3) if quant else g.integers(-200, 201, (N, H, W)).astype(np.int16)
    par = torch.from_numpy(np.ascontiguousarray(params.transpose(0, 3, 1, 2)))
    sc, mn = par[:, 0:1], par[:, 1:2]
    if big[2][8] == "psub":
        sc, mn = er.place_class(sc, lp.FOURSTEP_K, H, W, 7.0), er.place_class(mn, lp.FOURSTEP_K, H, W, -3.0)
    pl = torch.from_numpy(planes)[:, None]
    if quant:
        so_far, sym, idx = er.fourstep_quant(pl, sc, mn, None, lp.FOURSTEP_K)
        full = (so_far.numpy()[:, 0], sym.reshape(N, H, W).numpy(), idx.reshape(N, H, W).numpy())
    else:
        full = (er.fourstep_dequant(pl, mn, None, lp.FOURSTEP_K).numpy()[:, 0],)
    assert (full[0] != 0).mean() > 0.2
    for win in lp.windows(r) + [("odd interior", 1, 3, 5, 6, 11)]:
        what, n, oy0, ox0, h, wd = win
        ey0, ex0, eh, ew = lp.even_window(win)
        assert ey0 % 2 == 0 and ex0 % 2 == 0 and eh % 2 == 0 and ew % 2 == 0 and ey0 <= oy0 and oy0 + h <= ey0 + eh <= H and ex0 + ew <= W
        iy0, ix0, ih, iw = lp.input_window(r, win)
        got = lp.window_reference(r, win, params[n, iy0:iy0 + ih, ix0:ix0 + iw], extra=planes[n, ey0:ey0 + eh, ex0:ex0 + ew])
        for a, b in zip(got, full):
            want = b[n, oy0:oy0 + h, ox0:ox0 + wd]
            assert a.shape == want.shape and a.tobytes() == np.ascontiguousarray(want).tobytes(), (rid, what)
