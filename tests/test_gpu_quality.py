"""Picture-quality kernels on the GPU (csrc/quality_ops.hip through pMCTF.hip.ops.frame_quality, pmctf_gop.gop_quality /
encode_sequence(msssim=True) / sequence_quality and tools/sequence_quality.py).

Yardsticks (tests/quality_restatement.py): the harness's own torch statements on CPU tensors with int64 error sums — the
kernel's four sums must EQUAL them; the project's gop_psnr / rgb_psnr on the CPU at the standing 1e-4 dB; the float64
restatement of MS-SSIM on the CPU, with the float32 run of the same code (what the package would have computed) giving the
scale of the allowed error:  |hip - r64| <= max(2 * |r32 - r64|, 16 * 2^-24),  for the result and for each of the 30 map
means; the real reference's per-frame PSNR stored in the 1080p digest."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import quality_restatement as qr
from helpers import frames, product_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 16 * 2.0 ** -24
PSNR_BAR = 1e-4                                   # dB, README "Parity"
_cases = {}


def _case(Hp, Wp, h, w, i):
    """the picture pair, its CPU yardsticks (computed once per session) -> dict"""
    key = (Hp, Wp, h, w, i)
    if key not in _cases:
        t = qr.quality_case(Hp, Wp, h, w, qr.NOISE[i], seed=i)
        sse, rgb_rec, rgb_org = qr.integer_sse(*t, h, w)
        c = {"tensors": t, "sse": sse}
        if min(h, w) > qr.MIN_SIDE:
            c["r64"], c["m64"] = qr.ms_ssim(rgb_rec, rgb_org, dtype=torch.float64)
            c["r32"], c["m32"] = qr.ms_ssim(rgb_rec, rgb_org, dtype=torch.float32)
        _cases[key] = c
    return _cases[key]


def _bound(v64, v32):
    return max(2.0 * abs(v32 - v64), FLOOR)


@pytest.mark.parametrize("Hp,Wp,h,w", qr.CASES)
def test_squared_error_sums_are_exact_and_psnr_matches(cuda, Hp, Wp, h, w):
    import pmctf_gop
    from pMCTF.hip import ops
    for i, sigma in enumerate(qr.NOISE):
        c = _case(Hp, Wp, h, w, i)
        rec_y, rec_c, org_y, org_c = c["tensors"]
        if i == len(qr.NOISE) - 1:              # premises: the clamp and the ties are live
            assert float(rec_y.min()) < -1.0 and float(rec_y.max()) > 256.0
        assert float(rec_y[0, 0, 3, 2]) == -1.5 and float(rec_c[1, 0, 4, 3]) % 1.0 == 0.5
        q = ops.frame_quality(*(t.to(cuda) for t in c["tensors"]), h, w, msssim=False)
        print(f"\n{h}x{w} in {Hp}x{Wp}, sigma {sigma}: SSE (Y, Cb, Cr, RGB) {q['sse']}, CPU int64 {c['sse']}")
        assert q["sse"] == c["sse"]
        assert all(type(v) is int for v in q["sse"]) and q["msssim"] == 0.0
        ref = pmctf_gop.gop_psnr([(rec_y, rec_c, None)], [(org_y, org_c)], h, w)[0]
        ry = torch.round(rec_y.clamp(0, 255.0))[:, :, :h, :w]
        rc = torch.round(rec_c.clamp(0, 255.0))[:, :, :h // 2, :w // 2]
        ref["rgb"] = pmctf_gop.rgb_psnr(ry, rc, org_y, org_c)
        for k in ("y", "cb", "cr", "yuv", "rgb"):
            print(f"    {k}-PSNR {q[k]:.6f} dB, torch on the CPU {ref[k]:.6f} dB")
            assert type(q[k]) is float and abs(q[k] - ref[k]) < PSNR_BAR, k


@pytest.mark.parametrize("Hp,Wp,h,w", [c for c in qr.CASES if min(c[2:]) > qr.MIN_SIDE])
def test_msssim_against_the_float64_restatement(cuda, Hp, Wp, h, w):
    from pMCTF.hip import ops
    for i, sigma in enumerate(qr.NOISE):
        c = _case(Hp, Wp, h, w, i)
        assert all(m > 0 for scale in c["m64"] for ch in scale for m in ch), "a relu fires: the comparison would be empty"
        q = ops.frame_quality(*(t.to(cuda) for t in c["tensors"]), h, w, msssim=True, return_means=True)
        assert q["sse"] == c["sse"]
        err, e32 = abs(q["msssim"] - c["r64"]), abs(c["r32"] - c["r64"])
        worst = (0.0, None)
        for s in range(5):
            for ch in range(3):
                for k in range(2):
                    e = abs(q["means"][s][ch][k] - c["m64"][s][ch][k])
                    b = _bound(c["m64"][s][ch][k], c["m32"][s][ch][k])
                    worst = max(worst, (e / b, (s, ch, "cs ssim".split()[k], e, b)))
        print(f"\nmsssim-accuracy {h}x{w} sigma {sigma}: r64 {c['r64']:.12f} e32 {e32:.3e} hip {q['msssim']:.12f} "
              f"|hip-r64| {err:.3e} bound {_bound(c['r64'], c['r32']):.3e}; worst mean (scale, channel, map, error, bound) "
              f"{worst[1]}")
        assert err <= _bound(c["r64"], c["r32"])
        assert worst[0] <= 1.0, worst
        assert 0.0 < q["msssim"] < 1.0


def test_identical_pictures_determinism_and_streams(cuda):
    from pMCTF.hip import ops
    h, w, Hp, Wp = 192, 256, 256, 256
    c = _case(Hp, Wp, h, w, 1)
    rec_y, rec_c, org_y, org_c = (t.to(cuda) for t in c["tensors"])
    pad = lambda t, hh, ww: torch.nn.functional.pad(t, (0, ww - t.shape[-1], 0, hh - t.shape[-2])) + 0.25
    same = ops.frame_quality(pad(org_y, Hp, Wp), pad(org_c, Hp // 2, Wp // 2), org_y, org_c, h, w)     # rounds back
    assert same["msssim"] == 1.0 and same["sse"] == (0, 0, 0, 0)
    assert all(same[k] == math.inf for k in ("y", "cb", "cr", "yuv", "rgb"))
    a = ops.frame_quality(rec_y, rec_c, org_y, org_c, h, w, return_means=True)
    b = ops.frame_quality(rec_y, rec_c, org_y, org_c, h, w, return_means=True)
    assert a == b                                # every float bit-identical
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        d = ops.frame_quality(rec_y, rec_c, org_y, org_c, h, w, return_means=True)
    s.synchronize()
    assert d == a
    # the sizes the harness and the package treat specially
    small = _case(128, 256, 100, 132, 0)
    assert ops.frame_quality(*(t.to(cuda) for t in small["tensors"]), 100, 132, msssim=True)["msssim"] == 0.0
    y, cc = torch.zeros((1, 1, 256, 256), device=cuda), torch.zeros((2, 1, 128, 128), device=cuda)
    with pytest.raises(ValueError, match="160"):
        ops.frame_quality(y, cc, y[..., :160, :200].contiguous(), cc[..., :80, :100].contiguous(), 160, 200)
    assert ops.frame_quality(y, cc, y[..., :160, :200].contiguous(), cc[..., :80, :100].contiguous(), 160, 200,
                             msssim=False)["y"] == math.inf


@pytest.fixture(scope="module")
def driven(cuda, tmp_path_factory):
    """8 frames 264x200 (padded 384x256), GOP 4, q_index 3: coded twice (with and without MS-SSIM), decoded to a .yuv"""
    import pmctf_gop
    import pmctf_synth
    td = tmp_path_factory.mktemp("quality")
    w, h, gop, n = 264, 200, 4, 8
    src = str(td / "src.yuv")
    pmctf_gop.write_yuv(src, pmctf_synth.synth_yuv420(w, h, n, seed=11))
    net, _ = product_model(1)
    out = {}
    for name, ms in (("with", True), ("without", False)):
        bins = str(td / f"bins_{name}")
        os.makedirs(bins)
        out[name] = pmctf_gop.encode_sequence(net, src, w, h, n, gop, 3, bins, "cuda", keep_gops=True, msssim=ms)
        out["bins_" + name] = bins
    dec_net, _ = product_model(1)
    dec = str(td / "dec.yuv")
    pmctf_gop.decode_sequence(dec_net, out["bins_with"], dec, "cuda")
    out.update(src=src, dec=dec, w=w, h=h, gop=gop, n=n)
    return out


def test_quality_through_the_sequence_driver(cuda, driven):
    import pmctf_gop
    a, b, n = driven["with"], driven["without"], driven["n"]
    assert "msssim" not in b and b["log"]["frame_msssim"] == [0] * n and b["log"]["ave_all_frame_msssim"] == 0
    ms = a["msssim"]
    assert len(ms) == n and all(type(v) is float and 0.0 < v <= 1.0 for v in ms), ms
    assert a["log"]["frame_msssim"] == ms and json.loads(a["json"])["frame_msssim"] == [round(v, 6) for v in ms]
    assert a["log"]["ave_all_frame_msssim"] == pytest.approx(sum(ms) / n, abs=1e-15)
    assert a["log"]["ave_i_frame_msssim"] == pytest.approx((ms[0] + ms[4]) / 2, abs=1e-15)
    assert a["log"]["ave_p_frame_msssim"] == pytest.approx((sum(ms) - ms[0] - ms[4]) / 6, abs=1e-15)
    assert a["bits"] == b["bits"] and a["bpp_mv"] == b["bpp_mv"] and a["frame_types"] == b["frame_types"]
    for k in ("psnr", "psnr_rgb"):
        d = np.abs(np.array(a[k]) - np.array(b[k])).max()
        print(f"\n{k}: max |HIP quality kernels - torch path| = {d:.3e} dB")
        assert d < PSNR_BAR
    for name in sorted(os.listdir(driven["bins_with"])):         # the same files either way
        pa, pb = os.path.join(driven["bins_with"], name), os.path.join(driven["bins_without"], name)
        if os.path.isdir(pa):
            for f in sorted(os.listdir(pa)):
                assert open(os.path.join(pa, f), "rb").read() == open(os.path.join(pb, f), "rb").read(), (name, f)
    # files -> .yuv -> quality: the same integers into the same deterministic kernels
    sq = pmctf_gop.sequence_quality(driven["src"], driven["dec"], driven["w"], driven["h"], n, "cuda", gop=driven["gop"])
    assert sq["psnr"] == a["psnr"] and sq["psnr_rgb"] == a["psnr_rgb"] and sq["msssim"] == a["msssim"]
    assert sq["frame_types"] == a["frame_types"] and len(sq["lines"]) == n
    assert sq["mean"]["msssim"] == sum(ms) / n
    assert sq["lines"][0].startswith("frame 0, YUV-PSNR: %.4f, RGB-PSNR: %.4f,MS-SSIM: %.4f," % (a["psnr"][0], a["psnr_rgb"][0], ms[0]))
    none = pmctf_gop.sequence_quality(driven["src"], driven["src"], driven["w"], driven["h"], 2, "cuda")
    assert none["msssim"] == [1.0, 1.0] and none["psnr"] == [math.inf] * 2 and none["frame_types"] is None


def test_sequence_quality_tool(cuda, driven, tmp_path):
    import pmctf_gop
    out_json = str(tmp_path / "q.json")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "sequence_quality.py"), driven["src"], driven["dec"], "--width",
           str(driven["w"]), "--height", str(driven["h"]), "--frames", str(driven["n"]), "--json", out_json]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    sq = pmctf_gop.sequence_quality(driven["src"], driven["dec"], driven["w"], driven["h"], driven["n"], "cuda")
    got = json.load(open(out_json))
    for k in ("psnr", "psnr_rgb", "msssim", "psnr_y", "psnr_cb", "psnr_cr"):
        assert got[k] == sq[k], k
    assert got["mean"] == sq["mean"] and [tuple(s) for s in got["sse"]] == sq["sse"]
    lines = r.stdout.splitlines()
    assert [l for l in lines if l.startswith("frame ")] == sq["lines"]
    assert any(l.startswith("average") for l in lines)
    # all frames of the files when --frames is left out
    r2 = subprocess.run(cmd[:8], capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0 and len([l for l in r2.stdout.splitlines() if l.startswith("frame ")]) == driven["n"]


def test_1080p_gop_against_the_reference_and_the_restatement(cuda, tmp_path):
    """One 1080p GOP 8 at q_index 3 with four motion stages, the configuration of the digest the real reference left:
    per-frame YUV- and Y-PSNR of gop_quality against the reference's own figures, MS-SSIM against the float64 restatement
    on the same pictures."""
    import pmctf_gop
    g = np.load(os.path.join(ROOT, "tests", "golden", "reference_1920x1080_gop8_me4_digest.npz"))
    w, h, gop = 1920, 1080, 8
    net, _ = product_model(4)
    net.engine().keep_streams = True
    fr = frames(w, h, gop, device="cuda")
    enc = pmctf_gop.encode_gop(net, fr, h, w, 3, str(tmp_path))
    assert enc["bits"] == g["gop.bits"].tolist()
    rec = pmctf_gop.decode_gop(net, enc["frames_coded"])
    orig = [(y[:, :, :h, :w].contiguous(), c[:, :, :h // 2, :w // 2].contiguous()) for y, c in fr]
    qs = pmctf_gop.gop_quality(rec, orig, h, w)
    for k, ref in (("yuv", g["gop.psnr_yuv"]), ("y", g["gop.psnr_y"])):
        err = np.abs(np.array([q[k] for q in qs]) - ref)
        print(f"\n1080p GOP 8 {k}-PSNR: per-frame |gop_quality - reference's| = {err.tolist()}")
        assert err.max() < PSNR_BAR
    for i, q in enumerate(qs):
        t = (rec[i][0].cpu(), rec[i][1].cpu(), orig[i][0].cpu(), orig[i][1].cpu())
        sse, rgb_rec, rgb_org = qr.integer_sse(*t, h, w)
        assert q["sse"] == sse
        r64, m64 = qr.ms_ssim(rgb_rec, rgb_org, dtype=torch.float64)
        r32, _ = qr.ms_ssim(rgb_rec, rgb_org, dtype=torch.float32)
        assert all(m > 0 for scale in m64 for ch in scale for m in ch)
        err = abs(q["msssim"] - r64)
        print(f"msssim-accuracy 1080p GOP 8 frame {i}: r64 {r64:.12f} e32 {abs(r32 - r64):.3e} hip {q['msssim']:.12f} "
              f"|hip-r64| {err:.3e} bound {_bound(r64, r32):.3e}")
        assert err <= _bound(r64, r32)
