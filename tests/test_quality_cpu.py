"""Quality metrics without a GPU: the MS-SSIM restatement the GPU tests are measured against (tests/quality_restatement.py)
checked for the properties its definition gives, the argument checks of the new C entry points (they refuse before any
GPU call), and the host-side pieces of the public interface."""
import inspect

import numpy as np
import pytest
import torch

import quality_restatement as qr


def _pictures(h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.round(torch.rand((3, h, w), generator=g) * 255.0)
    y = torch.round((x + 20.0 * torch.randn((3, h, w), generator=g)).clamp(0, 255))
    return x, y


def test_restatement_identical_pictures_give_exactly_one():
    x, _ = _pictures(200, 232)
    for dtype in (torch.float64, torch.float32):
        v, means = qr.ms_ssim(x, x.clone(), dtype=dtype)
        if dtype == torch.float64:
            assert v == 1.0
            assert all(m == (1.0, 1.0) for scale in means for m in scale)
        else:
            assert abs(v - 1.0) < 1e-5           # E[x^2] - mu^2 in float32: the package's own rounding


def test_restatement_scale_sizes():
    assert qr.scale_sizes(1080, 1920) == [(1080, 1920), (540, 960), (270, 480), (135, 240), (68, 120)]
    x = torch.zeros((1, 1, 135, 240))
    assert tuple(qr.pool(x).shape[-2:]) == (68, 120)
    # the padding is counted in the average: a row of ones next to the zero padding averages to 0.5
    ones = torch.ones((1, 1, 135, 240))
    p = qr.pool(ones)
    assert float(p[0, 0, 0, 5]) == 0.5 and float(p[0, 0, 1, 5]) == 1.0 and float(p[0, 0, 67, 5]) == 1.0


def test_restatement_refuses_pictures_too_small_for_five_scales():
    x, y = _pictures(160, 200)
    with pytest.raises(ValueError):
        qr.ms_ssim(x, y)
    x, y = _pictures(162, 200)
    v, means = qr.ms_ssim(x, y)
    assert 0.0 < v < 1.0 and len(means) == 5 and len(means[0]) == 3


def test_restatement_window_and_ordering():
    g = qr.gauss_window(torch.float64)
    assert g.numel() == 11 and abs(float(g.sum()) - 1.0) < 1e-15 and torch.equal(g, g.flip(0))
    assert abs(float(g[5] / g[4]) - np.exp(1.0 / (2 * 1.5 ** 2))) < 1e-12
    x, y = _pictures(192, 208, seed=3)
    near = torch.round((x + 0.25 * (y - x)))
    a, _ = qr.ms_ssim(near, x)
    b, _ = qr.ms_ssim(y, x)
    assert b < a < 1.0                           # less distortion scores higher
    assert qr.ms_ssim(x, y)[0] == pytest.approx(b, abs=1e-12)          # symmetric in its arguments


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    import ctypes as C
    from pMCTF.hip import lib
    L = lib.hip()
    assert {"pmctf_frame_quality_f32", "pmctf_msssim_scratch_floats"} <= set(lib.exported_symbols())
    one = C.c_void_p(4096)                       # non-null, 8-byte aligned, never dereferenced: the checks come first
    fq = L.pmctf_frame_quality_f32
    assert fq(None, None, None, None, 256, 256, 192, 256, 1, None, None, None) == -1
    for k in range(6):                           # each pointer on its own
        ptrs = [one] * 6
        ptrs[k] = None
        assert fq(ptrs[0], ptrs[1], ptrs[2], ptrs[3], 256, 256, 192, 256, 1, ptrs[4], ptrs[5], None) == -1, k
    bad = [(256, 256, 191, 256), (256, 256, 192, 255), (256, 256, 0, 256), (256, 256, 192, -2), (128, 256, 192, 256),
           (256, 128, 192, 256), (255, 256, 192, 256)]
    for ms in (0, 1):
        for Hp, Wp, h, w in bad:
            assert fq(one, one, one, one, Hp, Wp, h, w, ms, one, one, None) == -1, (Hp, Wp, h, w, ms)
    assert fq(one, one, one, one, 256, 256, 160, 256, 1, one, one, None) == -1          # five scales need more than 160
    assert fq(one, one, one, one, 256, 256, 192, 160, 1, one, one, None) == -1
    assert fq(one, one, one, one, 256, 256, 192, 256, 1, C.c_void_p(4100), one, None) == -1      # scratch holds doubles
    for h, w in ((0, 16), (16, 0), (-2, 16), (15, 16), (16, 15)):
        assert L.pmctf_msssim_scratch_floats(h, w) == -1


def test_scratch_query_is_positive_and_monotone():
    from pMCTF.hip import lib, ops
    L = lib.hip()
    sizes = [(2, 2), (100, 132), (162, 162), (192, 256), (360, 636), (1080, 1920), (2160, 3840)]
    got = [L.pmctf_msssim_scratch_floats(h, w) for h, w in sizes]
    assert all(g > 0 for g in got) and got == sorted(got) and len(set(got)) == len(got)
    assert got[0] >= ops.QUALITY_FRONT_FLOATS
    for (h, w), g in zip(sizes, got):
        # at least the two RGB pictures of every scale
        assert g >= 6 * sum(a * b for a, b in qr.scale_sizes(h, w))
        assert L.pmctf_msssim_scratch_floats(h + 2, w) >= g and L.pmctf_msssim_scratch_floats(h, w + 2) >= g


def test_msssim_from_means_is_the_restatements_product():
    from pMCTF.hip import ops
    assert ops.MSSSIM_WEIGHTS == qr.WEIGHTS and ops.MSSSIM_MIN_SIDE == qr.MIN_SIDE
    x, y = _pictures(176, 240, seed=5)
    v, means = qr.ms_ssim(x, y)
    assert ops.msssim_from_means(means) == pytest.approx(v, abs=1e-14)
    means[2][1] = (-0.25, 0.5)                   # a relu that fires zeroes that channel
    one = ops.msssim_from_means(means)
    assert 0.0 < one < v


def test_public_interface_without_a_gpu(tmp_path):
    import pmctf_gop
    sig = inspect.signature(pmctf_gop.encode_sequence)
    assert list(sig.parameters)[-2:] == ["keep_gops", "msssim"] and sig.parameters["msssim"].default is False
    assert list(inspect.signature(pmctf_gop.gop_quality).parameters) == ["frames_rec", "frames_orig", "pic_height",
                                                                         "pic_width", "msssim"]
    assert list(inspect.signature(pmctf_gop.sequence_quality).parameters)[:7] == ["src_yuv", "rec_yuv", "width", "height",
                                                                                  "frame_num", "device", "gop"]
    y, c = torch.zeros((1, 1, 192, 256)), torch.zeros((2, 1, 96, 128))
    with pytest.raises(RuntimeError, match="GPU"):          # no CPU fallback
        pmctf_gop.gop_quality([(y, c, None)], [(y, c)], 192, 256)
    with pytest.raises(RuntimeError, match="GPU"):
        pmctf_gop.sequence_quality("a.yuv", "b.yuv", 256, 192, 1, "cpu")
    q = {"yuv": 38.12346, "rgb": 36.5, "msssim": 0.98765, "y": 39.0, "cb": 41.25, "cr": 42.0}
    line = pmctf_gop.quality_line(3, q)
    assert line.startswith("frame 3, YUV-PSNR: 38.1235, RGB-PSNR: 36.5000,MS-SSIM: 0.9877, Y-PSNR: 39.0000,")
    assert "Cb-PSNR: 41.2500, Cr-PSNR: 42.0000" in line
    assert "bpps: 0.125, " in pmctf_gop.quality_line(3, q, bpp=0.125, seconds=1.5)


def test_noise_strengths_of_the_gpu_cases_keep_every_mean_positive():
    """condition of the MS-SSIM accuracy test (tests/test_gpu_quality.py): with the strongest noise used there no relu
    fires in the float64 restatement, on the smallest of the cases (the others are checked where they run)"""
    rec_y, rec_c, org_y, org_c = qr.quality_case(256, 256, 192, 256, max(qr.NOISE))
    _, rgb_rec, rgb_org = qr.integer_sse(rec_y, rec_c, org_y, org_c, 192, 256)
    v, means = qr.ms_ssim(rgb_rec, rgb_org)
    assert all(m > 0 for scale in means for ch in scale for m in ch) and 0 < v < 1
