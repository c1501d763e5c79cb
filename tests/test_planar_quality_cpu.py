"""Per-plane quality without a GPU: the five entries of include/pmctf_quality.h are declared, exported and
refuse every bad argument before any launch (the pointers are never dereferenced); include/pmctf_hip.h and lib._SIGS keep
their sets of names; the restatement the GPU tests are measured against has the properties its definition gives; and what
pmctf_quality.compare_files and the tools refuse, they refuse without a GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import planar_quality_restatement as pq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pmctf_planar_sse_u8", "pmctf_planar_sse_u16", "pmctf_plane_msssim_scratch_floats", "pmctf_plane_msssim_u8",
           "pmctf_plane_msssim_u16")


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(pmctf_\w+)\s*\(", text))


def test_entries_are_declared_in_their_own_header_and_exported():
    import pmctf_quality
    from pMCTF.hip import lib
    assert _declared("pmctf_quality.h") == set(ENTRIES) == set(pmctf_quality.SIGS)
    H = C.CDLL(lib.HIP_SO)
    for s in ENTRIES:
        assert hasattr(H, s), f"libpmctf_hip.so does not export {s}"
    L = pmctf_quality.library()
    assert L is lib.hip() and L.pmctf_plane_msssim_scratch_floats.restype is C.c_int64
    src = open(os.path.join(ROOT, "learned-pmctf_amd", "csrc", "quality_planar.hip")).read()
    for s in ENTRIES:
        assert re.search(r'extern "C" (int|int64_t) ' + s + r"\(", src), s


def test_the_pinned_header_and_signature_table_keep_their_names():
    from pMCTF.hip import lib
    hip_h = _declared("pmctf_hip.h")
    assert not hip_h & set(ENTRIES) and not set(lib.exported_symbols()) & set(ENTRIES)
    assert hip_h == set(lib.exported_symbols())
    assert len(hip_h) == 79                      # 62 stream takers + 17 exempt (tests/stream_order.py)


def test_sse_entries_refuse_bad_arguments_before_any_launch():
    import pmctf_quality
    L = pmctf_quality.library()
    one, odd = C.c_void_p(4096), C.c_void_p(4097)
    u8 = lambda a, b, h, w, fmt, s: L.pmctf_planar_sse_u8(a, b, h, w, fmt, s, None)
    u16 = lambda a, b, h, w, fmt, s, depth=10: L.pmctf_planar_sse_u16(a, b, h, w, fmt, depth, s, None)
    for fn in (u8, u16):
        assert fn(None, None, 6, 10, 420, None) == -1
        for k in range(3):                       # each pointer on its own
            p = [one] * 3
            p[k] = None
            assert fn(p[0], p[1], 6, 10, 420, p[2]) == -1, k
        for fmt in (0, 400, 411, 421, 440, -420, 4200):
            assert fn(one, one, 6, 10, fmt, one) == -1, fmt
        for h, w in ((5, 10), (6, 9), (0, 10), (6, 0), (-2, 10), (6, -2), (16386, 10), (6, 16386)):
            assert fn(one, one, h, w, 444, one) == -1, (h, w)
        assert fn(one, one, 6, 10, 420, C.c_void_p(4100)) == -1          # the sums are 64-bit words
    assert u16(odd, one, 6, 10, 420, one) == -1 and u16(one, odd, 6, 10, 420, one) == -1
    for depth in (8, 0, -1, 17, 32):
        assert u16(one, one, 6, 10, 420, one, depth) == -1, depth


def test_msssim_entries_refuse_bad_arguments_before_any_launch():
    import pmctf_quality
    L = pmctf_quality.library()
    one, odd = C.c_void_p(4096), C.c_void_p(4097)
    u8 = lambda a, b, h, w, s, o: L.pmctf_plane_msssim_u8(a, b, h, w, s, o, None)
    u16 = lambda a, b, h, w, s, o, depth=10: L.pmctf_plane_msssim_u16(a, b, h, w, depth, s, o, None)
    for fn in (u8, u16):
        assert fn(None, None, 192, 256, None, None) == -1
        for k in range(4):
            p = [one] * 4
            p[k] = None
            assert fn(p[0], p[1], 192, 256, p[2], p[3]) == -1, k
        for h, w in ((160, 256), (192, 160), (161, 100), (0, 256), (-161, 256), (192, -1), (16385, 256), (192, 16385)):
            assert fn(one, one, h, w, one, one) == -1, (h, w)
        assert fn(one, one, 192, 256, C.c_void_p(4100), one) == -1       # scratch holds doubles
        assert fn(one, one, 192, 256, one, C.c_void_p(4100)) == -1
    assert u16(odd, one, 192, 256, one, one) == -1 and u16(one, odd, 192, 256, one, one) == -1
    for depth in (8, 0, -1, 17):
        assert u16(one, one, 192, 256, one, one, depth) == -1, depth
    for h, w in ((160, 256), (256, 160), (0, 256), (16385, 161), (-5, 161)):
        assert L.pmctf_plane_msssim_scratch_floats(h, w) == -1, (h, w)


def test_scratch_query_is_positive_and_monotone():
    import quality_restatement as qr
    import pmctf_quality
    L = pmctf_quality.library()
    sizes = [(161, 161), (162, 170), (192, 256), (193, 323), (361, 637), (1080, 1920), (2160, 3840), (16384, 16384)]
    got = [L.pmctf_plane_msssim_scratch_floats(h, w) for h, w in sizes]
    assert all(g > 0 for g in got) and got == sorted(got) and len(set(got)) == len(got)
    for (h, w), g in zip(sizes, got):
        # at least both planes of the four pooled scales (scale 0 is read where it lies)
        assert g >= 2 * sum(a * b for a, b in qr.scale_sizes(h, w)[1:])
        assert g < 2 * h * w                     # and less than a float copy of the two planes
        if max(h, w) < 16384:
            assert L.pmctf_plane_msssim_scratch_floats(h + 1, w) >= g and L.pmctf_plane_msssim_scratch_floats(h, w + 1) >= g


def test_restatement_identical_planes_give_one_and_the_scaling_is_exact():
    for depth in (8, 10, 12, 16):
        a, b = pq.plane_pair(162, 170, depth, 0.02, seed=depth)
        v, means = pq.ms_ssim(a, a.copy(), depth)
        assert v == 1.0 and all(m == (1.0, 1.0) for m in means)
        v, means = pq.ms_ssim(a, b, depth)
        assert 0.0 < v < 1.0 and len(means) == 5 and all(0.0 < m[1] <= m[0] < 1.0 for m in means)
        # both planes and the data range times 2^-(b - 8): every float64 operation scales by a power of two, or not at all
        vs, ms = pq.ms_ssim(a, b, depth, scale=2.0 ** -(depth - 8))
        assert vs == v and ms == means, depth
    # an odd plane goes 161 -> 81 -> 41 -> 21 -> 11
    import quality_restatement as qr
    assert qr.scale_sizes(161, 323) == [(161, 323), (81, 162), (41, 81), (21, 41), (11, 21)]


def test_restatement_sums_psnr_and_the_product():
    import pmctf_quality
    assert pq.SUBSAMPLING == __import__("pmctf_chroma").SUBSAMPLING
    assert pmctf_quality.MSSSIM_WEIGHTS == __import__("quality_restatement").WEIGHTS
    for fmt, n_c in (("420", 15), ("422", 30), ("444", 60)):
        assert pq.frame_samples(6, 10, fmt) == 60 + 2 * n_c == __import__("pmctf_chroma").frame_samples(10, 6, fmt)
        assert pmctf_quality.plane_shapes(6, 10, fmt) == pq.plane_shapes(6, 10, fmt)
    a = np.zeros(pq.frame_samples(64, 64, "444"), np.uint16)
    b = np.full_like(a, 65535)
    assert pq.sse(a, b, 64, 64, "444") == (4096 * 65535 ** 2,) * 3 and 4096 * 65535 ** 2 > 2 ** 32
    assert pq.sse(a, a, 64, 64, "444") == (0, 0, 0)
    assert pq.psnr(0, 10, 10) == float("inf") and pq.psnr(1023 ** 2 * 10, 10, 10) == 0.0
    assert pmctf_quality.psnr_from_sse(777, 60, 10) == pq.psnr(777, 60, 10)
    assert pq.yuv(40.0, 32.0, 24.0) == 37.0 == pmctf_quality.yuv_psnr(40.0, 32.0, 24.0)          # 6:1:1
    x, y = pq.plane_pair(176, 164, 10, 0.05)
    v, means = pq.ms_ssim(x, y, 10)
    assert pmctf_quality.msssim_from_means(means) == pytest.approx(v, abs=1e-14)
    means[1] = (-0.25, 0.5)                      # a relu that fires zeroes the product
    assert pmctf_quality.msssim_from_means(means) == 0.0


def test_noise_strengths_of_the_gpu_cases_keep_every_mean_positive_and_the_clamp_live():
    h, w = pq.MSSSIM_SIZES[0]
    for depth in pq.DEPTHS:
        a, b = pq.plane_pair(h, w, depth, max(pq.NOISE))
        top = (1 << depth) - 1
        assert (b == 0).any() and (b == top).any() and a.min() < 0.12 * top and a.max() > 0.88 * top
        v, means = pq.ms_ssim(a, b, depth)
        assert all(m > 0 for pair in means for m in pair) and 0 < v < 1


# ------------------------------------------------------------------------------------------------ the public interface
def _y4m(path, w, h, fmt, depth, n, seed=0):
    import pmctf_chroma
    with open(path, "wb") as f:
        f.write(pmctf_chroma.y4m_header(w, h, (25, 1), fmt, depth))
        for k in range(n):
            f.write(b"FRAME\n")
            f.write(pq.random_frame(h, w, fmt, depth, seed + k).astype("<u2" if depth > 8 else np.uint8).tobytes())
    return str(path)


def test_frame_quality_planar_checks_its_arguments_and_has_no_cpu_fallback():
    import pmctf_quality
    f8 = torch.zeros(pq.frame_samples(6, 10, "420"), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        pmctf_quality.frame_quality_planar(f8, f8, 6, 10)
    with pytest.raises(RuntimeError, match="GPU"):
        pmctf_quality.planar_sse(f8, f8, 6, 10)
    p = torch.zeros((192, 256), dtype=torch.uint16)
    with pytest.raises(RuntimeError, match="GPU"):
        pmctf_quality.plane_msssim(p, p, 10)
    with pytest.raises(ValueError, match="160"):
        pmctf_quality.plane_msssim(p[:160], p[:160], 10)
    with pytest.raises(ValueError):
        pmctf_quality.frame_quality_planar(f8, f8, 6, 10, "422")            # another number of samples
    with pytest.raises(ValueError):
        pmctf_quality.frame_quality_planar(f8, f8, 6, 10, bitdepth=10)      # bytes at 10 bits
    with pytest.raises(ValueError):
        pmctf_quality.frame_quality_planar(f8, f8, 6, 10, "400")
    with pytest.raises(ValueError):
        pmctf_quality.frame_quality_planar(f8, f8, 5, 12)
    with pytest.raises(ValueError):
        pmctf_quality.frame_quality_planar(f8, f8, 6, 10, bitdepth=17)


def test_compare_files_refuses_without_a_gpu(tmp_path):
    import pmctf_quality
    a = _y4m(tmp_path / "a.y4m", 10, 6, "444", 10, 2)
    same = _y4m(tmp_path / "same.y4m", 10, 6, "444", 10, 3, seed=5)
    for name, args in (("size.y4m", (12, 6, "444", 10)), ("format.y4m", (10, 6, "422", 10)), ("depth.y4m", (10, 6, "444", 12))):
        other = _y4m(tmp_path / name, *args, 2)
        with pytest.raises(ValueError) as e:
            pmctf_quality.compare_files(a, other, "cpu")
        assert "a.y4m" in str(e.value) and name in str(e.value), str(e.value)     # names both
    raw = str(tmp_path / "raw.yuv")
    pq.random_frame(6, 10, "444", 10, 3).astype("<u2").tofile(raw)
    with pytest.raises(ValueError, match="width and height"):
        pmctf_quality.compare_files(a, raw, "cpu")                               # a raw file needs its size
    with pytest.raises(ValueError, match="raw.yuv"):
        pmctf_quality.compare_files(a, raw, "cpu", width=10, height=6)           # ... and is 8-bit 4:2:0 by default
    with pytest.raises(ValueError, match="shorter than 2"):
        pmctf_quality.compare_files(a, raw, "cpu", width=10, height=6, chroma_format="444", bitdepth=10, frame_num=2)
    with pytest.raises(ValueError, match="shorter than 3"):
        pmctf_quality.compare_files(same, a, "cpu", frame_num=3)
    with pytest.raises(ValueError, match="multiple of gop"):
        pmctf_quality.compare_files(a, same, "cpu", gop=4)
    empty = str(tmp_path / "empty.yuv")
    open(empty, "wb").close()
    with pytest.raises(ValueError, match="no whole picture"):
        pmctf_quality.compare_files(empty, empty, "cpu", width=10, height=6)
    with pytest.raises(RuntimeError, match="GPU"):                               # everything agrees: only the GPU is missing
        pmctf_quality.compare_files(a, same, "cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        pmctf_quality.compare_files(a, raw, "cpu", width=10, height=6, chroma_format="444", bitdepth=10)


def _tool(name, *args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", name), *args], capture_output=True, text=True,
                          timeout=300)


def test_the_tools_refuse_without_a_gpu(tmp_path):
    a = _y4m(tmp_path / "a.y4m", 10, 6, "444", 10, 2)
    b = _y4m(tmp_path / "b.y4m", 10, 6, "420", 10, 2)
    r = _tool("compare_sequences.py", a, b)
    assert r.returncode == 2 and "a.y4m" in r.stderr and "b.y4m" in r.stderr and "agree" in r.stderr
    r = _tool("compare_sequences.py", a, str(tmp_path / "missing.y4m"))
    assert r.returncode == 2 and "no such file" in r.stderr
    r = _tool("compare_sequences.py", a, a, "--bitdepth", "7")
    assert r.returncode == 2 and "bitdepth" in r.stderr
    # tools/decode_sequence.py --compare: refused before the folder is looked at
    dec = ("decode_sequence.py", "--synth-seed", "0", "--compare", a)
    r = _tool(*dec, str(tmp_path), "--png", str(tmp_path / "png"))
    assert r.returncode == 2 and "--compare: needs an OUT file" in r.stderr
    out = str(tmp_path / "out.y4m")
    for flag in (("--output-layout", "nv12"), ("--spatial-level", "1"), ("--temporal-level", "1"), ("--temporal-level", "0")):
        r = _tool(*dec, *flag, str(tmp_path), out)
        assert r.returncode == 2 and f"--compare: cannot be combined with {flag[0]}" in r.stderr, (flag, r.stderr)
    r = _tool("decode_sequence.py", "--synth-seed", "0", "--compare", str(tmp_path / "missing.y4m"), str(tmp_path), out)
    assert r.returncode == 2 and "--compare: no such file" in r.stderr
    assert not os.path.exists(out)
