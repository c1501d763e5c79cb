"""The device's scalar functions (learned-pmctf_amd/csrc/pm_device_math.h and the generated headers it includes) without a
GPU: compiled for the host and compared with the oracle on the stratified set S of math_sweep.py; the shared headers are
one text in both trees; what pm_glibc_expf is against this machine's libm; and the inventory of direct kernel tests.
The compiler-dependent half — the same functions as the GPU compiler builds them, on all 2^32 inputs — is
test_gpu_math_sweep.py; tools/math_sweep.py --host runs all 2^32 inputs through the host build."""
import glob
import os
import re

import numpy as np
import pytest

import math_sweep as ms

ROOT = ms.ROOT


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ms.HostBuild(str(tmp_path_factory.mktemp("host_probe")))


def test_the_set_s_is_what_it_says():
    pieces = list(ms.stratified())
    assert [p[1].dtype for p in pieces] == [np.uint32] * 6
    sp = ms.special_patterns()
    assert pieces[0][1].size == 512 * 3 * 4096 + sp.size and all(p[1].size == 1 << 23 for p in pieces[1:])
    strata = pieces[0][1][:512 * 3 * 4096].reshape(512, 3 * 4096)
    assert np.array_equal(strata >> 23, np.repeat(np.arange(512, dtype=np.uint32)[:, None], 3 * 4096, 1))
    assert np.unique(strata).size == strata.size - 512 * 4            # two evenly spaced mantissas fall into each end group
    for v in (0.0, -0.0, np.inf, -np.inf, 0.046875, 9.0, 87.0, -87.0, 88.0, 2.0 ** 100, 2.0 ** -100, 2.0 ** 127 * 1.25,
              1e-45, 1.1754942e-38, 1.1754944e-38, 3.4028235e38):
        assert np.array([v], np.float32).view(np.uint32)[0] in sp, v
    assert set(ms.EXPF_DEVIATIONS) <= set(sp.tolist())
    assert [int(p[1][0]) for p in pieces[1:]] == list(ms.FULL_BINADES)
    assert sum(p[1].size for p in pieces) > 48_000_000
    assert sum(n for _, n in ms.chunks()) == 1 << 32 and len(list(ms.chunks())) == 64


def test_host_compiled_device_header_equals_the_oracle_on_s(host):
    """every function of the probe's table, device text compiled by the host compiler, against the oracle map that
    specifies it: bit for bit on every pattern of S, NaN payloads included (the full sweep holds with none exempt)"""
    for label, bits in ms.stratified():
        x = bits.view(np.float32)
        want = {}
        for name, _, spec in ms.FUNCTIONS:
            if spec not in want:
                want[spec] = spec(x).view(np.uint32)
            got = host.probe(name, bits).view(np.uint32)
            count, first, exempt = ms.compare(got, want[spec])
            assert count == 0, ms.describe(f"{name} on {label}", bits, got, want[spec], count, first)
            assert exempt == 0, f"{name} on {label}: {exempt} NaN results differ in their payload"


def test_host_build_sees_a_changed_table_word(tmp_path):
    """the comparison is live: a copy of the sources with one low bit of one tanh table word flipped, and one with one
    log threshold moved by one, no longer equal the oracle, and the first affected input is named"""
    import shutil
    for header, macro, fn in (("pm_tanh_tables.h", "PM_TANH_TABLE_BY_INTERVAL", "tanh"),
                              ("pm_log_tables.h", "PM_LOG_STEP_M_PADDED", "log")):
        src = tmp_path / fn
        shutil.copytree(ms.CSRC, src, ignore=shutil.ignore_patterns("*.hip", "*.cpp"))
        text = (src / header).read_text()
        at = text.index(macro)
        words = list(re.finditer(r"0x[0-9a-fA-F]{8}", text[at:]))
        # T_hi of interval 16; the last threshold: the only one of five tried (1, 5, 17, 25, 32) whose move by one changes
        # any result at all (log(0x3f7c1280)) — at the others both reciprocals give the same rounded logarithm.
        # The indices follow the word layout the generators write (twelve words per tanh interval, T_hi second; 33
        # thresholds first in the padded list): revisit them when tools/mkl_tanh_tables.py or mkl_log_tables.py change it
        w = words[16 * 12 + 1 if fn == "tanh" else 32]
        changed = f"0x{int(w.group(), 16) ^ 1:08x}" if fn == "tanh" else f"0x{int(w.group(), 16) + 1:08x}"
        (src / header).write_text(text[:at + w.start()] + changed + text[at + w.end():])
        mutant = ms.HostBuild(str(tmp_path / (fn + "_build")), csrc=str(src))
        bad = 0
        for label, bits in ms.stratified():
            got, want = mutant.probe(fn, bits).view(np.uint32), ms.SPEC[fn](bits.view(np.float32)).view(np.uint32)
            count, first, _ = ms.compare(got, want)
            if count:
                assert "first at input 0x" in ms.describe(fn, bits, got, want, count, first)
            bad += count
        assert bad > 0, f"{header}: a changed word of {macro} went unnoticed on S"


@pytest.mark.parametrize("header", ["pm_tanh_tables.h", "pm_log_tables.h", "pm_glibc_expf.h"])
def test_table_and_glibc_headers_are_one_text(header):
    """(pm_sleef_f32.h: test_oracle_math.py)"""
    a = open(os.path.join(ROOT, "oracle", "c", header), "rb").read()
    b = open(os.path.join(ms.CSRC, header), "rb").read()
    assert a == b, f"oracle/c/{header} and learned-pmctf_amd/csrc/{header} differ"


def test_glibc_expf_and_the_scalar_sigmoid_are_libm_s_on_s():
    """pm_glibc_expf equals this machine's libm expf on S with no deviation — S holds 0x4202422f and 0xc27c65d9, the two
    inputs of 2^32 that were one ulp off until the remainder's multiply-add was contracted as glibc's FMA build does
    (tools/glibc_expf_header.py --all checks all 2^32) — and pm_aten_sigmoidf_scalar(x) equals 1 / (1 + expf(-x)), what
    ATen's scalar tail computes."""
    from pmctf_oracle import clib
    if not ms.libm_is_fma_build():
        pytest.skip("this machine's libm expf is not the FMA build the transcription follows "
                    f"(expf({ms.LIBM_FMA_PROBE[0]:#010x}) != {ms.LIBM_FMA_PROBE[1]:#010x})")
    one = np.float32(1)
    for label, bits in ms.stratified():
        x = bits.view(np.float32)
        with np.errstate(all="ignore"):
            want = (one / (one + clib.libm_exp(-x))).view(np.uint32)
        got = clib.sigmoid_scalar(x).view(np.uint32)
        count, first, exempt = ms.compare(got, want)
        assert count == 0 and exempt == 0, ms.describe(f"scalar sigmoid vs libm on {label}", bits, got, want, count, first)
        got, want = clib.glibc_exp(x).view(np.uint32), clib.libm_exp(x).view(np.uint32)
        count, first, exempt = ms.compare(got, want)
        assert count == 0 and exempt == 0, ms.describe(f"pm_glibc_expf vs libm on {label}", bits, got, want, count, first)
    x = np.array(ms.EXPF_DEVIATIONS, np.uint32).view(np.float32)
    assert clib.glibc_exp(x).view(np.uint32).tolist() == [0x56fc9f1c, 0x11fa2993]


# entry point -> the pMCTF.hip.ops wrapper a direct GPU test calls it through.  The long-index forms of the elementwise
# kernels (totals >= 2^31 elements) are NOT covered: they need operands of 8.6 GB each, and the largest tensor of the
# path has 566 MB.  Every grid-stride kernel is run past its grid cap (16384 x 256 work items; 8192 x 256 for
# conv_smallcin_kernel) by test_gpu_kernels.py::test_grid_stride_kernels_past_the_grid_cap and the tests beside it.
WRAPPERS = {
    "pmctf_ew_f32": "ew", "pmctf_spynet_pack8_f32": "spynet_pack8", "pmctf_lift_skip3_f32": "lift_skip3",
    "pmctf_nearest_up2_nhwc_f32": "nearest_up2", "pmctf_pixel_shuffle2_nhwc_f32": "pixel_shuffle2",
    "pmctf_ffn3_mix_f32": "ffn3_mix", "pmctf_lstm_gates_f32": "lstm_gates", "pmctf_lstm_gates_aten_f32": "lstm_gates",
    "pmctf_planes_to_u8": "planes_to_u8",                                        # csrc/picture_ops.hip
    "pmctf_conv2d_smallcin_f32": "Conv2d", "pmctf_conv3x3_cin1_dual_f32": "conv3x3_cin1_dual",
    "pmctf_conv2d_fewcout_supported": "Conv2d", "pmctf_conv2d_fewcout_f32": "Conv2d",
    "pmctf_valu_conv_last_launch": "valu_conv_last_launch", "pmctf_ew_last_launch": "ew_last_launch",
    "pmctf_dwconv2d_nhwc_f32": "DepthwiseConv2d", "pmctf_flow_warp_f32": "flow_warp", "pmctf_avgpool2_f32": "avgpool2",
    "pmctf_bilinear_up_f32": "bilinear_up2", "pmctf_bilinear_down_f32": "bilinear_down2",
    "pmctf_bilinear_up2_f32": "bilinear_up2", "pmctf_bilinear_down2_f32": "bilinear_down2",
}


def test_every_layout_and_network_kernel_has_a_direct_gpu_test():
    """every other export of ew_ops.hip (OTHER_EXPORTS of test_entropy_restatement_cpu.py) and every export of
    basic_ops.hip is reached through its ops wrapper, by name, in some tests/test_gpu_*.py; an export added to either file
    shows up here until it is given a test"""
    from test_entropy_restatement_cpu import OTHER_EXPORTS
    basic = set(re.findall(r'extern "C" \w+ (pmctf_\w+)\(', open(os.path.join(ms.CSRC, "basic_ops.hip")).read()))
    reached = OTHER_EXPORTS["ew_ops"] | basic | {"pmctf_planes_to_u8"}
    assert set(WRAPPERS) == reached, set(WRAPPERS) ^ reached
    ops_text = open(os.path.join(ROOT, "learned-pmctf_amd", "pMCTF", "hip", "ops.py")).read()
    texts = {f: open(f).read() for f in sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py")))}
    for entry, wrapper in WRAPPERS.items():
        assert re.search(rf"^(def|class) {wrapper}\b", ops_text, re.M), f"pMCTF.hip.ops has no {wrapper}"
        assert any(re.search(rf"\bops\.{wrapper}\(", t) for t in texts.values()), \
            f"no tests/test_gpu_*.py calls ops.{wrapper} ({entry})"
    kernels = texts[os.path.join(ROOT, "tests", "test_gpu_kernels.py")]
    for wrapper in ("spynet_pack8", "lift_skip3", "ffn3_mix", "flow_warp", "avgpool2", "lstm_gates", "nearest_up2",
                    "pixel_shuffle2", "DepthwiseConv2d", "conv3x3_cin1_dual", "bilinear_up2", "bilinear_down2"):
        assert re.search(rf"\bops\.{wrapper}\(", kernels), f"tests/test_gpu_kernels.py never calls ops.{wrapper}"
    probe = open(os.path.join(ROOT, "tests", "test_gpu_math_sweep.py")).read()
    assert re.search(r"\bops\.math_probe\(", probe)
