"""Per-plane quality on the GPU (csrc/quality_planar.hip through pmctf_quality).

Yardsticks (tests/planar_quality_restatement.py): numpy int64 for the error sums, which the kernels must EQUAL, at every
format, depth and alignment, and the existing 4:2:0 paths (ops.frame_quality at 8 bits, ops.frame_sse_hbd above) on the same
integer pictures; the float64 restatement of MS-SSIM on the CPU with one channel at the data range 2^b - 1, the float32 run
of the same code giving the scale of the allowed error, the rule of DESIGN 5e:
|hip - r64| <= max(2 * |r32 - r64|, 16 * 2^-24), for the result and for each of the ten map means.  The entries' stream
order is held by the instrument of tests/stream_order.py, one row per launch path."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import planar_quality_restatement as pq
import stream_order as so
from helpers import product_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
_refs = {}


def _np_dtype(depth):
    return np.uint8 if depth == 8 else np.uint16


def _placed(frame, off, dev):
    """the picture inside a byte buffer with guard bands, its first byte `off` bytes past a multiple of 4 -> the tensor
    view of the picture (the buffer lives as long as the view)"""
    raw = np.ascontiguousarray(frame).view(np.uint8)
    buf = torch.full((2 * GUARD + 4 + raw.size,), 0xA5, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 4 == 0
    view = buf[GUARD + off:GUARD + off + raw.size]
    view.copy_(torch.from_numpy(raw))
    t = view if frame.dtype == np.uint8 else view.view(torch.uint16)
    assert t.data_ptr() % 4 == off and t.numel() == frame.size
    return t


@pytest.mark.parametrize("depth", pq.DEPTHS)
def test_error_sums_equal_int64_at_every_format_size_and_alignment(cuda, depth):
    import pmctf_quality
    offsets = (0, 1, 2, 3) if depth == 8 else (0, 2)
    for fmt in ("420", "422", "444"):
        for h, w in pq.SSE_SIZES:
            a = pq.random_frame(h, w, fmt, depth, seed=h + depth)
            b = pq.random_frame(h, w, fmt, depth, seed=h + depth + 1)
            want = pq.sse(a, b, h, w, fmt)
            for oa in offsets:
                ob = offsets[(offsets.index(oa) + 1) % len(offsets)]         # the two pictures at different alignments
                ta, tb = _placed(a, oa, cuda), _placed(b, ob, cuda)
                got = pmctf_quality.planar_sse(ta, tb, h, w, fmt, depth)
                assert got == want and all(type(v) is int for v in got), (fmt, h, w, oa, ob, got, want)
            q = pmctf_quality.frame_quality_planar(_placed(a, offsets[-1], cuda), _placed(b, 0, cuda), h, w, fmt, depth)
            assert q["sse"] == want
            shapes = pq.plane_shapes(h, w, fmt)
            for k, p in enumerate(("y", "cb", "cr")):
                assert q[p] == pq.psnr(want[k], shapes[k][0] * shapes[k][1], depth), (fmt, h, w, p)
                assert q["msssim_" + p] is None                              # no plane of these has five scales
            assert q["yuv"] == pq.yuv(q["y"], q["cb"], q["cr"])


def test_error_sums_above_32_bits_and_of_identical_pictures(cuda):
    import pmctf_quality
    n = pq.frame_samples(64, 64, "444")
    a = torch.from_numpy(np.zeros(n, np.uint16)).to(cuda)
    b = torch.from_numpy(np.full(n, 65535, np.uint16)).to(cuda)
    want = (4096 * 65535 ** 2,) * 3
    assert want[0] > 2 ** 32
    assert pmctf_quality.planar_sse(a, b, 64, 64, "444", 16) == want == pmctf_quality.planar_sse(b, a, 64, 64, "444", 16)
    q = pmctf_quality.frame_quality_planar(b, b.clone(), 64, 64, "444", 16)
    assert q["sse"] == (0, 0, 0) and all(q[k] == math.inf for k in ("y", "cb", "cr", "yuv"))


def test_error_sums_of_a_picture_beyond_one_step_of_the_grid(cuda):
    """the sizes above fit one step of the kernel's grid; 720x1280 4:2:2 has 460800 groups of four samples, more than the 256
    workgroups of 256 threads take in one step of four groups each: the grid-stride loop runs twice"""
    import pmctf_quality
    h, w, fmt = 720, 1280, "422"
    assert pq.frame_samples(h, w, fmt) // 4 > 256 * 256 * 4
    for depth in (8, 10):
        a, b = pq.random_frame(h, w, fmt, depth, seed=1), pq.random_frame(h, w, fmt, depth, seed=2)
        got = pmctf_quality.planar_sse(_placed(a, 2, cuda), _placed(b, 0, cuda), h, w, fmt, depth)
        assert got == pq.sse(a, b, h, w, fmt), depth


@pytest.mark.parametrize("depth", (8, 10))
def test_error_sums_equal_the_existing_420_paths(cuda, depth):
    """the same integer pictures through the float planes of the codec's own quality paths"""
    import pmctf_quality
    from pMCTF.hip import ops
    for h, w in pq.SSE_SIZES[1:]:
        a, b = (torch.from_numpy(pq.random_frame(h, w, "420", depth, seed=s)).to(cuda) for s in (3, 4))
        got = pmctf_quality.planar_sse(a, b, h, w, "420", depth)
        _, _, a_y, a_c = ops.planes_from(a, h, w, depth, psize=2)
        b_y, b_c, _, _ = ops.planes_from(b, h, w, depth, psize=2)
        if depth == 8:
            old = ops.frame_quality(b_y, b_c, a_y, a_c, h, w, msssim=False)["sse"][:3]
        else:
            old = ops.frame_sse_hbd(b_y, b_c, a_y, a_c, h, w, depth)["sse"]
        assert got == tuple(old) == pq.sse(a.cpu().numpy(), b.cpu().numpy(), h, w, "420"), (h, w, got, old)


def _ref(h, w, depth, i):
    """the plane pair and its CPU yardsticks, computed once per session"""
    key = (h, w, depth, i)
    if key not in _refs:
        a, b = pq.plane_pair(h, w, depth, pq.NOISE[i], seed=i)
        r64, m64 = pq.ms_ssim(a, b, depth, torch.float64)
        r32, m32 = pq.ms_ssim(a, b, depth, torch.float32)
        _refs[key] = {"a": a, "b": b, "r64": r64, "m64": m64, "r32": r32, "m32": m32}
    return _refs[key]


def _hold(got, means, c, what):
    """the rule of DESIGN 5e on the result and on each of the ten means"""
    err = abs(got - c["r64"])
    worst = (0.0, None)
    for s in range(5):
        for k in range(2):
            e, bd = abs(means[s][k] - c["m64"][s][k]), pq.bound(c["m64"][s][k], c["m32"][s][k])
            if e / bd >= worst[0]:
                worst = (e / bd, (s, "cs ssim".split()[k], e, bd))
    print(f"\nplane-msssim {what}: r64 {c['r64']:.12f} e32 {abs(c['r32'] - c['r64']):.3e} hip {got:.12f} |hip-r64| {err:.3e} "
          f"bound {pq.bound(c['r64'], c['r32']):.3e}; worst mean (scale, map, error, bound) {worst[1]}")
    assert err <= pq.bound(c["r64"], c["r32"]), what
    assert worst[0] <= 1.0, (what, worst)


@pytest.mark.parametrize("h,w", pq.MSSSIM_SIZES)
def test_plane_msssim_against_the_float64_restatement(cuda, h, w):
    import pmctf_quality
    for depth in pq.DEPTHS:
        for i, sigma in enumerate(pq.NOISE):
            c = _ref(h, w, depth, i)
            assert all(m > 0 for pair in c["m64"] for m in pair), "a relu fires: the comparison would be empty"
            if i == len(pq.NOISE) - 1:           # premise: the clamp is live
                assert (c["b"] == 0).any() and (c["b"] == (1 << depth) - 1).any()
            got, means = pmctf_quality.plane_msssim(torch.from_numpy(c["a"]).to(cuda), torch.from_numpy(c["b"]).to(cuda), depth)
            _hold(got, means, c, f"{h}x{w} {depth}-bit sigma {sigma}")
            assert 0.0 < got < 1.0


def test_constant_and_identical_planes_and_determinism(cuda):
    import pmctf_quality
    one = {"r64": 1.0, "r32": 1.0, "m64": [(1.0, 1.0)] * 5, "m32": [(1.0, 1.0)] * 5}
    for depth in pq.DEPTHS:
        top = (1 << depth) - 1
        c = _ref(161, 323, depth, 1)
        a, b = torch.from_numpy(c["a"]).to(cuda), torch.from_numpy(c["b"]).to(cuda)
        got, means = pmctf_quality.plane_msssim(a, a.clone(), depth)
        _hold(got, means, one, f"identical planes, {depth}-bit")
        for level in (0, 1, top // 3, top):
            flat = torch.from_numpy(np.full((161, 323), level, _np_dtype(depth))).to(cuda)
            got, means = pmctf_quality.plane_msssim(flat, flat.clone(), depth)
            _hold(got, means, one, f"constant planes of {level}, {depth}-bit")
        first, again = pmctf_quality.plane_msssim(a, b, depth), pmctf_quality.plane_msssim(a, b, depth)
        assert first == again                    # every float bit-identical
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            other = pmctf_quality.plane_msssim(a, b, depth)
        s.synchronize()
        assert other == first


def test_frame_quality_planar_agrees_with_the_entries(cuda):
    import pmctf_quality
    h, w = 164, 176
    for depth in (8, 10):
        a, b = (torch.from_numpy(f).to(cuda) for f in pq.synth_frames(h, w, "444", depth, 2, seed=depth))
        q = pmctf_quality.frame_quality_planar(a, b, h, w, "444", depth)
        assert q == pmctf_quality.frame_quality_planar(a, b, h, w, "444", depth)
        assert q["sse"] == pmctf_quality.planar_sse(a, b, h, w, "444", depth) == pq.sse(a.cpu().numpy(), b.cpu().numpy(), h, w, "444")
        for k, p in enumerate(("y", "cb", "cr")):
            pa, pb = (t[k * h * w:(k + 1) * h * w].reshape(h, w) for t in (a, b))
            assert q["msssim_" + p] == pmctf_quality.plane_msssim(pa, pb, depth)[0], p
            assert q[p] == pq.psnr(q["sse"][k], h * w, depth)
        assert q["yuv"] == pq.yuv(q["y"], q["cb"], q["cr"])
        off = pmctf_quality.frame_quality_planar(a, b, h, w, "444", depth, msssim=False)
        assert off["sse"] == q["sse"] and off["msssim_y"] is off["msssim_cb"] is off["msssim_cr"] is None
        # 4:2:0 and 4:2:2 of the same size: the chroma planes are 82x88 and 164x88, neither has five scales
        for fmt in ("420", "422"):
            n = pq.frame_samples(h, w, fmt)
            q2 = pmctf_quality.frame_quality_planar(a[:n].clone(), b[:n].clone(), h, w, fmt, depth)
            assert q2["msssim_y"] == q["msssim_y"] and q2["msssim_cb"] is None and q2["msssim_cr"] is None
            assert q2["sse"] == pq.sse(a[:n].cpu().numpy(), b[:n].cpu().numpy(), h, w, fmt)


# ------------------------------------------------------------------------------------------------------- stream order
def _vp(t):
    return C.c_void_p(t.data_ptr())


def _b_sse(name, depth):
    def build():
        import pmctf_quality
        from pMCTF.hip import lib
        L = pmctf_quality.library()
        h, w, fmt = 18, 34, "422"
        draw = lambda s: {k: pq.random_frame(h, w, fmt, depth, seed=s + i) for i, k in enumerate("ab")}

        def call(t):                             # the entry's own clear, onto garbage the caller left on S
            if depth == 8:
                rc = L.pmctf_planar_sse_u8(_vp(t["a"]), _vp(t["b"]), h, w, 422, _vp(t["sse"]), pmctf_quality._stream())
            else:
                rc = L.pmctf_planar_sse_u16(_vp(t["a"]), _vp(t["b"]), h, w, 422, depth, _vp(t["sse"]), pmctf_quality._stream())
            lib.check(rc, name)
        return so.Case(draw(10), call, draw(20), outs={"sse": ((3,), "int64")}, clears=("sse",))
    return build


def _b_msssim(name, depth):
    def build():
        import pmctf_quality
        from pMCTF.hip import lib
        L = pmctf_quality.library()
        h, w = 162, 165
        n_scratch = L.pmctf_plane_msssim_scratch_floats(h, w)

        def draw(s):
            a, b = pq.plane_pair(h, w, depth, 0.05, seed=s)
            return {"a": a, "b": b}

        def call(t):
            scratch = torch.empty(n_scratch, dtype=torch.float32, device=t["a"].device)
            if depth == 8:
                rc = L.pmctf_plane_msssim_u8(_vp(t["a"]), _vp(t["b"]), h, w, _vp(scratch), _vp(t["out"]), pmctf_quality._stream())
            else:
                rc = L.pmctf_plane_msssim_u16(_vp(t["a"]), _vp(t["b"]), h, w, depth, _vp(scratch), _vp(t["out"]),
                                              pmctf_quality._stream())
            lib.check(rc, name)
        return so.Case(draw(1), call, draw(2), outs={"out": ((10,), "float64")})
    return build


ROWS = [so.Row("planar_sse_u8", "pmctf_planar_sse_u8", _b_sse("planar_sse_u8", 8)),
        so.Row("planar_sse_u16", "pmctf_planar_sse_u16", _b_sse("planar_sse_u16", 12)),
        so.Row("plane_msssim_u8", "pmctf_plane_msssim_u8", _b_msssim("plane_msssim_u8", 8)),
        so.Row("plane_msssim_u16", "pmctf_plane_msssim_u16", _b_msssim("plane_msssim_u16", 10))]


@pytest.fixture(scope="module")
def caller(cuda):
    s, report = so.pick_stream(cuda)
    print(f"\ncaller stream: candidate {report[-1][0]} of {len(report)}; windows (name, forward, back): {report}")
    return s


def test_the_rows_cover_every_stream_taking_entry_of_the_new_header():
    import pmctf_quality
    takers = set(pmctf_quality.SIGS) - {"pmctf_plane_msssim_scratch_floats"}          # host arithmetic: a size
    assert {r.entry for r in ROWS} == takers and len({r.name for r in ROWS}) == len(ROWS)


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_entry_runs_in_its_stream_s_order(cuda, caller, row):
    so.check_row(row, cuda, caller)


# --------------------------------------------------------------------------------------------------------- end to end
W, H, N, GOP, Q = 176, 164, 4, 4, 3


def _write_y4m(path, frames, fmt, depth):
    import pmctf_chroma
    with open(path, "wb") as f:
        f.write(pmctf_chroma.y4m_header(W, H, (25, 1), fmt, depth))
        for fr in frames:
            f.write(b"FRAME\n" + fr.astype("<u2" if depth > 8 else np.uint8).tobytes())


def _read(path, **kw):
    """every picture of a file as packed arrays, through the reader compare_files uses"""
    import pmctf_chroma
    r = pmctf_chroma.PlanarReader(path, **kw)
    try:
        return [np.concatenate([p.reshape(-1) for p in r.read_one_frame()]) for _ in range(len(r))]
    finally:
        r.close()


@pytest.fixture(scope="module")
def loop444(cuda, tmp_path_factory):
    """4 pictures 176x164 10-bit 4:4:4 in a .y4m, GOP 4: coded, decoded to a .y4m"""
    import pmctf_layout
    td = tmp_path_factory.mktemp("planar_quality")
    src, bins, dec = str(td / "src.y4m"), str(td / "bins"), str(td / "dec.y4m")
    os.makedirs(bins)
    _write_y4m(src, pq.synth_frames(H, W, "444", 10, N, seed=5), "444", 10)
    enc_net, dec_net = product_model(1)[0], product_model(1)[0]
    with torch.no_grad():
        pmctf_layout.encode_sequence(enc_net, src, W, H, N, GOP, Q, bins, "cuda", keep_gops=True, bitdepth=10)
        d = pmctf_layout.decode_sequence_checked(dec_net, bins, dec, "cuda")
    assert d["frames"] == [(H, W)] * N and d["bitdepth"] == 10
    return {"td": td, "src": src, "bins": bins, "dec": dec, "enc_net": enc_net, "dec_net": dec_net}


def test_y4m_to_folder_to_y4m_to_quality(cuda, loop444):
    import pmctf_quality
    q = pmctf_quality.compare_files(loop444["src"], loop444["dec"], "cuda", gop=GOP)
    assert (q["width"], q["height"], q["chroma_format"], q["bitdepth"], q["frame_num"]) == (W, H, "444", 10, N)
    assert q["frame_types"] == [0, 1, 1, 1] and len(q["lines"]) == N and q["lines"][2].startswith("frame 2, YUV-PSNR: ")
    src, dec = _read(loop444["src"]), _read(loop444["dec"])
    assert len(src) == len(dec) == N
    for i in range(N):
        want = pq.sse(src[i], dec[i], H, W, "444")
        assert q["sse"][i] == want and all(e > 0 for e in want)              # the coder is lossy: something is measured
        psnrs = [pq.psnr(e, H * W, 10) for e in want]
        assert [q["psnr_y"][i], q["psnr_cb"][i], q["psnr_cr"][i]] == psnrs and q["psnr"][i] == pq.yuv(*psnrs)
        for p, a, b in zip(("y", "cb", "cr"), pq.split(src[i], H, W, "444"), pq.split(dec[i], H, W, "444")):
            r64, m64 = pq.ms_ssim(a, b, 10, torch.float64)
            r32, _ = pq.ms_ssim(a, b, 10, torch.float32)
            got = q["msssim_" + p][i]
            print(f"\nframe {i} {p}: r64 {r64:.12f} e32 {abs(r32 - r64):.3e} hip {got:.12f} |hip-r64| {abs(got - r64):.3e}")
            assert abs(got - r64) <= pq.bound(r64, r32), (i, p)
    for k in pmctf_quality.TABLES:
        assert q["mean"][k] == sum(q[k]) / N, k
    # fewer frames, PSNR only: a table with None entries has no mean
    part = pmctf_quality.compare_files(loop444["src"], loop444["dec"], "cuda", frame_num=2, msssim=False)
    assert part["sse"] == q["sse"][:2] and part["msssim_y"] == [None, None] and part["mean"]["msssim_y"] is None
    assert part["mean"]["psnr_y"] == sum(q["psnr_y"][:2]) / 2 and part["frame_types"] is None


def test_raw_8bit_420_loop_equals_sequence_quality(cuda, loop444, tmp_path):
    import pmctf_gop
    import pmctf_quality
    import pmctf_synth
    src, bins, dec = str(tmp_path / "src.yuv"), str(tmp_path / "bins"), str(tmp_path / "dec.yuv")
    os.makedirs(bins)
    pmctf_gop.write_yuv(src, pmctf_synth.synth_yuv420(W, H, N, seed=11))
    with torch.no_grad():
        pmctf_gop.encode_sequence(loop444["enc_net"], src, W, H, N, GOP, Q, bins, "cuda", keep_gops=True)
        pmctf_gop.decode_sequence(loop444["dec_net"], bins, dec, "cuda")
    old = pmctf_gop.sequence_quality(src, dec, W, H, N, "cuda", gop=GOP, msssim=False)
    new = pmctf_quality.compare_files(src, dec, "cuda", width=W, height=H, gop=GOP)
    for k in ("psnr", "psnr_y", "psnr_cb", "psnr_cr"):
        assert new[k] == old[k], k               # to the last bit of the float64
        assert new["mean"][k] == old["mean"][k]
    assert new["sse"] == [tuple(s[:3]) for s in old["sse"]] and new["frame_types"] == old["frame_types"]
    assert all(v is not None and 0.0 < v < 1.0 for v in new["msssim_y"])
    assert new["msssim_cb"] == [None] * N and new["mean"]["msssim_cr"] is None          # 82x88 chroma planes


def test_decode_tool_compares_what_it_wrote(cuda, loop444):
    import pmctf_quality
    out = str(loop444["td"] / "tool.y4m")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "decode_sequence.py"), "--synth-seed", "0", "--compare", loop444["src"],
           loop444["bins"], out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(out, "rb").read() == open(loop444["dec"], "rb").read()
    q = pmctf_quality.compare_files(loop444["src"], loop444["dec"], "cuda")
    lines = r.stdout.splitlines()
    assert [l for l in lines if l.startswith("frame ")] == q["lines"]
    assert lines[-1] == pmctf_quality.average_line(q) and lines[-1].startswith(f"average of {N} frames (176x164 444 10-bit)")
    # the stand-alone tool on the same two files, with the tables as JSON
    import json
    js = str(loop444["td"] / "q.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "compare_sequences.py"), loop444["src"], out, "--gop",
                        str(GOP), "--json", js], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.splitlines() == q["lines"] + [pmctf_quality.average_line(q)]
    got = json.load(open(js))
    assert all(got[k] == q[k] for k in pmctf_quality.TABLES) and got["mean"] == q["mean"]
    assert [tuple(s) for s in got["sse"]] == q["sse"] and got["frame_types"] == [0, 1, 1, 1]
