"""Quality of pictures as they lie in files: per-plane PSNR and per-plane MS-SSIM of planar 4:2:0, 4:2:2 and
4:4:4 pictures at 8..16 bits, in the picture's own chroma format and at its own data range 2^b - 1, from the HIP kernels of
csrc/quality_planar.hip (C ABI: include/pmctf_quality.h).

  frame_quality_planar   two packed pictures on the device (what pmctf_chroma.PlanarReader's planes concatenate to, what the
                         decoders' sinks write) -> PSNR of Y, Cb, Cr, their 6:1:1 mean, the exact error sums, MS-SSIM per
                         plane; a handful of launches and one device->host copy per picture
  compare_files          two files (.y4m, or raw planar with the keywords) -> per-frame tables, means and report lines in
                         the shape of pmctf_gop.sequence_quality
  planar_sse, plane_msssim   the entries one by one

The error sums are 64-bit integers and exact.  MS-SSIM is the algorithm of pmctf_frame_quality_f32 with one
channel and the constants C1 = (0.01 L)^2, C2 = (0.03 L)^2 at L = 2^b - 1; the five powers and their product are taken on
the host in float64.  A plane whose smaller side is 160 or less has no five scales: its MS-SSIM is None.

The ctypes signatures of the five entries live here, with their only caller (pMCTF/hip/lib.py holds those of
include/pmctf_hip.h).  Like the rest of the product path there is no CPU fallback: RuntimeError without a GPU.

Out of scope: 4:0:0 and interlaced material, other metrics.  RGB above 8 bits: two gbrp10 / gbrp12 / gbrp16 files
(pmctf_colour) are planar 4:4:4 files here, planes G, B, R; one RGB-domain MS-SSIM figure is not computed."""
import ctypes as C
import math
import os

import pmctf_chroma

FORMAT_CODES = {"420": 420, "422": 422, "444": 444}             # the integer codes of pmctf_convert_chroma_*
MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MSSSIM_MIN_SIDE = 160                                           # (11 - 1) * 2^4: the smaller side must exceed it
MSSSIM_OUT_DOUBLES = 10                                         # PMCTF_PLANE_MSSSIM_OUT_DOUBLES
MAX_SIDE = 16384
PLANES = ("y", "cb", "cr")
TABLES = ("psnr", "psnr_y", "psnr_cb", "psnr_cr", "msssim_y", "msssim_cb", "msssim_cr")

_P, _I = C.c_void_p, C.c_int
SIGS = {
    "pmctf_planar_sse_u8": (_I, [_P, _P, _I, _I, _I, _P, _P]),
    "pmctf_planar_sse_u16": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "pmctf_plane_msssim_scratch_floats": (C.c_int64, [_I, _I]),
    "pmctf_plane_msssim_u8": (_I, [_P, _P, _I, _I, _P, _P, _P]),
    "pmctf_plane_msssim_u16": (_I, [_P, _P, _I, _I, _I, _P, _P, _P]),
}


def library():
    """libpmctf_hip.so as pMCTF.hip.lib loads it, with the signatures of the five entries of include/pmctf_quality.h set"""
    from pMCTF.hip import lib
    L = lib.hip()
    for name, (res, args) in SIGS.items():
        fn = getattr(L, name)                                   # AttributeError if the symbol is missing
        fn.restype, fn.argtypes = res, args
    return L


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(rc, what):
    from pMCTF.hip import lib
    lib.check(rc, what)


# ------------------------------------------------------------------------------------------------------ host arithmetic
def check_bitdepth(bitdepth):
    if isinstance(bitdepth, bool) or not isinstance(bitdepth, int) or not 8 <= bitdepth <= 16:
        raise ValueError(f"bitdepth is 8 or 9..16 (got {bitdepth!r})")
    return bitdepth


def plane_shapes(height, width, chroma_format):
    """-> ((h, w) of Y, of Cb, of Cr) of a picture of that chroma format"""
    sx, sy = pmctf_chroma.SUBSAMPLING[pmctf_chroma.check_format(chroma_format)]
    return (height, width), (height // sy, width // sx), (height // sy, width // sx)


def psnr_from_sse(sse, n, bitdepth=8):
    """10 log10(max^2 n / sse) with max = 2^bitdepth - 1, float64 on the host; inf for sse == 0"""
    return math.inf if sse == 0 else 10.0 * math.log10(float((1 << bitdepth) - 1) ** 2 * n / sse)


def yuv_psnr(y, cb, cr):
    """(6 Y + Cb + Cr) / 8, as pmctf_gop.gop_psnr defines it"""
    return (6.0 * y + cb + cr) / 8.0


def msssim_from_means(means):
    """means[s] = (mean cs, mean ssim) of scale s of one plane -> the product of relu(cs_s)^w_s over scales 0..3 and
    relu(ssim_4)^w_4; float64 on the host (pMCTF.hip.ops.msssim_from_means with one channel)"""
    v = 1.0
    for s, wgt in enumerate(MSSSIM_WEIGHTS):
        v *= max(float(means[s][1 if s == len(MSSSIM_WEIGHTS) - 1 else 0]), 0.0) ** wgt
    return v


def has_msssim(h, w):
    return min(h, w) > MSSSIM_MIN_SIDE


# --------------------------------------------------------------------------------------------------------- the entries
def _picture(frame, height, width, chroma_format, bitdepth, what):
    """a packed picture on the device, checked -> the contiguous tensor"""
    import torch
    dtype = torch.uint8 if bitdepth == 8 else torch.uint16
    if not isinstance(frame, torch.Tensor) or frame.dtype != dtype:
        raise ValueError(f"{what}: expect a {dtype} tensor at bitdepth {bitdepth}")
    n = pmctf_chroma.frame_samples(width, height, chroma_format)
    if frame.numel() != n:
        raise ValueError(f"{what}: a {height}x{width} {chroma_format} picture has {n} samples, got {frame.numel()}")
    if not frame.is_cuda:
        raise RuntimeError("pmctf_quality runs on the GPU (no CPU fallback): pass device tensors")
    return frame.contiguous().reshape(-1)


def _sizes(height, width, chroma_format, bitdepth):
    pmctf_chroma.check_format(chroma_format)
    pmctf_chroma.check_side(width, height)
    return int(height), int(width), check_bitdepth(bitdepth)


def _enqueue_sse(L, a, b, h, w, chroma_format, bitdepth, sse_ptr):
    pa, pb = C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr())
    if bitdepth == 8:
        rc = L.pmctf_planar_sse_u8(pa, pb, h, w, FORMAT_CODES[chroma_format], sse_ptr, _stream())
    else:
        rc = L.pmctf_planar_sse_u16(pa, pb, h, w, FORMAT_CODES[chroma_format], bitdepth, sse_ptr, _stream())
    _check(rc, "planar_sse")


def _enqueue_msssim(L, a_ptr, b_ptr, h, w, bitdepth, scratch, out_ptr):
    pa, pb, ps = C.c_void_p(a_ptr), C.c_void_p(b_ptr), C.c_void_p(scratch.data_ptr())
    if bitdepth == 8:
        rc = L.pmctf_plane_msssim_u8(pa, pb, h, w, ps, out_ptr, _stream())
    else:
        rc = L.pmctf_plane_msssim_u16(pa, pb, h, w, bitdepth, ps, out_ptr, _stream())
    _check(rc, "plane_msssim")


def planar_sse(frame_a, frame_b, height, width, chroma_format="420", bitdepth=8):
    """sums of squared differences of two packed pictures on the device -> (Y, Cb, Cr) ints, exact.  One clear, one launch,
    one device->host copy."""
    import torch
    h, w, bitdepth = _sizes(height, width, chroma_format, bitdepth)
    a = _picture(frame_a, h, w, chroma_format, bitdepth, "frame_a")
    b = _picture(frame_b, h, w, chroma_format, bitdepth, "frame_b")
    out = torch.empty(3, dtype=torch.int64, device=a.device)
    _enqueue_sse(library(), a, b, h, w, chroma_format, bitdepth, C.c_void_p(out.data_ptr()))
    return tuple(v & 0xffffffffffffffff for v in out.cpu().tolist())


def plane_msssim(plane_a, plane_b, bitdepth=8):
    """MS-SSIM of one plane against another: two (h, w) device tensors, uint8 at bitdepth 8 and uint16 above, any sizes with
    min(h, w) > 160 -> (MS-SSIM, means [5] of (mean cs, mean ssim)).  Six launches, one device->host copy."""
    import torch
    bitdepth = check_bitdepth(bitdepth)
    dtype = torch.uint8 if bitdepth == 8 else torch.uint16
    for t in (plane_a, plane_b):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != 2:
            raise ValueError(f"expect two (h, w) {dtype} tensors at bitdepth {bitdepth}")
    if plane_a.shape != plane_b.shape:
        raise ValueError(f"the planes differ in size: {tuple(plane_a.shape)} and {tuple(plane_b.shape)}")
    h, w = (int(s) for s in plane_a.shape)
    if not has_msssim(h, w) or max(h, w) > MAX_SIDE:
        raise ValueError(f"MS-SSIM with five scales needs a smaller side above {MSSSIM_MIN_SIDE} and sides up to {MAX_SIDE}, "
                         f"got {h}x{w}")
    if not (plane_a.is_cuda and plane_b.is_cuda):
        raise RuntimeError("pmctf_quality runs on the GPU (no CPU fallback): pass device tensors")
    a, b = plane_a.contiguous(), plane_b.contiguous()
    L = library()
    scratch = torch.empty(L.pmctf_plane_msssim_scratch_floats(h, w), dtype=torch.float32, device=a.device)
    out = torch.empty(MSSSIM_OUT_DOUBLES, dtype=torch.float64, device=a.device)
    _enqueue_msssim(L, a.data_ptr(), b.data_ptr(), h, w, bitdepth, scratch, C.c_void_p(out.data_ptr()))
    host = out.cpu().tolist()
    means = [(host[2 * s], host[2 * s + 1]) for s in range(len(MSSSIM_WEIGHTS))]
    return msssim_from_means(means), means


def frame_quality_planar(frame_a, frame_b, height, width, chroma_format="420", bitdepth=8, msssim=True):
    """Quality of one picture against another, both packed planar pictures on the device (uint8 at bitdepth 8, uint16 at
    9..16): Y of height x width, then Cb and Cr in chroma_format "420", "422" or "444".
    -> {"y", "cb", "cr": PSNR in dB against 2^bitdepth - 1 (inf for identical planes), "yuv": (6 y + cb + cr) / 8,
        "sse": (Y, Cb, Cr) ints, "msssim_y", "msssim_cb", "msssim_cr": MS-SSIM of the plane at its own data range, None
        where the plane's smaller side is 160 or less or when msssim is false}.
    One clear and one launch for the sums, six launches per plane with MS-SSIM, ONE device->host copy."""
    import torch
    h, w, bitdepth = _sizes(height, width, chroma_format, bitdepth)
    a = _picture(frame_a, h, w, chroma_format, bitdepth, "frame_a")
    b = _picture(frame_b, h, w, chroma_format, bitdepth, "frame_b")
    shapes = plane_shapes(h, w, chroma_format)
    with_ms = [bool(msssim) and has_msssim(*s) for s in shapes]
    L = library()
    # one result buffer of 8-byte words: the three sums, then ten means per plane
    out = torch.empty(3 + 3 * MSSSIM_OUT_DOUBLES, dtype=torch.int64, device=a.device)
    _enqueue_sse(L, a, b, h, w, chroma_format, bitdepth, C.c_void_p(out.data_ptr()))
    if any(with_ms):
        need = max(L.pmctf_plane_msssim_scratch_floats(*s) for s, ms in zip(shapes, with_ms) if ms)
        scratch = torch.empty(need, dtype=torch.float32, device=a.device)     # the planes follow each other on the stream
        off, item = 0, a.element_size()
        for k, (s, ms) in enumerate(zip(shapes, with_ms)):
            if ms:
                _enqueue_msssim(L, a.data_ptr() + off * item, b.data_ptr() + off * item, s[0], s[1], bitdepth, scratch,
                                C.c_void_p(out.data_ptr() + 8 * (3 + k * MSSSIM_OUT_DOUBLES)))
            off += s[0] * s[1]
    host = out.cpu()                                            # the picture's one copy to the host
    sse = tuple(v & 0xffffffffffffffff for v in host[:3].tolist())
    means = host[3:].view(torch.float64).tolist()
    res = {p: psnr_from_sse(e, s[0] * s[1], bitdepth) for p, e, s in zip(PLANES, sse, shapes)}
    res["yuv"] = yuv_psnr(res["y"], res["cb"], res["cr"])
    res["sse"] = sse
    for k, (p, ms) in enumerate(zip(PLANES, with_ms)):
        m = means[k * MSSSIM_OUT_DOUBLES:(k + 1) * MSSSIM_OUT_DOUBLES]
        res["msssim_" + p] = msssim_from_means([(m[2 * s], m[2 * s + 1]) for s in range(len(MSSSIM_WEIGHTS))]) if ms else None
    return res


# ----------------------------------------------------------------------------------------------------------- two files
def _fmt(v, digits=4):
    return "n/a" if v is None else f"{v:.{digits}f}"


def quality_line(idx, q):
    """one frame's report line"""
    return (f"frame {idx}, YUV-PSNR: {q['yuv']:.4f}, Y-PSNR: {q['y']:.4f}, Cb-PSNR: {q['cb']:.4f}, Cr-PSNR: {q['cr']:.4f}, "
            f"MS-SSIM Y: {_fmt(q['msssim_y'], 6)}, Cb: {_fmt(q['msssim_cb'], 6)}, Cr: {_fmt(q['msssim_cr'], 6)}")


def average_line(result):
    """the averages of compare_files' result, in the wording of quality_line"""
    m = result["mean"]
    return (f"average of {result['frame_num']} frames ({result['width']}x{result['height']} {result['chroma_format']} "
            f"{result['bitdepth']}-bit), YUV-PSNR: {m['psnr']:.4f}, Y-PSNR: {m['psnr_y']:.4f}, Cb-PSNR: {m['psnr_cb']:.4f}, "
            f"Cr-PSNR: {m['psnr_cr']:.4f}, MS-SSIM Y: {_fmt(m['msssim_y'], 6)}, Cb: {_fmt(m['msssim_cb'], 6)}, "
            f"Cr: {_fmt(m['msssim_cr'], 6)}")


def _open(path, width, height, chroma_format, bitdepth):
    """a .y4m speaks for itself; a raw file takes the keywords"""
    if pmctf_chroma.is_y4m(path):
        return pmctf_chroma.PlanarReader(path)
    return pmctf_chroma.PlanarReader(path, width, height, 0, bitdepth, chroma_format)


def _describe(r):
    return f"{r.src_file}: {r.width}x{r.height} {r.chroma_format} {r.bitdepth}-bit"


def compare_files(src, rec, device, width=None, height=None, frame_num=None, chroma_format=None, bitdepth=None, msssim=True,
                  gop=None):
    """Quality of the pictures of file rec against those of file src, frame by frame, in the files' own chroma format and
    bit depth.  Both are opened with pmctf_chroma.PlanarReader: a .y4m carries its size, format and depth, a raw planar
    file takes width, height, chroma_format (default "420") and bitdepth (default 8).  The two must agree in size, format
    and depth (ValueError naming both).  frame_num=None: the whole pictures of the shorter file.
    -> {"psnr" (YUV), "psnr_y", "psnr_cb", "psnr_cr", "msssim_y", "msssim_cb", "msssim_cr": per-frame lists, "sse":
        [(Y, Cb, Cr)], "mean": {table: mean, None for a table with None entries}, "frame_types": [0] + [1] * (gop - 1) per
        GOP when gop is given, else None, "lines": one report line per frame, "width", "height", "chroma_format",
        "bitdepth", "frame_num"}.
    What can be refused without a GPU is refused first; then RuntimeError unless device is a GPU."""
    readers = []
    try:
        for path in (src, rec):
            readers.append(_open(path, width, height, chroma_format, bitdepth))
        ro, rd = readers
        key = lambda r: (r.width, r.height, r.chroma_format, r.bitdepth)
        if key(ro) != key(rd):
            raise ValueError(f"{_describe(ro)} and {_describe(rd)}: the two files must agree in size, chroma format and "
                             f"bit depth")
        if frame_num is None:
            frame_num = min(len(ro), len(rd))
            if frame_num <= 0:
                raise ValueError(f"{src}, {rec}: no whole picture to compare")
        if isinstance(frame_num, bool) or not isinstance(frame_num, int) or frame_num <= 0:
            raise ValueError(f"frame_num is a positive integer or None (got {frame_num!r})")
        for r in readers:
            if len(r) < frame_num:
                raise ValueError(f"{_describe(r)}: shorter than {frame_num} pictures (it holds {len(r)})")
        if gop is not None and (gop < 1 or frame_num % gop):
            raise ValueError(f"frame_num {frame_num} is not a multiple of gop {gop}")
        import torch
        if torch.device(device).type != "cuda":
            raise RuntimeError("compare_files runs on the GPU (no CPU fallback)")
        import numpy as np
        w, h, fmt, depth = key(ro)
        names = {"yuv": "psnr", "y": "psnr_y", "cb": "psnr_cb", "cr": "psnr_cr", "msssim_y": "msssim_y",
                 "msssim_cb": "msssim_cb", "msssim_cr": "msssim_cr"}
        out = {v: [] for v in names.values()}
        out.update(sse=[], lines=[])
        for idx in range(frame_num):
            pics = [torch.from_numpy(np.concatenate([p.reshape(-1) for p in r.read_one_frame()])).to(device)
                    for r in readers]
            q = frame_quality_planar(pics[0], pics[1], h, w, fmt, depth, msssim=msssim)
            for k, v in names.items():
                out[v].append(q[k])
            out["sse"].append(q["sse"])
            out["lines"].append(quality_line(idx, q))
    finally:
        for r in readers:
            r.close()
    out["mean"] = {v: None if any(x is None for x in out[v]) else sum(out[v]) / frame_num for v in names.values()}
    out["frame_types"] = None if gop is None else ([0] + [1] * (gop - 1)) * (frame_num // gop)
    out.update(width=w, height=h, chroma_format=fmt, bitdepth=depth, frame_num=frame_num)
    return out


def print_report(result, file=None):
    """one line per frame, then the averages"""
    for line in result["lines"]:
        print(line, file=file)
    print(average_line(result), file=file)
