"""RGB pictures in and out: a colour description (matrix, range) with matrix "bt601", "bt709" or "bt2020"
(non-constant luminance) and range "full" or "limited" turns RGB pictures into 4:4:4 YCbCr pictures and back, in integers,
on the device (csrc/picture_colour.hip, C ABI: include/pmctf_colour.h).  The integers are part of the format.

  (Kr, Kb) = (299/1000, 114/1000), (2126/10000, 722/10000), (2627/10000, 593/10000); Kg = 1 - Kr - Kb
  RGB is full range 0..M, M = 2^b - 1, at the bit depth b (8..16) of the YCbCr picture
  range     sY            sC            oY           oC
  full      M             M             0            2^(b-1)
  limited   219 2^(b-8)   224 2^(b-8)   16 2^(b-8)   2^(b-1)
  forward   Y: sY/M (Kr, Kg, Kb)   Cb: sC/(2(1-Kb)M) (-Kr, -Kg, 1-Kb)   Cr: sC/(2(1-Kr)M) (1-Kr, -Kg, -Kb)
  inverse   on (Y-oY, Cb-oC, Cr-oC), a = M/sY, cb = 2(1-Kb)M/sC, cr = 2(1-Kr)M/sC:
            R: (a, 0, cr)   G: (a, -Kb/Kg cb, -Kr/Kg cr)   B: (a, cb, 0)

Every coefficient is k = round_half_even(c 2^29), taken with fractions.Fraction, except the forward G column, which is set
so that the row's integer sum is exact: round_half_even(sY/M 2^29) for the Y row (2^29 in full range), 0 for the chroma
rows.  So R = G = B = v gives Cb = Cr = 2^(b-1) exactly, and Y = v in full range; the inverse of a grey is R = G = B because
one `a` serves its three rows.  out = clamp((k0 x0 + k1 x1 + k2 x2 + (o << 29) + (1 << 28)) >> 29, 0, M) on a 64-bit signed
accumulator with an arithmetic shift; o is the row's offset going forward and 0 going back, where the inputs have their
offsets subtracted first.  Samples above the depth in 16-bit words are masked to b bits.  max |k| < 2^31: the coefficients
are int32.

RGB layouts (rows tight, pictures at frame_bytes): rgb24 / bgr24 (8 bits, R G B / B G R bytes per pixel), rgba / bgra (a
fourth byte: ignored on input, 255 on output), rgb48 (16 bits, little-endian words), gbrp (8 bits, planes G, B, R), gbrp10 /
gbrp12 / gbrp16 (planes of little-endian words, value in the low bits).

This module holds the arithmetic (coefficients), the wrappers of the four entries with their ctypes signatures (SIGS,
library), RgbUnpacker / RgbPacker (the counterparts of pmctf_layout.Unpacker / Packer: an RGB file is read by
pmctf_layout.PackedReader through them), colour_format.json, and the entry points: pmctf_layout's with rgb_layout / colour
(encoding) and rgb_out / rgb_layout / colour (decoding) added, and convert_file.  An RGB source is coded as the planar 4:4:4
source its conversion gives; a YCbCr source with a `colour` has the description recorded and nothing else changed.  Without
the new keywords every entry point does what pmctf_layout's does.  Like the rest of the product path there is no CPU
fallback.

Out of scope: limited-range RGB; constant-luminance BT.2020, ICtCp and transfer functions; 16-bit PNG files (deep RGB enters
as raw rgb48 / gbrp*); 10-bit packed RGB words; pitched rows; Y4M colour-range tags; RGB-domain MS-SSIM above 8 bits."""
import ctypes as C
import functools
import os
from fractions import Fraction

import pmctf_chroma
import pmctf_layout
from pmctf_records import is_int, read_record, write_record

FIXED_POINT_BITS = 29
MATRICES = {"bt601": (Fraction(299, 1000), Fraction(114, 1000)), "bt709": (Fraction(2126, 10000), Fraction(722, 10000)),
            "bt2020": (Fraction(2627, 10000), Fraction(593, 10000))}
RANGES = ("full", "limited")
DEFAULT_COLOUR = ("bt709", "limited")                         # of an RGB source that does not say
SOURCES = ("rgb", "ycbcr")
COLOUR_FORMAT = "colour_format.json"
COLOUR_FORMAT_VERSION = 1
COLOUR_FIELDS = ("format_version", "matrix", "range", "fixed_point_bits", "source")
PLANAR444 = "planar444"
# name -> (code of include/pmctf_colour.h, bit depth, components of a pixel or planes of a picture)
LAYOUTS = {"rgb24": (0, 8, 3), "bgr24": (1, 8, 3), "rgba": (2, 8, 4), "bgra": (3, 8, 4), "rgb48": (4, 16, 3),
           "gbrp": (5, 8, 3), "gbrp10": (6, 10, 3), "gbrp12": (7, 12, 3), "gbrp16": (8, 16, 3)}

_P, _I = C.c_void_p, C.c_int
SIGS = {
    "pmctf_rgb_to_ycc_u8": (_I, [_P, _P, _I, _I, _I, _P, _P, _P]),
    "pmctf_rgb_to_ycc_u16": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "pmctf_ycc_to_rgb_u8": (_I, [_P, _P, _I, _I, _I, _P, _P, _P]),
    "pmctf_ycc_to_rgb_u16": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P]),
}


def library():
    """libpmctf_hip.so as pMCTF.hip.lib loads it, with the signatures of the four entries of include/pmctf_colour.h set"""
    from pMCTF.hip import lib
    L = lib.hip()
    for name, (res, args) in SIGS.items():
        fn = getattr(L, name)                                   # AttributeError if the symbol is missing
        fn.restype, fn.argtypes = res, args
    return L


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------------ the arithmetic
def check_colour(colour, what="colour"):
    """-> (matrix, range); ValueError naming `what` for anything else"""
    try:
        matrix, rng = colour
    except (TypeError, ValueError):
        raise ValueError(f"{what} is (matrix, range) (got {colour!r})") from None
    if not isinstance(matrix, str) or matrix not in MATRICES:
        raise ValueError(f"{what}: the matrix is one of {sorted(MATRICES)} (got {matrix!r})")
    if not isinstance(rng, str) or rng not in RANGES:
        raise ValueError(f"{what}: the range is one of {RANGES} (got {rng!r})")
    return matrix, rng


def check_bitdepth(bitdepth):
    if not is_int(bitdepth) or not 8 <= bitdepth <= 16:
        raise ValueError(f"bitdepth is 8 or 9..16 (got {bitdepth!r})")
    return bitdepth


def check_rgb_layout(layout, what="rgb_layout"):
    """-> (code, bitdepth, components); ValueError naming `what` otherwise"""
    if not isinstance(layout, str) or layout not in LAYOUTS:
        raise ValueError(f"{what} is one of {sorted(LAYOUTS)} (got {layout!r})")
    return LAYOUTS[layout]


def scales(rng, bitdepth):
    """-> (sY, sC, oY, oC)"""
    top = (1 << bitdepth) - 1
    if rng == "full":
        return top, top, 0, 1 << (bitdepth - 1)
    return 219 << (bitdepth - 8), 224 << (bitdepth - 8), 16 << (bitdepth - 8), 1 << (bitdepth - 1)


def exact_rows(matrix, rng, bitdepth):
    """-> (the forward rows, the inverse rows) as exact Fractions, as the module text states them"""
    kr, kb = MATRICES[matrix]
    kg = 1 - kr - kb
    top = (1 << bitdepth) - 1
    sy, sc, _, _ = scales(rng, bitdepth)
    fy, fcb, fcr = Fraction(sy, top), Fraction(sc) / (2 * (1 - kb) * top), Fraction(sc) / (2 * (1 - kr) * top)
    forward = ((fy * kr, fy * kg, fy * kb), (-fcb * kr, -fcb * kg, fcb * (1 - kb)), (fcr * (1 - kr), -fcr * kg, -fcr * kb))
    a, cb, cr = Fraction(top, sy), 2 * (1 - kb) * top / Fraction(sc), 2 * (1 - kr) * top / Fraction(sc)
    inverse = ((a, Fraction(0), cr), (a, -kb / kg * cb, -kr / kg * cr), (a, cb, Fraction(0)))
    return forward, inverse


@functools.lru_cache(maxsize=None)
def coefficients(matrix, rng, bitdepth):
    """-> (forward, inverse, offsets): two 3x3 tuples of Python ints (rows Y, Cb, Cr over R, G, B; rows R, G, B over Y, Cb,
    Cr) and (oY, oC, oC).  These integers are the format."""
    matrix, rng = check_colour((matrix, rng))
    check_bitdepth(bitdepth)
    one = 1 << FIXED_POINT_BITS
    exact_f, exact_i = exact_rows(matrix, rng, bitdepth)
    sy, _, oy, oc = scales(rng, bitdepth)
    sums = (round(Fraction(sy, (1 << bitdepth) - 1) * one), 0, 0)    # round() of a Fraction is half to even
    forward = []
    for row, total in zip(exact_f, sums):
        r, b = round(row[0] * one), round(row[2] * one)
        forward.append((r, total - r - b, b))
    inverse = tuple(tuple(round(c * one) for c in row) for row in exact_i)
    return tuple(forward), inverse, (oy, oc, oc)


def frame_bytes(layout, width, height):
    """bytes of a picture of width x height in an RGB layout"""
    _, depth, comps = check_rgb_layout(layout)
    pmctf_chroma.check_side(width, height)
    return width * height * comps * (1 if depth == 8 else 2)


# --------------------------------------------------------------------------------------------------------- the entries
def _tables(colour, bitdepth, forward):
    fwd, inv, off = coefficients(colour[0], colour[1], bitdepth)
    rows = fwd if forward else inv
    return (C.c_int32 * 9)(*[k for row in rows for k in row]), (C.c_int64 * 3)(*off)


def _call(forward, src, dst, code, h, w, bitdepth, colour):
    from pMCTF.hip import lib
    k, o = _tables(colour, bitdepth, forward)
    L = library()
    ps, pd = C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr())
    if bitdepth == 8:
        fn = L.pmctf_rgb_to_ycc_u8 if forward else L.pmctf_ycc_to_rgb_u8
        rc = fn(ps, pd, code, h, w, k, o, _stream())
    else:
        fn = L.pmctf_rgb_to_ycc_u16 if forward else L.pmctf_ycc_to_rgb_u16
        rc = fn(ps, pd, code, h, w, bitdepth, k, o, _stream())
    lib.check(rc, "rgb_to_ycc" if forward else "ycc_to_rgb")


def _need_device(t, what):
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: expect a tensor")
    if not t.is_cuda:
        raise RuntimeError("pmctf_colour runs on the GPU (no CPU fallback): pass device tensors")


def rgb_to_ycc(surface, layout, height, width, colour, out=None):
    """A surface in an RGB layout (1-D uint8 device tensor of frame_bytes bytes or more) -> the packed planar 4:4:4 picture:
    3 * height * width samples, uint8 at 8 bits and uint16 above.  One launch.  out: a contiguous tensor of that type and
    size to write into."""
    import torch
    code, depth, _ = check_rgb_layout(layout)
    colour = check_colour(colour)
    need = frame_bytes(layout, width, height)
    _need_device(surface, "surface")
    if surface.dtype != torch.uint8 or surface.dim() != 1 or surface.numel() < need or not surface.is_contiguous():
        raise ValueError(f"surface: expect a contiguous 1-D uint8 tensor of at least {need} bytes for {layout} {width}x{height}")
    dtype = torch.uint8 if depth == 8 else torch.uint16
    n = 3 * height * width
    if out is None:
        out = torch.empty(n, dtype=dtype, device=surface.device)
    elif out.dtype != dtype or out.numel() != n or not out.is_contiguous() or out.device != surface.device:
        raise ValueError(f"out: expect a contiguous {dtype} tensor of {n} samples on {surface.device}")
    _call(True, surface, out, code, height, width, depth, colour)
    return out


def ycc_to_rgb(frame, layout, height, width, colour, out=None):
    """The inverse: a packed planar 4:4:4 picture (uint8 at 8 bits, uint16 above, 3 * height * width samples) -> the
    surface's bytes (1-D uint8 tensor of frame_bytes).  One launch.  out: a contiguous uint8 tensor of that size."""
    import torch
    code, depth, _ = check_rgb_layout(layout)
    colour = check_colour(colour)
    need = frame_bytes(layout, width, height)
    _need_device(frame, "frame")
    dtype = torch.uint8 if depth == 8 else torch.uint16
    if frame.dtype != dtype or frame.numel() != 3 * height * width or not frame.is_contiguous():
        raise ValueError(f"frame: expect a contiguous {dtype} tensor of {3 * height * width} samples for {layout} "
                         f"{width}x{height}")
    if out is None:
        out = torch.empty(need, dtype=torch.uint8, device=frame.device)
    elif out.dtype != torch.uint8 or out.numel() != need or not out.is_contiguous() or out.device != frame.device:
        raise ValueError(f"out: expect a contiguous uint8 tensor of {need} bytes on {frame.device}")
    _call(False, frame, out, code, height, width, depth, colour)
    return out


class _RgbStep:
    """what RgbUnpacker and RgbPacker share: the attributes pmctf_layout.Unpacker / Packer have"""
    chroma_format = "444"

    def __init__(self, layout, width, height, colour, what="rgb_layout"):
        _, depth, _ = check_rgb_layout(layout, what)
        self.colour = check_colour(colour)
        pmctf_chroma.check_side(width, height)
        self.layout, self.size, self.shape, self.bitdepth = layout, (width, height), (height, width), depth
        self.frame_bytes = frame_bytes(layout, width, height)


class RgbUnpacker(_RgbStep):
    """Surfaces of width x height in an RGB layout -> packed planar 4:4:4 YCbCr pictures on the device, one launch each"""

    def __call__(self, surface, out=None):
        return rgb_to_ycc(surface, self.layout, self.shape[0], self.shape[1], self.colour, out=out)


class RgbPacker(_RgbStep):
    """The inverse: __call__(frame, out=None) -> the surface's bytes"""

    def __call__(self, frame, out=None):
        return ycc_to_rgb(frame, self.layout, self.shape[0], self.shape[1], self.colour, out=out)


class PngRgbReader:
    """pmctf_layout.PackedReader's interface over a PNG sequence (pmctf_gop.PNGReader): read_one_frame() gives a picture's
    rgb24 bytes, which pmctf_gop.read_gop_device uploads and converts with `unpack` (an RgbUnpacker of rgb24)"""
    truncated = False

    def __init__(self, paths_or_folder, unpack):
        import pmctf_gop
        assert unpack.layout == "rgb24"
        self._png = pmctf_gop.PNGReader(paths_or_folder)
        if (self._png.width, self._png.height) != unpack.size:
            raise ValueError(f"the pictures are {self._png.width}x{self._png.height}, not {unpack.size[0]}x{unpack.size[1]}")
        self.unpack = unpack
        self.width, self.height = unpack.size
        self.bitdepth, self.chroma_format = 8, "444"
        self.eof = False

    @property
    def current_frame_index(self):
        return self._png.current_frame_index

    def __len__(self):
        return len(self._png)

    def read_one_frame(self):
        pic = self._png.read_one_frame()
        self.eof = self._png.eof
        return None if pic is None else pic.reshape(-1)

    def close(self):
        self._png.close()
        self.eof = False


# ------------------------------------------------------------------------------------------------- colour_format.json
def _check_colour_record(path, record):
    if record["fixed_point_bits"] != FIXED_POINT_BITS or not is_int(record["fixed_point_bits"]):
        raise ValueError(f"{path}: fixed_point_bits {record['fixed_point_bits']!r}, this decoder knows {FIXED_POINT_BITS}")
    if not isinstance(record["matrix"], str) or record["matrix"] not in MATRICES:
        raise ValueError(f"{path}: matrix {record['matrix']!r}, one of {sorted(MATRICES)}")
    if not isinstance(record["range"], str) or record["range"] not in RANGES:
        raise ValueError(f"{path}: range {record['range']!r}, one of {RANGES}")
    if not isinstance(record["source"], str) or record["source"] not in SOURCES:
        raise ValueError(f"{path}: source {record['source']!r}, one of {SOURCES}")


def write_colour_format(bin_folder, colour, source):
    """bin_folder/colour_format.json: {"format_version", "matrix", "range", "fixed_point_bits", "source": "rgb" for a source
    that was RGB and was converted by this description, "ycbcr" for one the description only describes} -> the path"""
    matrix, rng = check_colour(colour)
    path = os.path.join(bin_folder, COLOUR_FORMAT)
    record = {"format_version": COLOUR_FORMAT_VERSION, "matrix": matrix, "range": rng, "fixed_point_bits": FIXED_POINT_BITS,
              "source": source}
    _check_colour_record(path, record)
    return write_record(path, record, indent=2)


def read_colour_format(bin_folder):
    """-> None when bin_folder has no colour_format.json, else its record; ValueError naming the path for a malformed file,
    another version or fixed_point_bits, an unknown or missing field, an unknown matrix, range or source"""
    path = os.path.join(bin_folder, COLOUR_FORMAT)
    record = read_record(path, "colour format file", COLOUR_FORMAT_VERSION, fields=COLOUR_FIELDS,
                         expected=sorted(COLOUR_FIELDS))
    if record is not None:
        _check_colour_record(path, record)
    return record


# ------------------------------------------------------------------------------------------------------------ encoding
class _RgbPipeline(pmctf_chroma.SourcePipeline):
    """the SourcePipeline of an RGB source: the planar 4:4:4 source's, with the RgbUnpacker as its layout step and, for a
    PNG sequence, the reader that hands out rgb24 bytes"""

    def __init__(self, source_size, chroma_loc, to420, size, unpack, png):
        super().__init__(source_size, "444", chroma_loc, to420, size, layout=unpack)
        self.png = png

    def open_reader(self, src_file, width, height, bitdepth=8):
        if self.png:
            return PngRgbReader(src_file, self.layout)
        return pmctf_layout.PackedReader(src_file, self.layout)


def _pipeline(source, width, height, frame_num, device, kwargs, coded_size, chroma_loc, chroma_format, pixel_layout, pitch,
              luma_rows, rgb_layout, colour, what, need_rate=False):
    """-> (the SourcePipeline or None, the (colour, source) to record or None).  Without rgb_layout, and without a PNG source
    that has a colour, the pipeline is pmctf_layout._pipeline's.  Every refusal is raised before the device is asked for."""
    import pmctf_gop
    import pmctf_scale
    png = kwargs.get("src_format", "yuv") == "png" and colour is not None and rgb_layout is None
    if rgb_layout is None and not png:
        if colour is not None:
            colour = check_colour(colour)
        pipeline = pmctf_layout._pipeline(source, width, height, device, kwargs, coded_size, chroma_format, chroma_loc,
                                          pixel_layout, pitch, luma_rows, what, need_rate)
        return pipeline, None if colour is None else (colour, "ycbcr")
    layout = "rgb24" if png else rgb_layout
    _, depth, _ = check_rgb_layout(layout)
    key = "src_format='png' with a colour" if png else f"rgb_layout {rgb_layout!r}"
    if not png and pmctf_chroma.is_y4m(source):
        raise ValueError(f"{key} with a .y4m source: Y4M pictures are YCbCr")
    if not png and kwargs.get("src_format", "yuv") != "yuv":
        raise ValueError(f"{key} with src_format {kwargs['src_format']!r}: rgb_layout describes a raw file "
                         f"(src_format='yuv'); a PNG sequence is rgb24 by itself")
    for name, given in (("pixel_layout", pixel_layout), ("pitch", pitch), ("luma_rows", luma_rows)):
        if given is not None:
            raise ValueError(f"{key} with {name} {given!r}: a pixel_layout describes YCbCr pictures")
    if chroma_format is not None and (png or chroma_format != "444"):
        raise ValueError(f"{key} with chroma_format {chroma_format!r}: RGB pictures are converted to '444'")
    if kwargs.get("bitdepth") is not None and kwargs["bitdepth"] != depth:
        raise ValueError(f"bitdepth {kwargs['bitdepth']!r} contradicts {key}, which has {depth} bits")
    colour = check_colour(DEFAULT_COLOUR if colour is None else colour)
    chroma_loc = pmctf_chroma.resolve_loc("444", chroma_loc)
    if need_rate:
        raise ValueError("fps=None takes the frame rate of a .y4m header; this source has none")
    pmctf_chroma.check_side(width, height, "source")
    unpack = RgbUnpacker(layout, width, height, colour)
    if png:
        reader = PngRgbReader(source, unpack)
        if len(reader) < frame_num:
            raise ValueError(f"{frame_num} frames asked for, {len(reader)} pictures found")
    else:
        nbytes = os.path.getsize(source)
        if nbytes % unpack.frame_bytes:
            raise ValueError(f"{source}: {nbytes} bytes are not a whole number of {rgb_layout} pictures of {width}x{height} "
                             f"({unpack.frame_bytes} bytes each; rgb_layout)")
    kwargs["bitdepth"] = depth
    kwargs["src_format"] = "yuv"                                # the reader is the pipeline's, PNGs included
    pmctf_gop._need_gpu(device, f"{what}({key})")
    size = None if coded_size is None else pmctf_scale.CodedSize(width, height, coded_size, device, depth, chroma_loc)
    to420 = pmctf_chroma.Converter(width, height, "444", "420", device, depth, chroma_loc)
    return _RgbPipeline((width, height), chroma_loc, to420, size, unpack, png), (colour, "rgb")


def encode_sequence(codec, yuv_path, width, height, frame_num, gop, q_index, bin_folder, device, *, coded_size=None,
                    chroma_loc=None, chroma_format=None, pixel_layout=None, pitch=None, luma_rows=None, rgb_layout=None,
                    colour=None, **kwargs):
    """pmctf_layout.encode_sequence with rgb_layout and colour.  rgb_layout (LAYOUTS): yuv_path holds RGB pictures; each is
    uploaded as its bytes and converted to 4:4:4 YCbCr by `colour` (default ("bt709", "limited")) in one launch, and from
    there the source is the planar 4:4:4 source of the layout's depth: the folder is the one that source codes to, plus
    colour_format.json (with keep_gops=True).  src_format="png" with a colour: the PNGs are rgb24 pictures of the same path
    (without a colour they take the harness's float formulas, as before).  A YCbCr source with a colour: the description
    is recorded in colour_format.json and nothing else changes.  ValueError, before the device is asked for, for rgb_layout
    with a .y4m, a pixel_layout, a chroma_format other than "444" or a contradicting bitdepth, for a file that is no whole
    number of pictures, and for an unknown matrix or range."""
    import pmctf_gop
    pipeline, record = _pipeline(yuv_path, width, height, frame_num, device, kwargs, coded_size, chroma_loc, chroma_format,
                                 pixel_layout, pitch, luma_rows, rgb_layout, colour, "encode_sequence")
    out = pmctf_gop._encode_equal_gops(codec, yuv_path, width, height, frame_num, gop, q_index, bin_folder, device,
                                       pipeline=pipeline, **kwargs)
    if record is not None and kwargs.get("keep_gops"):
        write_colour_format(bin_folder, *record)
    return out


def encode_sequence_gops(codec, source, width, height, frame_num, max_gop, q_index, bin_folder, device, *,
                         coded_size=None, chroma_loc=None, chroma_format=None, pixel_layout=None, pitch=None,
                         luma_rows=None, rgb_layout=None, colour=None, **kwargs):
    """pmctf_layout.encode_sequence_gops with rgb_layout / colour as encode_sequence above has them"""
    import pmctf_seq
    pipeline, record = _pipeline(source, width, height, frame_num, device, kwargs, coded_size, chroma_loc, chroma_format,
                                 pixel_layout, pitch, luma_rows, rgb_layout, colour, "encode_sequence_gops")
    out = pmctf_seq._encode_gop_list(codec, source, width, height, frame_num, max_gop, q_index, bin_folder, device,
                                     pipeline=pipeline, **kwargs)
    if record is not None:
        write_colour_format(bin_folder, *record)
    return out


def encode_sequence_rate(codec, source, width, height, frame_num, max_gop, bitrate, fps, bin_folder, device, *,
                         coded_size=None, chroma_loc=None, chroma_format=None, pixel_layout=None, pitch=None,
                         luma_rows=None, rgb_layout=None, colour=None, **kwargs):
    """pmctf_layout.encode_sequence_rate with rgb_layout / colour as encode_sequence above has them; an RGB source has no
    frame rate of its own, so fps=None is a ValueError"""
    import pmctf_rate
    pipeline, record = _pipeline(source, width, height, frame_num, device, kwargs, coded_size, chroma_loc, chroma_format,
                                 pixel_layout, pitch, luma_rows, rgb_layout, colour, "encode_sequence_rate",
                                 need_rate=fps is None)
    if fps is None:
        fps = pipeline.frame_rate
    out = pmctf_rate._encode_at_rate(codec, source, width, height, frame_num, max_gop, bitrate, fps, bin_folder, device,
                                     pipeline=pipeline, **kwargs)
    if record is not None:
        write_colour_format(bin_folder, *record)
    return out


# ------------------------------------------------------------------------------------------------------------ decoding
class RgbOutput:
    """A decode mode (what pmctf_gop.decode_sequence_with is parameterised by) around another: every hook is the wrapped
    mode's, and `taken`, which sees every GOP's pictures once they are verified, also writes them as RGB: through the
    folder's own picture sink (display size, source chroma format), to 4:4:4 by pmctf_chroma.Converter where they are not
    4:4:4 already, then one launch to the RGB layout.  rgb_out gets the layout's bytes, png_out 8-bit PNGs named by source
    index.  Works around pmctf_gop.FullDecode, pmctf_layers.LayerDecode (temporal and spatial levels) and
    pmctf_access.FrameDecode alike."""
    keeps = True

    def __init__(self, mode, codec, rgb_out, rgb_layout, colour, png_out, coded_size_output=False, coded_format_output=False):
        self.mode, self.codec, self.colour = mode, codec, check_colour(colour)
        self.rgb_out, self.rgb_layout, self.png_out = rgb_out, rgb_layout, png_out
        self.flags = (coded_size_output, coded_format_output)
        self._file = self._steps = None

    def __getattr__(self, name):                                # every other hook and attribute: the wrapped mode's
        return getattr(self.mode, name)

    @property
    def hash_level(self):
        return self.mode.hash_level

    def check_folder(self, bin_folder):
        import pmctf_gop
        self.mode.check_folder(bin_folder)
        self.bin_folder = bin_folder
        depth = pmctf_gop.read_picture_format(bin_folder)
        if self.rgb_layout is not None and LAYOUTS[self.rgb_layout][1] != depth:
            raise ValueError(f"rgb_layout {self.rgb_layout!r} holds pictures of {LAYOUTS[self.rgb_layout][1]} bits; the "
                             f"pictures of {bin_folder} have {depth} bits")
        if depth > 8 and self.png_out is not None:
            raise ValueError(f"{os.path.join(bin_folder, pmctf_gop.PICTURE_FORMAT)}: the pictures have {depth} bits, "
                             f"png_out writes 8-bit PNGs; decode to rgb_out")

    def picture_size(self, bin_folder, h, w, coded_size_output, coded_format_output):
        self.coded = (h, w)
        self.decoded = self.mode.picture_size(bin_folder, h, w, coded_size_output, coded_format_output)
        return self.decoded

    def _build(self, bitdepth):
        """-> (the sink, the step to 4:4:4 or None, the packer of rgb_out or None, the packer of the PNGs or None)"""
        import pmctf_gop
        dev = self.codec.engine().dev
        (h, w), (ph, pw) = self.coded, self.decoded
        sink = pmctf_gop.picture_sink(self.bin_folder, None, w, h, dev, bitdepth, *self.flags)
        if (ph, pw) != (h, w):
            sink = pmctf_chroma.output_format(self.bin_folder, None, pw, ph, None, dev, bitdepth, self.flags[1]) \
                or pmctf_gop.PlainSink(ph, pw, bitdepth)
        H, W = sink.shape
        fmt = getattr(sink, "chroma_format", "420")
        loc = getattr(sink, "chroma_loc", None) or (sink.up.chroma_loc if hasattr(sink, "up") else "center")
        to444 = None if fmt == "444" else pmctf_chroma.Converter(W, H, fmt, "444", dev, bitdepth, loc)
        pack = None if self.rgb_out is None else RgbPacker(self.rgb_layout, W, H, self.colour)
        png = None if self.png_out is None else RgbPacker("rgb24", W, H, self.colour)
        return sink, to444, pack, png

    def taken(self, source, frames, bitdepth):
        import pmctf_gop
        self.mode.taken(source, frames, bitdepth)
        if self._steps is None:
            self._steps = self._build(bitdepth)
            if self.rgb_out is not None:
                self._file = open(self.rgb_out, "wb")
        sink, to444, pack, png = self._steps
        pictures = sink.frames(frames)
        if to444 is not None:
            pictures = [to444(p) for p in pictures]
        surfaces = [(None if pack is None else pack(p), None if png is None else png(p)) for p in pictures]
        for t, (s, p) in zip(source, surfaces):
            if s is not None:
                self._file.write(s.cpu().numpy().tobytes(order="C"))
            if p is not None:
                pmctf_gop.write_pngs(self.png_out, t, [p.cpu().numpy().reshape(sink.shape[0], sink.shape[1], 3)])

    def close(self):
        if self._file is not None:
            self._file.close()
            self._file = None


def decode_with(mode, codec, bin_folder, yuv_out, device=None, png_out=None, verify="auto", *, coded_size_output=False,
                coded_format_output=False, output_layout=None, rgb_out=None, rgb_layout=None, colour=None):
    """pmctf_gop.decode_sequence_with for any decode mode, with RGB output: rgb_out (a file) and rgb_layout (LAYOUTS, of the
    folder's bit depth) go together; colour=None takes the description colour_format.json records.  With a description in
    force png_out (8 bits) writes its PNGs by it instead of the harness's formula.  ValueError, before the codec is looked
    at, for rgb_out without rgb_layout or the reverse, an unknown layout, matrix or range, rgb_out on a folder that records
    no description (naming the file) and a layout of another depth than the folder's (naming both)."""
    import pmctf_gop
    if (rgb_out is None) != (rgb_layout is None):
        raise ValueError(f"rgb_out and rgb_layout go together (got rgb_out {rgb_out!r}, rgb_layout {rgb_layout!r})")
    if rgb_layout is not None:
        check_rgb_layout(rgb_layout)
    if colour is not None:
        colour = check_colour(colour)
    plain = dict(coded_size_output=coded_size_output, coded_format_output=coded_format_output, output_layout=output_layout)
    if colour is None and (rgb_out is not None or png_out is not None):
        record = read_colour_format(bin_folder)
        if record is not None:
            colour = (record["matrix"], record["range"])
        elif rgb_out is not None:
            raise ValueError(f"{os.path.join(bin_folder, COLOUR_FORMAT)}: missing (rgb_out needs the colour description of "
                             f"the pictures: give colour=(matrix, range))")
    if colour is None or (rgb_out is None and png_out is None):
        return pmctf_gop.decode_sequence_with(mode, codec, bin_folder, yuv_out, device, png_out, verify, **plain)
    wrapped = RgbOutput(mode, codec, rgb_out, rgb_layout, colour, png_out, coded_size_output, coded_format_output)
    try:
        return pmctf_gop.decode_sequence_with(wrapped, codec, bin_folder, yuv_out, device, None, verify, **plain)
    finally:
        wrapped.close()


def decode_sequence_checked(codec, bin_folder, yuv_out, device=None, png_out=None, verify="auto", coded_size_output=False,
                            coded_format_output=False, output_layout=None, rgb_out=None, rgb_layout=None, colour=None):
    """pmctf_layout.decode_sequence_checked with rgb_out / rgb_layout / colour as decode_with has them: the verified pictures
    are also written to rgb_out as the layout's bytes.  The hashes are those of the coded 4:2:0 pictures and are verified
    first.  Without the three keywords, on a folder without colour_format.json: pmctf_layout.decode_sequence_checked."""
    import pmctf_gop
    return decode_with(pmctf_gop.FullDecode(), codec, bin_folder, yuv_out, device, png_out, verify,
                       coded_size_output=coded_size_output, coded_format_output=coded_format_output,
                       output_layout=output_layout, rgb_out=rgb_out, rgb_layout=rgb_layout, colour=colour)


def decode_sequence_layer(codec, bin_folder, yuv_out, level, device=None, png_out=None, verify="auto", motion_fill=False,
                          coded_size_output=False, coded_format_output=False, output_layout=None, rgb_out=None,
                          rgb_layout=None, colour=None):
    """pmctf_layout.decode_sequence_layer with rgb_out / rgb_layout / colour as decode_sequence_checked above has them"""
    import pmctf_layers
    return decode_with(pmctf_layers.LayerDecode(level, motion_fill), codec, bin_folder, yuv_out, device, png_out, verify,
                       coded_size_output=coded_size_output, coded_format_output=coded_format_output,
                       output_layout=output_layout, rgb_out=rgb_out, rgb_layout=rgb_layout, colour=colour)


# ---------------------------------------------------------------------------------------------------------- conversion
def convert_file(src, dst, width, height, from_layout, to_layout, colour, device, bitdepth=None):
    """A file of pictures in an RGB layout -> the same pictures as planar 4:4:4 YCbCr ("planar444": bytes at 8 bits,
    little-endian words above), or the reverse, converted on the device by `colour`.  One side is an RGB layout, the other
    "planar444"; bitdepth, when given, must be the layout's.  -> the number of pictures.  The counterpart of
    pmctf_layout.convert_file."""
    import numpy as np
    import torch
    import pmctf_gop
    if (from_layout == PLANAR444) == (to_layout == PLANAR444):
        raise ValueError(f"one of from_layout and to_layout is {PLANAR444!r}, the other an RGB layout (got {from_layout!r}, "
                         f"{to_layout!r})")
    forward = to_layout == PLANAR444
    layout = from_layout if forward else to_layout
    _, depth, _ = check_rgb_layout(layout, "from_layout" if forward else "to_layout")
    if bitdepth is not None and bitdepth != depth:
        raise ValueError(f"bitdepth {bitdepth!r} contradicts {layout!r}, which has {depth} bits")
    colour = check_colour(colour)
    step = (RgbUnpacker if forward else RgbPacker)(layout, width, height, colour)
    planar_bytes = 3 * width * height * (1 if depth == 8 else 2)
    in_bytes = step.frame_bytes if forward else planar_bytes
    nbytes = os.path.getsize(src)
    if nbytes == 0 or nbytes % in_bytes:
        raise ValueError(f"{src}: {nbytes} bytes are not a whole number of {from_layout} pictures of {width}x{height} "
                         f"({in_bytes} bytes each)")
    pmctf_gop._need_gpu(device, "convert_file")
    with open(src, "rb") as fin, open(dst, "wb") as fout:
        for _ in range(nbytes // in_bytes):
            data = torch.from_numpy(np.fromfile(fin, dtype=np.uint8, count=in_bytes)).to(device)
            out = step(data if forward or depth == 8 else data.view(torch.uint16))
            fout.write(out.cpu().numpy().tobytes(order="C"))
    return nbytes // in_bytes
