"""Reduced-resolution coding: pictures are resampled on the device, in and out of the codec, by one exact
integer filter, so that a sequence can be coded at another size than its source has.

The filter is the separable Catmull-Rom bicubic (a = -1/2) with an antialiasing stretch, the definition of Pillow's BICUBIC
and of torch's interpolate(mode="bicubic", antialias=True, align_corners=False), with 14-bit integer coefficients.  For one
axis of n_in -> n_out samples and a phase offset `phase`, in exact rationals:

    scale = n_in / n_out, fs = max(scale, 1), support = 2 fs
    c     = scale (i + 1/2) + phase                          centre of output i
    xmin  = max(int(c - support + 1/2), 0), xmax = min(int(c + support + 1/2), n_in)
    w_j   = w((j - c + 1/2) / fs) / sum, j = xmin .. xmax - 1  (the window is clipped at the edge and renormalised)
    q_j   = floor(w_j 16384 + 1/2), and 16384 - sum q is added to the largest q_j (the first of equals)

A plane of b-bit samples goes through the horizontal pass t = (sum q x + 32) >> 6 and the vertical pass
out = clamp((sum q t + 2^21) >> 22, 0, 2^b - 1), all in integers (csrc/picture_scale.hip: one launch per picture).

This module holds the tables (axis_table, cached, uploaded once per device), the display_format.json header, the
Resampler that applies the kernel to packed 4:2:0 pictures, and the entry points that code and decode a sequence at a
coded size: encode_sequence, encode_sequence_gops, encode_sequence_rate, decode_sequence_checked, decode_sequence_layer.
They are pmctf_gop's, pmctf_seq's, pmctf_rate's and pmctf_layers' functions with the keywords coded_size / chroma_loc
(encoding; what follows `device` is given by keyword) and coded_size_output (decoding) added; with coded_size=None they
are those functions."""
import functools
import os
from fractions import Fraction

from pmctf_records import is_int, read_record, write_record

COEF_BITS = 14
COEF_ONE = 1 << COEF_BITS
MAX_SIDE = 16384
MAX_RATIO = 4
FILTER = "catmull-rom-aa/14"
CHROMA_LOCS = ("center", "left")
DISPLAY_FORMAT = "display_format.json"
DISPLAY_FORMAT_VERSION = 1
DISPLAY_FIELDS = ("format_version", "width", "height", "filter", "chroma_loc")


def catmull_rom(x):
    """the cubic convolution kernel with a = -1/2, on a Fraction"""
    x = abs(x)
    if x < 1:
        return (Fraction(3, 2) * x - Fraction(5, 2)) * x * x + 1
    if x < 2:
        return ((Fraction(-1, 2) * x + Fraction(5, 2)) * x - 4) * x + 2
    return Fraction(0)


@functools.lru_cache(maxsize=64)
def axis_table(n_in, n_out, phase=Fraction(0)):
    """-> (start: tuple of n_out ints, coef: tuple of n_out tuples of T ints, T) of one axis, as the module text defines
    them; rows shorter than T are zero-filled.  Cached per (n_in, n_out, phase)."""
    if not is_int(n_in) or not is_int(n_out) or n_in < 1 or n_out < 1:
        raise ValueError(f"an axis has positive integer lengths (got {n_in!r} -> {n_out!r})")
    phase = Fraction(phase)
    half = Fraction(1, 2)
    scale = Fraction(n_in, n_out)
    fs = max(scale, Fraction(1))
    support = 2 * fs
    starts, rows = [], []
    for i in range(n_out):
        c = scale * (i + half) + phase
        xmin = max(int(c - support + half), 0)
        xmax = min(int(c + support + half), n_in)
        w = [catmull_rom((j - c + half) / fs) for j in range(xmin, xmax)]
        total = sum(w)
        q = [(wj / total * COEF_ONE + half).__floor__() for wj in w]
        q[q.index(max(q))] += COEF_ONE - sum(q)
        starts.append(xmin)
        rows.append(q)
    taps = max(len(q) for q in rows)
    return tuple(starts), tuple(tuple(q) + (0,) * (taps - len(q)) for q in rows), taps


def chroma_phase(n_in, n_out, chroma_loc):
    """horizontal phase of the chroma planes: 0 for samples centred in their 2x2 luma block, scale/4 - 1/4 for MPEG-2
    siting (chroma on the left luma column)"""
    if chroma_loc not in CHROMA_LOCS:
        raise ValueError(f"chroma_loc is one of {CHROMA_LOCS} (got {chroma_loc!r})")
    return Fraction(0) if chroma_loc == "center" else (Fraction(n_in, n_out) - 1) / 4


def check_sizes(src_w, src_h, dst_w, dst_h, what="size"):
    """both sizes even, positive, at most MAX_SIDE a side, and dst / src within [1/4, 4] on each axis; ValueError"""
    for n in (src_w, src_h, dst_w, dst_h):
        if not is_int(n) or n <= 0 or n & 1 or n > MAX_SIDE:
            raise ValueError(f"{what}: 4:2:0 pictures have even, positive sides up to {MAX_SIDE} "
                             f"(got {src_w!r}x{src_h!r} and {dst_w!r}x{dst_h!r})")
    for a, b in ((src_w, dst_w), (src_h, dst_h)):
        if MAX_RATIO * b < a or b > MAX_RATIO * a:
            raise ValueError(f"{what}: {src_w}x{src_h} and {dst_w}x{dst_h} differ by more than a factor of {MAX_RATIO} "
                             f"on an axis")


def parse_size(text):
    """"WxH" -> (W, H) positive even integers; ValueError otherwise"""
    parts = str(text).lower().split("x")
    if len(parts) != 2 or not all(p.isdigit() for p in parts):
        raise ValueError(f"a size is WxH, two positive integers (got {text!r})")
    w, h = int(parts[0]), int(parts[1])
    if w <= 0 or h <= 0 or (w | h) & 1:
        raise ValueError(f"a 4:2:0 size is even and positive (got {text!r})")
    return w, h


# ------------------------------------------------------------------------------------------------------------ the header
def write_display_format(bin_folder, width, height, chroma_loc="center"):
    """bin_folder/display_format.json: {"format_version", "width", "height": the size the decoded pictures are shown at (the
    source's), "filter", "chroma_loc"}.  Written only for a sequence coded at another size than its source's."""
    path = os.path.join(bin_folder, DISPLAY_FORMAT)
    record = {"format_version": DISPLAY_FORMAT_VERSION, "width": width, "height": height, "filter": FILTER,
              "chroma_loc": chroma_loc}
    _check_display_record(path, record)
    return write_record(path, record, indent=2)


def _check_display_record(path, record, coded=None):
    if record["filter"] != FILTER:
        raise ValueError(f"{path}: filter {record['filter']!r}, this decoder knows {FILTER!r}")
    if record["chroma_loc"] not in CHROMA_LOCS:
        raise ValueError(f"{path}: chroma_loc {record['chroma_loc']!r}, one of {CHROMA_LOCS}")
    w, h = record["width"], record["height"]
    for n in (w, h):
        if not is_int(n) or n <= 0 or n & 1 or n > MAX_SIDE:
            raise ValueError(f"{path}: width and height are even, positive integers up to {MAX_SIDE} (got {w!r}x{h!r})")
    if coded is not None:
        try:
            check_sizes(coded[0], coded[1], w, h, what=path)
        except ValueError as e:
            raise ValueError(str(e)) from None


def read_display_format(bin_folder, coded_width=None, coded_height=None):
    """-> None when bin_folder has no display_format.json (the pictures are shown as coded), else its record; ValueError
    naming the path for a malformed file, another version or filter, an unknown or missing field, a size that is not even
    and positive, and, when the coded size is given, a display size more than a factor of 4 from it"""
    path = os.path.join(bin_folder, DISPLAY_FORMAT)
    record = read_record(path, "display format file", DISPLAY_FORMAT_VERSION, fields=DISPLAY_FIELDS,
                         expected=sorted(DISPLAY_FIELDS))
    if record is not None:
        _check_display_record(path, record, None if coded_width is None else (coded_width, coded_height))
    return record


# --------------------------------------------------------------------------------------------------------- on the device
_device_tables = {}


def device_table(n_in, n_out, phase, device):
    """the axis table as the kernel reads it, uploaded once per (n_in, n_out, phase, device): int32 start[n_out], then
    int16 coef[n_out][T] -> (uint8 device tensor, T)"""
    import numpy as np
    import torch
    key = (n_in, n_out, Fraction(phase), str(torch.device(device)))
    if key not in _device_tables:
        start, coef, taps = axis_table(n_in, n_out, Fraction(phase))
        raw = np.asarray(start, dtype="<i4").tobytes() + np.asarray(coef, dtype="<i2").tobytes()
        _device_tables[key] = (torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device), taps)
    return _device_tables[key]


class Resampler:
    """Packed planar 4:2:0 pictures of src_w x src_h -> dst_w x dst_h on the device: __call__(frame) takes the picture as
    it lies in a file (uint8 tensor of h*w*3/2 bytes at bitdepth 8, uint16 above) and returns the resampled one, one launch
    (ops.resize_yuv420).  The four tables are built and uploaded here, once."""

    def __init__(self, src_w, src_h, dst_w, dst_h, device, bitdepth=8, chroma_loc="center"):
        check_sizes(src_w, src_h, dst_w, dst_h)
        if not is_int(bitdepth) or not 8 <= bitdepth <= 16:
            raise ValueError(f"bitdepth is 8 or 9..16 (got {bitdepth!r})")
        self.src, self.dst = (src_w, src_h), (dst_w, dst_h)
        self.bitdepth, self.chroma_loc, self.device = bitdepth, chroma_loc, device
        phase = chroma_phase(src_w // 2, dst_w // 2, chroma_loc)
        self.tables = (device_table(src_w, dst_w, 0, device), device_table(src_h, dst_h, 0, device),
                       device_table(src_w // 2, dst_w // 2, phase, device), device_table(src_h // 2, dst_h // 2, 0, device))

    def __call__(self, frame):
        from pMCTF.hip import ops
        return ops.resize_yuv420(frame, self.src[1], self.src[0], self.dst[1], self.dst[0],
                                 [t for t, _ in self.tables], [n for _, n in self.tables], self.bitdepth)


def pack_frame(rec_y, rec_c, h, w, bitdepth=8):
    """a reconstructed (padded, float) picture -> the packed integer picture of its un-padded size, on the device, as
    frames_to_u8 / frames_to_u16 round it"""
    import torch
    from pMCTF.hip import ops
    y = ops.planes_to(rec_y.contiguous(), h, w, bitdepth)
    c = ops.planes_to(rec_c.contiguous(), h // 2, w // 2, bitdepth)
    return torch.cat([y.reshape(-1), c.reshape(-1)])


def unpack_frame(frame, h, w, bitdepth=8):
    """a packed picture on the device -> (Y, Cb, Cr) numpy arrays, the planes write_yuv writes"""
    host = frame.cpu().numpy()
    hc, wc = h // 2, w // 2
    return (host[:h * w].reshape(h, w), host[h * w:h * w + hc * wc].reshape(hc, wc), host[h * w + hc * wc:].reshape(hc, wc))


class _Ingest:
    """The `resample` hook of a reader (pmctf_gop.read_gop_device applies it to every packed picture after upload): to
    4:2:0 first (to420: a pmctf_chroma.Converter or None), then to the coded size (size: a CodedSize or None), which with
    keep also keeps the 4:2:0 source picture for its display_quality.  shape: (height, width) of what comes out."""

    def __init__(self, to420, size, keep, shape):
        self.to420, self.size, self.keep, self.shape = to420, size, keep, shape

    def __call__(self, frame):
        if self.to420 is not None:
            frame = self.to420(frame)
        if self.size is None:
            return frame
        if self.keep:
            self.size.sources.append(frame)
        return self.size.down(frame)


class CodedSize:
    """The "to coded size" step of a source's way into the codec (pmctf_chroma.SourcePipeline), for a 4:2:0 source of
    width x height coded at coded_size = (W, H): the two Resamplers, the source pictures kept for the display quality of a
    reconstructed GOP, and the header."""

    def __init__(self, width, height, coded_size, device, bitdepth=8, chroma_loc="center"):
        try:
            cw, ch = coded_size
        except (TypeError, ValueError):
            raise ValueError(f"coded_size is (width, height) (got {coded_size!r})") from None
        check_sizes(width, height, cw, ch, what="coded_size")
        chroma_phase(2, 2, chroma_loc)
        self.source, self.coded = (width, height), (cw, ch)
        self.bitdepth, self.chroma_loc = bitdepth, chroma_loc
        self.down = Resampler(width, height, cw, ch, device, bitdepth, chroma_loc)
        self.up = Resampler(cw, ch, width, height, device, bitdepth, chroma_loc)
        self.sources = []

    def ingest(self, keep):
        """the `resample` attribute of a reader (pmctf_gop.read_gop_device): frame -> coded-size frame; keep=True also
        keeps the source picture for display_quality"""
        return _Ingest(None, self, keep, self.coded[::-1])

    def write_header(self, bin_folder):
        return write_display_format(bin_folder, self.source[0], self.source[1], self.chroma_loc)

    def display_quality(self, rec):
        """rec: the reconstructed pictures of the next len(rec) source pictures kept by ingest(keep=True) -> per picture
        {"display_psnr_y", "_cb", "_cr", "_yuv"}: the integer reconstruction resampled to the source's size against the
        source, through frame_quality (8 bit) or frame_sse_hbd"""
        import pmctf_gop
        from pMCTF.hip import ops
        (W, H), (cw, ch), b = self.source, self.coded, self.bitdepth
        sources, self.sources = self.sources[:len(rec)], self.sources[len(rec):]
        assert len(sources) == len(rec), "a reconstructed picture without its source"
        planes = lambda f: ops.planes_from(f, H, W, b, psize=2)
        out = []
        for (rec_y, rec_c, *_), src in zip(rec, sources):
            y, c, _, _ = planes(self.up(pack_frame(rec_y, rec_c, ch, cw, b)))
            _, _, oy, oc = planes(src)
            q = (pmctf_gop.gop_quality_hbd([(y, c, None)], [(oy, oc)], H, W, b) if b > 8 else
                 pmctf_gop.gop_quality([(y, c, None)], [(oy, oc)], H, W, msssim=False))[0]
            out.append({f"display_psnr_{k}": q[k] for k in ("y", "cb", "cr", "yuv")})
        return out


class DisplaySize:
    """What the decoders need to write the pictures of a folder with a display_format.json at their display size: the
    picture sink (pmctf_gop.picture_sink) of raw 4:2:0 output at that size."""
    stream_header = frame_marker = b""

    def __init__(self, record, coded_width, coded_height, device, bitdepth=8):
        self.size = (record["width"], record["height"])
        self.shape = self.size[::-1]
        self.coded = (coded_width, coded_height)
        self.bitdepth = bitdepth
        self.up = Resampler(coded_width, coded_height, record["width"], record["height"], device, bitdepth,
                            record["chroma_loc"])

    def frames(self, frames_rec):
        """reconstructed (padded, float) pictures -> the packed display-size pictures, on the device"""
        (cw, ch) = self.coded
        return [self.up(pack_frame(rec[0], rec[1], ch, cw, self.bitdepth)) for rec in frames_rec]

    def pictures(self, frames_rec):
        """-> [(Y, Cb, Cr)] integer arrays of the display size: what frames_to_u8 / frames_to_u16 give for the coded size"""
        return [unpack_frame(f, self.size[1], self.size[0], self.bitdepth) for f in self.frames(frames_rec)]

    def rgb8(self, frames_rec):
        """-> [(H, W, 3) uint8 RGB arrays] of the display size (frames_to_rgb8 of the resampled 8-bit pictures)"""
        from pMCTF.hip import ops
        W, H = self.size
        out = []
        for f in self.frames(frames_rec):
            y, c, _, _ = ops.planes_from_u8(f, H, W, psize=2, originals=False)
            out.append(ops.frame_to_rgb8(y, c, H, W))
        return [rgb.cpu().numpy() for rgb in out]


def display_size(bin_folder, coded_width, coded_height, device, bitdepth=8, coded_size_output=False):
    """-> the DisplaySize of a folder, or None when it has no display_format.json or the coded-size pictures are asked for
    (the file is validated either way)"""
    record = read_display_format(bin_folder, coded_width, coded_height)
    if record is None or coded_size_output:
        return None
    return DisplaySize(record, coded_width, coded_height, device, bitdepth)


def _pipeline(width, height, coded_size, device, bitdepth, chroma_loc, what):
    """-> the pmctf_chroma.SourcePipeline of a 4:2:0 source coded at coded_size; None (no pipeline: the source enters the
    codec as it is) without one"""
    import pmctf_gop
    if coded_size is None:
        chroma_phase(2, 2, chroma_loc)
        return None
    import pmctf_chroma
    pmctf_gop._need_gpu(device, f"{what}(coded_size={coded_size!r})")
    size = CodedSize(width, height, coded_size, device, pmctf_gop.check_bitdepth(bitdepth), chroma_loc)
    return pmctf_chroma.SourcePipeline((width, height), chroma_loc=chroma_loc, size=size)


# ---------------------------------------------------------------------------------------------------------- entry points
def encode_sequence(codec, yuv_path, width, height, frame_num, gop, q_index, bin_folder, device, *, coded_size=None,
                    chroma_loc="center", **kwargs):
    """pmctf_gop.encode_sequence with coded_size=(W, H): every picture of the width x height source is resampled on the
    device directly after upload (after the conversion to 4:2:0 for PNGs) and everything downstream sees a source of W x H:
    the files, sequence.json, the hashes and the quality tables are those of coding the resampled pictures.  With
    keep_gops=True the folder also gets display_format.json.  The result gains "display_quality": per picture
    {"display_psnr_y", "display_psnr_cb", "display_psnr_cr", "display_psnr_yuv"}, the integer reconstruction resampled back
    to width x height against the source.  chroma_loc: "center" (what the RGB conversion here produces) or "left".
    coded_size=None: pmctf_gop.encode_sequence itself."""
    import pmctf_gop
    pipeline = _pipeline(width, height, coded_size, device, kwargs.get("bitdepth", 8), chroma_loc, "encode_sequence")
    return pmctf_gop._encode_equal_gops(codec, yuv_path, width, height, frame_num, gop, q_index, bin_folder, device,
                                        pipeline=pipeline, **kwargs)


def encode_sequence_gops(codec, source, width, height, frame_num, max_gop, q_index, bin_folder, device, *,
                         coded_size=None, chroma_loc="center", **kwargs):
    """pmctf_seq.encode_sequence_gops with coded_size / chroma_loc as encode_sequence above has them; gop_structure.json
    carries the coded size and the folder gets display_format.json.  The scene-cut pass looks at the resampled pictures."""
    import pmctf_seq
    pipeline = _pipeline(width, height, coded_size, device, kwargs.get("bitdepth", 8), chroma_loc, "encode_sequence_gops")
    return pmctf_seq._encode_gop_list(codec, source, width, height, frame_num, max_gop, q_index, bin_folder, device,
                                      pipeline=pipeline, **kwargs)


def encode_sequence_rate(codec, source, width, height, frame_num, max_gop, bitrate, fps, bin_folder, device, *,
                         coded_size=None, chroma_loc="center", **kwargs):
    """pmctf_rate.encode_sequence_rate with coded_size / chroma_loc as encode_sequence above has them: the way to a
    bitrate below what the coarsest q_index reaches at the source's size."""
    import pmctf_rate
    pipeline = _pipeline(width, height, coded_size, device, kwargs.get("bitdepth", 8), chroma_loc, "encode_sequence_rate")
    return pmctf_rate._encode_at_rate(codec, source, width, height, frame_num, max_gop, bitrate, fps, bin_folder, device,
                                      pipeline=pipeline, **kwargs)


def decode_sequence_checked(codec, bin_folder, yuv_out, device=None, png_out=None, verify="auto", coded_size_output=False):
    """pmctf_gop.decode_sequence_checked with the choice of the output size for a folder with a display_format.json:
    coded_size_output=True writes the pictures as they were coded (the ones the picture hashes describe) instead of
    resampling them to the display size."""
    import pmctf_gop
    return pmctf_gop.decode_sequence_with(pmctf_gop.FullDecode(), codec, bin_folder, yuv_out, device, png_out, verify,
                                          coded_size_output=coded_size_output)


def decode_sequence_layer(codec, bin_folder, yuv_out, level, device=None, png_out=None, verify="auto", motion_fill=False,
                          coded_size_output=False):
    """pmctf_layers.decode_sequence_layer with coded_size_output as decode_sequence_checked above has it"""
    import pmctf_gop
    import pmctf_layers
    return pmctf_gop.decode_sequence_with(pmctf_layers.LayerDecode(level, motion_fill), codec, bin_folder, yuv_out, device,
                                          png_out, verify, coded_size_output=coded_size_output)
