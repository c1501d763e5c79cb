"""Pixel layouts: sources and outputs that are not planar.  Decoder surfaces (NV12, P010, P016), raw dumps
(nv12, p010le, yuyv422, uyvy422, y210le) and capture files (v210, UYVY) are unpacked on the device into the packed planar
picture of their chroma format directly after upload, and decoded pictures are packed on the device directly before they are
written.  Everything between is pmctf_chroma's: a layout is one more step in front of SourcePipeline's format and size
steps, and one more behind the decoders' picture sink.  The arithmetic is bit movement and exact.

name    chroma  depth  bytes of a picture of w x h ("word": little-endian 16 bits, a sample v stored as v << (16 - depth))
nv12    420     8      h rows of w Y bytes, then h/2 rows of w bytes Cb0 Cr0 Cb1 Cr1 ..
nv21    420     8      nv12 with Cr first
nv16    422     8      h rows of Y, then h rows of w bytes Cb Cr ..
p010 p012 p016  420  10 12 16   nv12 in words
p210 p212 p216  422  10 12 16   nv16 in words
yuyv    422     8      rows of 2w bytes Y0 Cb Y1 Cr per pixel pair
uyvy    422     8      Cb Y0 Cr Y1
y210 y212 y216  422  10 12 16   yuyv in words
v210    422     10     six pixels in four little-endian 32-bit words of three 10-bit values (bits 0-9, 10-19, 20-29):
                       (Cb0, Y0, Cr0) (Y1, Cb1, Y2) (Cr1, Y3, Cb2) (Y4, Cr2, Y5); a row is ((w + 47) // 48) * 128 bytes, the
                       rest of it zero

A row takes `pitch` bytes: by default its own (for v210 the 128-byte multiple, which is part of the format), else a
multiple of the container (1, 2; 4 for v210) up to 2^20.  The chroma plane of a semi-planar layout has the same pitch and
starts at pitch * luma_rows, luma_rows from h (the default) to 2^17: the aligned heights decoders allocate.  frame_bytes is
the offset of the last row's end; pictures follow each other in a file at that distance.  luma_rows is validated for every
layout and used by the semi-planar ones.

Nothing new is recorded in a folder: the layout belongs to the file at hand, not to the coded sequence, and the decoder is
told its output layout.  Out of scope: 4:4:4 packed forms (AYUV, Y410), NV24, big-endian words, tiled surfaces."""
import os

import pmctf_chroma
from pMCTF.hip import ops as _ops

FAMILIES = ("semi", "pair", "v210")
LAYOUTS = {name: {"chroma_format": fmt, "bitdepth": depth, "container": container, "family": family}
           for name, (_, fmt, depth, container, family) in _ops.LAYOUTS.items()}
MAX_PITCH, MAX_LUMA_ROWS = _ops.LAYOUT_MAX_PITCH, _ops.LAYOUT_MAX_LUMA_ROWS
PLANAR = "planar"


def check_layout(layout, what="pixel_layout"):
    """-> LAYOUTS[layout]; ValueError naming `what` otherwise"""
    if not isinstance(layout, str) or layout not in LAYOUTS:
        raise ValueError(f"{what} is one of {sorted(LAYOUTS)} (got {layout!r})")
    return LAYOUTS[layout]


def default_pitch(layout, width):
    check_layout(layout)
    return _ops.layout_row_bytes(layout, width)


def frame_bytes(layout, width, height, pitch=None, luma_rows=None):
    """bytes from the start of a picture to the end of its last row; ValueError naming pitch or luma_rows outside the rules"""
    check_layout(layout)
    pmctf_chroma.check_side(width, height)
    return _ops.layout_geometry(layout, height, width, None, pitch, luma_rows)[2]


class _Step:
    """what Unpacker and Packer share: the checked geometry of pictures of width x height in `layout`"""

    def __init__(self, layout, width, height, pitch=None, luma_rows=None, what="pixel_layout"):
        info = check_layout(layout, what)
        pmctf_chroma.check_side(width, height)
        self.layout, self.size, self.shape = layout, (width, height), (height, width)
        self.chroma_format, self.bitdepth = info["chroma_format"], info["bitdepth"]
        self.pitch, self.luma_rows, self.frame_bytes = _ops.layout_geometry(layout, height, width, None, pitch, luma_rows)


class Unpacker(_Step):
    """Surfaces of width x height in `layout` -> packed planar pictures of its chroma format on the device: __call__(surface)
    takes a 1-D uint8 device tensor of frame_bytes bytes (or more), one launch (ops.unpack_layout).  Built once per
    sequence, like pmctf_chroma.Converter."""

    def __call__(self, surface, out=None):
        return _ops.unpack_layout(surface, self.layout, self.shape[0], self.shape[1], self.bitdepth, self.pitch,
                                  self.luma_rows, out=out)


class Packer(_Step):
    """The inverse: __call__(frame, out=None) -> the surface's bytes (ops.pack_layout); with out, nothing outside the rows
    is written."""

    def __call__(self, frame, out=None):
        return _ops.pack_layout(frame, self.layout, self.shape[0], self.shape[1], self.bitdepth, self.pitch, self.luma_rows,
                                out=out)


class PackedReader:
    """YUVReader's interface for a file of pictures in a pixel layout: read_one_frame() gives the next picture's raw bytes (a
    uint8 array of unpack.frame_bytes), which pmctf_gop.read_gop_device uploads and unpacks with `unpack` (the Unpacker it
    carries).  len(): the whole pictures of the file; truncated: the file ends inside a picture, which raises when that
    picture is read, as YUVReader does."""

    def __init__(self, src_file, unpack, start_index=0):
        if not os.path.exists(src_file):
            raise AssertionError(f"no such sequence: {src_file}")
        self.src_file, self.unpack = src_file, unpack
        self.width, self.height = unpack.size
        self.bitdepth, self.chroma_format = unpack.bitdepth, unpack.chroma_format
        self.current_frame_index = int(start_index)
        self.eof = False
        self._fh = None
        size = os.path.getsize(src_file)
        self._frames = size // unpack.frame_bytes
        self.truncated = size != self._frames * unpack.frame_bytes

    def __len__(self):
        return self._frames

    def read_one_frame(self):
        import numpy as np
        if self.eof:
            return None
        assert self.current_frame_index < self._frames, "sequence ends inside a picture"
        if self._fh is None:
            self._fh = open(self.src_file, "rb")
        self._fh.seek(self.current_frame_index * self.unpack.frame_bytes)
        data = np.fromfile(self._fh, dtype=np.uint8, count=self.unpack.frame_bytes)
        assert data.size == self.unpack.frame_bytes, "sequence ends inside a picture"
        self.current_frame_index += 1
        return data

    def close(self):
        if self._fh is not None:
            self._fh.close()
            self._fh = None
        self.current_frame_index = 0


class SurfaceReader:
    """The same interface over an iterable of 1-D uint8 tensors that already lie in GPU memory (a decoder's surfaces):
    read_gop_device(SurfaceReader(frames, "nv12", w, h, pitch, luma_rows), gop, device) gives the triple encode_gop takes
    without a trip through the host.  read_one_frame() is None past the end."""
    truncated = False

    def __init__(self, frames, layout, width, height, pitch=None, luma_rows=None):
        self.unpack = Unpacker(layout, width, height, pitch, luma_rows)
        self.width, self.height = width, height
        self.bitdepth, self.chroma_format = self.unpack.bitdepth, self.unpack.chroma_format
        self._frames = frames
        self._it = iter(frames)
        self.current_frame_index = 0
        self.eof = False

    def __len__(self):
        return len(self._frames)

    def read_one_frame(self):
        frame = next(self._it, None)
        if frame is None:
            self.eof = True
            return None
        self.current_frame_index += 1
        return frame

    def close(self):
        self._it = iter(self._frames)
        self.current_frame_index = 0
        self.eof = False


# ------------------------------------------------------------------------------------------------------------ encoding
def _pipeline(source, width, height, device, kwargs, coded_size, chroma_format, chroma_loc, pixel_layout, pitch, luma_rows,
              what, need_rate=False):
    """-> the SourcePipeline of the source (None where it has none).  Without a pixel_layout this is pmctf_chroma._pipeline.
    With one the pipeline starts with the layout's Unpacker, the bit depth is the layout's (written into kwargs), and every
    refusal is raised before the device is asked for."""
    import pmctf_gop
    import pmctf_scale
    if pixel_layout is None:
        for name, given in (("pitch", pitch), ("luma_rows", luma_rows)):
            if given is not None:
                raise ValueError(f"{name} describes a pixel_layout, and none is given")
        return pmctf_chroma._pipeline(source, width, height, device, kwargs, coded_size, chroma_format, chroma_loc, what,
                                      need_rate)
    info = check_layout(pixel_layout)
    if pmctf_chroma.is_y4m(source):
        raise ValueError(f"pixel_layout {pixel_layout!r} with a .y4m source: Y4M pictures are planar")
    if kwargs.get("src_format", "yuv") != "yuv":
        raise ValueError(f"pixel_layout {pixel_layout!r} with src_format {kwargs['src_format']!r}: a layout describes a raw "
                         f"file (src_format='yuv'), PNGs are RGB")
    if kwargs.get("bitdepth") is not None and kwargs["bitdepth"] != info["bitdepth"]:
        raise ValueError(f"bitdepth {kwargs['bitdepth']!r} contradicts pixel_layout {pixel_layout!r}, which has "
                         f"{info['bitdepth']} bits")
    if chroma_format is not None and chroma_format != info["chroma_format"]:
        raise ValueError(f"chroma_format {chroma_format!r} contradicts pixel_layout {pixel_layout!r}, which is "
                         f"{info['chroma_format']!r}")
    fmt, bitdepth = info["chroma_format"], info["bitdepth"]
    chroma_loc = pmctf_chroma.resolve_loc(fmt, chroma_loc)
    if need_rate:
        raise ValueError("fps=None takes the frame rate of a .y4m header; this source has none")
    pmctf_chroma.check_side(width, height, "source")
    unpack = Unpacker(pixel_layout, width, height, pitch, luma_rows)
    nbytes = os.path.getsize(source)
    if nbytes % unpack.frame_bytes:
        raise ValueError(f"{source}: {nbytes} bytes are not a whole number of {pixel_layout} pictures of {width}x{height} "
                         f"({unpack.frame_bytes} bytes each with pitch {unpack.pitch} and luma_rows {unpack.luma_rows})")
    kwargs["bitdepth"] = bitdepth
    pmctf_gop._need_gpu(device, f"{what}(pixel_layout={pixel_layout!r})")
    size = None if coded_size is None else pmctf_scale.CodedSize(width, height, coded_size, device, bitdepth, chroma_loc)
    to420 = None if fmt == "420" else pmctf_chroma.Converter(width, height, fmt, "420", device, bitdepth, chroma_loc)
    return pmctf_chroma.SourcePipeline((width, height), fmt, chroma_loc, to420, size, layout=unpack)


def encode_sequence(codec, yuv_path, width, height, frame_num, gop, q_index, bin_folder, device, *, coded_size=None,
                    chroma_loc=None, chroma_format=None, pixel_layout=None, pitch=None, luma_rows=None, **kwargs):
    """pmctf_chroma.encode_sequence for a source in a pixel layout (LAYOUTS; pitch and luma_rows as the module text has
    them): every picture's bytes are uploaded as they lie in the file and unpacked on the device (one launch), then
    converted to 4:2:0 and resampled as a planar source of the layout's chroma format and depth is.  The folder is the one
    that planar source codes to.  A layout implies its bitdepth and chroma_format; giving another, a .y4m or PNG source, a
    pitch or luma_rows outside the rules or a file that is no whole number of pictures is a ValueError.
    pixel_layout=None: pmctf_chroma.encode_sequence itself."""
    import pmctf_gop
    pipeline = _pipeline(yuv_path, width, height, device, kwargs, coded_size, chroma_format, chroma_loc, pixel_layout, pitch,
                         luma_rows, "encode_sequence")
    return pmctf_gop._encode_equal_gops(codec, yuv_path, width, height, frame_num, gop, q_index, bin_folder, device,
                                        pipeline=pipeline, **kwargs)


def encode_sequence_gops(codec, source, width, height, frame_num, max_gop, q_index, bin_folder, device, *,
                         coded_size=None, chroma_loc=None, chroma_format=None, pixel_layout=None, pitch=None,
                         luma_rows=None, **kwargs):
    """pmctf_chroma.encode_sequence_gops with pixel_layout / pitch / luma_rows as encode_sequence above has them"""
    import pmctf_seq
    pipeline = _pipeline(source, width, height, device, kwargs, coded_size, chroma_format, chroma_loc, pixel_layout, pitch,
                         luma_rows, "encode_sequence_gops")
    return pmctf_seq._encode_gop_list(codec, source, width, height, frame_num, max_gop, q_index, bin_folder, device,
                                      pipeline=pipeline, **kwargs)


def encode_sequence_rate(codec, source, width, height, frame_num, max_gop, bitrate, fps, bin_folder, device, *,
                         coded_size=None, chroma_loc=None, chroma_format=None, pixel_layout=None, pitch=None,
                         luma_rows=None, **kwargs):
    """pmctf_chroma.encode_sequence_rate with pixel_layout / pitch / luma_rows as encode_sequence above has them; a source
    in a layout has no frame rate of its own, so fps=None is a ValueError"""
    import pmctf_rate
    pipeline = _pipeline(source, width, height, device, kwargs, coded_size, chroma_format, chroma_loc, pixel_layout, pitch,
                         luma_rows, "encode_sequence_rate", need_rate=fps is None)
    if fps is None:
        fps = pipeline.frame_rate
    return pmctf_rate._encode_at_rate(codec, source, width, height, frame_num, max_gop, bitrate, fps, bin_folder, device,
                                      pipeline=pipeline, **kwargs)


# ------------------------------------------------------------------------------------------------------------ decoding
class PackedSink:
    """The picture sink (pmctf_gop.picture_sink) of a decode with an output_layout: the pictures of the sink it wraps, as
    they would be written planar, packed on the device by one launch each and written as the surface's bytes with tight
    rows.  PNGs are the wrapped sink's."""
    stream_header = frame_marker = b""

    def __init__(self, sink, output_layout, yuv_out, bitdepth):
        info = check_layout(output_layout, "output_layout")
        if yuv_out is not None and pmctf_chroma.is_y4m(yuv_out):
            raise ValueError(f"output_layout {output_layout!r} with a .y4m output: Y4M pictures are planar")
        fmt = getattr(sink, "chroma_format", "420")
        if (info["chroma_format"], info["bitdepth"]) != (fmt, bitdepth):
            raise ValueError(f"output_layout {output_layout!r} holds {info['chroma_format']} pictures of {info['bitdepth']} "
                             f"bits; the pictures being written are {fmt} of {bitdepth} bits")
        self.sink, self.shape = sink, sink.shape
        self.pack = Packer(output_layout, sink.shape[1], sink.shape[0], what="output_layout")

    def pictures(self, frames_rec):
        surfaces = [self.pack(f) for f in self.sink.frames(frames_rec)]
        return [(s.cpu().numpy(),) for s in surfaces]

    def rgb8(self, frames_rec):
        return self.sink.rgb8(frames_rec)


def decode_sequence_checked(codec, bin_folder, yuv_out, device=None, png_out=None, verify="auto", coded_size_output=False,
                            coded_format_output=False, output_layout=None):
    """pmctf_chroma.decode_sequence_checked with the choice of the output's pixel layout: the pictures are rounded,
    resampled and converted as without one, then packed on the device (one launch each) and written as the layout's bytes,
    rows tight.  output_layout must have the chroma format and depth of the pictures being written (the coded 4:2:0
    pictures with coded_format_output=True, else the recorded format): a mismatch is a ValueError naming both, and so is a
    yuv_out ending in .y4m.  Hashes, PNGs and quality tables are those of the planar 4:2:0 pictures."""
    import pmctf_gop
    return pmctf_gop.decode_sequence_with(pmctf_gop.FullDecode(), codec, bin_folder, yuv_out, device, png_out, verify,
                                          coded_size_output=coded_size_output, coded_format_output=coded_format_output,
                                          output_layout=output_layout)


def decode_sequence_layer(codec, bin_folder, yuv_out, level, device=None, png_out=None, verify="auto", motion_fill=False,
                          coded_size_output=False, coded_format_output=False, output_layout=None):
    """pmctf_chroma.decode_sequence_layer with output_layout as decode_sequence_checked above has it"""
    import pmctf_gop
    import pmctf_layers
    return pmctf_gop.decode_sequence_with(pmctf_layers.LayerDecode(level, motion_fill), codec, bin_folder, yuv_out, device,
                                          png_out, verify, coded_size_output=coded_size_output,
                                          coded_format_output=coded_format_output, output_layout=output_layout)


# ---------------------------------------------------------------------------------------------------------- conversion
def convert_file(src, dst, width, height, from_layout, to_layout, device, pitch=None, luma_rows=None):
    """A file of pictures in from_layout -> the same pictures in to_layout, unpacked and packed on the device; "planar" is a
    layout name here and means the packed planar pictures of the other side's chroma format and depth (bytes at 8 bits,
    little-endian words above).  The two layouts must agree in chroma format and depth (ValueError naming both).  pitch,
    luma_rows: of the source; the output has tight rows.  -> the number of pictures.  The counterpart of pngs_to_yuv."""
    import numpy as np
    import torch
    import pmctf_gop
    if from_layout == PLANAR and to_layout == PLANAR:
        raise ValueError("from_layout and to_layout are both 'planar': nothing to convert")
    a = None if from_layout == PLANAR else check_layout(from_layout, "from_layout")
    b = None if to_layout == PLANAR else check_layout(to_layout, "to_layout")
    if a is not None and b is not None and (a["chroma_format"], a["bitdepth"]) != (b["chroma_format"], b["bitdepth"]):
        raise ValueError(f"from_layout {from_layout!r} holds {a['chroma_format']} pictures of {a['bitdepth']} bits, "
                         f"to_layout {to_layout!r} {b['chroma_format']} of {b['bitdepth']}")
    info = a or b
    pmctf_chroma.check_side(width, height)
    if a is None and (pitch is not None or luma_rows is not None):
        raise ValueError("pitch and luma_rows describe from_layout, which is 'planar'")
    unpack = None if a is None else Unpacker(from_layout, width, height, pitch, luma_rows, what="from_layout")
    pack = None if b is None else Packer(to_layout, width, height, what="to_layout")
    word = 1 if info["bitdepth"] == 8 else 2
    planar_bytes = pmctf_chroma.frame_samples(width, height, info["chroma_format"]) * word
    in_bytes = planar_bytes if unpack is None else unpack.frame_bytes
    nbytes = os.path.getsize(src)
    if nbytes == 0 or nbytes % in_bytes:
        raise ValueError(f"{src}: {nbytes} bytes are not a whole number of {from_layout} pictures of {width}x{height} "
                         f"({in_bytes} bytes each)")
    pmctf_gop._need_gpu(device, "convert_file")
    with open(src, "rb") as fin, open(dst, "wb") as fout:
        for _ in range(nbytes // in_bytes):
            data = torch.from_numpy(np.fromfile(fin, dtype=np.uint8, count=in_bytes)).to(device)
            frame = unpack(data) if unpack is not None else (data if word == 1 else data.view(torch.uint16))
            out = pack(frame) if pack is not None else frame
            fout.write(out.cpu().numpy().tobytes(order="C"))
    return nbytes // in_bytes
