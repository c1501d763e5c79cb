"""Y4M files and 4:4:4 / 4:2:2 sources: the codec codes 4:2:0 pictures; a source in another chroma format is
converted to 4:2:0 on the device before it enters the codec and converted back after it leaves, by the exact integer
filter of pmctf_scale.  Nothing inside the codec changes.

A picture in chroma format F in ("420", "422", "444") is Y of h x w, then Cb and Cr of h/sy x w/sx each, (sx, sy) = (2,2),
(2,1), (1,1).  Converting F_in -> F_out copies Y and sends Cb and Cr through pmctf_scale's two passes with
pmctf_scale.axis_table(n_in, n_out, phase) per axis; an axis whose length does not change gets the single-tap table
(start[i] = i, coef[i] = (16384,)), which is exact.  The vertical phase is 0.  The horizontal phase is 0 for chroma_loc
"center" and format_phase(s_in, s_out) for "left" (chroma co-sited with the left luma column): -1/2 going 4:4:4 -> 4:2:0
or 4:2:2, +1/4 going back.  4:2:2 is horizontally co-sited (the Y4M / MPEG-2 layout, the only one defined): a 4:2:2 source
is coded as 4:2:0 "left", and "center" with it is a ValueError.  4:4:4 sources default to "center".

This module holds that arithmetic's tables, the Y4M header (parse_y4m_header, y4m_header), PlanarReader (.y4m files and
raw planar files of any of the three formats), SourcePipeline (what the encoders' bodies take: an optional step to 4:2:0,
an optional pmctf_scale.CodedSize, format first, size second), source_format.json, OutputFormat (what the decoders need)
and the entry points encode_sequence, encode_sequence_gops, encode_sequence_rate, decode_sequence_checked,
decode_sequence_layer: pmctf_scale's functions with the keywords chroma_format (encoding) and coded_format_output
(decoding) added.  With a raw 4:2:0 source and chroma_format=None they do what pmctf_scale's functions do.

Out of scope: 4:0:0, 420paldv, 4:1:1, alpha, interlaced material.  The encoders' quality tables are those of the coded
4:2:0 pictures against the converted source; figures in the source's own format come from pmctf_quality."""
import functools
import os
import re
from fractions import Fraction

import pmctf_scale
from pmctf_records import is_int, read_record, write_record
from pmctf_scale import CHROMA_LOCS, COEF_ONE, FILTER, MAX_SIDE

FORMATS = ("420", "422", "444")
SUBSAMPLING = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}            # format -> (sx, sy)
SOURCE_FORMAT = "source_format.json"
SOURCE_FORMAT_VERSION = 1
SOURCE_FIELDS = ("format_version", "chroma_format", "chroma_loc", "filter", "frame_rate")
Y4M_MAGIC = b"YUV4MPEG2"
Y4M_DEFAULT_RATE = (25, 1)                     # written when a folder records no frame rate
Y4M_REFUSED = ("420paldv", "411", "444alpha")  # and everything starting with "mono"
_HEADER_MAX = 4096


# ---------------------------------------------------------------------------------------------------- the arithmetic
def check_format(fmt):
    if fmt not in FORMATS:
        raise ValueError(f"chroma_format is one of {FORMATS} (got {fmt!r})")
    return fmt


def format_phase(s_in, s_out, chroma_loc):
    """horizontal phase of a chroma plane going from subsampling s_in to s_out (1 or 2).  "center": 0.  "left": a plane
    subsampled by s, co-sited with the left luma column, has the continuous coordinate x_s = x_luma / s + (1 - 1/s) / 2;
    with scale = n_in / n_out = s_out / s_in the centre of output i is scale (i + 1/2) + phase, so
    phase = ((1 - 1/s_in) - scale (1 - 1/s_out)) / 2: -1/2 for 1 -> 2, +1/4 for 2 -> 1, 0 for s_in == s_out."""
    if chroma_loc not in CHROMA_LOCS:
        raise ValueError(f"chroma_loc is one of {CHROMA_LOCS} (got {chroma_loc!r})")
    if s_in not in (1, 2) or s_out not in (1, 2):
        raise ValueError(f"a chroma plane is subsampled by 1 or 2 (got {s_in!r} -> {s_out!r})")
    if chroma_loc == "center":
        return Fraction(0)
    return ((1 - Fraction(1, s_in)) - Fraction(s_out, s_in) * (1 - Fraction(1, s_out))) / 2


def resolve_loc(chroma_format, chroma_loc=None):
    """the siting of the 4:2:0 pictures a source of chroma_format is coded as: 4:2:2 is "left" ("center" refused), 4:4:4
    and 4:2:0 default to "center" """
    check_format(chroma_format)
    if chroma_loc is not None and chroma_loc not in CHROMA_LOCS:
        raise ValueError(f"chroma_loc is one of {CHROMA_LOCS} or None (got {chroma_loc!r})")
    if chroma_format == "422":
        if chroma_loc == "center":
            raise ValueError("4:2:2 chroma is co-sited with the left luma column (the Y4M / MPEG-2 layout): chroma_loc "
                             "'center' is not defined for a 422 source")
        return "left"
    return chroma_loc or "center"


def check_side(width, height, what="picture"):
    for n in (width, height):
        if not is_int(n) or n <= 0 or n & 1 or n > MAX_SIDE:
            raise ValueError(f"{what}: sides are even, positive and at most {MAX_SIDE} (got {width!r}x{height!r})")


@functools.lru_cache(maxsize=64)
def identity_table(n):
    """the single-tap table of an axis that keeps its length"""
    return tuple(range(n)), ((COEF_ONE,),) * n, 1


def chroma_axes(width, height, fmt_in, fmt_out, chroma_loc):
    """-> ((n_in, n_out, phase) of the chroma planes' x axis, the same of their y axis)"""
    check_side(width, height)
    (sxi, syi), (sxo, syo) = SUBSAMPLING[check_format(fmt_in)], SUBSAMPLING[check_format(fmt_out)]
    return (width // sxi, width // sxo, format_phase(sxi, sxo, chroma_loc)), (height // syi, height // syo, Fraction(0))


def chroma_tables(width, height, fmt_in, fmt_out, chroma_loc="center"):
    """-> ((start, coef, T) of the chroma planes' x axis, the same of their y axis), as pmctf_scale.axis_table gives them"""
    return tuple(identity_table(n_in) if n_in == n_out else pmctf_scale.axis_table(n_in, n_out, phase)
                 for n_in, n_out, phase in chroma_axes(width, height, fmt_in, fmt_out, chroma_loc))


_device_tables = {}


def _device_table(n_in, n_out, phase, device):
    if n_in != n_out:
        return pmctf_scale.device_table(n_in, n_out, phase, device)
    import numpy as np
    import torch
    key = (n_in, str(torch.device(device)))
    if key not in _device_tables:
        start, coef, taps = identity_table(n_in)
        raw = np.asarray(start, dtype="<i4").tobytes() + np.asarray(coef, dtype="<i2").tobytes()
        _device_tables[key] = (torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device), taps)
    return _device_tables[key]


def frame_samples(width, height, fmt):
    sx, sy = SUBSAMPLING[check_format(fmt)]
    return width * height + 2 * (width // sx) * (height // sy)


class Converter:
    """Packed planar pictures of width x height from fmt_in to fmt_out on the device: __call__(frame) takes the picture as
    it lies in a file (uint8 tensor at bitdepth 8, uint16 above), one launch (ops.convert_chroma).  The tables are built
    and uploaded here, once."""

    def __init__(self, width, height, fmt_in, fmt_out, device, bitdepth=8, chroma_loc="center"):
        if not is_int(bitdepth) or not 8 <= bitdepth <= 16:
            raise ValueError(f"bitdepth is 8 or 9..16 (got {bitdepth!r})")
        axes = chroma_axes(width, height, fmt_in, fmt_out, chroma_loc)
        self.size, self.fmt_in, self.fmt_out = (width, height), fmt_in, fmt_out
        self.bitdepth, self.chroma_loc = bitdepth, chroma_loc
        self.tables = tuple(_device_table(n_in, n_out, phase, device) for n_in, n_out, phase in axes)

    def __call__(self, frame):
        from pMCTF.hip import ops
        return ops.convert_chroma(frame, self.size[1], self.size[0], self.fmt_in, self.fmt_out,
                                  [t for t, _ in self.tables], [n for _, n in self.tables], self.bitdepth)


def unpack_frame(frame, height, width, fmt):
    """a packed picture on the device -> (Y, Cb, Cr) numpy arrays"""
    host = frame.cpu().numpy()
    sx, sy = SUBSAMPLING[fmt]
    hc, wc, n = height // sy, width // sx, height * width
    return host[:n].reshape(height, width), host[n:n + hc * wc].reshape(hc, wc), host[n + hc * wc:].reshape(hc, wc)


# ------------------------------------------------------------------------------------------------------------ Y4M
def _y4m_tag_fields(tag):
    """a C tag -> (chroma_format, bitdepth, chroma_loc or None where the tag does not say); ValueError naming the tag"""
    if tag in Y4M_REFUSED or tag.startswith("mono"):
        raise ValueError(f"Y4M chroma tag C{tag}: not supported (4:2:0, 4:2:2 and 4:4:4 without alpha are)")
    if tag == "420jpeg":
        return "420", 8, "center"
    if tag == "420mpeg2":
        return "420", 8, "left"
    m = re.fullmatch(r"(420|422|444)(?:p(9|1[0-6]))?", tag)
    if m is None:
        raise ValueError(f"Y4M chroma tag C{tag}: not known")
    fmt, depth = m.group(1), m.group(2)
    return fmt, int(depth) if depth else 8, "center" if tag == "420" else None


def y4m_tag(chroma_format, bitdepth=8, chroma_loc="center"):
    """the C tag written for pictures of that format, depth and siting"""
    check_format(chroma_format)
    if not is_int(bitdepth) or not 8 <= bitdepth <= 16:
        raise ValueError(f"bitdepth is 8 or 9..16 (got {bitdepth!r})")
    if bitdepth > 8:
        return f"{chroma_format}p{bitdepth}"
    if chroma_format == "420":
        return "420mpeg2" if chroma_loc == "left" else "420jpeg"
    return chroma_format


def _check_rate(frame_rate, what):
    try:
        num, den = frame_rate
    except (TypeError, ValueError):
        raise ValueError(f"{what}: a frame rate is (num, den) (got {frame_rate!r})") from None
    if not is_int(num) or not is_int(den) or num <= 0 or den <= 0:
        raise ValueError(f"{what}: a frame rate is two positive integers (got {num!r}:{den!r})")
    return num, den


def y4m_header(width, height, frame_rate=Y4M_DEFAULT_RATE, chroma_format="420", bitdepth=8, chroma_loc="center", tag=None):
    """the stream header line of a progressive Y4M file with square pixels unknown (Ip A0:0), as bytes.  tag: the C tag to
    write instead of y4m_tag(chroma_format, bitdepth, chroma_loc) (one parse_y4m_header accepts)."""
    check_side(width, height, "Y4M")
    num, den = _check_rate(frame_rate, "Y4M")
    if tag is None:
        tag = y4m_tag(chroma_format, bitdepth, chroma_loc)
    else:
        _y4m_tag_fields(tag)
    return f"YUV4MPEG2 W{width} H{height} F{num}:{den} Ip A0:0 C{tag}\n".encode("ascii")


def parse_y4m_header(data):
    """data: the first bytes of a Y4M file (the stream header line at least) -> {"width", "height", "frame_rate": (num, den)
    or None without an F tag, "chroma_format", "chroma_loc", "bitdepth", "tag", "interlace", "aspect", "header_bytes": the
    length of the line with its newline}.  chroma_loc is the tag's siting ("center" for 420jpeg and 420, "left" for
    420mpeg2), resolve_loc's default where the tag does not say.  ValueError, naming the tag, for what the module text
    lists as refused."""
    data = bytes(data[:_HEADER_MAX])
    end = data.find(b"\n")
    if not data.startswith(Y4M_MAGIC + b" ") or end < 0:
        raise ValueError("not a Y4M file: no YUV4MPEG2 stream header line")
    try:
        tags = data[len(Y4M_MAGIC) + 1:end].decode("ascii").split()
    except UnicodeDecodeError:
        raise ValueError("Y4M: the stream header is not ASCII") from None
    out = {"width": None, "height": None, "frame_rate": None, "interlace": "?", "aspect": None, "tag": "420jpeg",
           "header_bytes": end + 1}
    for t in tags:
        key, val = t[0], t[1:]
        if key in "WH":
            if not val.isdigit():
                raise ValueError(f"Y4M tag {t}: not a size")
            out["width" if key == "W" else "height"] = int(val)
        elif key == "F":
            parts = val.split(":")
            if len(parts) != 2 or not all(p.isdigit() for p in parts):
                raise ValueError(f"Y4M tag {t}: a frame rate is F<num>:<den>")
            if int(parts[0]) == 0 or int(parts[1]) == 0:
                raise ValueError(f"Y4M tag {t}: the frame rate is zero")
            out["frame_rate"] = (int(parts[0]), int(parts[1]))
        elif key == "I":
            if val not in ("p", "?"):
                raise ValueError(f"Y4M tag {t}: interlaced material is not supported (Ip or I? is)")
            out["interlace"] = val
        elif key == "A":
            out["aspect"] = val
        elif key == "C":
            out["tag"] = val
        elif key != "X":
            raise ValueError(f"Y4M tag {t}: not known")
    for key, name in (("W", "width"), ("H", "height")):
        if out[name] is None:
            raise ValueError(f"Y4M: the stream header has no {key} tag")
    fmt, depth, loc = _y4m_tag_fields(out["tag"])
    try:
        check_side(out["width"], out["height"])
    except ValueError:
        raise ValueError(f"Y4M tags W{out['width']} H{out['height']}: sides are even, positive and at most "
                         f"{MAX_SIDE}") from None
    out.update(chroma_format=fmt, bitdepth=depth, chroma_loc=loc or resolve_loc(fmt))
    return out


def is_y4m(path):
    return isinstance(path, (str, os.PathLike)) and os.fspath(path).lower().endswith(".y4m")


def read_y4m_header(path):
    with open(path, "rb") as f:
        return parse_y4m_header(f.read(_HEADER_MAX))


class PlanarReader:
    """YUVReader's interface (read_one_frame() -> (Y, Cb, Cr) arrays, uint8 or uint16; close()) for a .y4m file or a raw
    planar file of a stated chroma_format.  A .y4m carries its own width, height, bitdepth, chroma_format and frame_rate;
    what is given here (not None) must agree with it (ValueError).  chroma_loc=None: the header's (the format's default for
    a raw file).  Every FRAME marker is checked when the file is opened (ValueError naming the offset); a file that ends
    inside a picture raises when that picture is read, as YUVReader does.  len(): the whole pictures of the file."""

    def __init__(self, src_file, width=None, height=None, start_index=0, bitdepth=None, chroma_format=None, chroma_loc=None):
        if not os.path.exists(src_file):
            raise AssertionError(f"no such sequence: {src_file}")
        self.src_file = src_file
        self.y4m = is_y4m(src_file)
        self.frame_rate = None
        if self.y4m:
            head = read_y4m_header(src_file)
            for name, given in (("width", width), ("height", height), ("bitdepth", bitdepth), ("chroma_format", chroma_format)):
                if given is not None and given != head[name]:
                    raise ValueError(f"{src_file}: the Y4M header (C{head['tag']}, {head['width']}x{head['height']}) has "
                                     f"{name} {head[name]!r}, not {given!r}")
            width, height, bitdepth, chroma_format = (head[k] for k in ("width", "height", "bitdepth", "chroma_format"))
            self.frame_rate = head["frame_rate"]
            if chroma_loc is None:
                chroma_loc = head["chroma_loc"]
        else:
            if width is None or height is None:
                raise ValueError("a raw planar file needs its width and height")
            bitdepth = 8 if bitdepth is None else bitdepth
            chroma_format = chroma_format or "420"
        check_side(width, height, str(src_file))
        if not is_int(bitdepth) or not 8 <= bitdepth <= 16:
            raise ValueError(f"bitdepth is 8, or 9..16 for files of 16-bit samples (got {bitdepth!r})")
        self.width, self.height, self.bitdepth = width, height, bitdepth
        self.chroma_format = check_format(chroma_format)
        self.chroma_loc = resolve_loc(chroma_format, chroma_loc)
        self.current_frame_index = int(start_index)
        self.eof = False
        self._fh = None
        sx, sy = SUBSAMPLING[chroma_format]
        self._shapes = ((height, width), (height // sy, width // sx), (height // sy, width // sx))
        self._frame_bytes = frame_samples(width, height, chroma_format) * (2 if bitdepth > 8 else 1)
        self._offsets, self.truncated = self._scan(head["header_bytes"] if self.y4m else 0)

    def _scan(self, at):
        """-> (the offset of every whole picture's first sample, whether the file ends inside a picture)"""
        size = os.path.getsize(self.src_file)
        offsets = []
        if not self.y4m:
            n = size // self._frame_bytes
            return [k * self._frame_bytes for k in range(n)], size != n * self._frame_bytes
        with open(self.src_file, "rb") as f:
            while at < size:
                f.seek(at)
                line = f.read(256)
                end = line.find(b"\n")
                if end < 0 and len(line) < 256 and (b"FRAME".startswith(line) or line.startswith(b"FRAME ")):
                    return offsets, True                                # the file ends inside a FRAME line
                if end < 0 or not (line[:end] == b"FRAME" or line.startswith(b"FRAME ")):
                    raise ValueError(f"{self.src_file}: no FRAME marker at offset {at} (picture {len(offsets)})")
                at += end + 1
                if at + self._frame_bytes > size:
                    return offsets, True
                offsets.append(at)
                at += self._frame_bytes
        return offsets, False

    def __len__(self):
        return len(self._offsets)

    def read_one_frame(self, src_format="rgb"):
        import numpy as np
        if self.eof:
            return None if src_format == "rgb" else (None, None, None)
        assert self.current_frame_index < len(self._offsets), "sequence ends inside a picture"
        if self._fh is None:
            self._fh = open(self.src_file, "rb")
        self._fh.seek(self._offsets[self.current_frame_index])
        planes = []
        for rows, cols in self._shapes:
            data = np.fromfile(self._fh, dtype=np.uint8 if self.bitdepth == 8 else "<u2", count=rows * cols)
            assert data.size == rows * cols, "sequence ends inside a picture"
            planes.append(data.astype(np.uint8 if self.bitdepth == 8 else np.uint16, copy=False).reshape(rows, cols))
        self.current_frame_index += 1
        return tuple(planes)

    def close(self):
        if self._fh is not None:
            self._fh.close()
            self._fh = None
        self.current_frame_index = 0


# ----------------------------------------------------------------------------------------------------- the header file
def _check_source_record(path, record):
    if record["filter"] != FILTER:
        raise ValueError(f"{path}: filter {record['filter']!r}, this decoder knows {FILTER!r}")
    if record["chroma_format"] not in FORMATS or not isinstance(record["chroma_format"], str):
        raise ValueError(f"{path}: chroma_format {record['chroma_format']!r}, one of {FORMATS}")
    if record["chroma_loc"] not in CHROMA_LOCS or not isinstance(record["chroma_loc"], str):
        raise ValueError(f"{path}: chroma_loc {record['chroma_loc']!r}, one of {CHROMA_LOCS}")
    if record["chroma_format"] == "422" and record["chroma_loc"] == "center":
        raise ValueError(f"{path}: chroma_format '422' with chroma_loc 'center': 4:2:2 chroma is co-sited (left)")
    rate = record["frame_rate"]
    if rate is not None:
        if not isinstance(rate, (list, tuple)) or len(rate) != 2:
            raise ValueError(f"{path}: frame_rate is [num, den] or null (got {rate!r})")
        _check_rate(rate, path)


def write_source_format(bin_folder, chroma_format, chroma_loc, frame_rate=None):
    """bin_folder/source_format.json: {"format_version", "chroma_format": the source's, "chroma_loc": the siting of the coded
    4:2:0 pictures, "filter", "frame_rate": [num, den] or null}.  Written only for a .y4m source or one that is not 4:2:0."""
    path = os.path.join(bin_folder, SOURCE_FORMAT)
    record = {"format_version": SOURCE_FORMAT_VERSION, "chroma_format": chroma_format, "chroma_loc": chroma_loc,
              "filter": FILTER, "frame_rate": list(frame_rate) if isinstance(frame_rate, tuple) else frame_rate}
    _check_source_record(path, record)
    return write_record(path, record, indent=2)


def read_source_format(bin_folder):
    """-> None when bin_folder has no source_format.json, else its record; ValueError naming the path for a malformed
    file, another version or filter, an unknown or missing field, an unknown format or siting, a wrong type, and 4:2:2
    with "center" """
    path = os.path.join(bin_folder, SOURCE_FORMAT)
    record = read_record(path, "source format file", SOURCE_FORMAT_VERSION, fields=SOURCE_FIELDS,
                         expected=sorted(SOURCE_FIELDS))
    if record is not None:
        _check_source_record(path, record)
    return record


# ------------------------------------------------------------------------------------------------------------ encoding
class SourcePipeline:
    """The one description of a source's way into the codec that the encoders' bodies take (pmctf_gop.SequenceEncode): an
    optional step out of a pixel layout (layout: a pmctf_layout.Unpacker), an optional step to 4:2:0 (to420: a
    Converter), an optional step to the coded size (size: a pmctf_scale.CodedSize), layout first, format second, size
    third.  The layout's step is applied by read_gop_device to the uploaded bytes of a picture (the reader carries the
    Unpacker), the other two by the one hook ingest gives it.  chroma_format is then the layout's.  source_size: (width, height) of the source; coded:
    of what enters the codec.  y4m: the source is a .y4m file.  A .y4m or a source that is not 4:2:0 is read by
    PlanarReader and recorded in source_format.json; a raw 4:2:0 file by YUVReader, with no record of its format; a source
    in a pixel layout by pmctf_layout.PackedReader, recorded as the planar source of its chroma format is.
    A raw 4:2:0 source without a coded size has no pipeline at all (None)."""

    def __init__(self, source_size, chroma_format="420", chroma_loc="center", to420=None, size=None, frame_rate=None,
                 y4m=False, layout=None):
        self.source, self.chroma_format, self.chroma_loc = source_size, chroma_format, chroma_loc
        self.to420, self.size, self.frame_rate, self.layout = to420, size, frame_rate, layout
        self.planar = y4m or chroma_format != "420"
        self.coded = source_size if size is None else size.coded

    def open_reader(self, src_file, width, height, bitdepth=8):
        if self.layout is not None:
            import pmctf_layout
            return pmctf_layout.PackedReader(src_file, self.layout)
        if self.planar:
            return PlanarReader(src_file, width, height, 0, bitdepth, self.chroma_format, self.chroma_loc)
        from pMCTF.utils.yuv_reader import YUVReader
        return YUVReader(src_file, width, height, start_index=0, bitdepth=bitdepth)

    def ingest(self, keep):
        """the hook read_gop_device applies to every packed picture after upload; keep=True also keeps the 4:2:0 source
        pictures for display_quality"""
        return pmctf_scale._Ingest(self.to420, self.size, keep, self.coded[::-1])

    def display_quality(self, rec):
        return [] if self.size is None else self.size.display_quality(rec)

    def write_header(self, bin_folder):
        """display_format.json when coded at another size; source_format.json for a .y4m or a source that is not 4:2:0"""
        written = [] if self.size is None else [self.size.write_header(bin_folder)]
        if self.planar:
            written.append(write_source_format(bin_folder, self.chroma_format, self.chroma_loc, self.frame_rate))
        return written


def _pipeline(source, width, height, device, kwargs, coded_size, chroma_format, chroma_loc, what, need_rate=False):
    """-> the SourcePipeline of the source, None where it has none.  A raw 4:2:0 source is pmctf_scale's case.
    need_rate: a source without a frame rate (all but a .y4m with an F tag) is a ValueError."""
    no_rate = "fps=None takes the frame rate of a .y4m header; this source has none"
    import pmctf_gop
    if chroma_format is not None:
        check_format(chroma_format)
    y4m = is_y4m(source)
    if not y4m and chroma_format in (None, "420"):
        if need_rate:
            raise ValueError(no_rate)
        return pmctf_scale._pipeline(width, height, coded_size, device, kwargs.get("bitdepth", 8), chroma_loc or "center", what)
    if kwargs.get("src_format", "yuv") != "yuv":
        raise ValueError(f"{what}: chroma_format and .y4m sources are planar files (src_format='yuv')")
    bitdepth = pmctf_gop.check_bitdepth(kwargs.get("bitdepth", 8))
    rate = None
    if y4m:
        head = read_y4m_header(source)
        for name, given in (("width", width), ("height", height), ("bitdepth", bitdepth), ("chroma_format", chroma_format)):
            if given is not None and given != head[name]:
                raise ValueError(f"{source}: the Y4M header (C{head['tag']}, {head['width']}x{head['height']}) has {name} "
                                 f"{head[name]!r}, not {given!r}")
        chroma_format, rate = head["chroma_format"], head["frame_rate"]
        if chroma_loc is None:
            chroma_loc = head["chroma_loc"]
    chroma_loc = resolve_loc(chroma_format, chroma_loc)
    pmctf_gop._need_gpu(device, f"{what}(chroma_format={chroma_format!r}, source={os.path.basename(os.fspath(source))!r})")
    check_side(width, height, "source")
    if rate is not None:
        rate = _check_rate(rate, "frame_rate")
    size = None if coded_size is None else pmctf_scale.CodedSize(width, height, coded_size, device, bitdepth, chroma_loc)
    to420 = None if chroma_format == "420" else Converter(width, height, chroma_format, "420", device, bitdepth, chroma_loc)
    if need_rate and rate is None:
        raise ValueError(no_rate)
    return SourcePipeline((width, height), chroma_format, chroma_loc, to420, size, rate, y4m)


def encode_sequence(codec, yuv_path, width, height, frame_num, gop, q_index, bin_folder, device, *, coded_size=None,
                    chroma_loc=None, chroma_format=None, **kwargs):
    """pmctf_scale.encode_sequence for a source of chroma_format "420", "422" or "444" (None: a .y4m's own, else "420"): a
    path ending in .y4m is read as Y4M, and its header's size and depth must agree with width / height / bitdepth
    (ValueError).  Every picture is converted to 4:2:0 on the device directly after upload, then resampled to coded_size
    if one is given; everything downstream sees a 4:2:0 source: the files, sequence.json, the hashes and the quality
    tables are those of coding the converted pictures.  chroma_loc=None: the header's siting, else the format's default
    ("left" for 4:2:2, "center" otherwise).  With keep_gops=True the folder gets source_format.json when the source is a
    .y4m or not 4:2:0.  The result has "display_quality" (empty without a coded_size).
    A raw 4:2:0 .yuv with chroma_format=None: what pmctf_scale.encode_sequence does, same files, no new header."""
    import pmctf_gop
    pipeline = _pipeline(yuv_path, width, height, device, kwargs, coded_size, chroma_format, chroma_loc, "encode_sequence")
    return pmctf_gop._encode_equal_gops(codec, yuv_path, width, height, frame_num, gop, q_index, bin_folder, device,
                                        pipeline=pipeline, **kwargs)


def encode_sequence_gops(codec, source, width, height, frame_num, max_gop, q_index, bin_folder, device, *,
                         coded_size=None, chroma_loc=None, chroma_format=None, **kwargs):
    """pmctf_scale.encode_sequence_gops with chroma_format / chroma_loc as encode_sequence above has them; the scene-cut
    pass looks at the converted pictures."""
    import pmctf_seq
    pipeline = _pipeline(source, width, height, device, kwargs, coded_size, chroma_format, chroma_loc, "encode_sequence_gops")
    return pmctf_seq._encode_gop_list(codec, source, width, height, frame_num, max_gop, q_index, bin_folder, device,
                                      pipeline=pipeline, **kwargs)


def encode_sequence_rate(codec, source, width, height, frame_num, max_gop, bitrate, fps, bin_folder, device, *,
                         coded_size=None, chroma_loc=None, chroma_format=None, **kwargs):
    """pmctf_scale.encode_sequence_rate with chroma_format / chroma_loc as encode_sequence above has them; fps=None takes
    the frame rate of the .y4m header (ValueError when there is none)."""
    import pmctf_rate
    pipeline = _pipeline(source, width, height, device, kwargs, coded_size, chroma_format, chroma_loc, "encode_sequence_rate",
                         need_rate=fps is None)
    if fps is None:
        fps = pipeline.frame_rate
    return pmctf_rate._encode_at_rate(codec, source, width, height, frame_num, max_gop, bitrate, fps, bin_folder, device,
                                      pipeline=pipeline, **kwargs)


# ------------------------------------------------------------------------------------------------------------ decoding
class OutputFormat:
    """What the decoders need to write pictures in another chroma format than the coded 4:2:0, or into a .y4m file:
    stream_header (bytes written once), frame_marker (bytes before every picture), pictures(frames_rec)."""

    def __init__(self, record, y4m, coded, display, device, bitdepth):
        self.display, self.coded, self.bitdepth = display, coded, bitdepth
        self.size = coded if display is None else display.size
        self.shape = self.size[::-1]
        self.chroma_format = "420" if record is None else record["chroma_format"]
        self.chroma_loc = record["chroma_loc"] if record is not None else \
            (display.up.chroma_loc if display is not None else "center")
        rate = Y4M_DEFAULT_RATE if record is None or record["frame_rate"] is None else tuple(record["frame_rate"])
        self.stream_header = y4m_header(self.size[0], self.size[1], rate, self.chroma_format, bitdepth,
                                        self.chroma_loc) if y4m else b""
        self.frame_marker = b"FRAME\n" if y4m else b""
        self.from420 = None if self.chroma_format == "420" else \
            Converter(self.size[0], self.size[1], "420", self.chroma_format, device, bitdepth, self.chroma_loc)

    def frames(self, frames_rec):
        """reconstructed (padded, float) pictures -> the packed integer pictures on the device: rounded as frames_to_u8 /
        frames_to_u16 round them, resampled to the display size if there is one, then converted to the output's chroma
        format"""
        cw, ch = self.coded
        if self.display is not None:
            frames = self.display.frames(frames_rec)
        else:
            frames = [pmctf_scale.pack_frame(rec[0], rec[1], ch, cw, self.bitdepth) for rec in frames_rec]
        if self.from420 is not None:
            frames = [self.from420(f) for f in frames]
        return frames

    def pictures(self, frames_rec):
        """-> [(Y, Cb, Cr)] integer arrays of frames(frames_rec)"""
        W, H = self.size
        return [unpack_frame(f, H, W, self.chroma_format) for f in self.frames(frames_rec)]

    def rgb8(self, frames_rec):
        """the PNGs' pictures: those of the 4:2:0 pictures, at the display size if there is one"""
        if self.display is not None:
            return self.display.rgb8(frames_rec)
        import pmctf_gop
        return pmctf_gop.frames_to_rgb8(frames_rec, self.coded[1], self.coded[0])


def output_format(bin_folder, yuv_out, coded_width, coded_height, display, device, bitdepth=8, coded_format_output=False):
    """-> the OutputFormat of a decode of bin_folder into yuv_out, or None when the pictures are written as before: no
    source_format.json asks for another format than 4:2:0 (or coded_format_output says to ignore it) and yuv_out is no
    .y4m.  The file is validated either way.  display: the pmctf_scale.DisplaySize in force, or None."""
    record = read_source_format(bin_folder)
    y4m = yuv_out is not None and is_y4m(yuv_out)
    if record is not None and coded_format_output:
        record = dict(record, chroma_format="420")
    if not y4m and (record is None or record["chroma_format"] == "420"):
        return None
    return OutputFormat(record, y4m, (coded_width, coded_height), display, device, bitdepth)


def decode_sequence_checked(codec, bin_folder, yuv_out, device=None, png_out=None, verify="auto", coded_size_output=False,
                            coded_format_output=False):
    """pmctf_scale.decode_sequence_checked with the choice of the output's chroma format for a folder with a
    source_format.json: by default the pictures are written in the source's format (the rounded pictures, then the display
    size if display_format.json asks for one, then the chroma format, all on the device); coded_format_output=True writes
    the coded 4:2:0 pictures.  A yuv_out ending in .y4m gets a Y4M header (W, H and the C tag of what is written, F from the
    recorded frame rate, 25:1 when none is recorded, Ip A0:0) and FRAME markers; any other path raw planes.  png_out takes
    its RGB from the 4:2:0 pictures; the hashes are those of the coded 4:2:0 pictures and are verified before."""
    import pmctf_gop
    return pmctf_gop.decode_sequence_with(pmctf_gop.FullDecode(), codec, bin_folder, yuv_out, device, png_out, verify,
                                          coded_size_output=coded_size_output, coded_format_output=coded_format_output)


def decode_sequence_layer(codec, bin_folder, yuv_out, level, device=None, png_out=None, verify="auto", motion_fill=False,
                          coded_size_output=False, coded_format_output=False):
    """pmctf_scale.decode_sequence_layer with coded_format_output as decode_sequence_checked above has it"""
    import pmctf_gop
    import pmctf_layers
    return pmctf_gop.decode_sequence_with(pmctf_layers.LayerDecode(level, motion_fill), codec, bin_folder, yuv_out, device,
                                          png_out, verify, coded_size_output=coded_size_output,
                                          coded_format_output=coded_format_output)
