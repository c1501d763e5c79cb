"""The chroma format conversion of DESIGN 5m restated in numpy and exact rationals, on the functions of
tests/scale_restatement.py, and a Y4M reader and writer of its own: the yardstick of tests/test_picture_chroma_cpu.py and
tests/test_gpu_picture_chroma.py.  Written from the definition, not from pmctf_chroma.py.

A picture of h x w in format F is Y (h x w), then Cb and Cr (h / sy x w / sx).  F_in -> F_out copies Y and resamples Cb
and Cr with the filter of scale_restatement, both passes always (an axis that keeps its length has the rows
(.., 0, 16384, 0, ..), which give the plane back).

Siting.  Put luma sample k on [k, k + 1).  A chroma plane subsampled by s horizontally has its sample j
  "center": in the middle of its s luma samples, at s (j + 1/2);
  "left":   on the first of them, at s j + 1/2.
In the plane's own coordinates sample j lies at u = j + 1/2.  For "left", output i of a plane subsampled by s_out lies at
luma position s_out i + 1/2, which in the input plane (subsampled by s_in) is u = (s_out i + 1/2 - 1/2) / s_in + 1/2
= scale i + 1/2 with scale = s_out / s_in.  The filter puts output i at scale (i + 1/2) + phase, so phase = (1 - scale) / 2.
For "center" the same reasoning gives u = scale (i + 1/2): phase 0.  Vertically nothing moves: phase 0.
Nothing here touches torch or the product."""
from fractions import Fraction as Fr

import numpy as np

import scale_restatement as sr

SUB = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}


def phase(s_in, s_out, loc):
    assert loc in ("center", "left") and s_in in (1, 2) and s_out in (1, 2)
    return Fr(0) if loc == "center" else (1 - Fr(s_out, s_in)) / 2


def plane_shapes(h, w, fmt):
    sx, sy = SUB[fmt]
    return (h, w), (h // sy, w // sx), (h // sy, w // sx)


def samples(h, w, fmt):
    return sum(r * c for r, c in plane_shapes(h, w, fmt))


def split(frame, h, w, fmt):
    """packed picture -> (Y, Cb, Cr) views"""
    frame = np.asarray(frame)
    assert frame.shape == (samples(h, w, fmt),)
    out, at = [], 0
    for r, c in plane_shapes(h, w, fmt):
        out.append(frame[at:at + r * c].reshape(r, c))
        at += r * c
    return tuple(out)


def convert(frame, h, w, fmt_in, fmt_out, b, loc="center"):
    """one packed planar picture of fmt_in (1-D integer array) -> the packed picture of fmt_out"""
    assert not (h | w) & 1 and h > 0 and w > 0
    y, cb, cr = split(frame, h, w, fmt_in)
    (sxi, _), (sxo, _) = SUB[fmt_in], SUB[fmt_out]
    _, (hc, wc), _ = plane_shapes(h, w, fmt_out)
    px = phase(sxi, sxo, loc)
    out = [y] + [sr.resize_plane(c, hc, wc, b, phase_x=px, phase_y=0) for c in (cb, cr)]
    return np.concatenate([p.reshape(-1) for p in out])


def axis_tables(h, w, fmt_in, fmt_out, loc):
    """-> ((start, coef, T) of the chroma x axis, of the chroma y axis) as scale_restatement.tables gives them"""
    (sxi, syi), (sxo, syo) = SUB[fmt_in], SUB[fmt_out]
    return sr.tables(w // sxi, w // sxo, phase(sxi, sxo, loc)), sr.tables(h // syi, h // syo, 0)


# ---------------------------------------------------------------------------------------------------------------- Y4M
def _tag_layout(tag):
    """C tag -> (format, bit depth)"""
    base, _, depth = tag.partition("p")
    if tag in ("420jpeg", "420mpeg2"):
        return "420", 8
    return base, int(depth) if depth else 8


def write_y4m(path, frames, w, h, tag=None, rate=(30, 1), extra="Ip A1:1", frame_params=""):
    """frames: packed pictures (uint8, or uint16 for a pNN tag).  tag=None writes no C tag.  frame_params: text put after
    every FRAME word."""
    head = f"YUV4MPEG2 W{w} H{h}" + (f" F{rate[0]}:{rate[1]}" if rate else "") + (f" {extra}" if extra else "") + \
        (f" C{tag}" if tag is not None else "")
    with open(path, "wb") as f:
        f.write(head.encode() + b"\n")
        for fr in frames:
            f.write(b"FRAME" + (b" " + frame_params.encode() if frame_params else b"") + b"\n")
            f.write(np.asarray(fr).astype("<u2" if np.asarray(fr).dtype.itemsize == 2 else np.uint8).tobytes())


def read_y4m(path):
    """-> ({"W", "H", "F", "I", "A", "C": the header's tags as text, None when absent}, [packed pictures])"""
    data = open(path, "rb").read()
    line, _, rest = data.partition(b"\n")
    words = line.decode().split(" ")
    assert words[0] == "YUV4MPEG2"
    info = dict.fromkeys("WHFIAC")
    for word in words[1:]:
        info[word[0]] = word[1:]
    fmt, depth = _tag_layout(info["C"] or "420jpeg")
    n = samples(int(info["H"]), int(info["W"]), fmt)
    size = n * (2 if depth > 8 else 1)
    frames = []
    while rest:
        marker, _, rest = rest.partition(b"\n")
        assert marker == b"FRAME" or marker.startswith(b"FRAME "), marker
        assert len(rest) >= size, "the file ends inside a picture"
        frames.append(np.frombuffer(rest[:size], dtype="<u2" if depth > 8 else np.uint8).astype(
            np.uint16 if depth > 8 else np.uint8))
        rest = rest[size:]
    return info, frames
