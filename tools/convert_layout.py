#!/usr/bin/env python3
"""Convert a raw file of pictures between pixel layouts on the GPU (pmctf_layout.convert_file).

    python tools/convert_layout.py --width 1920 --height 1080 --from nv12 --to planar IN.nv12 OUT.yuv
    python tools/convert_layout.py --width 1920 --height 1080 --from planar --to v210 IN_422p10.yuv OUT.v210

A layout is one of pmctf_layout.LAYOUTS (nv12, nv21, nv16, p010..p216, yuyv, uyvy, y210..y216, v210) or "planar": the
packed planar pictures of the other side's chroma format and depth, bytes at 8 bits and little-endian 16-bit words above,
which is what tools/encode_sequence.py reads (with --bitdepth / --chroma-format) and tools/decode_sequence.py writes.  The
two layouts must agree in chroma format and depth: the arithmetic is bit movement and exact, nothing is resampled or
rounded.  --pitch and --luma-rows describe IN; OUT has tight rows.  Prints the number of pictures as JSON.  The counterpart
of pmctf_gop.pngs_to_yuv for sources that are not PNGs."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learned-pmctf_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--width", type=int, required=True)
    ap.add_argument("--height", type=int, required=True)
    ap.add_argument("--from", dest="from_layout", required=True, metavar="NAME", help="layout of IN, or planar")
    ap.add_argument("--to", dest="to_layout", required=True, metavar="NAME", help="layout of OUT, or planar")
    ap.add_argument("--pitch", type=int, metavar="BYTES", help="bytes from one row of IN to the next (default: tight)")
    ap.add_argument("--luma-rows", type=int, metavar="N", help="semi-planar IN: rows of its luma plane (default: the height)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("src")
    ap.add_argument("dst")
    a = ap.parse_args(argv)
    import pmctf_layout
    try:
        n = pmctf_layout.convert_file(a.src, a.dst, a.width, a.height, a.from_layout, a.to_layout, a.device, a.pitch,
                                      a.luma_rows)
    except (OSError, ValueError) as e:
        ap.error(str(e))
    print(json.dumps({"frames": n, "width": a.width, "height": a.height, "from": a.from_layout, "to": a.to_layout,
                      "out": a.dst}))


if __name__ == "__main__":
    main()
