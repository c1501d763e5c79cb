#!/usr/bin/env python3
"""Convert a raw file of pictures between an RGB layout and planar 4:4:4 YCbCr on the GPU (pmctf_colour.convert_file,
DESIGN 5s).

    python tools/convert_colour.py --width 1920 --height 1080 --from rgb24 --to planar444 IN.rgb OUT_444.yuv
    python tools/convert_colour.py --width 1920 --height 1080 --from planar444 --to gbrp10 --matrix bt2020 IN.yuv OUT.gbr

One side is one of pmctf_colour.LAYOUTS (rgb24, bgr24, rgba, bgra, rgb48, gbrp, gbrp10, gbrp12, gbrp16), the other
"planar444": the packed planar 4:4:4 pictures of the layout's depth, bytes at 8 bits and little-endian 16-bit words above,
which is what tools/encode_sequence.py reads with --chroma-format 444 (and --bitdepth) and tools/decode_sequence.py writes
for such a folder.  --matrix bt601|bt709|bt2020 and --range full|limited are the colour description (default bt709
limited); the arithmetic is the 29-bit fixed point of the format.  Prints the number of pictures as JSON.  The counterpart
of tools/convert_layout.py."""
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
    ap.add_argument("--from", dest="from_layout", required=True, metavar="NAME", help="layout of IN, or planar444")
    ap.add_argument("--to", dest="to_layout", required=True, metavar="NAME", help="layout of OUT, or planar444")
    ap.add_argument("--matrix", default="bt709", help="bt601, bt709 (default) or bt2020")
    ap.add_argument("--range", dest="range_", default="limited", help="full or limited (default)")
    ap.add_argument("--bitdepth", type=int, help="checked against the layout's when given")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("src")
    ap.add_argument("dst")
    a = ap.parse_args(argv)
    import pmctf_colour
    try:
        n = pmctf_colour.convert_file(a.src, a.dst, a.width, a.height, a.from_layout, a.to_layout, (a.matrix, a.range_),
                                      a.device, a.bitdepth)
    except (OSError, ValueError) as e:
        ap.error(str(e))
    print(json.dumps({"frames": n, "width": a.width, "height": a.height, "from": a.from_layout, "to": a.to_layout,
                      "matrix": a.matrix, "range": a.range_, "out": a.dst}))


if __name__ == "__main__":
    main()
