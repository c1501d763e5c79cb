#!/usr/bin/env python3
"""Quality of one planar file against another in their own chroma format and bit depth: per-plane PSNR and MS-SSIM.

    python tools/compare_sequences.py SRC.y4m REC.y4m
    python tools/compare_sequences.py SRC.yuv REC.yuv --width 1920 --height 1080 --chroma-format 444 --bitdepth 10

One line per frame, then the averages.  A .y4m file carries its size, chroma format and depth; a raw planar file takes
--width, --height, --chroma-format (420, 422 or 444; default 420) and --bitdepth (8, or 9..16 for little-endian 16-bit
samples; default 8).  The two files must agree in all four.  PSNR is against 2^bitdepth - 1, YUV-PSNR is (6 Y + Cb + Cr) / 8,
MS-SSIM is computed per plane at the plane's own data range and printed as n/a for a plane whose smaller side is 160 or
less.  The metrics run on the GPU (pmctf_quality.compare_files)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learned-pmctf_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("src")
    ap.add_argument("rec")
    ap.add_argument("--width", type=int, help="of a raw planar file")
    ap.add_argument("--height", type=int, help="of a raw planar file")
    ap.add_argument("--chroma-format", choices=("420", "422", "444"), help="of a raw planar file (default 420)")
    ap.add_argument("--bitdepth", type=int, help="of a raw planar file: 8, or 9..16 for 16-bit samples (default 8)")
    ap.add_argument("--frames", type=int, help="number of pictures to compare (default: all of the shorter file)")
    ap.add_argument("--gop", type=int, help="GOP length, to label the frame types as encode_sequence does")
    ap.add_argument("--no-msssim", action="store_true", help="PSNR only")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--json", help="write the per-frame tables and their means here")
    a = ap.parse_args(argv)
    for name in ("src", "rec"):
        if not os.path.exists(getattr(a, name)):
            ap.error(f"no such file: {getattr(a, name)}")
    if a.bitdepth is not None and not 8 <= a.bitdepth <= 16:
        ap.error("bitdepth is 8 or 9..16")
    if a.frames is not None and a.frames <= 0:
        ap.error("--frames is positive")
    import pmctf_quality
    try:
        out = pmctf_quality.compare_files(a.src, a.rec, a.device, width=a.width, height=a.height, frame_num=a.frames,
                                          chroma_format=a.chroma_format, bitdepth=a.bitdepth, msssim=not a.no_msssim,
                                          gop=a.gop)
    except ValueError as e:
        ap.error(str(e))
    pmctf_quality.print_report(out)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({k: v for k, v in out.items() if k != "lines"}, f, indent=2)
            f.write("\n")


if __name__ == "__main__":
    main()
