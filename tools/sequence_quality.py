#!/usr/bin/env python3
"""Quality of a decoded planar 8-bit 4:2:0 file against its source: YUV-, RGB-, Y-, Cb-, Cr-PSNR and MS-SSIM per frame.

    python tools/sequence_quality.py SRC.yuv REC.yuv --width 1920 --height 1080 [--frames N] [--json out.json]

One line per frame in the evaluation script's wording, then the averages.  With tools/decode_sequence.py this closes the
loop  bitstream folder -> .yuv -> quality.  The metrics run on the GPU (pmctf_gop.sequence_quality).  --bitdepth B (9..16):
both files hold little-endian 16-bit samples of that depth; the PSNRs are against 2^B - 1, RGB-PSNR and MS-SSIM (defined
on 8-bit RGB) are reported as 0.  Per-plane MS-SSIM at the files' own depth and chroma format: tools/compare_sequences.py."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learned-pmctf_amd"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("src_yuv")
    ap.add_argument("rec_yuv")
    ap.add_argument("--width", type=int, required=True)
    ap.add_argument("--height", type=int, required=True)
    ap.add_argument("--frames", type=int, help="number of pictures to compare (default: all of the shorter file)")
    ap.add_argument("--gop", type=int, help="GOP length, to label the frame types as encode_sequence does")
    ap.add_argument("--no-msssim", action="store_true", help="PSNR only")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--bitdepth", type=int, default=8, help="bit depth of both files: 8, or 9..16 for 16-bit samples")
    ap.add_argument("--json", help="write the per-frame tables and their means here")
    a = ap.parse_args()
    if a.width <= 0 or a.height <= 0 or (a.width | a.height) & 1:
        ap.error("width and height must be even and positive")
    if a.bitdepth != 8 and not 9 <= a.bitdepth <= 16:
        ap.error("bitdepth is 8 or 9..16")
    frame_bytes = (a.width * a.height + 2 * (a.width // 2) * (a.height // 2)) * (2 if a.bitdepth > 8 else 1)
    n = a.frames if a.frames is not None else min(os.path.getsize(p) for p in (a.src_yuv, a.rec_yuv)) // frame_bytes
    if n <= 0:
        ap.error("no complete picture to compare")
    import pmctf_gop
    out = pmctf_gop.sequence_quality(a.src_yuv, a.rec_yuv, a.width, a.height, n, a.device, gop=a.gop,
                                     msssim=not a.no_msssim, bitdepth=a.bitdepth)
    for line in out["lines"]:
        print(line)
    m = out["mean"]
    print(f"average of {n} frames, YUV-PSNR: {m['psnr']:.4f}, RGB-PSNR: {m['psnr_rgb']:.4f}, MS-SSIM: {m['msssim']:.4f}, "
          f"Y-PSNR: {m['psnr_y']:.4f}, Cb-PSNR: {m['psnr_cb']:.4f}, Cr-PSNR: {m['psnr_cr']:.4f}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump({k: v for k, v in out.items() if k != "lines"}, f, indent=2)
            f.write("\n")


if __name__ == "__main__":
    main()
