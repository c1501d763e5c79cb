#!/usr/bin/env python3
"""Check a decoded planar 4:2:0 file against the picture hashes its encoder recorded, on the CPU with zlib alone.

    python tools/check_picture_hashes.py BIN_FOLDER DECODED.yuv

BIN_FOLDER was written by tools/encode_sequence.py --picture-hash u8|f32 (sequence.json, or gop_structure.json with
--structure, and picture_hashes.json); the
check is at the u8 level: the CRC-32 of every plane and of every whole frame of DECODED.yuv.  Prints the first mismatching
frame and plane and exits with status 1 on a mismatch, with status 2 when the folder or the file cannot be checked.
A folder coded above 8 bits (picture_format.json) is checked at the u16 level: two bytes per sample.
A folder coded at another size than its source's (display_format.json) records the hashes of the coded-size pictures:
DECODED.yuv is then the one tools/decode_sequence.py --coded-size-output writes."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learned-pmctf_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("bin_folder")
    ap.add_argument("yuv")
    a = ap.parse_args(argv)
    import pmctf_gop
    try:
        frames, bad = pmctf_gop.check_yuv_hashes(a.bin_folder, a.yuv)
    except (ValueError, OSError) as e:
        print(f"cannot check: {e}", file=sys.stderr)
        return 2
    if bad:
        print(f"MISMATCH ({len(bad)} values of {frames} frames differ); the first: " + pmctf_gop.describe_hash_mismatch(bad[0]))
        return 1
    print(f"{a.yuv}: all {frames} frames match {os.path.join(a.bin_folder, pmctf_gop.PICTURE_HASHES)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
