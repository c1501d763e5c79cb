#!/usr/bin/env python3
"""Copy the files of one temporal level of a coded sequence into a new folder (pmctf_layers.extract_layer): no weights, no
GPU.

    python tools/extract_temporal_layer.py SRC DST K [--motion]

DST (new or empty) receives the header, picture_format.json and layer_hashes.json where SRC has them, per GOP exactly the
files a decode at level K reads (pmctf_layers.layer_file_names) and layer_extract.json, which tells
tools/decode_sequence.py --temporal-level that levels below K are not there.  --motion also copies the motion files of the
left-out stages, which --motion-fill needs.  picture_hashes.json is not copied: DST cannot produce the full-rate
pictures.  Prints the bytes of SRC's level 0 and of DST's level K."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learned-pmctf_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("level", type=int, metavar="K")
    ap.add_argument("--motion", action="store_true", help="keep the motion files of the left-out stages (for --motion-fill)")
    a = ap.parse_args(argv)
    import pmctf_layers
    try:
        written = pmctf_layers.extract_layer(a.src, a.dst, a.level, motion_fill=a.motion)
        marker = pmctf_layers.read_layer_extract(a.src)
        base = marker["min_level"] if marker is not None else 0
        print(json.dumps({"files": len(written), "level": a.level, "motion": a.motion,
                          "bytes": pmctf_layers.layer_bytes(a.dst, a.level, a.motion),
                          "source_level": base, "source_bytes": pmctf_layers.layer_bytes(a.src, base)}))
    except ValueError as e:
        sys.exit(str(e))
    return 0


if __name__ == "__main__":
    sys.exit(main())
