#!/usr/bin/env python3
"""Print the parsed stream header of a Y4M file and the number of pictures it holds, as one JSON line.  No GPU.

    python tools/y4m_info.py FILE.y4m

Every FRAME marker is checked; a file that ends inside a picture is reported ("truncated": true) and counts its whole
pictures.  A header pmctf_chroma refuses (interlaced, 4:1:1, alpha, mono, odd sides, ...) ends with its message and
status 1."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learned-pmctf_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("file")
    a = ap.parse_args(argv)
    import pmctf_chroma
    try:
        head = pmctf_chroma.read_y4m_header(a.file)
        reader = pmctf_chroma.PlanarReader(a.file)
    except (OSError, ValueError) as e:
        sys.exit(f"{a.file}: {e}")
    print(json.dumps(dict(head, frames=len(reader), truncated=reader.truncated), sort_keys=True))


if __name__ == "__main__":
    main()
