#!/usr/bin/env python3
"""Check a folder coded to a bitrate (tools/encode_sequence.py --bitrate) against its rate_control.json, with no GPU and no
codec (pmctf_rate.verify_rate_record): every GOP's size from its files, the credit arithmetic, every fits flag, the q_index
of every GOP against gop_structure.json.

    python tools/check_rate.py BIN_FOLDER

Prints one line per GOP (q_index, bits, budget, credit, trials) and the bits per second the sequence came to; exit
status 1 and the first violation when the record does not hold."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learned-pmctf_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("bin_folder")
    a = ap.parse_args(argv)
    import pmctf_rate
    try:
        v = pmctf_rate.verify_rate_record(a.bin_folder)
    except ValueError as e:
        print(f"rate record does not hold: {e}")
        return 1
    rec = v["record"]
    print(f"{'GOP':>5} {'first':>6} {'size':>4} {'q':>3} {'bits':>12} {'budget':>12} {'credit':>12} {'fits':>5} trials")
    for k, (g, r) in enumerate(zip(v["header"]["gops"], rec["gops"])):
        print(f"{k:>5} {g['first']:>6} {g['size']:>4} {r['q_index']:>3} {r['bits']:>12} {r['budget']:>12} {r['credit']:>12} "
              f"{'yes' if r['fits'] else 'NO':>5} {' '.join(f'{q}:{b}' for q, b in r['trials'])}")
    num, den = rec["fps"]
    misses = sum(not r["fits"] for r in rec["gops"])
    print(f"{v['frame_num']} pictures at {num}/{den} per second, {v['total_bits']} bits: {v['bits_per_second']:.0f} bits per "
          f"second, target {rec['bitrate']}; {misses} of {len(rec['gops'])} GOPs over their budget")
    return 0


if __name__ == "__main__":
    sys.exit(main())
