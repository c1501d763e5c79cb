#!/usr/bin/env python3
"""Decode a folder written by pmctf_gop.encode_sequence(keep_gops=True) into a planar 8-bit 4:2:0 file.

    python tools/decode_sequence.py --checkpoint model.pth BIN_FOLDER OUT.yuv
    python tools/decode_sequence.py --synth-seed 0 BIN_FOLDER OUT.yuv        (the deterministic synthetic weights)
    python tools/decode_sequence.py --synth-seed 0 --png DIR BIN_FOLDER      (RGB pictures DIR/{index}.png; OUT.yuv optional)

The number of motion stages comes from the folder's sequence.json; the weights must be the ones the sequence was coded
with.  The decoder refuses a header whose arithmetic profile (PMCTF_PRECISION) or ATen thread setting
(PMCTF_ATEN_THREADS) differs from this process's."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learned-pmctf_amd"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    w = ap.add_mutually_exclusive_group(required=True)
    w.add_argument("--checkpoint", help="weights file (torch.save of a state_dict, or of a dict holding one)")
    w.add_argument("--synth-seed", type=int, help="deterministic synthetic weights (pmctf_synth) with this seed")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--png", metavar="DIR", help="also write every decoded picture there as {index}.png (RGB)")
    ap.add_argument("bin_folder")
    ap.add_argument("yuv_out", nargs="?", help="may be left out when --png is given")
    a = ap.parse_args()
    if a.yuv_out is None and a.png is None:
        ap.error("give OUT.yuv, --png DIR or both")
    import torch
    import pmctf_gop
    from pMCTF.models.video.pMCTF_L import pMCTF
    header = pmctf_gop.read_sequence_header(a.bin_folder)
    net = pMCTF(num_me_stages=header["num_me_stages"]).eval()
    if a.checkpoint is not None:
        from pMCTF.utils.stream_helper import get_state_dict
        net.load_state_dict(get_state_dict(a.checkpoint), strict=True)
    else:
        import pmctf_synth
        net.load_state_dict(pmctf_synth.synth_state_dict(net.state_dict(), seed=a.synth_seed), strict=True)
    net = net.to(a.device)
    net.update(force=True)
    with torch.no_grad():
        out = pmctf_gop.decode_sequence(net, a.bin_folder, a.yuv_out, a.device, png_out=a.png)
    n = len(out["frames"])
    print(json.dumps({"frames": n, "height": header["height"], "width": header["width"], "yuv": a.yuv_out, "png": a.png,
                      "seconds": sum(out["seconds"]), "frames_per_second": n / max(sum(out["seconds"]), 1e-9)}))


if __name__ == "__main__":
    main()
