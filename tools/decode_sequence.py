#!/usr/bin/env python3
"""Decode a folder written by pmctf_gop.encode_sequence(keep_gops=True) into a planar 8-bit 4:2:0 file.

    python tools/decode_sequence.py --checkpoint model.pth BIN_FOLDER OUT.yuv
    python tools/decode_sequence.py --synth-seed 0 BIN_FOLDER OUT.yuv        (the deterministic synthetic weights)
    python tools/decode_sequence.py --synth-seed 0 --png DIR BIN_FOLDER      (RGB pictures DIR/{index}.png; OUT.yuv optional)

The number of motion stages comes from the folder's sequence.json (or gop_structure.json: a sequence coded with
tools/encode_sequence.py --structure, whose GOPs have their own sizes); the weights must be the ones the sequence was coded
with.  The decoder refuses a header whose arithmetic profile (PMCTF_PRECISION) or ATen thread setting
(PMCTF_ATEN_THREADS) differs from this process's.  A folder coded with --picture-hash holds the encoder's picture hashes:
every decoded picture is checked against them (a mismatch stops the decoder before that GOP is written) unless --no-verify
is given; --verify insists on the hashes being there, --verify-report writes everything and lists the mismatches.
A folder coded with --bitdepth above 8 (it holds picture_format.json) is written as little-endian 16-bit samples of that
depth; the depth found is printed with the summary.
--temporal-level K (pmctf_layers.decode_sequence_layer) decodes the sequence at 1/2^K of its frame rate from the files of
that level alone: one picture per 2^K of a GOP, a shallower GOP its one low-band picture; the PNGs keep the source
indices.  Level 1 and above are checked against layer_hashes.json (tools/encode_sequence.py --layer-hashes).
--motion-fill gives every picture from the same picture files: the motion of the left-out stages is read too and their
high-band pictures are taken as zero; that output has no hashes to be checked against.
A folder coded with --coded-size (it holds display_format.json) is written at the size of its source: every decoded picture
is resampled there on the GPU after the hashes, which describe the coded-size pictures, have been checked.
--coded-size-output writes the pictures as they were coded instead: the file tools/check_picture_hashes.py checks.
A folder coded from a .y4m or from a 4:2:2 / 4:4:4 source (it holds source_format.json) is written in the chroma format of
its source, converted on the GPU after the resampling (pmctf_chroma); --coded-format-output writes the coded
4:2:0 pictures instead.  An OUT path ending in .y4m becomes a Y4M file (its F tag is the recorded frame rate, 25:1 when
there is none).
--spatial-level K (pmctf_spatial.decode_sequence_layer) decodes every picture at 1/2^K of its size from the
coarse subbands of the same files: nothing behind the level-K subbands of a file is decoded.  The size must offer the level
(both sides multiples of 2^(K+1)); it composes with --temporal-level, --motion-fill, --png and --output-layout.  Level 1 and
above are checked against spatial_hashes.json (tools/encode_sequence.py --spatial-hashes).  A folder with a display form of
its own is decoded this way only with --coded-size-output (and --coded-format-output where the source was not 4:2:0).
--output-layout NAME (pmctf_layout) writes every picture in that pixel layout (nv12, p010, v210, ...), packed
on the GPU after the steps above; the layout must have the chroma format and depth of the pictures being written.
--compare SOURCE (pmctf_quality.compare_files) compares the file just written with SOURCE, in the chroma format
and at the bit depth both have: one line per frame and the averages, per-plane PSNR and MS-SSIM.  SOURCE is a .y4m, or a raw
planar file of the size, chroma format and depth of what was written; it needs an OUT file and is refused together with
--output-layout, --spatial-level and --temporal-level, whose outputs are not pictures of the source's form.
--frames SPEC (pmctf_access.decode_frames) decodes chosen pictures alone: SPEC is N, A:B (half-open, as in Python)
or a comma list of those, e.g. 37 or 1000:1100 or 0,8:12,40.  Only the GOPs that hold one of them are opened, and of those
only the files the pictures depend on; the pictures are written in ascending order, the PNGs under their source indices, and
each is checked against its own picture hash.  It composes with --png, --spatial-level, --coded-size-output,
--coded-format-output, --output-layout and the verify flags, and is refused together with --temporal-level, --motion-fill
and --compare.  The summary then holds the bytes of the files read and the number of GOPs opened.
--rgb-output FILE --rgb-layout NAME (pmctf_colour) also writes every verified picture as RGB in that layout
(rgb24, bgr24, rgba, bgra, rgb48, gbrp, gbrp10, gbrp12, gbrp16; of the folder's bit depth): the pictures as OUT would hold
them, converted to 4:4:4 and then to RGB on the GPU by the colour description of the folder's colour_format.json
(tools/encode_sequence.py --rgb-layout / --colour-matrix / --colour-range), or by --colour-matrix / --colour-range given
here.  --png on a folder with a colour_format.json (or with the two options) writes its PNGs by that description instead of
the harness's BT.601 full-range formulas.  Both compose with every decoder above; OUT may be left out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learned-pmctf_amd"))


def parse_frames(spec):
    """--frames SPEC -> the picture indices it names, in the order given; ValueError naming the malformed part"""
    out = []
    for part in spec.split(","):
        ends = part.split(":")
        if len(ends) > 2 or not all(e.strip().isdigit() for e in ends):
            raise ValueError(f"{part!r} is neither N nor A:B")
        ends = [int(e) for e in ends]
        out += list(range(*ends)) if len(ends) == 2 else ends
        if len(ends) == 2 and ends[0] >= ends[1]:
            raise ValueError(f"{part!r} selects no picture")
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    w = ap.add_mutually_exclusive_group(required=True)
    w.add_argument("--checkpoint", help="weights file (torch.save of a state_dict, or of a dict holding one)")
    w.add_argument("--synth-seed", type=int, help="deterministic synthetic weights (pmctf_synth) with this seed")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--png", metavar="DIR", help="also write every decoded picture there as {index}.png (RGB)")
    v = ap.add_mutually_exclusive_group()
    v.add_argument("--verify", dest="verify", action="store_const", const=True, default="auto",
                   help="check the picture hashes and fail when the folder has none (default: check them when it has)")
    v.add_argument("--no-verify", dest="verify", action="store_const", const=False, help="do not check picture hashes")
    v.add_argument("--verify-report", dest="verify", action="store_const", const="report",
                   help="check, write every picture all the same, list the mismatches and exit with status 1 if there are any")
    ap.add_argument("--temporal-level", type=int, metavar="K",
                    help="decode at 1/2^K of the frame rate from the files of that level alone (default: everything)")
    ap.add_argument("--motion-fill", action="store_true",
                    help="with --temporal-level: full frame rate, the left-out high bands taken as zero (never verified)")
    ap.add_argument("--spatial-level", type=int, metavar="K",
                    help="decode at 1/2^K of the picture size from the coarse subbands alone (default: the full size)")
    ap.add_argument("--coded-size-output", action="store_true",
                    help="a folder coded with --coded-size: write the coded-size pictures, not the display-size ones")
    ap.add_argument("--coded-format-output", action="store_true",
                    help="a folder with a source_format.json: write the coded 4:2:0 pictures, not the source's chroma format")
    ap.add_argument("--output-layout", metavar="NAME", help="write the pictures in this pixel layout (pmctf_layout.LAYOUTS)")
    ap.add_argument("--compare", metavar="SOURCE",
                    help="after the decode, compare OUT with this file: per-plane PSNR and MS-SSIM in their own format")
    ap.add_argument("--frames", metavar="SPEC",
                    help="decode these pictures alone, from the files they depend on: N, A:B (half-open) or a comma list")
    ap.add_argument("--rgb-output", metavar="FILE", help="also write every picture there as RGB (needs --rgb-layout)")
    ap.add_argument("--rgb-layout", metavar="NAME", help="the layout of --rgb-output (pmctf_colour.LAYOUTS)")
    ap.add_argument("--colour-matrix", choices=("bt601", "bt709", "bt2020"),
                    help="convert to RGB by this matrix instead of the folder's colour_format.json (needs --colour-range)")
    ap.add_argument("--colour-range", choices=("full", "limited"), help="the range that goes with --colour-matrix")
    ap.add_argument("bin_folder")
    ap.add_argument("yuv_out", nargs="?", help="may be left out when --png or --rgb-output is given")
    a = ap.parse_args(argv)
    if (a.rgb_output is None) != (a.rgb_layout is None):
        ap.error("--rgb-output and --rgb-layout go together")
    if (a.colour_matrix is None) != (a.colour_range is None):
        ap.error("--colour-matrix and --colour-range go together")
    colour = None if a.colour_matrix is None else (a.colour_matrix, a.colour_range)
    layered = a.temporal_level is not None or a.motion_fill
    if layered and (a.temporal_level or 0) < 0:
        ap.error("--temporal-level is 0 or more")
    if a.spatial_level is not None and not 0 <= a.spatial_level <= 4:
        ap.error("--spatial-level is 0 to 4")
    if a.motion_fill and a.verify is True:
        ap.error("--motion-fill output has no hashes: it cannot be combined with --verify")
    if a.yuv_out is None and a.png is None and a.rgb_output is None:
        ap.error("give OUT.yuv, --png DIR or both")
    if a.compare is not None:
        if a.yuv_out is None:
            ap.error("--compare: needs an OUT file to compare with")
        for flag, given in (("--output-layout", a.output_layout), ("--spatial-level", a.spatial_level),
                            ("--temporal-level", a.temporal_level)):
            if given is not None:
                ap.error(f"--compare: cannot be combined with {flag} (its output is not a picture of the source's form)")
        if not os.path.exists(a.compare):
            ap.error(f"--compare: no such file: {a.compare}")
    frames = None
    if a.frames is not None:
        for flag, given in (("--temporal-level", a.temporal_level is not None), ("--motion-fill", a.motion_fill),
                            ("--compare", a.compare is not None)):
            if given:
                ap.error(f"--frames: cannot be combined with {flag}")
        try:
            frames = parse_frames(a.frames)
        except ValueError as e:
            ap.error(f"--frames: {e}")
    import pmctf_layout
    if a.output_layout is not None:
        try:
            pmctf_layout.check_layout(a.output_layout, "--output-layout")
        except ValueError as e:
            ap.error(str(e))
        if a.yuv_out is None or pmctf_layout.pmctf_chroma.is_y4m(a.yuv_out):
            ap.error("--output-layout: needs an OUT file that is no .y4m (Y4M pictures are planar)")
    import pmctf_colour
    if a.rgb_layout is not None:
        try:
            pmctf_colour.check_rgb_layout(a.rgb_layout, "--rgb-layout")
        except ValueError as e:
            ap.error(str(e))
    try:                                                 # a colour description in force: the decode goes through pmctf_colour
        recorded = pmctf_colour.read_colour_format(a.bin_folder) if colour is None else None
    except ValueError as e:
        ap.error(str(e))
    if a.rgb_output is not None and colour is None and recorded is None:
        ap.error(f"--rgb-output: {os.path.join(a.bin_folder, pmctf_colour.COLOUR_FORMAT)} is missing; give --colour-matrix "
                 f"and --colour-range")
    as_rgb = (a.rgb_output is not None or a.png is not None) and (colour is not None or recorded is not None)
    import torch
    import pmctf_gop
    from pMCTF.models.video.pMCTF_L import pMCTF
    header, _ = pmctf_gop.sequence_layout(a.bin_folder)
    if a.spatial_level:                                  # what needs no weights is refused before they are loaded
        import pmctf_layers
        try:
            mode = pmctf_layers.LayerDecode(a.temporal_level or 0, a.motion_fill, a.spatial_level)
            mode.refuse(a.verify)
            mode.picture_size(a.bin_folder, header["height"], header["width"], a.coded_size_output, a.coded_format_output)
        except ValueError as e:
            ap.error(f"--spatial-level: {e}")
    if frames is not None:
        import pmctf_access
        try:
            pmctf_access.FrameDecode(frames, a.spatial_level or 0).check_folder(a.bin_folder)
        except ValueError as e:
            ap.error(f"--frames: {e}")
    net =pMCTF(num_me_stages=header["num_me_stages"]).eval()
    if a.checkpoint is not None:
        from pMCTF.utils.stream_helper import get_state_dict
        net.load_state_dict(get_state_dict(a.checkpoint), strict=True)
    else:
        import pmctf_synth
        net.load_state_dict(pmctf_synth.synth_state_dict(net.state_dict(), seed=a.synth_seed), strict=True)
    net = net.to(a.device)
    net.update(force=True)
    with torch.no_grad():
        try:
            if as_rgb:
                if frames is not None:
                    mode = pmctf_access.FrameDecode(frames, a.spatial_level or 0)
                elif layered or a.spatial_level is not None:
                    import pmctf_layers
                    mode = pmctf_layers.LayerDecode(a.temporal_level or 0, a.motion_fill, a.spatial_level or 0)
                else:
                    mode = pmctf_gop.FullDecode()
                try:
                    out = pmctf_colour.decode_with(mode, net, a.bin_folder, a.yuv_out, a.device, a.png, a.verify,
                                                   coded_size_output=a.coded_size_output,
                                                   coded_format_output=a.coded_format_output, output_layout=a.output_layout,
                                                   rgb_out=a.rgb_output, rgb_layout=a.rgb_layout, colour=colour)
                except ValueError as e:
                    if isinstance(e, pmctf_gop.PictureHashMismatch) or "rgb_layout" not in str(e):
                        raise
                    sys.exit(f"--rgb-layout: {e}")
            elif frames is not None:
                out = pmctf_access.decode_frames(net, a.bin_folder, a.yuv_out, frames, a.device, png_out=a.png,
                                                 verify=a.verify, spatial_level=a.spatial_level or 0,
                                                 coded_size_output=a.coded_size_output,
                                                 coded_format_output=a.coded_format_output, output_layout=a.output_layout)
            elif a.spatial_level is not None:
                import pmctf_spatial
                out = pmctf_spatial.decode_sequence_layer(net, a.bin_folder, a.yuv_out, a.temporal_level or 0, a.device,
                                                          png_out=a.png, verify=a.verify, motion_fill=a.motion_fill,
                                                          coded_size_output=a.coded_size_output,
                                                          coded_format_output=a.coded_format_output,
                                                          output_layout=a.output_layout, spatial_level=a.spatial_level)
            elif layered:
                out = pmctf_layout.decode_sequence_layer(net, a.bin_folder, a.yuv_out, a.temporal_level or 0, a.device,
                                                         png_out=a.png, verify=a.verify, motion_fill=a.motion_fill,
                                                         coded_size_output=a.coded_size_output,
                                                         coded_format_output=a.coded_format_output,
                                                         output_layout=a.output_layout)
            else:
                out = pmctf_layout.decode_sequence_checked(net, a.bin_folder, a.yuv_out, a.device, png_out=a.png,
                                                           verify=a.verify, coded_size_output=a.coded_size_output,
                                                           coded_format_output=a.coded_format_output,
                                                           output_layout=a.output_layout)
        except pmctf_gop.PictureHashMismatch as e:
            sys.exit(f"picture hash mismatch: {e}")
        except ValueError as e:
            if a.output_layout is None:
                raise
            sys.exit(f"--output-layout: {e}")
    n = len(out["frames"])
    height, width = out["frames"][0] if n else (header["height"], header["width"])
    print(json.dumps({"frames": n, "height": height, "width": width, "yuv": a.yuv_out, "png": a.png,
                      "bitdepth": out["bitdepth"],
                      "seconds": sum(out["seconds"]), "frames_per_second": n / max(sum(out["seconds"]), 1e-9),
                      "verified": out["verified"], "hash_mismatches": len(out["hash_mismatches"]),
                      **({"frames_wanted": out["times"], "bytes_read": out["bytes_read"], "gops_opened": out["gops_opened"],
                          "spatial_level": out["spatial_level"]} if frames is not None else {}),
                      **({"temporal_level": out["level"], "motion_fill": a.motion_fill, "bytes_read": out["bytes_read"]}
                         if frames is None and (layered or a.spatial_level is not None) else {}),
                      **({"spatial_level": out["spatial_level"],
                          "payload_bytes_used": sum(sum(g.values()) for g in out["payload_bytes_used"])}
                         if frames is None and a.spatial_level is not None else {})}))
    for m in out["hash_mismatches"]:
        print(pmctf_gop.describe_hash_mismatch(m), file=sys.stderr)
    if out["hash_mismatches"]:
        sys.exit(1)
    if a.compare is not None:
        import pmctf_chroma
        import pmctf_quality
        record = None if a.coded_format_output else pmctf_chroma.read_source_format(a.bin_folder)
        try:                                             # a raw file has the form of what was written; a .y4m its own
            q = pmctf_quality.compare_files(a.compare, a.yuv_out, a.device, width=width, height=height,
                                            chroma_format="420" if record is None else record["chroma_format"],
                                            bitdepth=out["bitdepth"])
        except ValueError as e:
            sys.exit(f"--compare: {e}")
        pmctf_quality.print_report(q)


if __name__ == "__main__":
    main()
