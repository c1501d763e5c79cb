"""Spatial layers: a coded sequence at 1/2^k of its picture size, decoded from the coarse subbands of its files.

Every coded plane is an L-level 2-D DWT (L = decomp_levels = 4) whose file is one rANS stream in the order LL, then the
levels L-1 .. 0 (HipEngine.pwave_walk), so what a decode at spatial level k needs, the LL subband and the levels >= k, is a
prefix of every file.  The level-k plane is the inverse DWT stopped after level k, times 2^-k (the low band's DC gain is 2
per 2-D level), without the post-processing network; the temporal synthesis then runs on those planes with the motion
field reduced k times by factor-2 bilinear steps, as chroma's already is once.  Level 0 is the full decode.
  max_spatial_level, spatial_size, level_symbol_count   the size rule and what a level reads (pure Python)
  write_spatial_hashes, read_spatial_hashes             spatial_hashes.json: the CRC-32 of every picture of every
                                                        (spatial level, temporal level), from the encoder side's decode
  decode_gop_files_layer, decode_sequence_layer         pmctf_layers' decoders with spatial_level=k: the one loop, in which
                                                        temporal level, motion_fill and spatial level compose
This module needs no torch at import; the decoders and write_spatial_hashes have no CPU path."""
import os

from pmctf_records import is_int, read_record, write_record

SPATIAL_HASHES = "spatial_hashes.json"
SPATIAL_HASH_FORMAT_VERSION = 1
DECOMP_LEVELS = 4


# -------------------------------------------------------------------------------------------------------------- the rule
def check_spatial_level(level, decomp_levels=DECOMP_LEVELS):
    """the spatial level as given: an integer 0..decomp_levels; ValueError otherwise"""
    if not is_int(level) or not 0 <= level <= decomp_levels:
        raise ValueError(f"spatial_level is an integer from 0 to {decomp_levels} (got {level!r})")
    return level


def _check_size(h, w):
    if not is_int(h) or not is_int(w) or h < 1 or w < 1:
        raise ValueError(f"a picture size is two integers, 1 or more (got {w!r}x{h!r})")


def max_spatial_level(h, w, decomp_levels=DECOMP_LEVELS):
    """the largest spatial level pictures of h x w offer: level k >= 1 needs h and w to be multiples of 2^(k+1), so that
    the 4:2:0 picture (h >> k) x (w >> k) has even sides; level 0, the full decode, is there for every size"""
    _check_size(h, w)
    k = 0
    while k < decomp_levels and h % (2 << (k + 1)) == 0 and w % (2 << (k + 1)) == 0:
        k += 1
    return k


def spatial_size(h, w, level):
    """-> (h >> level, w >> level), the size of the level's pictures; ValueError naming the size and the largest level it
    offers when the level is not one of them"""
    check_spatial_level(level)
    top = max_spatial_level(h, w)
    if level > top:
        raise ValueError(f"pictures of {w}x{h} offer the spatial levels 0..{top}: level {level} needs both sides to be "
                         f"multiples of {2 << level}")
    return h >> level, w >> level


def level_symbol_count(N, Hp, Wp, level, decomp_levels=DECOMP_LEVELS):
    """the symbols a level-`level` decode reads from the file of N planes padded to Hp x Wp: the LL subband's and those of
    the three subbands of every DWT level >= `level`, four steps of a quarter of the positions each (the terms of
    HipEngine.pwave_symbol_count for lvl >= level).  Level 0: all of the file's."""
    check_spatial_level(level, decomp_levels)
    n = N * (Hp >> decomp_levels) * (Wp >> decomp_levels)
    for lvl in range(level, decomp_levels):
        n += 3 * 4 * N * (Hp >> (lvl + 1)) * (Wp >> (lvl + 1))
    return n


# ------------------------------------------------------------------------------------------------------------ the record
def _path(bin_folder):
    return os.path.join(bin_folder, SPATIAL_HASHES)


def _check_spatial_record(path, record, gops, h, w):
    """what a spatial hash record says against the folder's size and layout (see read_spatial_hashes)"""
    import pmctf_gop
    import pmctf_layers
    level, layers = record["level"], record["layers"]
    if level not in pmctf_gop.HASH_LEVELS:
        raise ValueError(f"{path}: level {level!r}, this decoder knows {pmctf_gop.HASH_LEVELS}")
    if record["size"] != [w, h]:
        raise ValueError(f"{path}: size {record['size']!r}, the folder's pictures are {[w, h]}")
    names = [str(k) for k in range(1, max_spatial_level(h, w) + 1)]
    if not isinstance(layers, dict) or sorted(layers) != sorted(names):
        got = sorted(layers) if isinstance(layers, dict) else layers
        raise ValueError(f"{path}: layers {got!r}, pictures of {w}x{h} offer the spatial levels {names}")
    temporal = [str(t) for t in range(pmctf_layers._max_level(gops) + 1)]
    keys = set(pmctf_gop.HASH_KEYS[level]) | {"index"}
    for k in names:
        if not isinstance(layers[k], dict) or sorted(layers[k]) != sorted(temporal):
            got = sorted(layers[k]) if isinstance(layers[k], dict) else layers[k]
            raise ValueError(f"{path}: spatial level {k}: temporal levels {got!r}, the sequence has {temporal}")
        for t in temporal:
            recs, where = layers[k][t], f"{path}: spatial level {k}, temporal level {t}"
            if not isinstance(recs, list) or not all(isinstance(r, dict) and set(r) == keys for r in recs):
                raise ValueError(f"{where}: a list of records that hold exactly 'index' and {pmctf_gop.HASH_KEYS[level]}")
            times = [i for _, i in pmctf_layers.layer_times(gops, int(t))]
            if [r["index"] for r in recs] != times:
                raise ValueError(f"{where}: source indices {[r['index'] for r in recs]}, the layout gives {times}")
            for r in recs:
                for key, v in r.items():
                    if key != "index" and (not is_int(v) or not 0 <= v <= 0xffffffff):
                        raise ValueError(f"{where}: picture {r['index']}: {key} is not a 32-bit value ({v!r})")


def read_spatial_hashes(bin_folder):
    """-> {"format_version", "level", "size": [width, height], "layers": {"k": {"t": [{"index", *HASH_KEYS[level]}]}}} of
    bin_folder/spatial_hashes.json: per spatial level k >= 1 the folder's size offers and per temporal level t from 0 to
    log2 of the largest GOP, the pictures of pmctf_layers.layer_times(gops, t) at (h >> k) x (w >> k).  ValueError naming
    the path for a missing or malformed file, another version, unknown or missing fields, an unknown hash level, another
    size, spatial levels other than the offered ones, other temporal levels, and source indices that are not layer_times."""
    import pmctf_gop
    path = _path(bin_folder)
    header, gops = pmctf_gop.sequence_layout(bin_folder)
    record = read_record(path, "spatial hash file", SPATIAL_HASH_FORMAT_VERSION, fields=("level", "size", "layers"),
                         missing="write_spatial_hashes was not run on the folder")
    _check_spatial_record(path, record, gops, header["height"], header["width"])
    return record


def write_spatial_hashes(codec, bin_folder, hash_level=None):
    """Decode bin_folder GOP by GOP and write bin_folder/spatial_hashes.json.  As write_layer_hashes does, every GOP is
    decoded fully first and, where picture_hashes.json is present, checked against it (PictureHashMismatch, nothing
    written).  Then, for every spatial level k >= 1 the size offers, ONE reduced synthesis of the GOP runs and the
    pictures of every temporal level t are taken out of it, from the list as it stands once stage min(t, S) is undone,
    and hashed with pmctf_gop.picture_hashes at (h >> k) x (w >> k).  hash_level: that of picture_hashes.json by default,
    or "u8" ("u16" above 8 bits) without one.  -> the path written."""
    import torch
    import pmctf_gop as G
    import pmctf_layers as Y
    header, gops, bitdepth, recorded, hash_level = Y._open_for_hashes(codec, bin_folder, hash_level)
    h, w = header["height"], header["width"]
    top = Y._max_level(gops)
    levels = range(1, max_spatial_level(h, w) + 1)
    q_indexes = G.gop_q_indexes(header, len(gops))
    layers = {str(k): {str(t): [] for t in range(top + 1)} for k in levels}
    with torch.no_grad():
        for g, (first, size, psize, me_downsample) in enumerate(gops):
            folder = os.path.join(bin_folder, G.gop_folder(g))
            shots = lambda k: Y._gop_snapshots(codec, folder, size, h, w, q_indexes[g], psize, me_downsample,
                                               header["ll_order"], k)
            if recorded is not None:
                Y._check_full_rate(shots(0)[0], recorded, h, w, bitdepth, first, g, folder)
            for k in levels:
                at = shots(k)
                for t in range(top + 1):
                    tt = min(t, Y.gop_stages(size))
                    for j, rec in enumerate(G.picture_hashes(at[tt], h >> k, w >> k, hash_level, bitdepth)):
                        layers[str(k)][str(t)].append(dict({key: int(rec[key]) for key in G.HASH_KEYS[hash_level]},
                                                           index=first + (j << tt)))
    record = {"format_version": SPATIAL_HASH_FORMAT_VERSION, "level": hash_level, "size": [w, h], "layers": layers}
    path = _path(bin_folder)
    _check_spatial_record(path, record, gops, h, w)
    return write_record(path, record, indent=1)


# ----------------------------------------------------------------------------------------------------------- the decoders
def decode_gop_files_layer(codec, bin_folder, gop, pic_height, pic_width, q_index, level, psize=128, me_downsample=1,
                           ll_order="plane", motion_fill=False, spatial_level=0):
    """pmctf_layers.decode_gop_files_layer at spatial level `spatial_level`, which composes with the temporal level and
    motion_fill: the same files are opened, every picture file is decoded up to its level-k subbands (the walk of the levels
    L-1 .. k, the inverse DWT stopped there, times 2^-k, no post-processing; nothing behind is read from the stream), the
    motion fields are reduced k times by ops.bilinear_down2(., 2.0) and decode_gop's loop runs unchanged on the reduced
    planes, chroma with the field reduced once more as at full size.  Under motion_fill the zero H planes have the reduced
    shapes.  A size that does not offer the level raises the ValueError of spatial_size before any file is opened.
    Returns pmctf_layers.decode_gop_files_layer's dict: "frames" are padded planes of (pad_h >> k) x (pad_w >> k), to be
    cropped to "size" = spatial_size; "symbols_decoded" and "payload_bytes_used" say, per picture file name, how many
    symbols were decoded (level_symbol_count) and how many bytes of the payload the decoder had read when it stopped.
    spatial_level=0 is pmctf_layers.decode_gop_files_layer."""
    import pmctf_layers
    return pmctf_layers._decode_gop_layer(codec, bin_folder, gop, pic_height, pic_width, q_index, level, psize, me_downsample,
                                          ll_order, motion_fill, spatial_level)


def decode_sequence_layer(codec, bin_folder, yuv_out, level, device=None, png_out=None, verify="auto", motion_fill=False,
                          coded_size_output=False, coded_format_output=False, output_layout=None, spatial_level=0):
    """pmctf_layout.decode_sequence_layer at spatial level `spatial_level`: the pictures of the temporal level (all of them
    under motion_fill) at (height >> k) x (width >> k), from the coarse subbands of the same files.  The .yuv, the PNGs and
    an output_layout are those of pictures of that size; 16-bit samples above 8 bits.  The size must offer the level
    (ValueError naming the size and the largest level, before any file of a GOP is opened).
    Above level 0 the pictures are verified against the record of (spatial level, temporal level) in spatial_hashes.json
    (write_spatial_hashes) under the four verify modes of decode_sequence_checked: PictureHashMismatch before anything of
    the GOP is written; verify=True without the file is refused; motion_fill output is never verified.
    A folder whose display form is not its coded form (a display_format.json; a source_format.json of another chroma format
    than 4:2:0) is decoded above level 0 only where the caller asks for the coded form (coded_size_output=True,
    coded_format_output=True); otherwise a ValueError names the file: reduced pictures are not resampled.
    spatial_level=0 writes the bytes pmctf_layout.decode_sequence_layer writes.
    Returns its dict plus "spatial_level", "size": (height, width) of the decoded pictures, and "symbols_decoded" and
    "payload_bytes_used": per GOP, per picture file name, as decode_gop_files_layer gives them."""
    import pmctf_gop
    import pmctf_layers
    return pmctf_gop.decode_sequence_with(pmctf_layers.LayerDecode(level, motion_fill, spatial_level), codec, bin_folder,
                                          yuv_out, device, png_out, verify, coded_size_output=coded_size_output,
                                          coded_format_output=coded_format_output, output_layout=output_layout)
