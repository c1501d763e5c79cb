"""Temporal layers: a coded sequence at 1/2^k of its frame rate, decoded from a subset of its files.

Stage s of a GOP turns pairs of pictures into a low-band and a high-band picture and the next stage works on the low-band
pictures alone (pmctf_gop.encode_gop), so a decoder that leaves out the high-band pictures of stages 0..k-1 and stops the
synthesis after stage k holds the GOP's low-band pictures of level k: one picture per 2^k source pictures.  Nothing in
the files has to change for that.  encode_gop names a pair's three files after its high-band picture, and both encode_gop
and the decoder restart the motion context ({"mv_feature": None, "ref_mv_y": None}) at every stage, so the motion files
of stage s decode without any file of an earlier stage.

Level k >= 0; a GOP of size = 2^S pictures; kk = min(k, S): a GOP shallower than k gives its one low-band picture.
  layer_times, layer_file_names, layer_bytes     the plan: which pictures come out, which files are read (pure Python)
  decode_gop_files_layer, decode_sequence_layer  the decoder, on pmctf_gop's batched file decode and inverse_MCTF
  write_layer_hashes, read_layer_hashes          layer_hashes.json: the CRC-32 of every layer picture, from a full decode
  extract_layer                                  copies exactly the files of a level into a new folder (no codec, no GPU)
motion_fill=True is the other classical use of the same picture files: the motion of the left-out stages is read as
well, their high-band pictures are taken as zero and the whole synthesis runs, which gives every picture of the GOP.
The plan, the hash record and extract_layer need no GPU; the decoders have no CPU path."""
import os

import pmctf_gop
import pmctf_spatial
from pmctf_records import is_int, read_record, write_record

LAYER_HASHES = "layer_hashes.json"
LAYER_HASH_FORMAT_VERSION = 1
LAYER_EXTRACT = "layer_extract.json"
LAYER_EXTRACT_VERSION = 1
L_FILES = ("0_main.bin", "0_C_main.bin")


def check_level(level):
    """the temporal level as given: an integer >= 0; ValueError otherwise"""
    if not is_int(level) or level < 0:
        raise ValueError(f"level is an integer, 0 or more (got {level!r})")
    return level


def gop_stages(gop):
    """S of a GOP of 2^S pictures (0 for a lone picture); ValueError for a size that is not a power of two"""
    if not is_int(gop) or gop < 1 or gop & (gop - 1):
        raise ValueError(f"the GOP length must be a power of two (got {gop!r})")
    return gop.bit_length() - 1


# --------------------------------------------------------------------------------------------------------------- the plan
def layer_times(gops, level):
    """[(gop index, source picture index)] of the pictures a level-`level` decode gives, in output order.  gops: the list
    pmctf_gop.sequence_layout returns, [(first, size, ...)].  GOP (first, size = 2^S) yields first + j * 2^kk for
    j < size >> kk, kk = min(level, S): a GOP shallower than the level yields its one low-band picture, a lone picture
    itself, level 0 every picture."""
    check_level(level)
    out = []
    for k, g in enumerate(gops):
        first, size = g[0], g[1]
        kk = min(level, gop_stages(size))
        out += [(k, first + (j << kk)) for j in range(size >> kk)]
    return out


def layer_file_names(gop, level, motion_fill=False):
    """the files a level-`level` decode of one GOP of `gop` pictures reads, in pmctf_gop.gop_file_names order: the three
    files of every pair whose stage is >= kk, then 0_main.bin and 0_C_main.bin.  motion_fill: the {i}_mv.bin of the pairs
    of stages < kk as well.  gop == 1: the two L files.  Level 0 is gop_file_names(gop); files(k) is a subset of
    files(k - 1)."""
    check_level(level)
    kk = min(level, gop_stages(gop))
    names = []
    for stage, _, i_cur in (pmctf_gop.gop_pairs(gop) if gop != 1 else []):
        if stage >= kk:
            names += [f"{i_cur}.bin", f"{i_cur}_C_main.bin", f"{i_cur}_mv.bin"]
        elif motion_fill:
            names.append(f"{i_cur}_mv.bin")
    return names + list(L_FILES)


def layer_bytes(bin_folder, level, motion_fill=False):
    """the rate of the layer: the sizes of exactly the files a level-`level` decode of the sequence in bin_folder reads,
    summed over its GOPs.  ValueError naming a file that is missing."""
    check_level(level)
    _, gops = pmctf_gop.sequence_layout(bin_folder)
    return files_bytes(bin_folder, ((k, layer_file_names(g[1], level, motion_fill)) for k, g in enumerate(gops)))


def files_bytes(bin_folder, per_gop):
    """the sizes of the files [(gop index, names)] of the sequence in bin_folder, summed; ValueError naming a file that is
    missing"""
    total = 0
    for k, names in per_gop:
        for name in names:
            path = os.path.join(bin_folder, pmctf_gop.gop_folder(k), name)
            try:
                total += os.path.getsize(path)
            except FileNotFoundError:
                raise ValueError(f"{path}: missing") from None
    return total


# ---------------------------------------------------------------------------------------------------------------- one GOP
def reduce_motion(frames_coded, spatial_level):
    """the motion fields of a GOP's entries for planes of spatial level k: each reduced k times by ops.bilinear_down2(., 2.0),
    which halves the size and the vectors, so that every vector contributes; once per pair, shared by luma (as it is) and
    chroma (whose synthesis, downscale=True, reduces it once more, as at full size).  Modifies and returns frames_coded."""
    from pMCTF.hip import ops
    for entry in frames_coded:
        for _ in range(spatial_level if entry[2] is not None else 0):
            entry[2] = ops.bilinear_down2(entry[2].contiguous(), 2.0)
    return frames_coded


def _check_decode_args(level, motion_fill, ll_order=None, spatial_level=0):
    check_level(level)
    pmctf_spatial.check_spatial_level(spatial_level)
    if not any(motion_fill is v for v in (True, False)):
        raise ValueError(f"motion_fill is True or False (got {motion_fill!r})")
    if ll_order is not None and ll_order not in pmctf_gop.LL_ORDERS:
        raise ValueError(f"ll_order must be one of {pmctf_gop.LL_ORDERS}")


def decode_gop_files_layer(codec, bin_folder, gop, pic_height, pic_width, q_index, level, psize=128, me_downsample=1,
                           ll_order="plane", motion_fill=False):
    """pmctf_gop.decode_gop_files at temporal level `level`: only the files of layer_file_names(gop, level, motion_fill)
    are opened (anything else in the folder may be absent, cut short or garbage); a missing, truncated or surplus-length
    file of that set raises a ValueError naming it.  The picture files go through one batch, under it the motion files of
    the stages >= kk decode stage by stage in coding order with the context reset per stage (a reduced-resolution motion
    stream at the size it was coded at), and decode_gop's loop runs for the stages S-1 .. kk with the GOP's own stage
    numbers.  The pictures are the list's entries at j * 2^kk; for kk == S there is no synthesis and the picture is the
    decoded L planes as they are.
    motion_fill=True: full-rate output from the same picture files.  The motion of the stages < kk is decoded too, the H
    planes of those stages are zero tensors, and the result is exactly pmctf_gop.decode_gop of those inputs: every picture
    of the GOP.
    pmctf_spatial.decode_gop_files_layer(..., spatial_level=k) is this function at 1/2^k of the picture size.
    Returns {"frames": [[Y, UV, None]] (padded), "times": their offsets within the GOP, "frames_coded": the decoded
    entries the synthesis consumed ([None, None, None] where nothing was read; zero H planes under motion_fill; the motion
    as reduced), "stages": S, "files": the names read, in order, "bytes_read": their sizes summed, "spatial_level",
    "size": (height, width) of the pictures, "symbols_decoded" and "payload_bytes_used": per picture file name what the
    engine decoded of it and how far into its payload it read}."""
    return _decode_gop_layer(codec, bin_folder, gop, pic_height, pic_width, q_index, level, psize, me_downsample, ll_order,
                             motion_fill, 0)


def _decode_gop_layer(codec, bin_folder, gop, pic_height, pic_width, q_index, level, psize, me_downsample, ll_order,
                      motion_fill, spatial_level):
    """decode_gop_files_layer, and at spatial_level=k > 0 (pmctf_spatial) the same loop at 1/2^k of the size:
    _decode_gop_planned with the plan of a level.  Without motion_fill that is the full plan of a GOP of gop >> kk pictures
    with every index shifted left by kk: the pairs of the stages S-1 .. kk and their files."""
    def plan():
        kk = min(level, gop_stages(gop))
        pairs = pmctf_gop.gop_pairs(gop) if gop != 1 else []
        pictures = {i_cur for stage, _, i_cur in pairs if stage >= kk}
        if not motion_fill:
            return pmctf_gop.synthesis_pairs(gop, kk), pictures, pictures, [], [j << kk for j in range(gop >> kk)]
        fill = [i_cur for stage, _, i_cur in pairs if stage < kk]
        return pmctf_gop.synthesis_pairs(gop), pictures, pictures | set(fill), fill, list(range(gop))

    return _decode_gop_planned(codec, bin_folder, gop, pic_height, pic_width, q_index, psize, me_downsample, ll_order,
                               spatial_level, plan, level, motion_fill)[0]


def _decode_gop_planned(codec, bin_folder, gop, pic_height, pic_width, q_index, psize, me_downsample, ll_order, spatial_level,
                        plan, level=0, motion_fill=False, one_sided=False):
    """The one per-GOP body under the temporal levels, motion_fill, the spatial levels and random access
    (pmctf_access.decode_gop_files_frames): the argument checks, the size of the pictures, pmctf_gop's reader, the motion
    reduced for the spatial level, the zero H planes, pmctf_gop's synthesis loop and the counters.
    plan: called once the arguments are checked -> (pairs: [(stage, i_ref, i_cur, want_cur)] for pmctf_gop.synthesise,
    pictures, motions: the sets of i_cur whose picture and motion files are read, fill: the i_cur whose H planes are zero
    tensors, times: the offsets of the pictures that come out).
    At spatial_level=k every picture file is decoded at spatial level k (nothing behind its level-k subbands is read from the
    stream), the motion fields are reduced k times (reduce_motion) and the synthesis runs on the reduced planes; the pictures
    are padded planes of 1/2^k of the size, to be cropped to pmctf_spatial.spatial_size.  A size that does not offer the
    level raises the ValueError of spatial_size before any file is opened.
    one_sided: pmctf_gop.synthesise's, for a plan with pairs whose want_cur is False.  -> (decode_gop_files_layer's dict, the plan's pairs)."""
    import torch
    _check_decode_args(level, motion_fill, ll_order, spatial_level)
    if not any(one_sided is v for v in (True, False)):
        raise ValueError(f"one_sided is True or False (got {one_sided!r})")
    size = pmctf_spatial.spatial_size(pic_height, pic_width, spatial_level)
    stages = gop_stages(gop)
    pairs, pictures, motions, fill, times = plan()
    counters = {}
    with torch.no_grad():
        frames_coded, read, nbytes = pmctf_gop._read_gop_files(codec, bin_folder, gop, pic_height, pic_width, q_index, psize,
                                                               me_downsample, ll_order, pictures, motions, spatial_level,
                                                               counters)
        for i in motions - pictures - set(fill):          # decoded for the context of a later pair alone
            frames_coded[i][2] = None
        reduce_motion(frames_coded, spatial_level)
        for i in fill:
            frames_coded[i][0] = torch.zeros_like(frames_coded[0][0])
            frames_coded[i][1] = torch.zeros_like(frames_coded[0][1])
        coded = [list(fc) for fc in frames_coded]
        pmctf_gop.synthesise(codec, frames_coded, pairs, one_sided=one_sided)
    return {"frames": [frames_coded[t] for t in times], "times": times, "frames_coded": coded, "stages": stages, "files": read,
            "bytes_read": nbytes, "spatial_level": spatial_level, "size": size,
            "symbols_decoded": {n: c["symbols_decoded"] for n, c in counters.items()},
            "payload_bytes_used": {n: c["payload_bytes_used"] for n, c in counters.items()}}, pairs


# ------------------------------------------------------------------------------------------------------------ layer hashes
def _max_level(gops):
    return max(gop_stages(g[1]) for g in gops)


def _layer_path(bin_folder):
    return os.path.join(bin_folder, LAYER_HASHES)


def _check_layer_record(path, record, gops):
    """what a layer hash record says against the folder's layout (see read_layer_hashes)"""
    level, layers = record["level"], record["layers"]
    if level not in pmctf_gop.HASH_LEVELS:
        raise ValueError(f"{path}: level {level!r}, this decoder knows {pmctf_gop.HASH_LEVELS}")
    names = [str(k) for k in range(1, _max_level(gops) + 1)]
    if not isinstance(layers, dict) or sorted(layers) != sorted(names):
        got = sorted(layers) if isinstance(layers, dict) else layers
        raise ValueError(f"{path}: layers {got!r}, the sequence has the layers {names}")
    keys = set(pmctf_gop.HASH_KEYS[level]) | {"index"}
    for k in names:
        recs = layers[k]
        if not isinstance(recs, list) or not all(isinstance(r, dict) and set(r) == keys for r in recs):
            raise ValueError(f"{path}: layer {k}: a list of records that hold exactly 'index' and "
                             f"{pmctf_gop.HASH_KEYS[level]}")
        times = [t for _, t in layer_times(gops, int(k))]
        if [r["index"] for r in recs] != times:
            raise ValueError(f"{path}: layer {k}: source indices {[r['index'] for r in recs]}, the layout gives {times}")
        for r in recs:
            for key, v in r.items():
                if key != "index" and (not is_int(v) or not 0 <= v <= 0xffffffff):
                    raise ValueError(f"{path}: layer {k}: picture {r['index']}: {key} is not a 32-bit value ({v!r})")


def read_layer_hashes(bin_folder):
    """-> {"format_version", "level", "layers": {"1": [{"index", *HASH_KEYS[level]}], ...}} of bin_folder/layer_hashes.json.
    ValueError naming the path for a missing or malformed file, another version, unknown or missing fields, an unknown
    hash level, layers other than 1..log2(largest GOP), and a layer whose source indices are not layer_times of the
    folder's layout."""
    path = _layer_path(bin_folder)
    _, gops = pmctf_gop.sequence_layout(bin_folder)
    record = read_record(path, "layer hash file", LAYER_HASH_FORMAT_VERSION, fields=("level", "layers"),
                         missing="write_layer_hashes was not run on the folder")
    _check_layer_record(path, record, gops)
    return record


def _open_for_hashes(codec, bin_folder, hash_level):
    """what write_layer_hashes and pmctf_spatial.write_spatial_hashes do before their first GOP: the folder's layout and bit
    depth, its recorded picture hashes where it has some, the hash level (that of the record by default, or "u8", "u16"
    above 8 bits, without one), the refusal of an extracted folder and the header check against the codec
    -> (header, gops, bitdepth, recorded or None, hash_level)"""
    G = pmctf_gop
    header, gops = G.sequence_layout(bin_folder)
    bitdepth = G.read_picture_format(bin_folder)
    recorded = None
    if os.path.exists(os.path.join(bin_folder, G.PICTURE_HASHES)):
        recorded = G.read_picture_hashes(bin_folder, header["frame_num"])
    if hash_level is None:
        hash_level = recorded["level"] if recorded is not None else ("u16" if bitdepth > 8 else "u8")
    G.check_hash_level(hash_level, bitdepth)
    if os.path.exists(os.path.join(bin_folder, LAYER_EXTRACT)):
        raise ValueError(f"{os.path.join(bin_folder, LAYER_EXTRACT)}: an extracted folder cannot be decoded fully")
    G.check_sequence_header(header, G.codec_header_fields(codec))
    return header, gops, bitdepth, recorded, hash_level


def _gop_snapshots(codec, folder, size, h, w, q_index, psize, me_downsample, ll_order, spatial_level=0):
    """one GOP decoded from all of its files at a spatial level -> {t: the pictures of temporal level t}, t = 0..S, out of
    ONE synthesis (pmctf_gop.synthesise's snapshots)"""
    coded, _, _ = pmctf_gop._read_gop_files(codec, folder, size, h, w, q_index, psize, me_downsample, ll_order,
                                            spatial_level=spatial_level)
    shots = {}
    pmctf_gop.synthesise(codec, reduce_motion(coded, spatial_level), pmctf_gop.synthesis_pairs(size), snapshots=shots)
    return shots


def _check_full_rate(pictures, recorded, h, w, bitdepth, first, g, folder):
    """GOP g's full-rate pictures against the folder's recorded picture hashes, where it has some: PictureHashMismatch"""
    if recorded is None:
        return
    G = pmctf_gop
    bad = G.compare_hash_records(G.picture_hashes(pictures, h, w, recorded["level"], bitdepth),
                                 recorded["frames"][first:first + len(pictures)], first, gop=g, folder=folder)
    if bad:
        raise G.PictureHashMismatch(bad[0])


def write_layer_hashes(codec, bin_folder, hash_level=None):
    """Decode bin_folder fully, GOP by GOP, and write bin_folder/layer_hashes.json: for every k from 1 to log2 of the
    largest GOP the CRC-32 (pmctf_gop.picture_hashes) of every picture of layer k, taken out of the SAME synthesis as the
    full-rate pictures, from the list as it stands once stage min(k, S) is undone.  Where picture_hashes.json is present
    every GOP's full-rate pictures are checked against it first (PictureHashMismatch, nothing written): the layer record
    is then anchored to the encoder's own reconstruction.  hash_level: that of picture_hashes.json by default, or "u8"
    ("u16" above 8 bits) without one.  -> the path written."""
    import torch
    G = pmctf_gop
    header, gops, bitdepth, recorded, hash_level = _open_for_hashes(codec, bin_folder, hash_level)
    h, w = header["height"], header["width"]
    top = _max_level(gops)
    q_indexes = G.gop_q_indexes(header, len(gops))
    layers = {str(k): [] for k in range(1, top + 1)}
    with torch.no_grad():
        for g, (first, size, psize, me_downsample) in enumerate(gops):
            folder = os.path.join(bin_folder, G.gop_folder(g))
            shots = _gop_snapshots(codec, folder, size, h, w, q_indexes[g], psize, me_downsample, header["ll_order"])
            _check_full_rate(shots[0], recorded, h, w, bitdepth, first, g, folder)
            for k in range(1, top + 1):
                kk = min(k, gop_stages(size))
                for j, rec in enumerate(G.picture_hashes(shots[kk], h, w, hash_level, bitdepth)):
                    layers[str(k)].append(dict({key: int(rec[key]) for key in G.HASH_KEYS[hash_level]},
                                               index=first + (j << kk)))
    record = {"format_version": LAYER_HASH_FORMAT_VERSION, "level": hash_level, "layers": layers}
    path = _layer_path(bin_folder)
    _check_layer_record(path, record, gops)
    return write_record(path, record, indent=1)


# ------------------------------------------------------------------------------------------------------------- extraction
def read_layer_extract(bin_folder):
    """-> None for a folder without layer_extract.json, else its record {"format_version", "min_level", "motion"};
    ValueError naming the path for a malformed file, another version or other fields"""
    path = os.path.join(bin_folder, LAYER_EXTRACT)
    record = read_record(path, "layer extract file", LAYER_EXTRACT_VERSION, fields=("min_level", "motion"),
                         expected="format_version, min_level and motion")
    if record is None:
        return None
    if not is_int(record["min_level"]) or record["min_level"] < 0 or not isinstance(record["motion"], bool):
        raise ValueError(f"{path}: min_level {record['min_level']!r}, motion {record['motion']!r}")
    return record


def _check_against_extract(bin_folder, level, motion_fill):
    """refuse what an extracted folder cannot give: a level below its min_level, motion_fill without its motion files"""
    marker = read_layer_extract(bin_folder)
    if marker is None:
        return
    path = os.path.join(bin_folder, LAYER_EXTRACT)
    if level < marker["min_level"]:
        raise ValueError(f"{path}: the folder holds the files of temporal level {marker['min_level']} and above, "
                         f"level {level} cannot be decoded from it")
    if motion_fill and not marker["motion"] and marker["min_level"] > 0:
        raise ValueError(f"{path}: the folder was extracted without the motion files of the left-out stages "
                         f"(motion: false), motion_fill cannot be decoded from it")


def extract_layer(src_folder, dst_folder, level, motion_fill=False):
    """Copy what a level-`level` decode of the sequence in src_folder reads into dst_folder (created when missing; refused
    when not empty): the header, picture_format.json, display_format.json, source_format.json, layer_hashes.json and
    spatial_hashes.json where present, per GOP
    exactly layer_file_names(size, level, motion_fill), and layer_extract.json {"format_version", "min_level": level, "motion":
    motion_fill}, which decode_sequence_layer reads.  picture_hashes.json is not copied: the folder cannot produce those
    pictures.  No codec, no GPU.  -> the relative paths written, sorted."""
    import shutil
    _check_decode_args(level, motion_fill)
    G = pmctf_gop
    _, gops = G.sequence_layout(src_folder)
    _check_against_extract(src_folder, level, motion_fill)
    if os.path.exists(dst_folder) and (not os.path.isdir(dst_folder) or os.listdir(dst_folder)):
        raise ValueError(f"{dst_folder}: not an empty folder; extract_layer writes into a new or empty one")
    import pmctf_chroma
    import pmctf_scale
    copies = [n for n in (G.GOP_STRUCTURE, G.SEQUENCE_HEADER, G.PICTURE_FORMAT, pmctf_scale.DISPLAY_FORMAT,
                          pmctf_chroma.SOURCE_FORMAT, LAYER_HASHES, pmctf_spatial.SPATIAL_HASHES)
              if os.path.exists(os.path.join(src_folder, n))]
    for k, g in enumerate(gops):
        copies += [os.path.join(G.gop_folder(k), n) for n in layer_file_names(g[1], level, motion_fill)]
    for rel in copies:
        if not os.path.isfile(os.path.join(src_folder, rel)):
            raise ValueError(f"{os.path.join(src_folder, rel)}: missing")
    os.makedirs(dst_folder, exist_ok=True)
    for rel in copies:
        os.makedirs(os.path.dirname(os.path.join(dst_folder, rel)), exist_ok=True)
        shutil.copyfile(os.path.join(src_folder, rel), os.path.join(dst_folder, rel))
    write_record(os.path.join(dst_folder, LAYER_EXTRACT),
                 {"format_version": LAYER_EXTRACT_VERSION, "min_level": level, "motion": bool(motion_fill)}, indent=1)
    return sorted(copies + [LAYER_EXTRACT])


# ------------------------------------------------------------------------------------------------------------ a sequence
def spatial_picture_size(bin_folder, h, w, spatial_level, verify, coded_size_output, coded_format_output):
    """-> pmctf_spatial.spatial_size of the folder's pictures, with the refusals of a spatial level that need no codec, for
    LayerDecode and pmctf_access.FrameDecode: a size that does not offer the level, a display form the reduced pictures
    cannot be given, verify=True without spatial_hashes.json"""
    size = pmctf_spatial.spatial_size(h, w, spatial_level)
    if spatial_level:
        import pmctf_chroma
        import pmctf_scale
        source = pmctf_chroma.read_source_format(bin_folder)
        other_format = source is not None and source["chroma_format"] != "420"
        for name, differs, coded in ((pmctf_scale.DISPLAY_FORMAT, True, coded_size_output),
                                     (pmctf_chroma.SOURCE_FORMAT, other_format, coded_format_output)):
            path = os.path.join(bin_folder, name)
            if os.path.exists(path) and differs and not coded:
                raise ValueError(f"{path}: the folder's pictures are displayed in another form than they are coded in; "
                                 f"spatial level {spatial_level} gives the coded form alone (ask for the coded "
                                 f"size and the coded format), resampling a reduced picture is not done")
        path = os.path.join(bin_folder, pmctf_spatial.SPATIAL_HASHES)
        if verify is True and not os.path.exists(path):
            raise ValueError(f"{path}: missing (write_spatial_hashes was not run on the folder)")
    return size


class LayerDecode(pmctf_gop.FullDecode):
    """pmctf_gop.decode_sequence_with at a temporal level: every GOP through decode_gop_files_layer, the pictures checked
    against picture_hashes.json where they are the full-rate ones (level 0, or a sequence of lone pictures: exactly
    FullDecode's record) and against layer_hashes.json above; never under motion_fill.  The result gains "level", "times"
    and "bytes_read".
    spatial_level=k > 0: the pictures have pmctf_spatial.spatial_size and are checked against the record of (k, level) in
    spatial_hashes.json; the refusals that need no codec (a size that does not offer the level, a display form the reduced
    pictures cannot be given, verify=True without the record) are raised before the codec is looked at.  The result
    gains "spatial_level", "size" and, per GOP, "symbols_decoded" and "payload_bytes_used" per picture file."""

    def __init__(self, level, motion_fill=False, spatial_level=0):
        _check_decode_args(level, motion_fill, spatial_level=spatial_level)
        self.level, self.motion_fill, self.spatial_level = level, motion_fill, spatial_level
        self.verify, self.size, self.counters = "auto", None, {"symbols_decoded": [], "payload_bytes_used": []}

    def refuse(self, verify):
        if self.motion_fill and verify is True:
            raise ValueError("motion_fill output is never verified: there is no record of it (verify=True refused)")
        self.verify = verify

    def check_folder(self, bin_folder):
        _check_against_extract(bin_folder, self.level, self.motion_fill)

    def picture_size(self, bin_folder, h, w, coded_size_output, coded_format_output):
        self.size = spatial_picture_size(bin_folder, h, w, self.spatial_level, self.verify, coded_size_output,
                                         coded_format_output)
        return self.size

    def open(self, bin_folder, header, gops, verify):
        top = _max_level(gops)
        self.full_rate = (self.level == 0 or top == 0) and not self.spatial_level   # lone pictures: one layer, the full-rate one
        if self.motion_fill or verify is False:
            return
        if self.spatial_level:
            if verify != "auto" or os.path.exists(os.path.join(bin_folder, pmctf_spatial.SPATIAL_HASHES)):
                rec = pmctf_spatial.read_spatial_hashes(bin_folder)
                self.frames = rec["layers"][str(self.spatial_level)][str(min(self.level, top))]
                self.hash_level = rec["level"]
        elif self.full_rate:
            super().open(bin_folder, header, gops, verify)
        elif verify != "auto" or os.path.exists(_layer_path(bin_folder)):
            layers = read_layer_hashes(bin_folder)
            self.frames, self.hash_level = layers["layers"][str(min(self.level, top))], layers["level"]

    def decode_gop(self, codec, folder, size, h, w, q_index, psize, me_downsample, ll_order):
        out = _decode_gop_layer(codec, folder, size, h, w, q_index, self.level, psize, me_downsample, ll_order,
                                self.motion_fill, self.spatial_level)
        for key, per_gop in self.counters.items():
            per_gop.append(out[key])
        return out["frames"], out["times"], out["bytes_read"]

    def recorded(self, first, size, at, n):
        return super().recorded(first, size, at, n) if self.full_rate else self.frames[at:at + n]

    def result(self, times, nbytes):
        return dict({"level": self.level, "times": times, "bytes_read": nbytes, "spatial_level": self.spatial_level,
                     "size": self.size}, **self.counters)


def decode_sequence_layer(codec, bin_folder, yuv_out, level, device=None, png_out=None, verify="auto", motion_fill=False):
    """pmctf_gop.decode_sequence_checked at temporal level `level`: the folder's header (either kind), its
    picture_format.json (16-bit output above 8 bits, png_out refused) and the codec checks are the same, and every GOP is
    decoded with decode_gop_files_layer from its own size, psize and me_downsample.  The .yuv holds the pictures of
    layer_times in order; the PNGs are named by SOURCE picture index.
    level=0 without motion_fill writes the bytes decode_sequence writes and verifies against picture_hashes.json as it
    does.  Above level 0 the pictures are verified against layer_hashes.json (write_layer_hashes) under the same four
    verify modes: "auto" checks when the file is there, True insists on it, False never looks, "report" checks, writes
    everything and lists the mismatches; under "auto" and True the first mismatch raises PictureHashMismatch with none of
    that GOP's pictures written.  motion_fill output is never verified, and verify=True is refused with it.
    A folder written by extract_layer (layer_extract.json) refuses a level below its min_level, and motion_fill when it
    holds no motion files for the left-out stages.
    A folder with a display_format.json has its pictures resampled to the display size after the checks, as
    decode_sequence_checked does; pmctf_scale.decode_sequence_layer(..., coded_size_output=True) writes them
    as coded.  A source_format.json and a yuv_out ending in .y4m are honoured as decode_sequence_checked honours them
    (pmctf_chroma.decode_sequence_layer(..., coded_format_output=True): the coded 4:2:0 pictures).
    pmctf_spatial.decode_sequence_layer(..., spatial_level=k) is this function at 1/2^k of the picture size.
    Returns decode_sequence's dict ("frames", "seconds", "verified", "hash_mismatches", "header", "bitdepth") plus "level",
    "times": the source index of every written picture, "bytes_read": the sizes of the files read, layer_bytes,
    "spatial_level", "size": (height, width) of the decoded pictures (the coded size here), and "symbols_decoded" and
    "payload_bytes_used": per GOP, per picture file name, the symbols the engine decoded and how many bytes of the payload
    it read."""
    return pmctf_gop.decode_sequence_with(LayerDecode(level, motion_fill), codec, bin_folder, yuv_out, device, png_out, verify)
