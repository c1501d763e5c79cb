"""Sequences of any length: a sequence as a LIST of closed GOPs, each with its own size (1, 2, 4, ... up to a maximum) and
its own motion resolution, instead of pmctf_gop.encode_sequence's frame_num / gop equal ones.

Three ways of choosing the list (encode_sequence_gops(structure=...)):
  "fill"      plan_gops: the largest power of two that still fits, again and again: any frame count is coded whole;
  "scenecut"  a first pass over the source (sequence_activity: luma histogram and SAD of every picture against the one
              before it, pmctf_luma_activity_f32 on the GPU, exact integers), scene_cuts on its two figures, then plan_gops
              with a GOP boundary at every cut, so that no closed MCTF GOP filters two unrelated pictures together;
  "search"    the reference's rate-distortion search (pmctf_ca.search_gop, estimate mode) per window of max_gop pictures,
              whose choice is then coded once, for real, into folders a decoder can read;
or an explicit list of (size, me_downsample).

A picture with no partner (a GOP of one) is coded by the L coder alone, as the L picture of a pair is.  The folder gets
gop_structure.json (read_gop_structure) and no sequence.json: pmctf_gop.decode_sequence reads either.  Nothing here has a
CPU path for the coding itself; plan_gops, scene_cuts and the header functions are pure Python."""
import os

import pmctf_gop
from pmctf_gop import GOP_STRUCTURE, GOP_STRUCTURE_VERSION_Q      # 2: every GOP entry carries its own q_index (pmctf_rate)
from pmctf_records import check_fields, is_int, read_record, write_record

GOP_STRUCTURE_VERSION = 1                             # one q_index for the sequence
STRUCTURE_FIELDS = ("width", "height", "frame_num", "max_gop", "q_index", "num_me_stages", "ll_order", "precision",
                    "aten_threads", "gops")
GOP_FIELDS = ("first", "size", "me_downsample", "psize")
GOP_FIELDS_Q = GOP_FIELDS + ("q_index",)              # the entries of format version 2
Q_NUM = 21                                            # pWave.get_qp_num(): q_index is one of 0..20
STRUCTURES = ("fill", "scenecut", "search")
DS_FACTORS = (1, 2, 4, 8)
ACTIVITY_BATCH = 16                                   # pictures per device->host copy of sequence_activity

# Defaults of scene_cuts.  NOT tuned: there is no natural video where this project is built, only its own synthetic pans,
# on which any value between their in-scene maxima (hd 0.08, mad 19.7) and a cut between two different textures works.
# The values are common practice for histogram-based cut detection: a cut moves a quarter to a half of the picture's
# samples to other histogram bins (hd is that fraction), and the mean absolute difference guards against a global change
# of brightness that moves the histogram without changing the scene.  No test depends on them; pass your own.
HD_MIN = 0.35
MAD_MIN = 8.0


def _power_of_two(v):
    return is_int(v) and v >= 1 and not v & (v - 1)


def plan_gops(frame_num, max_gop, cuts=()):
    """-> [(first, size)]: GOPs that cover pictures 0..frame_num-1 in order.  max_gop: a power of two >= 2; cuts: picture
    indices in 1..frame_num-1 at which a new scene starts.  The segments between cuts are tiled from their start, every
    GOP the largest power of two that is <= max_gop and <= what is left of its segment: sizes come from {1, 2, 4, ...,
    max_gop} and no GOP has a cut in its interior.  21 frames, max_gop 8, a cut at 5 -> sizes 4, 1, 8, 8.
    ValueError for bad arguments."""
    if not is_int(frame_num) or frame_num < 1:
        raise ValueError(f"frame_num is a positive integer (got {frame_num!r})")
    if not _power_of_two(max_gop) or max_gop < 2:
        raise ValueError(f"max_gop is a power of two, at least 2 (got {max_gop!r})")
    cuts = list(cuts)
    for c in cuts:
        if not is_int(c) or not 1 <= c <= frame_num - 1:
            raise ValueError(f"a cut is a picture index in 1..{frame_num - 1} (got {c!r})")
    out = []
    bounds = sorted(set(cuts)) + [frame_num]
    first = 0
    for end in bounds:
        while first < end:
            size = max_gop
            while size > end - first:
                size >>= 1
            out.append((first, size))
            first += size
    return out


def scene_cuts(mad, hd, hd_min, mad_min):
    """-> sorted picture indices t with hd[t] >= hd_min and mad[t] >= mad_min (entries that are None, such as entry 0, never
    cut).  Both thresholds are needed: a pan inside a scene reaches a high mad while its histogram hardly moves, and two
    different textures of one value distribution differ in every sample while hd stays near 0.1."""
    if len(mad) != len(hd):
        raise ValueError(f"mad has {len(mad)} entries, hd {len(hd)}")
    return [t for t, (m, d) in enumerate(zip(mad, hd)) if m is not None and d is not None and d >= hd_min and m >= mad_min]


def sequence_activity(reader_factory, frame_num, device, bitdepth=8):
    """The first pass of structure="scenecut": every picture of a source against the one before it.
    reader_factory: a callable returning a fresh reader (YUVReader at either depth, PNGReader); the pictures go through the
    ingest of the coding path (pmctf_gop.read_gop_device: bytes to the device, PNGs converted there), only the previous luma
    is kept, and pmctf_luma_activity_f32 leaves 256 counts and one sum per picture in a device buffer that is copied to the
    host once per ACTIVITY_BATCH pictures.
    -> {"sad": [...], "hist_l1": [...], "mad": [...], "hd": [...]}: entry 0 of each list is None, entry t compares picture t
    with t - 1.  sad[t] = sum |v_t - v_{t-1}| over the luma samples at `bitdepth` bits and hist_l1[t] = sum_b |hist_t[b] -
    hist_{t-1}[b]| over the 256 bins of v >> (bitdepth - 8) are Python integers; mad = sad / (h w 2^(bitdepth - 8)), in 8-bit
    units; hd = hist_l1 / (2 h w), in [0, 1]."""
    import torch
    from pMCTF.hip import ops
    pmctf_gop._need_gpu(device, "sequence_activity")
    bitdepth = pmctf_gop.check_bitdepth(bitdepth)
    if not is_int(frame_num) or frame_num < 1:
        raise ValueError(f"frame_num is a positive integer (got {frame_num!r})")
    reader = reader_factory()
    hists, sads, size = [], [], None
    try:
        prev = None
        for start in range(0, frame_num, ACTIVITY_BATCH):
            n = min(ACTIVITY_BATCH, frame_num - start)
            # one buffer for the batch: n x 256 int32 counts, then n int64 sums (the first picture's sum stays 0)
            buf = torch.zeros(n * (256 * 4 + 8), dtype=torch.uint8, device=device)
            hist = buf[:n * 1024].view(torch.int32).view(n, 256)
            sad = buf[n * 1024:].view(torch.int64)
            for i in range(n):
                _, orig, shape = pmctf_gop.read_gop_device(reader, 1, device, psize=2)
                assert size in (None, shape), "picture size changes inside the sequence"
                size = shape
                cur = orig[0][0]
                ops.luma_activity(cur, prev, bitdepth, hist=hist[i], sad=None if prev is None else sad[i:i + 1])
                prev = cur
            host = buf.cpu()                                       # the batch's one copy to the host
            hists += host[:n * 1024].view(torch.int32).view(n, 256).tolist()
            sads += host[n * 1024:].view(torch.int64).tolist()
    finally:
        reader.close()
    h, w = size
    out = {"sad": [None], "hist_l1": [None], "mad": [None], "hd": [None]}
    for t in range(1, frame_num):
        l1 = sum(abs(a - b) for a, b in zip(hists[t], hists[t - 1]))
        out["sad"].append(int(sads[t]))
        out["hist_l1"].append(int(l1))
        out["mad"].append(sads[t] / (h * w * 2 ** (bitdepth - 8)))
        out["hd"].append(l1 / (2 * h * w))
    return out


# ------------------------------------------------------------------------------------------------------------- the header
def _check_gops(where, gops, frame_num, max_gop, version=GOP_STRUCTURE_VERSION):
    """the list of a structure header: contiguous from 0 to frame_num, sizes powers of two <= max_gop, me_downsample in
    DS_FACTORS, psize ca_psize(me_downsample) or the one other value the sequence uses.  version 2: every entry also holds
    its q_index, one of 0..20; entries of the other version are refused with a message that names the format version."""
    if not isinstance(gops, list) or not gops:
        raise ValueError(f"{where}: gops is a non-empty list")
    fields, other = (GOP_FIELDS_Q, GOP_FIELDS) if version == GOP_STRUCTURE_VERSION_Q else (GOP_FIELDS, GOP_FIELDS_Q)
    first, own = 0, set()
    for k, g in enumerate(gops):
        if isinstance(g, dict) and set(g) == set(other):
            raise ValueError(f"{where}: format version {version}: gops[{k}] " +
                             ("has no q_index, which every entry of version 2 holds" if version == GOP_STRUCTURE_VERSION_Q
                              else "carries q_index, which belongs to version 2"))
        if not isinstance(g, dict) or set(g) != set(fields):
            raise ValueError(f"{where}: gops[{k}] holds exactly {fields}")
        if not all(is_int(g[f]) for f in fields):
            raise ValueError(f"{where}: gops[{k}]: every field is an integer ({g!r})")
        if version == GOP_STRUCTURE_VERSION_Q and not 0 <= g["q_index"] < Q_NUM:
            raise ValueError(f"{where}: gops[{k}]: q_index {g['q_index']} is not one of 0..{Q_NUM - 1}")
        if not _power_of_two(g["size"]) or g["size"] > max_gop:
            raise ValueError(f"{where}: gops[{k}]: size {g['size']} is not a power of two up to max_gop {max_gop}")
        if g["first"] != first:
            raise ValueError(f"{where}: gops[{k}]: first is {g['first']}, the GOPs before it end at {first}")
        if g["me_downsample"] not in DS_FACTORS:
            raise ValueError(f"{where}: gops[{k}]: me_downsample {g['me_downsample']} is not one of {DS_FACTORS}")
        if g["psize"] <= 0 or g["psize"] & 1:
            raise ValueError(f"{where}: gops[{k}]: psize {g['psize']} is not even and positive")
        if g["psize"] != pmctf_gop.ca_psize(g["me_downsample"]):
            own.add(g["psize"])
        first += g["size"]
    if len(own) > 1:
        raise ValueError(f"{where}: psize values {sorted(own)}: a GOP is padded to ca_psize(me_downsample) or to the "
                         f"sequence's own psize, which is one value")
    if first != frame_num:
        raise ValueError(f"{where}: the GOPs cover {first} pictures, frame_num is {frame_num}")


def _check_structure(where, record):
    version = record["format_version"]
    for k in ("width", "height", "frame_num", "max_gop", "q_index", "num_me_stages", "aten_threads"):
        if not is_int(record[k]):
            raise ValueError(f"{where}: {k} is an integer (got {record[k]!r})")
    if record["width"] <= 0 or record["height"] <= 0 or (record["width"] | record["height"]) & 1 or record["frame_num"] < 1:
        raise ValueError(f"{where}: {record['frame_num']} pictures of {record['width']}x{record['height']}")
    if not _power_of_two(record["max_gop"]) or record["max_gop"] < 2:
        raise ValueError(f"{where}: max_gop {record['max_gop']!r} is not a power of two, at least 2")
    if record["ll_order"] not in pmctf_gop.LL_ORDERS:
        raise ValueError(f"{where}: ll_order {record['ll_order']!r}")
    if not isinstance(record["precision"], str):
        raise ValueError(f"{where}: precision {record['precision']!r}")
    _check_gops(where, record["gops"], record["frame_num"], record["max_gop"], version)
    if version == GOP_STRUCTURE_VERSION_Q and record["q_index"] != record["gops"][0]["q_index"]:
        raise ValueError(f"{where}: format version {version}: q_index {record['q_index']} is not the first GOP's "
                         f"({record['gops'][0]['q_index']})")


def write_gop_structure(bin_folder, **fields):
    """bin_folder/gop_structure.json: format version + STRUCTURE_FIELDS (all required, nothing else accepted); gops is the
    list [{"first", "size", "me_downsample", "psize"}] in order.  Checked as read_gop_structure checks it.
    Entries that all carry "q_index" as well (0..20, the first one's equal to the sequence's q_index) give format version 2,
    entries without it version 1, as ever; a list with both kinds is refused."""
    path = os.path.join(bin_folder, GOP_STRUCTURE)
    if set(fields) != set(STRUCTURE_FIELDS):
        raise ValueError(f"{path}: fields missing {sorted(set(STRUCTURE_FIELDS) - set(fields))}, "
                         f"unknown {sorted(set(fields) - set(STRUCTURE_FIELDS))}")
    with_q = {"q_index" in g for g in fields["gops"] if isinstance(g, dict)} if isinstance(fields["gops"], list) else set()
    if len(with_q) > 1:
        raise ValueError(f"{path}: gops: some entries carry q_index and some do not; format version 1 has none, "
                         f"version 2 one in every entry")
    record = {"format_version": GOP_STRUCTURE_VERSION_Q if with_q == {True} else GOP_STRUCTURE_VERSION}
    record.update({k: fields[k] for k in STRUCTURE_FIELDS})
    record["gops"] = [dict(g) if isinstance(g, dict) else g for g in fields["gops"]] if isinstance(fields["gops"], list) \
        else fields["gops"]
    _check_structure(path, record)
    return write_record(path, record, indent=1)


def read_gop_structure(bin_folder):
    """-> the record of bin_folder/gop_structure.json, format version 1 or 2 (2: a q_index in every GOP entry, see
    write_gop_structure).  ValueError naming the path for a missing or malformed file, another version, entries of the
    other version (the message names the format version), unknown or missing fields, a version-2 q_index outside 0..20 or
    other than the first GOP's, sizes that are not powers of two <= max_gop, `first` values that are not the running sum,
    a list that does not end at frame_num, a me_downsample outside {1, 2, 4, 8}, a psize other than
    ca_psize(me_downsample) or the sequence's own, and for a folder that also holds a sequence.json."""
    path = os.path.join(bin_folder, GOP_STRUCTURE)
    record = read_record(path, "GOP structure file", None, missing="not a folder written with encode_sequence_gops")
    if os.path.exists(os.path.join(bin_folder, pmctf_gop.SEQUENCE_HEADER)):
        raise ValueError(f"{path}: the folder also holds {pmctf_gop.SEQUENCE_HEADER}; a sequence has one header")
    versions = (GOP_STRUCTURE_VERSION, GOP_STRUCTURE_VERSION_Q)
    if not isinstance(record, dict) or not is_int(record.get("format_version")) or record["format_version"] not in versions:
        got = record.get("format_version") if isinstance(record, dict) else None
        raise ValueError(f"{path}: format version {got!r}, this decoder reads version {GOP_STRUCTURE_VERSION} and version "
                         f"{GOP_STRUCTURE_VERSION_Q}")
    check_fields(path, record, STRUCTURE_FIELDS)
    _check_structure(path, record)
    return record


# ------------------------------------------------------------------------------------------------------------ the encoder
def _explicit_structure(structure, frame_num, max_gop, psize):
    try:
        pairs = [(size, ds) for size, ds in structure]
    except (TypeError, ValueError):
        raise ValueError(f"structure is one of {STRUCTURES} or a list of (size, me_downsample) (got {structure!r})") from None
    gops, first = [], 0
    for size, ds in pairs:
        if ds not in DS_FACTORS or not is_int(ds):
            raise ValueError(f"structure: me_downsample {ds!r} is not one of {DS_FACTORS}")
        gops.append({"first": first, "size": size, "me_downsample": ds,
                     "psize": psize if ds == 1 else pmctf_gop.ca_psize(ds)})
        first += size if is_int(size) else 0
    _check_gops("structure", gops, frame_num, max_gop)
    return gops


def encode_sequence_gops(codec, source, width, height, frame_num, max_gop, q_index, bin_folder, device, structure="fill",
                         hd_min=HD_MIN, mad_min=MAD_MIN, ds_factors=DS_FACTORS, skip_decoding=True, psize=128,
                         src_format="yuv", ingest="host", decoded_frame_path=None, picture_hash=None, bitdepth=8,
                         msssim=False):
    """pmctf_gop.encode_sequence for a sequence that is a list of GOPs: any frame_num >= 1, GOP k in
    bin_folder/gop_{k:05d}/ (always kept: the function exists to write a decodable folder), gop_structure.json instead of
    sequence.json.  max_gop: the largest GOP, a power of two >= 2.  structure:
      "fill"      plan_gops(frame_num, max_gop);
      "scenecut"  sequence_activity over the source, scene_cuts(mad, hd, hd_min, mad_min), plan_gops with those cuts;
      "search"    every whole window of max_gop pictures (max_gop >= 4) goes through pmctf_ca.search_gop in estimate mode
                  (no files; ds_factors: the motion resolutions it tries) and is then coded as max_gop / gop_choice GOPs of
                  gop_choice pictures with me_downsample = ds_choice and psize = ca_psize(ds_choice); the pictures left
                  over are filled as above.  The search ranks options with the content-adaptive harness's synthesis; what
                  is written, reconstructed and reported is the ordinary one, as for every other structure;
      a list of (size, me_downsample) covering frame_num exactly (me_downsample > 1: padded to ca_psize(me_downsample)).
    GOPs of two or more pictures go through encode_gop, decode_gop and encode_sequence's quality and hash functions; a
    lone picture through codec.encode_lone_picture (0_main.bin and 0_C_main.bin, frame type 0, bpp_mv 0, bits 8 x the
    files' sizes).  The keywords after ds_factors are encode_sequence's, with their meanings and refusals.
    Returns encode_sequence's dictionary (frame_types: 0 for the first picture of every GOP, else 1; the two "average ms"
    lines only when a pair was coded) plus "gops": [{"first", "size", "me_downsample", "psize"}], and "cuts" and "activity"
    (scenecut), "searches": [{"first", "gop_choice", "ds_choice", "tested_opts", "trials"}] (search)."""
    return _encode_gop_list(codec, source, width, height, frame_num, max_gop, q_index, bin_folder, device,
                            structure=structure, hd_min=hd_min, mad_min=mad_min, ds_factors=ds_factors,
                            skip_decoding=skip_decoding, psize=psize, src_format=src_format, ingest=ingest,
                            decoded_frame_path=decoded_frame_path, picture_hash=picture_hash, bitdepth=bitdepth, msssim=msssim)


def _encode_gop_list(codec, source, width, height, frame_num, max_gop, q_index, bin_folder, device, *, choose=None,
                     pipeline=None, what="encode_sequence_gops", structure="fill", hd_min=HD_MIN, mad_min=MAD_MIN,
                     ds_factors=DS_FACTORS, **options):
    """The body of encode_sequence_gops, shared with pmctf_rate.encode_sequence_rate.  choose is None: every GOP is coded
    once, at q_index, into its folder.  Otherwise q_index is None and choose(k, g, trial) decides GOP k's: trial(q, folder)
    codes the GOP (g: its entry of the list) at q into folder (created) and returns {"q_index", "folder", "bits": 8 x the
    sizes of its files, "seconds", ...}; choose returns the trial it accepts, whose files it has moved to
    bin_folder/gop_{k:05d}.  Only the accepted trial is reconstructed, reported and counted in the "average ms" lines; the
    GOP entries then carry "q_index" and the header is format version 2.
    options: encode_sequence's keywords (pmctf_gop.SequenceEncode, which raises their refusals).
    pipeline: a pmctf_chroma.SourcePipeline or None.  With one, every reader converts its pictures on the device after
    upload (read_gop_device, whatever `ingest` says; the scene-cut pass too), everything below sees a 4:2:0 source of the
    coded size, the header included, bin_folder gets the pipeline's records and the result "display_quality"."""
    import time
    import torch
    G = pmctf_gop
    e = G.SequenceEncode(pipeline, keep_gops=True, **options)
    e.check_source_kind()
    skip_decoding, psize = e.skip_decoding, e.psize
    if not is_int(frame_num) or frame_num < 1:
        raise ValueError(f"frame_num is a positive integer (got {frame_num!r})")
    if not _power_of_two(max_gop) or max_gop < 2:
        raise ValueError(f"max_gop is a power of two, at least 2 (got {max_gop!r})")
    if not is_int(psize) or psize <= 0 or psize & 1:
        raise ValueError(f"psize must be even and positive (got {psize!r})")
    plan = None                                                       # [{"first","size","me_downsample","psize"}] known ahead
    if isinstance(structure, str):
        if structure not in STRUCTURES:
            raise ValueError(f"structure is one of {STRUCTURES} or a list of (size, me_downsample) (got {structure!r})")
        if structure == "search":
            if max_gop < 4:
                raise ValueError(f"structure 'search' needs max_gop >= 4 (got {max_gop}): the search tries GOPs down to 4")
            ds_factors = tuple(ds_factors)
            if not ds_factors or any(ds not in DS_FACTORS for ds in ds_factors):
                raise ValueError(f"ds_factors: a non-empty choice of {DS_FACTORS} (got {ds_factors!r})")
    else:
        plan = _explicit_structure(structure, frame_num, max_gop, psize)
    if e.on_device or structure == "scenecut":
        G._need_gpu(device, f"{what}(src_format={e.src_format!r}, ingest={e.ingest!r}, structure={structure!r})")
    make_reader = lambda keep=False: e.open_reader(source, width, height, frame_num, keep)
    t0 = time.time()
    extra = {}
    unit = lambda first, size, ds=1, ps=psize: {"first": first, "size": size, "me_downsample": ds, "psize": ps}
    if structure == "fill":
        plan = [unit(f, s) for f, s in plan_gops(frame_num, max_gop)]
    elif structure == "scenecut":
        with torch.no_grad():
            extra["activity"] = sequence_activity(make_reader, frame_num, device, e.bitdepth)
        extra["cuts"] = scene_cuts(extra["activity"]["mad"], extra["activity"]["hd"], hd_min, mad_min)
        plan = [unit(f, s) for f, s in plan_gops(frame_num, max_gop, extra["cuts"])]
    elif structure == "search":
        extra["searches"] = []
    reader = make_reader(keep=True)
    if pipeline is not None:
        width, height = pipeline.coded
    read = lambda size, ps: e.read_gop(reader, size, device, ps)
    gops = []

    def trial(g, padded, h, w, q, folder):
        """one GOP coded once, at q, into folder: its files and what report needs of it"""
        os.makedirs(folder, exist_ok=True)
        t = {"q_index": q, "folder": folder}
        t0 = time.time()
        if g["size"] == 1:
            t["lone"] = codec.encode_lone_picture(padded[0], folder, w, h, psize=g["psize"], skip_decoding=skip_decoding,
                                                  q_index=q)
            names = ("0_main.bin", "0_C_main.bin")
        else:
            t["enc"] = G.encode_gop(codec, padded, h, w, q, folder, skip_decoding=skip_decoding, psize=g["psize"],
                                    me_downsample=g["me_downsample"])
            names = G.gop_file_names(g["size"])
        if choose is not None:
            t["seconds"] = time.time() - t0
            t["bits"] = 8 * sum(os.path.getsize(os.path.join(folder, n)) for n in names)
        return t

    def code(g, padded, orig, h, w):
        """one GOP of the list: its folder, its files, and of the accepted coding the reconstruction and the tables' rows"""
        k = len(gops)
        if choose is None:
            t = trial(g, padded, h, w, q_index, os.path.join(bin_folder, G.gop_folder(k)))
        else:
            t = choose(k, dict(g), lambda q, folder: trial(g, padded, h, w, q, folder))
        if g["size"] == 1:
            r = t["lone"]
            rec, bits, bits_mv = [[r["L_t"], r["L_tc"], None]], [float(r["bit_L"])], [0.0]
        else:
            enc = t["enc"]
            e.add_pairs(enc)
            rec, bits, bits_mv = G.decode_gop(codec, enc["frames_coded"]), enc["bits"], enc["bits_mv"]
        e.add_gop(rec, orig, h, w, bits, bits_mv, g["first"])
        gops.append(dict(g) if choose is None else dict(g, q_index=t["q_index"]))

    try:
        with torch.no_grad():
            if plan is not None:
                for g in plan:
                    padded, orig, (h, w) = read(g["size"], g["psize"])
                    code(g, padded, orig, h, w)
            else:
                import pmctf_ca
                first = 0
                while frame_num - first >= max_gop:
                    _, orig, (h, w) = read(max_gop, psize)
                    s = pmctf_ca.search_gop(codec, orig, h, w, q_index, None, write_stream=False,
                                            skip_decoding=skip_decoding, ds_factors=ds_factors)
                    size, ds = s["gop_choice"], s["ds_choice"]
                    extra["searches"].append({"first": first, "gop_choice": size, "ds_choice": ds,
                                              "tested_opts": s["tested_opts"],
                                              "trials": [(sz, d, float(rd)) for sz, d, rd in s["trials"]]})
                    ps = G.ca_psize(ds)
                    for at in range(0, max_gop, size):
                        code(unit(first + at, size, ds, ps), pmctf_ca.pad_frames(orig[at:at + size], ps), orig[at:at + size],
                             h, w)
                    first += max_gop
                if first < frame_num:
                    for f, s in plan_gops(frame_num - first, max_gop):
                        padded, orig, (h, w) = read(s, psize)
                        code(unit(first + f, s), padded, orig, h, w)
    finally:
        reader.close()
    write_gop_structure(bin_folder, width=width, height=height, frame_num=frame_num, max_gop=max_gop,
                        q_index=q_index if choose is None else gops[0]["q_index"],
                        ll_order="plane" if skip_decoding else "position", gops=gops, **G.codec_header_fields(codec))
    e.write_sidecars(bin_folder)
    if e.pairs:
        e.average_lines()
    return e.result(frame_num, width, height, t0, gops=gops, **extra)
