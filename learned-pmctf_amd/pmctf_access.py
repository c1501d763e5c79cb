"""Random access: chosen pictures of a coded sequence, decoded from the files they depend on.

GOPs are closed, so a GOP without a wanted picture is never opened.  Inside a GOP of size = 2^S the synthesis is pairwise
(pmctf_gop.decode_gop): stage s turns the pair (i_ref = g * 2^(s+1), i_cur = i_ref + 2^s) of the list back into two entries,
so one picture hangs on the L files and on ONE high-band picture per stage.  "Index j at level s" is entry j of the list
once stage s is undone (a multiple of 2^s); level 0 is the pictures themselves.  Picture files decode independently; only
the motion files chain, pair to pair within a stage and restarting at every stage (pmctf_layers), so the motion of pair g
of a stage needs the motion files of the pairs 0..g of that stage and nothing of another stage.  Of a pair whose `cur`
side nobody needs only the update half of the lifting runs (inverse_MCTF_ref).
  check_frames, gop_plan, access_plan, access_file_names, access_bytes   the plan (pure Python)
  decode_gop_files_frames, decode_frames, read_frames                    the decoder, on pmctf_layers' per-GOP body
The worked example, a GOP of 8 and picture 5:
  needed = {0: [5], 1: [4], 2: [4], 3: [0]}        pairs = [(2, 0, 4, True), (1, 4, 6, False), (0, 4, 5, True)]
  files  = 1_mv 3_mv 5 5_C_main 5_mv | 2_mv 6 6_C_main 6_mv | 4 4_C_main 4_mv | 0_main 0_C_main: 14 of the GOP's 23 files,
  8 of its 16 picture files.
The plan needs no GPU and this module imports no torch itself; the decoders have no CPU path."""
import os

import pmctf_gop
import pmctf_layers
import pmctf_spatial
from pmctf_records import is_int


# --------------------------------------------------------------------------------------------------------------- the plan
def check_frames(frames, frame_num):
    """the selection as an ascending list of distinct picture indices.  frames: a range, any iterable of integers, or a
    tuple (start, stop) that stands for range(start, stop).  ValueError naming the offending value for an empty selection,
    a value that is no integer, an index outside 0..frame_num-1 and a duplicate."""
    given = frames
    if isinstance(frames, tuple) and len(frames) == 2:
        for v in frames:
            if not is_int(v):
                raise ValueError(f"frames: {v!r} is not an integer")
        frames = range(*frames)
    try:
        frames = list(frames)
    except TypeError:
        raise ValueError(f"frames: {given!r} is not a range, a (start, stop) pair or a list of integers") from None
    if not frames:
        raise ValueError(f"frames: {given!r} selects no picture")
    seen = set()
    for v in frames:
        if not is_int(v):
            raise ValueError(f"frames: {v!r} is not an integer")
        if not 0 <= v < frame_num:
            raise ValueError(f"frames: {v!r} is outside 0..{frame_num - 1}, the sequence's pictures")
        if v in seen:
            raise ValueError(f"frames: {v!r} is given twice")
        seen.add(v)
    return sorted(frames)


def gop_plan(size, wanted):
    """what a decode of the pictures `wanted` (ascending local indices) of one GOP of `size` = 2^S pictures needs:
    "needed": {s: the indices at level s that must exist}, s = 0..S: needed[0] = wanted, needed[s + 1] the i_ref of the
              pairs of stage s that needed[s] touches, needed[S] = [0]
    "pairs": [(stage, i_ref, i_cur, want_cur)] in synthesis order (stages S-1 .. 0, descending group index): the pairs one
              of whose sides is in needed[stage]; want_cur: i_cur is; where it is not, only `ref` has to be computed
    "picture_files": {i_cur}.bin and {i_cur}_C_main.bin of every listed pair, then 0_main.bin and 0_C_main.bin
    "motion_files": per stage with a listed pair, {i_cur}_mv.bin of the pairs 0..g_max, g_max its largest listed group
              index, in coding order: the context runs pair to pair from the stage's first
    "files": both, in pmctf_gop.gop_file_names order.
    size == 1: the two L files, no pairs, no motion."""
    stages = pmctf_layers.gop_stages(size)
    wanted = list(wanted)
    if not wanted or any(not is_int(j) or not 0 <= j < size for j in wanted) or \
            any(a >= b for a, b in zip(wanted, wanted[1:])):
        raise ValueError(f"wanted: ascending indices from 0 to {size - 1}, at least one (got {wanted!r})")
    needed = {0: wanted}
    for s in range(stages):
        needed[s + 1] = sorted({(j >> (s + 1)) << (s + 1) for j in needed[s]})
    pairs, motion = [], []
    for s in reversed(range(stages)):
        at = set(needed[s])
        listed = [g for g in reversed(range(size >> (s + 1))) if (g << (s + 1)) in at or (g << (s + 1)) + (1 << s) in at]
        pairs += [(s, g << (s + 1), (g << (s + 1)) + (1 << s), (g << (s + 1)) + (1 << s) in at) for g in listed]
        motion = [f"{(g << (s + 1)) + (1 << s)}_mv.bin" for g in range(listed[0] + 1)] + motion
    pictures = [n for _, _, i_cur, _ in pairs for n in (f"{i_cur}.bin", f"{i_cur}_C_main.bin")] + list(pmctf_layers.L_FILES)
    read = set(pictures) | set(motion)
    names = pmctf_gop.gop_file_names(size) if size != 1 else list(pmctf_layers.L_FILES)
    return {"needed": needed, "pairs": pairs, "picture_files": pictures, "motion_files": motion,
            "files": [n for n in names if n in read]}


def access_plan(gops, frames):
    """[(gop index, [local indices])] of the GOPs that hold a wanted picture, in order.  gops: pmctf_gop.sequence_layout's
    list [(first, size, ...)]; frames: ascending source indices (check_frames)."""
    out = []
    for k, g in enumerate(gops):
        local = [t - g[0] for t in frames if g[0] <= t < g[0] + g[1]]
        if local:
            out.append((k, local))
    return out


def access_file_names(size, wanted):
    """the files a decode of the pictures `wanted` of one GOP of `size` pictures reads, in gop_file_names order"""
    return gop_plan(size, wanted)["files"]


def access_bytes(bin_folder, frames):
    """the sizes of exactly the files a decode of `frames` from the sequence in bin_folder reads, summed over the GOPs that
    hold one of them: pmctf_layers.layer_bytes' counterpart.  ValueError naming a file that is missing."""
    header, gops = pmctf_gop.sequence_layout(bin_folder)
    return pmctf_layers.files_bytes(bin_folder, ((k, access_file_names(gops[k][1], local))
                                                 for k, local in access_plan(gops, check_frames(frames, header["frame_num"]))))


# ---------------------------------------------------------------------------------------------------------------- one GOP
def decode_gop_files_frames(codec, bin_folder, gop, pic_height, pic_width, q_index, wanted, psize=128, me_downsample=1,
                            ll_order="plane", spatial_level=0, one_sided=True):
    """The pictures `wanted` (ascending local indices) of one GOP from gop_plan(gop, wanted)["files"] alone: anything else
    in the folder may be absent, cut short or garbage; a missing, truncated or surplus-length file of that set raises the
    ValueError of pmctf_gop.decode_gop_files, which names it.  The picture files go through one batch; under it the
    listed motion files decode stage by stage in coding order with the context reset per stage (a reduced-resolution
    stream at the size it was coded at); at spatial_level k the motion is reduced (pmctf_layers.reduce_motion); then the
    plan's pairs are synthesised in its order, luma and chroma as decode_gop does.  Where a pair's want_cur is False only
    inverse_MCTF_ref runs: the same `ref`, bit for bit, without the predict half.  one_sided=False runs inverse_MCTF
    everywhere, for comparison.
    Returns {"frames": [[Y, UV, None]] (padded) in the order of `wanted`, "times": wanted, "files": the names read, in
    order, "bytes_read", "stages", "pairs": the plan's, "half_pairs": how many ran `ref` alone, "spatial_level", "size":
    (height, width) of the pictures, "symbols_decoded" and "payload_bytes_used" as decode_gop_files_layer reports them}."""
    def plan():
        found = gop_plan(gop, wanted)
        return (found["pairs"], {i_cur for _, _, i_cur, _ in found["pairs"]},
                {int(n.split("_")[0]) for n in found["motion_files"]}, [], list(found["needed"][0]))

    out, pairs = pmctf_layers._decode_gop_planned(codec, bin_folder, gop, pic_height, pic_width, q_index, psize, me_downsample,
                                                  ll_order, spatial_level, plan, one_sided=one_sided)
    del out["frames_coded"]
    return dict(out, pairs=pairs, half_pairs=sum(not want_cur for _, _, _, want_cur in pairs) if one_sided else 0)


# ------------------------------------------------------------------------------------------------------------ a sequence
class FrameDecode(pmctf_gop.FullDecode):
    """pmctf_gop.decode_sequence_with for chosen pictures: a GOP that holds one goes through decode_gop_files_frames, any
    other gives nothing and is not touched (its folder need not exist).  The pictures are checked against exactly their
    own records: those of picture_hashes.json, or at spatial level k the records of spatial_hashes.json (k, temporal level
    0) whose "index" is wanted.  The refusals of a spatial level are pmctf_layers.LayerDecode's; a folder written by
    extract_layer with min_level > 0 is refused.  keep=True: the packed pictures stay on the device in .kept,
    [(source index, picture)] (read_frames), and nothing need be written.  The result gains "times", "bytes_read",
    "gops_opened", "half_pairs", "spatial_level" and "size"."""

    def __init__(self, frames, spatial_level=0, one_sided=True, keep=False):
        pmctf_layers._check_decode_args(0, False, spatial_level=spatial_level)
        self.frames_given, self.spatial_level, self.one_sided, self.keeps = frames, spatial_level, one_sided, keep
        self.verify, self.size, self.kept, self.opened, self.half_pairs = "auto", None, [], 0, 0

    def refuse(self, verify):
        self.verify = verify

    def check_folder(self, bin_folder):
        marker = pmctf_layers.read_layer_extract(bin_folder)
        if marker is not None and marker["min_level"] > 0:
            raise ValueError(f"{os.path.join(bin_folder, pmctf_layers.LAYER_EXTRACT)}: the folder holds the files of temporal "
                             f"level {marker['min_level']} and above, single pictures cannot be decoded from it")
        header, gops = pmctf_gop.sequence_layout(bin_folder)
        plan = access_plan(gops, check_frames(self.frames_given, header["frame_num"]))
        self.by_folder = {os.path.join(bin_folder, pmctf_gop.gop_folder(k)): local for k, local in plan}
        self.by_first = {gops[k][0]: local for k, local in plan}

    def picture_size(self, bin_folder, h, w, coded_size_output, coded_format_output):
        self.size = pmctf_layers.spatial_picture_size(bin_folder, h, w, self.spatial_level, self.verify, coded_size_output,
                                                      coded_format_output)
        return self.size

    def open(self, bin_folder, header, gops, verify):
        if verify is False:
            return
        if not self.spatial_level:
            super().open(bin_folder, header, gops, verify)
            self.records = dict(enumerate(self.frames)) if self.hash_level is not None else {}
        elif verify != "auto" or os.path.exists(os.path.join(bin_folder, pmctf_spatial.SPATIAL_HASHES)):
            rec = pmctf_spatial.read_spatial_hashes(bin_folder)
            self.records = {r["index"]: r for r in rec["layers"][str(self.spatial_level)]["0"]}
            self.hash_level = rec["level"]

    def decode_gop(self, codec, folder, size, h, w, q_index, psize, me_downsample, ll_order):
        local = self.by_folder.get(folder)
        if local is None:
            return [], [], 0
        out = decode_gop_files_frames(codec, folder, size, h, w, q_index, local, psize, me_downsample, ll_order,
                                      self.spatial_level, self.one_sided)
        self.opened += 1
        self.half_pairs += out["half_pairs"]
        return out["frames"], out["times"], out["bytes_read"]

    def recorded(self, first, size, at, n):
        return [self.records[first + t] for t in self.by_first[first]]

    def taken(self, source, frames, bitdepth):
        if self.keeps:
            self.kept += zip(source, pmctf_gop.PlainSink(*self.size, bitdepth).frames(frames))

    def result(self, times, nbytes):
        return {"times": times, "bytes_read": nbytes, "gops_opened": self.opened, "half_pairs": self.half_pairs,
                "spatial_level": self.spatial_level, "size": self.size}


def decode_frames(codec, bin_folder, yuv_out, frames, device=None, png_out=None, verify="auto", *, spatial_level=0,
                  coded_size_output=False, coded_format_output=False, output_layout=None):
    """The pictures `frames` (check_frames: a range, integers or a (start, stop) pair) of the sequence in bin_folder,
    ascending, through the sinks of every other decode: the display size, the source's chroma format, a yuv_out ending in
    .y4m, an output_layout; the PNGs are named by source index.  Only the GOPs that hold one of them are opened, and of
    those only access_file_names.  The pictures are verified against their own records under the four verify modes of
    decode_sequence_checked (PictureHashMismatch before anything of the GOP is written).  spatial_level=k: at 1/2^k of the
    size, as pmctf_spatial.decode_sequence_layer gives and refuses it.  A temporal level is not combined with a selection.
    frames=range(frame_num) writes the bytes decode_sequence_checked writes.
    Returns decode_sequence's dict ("seconds": per GOP of the folder, next to nothing for one that was not opened) plus
    "times": the source indices written, "bytes_read": access_bytes, "gops_opened", "half_pairs": the pairs of which only
    `ref` was computed, "spatial_level" and "size": (height, width) of the decoded pictures."""
    return pmctf_gop.decode_sequence_with(FrameDecode(frames, spatial_level), codec, bin_folder, yuv_out, device, png_out,
                                          verify, coded_size_output=coded_size_output,
                                          coded_format_output=coded_format_output, output_layout=output_layout)


def read_frames(codec, bin_folder, frames, device=None, verify="auto"):
    """-> [(source index, packed picture)] of the pictures `frames`, ascending, for a caller that goes on in PyTorch: every
    picture a planar integer tensor on the device, of the coded size and depth, as pmctf_gop.PlainSink.frames packs it
    (pmctf_scale.unpack_frame splits it).  Verified as decode_frames verifies; nothing is written and nothing but the
    hashes goes to the host."""
    mode = FrameDecode(frames, keep=True)
    pmctf_gop.decode_sequence_with(mode, codec, bin_folder, None, device, None, verify, coded_size_output=True,
                                   coded_format_output=True)
    return mode.kept
