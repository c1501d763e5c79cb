"""GOP driver: the temporal-decomposition loop of the reference's evaluation harness
(test_pMCTF_flex.py:run_test, lines 131-327) restated as a reusable function over any codec object
exposing the reference model API (`num_me_stages`, `encode_one_stage`, `inverse_MCTF`).

Used by bench.py (HIP product), the parity tests (oracle vs product) and tools/make_golden.py (the
real reference, in the build container) so that all three run exactly the same schedule:
stage s codes pairs (2k*2^s, 2k*2^s + 2^s); dpb is reset per stage; the last stage also codes L;
then the inverse MCTF runs the stages backwards and PSNR is taken on the un-padded crop.
"""
import math
import os

import torch

from pmctf_records import is_int, read_record, write_record


def psnr(a, b):
    """test_pMCTF_flex.py:81-84"""
    mse = torch.mean((a - b) ** 2)
    return (20 * torch.log10(255.0 / torch.sqrt(mse))).item()


def ca_psize(me_downsample):
    """padding granularity the content-adaptive harness uses for a motion down-sampling factor (test_pMCTF_CA.py:121-123)"""
    psize = 256 if me_downsample > 2 else 128
    return psize * 2 if me_downsample > 4 else psize


def encode_gop_batched(codec, frames, pic_height, pic_width, q_index, bin_folder, psize=128):
    """The schedule of encode_gop with the pairs of each temporal stage handed to the codec in ONE call
    (codec.encode_stage_pairs): identical files, bits and tensors, larger launches.  skip_decoding=True only."""
    gop = len(frames)
    stages = int(round(math.log2(gop)))
    assert 2 ** stages == gop and gop >= 2
    frames_coded = [None] * gop
    bits = [None] * gop
    bits_mv = [None] * gop
    results = []
    num_frames = gop
    for stage_idx in range(stages):
        num_frames //= 2
        step = 2 ** stage_idx
        code_lt = (stage_idx + 1) == stages
        me_num = min(codec.num_me_stages - 1, stage_idx)
        idx = [(g * 2 * step, g * 2 * step + step) for g in range(num_frames)]
        if stage_idx == 0:
            pairs = [(frames[a], frames[b]) for a, b in idx]
        else:
            pairs = [(frames_coded[a][:2], frames_coded[b][:2]) for a, b in idx]
        paths = [os.path.join(bin_folder, f"{b}.bin") for _, b in idx]
        rs, _ = codec.encode_stage_pairs(pairs, code_lt, {"mv_feature": None, "ref_mv_y": None}, paths,
                                         pic_width=pic_width, pic_height=pic_height, psize=psize, stage_idx=me_num,
                                         q_index=q_index)
        for (i_ref, i_cur), r in zip(idx, rs):
            frames_coded[i_ref] = [r["L_t"], r["L_tc"], None]
            frames_coded[i_cur] = [r["H_t"], r["H_tc"], r["mv_hat"]]
            bits[i_cur] = float(r["bit_H"] + r["bit_ME"])
            bits_mv[i_cur] = float(r["bit_ME"])
            if code_lt:
                bits[i_ref] = float(r["bit_L"])
                bits_mv[i_ref] = 0.0
            results.append(r)
    return {"bits": bits, "bits_mv": bits_mv, "frames_coded": frames_coded, "results": results, "stages": stages}


def encode_gops_batched(codec, gops, pic_height, pic_width, q_index, bin_folders, psize=128):
    """K closed GOPs at once: stage s of ALL of them goes to the codec in one encode_stage_pairs call (the GOPs are
    independent units, test_pMCTF_flex.py:131-141, and use the same coder weights), so the late stages — 2 and 1 pairs
    per GOP — are batched K-fold as well.  The motion context restarts at every GOP boundary (chain_reset); each GOP's
    files go to its own folder.  Returns one encode_gop-style dict per GOP; files, bits and tensors are identical to
    coding the GOPs one after the other."""
    K = len(gops)
    gop = len(gops[0])
    stages = int(round(math.log2(gop)))
    assert 2 ** stages == gop and gop >= 2 and all(len(g) == gop for g in gops) and len(bin_folders) == K
    outs = [{"bits": [None] * gop, "bits_mv": [None] * gop, "frames_coded": [None] * gop, "results": [],
             "stages": stages} for _ in range(K)]
    num_frames = gop
    for stage_idx in range(stages):
        num_frames //= 2
        step = 2 ** stage_idx
        code_lt = (stage_idx + 1) == stages
        me_num = min(codec.num_me_stages - 1, stage_idx)
        idx = [(g * 2 * step, g * 2 * step + step) for g in range(num_frames)]
        pairs, paths = [], []
        for k in range(K):
            src = gops[k] if stage_idx == 0 else [f[:2] for f in outs[k]["frames_coded"]]
            pairs += [(src[a], src[b]) for a, b in idx]
            paths += [os.path.join(bin_folders[k], f"{b}.bin") for _, b in idx]
        rs, _ = codec.encode_stage_pairs(pairs, code_lt, {"mv_feature": None, "ref_mv_y": None}, paths,
                                         pic_width=pic_width, pic_height=pic_height, psize=psize, stage_idx=me_num,
                                         q_index=q_index, chain_reset=[k * num_frames for k in range(1, K)])
        for k in range(K):
            o = outs[k]
            for (i_ref, i_cur), r in zip(idx, rs[k * num_frames:(k + 1) * num_frames]):
                o["frames_coded"][i_ref] = [r["L_t"], r["L_tc"], None]
                o["frames_coded"][i_cur] = [r["H_t"], r["H_tc"], r["mv_hat"]]
                o["bits"][i_cur] = float(r["bit_H"] + r["bit_ME"])
                o["bits_mv"][i_cur] = float(r["bit_ME"])
                if code_lt:
                    o["bits"][i_ref] = float(r["bit_L"])
                    o["bits_mv"][i_ref] = 0.0
                o["results"].append(r)
    return outs


def encode_gop(codec, frames, pic_height, pic_width, q_index, bin_folder, skip_decoding=True, psize=128,
               on_pair=None, me_downsample=1, store_only=False):
    """frames: list (len = GOP size, power of two) of [Y (1,1,Hp,Wp), UV (2,1,Hp/2,Wp/2)] padded tensors.
    Returns dict(bits[], frames_coded (after forward), results[] per pair in coding order).
    me_downsample > 1: the schedule of test_pMCTF_CA.py:code_one_gop (motion at reduced resolution; pad the frames to
    ca_psize(me_downsample) and pass that as psize).
    store_only=True: a caller that keeps the results of every pair WITHOUT the harness's two prints (not what
    test_pMCTF_flex.py does): with the codec's opt-in deferral (lazy_stages) the pairs of a stage are then coded as one
    batch."""
    gop = len(frames)
    stages = int(round(math.log2(gop)))
    assert 2 ** stages == gop and gop >= 2
    frames_coded = [None] * gop
    bits = [None] * gop
    bits_mv = [None] * gop
    results = []
    log = []
    num_frames = gop
    for stage_idx in range(stages):
        num_frames //= 2
        dpb = {"mv_feature": None, "ref_mv_y": None}
        for group_idx in range(num_frames):
            step = 2 ** stage_idx
            i_ref = group_idx * 2 * step
            i_cur = i_ref + step
            if stage_idx == 0:
                y_ref, c_ref = frames[i_ref]
                y_cur, c_cur = frames[i_cur]
            else:
                y_ref, c_ref, mv_r = frames_coded[i_ref]
                y_cur, c_cur, mv_c = frames_coded[i_cur]
                assert mv_r is None and mv_c is None
            code_lt = (stage_idx + 1) == stages
            me_num = min(codec.num_me_stages - 1, stage_idx)
            # bin_folder None: the estimate-only branch of encode_one_stage (test_pMCTF_CA.py:153-154)
            bin_path = os.path.join(bin_folder, f"{i_cur}.bin") if bin_folder is not None else None
            r = codec.encode_one_stage(ref_frame=[y_ref, c_ref], cur_frame=[y_cur, c_cur], output_path=bin_path,
                                       pic_height=pic_height, pic_width=pic_width, stage_idx=me_num,
                                       code_lt=code_lt, psize=psize, skip_decoding=skip_decoding, dpb=dpb,
                                       q_index=q_index, **({"me_downsample": me_downsample} if me_downsample != 1 else {}))
            frames_coded[i_ref] = [r["L_t"], r["L_tc"], None]
            frames_coded[i_cur] = [r["H_t"], r["H_tc"], r["mv_hat"]]
            dpb = r["dpb"]
            # what the harness does with the numbers of every pair, statement for statement (test_pMCTF_flex.py:236-258):
            # the two f-strings it prints LOOK at the bit counts right here, before the next call
            curr_bits = r["bit_H"] + r["bit_ME"]
            if isinstance(curr_bits, torch.Tensor):
                curr_bits = curr_bits.item()
            tmp = r["bit_ME"] / curr_bits
            if not store_only:
                log.append(f"percentage MV: {tmp*100} %")
            bits[i_cur] = curr_bits
            bit_me = r["bit_ME"].item() if isinstance(r["bit_ME"], torch.Tensor) else r["bit_ME"]
            bits_mv[i_cur] = bit_me
            if not store_only:
                log.append(f"Frame {i_cur}: {curr_bits / (pic_height * pic_width)} bpp")
            if code_lt:
                curr_bits = r["bit_L"]
                if isinstance(curr_bits, torch.Tensor):
                    curr_bits = curr_bits.item()
                bits[i_ref] = curr_bits
                bits_mv[i_ref] = 0.0
            results.append(r)
            if on_pair is not None:
                on_pair(stage_idx, i_ref, i_cur, r)
    bits = [None if b is None else float(b) for b in bits]
    bits_mv = [None if b is None else float(b) for b in bits_mv]
    frames_coded = [[t if t is None or isinstance(t, torch.Tensor) else t.force() for t in fc] for fc in frames_coded]
    return {"bits": bits, "bits_mv": bits_mv, "frames_coded": frames_coded, "results": results, "stages": stages,
            "log": log}


def decode_gop(codec, frames_coded, luma_stage0=False):
    """Temporal synthesis, test_pMCTF_flex.py:268-291.  Modifies and returns frames_coded.
    luma_stage0: the content-adaptive harness's variant, which reconstructs luma with stage 0's lifting filters at every
    stage (inverse_MCTF without stage_idx, test_pMCTF_CA.py:239)."""
    return synthesise(codec, frames_coded, synthesis_pairs(len(frames_coded)), luma_stage0=luma_stage0)


def synthesis_pairs(gop, down_to=0):
    """[(stage, i_ref, i_cur, True)] in synthesis order: every pair of the stages S-1 .. down_to of a GOP of 2^S pictures,
    each stage from its last group to its first.  The True is want_cur (synthesise): both sides of every pair."""
    stages = int(round(math.log2(gop)))
    return [(s, g << (s + 1), (g << (s + 1)) + (1 << s), True)
            for s in reversed(range(down_to, stages)) for g in reversed(range(gop >> (s + 1)))]


def synthesise(codec, frames_coded, pairs, luma_stage0=False, one_sided=False, snapshots=None):
    """The one temporal synthesis loop (test_pMCTF_flex.py:268-291): the pairs (stage, i_ref, i_cur, want_cur) in the order
    given, luma and then chroma (downscale=True) of each through codec.inverse_MCTF, [ref, ref_c, None] and [cur, cur_c,
    None] written back.  Modifies and returns frames_coded.
    one_sided: of a pair whose want_cur is False only `ref` is computed (codec.inverse_MCTF_ref: the same tensor without the
    predict half) and the `cur` entry stays as it is.  synthesis_pairs never asks for that, so a codec without that method
    (the oracle model, the reference network) serves decode_gop.
    snapshots: a dict that receives, per level k, the low-band entries ([Y, UV, None] at the indices j * 2^k) as the list
    holds them once stage k is undone, and under S the state before the first pair; for pairs of synthesis_pairs."""
    def keep(k):
        if snapshots is not None:
            snapshots[k] = [list(frames_coded[j << k]) for j in range(len(frames_coded) >> k)]

    keep(int(round(math.log2(len(frames_coded)))))
    for n, (stage, i_ref, i_cur, want_cur) in enumerate(pairs):
        L_t, L_tc, mv_ref = frames_coded[i_ref]
        H_t, H_tc, mv_hat = frames_coded[i_cur]
        assert mv_ref is None
        me_num = min(codec.num_me_stages - 1, stage)
        me_luma = 0 if luma_stage0 else me_num
        if want_cur or not one_sided:
            ref, cur = codec.inverse_MCTF(L_t, H_t, mv_hat, stage_idx=me_luma)
            ref_c, cur_c = codec.inverse_MCTF(L_tc, H_tc, mv_hat, stage_idx=me_num, downscale=True)
            frames_coded[i_cur] = [cur, cur_c, None]
        else:
            ref = codec.inverse_MCTF_ref(L_t, H_t, mv_hat, stage_idx=me_luma)
            ref_c = codec.inverse_MCTF_ref(L_tc, H_tc, mv_hat, stage_idx=me_num, downscale=True)
        frames_coded[i_ref] = [ref, ref_c, None]
        if n + 1 == len(pairs) or pairs[n + 1][0] != stage:
            keep(stage)
    return frames_coded


def gop_psnr(frames_rec, frames_orig, pic_height, pic_width):
    """YUV-PSNR (6Y+Cb+Cr)/8 per frame on the un-padded crop, test_pMCTF_flex.py:294-325."""
    out = []
    for (rec_y, rec_c, _), (y, c) in zip(frames_rec, frames_orig):
        ry = torch.round(rec_y.clamp(0, 255.0))[:, :, :pic_height, :pic_width]
        rc = torch.round(rec_c.clamp(0, 255.0))[:, :, :pic_height // 2, :pic_width // 2]
        oy = y[:, :, :pic_height, :pic_width]
        oc = c[:, :, :pic_height // 2, :pic_width // 2]
        py = psnr(ry, oy)
        pcb = psnr(rc[0:1], oc[0:1])
        pcr = psnr(rc[1:2], oc[1:2])
        out.append({"y": py, "cb": pcb, "cr": pcr, "yuv": (6.0 * py + pcb + pcr) / 8.0})
    return out


def gop_quality(frames_rec, frames_orig, pic_height, pic_width, msssim=True):
    """gop_psnr + rgb_psnr + MS-SSIM of the rounded RGB pictures (test_pMCTF_flex.py:293-327) per frame, from the HIP
    quality kernels (pMCTF.hip.ops.frame_quality): a handful of launches and ONE device->host copy per frame, exact
    integer error sums, float64 PSNR.  frames_rec: [[Y, UV, ...]] as decode_gop returns them (padded, not clamped);
    frames_orig: the un-padded originals of read_gop.  -> [{"y","cb","cr","yuv","rgb","msssim","sse"}].
    msssim is 0.0 when not asked for or for pictures with a side of 128 or less (the harness's guard), and a ValueError
    for a smaller side of 129..160.  Like the rest of the product path there is no CPU fallback."""
    from pMCTF.hip import ops
    out = []
    for rec, (y, c) in zip(frames_rec, frames_orig):
        tensors = (rec[0], rec[1], y, c)
        if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors):
            raise RuntimeError("gop_quality runs on the GPU (no CPU fallback): pass device tensors, or use gop_psnr / "
                               "rgb_psnr for tensors on the host")
        rec_y, rec_c, y, c = (t.float().contiguous() for t in tensors)
        out.append(ops.frame_quality(rec_y, rec_c, y, c, pic_height, pic_width, msssim=msssim))
    return out


def gop_quality_hbd(frames_rec, frames_orig, pic_height, pic_width, bitdepth):
    """gop_quality for a source of `bitdepth` 9..16 bits: reconstruction and originals are taken back to integers of that
    depth (pMCTF.hip.ops.frame_sse_hbd: planes_to_u16's rounding, 64-bit integer error sums on the device) and the PSNR is
    against 2^bitdepth - 1.  -> [{"y","cb","cr","yuv","rgb","msssim","sse": (Y, Cb, Cr)}] with "rgb" and "msssim" 0.0: the
    harness defines RGB-PSNR and MS-SSIM on 8-bit RGB pictures.  gop_quality keeps its five parameters; this is its
    high-bit-depth form.  No CPU fallback."""
    from pMCTF.hip import ops
    bitdepth = check_bitdepth(bitdepth, above8=True)
    out = []
    for rec, (y, c) in zip(frames_rec, frames_orig):
        tensors = (rec[0], rec[1], y, c)
        if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors):
            raise RuntimeError("gop_quality_hbd runs on the GPU (no CPU fallback): pass device tensors")
        rec_y, rec_c, y, c = (t.float().contiguous() for t in tensors)
        q = ops.frame_sse_hbd(rec_y, rec_c, y, c, pic_height, pic_width, bitdepth)
        q.update(rgb=0.0, msssim=0.0)
        out.append(q)
    return out


def check_bitdepth(bitdepth, above8=False):
    """the source bit depth as an int: 8, or 9..16 (16-bit samples); ValueError otherwise, and for 8 with above8"""
    if isinstance(bitdepth, bool) or not isinstance(bitdepth, int) or not (8, 9)[above8] <= bitdepth <= 16:
        raise ValueError(f"bitdepth is {'' if above8 else '8 or '}9..16 (got {bitdepth!r})")
    return bitdepth


def write_yuv(path, frames_u8):
    """[(Y, Cb, Cr) uint8 arrays] -> planar 8-bit 4:2:0 file, the layout YUVReader / image_import read; uint16 arrays
    give the 16-bit layout of YUVReader(bitdepth=9..16) (the samples are written in the host's byte order: little-endian)"""
    with open(path, "wb") as f:
        for planes in frames_u8:
            for p in planes:
                f.write(p.tobytes(order="C"))


def read_gop(reader, gop, device, psize=128):
    """GOP pictures from a YUVReader as the model's inputs: ([Y (1,1,Hp,Wp), UV (2,1,Hp/2,Wp/2)] zero padded right/bottom
    to multiples of psize (chroma psize/2), the un-padded originals, (height, width)).  What the harness does per pair
    at stage 0 (test_pMCTF_flex.py:151-192), done here per GOP.  A reader of 16-bit samples (YUVReader(bitdepth=b)) has them
    scaled by 2^-(b - 8)."""
    import torch.nn.functional as F
    from pMCTF.utils.stream_helper import get_padding_size
    padded, orig, size = [], [], None
    shift = getattr(reader, "bitdepth", 8) - 8
    for _ in range(gop):
        if shift:                                   # b-bit samples enter as v * 2^-(b - 8): exact, the range stays 0..255
            import numpy as np
            y, cb, cr = (torch.from_numpy(p.astype(np.float32)) * 2.0 ** -shift for p in reader.read_one_frame())
        else:
            y, cb, cr = (torch.from_numpy(p).float() for p in reader.read_one_frame())
        assert size in (None, tuple(y.shape)), "picture size changes inside the sequence"
        size = tuple(y.shape)
        luma = y[None, None].to(device)
        chroma = torch.stack((cb, cr))[:, None].to(device)
        left, right, top, bottom = get_padding_size(size[0], size[1], p=psize)
        orig.append([luma, chroma])
        padded.append([F.pad(luma, (left, right, top, bottom)),
                       F.pad(chroma, (left // 2, right // 2, top // 2, bottom // 2))])
    return padded, orig, size


class PNGReader:
    """A sequence of PNG pictures with the YUVReader interface used here (read_one_frame, close, width, height), for
    sources that are not .yuv files.  paths_or_folder: a list of paths, taken in the given order, or a folder, meaning its
    *.png in natural numeric order (2.png before 10.png), then by name.  Pictures are opened as
    Image.open(p).convert("RGB") (read_image_to_torch, test_pMCTF_flex.py:62-67) and returned as (h, w, 3) uint8 RGB
    arrays: the conversion to 4:2:0 happens on the device (read_gop_device, pngs_to_yuv).  Every picture must have the size
    of the first (AssertionError, as in read_gop), and that size must be even (ValueError)."""

    def __init__(self, paths_or_folder):
        import re
        if isinstance(paths_or_folder, (str, os.PathLike)):
            folder = os.fspath(paths_or_folder)
            if not os.path.isdir(folder):
                raise AssertionError(f"no such folder of pictures: {folder}")
            names = [n for n in os.listdir(folder) if n.lower().endswith(".png")]
            # runs of digits compare as numbers (and before text at the same place), the rest as lower-case text
            names.sort(key=lambda n: ([(0, int(t), "") if t.isdigit() else (1, 0, t.lower())
                                       for t in re.split(r"(\d+)", n) if t], n))
            self.paths = [os.path.join(folder, n) for n in names]
        else:
            self.paths = [os.fspath(p) for p in paths_or_folder]
        if not self.paths:
            raise AssertionError(f"no PNG pictures in {paths_or_folder}")
        self.current_frame_index = 0
        self.eof = False
        first = self._open(self.paths[0])
        self.height, self.width = int(first.shape[0]), int(first.shape[1])
        if (self.width | self.height) & 1:
            raise ValueError(f"{self.paths[0]}: 4:2:0 coding needs an even picture size, got {self.width}x{self.height}")

    @staticmethod
    def _open(path):
        import numpy as np
        from PIL import Image
        with Image.open(path) as im:
            return np.array(im.convert("RGB"), dtype=np.uint8)          # a copy the caller owns: (h, w, 3), C order

    def __len__(self):
        return len(self.paths)

    def read_one_frame(self):
        """-> (h, w, 3) uint8 RGB array of the next picture, None past the end"""
        if self.current_frame_index >= len(self.paths):
            self.eof = True
            return None
        path = self.paths[self.current_frame_index]
        rgb = self._open(path)
        assert rgb.shape == (self.height, self.width, 3), f"picture size changes inside the sequence ({path})"
        self.current_frame_index += 1
        return rgb

    def close(self):
        self.current_frame_index = 0
        self.eof = False


def _need_gpu(device, what):
    if torch.device(device).type != "cuda":
        raise RuntimeError(f"{what} runs on the GPU (no CPU fallback)")


def read_gop_device(reader, gop, device, psize=128):
    """read_gop with the arithmetic on the device: the same triple, tensor for tensor and bit for bit.  From a YUVReader a
    picture costs one copy of its bytes to the device and one launch (pmctf_yuv420_u8_to_planes_f32: conversion, padding
    and the un-padded originals); from a PNGReader the RGB bytes are copied and converted to 4:2:0 first
    (pmctf_rgb8_to_yuv420_u8).  A YUVReader of 16-bit samples goes through pmctf_yuv420_u16_to_planes_f32 the same way.
    A reader with a `resample` attribute (pmctf_chroma.SourcePipeline.ingest: a source in another chroma format, or coded at
    another size than its own) has every packed picture converted on the device before the planes are made; the triple is
    then that of a 4:2:0 source of resample.shape.  A reader with an `unpack` attribute (pmctf_layout.PackedReader and
    SurfaceReader: pictures in a pixel layout) gives a picture's raw bytes, as an array or as a tensor that already lies
    on the device; they are unpacked there into the packed planar picture by one launch, before anything else."""
    import numpy as np
    from pMCTF.hip import ops
    _need_gpu(device, "read_gop_device")
    padded, orig, size = [], [], None
    bitdepth = getattr(reader, "bitdepth", 8)
    resample = getattr(reader, "resample", None)
    unpack = getattr(reader, "unpack", None)
    for _ in range(gop):
        pic = reader.read_one_frame()
        assert pic is not None, "sequence ends inside a GOP"
        if unpack is not None:                                          # the bytes of a picture in a pixel layout
            shape = unpack.shape
            frame = unpack((pic if isinstance(pic, torch.Tensor) else torch.from_numpy(pic)).to(device))
        elif isinstance(pic, np.ndarray):                               # RGB picture of a PNGReader
            shape = tuple(pic.shape[:2])
            frame = ops.rgb8_to_yuv420(torch.from_numpy(pic).to(device))
        else:
            shape = tuple(pic[0].shape)
            frame = torch.from_numpy(np.concatenate([p.reshape(-1) for p in pic])).to(device)
        assert size in (None, shape), "picture size changes inside the sequence"
        size = shape
        h, w = shape
        if resample is not None:
            frame, (h, w) = resample(frame), resample.shape
        y_pad, c_pad, y_org, c_org = ops.planes_from(frame, h, w, bitdepth, psize=psize)
        orig.append([y_org, c_org])
        padded.append([y_pad, c_pad])
    return padded, orig, size if resample is None else resample.shape


def pngs_to_yuv(paths_or_folder, yuv_out, device):
    """A PNG sequence (see PNGReader) -> planar 8-bit 4:2:0 file, converted on the device (pmctf_rgb8_to_yuv420_u8): the
    .yuv that codes to the same files as the PNGs themselves.  -> (width, height, frames)"""
    from pMCTF.hip import ops
    _need_gpu(device, "pngs_to_yuv")
    reader = PNGReader(paths_or_folder)
    with open(yuv_out, "wb") as f:
        for _ in range(len(reader)):
            frame = ops.rgb8_to_yuv420(torch.from_numpy(reader.read_one_frame()).to(device))
            f.write(frame.cpu().numpy().tobytes(order="C"))
    reader.close()
    return reader.width, reader.height, len(reader)


def rgb_psnr(rec_y, rec_c, y, c):
    """PSNR of the rounded RGB pictures (chroma bilinearly up-sampled), test_pMCTF_flex.py:312-321"""
    from pMCTF.utils.util import ycbcr2rgb, yuv_420_to_444
    to_rgb = lambda luma, chroma: torch.round(ycbcr2rgb(yuv_420_to_444((luma, chroma[0:1], chroma[1:2]))))
    return psnr(to_rgb(y, c), to_rgb(rec_y, rec_c))


def report_gop(rec, orig, h, w, bits, bits_mv, first_frame, tables, ssims, hashes, picture_hash=None, bitdepth=8,
               decoded_frame_path=None, msssim=False):
    """What a sequence driver does with one reconstructed GOP (encode_sequence, pmctf_seq.encode_sequence_gops): the
    picture hashes, the saved PNGs, the quality functions and the per-frame tables, appended in place.  rec: the pictures
    decode_gop returned (a lone picture: its one reconstruction), orig: the un-padded originals."""
    if picture_hash is not None:
        hashes += picture_hashes(rec, h, w, picture_hash, bitdepth)
    if decoded_frame_path is not None:
        write_pngs(decoded_frame_path, first_frame, frames_to_rgb8(rec, h, w))
    if bitdepth > 8:
        quality = gop_quality_hbd(rec, orig, h, w, bitdepth)
    else:
        quality = gop_quality(rec, orig, h, w, msssim=True) if msssim else gop_psnr(rec, orig, h, w)
    tables["bits"] += bits
    tables["bpp_mv"] += [b / (h * w) for b in bits_mv]
    tables["psnr"] += [p["yuv"] for p in quality]
    tables["frame_types"] += [0] + [1] * (len(rec) - 1)         # the one coded L picture of a GOP, then its H pictures
    if msssim or bitdepth > 8:
        tables["psnr_rgb"] += [p["rgb"] for p in quality]
        ssims += [p["msssim"] for p in quality]
        return
    for (ry, rc, _), (y, c) in zip(rec, orig):
        crop_y = torch.round(ry.clamp(0, 255.0))[:, :, :h, :w]
        crop_c = torch.round(rc.clamp(0, 255.0))[:, :, :h // 2, :w // 2]
        tables["psnr_rgb"].append(rgb_psnr(crop_y, crop_c, y, c))


def encode_sequence(codec, yuv_path, width, height, frame_num, gop, q_index, bin_folder, device,
                    skip_decoding=True, psize=128, src_format="yuv", ingest="host", decoded_frame_path=None,
                    picture_hash=None, bitdepth=8, keep_gops=False, msssim=False):
    """What the evaluation harness produces for one sequence (test_pMCTF_flex.py:run_test, 86-346) built from this
    module's own pieces: pictures come from a planar .yuv through YUVReader and get_padding_size, every closed GOP goes
    through encode_gop (one encode_one_stage call per pair, both per-pair report lines), decode_gop and gop_psnr, and
    the per-frame tables are folded into the harness's log record by generate_log_json / dump_json.
    msssim=False (default): PSNR from gop_psnr / rgb_psnr, MS-SSIM reported as 0 — the record the fixtures hold.
    msssim=True: the per-frame quality comes from gop_quality (HIP kernels, no third-party package): frame_msssim and the
    ave_*_msssim fields of the record are filled, and the result gains "msssim".  Pictures need a smaller side above 160
    (0 is reported, as by the harness, when a side is 128 or less).
    keep_gops=True: GOP k goes to bin_folder/gop_{k:05d}/ instead of overwriting GOP k-1's files, and bin_folder gets the
    sequence.json header decode_sequence needs (write_sequence_header).
    src_format="png": yuv_path is a folder of PNGs or a list of paths (PNGReader); width and height are checked against
    the files; the pictures are converted to 4:2:0 and padded on the device (read_gop_device).
    ingest="device": a .yuv source goes through read_gop_device as well (bytes to the device, one launch per picture)
    instead of read_gop's host conversion; the tensors are the same bit for bit.  Either needs a GPU (RuntimeError).
    decoded_frame_path: a folder that receives every reconstructed frame as {frame index}.png, the harness's
    --save_decoded_frame (test_pMCTF_flex.py:334-336), through frames_to_rgb8; nothing is added to bin_folder.
    picture_hash="u8" or "f32" (needs keep_gops=True; default None: off, no file): the CRC-32 of every reconstructed picture,
    taken on the device (picture_hashes), goes to bin_folder/picture_hashes.json, where decode_sequence finds and checks
    it; the result gains "picture_hashes".  sequence.json is the same either way.
    bitdepth=9..16 (keyword; default 8: everything above): yuv_path holds little-endian 16-bit samples of that depth
    (yuv420p10le and its like; src_format "yuv" only, either ingest).  A sample v enters the codec as v * 2^-(bitdepth - 8),
    so a source whose samples are all multiples of 2^(bitdepth - 8) codes to the very files of its 8-bit form.  The quality
    tables come from gop_quality_hbd: "psnr" is the YUV-PSNR at that depth, "psnr_rgb" 0.0 per frame; msssim=True and
    decoded_frame_path are refused (ValueError), picture_hash is "u16" or "f32".  With keep_gops=True bin_folder also gets
    picture_format.json (write_picture_format), which tells decode_sequence the depth.
    pmctf_scale.encode_sequence(..., coded_size=(W, H)) is this function for a sequence coded at another size than its
    source's (the body with a pmctf_chroma.SourcePipeline): the pictures are resampled on the device after upload
    (read_gop_device, whatever `ingest` says) and everything below sees a source of the coded size, sequence.json included;
    with keep_gops=True bin_folder also gets display_format.json, and the result gains "display_quality".
    Returns {"log": record, "json": its text, "bits", "bpp_mv", "psnr", "psnr_rgb", "frame_types", "lines"} (+ "msssim")."""
    return _encode_equal_gops(codec, yuv_path, width, height, frame_num, gop, q_index, bin_folder, device,
                              skip_decoding=skip_decoding, psize=psize, src_format=src_format, ingest=ingest,
                              decoded_frame_path=decoded_frame_path, picture_hash=picture_hash, bitdepth=bitdepth,
                              keep_gops=keep_gops, msssim=msssim)


class SequenceEncode:
    """What encode_sequence's loop and pmctf_seq's GOP-list loop share: encode_sequence's keywords after `device` with their
    refusals (raised here, in this order, before the codec or the source is touched), the reader of the source, the tables
    of the GOPs coded so far, the sidecar files of the folder and the result.
    pipeline: the pmctf_chroma.SourcePipeline of a source that is converted or resampled on its way into the codec, None
    for one that enters as it is: then a .yuv is read by YUVReader and, with ingest="host", through read_gop."""

    def __init__(self, pipeline=None, skip_decoding=True, psize=128, src_format="yuv", ingest="host", decoded_frame_path=None,
                 picture_hash=None, bitdepth=8, keep_gops=False, msssim=False):
        if picture_hash is not None and picture_hash not in HASH_LEVELS:
            raise ValueError(f"picture_hash is None or one of {HASH_LEVELS} (got {picture_hash!r})")
        if picture_hash is not None and not keep_gops:
            raise ValueError("picture_hash needs keep_gops=True: the hashes belong to a folder decode_sequence can read")
        bitdepth = check_bitdepth(bitdepth)
        if picture_hash is not None:
            check_hash_level(picture_hash, bitdepth)
        if bitdepth > 8:
            if src_format == "png":
                raise ValueError(f"bitdepth {bitdepth}: a source above 8 bits is a .yuv file (src_format='yuv'), PNG input is 8-bit")
            if msssim:
                raise ValueError(f"bitdepth {bitdepth}: MS-SSIM and RGB-PSNR are defined on 8-bit RGB pictures (msssim=False)")
            if decoded_frame_path is not None:
                raise ValueError(f"bitdepth {bitdepth}: decoded_frame_path writes 8-bit PNGs; decode the folder to a .yuv instead")
        self.pipeline, self.skip_decoding, self.psize, self.keep_gops = pipeline, skip_decoding, psize, keep_gops
        self.src_format, self.ingest, self.bitdepth = src_format, ingest, bitdepth
        self.decoded_frame_path, self.picture_hash, self.msssim = decoded_frame_path, picture_hash, msssim
        self.on_device = src_format == "png" or ingest == "device" or pipeline is not None
        self.tables = {k: [] for k in ("bits", "bpp_mv", "psnr", "psnr_rgb", "frame_types")}
        self.lines, self.ssims, self.hashes, self.display = [], [], [], []
        self.pairs = 0
        self.seconds = {"encoding_time": 0.0, "decoding_time": 0.0}

    def check_source_kind(self):
        if self.src_format not in ("yuv", "png") or self.ingest not in ("host", "device"):
            raise ValueError(f"src_format is 'yuv' or 'png' and ingest 'host' or 'device' (got {self.src_format!r}, "
                             f"{self.ingest!r})")

    def open_reader(self, source, width, height, frame_num, keep=False):
        """a fresh reader of the source; with a pipeline its pictures are converted on the device after upload
        (read_gop_device), and keep=True keeps them for the pipeline's display_quality"""
        if self.src_format == "png":
            reader = PNGReader(source)
            if (reader.width, reader.height) != (width, height):
                raise ValueError(f"the pictures are {reader.width}x{reader.height}, not {width}x{height}")
            if len(reader) < frame_num:
                raise ValueError(f"{frame_num} frames asked for, {len(reader)} pictures found")
        elif self.pipeline is not None:
            reader = self.pipeline.open_reader(source, width, height, self.bitdepth)
        else:
            from pMCTF.utils.yuv_reader import YUVReader
            reader = YUVReader(source, width, height, start_index=0, bitdepth=self.bitdepth)
        if self.pipeline is not None:
            reader.resample = self.pipeline.ingest(keep)
        return reader

    def read_gop(self, reader, size, device, psize):
        return (read_gop_device if self.on_device else read_gop)(reader, size, device, psize)

    def add_pairs(self, enc):
        """the times and the report lines of the pairs of one encode_gop result"""
        for r in enc["results"]:
            self.pairs += 1
            for k in self.seconds:
                self.seconds[k] += r[k]
        self.lines += enc["log"]

    def add_gop(self, rec, orig, h, w, bits, bits_mv, first_frame):
        """one reconstructed GOP: report_gop, and the pipeline's display quality"""
        report_gop(rec, orig, h, w, bits, bits_mv, first_frame, self.tables, self.ssims, self.hashes,
                   picture_hash=self.picture_hash, bitdepth=self.bitdepth, decoded_frame_path=self.decoded_frame_path,
                   msssim=self.msssim)
        if self.pipeline is not None:
            self.display += self.pipeline.display_quality(rec)

    def write_sidecars(self, bin_folder):
        """what a folder holds beside its header: the picture hashes, the picture format, the pipeline's records"""
        if self.picture_hash is not None:
            write_picture_hashes(bin_folder, self.picture_hash, self.hashes)
        if self.bitdepth > 8:
            write_picture_format(bin_folder, self.bitdepth)
        if self.pipeline is not None:
            self.pipeline.write_header(bin_folder)

    def average_lines(self):
        for k, label in (("encoding_time", "encoding"), ("decoding_time", "decoding")):
            self.lines.append(f"{label} {self.pairs} P frames, average {self.seconds[k] / self.pairs * 1000:.0f} ms.")

    def result(self, frame_num, width, height, t0, **extra):
        import io
        import time
        from pMCTF.utils.video_eval_utils import dump_json, generate_log_json
        tables = self.tables
        record = generate_log_json(frame_num, tables["frame_types"], tables["bits"], tables["bpp_mv"], tables["psnr"],
                                   tables["psnr_rgb"], self.ssims if self.msssim else [0] * frame_num, height * width,
                                   time.time() - t0)
        text = io.StringIO()
        dump_json(record, text, float_digits=6, indent=2)
        out = dict(tables, log=record, json=text.getvalue(), lines=self.lines, **extra)
        if self.msssim:
            out["msssim"] = self.ssims
        if self.picture_hash is not None:
            out["picture_hashes"] = self.hashes
        if self.pipeline is not None:
            out["display_quality"] = self.display
        return out


def _encode_equal_gops(codec, yuv_path, width, height, frame_num, gop, q_index, bin_folder, device, *, pipeline=None, **options):
    """encode_sequence's body; options: its keywords after `device` (SequenceEncode)"""
    import time
    e = SequenceEncode(pipeline, **options)
    assert frame_num % gop == 0
    e.check_source_kind()
    if e.on_device:
        _need_gpu(device, f"encode_sequence(src_format={e.src_format!r}, ingest={e.ingest!r})")
    reader = e.open_reader(yuv_path, width, height, frame_num, keep=True)
    if pipeline is not None:
        width, height = pipeline.coded
    t0 = time.time()
    with torch.no_grad():
        for k in range(frame_num // gop):
            padded, orig, (h, w) = e.read_gop(reader, gop, device, e.psize)
            folder = bin_folder
            if e.keep_gops:
                folder = os.path.join(bin_folder, gop_folder(k))
                os.makedirs(folder, exist_ok=True)
            enc = encode_gop(codec, padded, h, w, q_index, folder, skip_decoding=e.skip_decoding, psize=e.psize)
            e.add_pairs(enc)
            e.add_gop(decode_gop(codec, enc["frames_coded"]), orig, h, w, enc["bits"], enc["bits_mv"], k * gop)
    reader.close()
    if e.keep_gops:
        write_sequence_header(bin_folder, width=width, height=height, frame_num=frame_num, gop=gop, q_index=q_index,
                              psize=e.psize, me_downsample=1, ll_order="plane" if e.skip_decoding else "position",
                              **codec_header_fields(codec))
        e.write_sidecars(bin_folder)
    e.average_lines()
    return e.result(frame_num, width, height, t0)


def quality_line(idx, q, bpp=None, seconds=None):
    """one frame's report line in the harness's wording (test_pMCTF_flex.py:330-332); the coding time and rate are left
    out where there is none (two files compared)"""
    head = f"frame {idx}" + ("" if seconds is None else f", {seconds:.3f} seconds") + ","
    rate = "" if bpp is None else f"bpps: {bpp:.3f}, "
    return (f"{head} {rate}YUV-PSNR: {q['yuv']:.4f}, RGB-PSNR: {q['rgb']:.4f},MS-SSIM: {q['msssim']:.4f}, "
            f"Y-PSNR: {q['y']:.4f},  Cb-PSNR: {q['cb']:.4f}, Cr-PSNR: {q['cr']:.4f}  ")


def sequence_quality(src_yuv, rec_yuv, width, height, frame_num, device, gop=None, msssim=True, bitdepth=8):
    """Quality of a decoded planar 8-bit 4:2:0 file against its source, frame by frame, through YUVReader and gop_quality
    (the files -> .yuv -> quality end of the loop decode_sequence opens).  bitdepth=9..16: both files hold 16-bit samples
    of that depth and the numbers come from gop_quality_hbd (PSNR against 2^bitdepth - 1, "sse" (Y, Cb, Cr); "psnr_rgb" and
    "msssim" are 0.0 whatever msssim says: they are defined on 8-bit RGB).
    -> {"psnr" (YUV), "psnr_rgb", "msssim", "psnr_y", "psnr_cb", "psnr_cr": per-frame lists, "sse": [(Y, Cb, Cr, RGB)],
        "mean": {table: mean}, "frame_types": [0] + [1] * (gop - 1) per GOP when gop is given (as encode_sequence), else
        None, "lines": one report line per frame}."""
    from pMCTF.utils.yuv_reader import YUVReader
    if torch.device(device).type != "cuda":
        raise RuntimeError("sequence_quality runs on the GPU (no CPU fallback)")
    if width <= 0 or height <= 0 or (width | height) & 1 or frame_num <= 0:
        raise ValueError(f"4:2:0 pictures have even, positive sizes (got {width}x{height}, {frame_num} frames)")
    if gop is not None and (gop < 1 or frame_num % gop):
        raise ValueError(f"frame_num {frame_num} is not a multiple of gop {gop}")
    bitdepth = check_bitdepth(bitdepth)
    frame_bytes = (width * height + 2 * (width // 2) * (height // 2)) * (2 if bitdepth > 8 else 1)
    for path in (src_yuv, rec_yuv):
        if os.path.getsize(path) < frame_num * frame_bytes:
            raise ValueError(f"{path}: shorter than {frame_num} pictures of {width}x{height}")
    ro, rd = (YUVReader(p, width, height, start_index=0, bitdepth=bitdepth) for p in (src_yuv, rec_yuv))
    names = {"yuv": "psnr", "rgb": "psnr_rgb", "msssim": "msssim", "y": "psnr_y", "cb": "psnr_cb", "cr": "psnr_cr"}
    out = {v: [] for v in names.values()}
    out.update(sse=[], lines=[])
    try:
        for idx in range(frame_num):
            # psize=2: nothing to pad (the sizes are even), the pictures go to the kernels as they are in the files
            _, orig, (h, w) = read_gop(ro, 1, device, psize=2)
            _, dec, _ = read_gop(rd, 1, device, psize=2)
            if bitdepth > 8:
                q = gop_quality_hbd([(dec[0][0], dec[0][1], None)], orig, h, w, bitdepth)[0]
            else:
                q = gop_quality([(dec[0][0], dec[0][1], None)], orig, h, w, msssim=msssim)[0]
            for k, v in names.items():
                out[v].append(q[k])
            out["sse"].append(q["sse"])
            out["lines"].append(quality_line(idx, q))
    finally:
        ro.close()
        rd.close()
    out["mean"] = {v: sum(out[v]) / frame_num for v in names.values()}
    out["frame_types"] = None if gop is None else ([0] + [1] * (gop - 1)) * (frame_num // gop)
    return out


# ---------------------------------------------------------------------------------------------------- decoding from files
SEQUENCE_HEADER = "sequence.json"
SEQUENCE_FORMAT_VERSION = 1
SEQUENCE_FIELDS = ("width", "height", "frame_num", "gop", "q_index", "psize", "me_downsample", "num_me_stages", "ll_order",
                   "precision", "aten_threads")
LL_ORDERS = ("position", "plane")


GOP_STRUCTURE = "gop_structure.json"                  # the header of a structured folder (pmctf_seq), instead of sequence.json
GOP_STRUCTURE_VERSION_Q = 2                           # its format version whose GOP entries carry their own q_index


def sequence_layout(bin_folder):
    """-> (header record, [(first, size, psize, me_downsample)] per GOP folder) of a folder written by encode_sequence
    (keep_gops=True: sequence.json, equal GOPs) or by pmctf_seq.encode_sequence_gops (gop_structure.json: a list of GOPs).
    ValueError as read_sequence_header / pmctf_seq.read_gop_structure raise it; a folder with both headers is refused."""
    if os.path.exists(os.path.join(bin_folder, GOP_STRUCTURE)):
        import pmctf_seq
        header = pmctf_seq.read_gop_structure(bin_folder)
        return header, [(g["first"], g["size"], g["psize"], g["me_downsample"]) for g in header["gops"]]
    header = read_sequence_header(bin_folder)
    gop = header["gop"]
    return header, [(k * gop, gop, header["psize"], header["me_downsample"]) for k in range(header["frame_num"] // gop)]


def gop_q_indexes(header, n_gops):
    """-> the q_index of each of the n_gops GOPs of a folder: a gop_structure.json of format version 2
    (pmctf_rate.encode_sequence_rate) holds one per GOP; every other header has one for the sequence"""
    if GOP_STRUCTURE_VERSION_Q == header.get("format_version") and "gops" in header:
        return [g["q_index"] for g in header["gops"]]
    return [header["q_index"]] * n_gops


def gop_folder(k):
    """sub-folder of GOP k in a sequence written with encode_sequence(keep_gops=True)"""
    return f"gop_{k:05d}"


def gop_pairs(gop):
    """[(stage, i_ref, i_cur)] in coding order: stage s codes the pairs (2k*2^s, 2k*2^s + 2^s)"""
    stages = int(round(math.log2(gop)))
    if 2 ** stages != gop or gop < 2:
        raise ValueError("the GOP length must be a power of two, at least 2")
    return [(s, g * 2 * 2 ** s, g * 2 * 2 ** s + 2 ** s) for s in range(stages) for g in range(gop >> (s + 1))]


def gop_file_names(gop):
    """the files encode_gop writes for one GOP, in coding order: per pair the H picture's luma, chroma and motion files;
    the one L picture's luma and chroma files come with the last pair"""
    names = []
    for _, _, i_cur in gop_pairs(gop):
        names += [f"{i_cur}.bin", f"{i_cur}_C_main.bin", f"{i_cur}_mv.bin"]
    return names + ["0_main.bin", "0_C_main.bin"]


def codec_header_fields(codec):
    """what a decoder must share with the encoder beyond the weights: the number of motion stages, the engine's
    arithmetic profile and the thread count its torch.sigmoid restatement assumes (PMCTF_ATEN_THREADS as the engine
    read it)"""
    eng = codec.engine()
    return {"num_me_stages": int(codec.num_me_stages), "precision": str(eng.precision),
            "aten_threads": int(eng.aten_threads)}


def write_sequence_header(bin_folder, **fields):
    """bin_folder/sequence.json: format version + SEQUENCE_FIELDS (all required, nothing else accepted)"""
    if set(fields) != set(SEQUENCE_FIELDS):
        raise ValueError(f"sequence header fields: missing {sorted(set(SEQUENCE_FIELDS) - set(fields))}, "
                         f"unknown {sorted(set(fields) - set(SEQUENCE_FIELDS))}")
    if fields["ll_order"] not in LL_ORDERS:
        raise ValueError(f"ll_order must be one of {LL_ORDERS}")
    record = {"format_version": SEQUENCE_FORMAT_VERSION}
    record.update({k: fields[k] if k in ("ll_order", "precision") else int(fields[k]) for k in SEQUENCE_FIELDS})
    return write_record(os.path.join(bin_folder, SEQUENCE_HEADER), record, indent=2)


def read_sequence_header(bin_folder):
    path = os.path.join(bin_folder, SEQUENCE_HEADER)
    record = read_record(path, "sequence header", SEQUENCE_FORMAT_VERSION,
                         missing="not a folder written with encode_sequence(keep_gops=True)")
    missing = [k for k in SEQUENCE_FIELDS if k not in record]
    if missing:
        raise ValueError(f"{path}: fields {missing} missing")
    if record["ll_order"] not in LL_ORDERS:
        raise ValueError(f"{path}: ll_order {record['ll_order']!r}")
    if record["frame_num"] % record["gop"]:
        raise ValueError(f"{path}: frame_num {record['frame_num']} is not a multiple of gop {record['gop']}")
    return record


def check_sequence_header(header, codec_fields):
    """refuse a decoder whose motion stages, arithmetic profile or ATen thread setting differ from the encoder's: its
    entropy parameters would differ in their last bits and the streams desynchronise silently"""
    diff = {k: (header[k], v) for k, v in codec_fields.items() if header[k] != v}
    if diff:
        raise ValueError("the sequence was coded with a different codec configuration: " +
                         ", ".join(f"{k} {a!r} in the header, {b!r} here" for k, (a, b) in sorted(diff.items())))


PICTURE_FORMAT = "picture_format.json"
PICTURE_FORMAT_VERSION = 1


def write_picture_format(bin_folder, bitdepth):
    """bin_folder/picture_format.json: {"format_version", "bitdepth"}, the depth 9..16 of the source's 16-bit samples.
    Written beside sequence.json only for a source above 8 bits; the bitstream files and sequence.json do not know it."""
    path = os.path.join(bin_folder, PICTURE_FORMAT)
    try:
        bitdepth = check_bitdepth(bitdepth, above8=True)
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None
    return write_record(path, {"format_version": PICTURE_FORMAT_VERSION, "bitdepth": bitdepth}, indent=2)


def read_picture_format(bin_folder):
    """-> the bit depth of the folder's pictures: 8 when there is no picture_format.json, else the 9..16 it holds;
    ValueError naming the path for a malformed file, another version, an unknown field or another depth"""
    path = os.path.join(bin_folder, PICTURE_FORMAT)
    record = read_record(path, "picture format file", PICTURE_FORMAT_VERSION, fields=("bitdepth",),
                         expected="format_version and bitdepth")
    if record is None:
        return 8
    try:
        return check_bitdepth(record["bitdepth"], above8=True)
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None


def _read_framed(path, header_bytes):
    """the bytes of a bitstream file whose header ends with a big-endian uint32 payload length; ValueError naming the
    file when it is missing, cut short or longer than its header says"""
    import struct
    try:
        with open(path, "rb") as f:
            data = f.read()
    except FileNotFoundError:
        raise ValueError(f"{path}: missing") from None
    if len(data) < header_bytes:
        raise ValueError(f"{path}: truncated ({len(data)} bytes, shorter than its header)")
    (n,) = struct.unpack(">I", data[header_bytes - 4:header_bytes])
    if len(data) < header_bytes + n:
        raise ValueError(f"{path}: truncated ({len(data)} bytes, the header announces {header_bytes + n})")
    if len(data) > header_bytes + n:
        raise ValueError(f"{path}: {len(data) - header_bytes - n} surplus bytes after the announced {header_bytes + n}")
    return data


def _read_gop_files(codec, bin_folder, gop, pic_height, pic_width, q_index, psize, me_downsample, ll_order, pictures=None,
                    motions=None, spatial_level=0, counters=None):
    """The one reader of a GOP's files, under every decoder: of the pairs of the GOP, in coding order, the two picture files
    of those whose i_cur is in `pictures` and the motion file of those whose i_cur is in `motions` (None: of every pair),
    then the two L files; gop == 1: the two L files alone.  `motions` holds, of every stage it touches, the pairs from the
    stage's first on: the context runs pair to pair.  Every file is read and its header checked before the codec is touched.
    The picture files are started as ONE batch (codec._decompress_gop_files_begin), under it the motion files are decoded in
    coding order (the context restarts per stage, as in encode_gop: what makes the temporal layers independent; a
    reduced-resolution stream is decoded at the size it was coded at), then the batch is finished.
    spatial_level=k: the planes of every picture file at spatial level k (the motion fields stay as coded).  counters: a
    dict that receives, per picture file name, what the engine says it read of it: {"symbols_decoded",
    "payload_bytes_used"}.
    -> (frames_coded: [L_t / H_t, L_tc / H_tc, mv_hat] entries with None where nothing was read, names read, bytes read)."""
    import struct
    pairs = gop_pairs(gop) if gop != 1 else []          # a lone picture (pmctf_seq): its two L files, no motion
    pad_h = -(-pic_height // psize) * psize
    pad_w = -(-pic_width // psize) * psize
    files, paths, slots, read = [], [], [], []
    nbytes = 0

    def picture(name, chroma, low, me_num, slot):
        nonlocal nbytes
        path = os.path.join(bin_folder, name)
        data = _read_framed(path, 16)
        h, w, n = struct.unpack(">III", data[:12])
        want = (pic_height // 2, pic_width // 2, 2) if chroma else (pic_height, pic_width, 1)
        if (h, w, n) != want:
            raise ValueError(f"{path}: header says {n} plane(s) of {h}x{w}, expected {want[2]} of {want[0]}x{want[1]}")
        files.append((data, chroma, low, me_num))
        paths.append(path)
        slots.append(slot)
        read.append(name)
        nbytes += len(data)

    motion = []
    for stage, _, i_cur in pairs:
        me_num = min(codec.num_me_stages - 1, stage)
        if pictures is None or i_cur in pictures:
            picture(f"{i_cur}.bin", False, False, me_num, (i_cur, 0))
            picture(f"{i_cur}_C_main.bin", True, False, me_num, (i_cur, 1))
        if motions is not None and i_cur not in motions:
            continue
        path = os.path.join(bin_folder, f"{i_cur}_mv.bin")
        data = _read_framed(path, 6)
        motion.append((stage, i_cur, me_num, path, data[6:]))
        read.append(f"{i_cur}_mv.bin")
        nbytes += len(data)
    picture("0_main.bin", False, True, 0, (0, 0))
    picture("0_C_main.bin", True, True, 0, (0, 1))

    begun = codec._decompress_gop_files_begin(files, psize, q_index, ll_order, paths, spatial_level=spatial_level)
    frames_coded = [[None, None, None] for _ in range(gop)]
    dpb, at_stage = None, None
    try:
        for stage, i_cur, me_num, path, string in motion:
            if stage != at_stage:
                dpb, at_stage = {"mv_feature": None, "ref_mv_y": None}, stage
            try:
                d = codec.decompress_mv(string, torch.float32, pad_h // me_downsample, pad_w // me_downsample, dpb,
                                        stage_idx=me_num, q_index=q_index, me_downsample=me_downsample)
            except (ValueError, RuntimeError) as e:
                raise ValueError(f"{path}: {e}") from e
            frames_coded[i_cur][2] = d["mv_hat"]
            dpb = {"mv_feature": d["mv_feature"], "ref_mv_y": d["mv_y_hat"]}
    finally:
        # the picture files are finished (and their threads and streams drained) whatever the motion files did
        planes = codec._decompress_gop_files_end(begun)
    for (i, c), plane in zip(slots, planes):
        frames_coded[i][c] = plane
    if counters is not None:
        for path, job in zip(paths, begun[0]):
            counters[os.path.basename(path)] = {key: job[key] for key in ("symbols_decoded", "payload_bytes_used")}
    return frames_coded, read, nbytes


def decode_gop_files(codec, bin_folder, gop, pic_height, pic_width, q_index, psize=128, me_downsample=1, ll_order="plane",
                     luma_stage0=False):
    """Decode one GOP from the files encode_gop wrote into bin_folder, with nothing else from the encoder.
    gop=1: a lone picture of a structured sequence (pmctf_seq): 0_main.bin and 0_C_main.bin through the same batch.
    Every picture file of the GOP is started as ONE batch (their sequential LL parts side by side, batched per geometry:
    codec._decompress_gop_files_begin); under them the motion files are decoded stage by stage, pair by pair in coding
    order (the motion context restarts per stage, as in encode_gop; a reduced-resolution motion stream is decoded at the
    size it was coded at); then the files' remaining subbands are finished and the temporal synthesis (decode_gop) runs.
    ll_order: "plane" for files written with skip_decoding=True (chroma's LL symbols plane after plane), "position" for
    decoder-order files (skip_decoding=False).
    Returns {"frames": [[Y, UV, None]] reconstructed (padded) pictures, "frames_coded": the decoded [L_t / H_t, L_tc /
    H_tc, mv_hat] entries decode_gop consumed}.  A missing, truncated or surplus-length file raises a ValueError that
    names it."""
    if ll_order not in LL_ORDERS:
        raise ValueError(f"ll_order must be one of {LL_ORDERS}")
    with torch.no_grad():
        frames_coded, _, _ = _read_gop_files(codec, bin_folder, gop, pic_height, pic_width, q_index, psize, me_downsample,
                                             ll_order)
        coded = [list(fc) for fc in frames_coded]
        rec = decode_gop(codec, frames_coded, luma_stage0=luma_stage0)
    return {"frames": rec, "frames_coded": coded, "stages": int(round(math.log2(gop)))}


def frames_to_samples(frames_rec, pic_height, pic_width, bitdepth=8):
    """reconstructed (padded, float) pictures -> [(Y, Cb, Cr)] arrays of the un-padded size, rint(clamp(x * 2^(bitdepth - 8),
    0, 2^bitdepth - 1)): uint8 at bitdepth 8, uint16 at 9..16 (write_yuv writes those as the 16-bit file layout).  One
    conversion launch per plane tensor (ops.planes_to) and one copy of bytes to the host"""
    from pMCTF.hip import ops
    out = []
    for rec_y, rec_c, _ in frames_rec:
        y = ops.planes_to(rec_y.contiguous(), pic_height, pic_width, bitdepth)
        c = ops.planes_to(rec_c.contiguous(), pic_height // 2, pic_width // 2, bitdepth)
        out.append((y, c))
    host = [(y.cpu().numpy(), c.cpu().numpy()) for y, c in out]
    return [(y[0], c[0], c[1]) for y, c in host]


def frames_to_u8(frames_rec, pic_height, pic_width):
    """frames_to_samples at 8 bits (pmctf_planes_to_u8)"""
    return frames_to_samples(frames_rec, pic_height, pic_width)


def frames_to_u16(frames_rec, pic_height, pic_width, bitdepth):
    """frames_to_samples at a bitdepth of 9..16 (pmctf_planes_to_u16); 8 is refused"""
    from pMCTF.hip import ops
    return frames_to_samples(frames_rec, pic_height, pic_width, ops._bitdepth(bitdepth))


def frames_to_rgb8(frames_rec, pic_height, pic_width):
    """reconstructed (padded, float) pictures -> [(h, w, 3) uint8 RGB arrays] of the un-padded size, the pictures the
    harness saves (test_pMCTF_flex.py:76-79,313-317): one launch (pmctf_yuv420_to_rgb8_f32) and one copy of bytes to the
    host per picture.  The sibling of frames_to_u8."""
    from pMCTF.hip import ops
    out = [ops.frame_to_rgb8(rec[0].float(), rec[1].float(), pic_height, pic_width) for rec in frames_rec]
    return [rgb.cpu().numpy() for rgb in out]


def write_pngs(folder, first_index, pictures):
    """[(h, w, 3) uint8 RGB arrays] -> folder/{first_index}.png, {first_index + 1}.png, ...: the harness's naming
    (test_pMCTF_flex.py:335).  -> the paths written"""
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    paths = []
    for i, rgb in enumerate(pictures):
        if rgb.ndim != 3 or rgb.shape[2] != 3 or str(rgb.dtype) != "uint8":
            raise ValueError(f"expect (h, w, 3) uint8 pictures, got {rgb.shape} {rgb.dtype}")
        paths.append(os.path.join(folder, f"{first_index + i}.png"))
        Image.fromarray(rgb).save(paths[-1])
    return paths


# ------------------------------------------------------------------------------------------------------- picture hashes
# The encoder records the CRC-32 (zlib.crc32) of every reconstructed picture, the decoder recomputes and compares: the
# check that the decoder reproduces the encoder's reconstruction, on the user's own sequence.  A frame's "frame" value is
# the CRC-32 of that frame's bytes in the decoded .yuv, so a decoded file can be checked with zlib alone
# (check_yuv_hashes, tools/check_picture_hashes.py).
PICTURE_HASHES = "picture_hashes.json"
PICTURE_HASH_FORMAT_VERSION = 1
HASH_LEVELS = ("u8", "f32", "u16")
HASH_KEYS = {"u8": ("y", "cb", "cr", "frame"), "f32": ("y", "cb", "cr", "frame", "y_f32", "c_f32"),
             "u16": ("y", "cb", "cr", "frame")}


def check_hash_level(level, bitdepth):
    """the integer planes hashed are the ones written to the decoded file: bytes at 8 bits ("u8"), 16-bit samples above
    ("u16"); "f32" adds the float tensors at either depth.  ValueError for a level that does not go with the depth."""
    if level not in HASH_LEVELS:
        raise ValueError(f"level is one of {HASH_LEVELS} (got {level!r})")
    if level == ("u8" if bitdepth > 8 else "u16"):
        raise ValueError(f"picture hash level {level!r} does not go with bitdepth {bitdepth}: "
                         f"{'u16' if bitdepth > 8 else 'u8'} or f32")
_CRC_POLY, _CRC_ONE = 0xEDB88320, 0x80000000


def _crc_mulmod(a, b):
    """a(x) * b(x) modulo the CRC-32 polynomial, in the CRC's reflected bit order (bit 31 is x^0)"""
    p = 0
    while a:
        if a & _CRC_ONE:
            p ^= b
        a = (a << 1) & 0xffffffff
        b = (b >> 1) ^ (_CRC_POLY if b & 1 else 0)
    return p


def crc32_combine(crc_a, crc_b, len_b):
    """zlib.crc32(A + B) from crc_a = zlib.crc32(A), crc_b = zlib.crc32(B) and len_b = len(B) (zlib's crc32_combine, which
    the standard library does not expose): crc_a * x^(8 len_b) + crc_b modulo the CRC polynomial.  Pure Python."""
    if len_b < 0:
        raise ValueError("len_b must not be negative")
    power, square, n = _CRC_ONE, _CRC_ONE >> 8, int(len_b)           # x^0; x^8, squared once per bit of len_b
    while n:
        if n & 1:
            power = _crc_mulmod(square, power)
        square = _crc_mulmod(square, square)
        n >>= 1
    return _crc_mulmod(power, crc_a & 0xffffffff) ^ (crc_b & 0xffffffff)


def picture_hashes(frames_rec, pic_height, pic_width, level, bitdepth=8):
    """CRC-32 of reconstructed (padded, float) pictures, taken on the device in ONE ops.crc32 call for all of them.
    -> per frame {"y", "cb", "cr": of the cropped, rounded planes as frames_to_u8 writes them (ops.planes_to_u8), "frame":
    of the three in file order (crc32_combine), the CRC-32 of the frame's bytes in the .yuv}; level "f32" adds "y_f32" and
    "c_f32", of the padded float32 luma and chroma tensors as stored, the stricter check.
    bitdepth=9..16: the integer planes are the 16-bit ones of frames_to_u16 (ops.planes_to_u16), hashed as their
    little-endian bytes go to the file; the levels are then "u16" (the keys of "u8") and "f32"."""
    from pMCTF.hip import ops
    bitdepth = check_bitdepth(bitdepth)
    check_hash_level(level, bitdepth)
    hc, wc = pic_height // 2, pic_width // 2
    per_frame = len(HASH_KEYS[level]) - 1
    sample_bytes = 2 if bitdepth > 8 else 1
    tensors = []
    for rec_y, rec_c, _ in frames_rec:
        y, c = rec_y.contiguous(), rec_c.contiguous()
        c8 = ops.planes_to(c, hc, wc, bitdepth)
        tensors += [ops.planes_to(y, pic_height, pic_width, bitdepth), c8[0], c8[1]]
        if level == "f32":
            tensors += [y, c]
    crcs = ops.crc32(tensors)
    out = []
    for i in range(len(frames_rec)):
        v = crcs[i * per_frame:(i + 1) * per_frame]
        rec = {"y": v[0], "cb": v[1], "cr": v[2],
               "frame": crc32_combine(crc32_combine(v[0], v[1], hc * wc * sample_bytes), v[2], hc * wc * sample_bytes)}
        if level == "f32":
            rec.update(y_f32=v[3], c_f32=v[4])
        out.append(rec)
    return out


def _check_hash_records(path, level, frames, frame_num=None):
    if level not in HASH_LEVELS:
        raise ValueError(f"{path}: level {level!r}, this decoder knows {HASH_LEVELS}")
    if not isinstance(frames, list) or (frame_num is not None and len(frames) != frame_num):
        got = len(frames) if isinstance(frames, list) else None
        raise ValueError(f"{path}: {got!r} frame records, the sequence has {frame_num}")
    for i, rec in enumerate(frames):
        if not isinstance(rec, dict) or set(rec) != set(HASH_KEYS[level]):
            raise ValueError(f"{path}: frame {i}: a record of level {level!r} holds exactly {HASH_KEYS[level]}")
        for k, v in rec.items():
            if not is_int(v) or not 0 <= v <= 0xffffffff:
                raise ValueError(f"{path}: frame {i}: {k} is not a 32-bit value ({v!r})")


def write_picture_hashes(bin_folder, level, frames):
    """bin_folder/picture_hashes.json: format version, level and one picture_hashes record per frame in display order"""
    path = os.path.join(bin_folder, PICTURE_HASHES)
    _check_hash_records(path, level, frames)
    record = {"format_version": PICTURE_HASH_FORMAT_VERSION, "level": level,
              "frames": [{k: int(rec[k]) for k in HASH_KEYS[level]} for rec in frames]}
    return write_record(path, record, indent=1)


def read_picture_hashes(bin_folder, frame_num):
    """-> {"format_version", "level", "frames"}; ValueError naming the path for a missing or malformed file, another
    version, an unknown level or a frame list that does not have frame_num well-formed records"""
    path = os.path.join(bin_folder, PICTURE_HASHES)
    record = read_record(path, "picture hash file", PICTURE_HASH_FORMAT_VERSION, fields=("level", "frames"),
                         missing="the sequence was coded without picture_hash", expected="format_version, level and frames")
    _check_hash_records(path, record["level"], record["frames"], frame_num)
    return record


class PictureHashMismatch(ValueError):
    """a decoded picture is not the one the encoder reconstructed; .mismatch: {"gop", "folder", "frame", "plane",
    "decoded", "recorded"}"""

    def __init__(self, mismatch):
        self.mismatch = dict(mismatch)
        super().__init__(describe_hash_mismatch(mismatch))


def describe_hash_mismatch(m):
    where = f"{m['folder']}: " if m.get("folder") else ""
    return (f"{where}frame {m['frame']}, plane {m['plane']}: decoded picture hashes to {m['decoded']:#010x}, the encoder "
            f"recorded {m['recorded']:#010x}")


def compare_hash_records(decoded, recorded, first_frame=0, **where):
    """mismatches between two lists of picture_hashes records, on the keys of the recorded ones, frame by frame in key
    order -> [{**where, "frame", "plane", "decoded", "recorded"}]"""
    out = []
    for i, (got, want) in enumerate(zip(decoded, recorded)):
        out += [dict(where, frame=first_frame + i, plane=k, decoded=got[k], recorded=want[k])
                for k in HASH_KEYS["f32"] if k in want and got[k] != want[k]]
    return out


def check_yuv_hashes(bin_folder, yuv_path):
    """A decoded planar 4:2:0 file against bin_folder's picture_hashes.json at the u8 level, on the host with zlib alone
    -> (frames checked, mismatches as compare_hash_records lists them).  ValueError for a file of the wrong length.
    A folder with a picture_format.json holds pictures of 16-bit samples: two bytes each, the u16 level."""
    import zlib
    header, _ = sequence_layout(bin_folder)
    sample_bytes = 2 if read_picture_format(bin_folder) > 8 else 1
    recorded = read_picture_hashes(bin_folder, header["frame_num"])["frames"]
    h, w = header["height"], header["width"]
    ny, nc = h * w * sample_bytes, (h // 2) * (w // 2) * sample_bytes
    if os.path.getsize(yuv_path) != header["frame_num"] * (ny + 2 * nc):
        raise ValueError(f"{yuv_path}: {os.path.getsize(yuv_path)} bytes, {header['frame_num']} pictures of {w}x{h} have "
                         f"{header['frame_num'] * (ny + 2 * nc)}")
    decoded = []
    with open(yuv_path, "rb") as f:
        for _ in recorded:
            data = f.read(ny + 2 * nc)
            decoded.append({"y": zlib.crc32(data[:ny]), "cb": zlib.crc32(data[ny:ny + nc]), "cr": zlib.crc32(data[ny + nc:]),
                            "frame": zlib.crc32(data)})
    u8 = [{k: rec[k] for k in HASH_KEYS["u8"]} for rec in recorded]
    return len(decoded), compare_hash_records(decoded, u8, folder=yuv_path)


def decode_sequence(codec, bin_folder, yuv_out, device=None, png_out=None):
    """Decode a folder written by encode_sequence(keep_gops=True) into a planar 8-bit 4:2:0 file (the layout YUVReader
    reads), GOP by GOP.  The codec holds the weights the sequence was coded with; its number of motion stages, arithmetic
    profile and ATen thread setting must equal the header's (ValueError otherwise).  device: checked against the
    codec's, if given.  png_out: a folder that receives every decoded picture as {index}.png (frames_to_rgb8, write_pngs);
    yuv_out may then be None (PNGs only).
    A folder that holds picture hashes (encode_sequence(picture_hash=...)) is checked against them:
    decode_sequence_checked with verify="auto", which also has the other modes.  Its parameters stay these five.
    A folder with a picture_format.json (encode_sequence(bitdepth=9..16)) is written as little-endian 16-bit samples of
    that depth (frames_to_u16); png_out is then refused (ValueError).
    A folder with a gop_structure.json instead of a sequence.json (pmctf_seq.encode_sequence_gops) is decoded GOP by GOP
    with every GOP's own size, psize and me_downsample (sequence_layout); "header" is then the structure record.
    Returns {"header", "frames": [(height, width)] per written picture, "seconds": per GOP, "verified": pictures checked,
    "hash_mismatches": [], "bitdepth"}."""
    return decode_sequence_checked(codec, bin_folder, yuv_out, device, png_out, verify="auto")


def decode_sequence_checked(codec, bin_folder, yuv_out, device=None, png_out=None, verify="auto"):
    """decode_sequence with the choice of what to do with the folder's picture_hashes.json.  verify="auto" (what
    decode_sequence does): check every decoded picture against it when it is there, nothing otherwise; True: the same,
    and a ValueError when it is missing; False: never look at it; "report": check, write every picture all the same and
    return the mismatches.  The hashes are taken on the device (picture_hashes, at the file's level) before anything of a
    GOP is written; under "auto" and True the first mismatch raises PictureHashMismatch (a ValueError naming the GOP's
    folder, the frame, the plane and both values) with none of that GOP's pictures written.
    A folder with a display_format.json (pmctf_scale: coded at another size than its source's) has every picture resampled
    to that display size on the device before it is written, .yuv and PNGs alike; the hashes are those of the coded-size
    pictures and are checked before.  pmctf_scale.decode_sequence_checked(..., coded_size_output=True) writes the
    coded-size pictures instead.
    A folder with a source_format.json (pmctf_chroma: a .y4m source, or one that is not 4:2:0) is then written in the chroma
    format of its source, converted on the device, and a yuv_out ending in .y4m as a Y4M file (header, FRAME markers);
    pmctf_chroma.decode_sequence_checked(..., coded_format_output=True) writes the coded 4:2:0 pictures.  PNGs and hashes
    are those of the 4:2:0 pictures either way.
    Returns decode_sequence's dict: "verified" counts the pictures checked, "hash_mismatches" lists {"gop", "folder",
    "frame", "plane", "decoded", "recorded"}; "frames" holds the written sizes."""
    return decode_sequence_with(FullDecode(), codec, bin_folder, yuv_out, device, png_out, verify)


class PlainSink:
    """The picture sink of a folder with no display_format.json and no source_format.json in force and no .y4m to write: the
    pictures as they were coded, through frames_to_u8 / frames_to_u16 and frames_to_rgb8, and nothing else of the device.
    pmctf_scale.DisplaySize and pmctf_chroma.OutputFormat are the other two sinks (picture_sink)."""
    stream_header = frame_marker = b""

    def __init__(self, height, width, bitdepth):
        self.shape, self.bitdepth = (height, width), bitdepth             # shape: of every written picture

    def pictures(self, frames_rec):
        return frames_to_samples(frames_rec, *self.shape, self.bitdepth)

    def frames(self, frames_rec):
        """the packed pictures on the device, for a sink that goes on from there (pmctf_layout.PackedSink)"""
        import pmctf_scale
        return [pmctf_scale.pack_frame(rec[0], rec[1], *self.shape, self.bitdepth) for rec in frames_rec]

    def rgb8(self, frames_rec):
        return frames_to_rgb8(frames_rec, *self.shape)


def picture_sink(bin_folder, yuv_out, width, height, device, bitdepth, coded_size_output=False, coded_format_output=False):
    """-> what turns the reconstructed pictures of a decode of bin_folder into bytes, built once per decode:
    .stream_header (written once), .frame_marker (before every picture), .pictures(frames) -> [(Y, Cb, Cr)] integer arrays,
    .rgb8(frames) -> [(h, w, 3) uint8 arrays] for the PNGs, .shape: (height, width) of what is written.
    display_format.json and source_format.json are validated even where coded_size_output / coded_format_output switch
    their effect off."""
    import pmctf_chroma
    import pmctf_scale
    display = pmctf_scale.display_size(bin_folder, width, height, device, bitdepth, coded_size_output)
    fmt = pmctf_chroma.output_format(bin_folder, yuv_out, width, height, display, device, bitdepth, coded_format_output)
    if fmt is not None:
        return fmt
    return display if display is not None else PlainSink(height, width, bitdepth)


class FullDecode:
    """What decode_sequence_with is parameterised by, here for every picture of the sequence (decode_sequence_checked):
    how one GOP is decoded and which recorded hashes apply to its pictures.  pmctf_layers.LayerDecode is the one for a
    temporal level."""
    hash_level = None                                                     # None: nothing to check the pictures against
    keeps = False                                                         # True: `taken` is the output, nothing need be written

    def refuse(self, verify):
        """refusals of its own, raised between that of `verify` and that of having nothing to write"""

    def check_folder(self, bin_folder):
        """refusals that need the folder, raised once its header is read"""

    def picture_size(self, bin_folder, h, w, coded_size_output, coded_format_output):
        """-> (height, width) of the decoded pictures, the coded size here; a mode that decodes at another size
        (pmctf_layers.LayerDecode at a spatial level) raises its refusals that need the size, before the codec is looked at"""
        return h, w

    def open(self, bin_folder, header, gops, verify):
        if verify is not False and (verify != "auto" or os.path.exists(os.path.join(bin_folder, PICTURE_HASHES))):
            full = read_picture_hashes(bin_folder, header["frame_num"])
            self.frames, self.hash_level = full["frames"], full["level"]

    def decode_gop(self, codec, folder, size, h, w, q_index, psize, me_downsample, ll_order):
        """-> (the GOP's pictures, their offsets within the GOP, the bytes read or None where they are not counted); no
        pictures and no offsets for a GOP the mode leaves out (pmctf_access.FrameDecode), whose folder is then not touched"""
        out = decode_gop_files(codec, folder, size, h, w, q_index, psize=psize, me_downsample=me_downsample, ll_order=ll_order)
        return out["frames"], range(size), None

    def recorded(self, first, size, at, n):
        """-> the records of the n pictures decoded from the GOP of `size` pictures at `first`, `at` pictures written so far"""
        return self.frames[first:first + size]

    def taken(self, source, frames, bitdepth):
        """every GOP's pictures (padded, on the device) with their source indices, once verified and before they are written"""

    def result(self, times, nbytes):
        return {}


def decode_sequence_with(mode, codec, bin_folder, yuv_out, device=None, png_out=None, verify="auto", *,
                         coded_size_output=False, coded_format_output=False, output_layout=None):
    """The one sequence decoder: decode_sequence_checked (mode: a FullDecode) and pmctf_layers.decode_sequence_layer (a
    LayerDecode), and under the output flags pmctf_scale's and pmctf_chroma's forms of both; with an output_layout
    (pmctf_layout) the pictures of the sink are packed on the device before they are written.  A FullDecode and a LayerDecode
    of level 0 without motion_fill decode the same pictures in the same order, so they write the same bytes.  A
    pmctf_access.FrameDecode decodes chosen pictures: a GOP for which the mode returns no pictures is passed over."""
    import contextlib
    import time
    if not any(verify is v for v in (True, False)) and verify not in ("auto", "report"):
        raise ValueError(f"verify is 'auto', True, False or 'report' (got {verify!r})")
    mode.refuse(verify)
    if yuv_out is None and png_out is None and not mode.keeps:
        raise ValueError("nothing to write: give yuv_out, png_out or both")
    header, gops = sequence_layout(bin_folder)
    mode.check_folder(bin_folder)
    ph, pw = mode.picture_size(bin_folder, header["height"], header["width"], coded_size_output, coded_format_output)
    bitdepth = read_picture_format(bin_folder)
    if bitdepth > 8 and png_out is not None:
        raise ValueError(f"{os.path.join(bin_folder, PICTURE_FORMAT)}: the pictures have {bitdepth} bits, png_out writes "
                         f"8-bit PNGs; decode to a .yuv")
    check_sequence_header(header, codec_header_fields(codec))
    dev = codec.engine().dev
    if device is not None and torch.device(device).type != dev.type:
        raise ValueError(f"the codec lives on {dev}, not on {device}")
    mode.open(bin_folder, header, gops, verify)
    h, w = header["height"], header["width"]
    sink = picture_sink(bin_folder, yuv_out, w, h, dev, bitdepth, coded_size_output, coded_format_output)
    if (ph, pw) != (h, w):                                                # the coded form at another size: validated above
        import pmctf_chroma
        sink = pmctf_chroma.output_format(bin_folder, yuv_out, pw, ph, None, dev, bitdepth, coded_format_output) \
            or PlainSink(ph, pw, bitdepth)
    if output_layout is not None:
        import pmctf_layout
        sink = pmctf_layout.PackedSink(sink, output_layout, yuv_out, bitdepth)
    q_indexes = gop_q_indexes(header, len(gops))
    shapes, seconds, mismatches, times = [], [], [], []
    verified = nbytes = 0
    with (open(yuv_out, "wb") if yuv_out is not None else contextlib.nullcontext()) as f:
        if f is not None:
            f.write(sink.stream_header)
        for k, (first, size, psize, me_downsample) in enumerate(gops):
            t0 = time.time()
            folder = os.path.join(bin_folder, gop_folder(k))
            frames, offsets, nread = mode.decode_gop(codec, folder, size, h, w, q_indexes[k], psize, me_downsample,
                                                     header["ll_order"])
            source = [first + t for t in offsets]                         # the source index of every decoded picture
            if not source:                                                # a GOP the mode left out
                seconds.append(time.time() - t0)
                continue
            if mode.hash_level is not None:
                got = picture_hashes(frames, ph, pw, mode.hash_level, bitdepth)
                bad = []
                for t, a, b in zip(source, got, mode.recorded(first, size, len(times), len(source))):
                    bad += compare_hash_records([a], [b], t, gop=k, folder=folder)   # per source frame
                if bad and verify != "report":
                    raise PictureHashMismatch(bad[0])
                mismatches += bad
                verified += len(source)
            mode.taken(source, frames, bitdepth)
            if f is not None:
                for planes in sink.pictures(frames):
                    f.write(sink.frame_marker)
                    for p in planes:
                        f.write(p.tobytes(order="C"))
            if png_out is not None:
                for t, rgb in zip(source, sink.rgb8(frames)):             # PNGs are named by source index
                    write_pngs(png_out, t, [rgb])
            times += source
            nbytes += nread or 0
            shapes += [sink.shape] * len(source)
            seconds.append(time.time() - t0)
    return dict({"header": header, "frames": shapes, "seconds": seconds, "verified": verified, "hash_mismatches": mismatches,
                 "bitdepth": bitdepth}, **mode.result(times, nbytes))
