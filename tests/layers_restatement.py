"""The definitions of the temporal layers written out once more, independently of pmctf_layers: the pictures
and the files of a level from the arithmetic of the indices alone (no gop_pairs, no gop_file_names), and the temporal
synthesis stopped after a stage, pair by pair with codec.inverse_MCTF.  The yardstick of tests/test_temporal_layers_cpu.py
and tests/test_gpu_temporal_layers.py."""
import os


def log2(size):
    s = 0
    while (1 << s) < size:
        s += 1
    assert (1 << s) == size, size
    return s


def times(gops, level):
    """[(gop index, source index)]: every 2^min(level, S)-th picture of every GOP, from its first"""
    out = []
    for k, (first, size) in enumerate((g[0], g[1]) for g in gops):
        step = 2 ** min(level, log2(size))
        out += [(k, t) for t in range(first, first + size, step)]
    return out


def file_names(gop, level, motion_fill=False):
    """stage s codes the high-band pictures at the odd multiples of 2^s, in rising order, stage after stage; a picture's
    files are kept when its stage is not below min(level, S), its motion file alone under motion_fill"""
    kk = min(level, log2(gop))
    names = []
    for s in range(log2(gop)):
        for i in range(2 ** s, gop, 2 ** (s + 1)):
            if s >= kk:
                names += ["%d.bin" % i, "%d_C_main.bin" % i, "%d_mv.bin" % i]
            elif motion_fill:
                names += ["%d_mv.bin" % i]
    return names + ["0_main.bin", "0_C_main.bin"]


def folder_files(gops, level, motion_fill=False):
    """the relative paths of the bitstream files of a level over a sequence"""
    return [os.path.join("gop_%05d" % k, n) for k, g in enumerate(gops) for n in file_names(g[1], level, motion_fill)]


def truncated_synthesis(codec, frames_coded, level):
    """the synthesis of one GOP from its decoded entries [[L_t / H_t, L_tc / H_tc, mv_hat]], stopped once stage min(level, S)
    is undone -> the [Y, UV] pictures at the multiples of 2^min(level, S).  The input list is left as it is."""
    fc = [list(e) for e in frames_coded]
    gop = len(fc)
    S = log2(gop)
    kk = min(level, S)
    for s in range(S - 1, kk - 1, -1):
        me = min(codec.num_me_stages - 1, s)
        for ref in range(0, gop, 2 ** (s + 1)):
            cur = ref + 2 ** s
            y_ref, y_cur = codec.inverse_MCTF(fc[ref][0], fc[cur][0], fc[cur][2], stage_idx=me)
            c_ref, c_cur = codec.inverse_MCTF(fc[ref][1], fc[cur][1], fc[cur][2], stage_idx=me, downscale=True)
            fc[ref], fc[cur] = [y_ref, c_ref, None], [y_cur, c_cur, None]
    return [fc[t][:2] for t in range(0, gop, 2 ** kk)]
