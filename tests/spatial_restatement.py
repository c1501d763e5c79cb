"""The definitions of the spatial layers written out once more, independently of pmctf_spatial and of the
engine's level-aware paths: the size rule and the symbol count from the arithmetic alone, the level-k plane of one file from
the engine's primitives (a FULL walk of the file with a HostDecoder, then the inverse lifting for the levels >= k and the
factor 2^-k), and the temporal synthesis of reduced planes with the test's own nested factor-2 reduction of the motion.
The yardstick of tests/test_spatial_layers_cpu.py and tests/test_gpu_spatial_layers.py."""
import struct

L = 4                                                                     # decomp_levels


def offered(h, w, level):
    """level 0 always; level k >= 1 when both sides are multiples of 2^(k+1) (every smaller level then is as well)"""
    return 0 <= level <= L and (level == 0 or (h % 2 ** (level + 1) == 0 and w % 2 ** (level + 1) == 0))


def top_level(h, w):
    return max(k for k in range(L + 1) if offered(h, w, k))


def size(h, w, level):
    assert offered(h, w, level)
    return h // 2 ** level, w // 2 ** level


def symbols(N, Hp, Wp, level):
    """the LL subband, then per DWT level >= `level` three subbands of (Hp / 2^(lvl+1)) x (Wp / 2^(lvl+1)) positions, each
    coded in four steps whose sizes are those of the whole subband (the positions off a step's mask are coded too)"""
    n = N * (Hp // 2 ** L) * (Wp // 2 ** L)
    for lvl in range(L - 1, level - 1, -1):
        n += 3 * 4 * N * (Hp // 2 ** (lvl + 1)) * (Wp // 2 ** (lvl + 1))
    return n


# ------------------------------------------------------------------------------------------------------------ on the GPU
def full_walk(eng, coder, data, padding, q_index, qp_scale=None, ll_order="position"):
    """one bitstream file -> (hat[lvl][sb] of the FULL walk, (q_scale, q_scale_ll), payload length): the header by hand, the
    sequential LL decode (per-file launches; plane after plane for ll_order "plane"), then pwave_walk with its defaults,
    exactly what pwave_decompress_end did before it knew levels"""
    import torch
    from pMCTF.hip.engine import HostDecoder
    height, width, N, n = struct.unpack(">IIII", data[:16])
    dec = HostDecoder(eng.tables, data[16:16 + n])
    hp = (height + padding - 1) // padding * padding
    wp = (width + padding - 1) // padding * padding
    if ll_order == "plane" and N > 1:
        ticket = eng._ll_ar_planes_one_by_one(coder, dec, N, hp >> L, wp >> L, torch.cuda.current_stream(eng.dev))
        ll_hat = eng.ll_ar_finish(ticket)
    else:
        ll_hat = eng.ll_ar_decode(coder, dec, N, hp >> L, wp >> L)
    return eng.pwave_walk(coder, ll_hat, dec), eng.q_scales(coder, q_index, qp_scale), n


def plane_of_level(eng, coder, hat, q, level):
    """the level-k plane from the full walk's subbands: dequantise, backward_lift_2d for lvl = L-1 .. k, times 2^-k"""
    from pMCTF.hip.ops import EW_DIVS, EW_MULS, ew
    q_scale, q_scale_ll = q
    rec = ew(EW_DIVS, hat[L - 1]["ll"], alpha=q_scale_ll)
    for lvl in range(L - 1, level - 1, -1):
        sbs = {sb: ew(EW_DIVS, hat[lvl][sb], alpha=q_scale) for sb in ("lh", "hl", "hh")}
        sbs["ll"] = rec
        rec = eng.backward_lift_2d(coder, sbs)
    return ew(EW_MULS, rec, alpha=2.0 ** -level)


def reduced_motion(mv, level):
    """the motion field for luma planes of spatial level k: k nested factor-2 reductions, each halving size and vectors"""
    from pMCTF.hip import ops
    for _ in range(level):
        mv = ops.bilinear_down2(mv.contiguous(), 2.0)
    return mv


def synthesis(codec, entries, level, down_to=0):
    """decode_gop's loop on reduced planes: entries [[Y_k, UV_k, mv_hat as decoded (full size) or None]] of one GOP -> the
    [Y, UV] pictures at the multiples of 2^min(down_to, S) once that stage is undone.  Luma takes the field reduced `level`
    times, chroma the same field with downscale=True.  The input list is left as it is."""
    import layers_restatement as lr
    fc = [[e[0], e[1], None if e[2] is None else reduced_motion(e[2], level)] for e in entries]
    return lr.truncated_synthesis(codec, fc, down_to)
