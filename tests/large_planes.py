"""Large-plane census: every kernel that takes an NHWC or N-stacked operand, on the smallest plane that puts one operand on
the named side of a 2^31 / 2^32 boundary.  The other censuses (conv_census.py, valu_conv_census.py, ew_census.py) hold
every kernel to the oracle on planes of a few thousand pixels; here the same kernels meet byte offsets inside an image at and
past 2^31 and 2^32, the size guards of the dispatchers from both sides, and the batch axis past 2^32.  Plain data and helpers:
no GPU import.  test_large_planes_cpu.py holds this table against the source text, test_gpu_large_planes.py runs the rows.

A row: (id, entry, geometry, rule, act, residual adds, knobs, expected launch key, boundary, side)
  entry      conv        ops.Conv2d on the matrix-core dispatcher (csrc/conv_mfma.hip)
             conv_geom   pmctf_conv2d_nhwc_geom_opts_f32: stride 2 with the per-class padding (pad = top = left, none below / right)
             smallcin    pmctf_conv2d_smallcin_f32;  fewcout  pmctf_conv2d_fewcout_f32;  dw  pmctf_dwconv2d_nhwc_f32
             nearest_up2 / pixel_shuffle2 / ffn3_mix / lstm_gates   the NHWC element kernels of csrc/ew_ops.hip
             ew          pmctf_ew_f32 with EW_MULS (a unary op: two operands per row, not three)
             fourstep_quant / fourstep_dequant   the four-step coder's element kernels (ew_ops.hip, decode_ops.hip): the
                         geometry is that of the NHWC PARAMETER tensor (N, H, W, 2) = (scale, mean), the operand that
                         crosses; the ninth field says whether it is full size ("full") or holds the class positions
                         only ("psub": the planes are 2H x 2W, as for nearest_up2); parity class 0, which writes every
                         element of every output
  geometry   (N, Cin, H, W, Cout, K, stride, pad) of the INPUT; the element kernels carry their output channels in Cout and
             K = 1, stride = 1, pad = 0 (nearest_up2 / pixel_shuffle2 write 2H x 2W); ew rows: Cin = Cout = C and a view name
  expected   conv / conv_geom: [(expression, MT, NT, TW16), ...] as conv_census.parse_launch gives them; the others: the launch
             expression of pmctf_valu_conv_last_launch / pmctf_ew_last_launch, None where the entry leaves no record
  boundary   (operand, 2^31 or 2^32, unit): operand "in" / "out" = bytes (or elements) of ONE image of the input / output,
             "in_batch" / "out_batch" = of the whole N-stacked tensor
  side       "under" / "over": where the operand lies; an "under" plane ends within one row pitch of the boundary.  The
             under rows of the 2^32 guards still cross 2^31 inside the image.
The widths are ragged (4001, 4003: no multiple of a 16- or 32-pixel tile), so the last tile of every row is partial.
A plane is the smallest that crosses: FLOPs = pixels x Cin x Cout x taps, pixels x Cin is fixed by the boundary, so the wide
input (112 channels where the kernel takes it) with few pixels and few couts is the cheapest and keeps the output small.
"""
import zlib

import numpy as np

G31, G32 = 1 << 31, 1 << 32
SENT = 0x5A5A5A5A           # as ew_census.SENT
PAD = 64                    # sentinel words before and after every output
MEMORY_CAP = 40 << 30       # no row may need more device memory than this
WIN_H, WIN_W = 16, 96       # largest output window handed to the oracle
N_RANDOM = 8

WAVE = {"NT": 4, "MSPLIT_PX": 0}
PIPE = {"NT": 1, "MSPLIT_PX": 0}

# planes next to 2^32 bytes of input per image: (under H, over H, W) by Cin
#   112: 2396 x 4001 x 448 B = 2^32 - 261 888, a row is 1 792 448 B;   64: 4191 x 4003 x 256 B = 2^32 - 164 608, row 1 024 768
#    32: 8382 x 4003 x 128 B = 2^32 - 164 608, row 512 384;            even sizes for stride 2: 2394 / 2396 x 4004 x 448 B
P112, P64, P32, P112E = (2396, 2397, 4001), (4191, 4192, 4003), (8382, 8383, 4003), (2394, 2396, 4004)


def _pair(rid, cin, cout, k, s, pad, rule, act, nres, knobs, under, over, plane, entry="conv"):
    hu, ho, w = plane
    return [(rid + "__under", entry, (1, cin, hu, w, cout, k, s, pad), rule, act, nres, knobs, under, ("in", G32, "bytes"), "under"),
            (rid + "__over", entry, (1, cin, ho, w, cout, k, s, pad), rule, act, nres, knobs, over, ("in", G32, "bytes"), "over")]


ROWS = []
# ---- (a) the six guards of conv_mfma.hip launch<>: `(size_t)a.H * a.W * a.Cin * sizeof(float) < (1ull << 32)` ---------------
# site "k33 wave" (chain, 8x32 tiles)
ROWS += _pair("wave33_mt7", 112, 100, 3, 1, 1, 0, 2, 1, WAVE, [("conv3x3s1_wave_kernel<MT, 2>", 7, 4, 2)],
              [("conv_mfma_wave_kernel<MT, 7>", 7, 4, 2)], P112)
ROWS += _pair("wave33_mt4", 112, 56, 3, 1, 1, 0, 1, 0, WAVE, [("conv3x3s1_wave_kernel<MT, 1>", 4, 4, 2)],
              [("conv_mfma_wave_kernel<MT, 7, 1>", 4, 4, 2)], P112)
ROWS += _pair("wave33_mt2", 112, 24, 3, 1, 1, 0, 2, 2, WAVE, [("conv3x3s1_wave_kernel<MT, 1>", 2, 4, 2)],
              [("conv_mfma_wave_kernel<MT, 7, 1>", 2, 4, 2)], P112)
ROWS += _pair("wave33_mt1", 112, 8, 3, 1, 1, 0, 0, 0, WAVE, [("conv3x3s1_wave_kernel<MT, 1>", 1, 4, 2)],
              [("conv_mfma_wave_kernel<MT, 7, 1>", 1, 4, 2)], P112)
# sites "k33 pipe, stride 1" and "k33 pipe, stride 2" (chain, 4x16 tiles); the stride-2 one also through the geom entry
ROWS += _pair("pipe33_mt7", 112, 100, 3, 1, 1, 0, 2, 1, PIPE, [("conv3x3s1_pipe_kernel<MT>", 7, 1, 1)],
              [("conv_mfma_pipe_kernel<MT, NT, TW16, 6>", 7, 1, 1)], P112)
ROWS += _pair("pipe33_s2_mt7", 112, 100, 3, 2, 1, 0, 1, 0, PIPE, [("conv3x3s1_pipe_kernel<MT, 2>", 7, 1, 1)],
              [("conv_mfma_pipe_kernel<MT, NT, TW16, 6>", 7, 1, 1)], P112)
ROWS += _pair("pipe33_s2_class3_mt7", 112, 100, 3, 2, 0, 0, 2, 1, PIPE, [("conv3x3s1_pipe_kernel<MT, 2>", 7, 1, 1)],
              [("conv_mfma_pipe_kernel<MT, NT, TW16, 6>", 7, 1, 1)], P112E, entry="conv_geom")
ROWS += _pair("pipe33_s2_class0_mt7", 112, 100, 3, 2, 1, 0, 0, 0, PIPE, [("conv3x3s1_pipe_kernel<MT, 2>", 7, 1, 1)],
              [("conv_mfma_pipe_kernel<MT, NT, TW16, 6>", 7, 1, 1)], P112E, entry="conv_geom")
# site "k77" (chain): SpyNet's 64 -> 32 and 32 -> 64
ROWS += _pair("k77_64_32", 64, 32, 7, 1, 3, 0, 1, 0, WAVE, [("conv7x7s1_pipe_kernel<MT, NT>", 2, 4, 2)],
              [("conv_mfma_kernel<MT, NT, TW16>", 2, 4, 2)], P64)
ROWS += _pair("k77_32_64", 32, 64, 7, 1, 3, 0, 2, 0, WAVE, [("conv7x7s1_pipe_kernel<MT, NT>", 4, 4, 2)],
              [("conv_mfma_kernel<MT, NT, TW16>", 4, 4, 2)], P32)
# site "plain_blocks" (rule blocks, 3x3): tile-outer, wave and pipelined forms, both strides
ROWS += _pair("blocks_tileouter_mt7", 112, 100, 3, 1, 1, 1, 2, 1, WAVE, [("conv3x3s1_blocks_tileouter_kernel", 7, 4, 2)],
              [("conv_mfma_bsum_kernel<MT, NT, TW16>", 7, 2, 1)], P112)
ROWS += _pair("blocks_wave_mt4", 112, 56, 3, 1, 1, 1, 1, 0, WAVE, [("conv3x3s1_wave_kernel<MT, NB, true>", 4, 4, 2)],
              [("conv_mfma_bsum_kernel<MT, NT, TW16>", 4, 4, 2)], P112)
ROWS += _pair("blocks_pipe_mt7", 112, 100, 3, 1, 1, 1, 0, 0, PIPE, [("conv3x3s1_pipe_kernel<MT, 1, true>", 7, 1, 1)],
              [("conv_mfma_bsum_kernel<MT, NT, TW16>", 7, 1, 1)], P112)
ROWS += _pair("blocks_pipe_s2_mt7", 112, 100, 3, 2, 1, 1, 2, 1, PIPE, [("conv3x3s1_pipe_kernel<MT, 2, true>", 7, 1, 1)],
              [("conv_mfma_bsum_kernel<MT, NT, TW16>", 7, 1, 1)], P112)
# site "k77 blocks"
ROWS += _pair("k77_blocks_64_32", 64, 32, 7, 1, 3, 1, 2, 0, WAVE, [("conv7x7s1_pipe_kernel<MT, NT, true>", 2, 4, 2)],
              [("conv_mfma_bsum_kernel<MT, NT, TW16>", 2, 4, 2)], P64)

# ---- (b) kernels without a size guard: one operand crosses 2^32 bytes inside an image ------------------------------------------
# (conv_mfma_wave_kernel<MT, 7>, conv_mfma_pipe_kernel<.., 6>, conv_mfma_bsum_kernel: the "over" rows above)
IN32, OUT32 = ("in", G32, "bytes"), ("out", G32, "bytes")
ROWS += [
    ("generic_tanh", "conv", (1, 112, 2397, 4001, 8, 3, 1, 1), 0, 3, 0, PIPE, [("conv_mfma_kernel<MT, NT, TW16>", 1, 1, 1)], IN32, "over"),
    ("pipegen9_s2", "conv", (1, 112, 2397, 4001, 100, 3, 2, 1), 0, 2, 0, {"NT": 2, "MSPLIT_PX": 0},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 9>", 7, 2, 1)], IN32, "over"),
    # 1x1 GEMM 64 -> 256: the output crosses while the input (a quarter of it) does not
    ("gemm1x1_64_256", "conv", (1, 64, 2051, 2047, 256, 1, 1, 0), 0, 2, 1, {}, [("conv1x1_kernel<MTW, NT>", 4, 4, 1)], OUT32, "over"),
    ("c16_band", "conv", (1, 16, 8192, 8200, 16, 3, 1, 1), 0, 0, 1, {"C16_OCC": 2}, [("conv16_band_kernel", 2, 1, 1)], IN32, "over"),
    ("c16_persistent", "conv", (1, 16, 8192, 8200, 16, 3, 1, 1), 1, 3, 0, {"C16_OCC": 0}, [("conv16_persistent_kernel", 1, 1, 1)], IN32, "over"),
    # vector-ALU first layers whose output crosses
    ("strip_1_112", "smallcin", (1, 1, 2397, 4001, 112, 3, 1, 1), 0, 2, 0, {}, "conv3x3_smallcin_strip_kernel<1>", OUT32, "over"),
    ("reg_2_112", "smallcin", (1, 2, 2397, 4001, 112, 1, 1, 0), 0, 1, 0, {}, "conv_smallcin_reg_kernel<1, 2>", OUT32, "over"),
    # 64 -> 1 on both sides of `(long)H * W * CI_ < 0x7fffffffL` (an element count): 8382 x 4003 x 64 = 2^31 - 82 304, a row is 256 192
    ("fewcout_64_1__under", "fewcout", (1, 64, 8382, 4003, 1, 3, 1, 1), 0, 2, 0, {}, "conv_fewcout_lds_kernel<3, 64, 1>", ("in", G31 - 1, "elements"), "under"),
    ("fewcout_64_1__over", "fewcout", (1, 64, 8383, 4003, 1, 3, 1, 1), 1, 0, 0, {}, "conv_fewcout_pix_kernel<3, 64, 1>", ("in", G31 - 1, "elements"), "over"),
    # 1 -> 1 on both sides of `(long)N * Ho * Wo < (1L << 31)` (pixels): 65530 x 32771 = 2^31 - 18; past it the generic kernel
    ("reg_1_1__under", "smallcin", (1, 1, 65530, 32771, 1, 3, 1, 1), 0, 2, 0, {}, "conv_smallcin_reg_kernel<3, 1>", ("out", G31, "elements"), "under"),
    ("reg_1_1__over", "smallcin", (1, 1, 65531, 32771, 1, 3, 1, 1), 0, 1, 0, {}, "conv_smallcin_kernel", ("out", G31, "elements"), "over"),
    # depthwise 3x3 at 112 channels: 6.7 M column threads against a grid of 16384 x 256 (the cap): every thread walks twice
    ("dw_column_112", "dw", (1, 112, 2397, 4001, 112, 3, 1, 1), 0, 0, 0, {}, "dwconv3_column_kernel<4, 8>", IN32, "over"),
    ("nearest_up2_112", "nearest_up2", (1, 112, 1199, 2001, 112, 1, 1, 0), 0, 0, 0, {}, "nearest_up2_vec4_kernel", OUT32, "over"),
    ("pixel_shuffle2_112", "pixel_shuffle2", (1, 448, 1199, 2001, 112, 1, 1, 0), 0, 0, 0, {}, "pixel_shuffle2_vec4_kernel", OUT32, "over"),
    ("ffn3_mix_112", "ffn3_mix", (1, 224, 1199, 4001, 112, 1, 1, 0), 0, 0, 0, {}, None, IN32, "over"),
    ("lstm_gates_112", "lstm_gates", (1, 112, 2397, 4001, 112, 1, 1, 0), 0, 0, 0, {}, None, IN32, "over"),
]

# four-step coder: 16390 x 32762 x 2 x 4 B of parameters = 2^32 + 784 448 (the planes have 2^29 pixels); at the class
# positions only, 32780 x 65526 planes (2^31 pixels: the plane index itself passes 2^31) over 16390 x 32763 x 2 parameters
ROWS += [
    ("fourstep_quant_full", "fourstep_quant", (1, 2, 16390, 32762, 1, 1, 1, 0, "full"), 0, 0, 0, {}, None, IN32, "over"),
    ("fourstep_dequant_full", "fourstep_dequant", (1, 2, 16390, 32762, 1, 1, 1, 0, "full"), 0, 0, 0, {}, None, IN32, "over"),
    ("fourstep_quant_psub", "fourstep_quant", (1, 2, 16390, 32763, 1, 1, 1, 0, "psub"), 0, 0, 0, {}, None, IN32, "over"),
    ("fourstep_dequant_psub", "fourstep_dequant", (1, 2, 16390, 32763, 1, 1, 1, 0, "psub"), 0, 0, 0, {}, None, IN32, "over"),
]
FOURSTEP = ("fourstep_quant", "fourstep_dequant")
FOURSTEP_K = 0

# ---- (c) the batch axis: five images of 936 MB, the tensor crosses 2^32 ---------------------------------------------------------
INB = ("in_batch", G32, "bytes")
ROWS += [
    ("batch_wave33", "conv", (5, 112, 1088, 1920, 8, 3, 1, 1), 0, 2, 0, WAVE, [("conv3x3s1_wave_kernel<MT, 1>", 1, 4, 2)], INB, "over"),
    ("batch_pipe33", "conv", (5, 112, 1088, 1920, 8, 3, 1, 1), 0, 1, 0, PIPE, [("conv3x3s1_pipe_kernel<MT>", 1, 1, 1)], INB, "over"),
    ("batch_gemm1x1", "conv", (5, 112, 1088, 1920, 112, 1, 1, 0), 0, 2, 0, {}, [("conv1x1_kernel<MTW, NT>", 2, 4, 1)], INB, "over"),
    ("batch_dw", "dw", (5, 112, 1088, 1920, 112, 3, 1, 1), 0, 0, 0, {}, "dwconv3_column_kernel<4, 8>", INB, "over"),
    ("batch_ew_flat", "ew", (5, 112, 1088, 1920, 112, 1, 1, 0, "dense_nhwc"), 0, 0, 0, {}, "ew_flat_kernel<true>", INB, "over"),
]

# ---- (d) elementwise: `const bool small = total < (1L << 31)` from both sides, and the flat form past it --------------------------
# views: dense_nhwc  both dense channels-last (the flat form)        slice_nhwc  a = the first C channels of a C + 4 tensor
#        window      planar, a = a column window of rows of W + 1    (C % 4 == 0: four-per-thread form; else the generic one)
EL31 = ("out", G31, "elements")
ROWS += [
    ("ew_flat_long", "ew", (1, 112, 4794, 4000, 112, 1, 1, 0, "dense_nhwc"), 0, 0, 0, {}, "ew_flat_kernel<true>", EL31, "over"),
    ("ew_c4__under", "ew", (1, 112, 4793, 4000, 112, 1, 1, 0, "slice_nhwc"), 0, 0, 0, {}, "ew_c4_kernel<int> channels", EL31, "under"),
    ("ew_c4__over", "ew", (1, 112, 4794, 4000, 112, 1, 1, 0, "slice_nhwc"), 0, 0, 0, {}, "ew_c4_kernel<long> channels", EL31, "over"),
    ("ew_cfast__under", "ew", (1, 110, 4880, 4000, 110, 1, 1, 0, "slice_nhwc"), 0, 0, 0, {}, "ew_kernel<true, int>", EL31, "under"),
    ("ew_cfast__over", "ew", (1, 110, 4881, 4000, 110, 1, 1, 0, "slice_nhwc"), 0, 0, 0, {}, "ew_kernel<true, long>", EL31, "over"),
    ("ew_planar__under", "ew", (1, 112, 4792, 4001, 112, 1, 1, 0, "window"), 0, 0, 0, {}, "ew_kernel<false, int>", EL31, "under"),
    ("ew_planar__over", "ew", (1, 112, 4793, 4001, 112, 1, 1, 0, "window"), 0, 0, 0, {}, "ew_kernel<false, long>", EL31, "over"),
]

EW_LONG_FORMS = ("ew_c4_kernel<long>", "ew_kernel<true, long>", "ew_kernel<false, long>")
EW_ALPHA = 0.37             # EW_MULS: out = a * alpha, one rounding

# ---- guards: every size guard of the dispatchers, with the rows on both of its sides or the reason there are none -----------------
# key: (source file, the guard's text as the source words it, whitespace collapsed); value: ("rows", [under id, over id]) per
# occurrence in source order, or ("exempt", reason)
SIX = "(size_t)a.H * a.W * a.Cin * sizeof(float) < (1ull << 32)"
GUARDS = {
    ("conv_mfma.hip", SIX): [("rows", "k77_blocks_64_32"), ("rows", "blocks_tileouter_mt7", "blocks_wave_mt4", "blocks_pipe_mt7", "blocks_pipe_s2_mt7"),
                             ("rows", "wave33_mt7", "wave33_mt4", "wave33_mt2", "wave33_mt1"), ("rows", "k77_64_32", "k77_32_64"),
                             ("rows", "pipe33_mt7"), ("rows", "pipe33_s2_mt7", "pipe33_s2_class3_mt7", "pipe33_s2_class0_mt7")],
    ("conv_mfma.hip", "tiles < (1L << 30)"): [("exempt", "2^30 tiles of 4x16 pixels at 16 channels are 4 TiB of input")],
    ("conv_mfma.hip", "gx > 0x7fffffffL"): [("refusal", "gemm1x1_grid")],       # 4 TiB of input: refused, never launched
    ("basic_ops.hip", "(long)N * Ho * Wo < (1L << 31)"): [("rows", "reg_1_1")],
    ("basic_ops.hip", "tiles <= 0x7fffffffL"): [("exempt", "2^31 tiles of 8x32 pixels at 16 channels are 32 TiB of input")],
    ("basic_ops.hip", "(long)H * W * CI_ < 0x7fffffffL"): [("rows", "fewcout_64_1")],
    ("ew_ops.hip", "total < (1L << 31)"): [("rows", "ew_c4", "ew_cfast", "ew_planar")],
    ("picture_ops.hip", "(long)N * Hp * Wp > 0x7fffffffL"): [("refusal", "planes_to_u8"), ("refusal", "planes_to_u16")],
    ("pu_fused.hip", "blocks > 0x7fffffffL"): [("refusal", "pu_fused")],
}

# rows that would pass the memory cap: (name, bytes, why)
EXEMPT_ROWS = []            # every row the census was asked for fits the cap and is built


# the host-side size refusals: name -> (entry point, arguments; "P" = a made-up non-null pointer, never dereferenced: the
# entry must return PMCTF_EINVAL (-1) before it touches memory or launches).  test_product_cpu.py makes exactly these calls.
REFUSALS = {
    "planes_to_u8": ("pmctf_planes_to_u8", ("P", "P", 2, 32768, 32768, 8, 8, None)),                  # N * Hp * Wp = 2^31
    "planes_to_u16": ("pmctf_planes_to_u16", ("P", "P", 8, 16384, 16384, 8, 8, 10, None)),            # the same at its side limit
    "pu_fused": ("pmctf_predict_update_fused_f32", ("P",) * 11 + (2048, 8192, 32768, 0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0, 0, None)),  # 2^31 blocks
    # 2^39 pixels in blocks of 64 pass 2^31 - 1 workgroups
    "gemm1x1_grid": ("pmctf_conv2d_nhwc_f32", ("P", "P", "P", None, None, "P", 2048, 16384, 16384, 16, 112, 1, 1, 1, 0, 0, 0, 0.0, None)),
}


def upsampled(r):
    """2 where the output has twice the input's rows and columns"""
    return 2 if r[1] in ("nearest_up2", "pixel_shuffle2") or (r[1] in FOURSTEP and r[2][8] == "psub") else 1


def row(rid):
    return next(r for r in ROWS if r[0] == rid)


def seed(rid):
    return zlib.crc32(rid.encode())


# ---- sizes ------------------------------------------------------------------------------------------------------------------------
def out_dims(r):
    """(Ho, Wo, Cout) of one output image"""
    rid, entry, g = r[0], r[1], r[2]
    N, Cin, H, W, Cout, K, S, pad = g[:8]
    if upsampled(r) == 2:
        return 2 * H, 2 * W, Cout
    if entry == "conv_geom":
        return H // 2, W // 2, Cout
    return (H + 2 * pad - K) // S + 1, (W + 2 * pad - K) // S + 1, Cout


def in_image_elems(r):
    N, Cin, H, W = r[2][:4]
    return H * W * Cin


def out_image_elems(r):
    Ho, Wo, Co = out_dims(r)
    return Ho * Wo * Co


def boundary_value(r):
    """the quantity the row's boundary speaks of, and the pitch of one image row of that operand, in the boundary's unit"""
    (operand, limit, unit), g = r[8], r[2]
    N, Cin, H, W = g[:4]
    Ho, Wo, Co = out_dims(r)
    per = 4 if unit == "bytes" else 1
    if operand == "in":
        return H * W * Cin * per, W * Cin * per
    if operand == "out":
        return Ho * Wo * Co * per, Wo * Co * per
    if operand == "in_batch":
        return N * H * W * Cin * per, W * Cin * per
    if operand == "out_batch":
        return N * Ho * Wo * Co * per, Wo * Co * per
    raise KeyError(operand)


def ew_views(r):
    """ew rows: ((a buffer elements, a offset, a strides), (out buffer elements, out strides)) over logical (N, C, H, W)"""
    N, C, H, W = r[2][:4]
    kind = r[2][8]
    if kind == "dense_nhwc":
        st = (H * W * C, 1, W * C, C)
        return (N * H * W * C, 0, st), (N * H * W * C, st)
    if kind == "slice_nhwc":
        ct = C + 4 if C % 4 == 0 else C + 2
        off = 0 if C % 4 == 0 else 1
        return (N * H * W * ct, off, (H * W * ct, 1, W * ct, ct)), (N * H * W * C, (H * W * C, 1, W * C, C))
    if kind == "window":
        return (N * C * H * (W + 1), 0, (C * H * (W + 1), H * (W + 1), W + 1, 1)), (N * C * H * W, (C * H * W, H * W, W, 1))
    raise KeyError(kind)


def need_bytes(r):
    """device memory the GPU test needs for the row: operands, residuals, the guarded output, one band of each again, and the
    temporaries of the chunked comparisons (1 GiB)"""
    N = r[2][0]
    if r[1] == "ew":
        (na, _, _), (no, _) = ew_views(r)
        return 4 * (na + no + 2 * PAD) + (3 << 30)
    xin, out = 4 * N * in_image_elems(r), 4 * N * out_image_elems(r)
    if r[1] in FOURSTEP:                                           # parameters, x or symbols, so_far, sym, idx; a band of each
        return xin + 3 * out + min(xin, G31) + 3 * min(out, G31) + (1 << 30)
    extra = 2 * out if r[1] == "lstm_gates" else 0                  # the cell input and the second output
    band = min(xin, G31) + (1 + r[5]) * min(out, G31)
    return xin + (1 + r[5]) * out + extra + band + min(extra, 2 * G31) + (1 << 30)


# ---- windows ----------------------------------------------------------------------------------------------------------------------
def _clip_origin(c, size, extent):
    """origin of a window of `size` around c inside [0, extent): odd (no tile starts on an odd pixel) unless an edge forces 0"""
    o = max(0, min(c - size // 2, extent - size))
    if o > 0 and o % 2 == 0 and o + size < extent:
        o += 1
    return o


def windows(r):
    """[(what, n, oy0, ox0, h, w), ...]: output windows of at most WIN_H x WIN_W — the four corners of the first and of the
    last image, the pixels whose input / output byte offset is the first >= 2^31 and every multiple of 2^32 inside the
    tensor, the last pixel, and N_RANDOM seeded ones.  The byte offsets are those of dense NHWC operands; for the strided
    and planar views of the ew rows they name pixels spread over the tensor, no more"""
    N, Cin, H, W, Cout, K, S, pad = r[2][:8]
    Ho, Wo, Co = out_dims(r)
    h, w = min(WIN_H, Ho), min(WIN_W, Wo)
    up = upsampled(r)
    out = []
    for n in sorted({0, N - 1}):
        for cy, cx, name in ((0, 0, "top-left"), (0, Wo - w, "top-right"), (Ho - h, 0, "bottom-left"), (Ho - h, Wo - w, "bottom-right")):
            out.append((f"corner {name} of image {n}", n, cy, cx, h, w))

    def around(what, n, oy, ox):
        out.append((what, n, _clip_origin(oy, h, Ho), _clip_origin(ox, w, Wo), h, w))

    def marks(total):
        return [G31] + [m for m in range(G32, total, G32)]

    in_px, out_px = 4 * Cin, 4 * Co
    for b in marks(4 * N * H * W * Cin):
        if b < 4 * N * H * W * Cin:
            p = b // in_px
            n, rem = divmod(p, H * W)
            around(f"input byte {b:#x}", n, min((rem // W) * up // S, Ho - 1), min((rem % W) * up // S, Wo - 1))
    for b in marks(4 * N * Ho * Wo * Co):
        if b < 4 * N * Ho * Wo * Co:
            p = b // out_px
            n, rem = divmod(p, Ho * Wo)
            around(f"output byte {b:#x}", n, rem // Wo, rem % Wo)
    around("last pixel", N - 1, Ho - 1, Wo - 1)
    g = np.random.default_rng(seed(r[0]))
    for i in range(N_RANDOM):
        around(f"random {i}", int(g.integers(N)), int(g.integers(Ho)), int(g.integers(Wo)))
    return out


def even_window(win):
    """the smallest window with even origin and even size that holds an output window: (ey0, ex0, eh, ew).  The four-step
    kernels' parity class is that of the pixel's coordinates, and the class-position parameters map two pixels to one"""
    what, n, oy0, ox0, h, w = win
    ey0, ex0 = oy0 - (oy0 & 1), ox0 - (ox0 & 1)
    return ey0, ex0, (oy0 + h + 1 - ey0) // 2 * 2, (ox0 + w + 1 - ex0) // 2 * 2


def input_window(r, win):
    """(iy0, ix0, ih, iw) of the input a window's outputs read, in image coordinates: may start before 0 and end past H / W
    (the layer's zero padding; for dw a halo clipped to the image, see window_reference)"""
    what, n, oy0, ox0, h, w = win
    N, Cin, H, W, Cout, K, S, pad = r[2][:8]
    if r[1] in FOURSTEP:
        ey0, ex0, eh, ew = even_window(win)
        u = upsampled(r)
        return ey0 // u, ex0 // u, eh // u, ew // u
    if r[1] in ("nearest_up2", "pixel_shuffle2"):
        iy0, ix0 = oy0 // 2, ox0 // 2
        return iy0, ix0, (oy0 + h - 1) // 2 - iy0 + 1, (ox0 + w - 1) // 2 - ix0 + 1
    if r[1] == "dw":
        iy0, ix0 = max(0, oy0 - 1), max(0, ox0 - 1)
        return iy0, ix0, min(H, oy0 + h + 1) - iy0, min(W, ox0 + w + 1) - ix0
    return oy0 * S - pad, ox0 * S - pad, (h - 1) * S + K, (w - 1) * S + K


def weights(r):
    """(w OIHW or depthwise (C, 1, 3, 3), b) of a row, host float32, seeded from the row id; None for the element kernels"""
    N, Cin, H, W, Cout, K, S, pad = r[2][:8]
    g = np.random.default_rng(seed(r[0]) ^ 0x77)
    if r[1] in ("conv", "conv_geom", "smallcin", "fewcout"):
        scale = np.float32(0.05 if Cin >= 16 else 0.5)
        return g.standard_normal((Cout, Cin, K, K), dtype=np.float32) * scale, g.standard_normal(Cout, dtype=np.float32)
    if r[1] == "dw":
        return g.standard_normal((Cin, 1, 3, 3), dtype=np.float32) * np.float32(0.3), g.standard_normal(Cin, dtype=np.float32)
    return None, None


def _act(v, act, slope=0.2):
    from pmctf_oracle import clib
    if act == 1:
        return np.where(v < 0, np.float32(0), v)
    if act == 2:
        return np.where(v > 0, v, v * np.float32(slope)).astype(np.float32)
    if act == 3:
        return clib.tanh(v)
    if act == 4:
        return clib.sigmoid(v)
    return v


SLOPE = 0.2


def window_reference(r, win, xw, w=None, b=None, res=(), extra=None):
    """the output window's values (h, w, Cout) float32 from the oracle, given xw = the input window of input_window(r, win)
    as (ih, iw, Cin) NHWC with zeros where it lies outside the image; res: the residual windows (h, w, Cout); extra: the cell
    window of lstm_gates.  Dense convolutions run the oracle's convolution without padding on the zero-extended crop (the
    oracle multiplies a padded zero in like any other value: equal to the layer's own padding bit for bit, asserted in
    test_large_planes_cpu.py); the depthwise oracle SKIPS a tap outside the image, so its crop ends at the image's edge
    where the window touches it and carries a halo (whose outputs are dropped) where it does not.
    lstm_gates returns (hidden, cell) stacked on a leading axis."""
    from pmctf_oracle import clib
    what, n, oy0, ox0, h, wd = win
    N, Cin, H, W, Cout, K, S, pad = r[2][:8]
    entry, rule, act = r[1], r[3], r[4]
    f = np.float32
    xw = np.ascontiguousarray(xw, dtype=f)
    if entry in ("conv", "conv_geom", "smallcin", "fewcout"):
        y = clib.conv2d(np.ascontiguousarray(xw.transpose(2, 0, 1))[None], w, b, S, (0, 0), rule)[0].transpose(1, 2, 0)
        y = _act(np.ascontiguousarray(y), act, SLOPE)
        for q in res:
            y = y + q
        assert y.shape == (h, wd, Cout), (y.shape, (h, wd, Cout))
        return np.ascontiguousarray(y, dtype=f)
    if entry == "dw":
        iy0, ix0, ih, iw = input_window(r, win)
        y = clib.dwconv2d(np.ascontiguousarray(xw.transpose(2, 0, 1))[None], w, b)[0].transpose(1, 2, 0)
        return np.ascontiguousarray(y[oy0 - iy0:oy0 - iy0 + h, ox0 - ix0:ox0 - ix0 + wd], dtype=f)
    if entry == "nearest_up2":
        iy0, ix0, ih, iw = input_window(r, win)
        yy, xx = (np.arange(oy0, oy0 + h) // 2 - iy0), (np.arange(ox0, ox0 + wd) // 2 - ix0)
        return np.ascontiguousarray(xw[yy][:, xx])
    if entry == "pixel_shuffle2":
        iy0, ix0, ih, iw = input_window(r, win)
        oy, ox = np.arange(oy0, oy0 + h), np.arange(ox0, ox0 + wd)
        x5 = xw.reshape(ih, iw, Cout, 2, 2)                       # channel c * 4 + i * 2 + j
        return np.ascontiguousarray(x5[(oy // 2 - iy0)[:, None], (ox // 2 - ix0)[None, :], :, (oy & 1)[:, None], (ox & 1)[None, :]])
    if entry == "ffn3_mix":
        x1, x2 = xw[..., :Cout], xw[..., Cout:]
        return (np.where(x1 > 0, x1, x1 * f(0.1)).astype(f) + np.where(x2 > 0, x2, x2 * f(0.01)).astype(f)).astype(f)
    if entry == "lstm_gates":
        g, ct = clib.sigmoid(xw), clib.tanh(xw)
        cn = (g * extra + g * ct).astype(f)
        return np.stack([(g * clib.tanh(cn)).astype(f), cn])
    if entry == "ew":
        return (xw * f(EW_ALPHA)).astype(f)
    if entry in FOURSTEP:
        # xw: the parameter window of input_window (scale, mean); extra: the planes' window over even_window(win), float x
        # for the encoder's kernel, int16 symbols for the decoder's.  The restatement of the entropy tests
        # (entropy_restatement.py) on the even-aligned crop, where the mask of a class is the plane's own.
        import torch
        import entropy_restatement as er
        ey0, ex0, eh, ew_ = even_window(win)
        par = torch.from_numpy(np.ascontiguousarray(xw.transpose(2, 0, 1)))[:, None]            # (2, 1, ih, iw)
        if upsampled(r) == 2:
            scales, means = er.place_class(par[0:1], FOURSTEP_K, eh, ew_, 1.0), er.place_class(par[1:2], FOURSTEP_K, eh, ew_, 0.5)
        else:
            scales, means = par[0:1], par[1:2]
        cut = lambda t, shape: np.ascontiguousarray(t.reshape(shape).numpy()[oy0 - ey0:oy0 - ey0 + h, ox0 - ex0:ox0 - ex0 + wd])
        planes = torch.from_numpy(np.ascontiguousarray(extra)).reshape(1, 1, eh, ew_)
        if entry == "fourstep_quant":
            so_far, sym, idx = er.fourstep_quant(planes, scales, means, None, FOURSTEP_K)
            return cut(so_far, (eh, ew_)), cut(sym, (eh, ew_)), cut(idx, (eh, ew_))
        return (cut(er.fourstep_dequant(planes, means, None, FOURSTEP_K), (eh, ew_)),)
    raise KeyError(entry)


def crop_zero_extended(x_nhwc, iy0, ix0, ih, iw):
    """the window [iy0, iy0 + ih) x [ix0, ix0 + iw) of an (H, W, C) image, zeros outside it"""
    H, W, C = x_nhwc.shape
    out = np.zeros((ih, iw, C), np.float32)
    y0, y1, x0, x1 = max(iy0, 0), min(iy0 + ih, H), max(ix0, 0), min(ix0 + iw, W)
    if y1 > y0 and x1 > x0:
        out[y0 - iy0:y1 - iy0, x0 - ix0:x1 - ix0] = x_nhwc[y0:y1, x0:x1]
    return out


# ---- bands: the whole output again from pieces of less than 2^31 bytes ----------------------------------------------------------------
def bands(r, limit=G31 - (1 << 20)):
    """[(n, o0, o1, i0, i1), ...]: output rows [o0, o1) of image n from input rows [i0, i1) (clipped to the image), every
    piece's input and output below `limit` bytes; i0 is a multiple of the stride (and of 2 where the output is upsampled),
    so that the band's own output row k is row i0 / stride + k of the large run.  Halo rows are part of [i0, i1) and their
    outputs are not compared."""
    N, Cin, H, W, Cout, K, S, pad = r[2][:8]
    Ho, Wo, Co = out_dims(r)
    up = upsampled(r)
    halo = 1 if r[1] == "dw" else 0
    in_row, out_row = 4 * W * Cin, 4 * Wo * Co
    rows = min((limit // in_row - K - 2 * S - 2 * halo) * up // S, limit // out_row - 4)
    rows -= rows % 2
    assert rows >= 16, r[0]
    out = []
    for n in range(N):
        o0 = 0
        while o0 < Ho:
            o1 = min(Ho, o0 + rows)
            if r[1] == "dw":
                i0, i1 = max(0, o0 - 1), min(H, o1 + 1)
            elif up == 2:
                i0, i1 = o0 // 2, (o1 + 1) // 2
            else:
                i0 = max(0, o0 * S - pad)
                i0 -= i0 % S
                i1 = min(H, (o1 - 1) * S - pad + K)
            out.append((n, o0, o1, i0, i1))
            o0 = o1
    return out


def first_difference(index, r):
    """flat element index inside the output tensor -> ((n, y, x, c), byte offset)"""
    Ho, Wo, Co = out_dims(r)
    n, rem = divmod(int(index), Ho * Wo * Co)
    y, rem = divmod(rem, Wo * Co)
    x, c = divmod(rem, Co)
    return (n, y, x, c), 4 * int(index)
