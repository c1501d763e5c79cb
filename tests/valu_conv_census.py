"""Census of the vector-ALU convolutions of csrc/basic_ops.hip: a row for every kernel instantiation behind
pmctf_conv2d_smallcin_f32, pmctf_conv3x3_cin1_dual_f32, pmctf_conv2d_fewcout_f32 and pmctf_dwconv2d_nhwc_f32, on the
smallest plane that is ragged against the kernel's own tile, and for every shape next to a dispatch threshold.  A row
names the kernel it must launch (what pmctf_valu_conv_last_launch reports), so a moved threshold fails on the name
instead of passing on another kernel.  Plain data and helpers: importing this module needs neither the product nor a GPU.

    test_gpu_valu_conv_census.py     runs the rows: kernel name, output as uint32 patterns between sentinels
    test_valu_conv_census_cpu.py     holds the table against the source text, the built library and the oracle

The rows that need an environment switch (read once per process) run in a child process:

    PMCTF_FEWCOUT_LDS=0 python valu_conv_census.py PMCTF_FEWCOUT_LDS out.npz
    PMCTF_DWCONV_COLUMN=0 python valu_conv_census.py PMCTF_DWCONV_COLUMN out.npz

Rows: (id, entry, geometry, rule, act, slope, residual adds, bias present, env, expected kernel, options)
    entry     "smallcin" | "fewcout" (both through ops.Conv2d), "cin1_dual" (ops.conv3x3_cin1_dual), "dwconv" (ops.DepthwiseConv2d)
    geometry  (N, Cin, H, W, Cout, KH, KW, stride, pad_h, pad_w); depthwise rows have Cin = Cout = C
    rule      0 chain, 1 blocks, 2 gemm, 3 gemv 3x3 (PMCTF_SUM_* of include/pmctf_hip.h); depthwise rows have none (0)
    act       0 none, 1 relu, 2 leaky(slope), 3 tanh, 4 sigmoid; for cin1_dual the activation of the second output
    env       None, or the name of the switch the row needs at "0"
    options   "data": "zeros" | "subnormal" | "cancel" | "cancel_rows" | "cancel_columns" (default: normal), "seed": the id whose data the row shares,
              "y2": False (cin1_dual with y2 == NULL), "c_entry": True (the C entry: the wrapper cannot express the row)

What the planes are ragged against.  Strip kernel (a lane owns 4 couts of an 8-pixel strip, Q = Cout/4 lanes per strip,
G = 64/Q strips per wave): every W ends a row in a partial strip and, where G > 1, in a wave run with idle strip groups.
Reg kernel (256/Cout pixels per pass): pixel counts that are no multiple of the pass, more than one block.  Few-cout LDS
form: 8x32 tiles (9x33 has four tiles, three of them one pixel thick).  Depthwise: 4-pixel strips, 8-row bands.  Larger
planes only for the column-walking depthwise kernel, which wants 262 144 column threads: N x ceil(H/8) x ceil(W/4) x C/4
= 2 x 3 x 128 x 342 = 262 656 on 2 x 17 x 509 with 1368 channels (bands of 8, 8 and 1 rows, the last strip one pixel
wide; 23.7 M elements, against 33.5 M for any plane of whole bands and strips); one strip less (W = 505) is below it."""
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SWITCHES = ("PMCTF_FEWCOUT_LDS", "PMCTF_DWCONV_COLUMN")         # the environment names of basic_ops.hip

STRIP = "conv3x3_smallcin_strip_kernel<%d>"
REG = "conv_smallcin_reg_kernel<%d, %d>"
GENERIC = "conv_smallcin_kernel"
PIX16 = "conv3x3_cin1_pix16_kernel"
LDS = "conv_fewcout_lds_kernel<%d, %d, %d>"
PIX = "conv_fewcout_pix_kernel<%d, %d, %d>"
COLUMN = "dwconv3_column_kernel<4, 8>"
DWSTRIP = "dwconv3_strip_kernel<4>"
DW = "dwconv_kernel"

# which rules an entry accepts, and whether it takes residual adds
RULES = {"smallcin": (0, 1, 2, 3), "cin1_dual": (0, 1), "fewcout": (0, 1), "dwconv": ()}
GENERIC_ONLY_RULES = (2, 3)                    # pmctf_conv2d_smallcin_f32 sends these to conv_smallcin_kernel whatever the shape
HAS_RESIDUALS = ("smallcin", "fewcout")

FEWCOUT = ((3, 16, 1), (3, 64, 1), (7, 16, 2))                  # (K, Cin, Cout) of pmctf_conv2d_fewcout_supported
COLUMN_PLANE = (2, 1368, 17, 509)                               # N, C, H, W: 262 656 column threads
BELOW_COLUMN_PLANE = (2, 1368, 17, 505)                         # 260 604

CENSUS = []


def _add(rid, entry, geometry, rule, act, slope, nres, bias, env, expected, **options):
    CENSUS.append((rid, entry, tuple(geometry), rule, act, slope, nres, bias, env, expected, options))


def _conv(N, Cin, H, W, Cout, K, S=1, pad=None, KW=None, pad_w=None):
    KW = K if KW is None else KW
    pad = K // 2 if pad is None else pad
    return (N, Cin, H, W, Cout, K, KW, S, pad, pad if pad_w is None else pad_w)


def _dw(N, C, H, W, K=3):
    return (N, C, H, W, C, K, K, 1, K // 2, K // 2)


_EPI = [(2, 0.2, 2), (1, 0.0, 1), (0, 0.0, 0), (3, 0.0, 1), (4, 0.0, 2)]          # (act, slope, residual adds)

# ---- strip kernel: Cin 1 - 3 x the couts whose lane mapping differs (Q lanes per strip, G strips per wave)
#   Cout 32: Q 8, G 8 (W 77: a run of 64, then 2 of 8 strips, the second 5 wide)     Cout 36: Q 9, G 7, lane 63 idle (W 69)
#   Cout 112: Q 28, G 2, 8 lanes idle (W 21: 16, then one strip of 5)   Cout 132: Q 33, G 1, 31 lanes idle (W 13)   Cout 256: Q 64 (W 11)
for _i, (_cout, _w) in enumerate(((32, 77), (36, 69), (112, 21), (132, 13), (256, 11))):
    for _cin in (1, 2, 3):
        _a, _s, _n = _EPI[(_i + _cin) % 5]
        _add(f"strip_cin{_cin}_cout{_cout}", "smallcin", _conv(2, _cin, 5, _w, _cout, 3), (_i + _cin) % 2, _a, _s, _n, True,
             None, STRIP % _cin)
_add("strip_w_below_a_strip", "smallcin", _conv(2, 2, 4, 5, 112, 3), 0, 2, 0.2, 2, True, None, STRIP % 2)
_add("strip_one_row", "smallcin", _conv(2, 1, 1, 19, 64, 3), 1, 1, 0.0, 1, True, None, STRIP % 1, data="cancel_rows")
_add("strip_one_pixel", "smallcin", _conv(3, 3, 1, 1, 32, 3), 0, 0, 0.0, 0, True, None, STRIP % 3)

# ---- the neighbours of the strip kernel's conditions that must NOT take it
_add("not_strip_cout28", "smallcin", _conv(2, 1, 5, 21, 28, 3), 1, 2, 0.2, 2, True, None, REG % (3, 1))
_add("not_strip_cout30", "smallcin", _conv(2, 2, 5, 21, 30, 3), 0, 1, 0.0, 1, True, None, REG % (3, 2))
_add("not_strip_stride2", "smallcin", _conv(2, 1, 5, 21, 64, 3, S=2), 1, 2, 0.2, 2, True, None, REG % (3, 1))
_add("not_strip_pad0", "smallcin", _conv(2, 3, 5, 21, 64, 3, pad=0), 0, 0, 0.0, 0, True, None, REG % (3, 3))
_add("not_strip_cout260", "smallcin", _conv(2, 1, 5, 21, 260, 3), 1, 2, 0.2, 2, True, None, GENERIC)
_add("not_strip_cin4", "smallcin", _conv(2, 4, 5, 21, 64, 3), 0, 1, 0.0, 1, True, None, GENERIC)
_add("not_strip_gemm", "smallcin", _conv(1, 1, 5, 21, 64, 3), 2, 2, 0.2, 2, True, None, GENERIC)
_add("not_strip_gemv", "smallcin", _conv(1, 1, 5, 21, 64, 3), 3, 0, 0.0, 0, True, None, GENERIC)

# ---- reg kernel: a thread owns one cout, 256/Cout pixels per pass; 2 x 9 x 15 = 270 pixels
_add("reg_cout1", "smallcin", _conv(2, 1, 9, 15, 1, 3), 0, 2, 0.2, 2, True, None, REG % (3, 1))           # 256 pixels per pass, two blocks
_add("reg_cout3", "smallcin", _conv(2, 2, 9, 15, 3, 3), 1, 1, 0.0, 1, True, None, REG % (3, 2))           # 85 per pass, thread 255 idle
_add("reg_cout5", "smallcin", _conv(2, 3, 9, 15, 5, 3), 0, 3, 0.0, 2, True, None, REG % (3, 3))
_add("reg_cout17", "smallcin", _conv(2, 1, 9, 15, 17, 3), 1, 4, 0.0, 0, True, None, REG % (3, 1))
_add("reg_cout200_pad0", "smallcin", _conv(2, 2, 5, 7, 200, 3, pad=0), 0, 2, 0.2, 2, True, None, REG % (3, 2))   # one pixel per pass, 56 threads idle
_add("reg_cout256_stride2", "smallcin", _conv(2, 3, 5, 7, 256, 3, S=2), 1, 2, 0.2, 2, True, None, REG % (3, 3))
_add("reg_cout5_stride2", "smallcin", _conv(2, 2, 9, 15, 5, 3, S=2), 1, 2, 0.2, 2, True, None, REG % (3, 2))
_add("reg_cout5_stride3", "smallcin", _conv(2, 1, 9, 15, 5, 3, S=3), 0, 1, 0.0, 1, True, None, REG % (3, 1))
_add("reg_cout5_stride3_cin3", "smallcin", _conv(2, 3, 9, 15, 5, 3, S=3), 1, 0, 0.0, 0, True, None, REG % (3, 3))
_add("reg_1x1_pad0", "smallcin", _conv(2, 2, 9, 15, 64, 1), 0, 2, 0.2, 2, True, None, REG % (1, 2))
_add("reg_1x1_pad1", "smallcin", _conv(2, 2, 9, 15, 12, 1, pad=1), 1, 1, 0.0, 1, True, None, REG % (1, 2), data="cancel")
_add("reg_1x1_pad1_stride2", "smallcin", _conv(2, 2, 9, 15, 12, 1, S=2, pad=1), 0, 0, 0.0, 0, True, None, REG % (1, 2))
_add("reg_plane_below_the_filter", "smallcin", _conv(2, 2, 1, 1, 5, 3), 0, 2, 0.2, 2, True, None, REG % (3, 2))

# ---- generic kernel
_add("generic_cin4", "smallcin", _conv(2, 4, 9, 15, 5, 3), 1, 2, 0.2, 2, True, None, GENERIC)
_add("generic_5x5_cin1", "smallcin", _conv(2, 1, 9, 15, 5, 5), 0, 1, 0.0, 1, True, None, GENERIC)
_add("generic_5x5_cin2", "smallcin", _conv(2, 2, 9, 15, 5, 5), 1, 2, 0.2, 2, True, None, GENERIC)
_add("generic_7x7_cin3", "smallcin", _conv(2, 3, 9, 15, 5, 7), 0, 3, 0.0, 2, True, None, GENERIC)
_add("generic_7x7_cin1_stride2", "smallcin", _conv(2, 1, 9, 15, 64, 7, S=2), 1, 0, 0.0, 0, True, None, GENERIC)
_add("generic_1x1_cin1", "smallcin", _conv(2, 1, 9, 15, 5, 1), 0, 2, 0.2, 2, True, None, GENERIC)
_add("generic_1x1_cin3", "smallcin", _conv(2, 3, 9, 15, 5, 1), 1, 4, 0.0, 1, True, None, GENERIC, data="cancel")
_add("generic_3x1_pad_1_0", "smallcin", _conv(2, 2, 9, 15, 5, 3, KW=1, pad=1, pad_w=0), 0, 2, 0.2, 2, True, None, GENERIC)
_add("generic_1x3_pad_0_1", "smallcin", _conv(2, 3, 9, 15, 5, 1, KW=3, pad=0, pad_w=1), 1, 1, 0.0, 1, True, None, GENERIC)
_add("generic_3x1_cin1_rule1", "smallcin", _conv(2, 1, 9, 15, 64, 3, KW=1, pad=1, pad_w=0), 1, 2, 0.2, 2, True, None, GENERIC, data="cancel")
_add("generic_cout300_1x1_cin2", "smallcin", _conv(2, 2, 5, 7, 300, 1), 0, 2, 0.2, 2, True, None, GENERIC)
_add("generic_cout300_3x3_cin3", "smallcin", _conv(2, 3, 5, 7, 300, 3), 1, 1, 0.0, 1, True, None, GENERIC)
_add("generic_gemm_cin2", "smallcin", _conv(1, 2, 9, 15, 5, 3), 2, 2, 0.2, 2, True, None, GENERIC, data="cancel")
_add("generic_gemm_cin3", "smallcin", _conv(1, 3, 9, 15, 64, 3), 2, 1, 0.0, 1, True, None, GENERIC)
_add("generic_gemm_cin4", "smallcin", _conv(1, 4, 9, 15, 5, 3), 2, 0, 0.0, 0, True, None, GENERIC)
_add("generic_gemv_cout1", "smallcin", _conv(1, 1, 9, 15, 1, 3), 3, 2, 0.2, 2, True, None, GENERIC, data="cancel")
_add("generic_gemv_cout16", "smallcin", _conv(1, 1, 9, 15, 16, 3), 3, 1, 0.0, 1, True, None, GENERIC)
_add("generic_gemv_cout1_stride2_pad0", "smallcin", _conv(1, 1, 9, 15, 1, 3, S=2, pad=0), 3, 0, 0.0, 0, True, None, GENERIC)
_add("generic_gemv_cout16_stride2_pad0", "smallcin", _conv(1, 1, 9, 15, 16, 3, S=2, pad=0), 3, 2, 0.2, 2, True, None, GENERIC)

# ---- 1 -> 16 with a second, activated output: lane = pixel, 256 pixels per block
for _rule in (0, 1):
    for _act in range(5):
        _add(f"dual_rule{_rule}_act{_act}", "cin1_dual", _conv(2, 1, 9, 33, 16, 3), _rule, _act, 0.0, 0, True, None, PIX16)
_add("dual_leaky_slope", "cin1_dual", _conv(2, 1, 9, 33, 16, 3), 1, 2, 0.2, 0, True, None, PIX16, c_entry=True)
_add("dual_without_y2", "cin1_dual", _conv(2, 1, 9, 33, 16, 3), 1, 3, 0.0, 0, True, None, PIX16, y2=False, c_entry=True)
_add("dual_without_y2_chain", "cin1_dual", _conv(3, 1, 5, 7, 16, 3), 0, 3, 0.0, 0, True, None, PIX16, y2=False, c_entry=True)
_add("dual_one_pixel", "cin1_dual", _conv(1, 1, 1, 1, 16, 3), 0, 3, 0.0, 0, True, None, PIX16)
_add("dual_one_row", "cin1_dual", _conv(2, 1, 1, 37, 16, 3), 1, 3, 0.0, 0, True, None, PIX16, data="cancel_rows")
_add("dual_one_column", "cin1_dual", _conv(2, 1, 37, 1, 16, 3), 1, 4, 0.0, 0, True, None, PIX16, data="cancel_columns")
_add("dual_three_images", "cin1_dual", _conv(3, 1, 9, 11, 16, 3), 1, 3, 0.0, 0, True, None, PIX16)

# ---- one or two couts: the LDS form on 8x32 tiles, and the grid-stride form behind PMCTF_FEWCOUT_LDS=0, on the same rows
for _k, _ci, _co in FEWCOUT:
    for _env, _kern in ((None, LDS), ("PMCTF_FEWCOUT_LDS", PIX)):
        _tag = f"few{_k}x{_k}_{_ci}to{_co}_{'pix' if _env else 'lds'}"
        for _rule in (0, 1):
            _seed = f"few{_k}x{_k}_{_ci}to{_co}_rule{_rule}"
            _add(f"{_tag}_rule{_rule}_9x33", "fewcout", _conv(2, _ci, 9, 33, _co, _k), _rule, 2, 0.2, 2, True, _env,
                 _kern % (_k, _ci, _co), seed=_seed + "_9x33")
            _add(f"{_tag}_rule{_rule}_7x31", "fewcout", _conv(2, _ci, 7, 31, _co, _k), _rule, 1, 0.0, 1, True, _env,
                 _kern % (_k, _ci, _co), seed=_seed + "_7x31")
            _add(f"{_tag}_rule{_rule}_8x32", "fewcout", _conv(2, _ci, 8, 32, _co, _k), _rule, 0, 0.0, 0, True, _env,
                 _kern % (_k, _ci, _co), seed=_seed + "_8x32")
        _add(f"{_tag}_one_pixel", "fewcout", _conv(2, _ci, 1, 1, _co, _k), 0, 2, 0.2, 2, True, _env, _kern % (_k, _ci, _co),
             seed=f"few{_k}x{_k}_{_ci}to{_co}_one_pixel")
for _env, _kern in ((None, LDS), ("PMCTF_FEWCOUT_LDS", PIX)):          # a plane smaller than the 7x7 filter's reach
    for _rule in (0, 1):
        _add(f"few7x7_16to2_{'pix' if _env else 'lds'}_rule{_rule}_3x3", "fewcout", _conv(2, 16, 3, 3, 2, 7), _rule, 2, 0.2, 2,
             True, _env, _kern % (7, 16, 2), seed=f"few7x7_16to2_rule{_rule}_3x3")

# ---- depthwise
_add("dw_k3_c6", "dwconv", _dw(2, 6, 9, 15), 0, 0, 0.0, 0, True, None, DW)
_add("dw_k3_c3", "dwconv", _dw(2, 3, 9, 15), 0, 0, 0.0, 0, True, None, DW)
_add("dw_k1", "dwconv", _dw(2, 4, 9, 15, 1), 0, 0, 0.0, 0, True, None, DW)
_add("dw_k5", "dwconv", _dw(2, 4, 9, 15, 5), 0, 0, 0.0, 0, True, None, DW)
_add("dw_k7_plane_below_the_filter", "dwconv", _dw(2, 8, 5, 3, 7), 0, 0, 0.0, 0, True, None, DW)
_add("dw_strip_w_ragged", "dwconv", _dw(2, 8, 9, 15), 0, 0, 0.0, 0, True, None, DWSTRIP)
_add("dw_strip_w_below_a_strip", "dwconv", _dw(2, 64, 5, 3), 0, 0, 0.0, 0, True, None, DWSTRIP)
_add("dw_strip_one_row", "dwconv", _dw(2, 12, 1, 13), 0, 0, 0.0, 0, True, None, DWSTRIP)
_add("dw_column_threshold", "dwconv", _dw(*COLUMN_PLANE), 0, 0, 0.0, 0, True, None, COLUMN, seed="dw_column_plane")
_add("dw_column_switched_off", "dwconv", _dw(*COLUMN_PLANE), 0, 0, 0.0, 0, True, "PMCTF_DWCONV_COLUMN", DWSTRIP,
     seed="dw_column_plane")
_add("dw_below_column_threshold", "dwconv", _dw(*BELOW_COLUMN_PLANE), 0, 0, 0.0, 0, True, None, DWSTRIP)

# ---- per kernel expression: no bias; zeros of both signs under every rule; subnormal products.  The plane of each
# expression has a border and an interior and room for the four patches of the zero data (zeros_plane below).
SPECIAL = [(STRIP % 1, "smallcin", _conv(2, 1, 5, 21, 112, 3), (0, 1), None),
           (STRIP % 2, "smallcin", _conv(2, 2, 5, 21, 36, 3), (0, 1), None),
           (STRIP % 3, "smallcin", _conv(2, 3, 5, 21, 32, 3), (0, 1), None),
           (REG % (3, 1), "smallcin", _conv(2, 1, 5, 21, 5, 3), (0, 1), None),
           (REG % (3, 2), "smallcin", _conv(2, 2, 5, 21, 3, 3), (0, 1), None),
           (REG % (3, 3), "smallcin", _conv(2, 3, 5, 21, 17, 3), (0, 1), None),
           (REG % (1, 2), "smallcin", _conv(2, 2, 5, 21, 5, 1, pad=1), (0, 1), None),
           (GENERIC, "smallcin", _conv(1, 4, 5, 21, 5, 3), (0, 1, 2), None),
           (PIX16, "cin1_dual", _conv(2, 1, 5, 21, 16, 3), (0, 1), None),
           (LDS % (3, 16, 1), "fewcout", _conv(2, 16, 5, 21, 1, 3), (0, 1), None),
           (LDS % (3, 64, 1), "fewcout", _conv(2, 64, 5, 21, 1, 3), (0, 1), None),
           (LDS % (7, 16, 2), "fewcout", _conv(2, 16, 9, 37, 2, 7), (0, 1), None),
           (PIX % (3, 16, 1), "fewcout", _conv(2, 16, 5, 21, 1, 3), (0, 1), "PMCTF_FEWCOUT_LDS"),
           (PIX % (3, 64, 1), "fewcout", _conv(2, 64, 5, 21, 1, 3), (0, 1), "PMCTF_FEWCOUT_LDS"),
           (PIX % (7, 16, 2), "fewcout", _conv(2, 16, 9, 37, 2, 7), (0, 1), "PMCTF_FEWCOUT_LDS"),
           (COLUMN, "dwconv", _dw(*COLUMN_PLANE), (0,), None),
           (DWSTRIP, "dwconv", _dw(2, 8, 5, 21), (0,), None),
           (DW, "dwconv", _dw(2, 6, 5, 21), (0,), None)]


def _short(expr):
    return expr.replace("_kernel", "").replace("<", "_").replace(">", "").replace(", ", "_")


for _expr, _entry, _geom, _rules, _env in SPECIAL:
    _res = 1 if _entry in HAS_RESIDUALS else 0
    _add(f"nobias_{_short(_expr)}", _entry, _geom, 0, 2 if _res else 0, 0.2 if _res else 0.0, _res, False, _env, _expr)
    for _rule in _rules:
        _add(f"zeros_{_short(_expr)}_rule{_rule}", _entry, _geom, _rule, 1 if _entry == "cin1_dual" else 0, 0.0, 0, True, _env,
             _expr, data="zeros")
    _add(f"subnormal_{_short(_expr)}", _entry, _geom, 0, 0, 0.0, 0, True, _env, _expr, data="subnormal")
_add("nobias_smallcin_gemm", "smallcin", _conv(1, 3, 5, 21, 5, 3), 2, 2, 0.2, 1, False, None, GENERIC)
_add("nobias_smallcin_gemv", "smallcin", _conv(1, 1, 5, 21, 5, 3), 3, 2, 0.2, 1, False, None, GENERIC)
_add("zeros_smallcin_gemv", "smallcin", _conv(1, 1, 5, 21, 5, 3), 3, 0, 0.0, 0, True, None, GENERIC, data="zeros")
_add("subnormal_smallcin_gemv", "smallcin", _conv(1, 1, 5, 21, 5, 3), 3, 0, 0.0, 0, True, None, GENERIC, data="subnormal")

N_ROWS = 206                                   # the count DESIGN 6d records: a row cannot leave unnoticed
MIN_RULE_SHARE = 0.5       # a row under rule R tests R only if the oracle's other rules give other bits in half the elements


def row(rid):
    return next(r for r in CENSUS if r[0] == rid)


def rows_for(env):
    return [r for r in CENSUS if r[8] == env]


def parse_launch(s):
    """'kernel expression grid G' (pmctf_valu_conv_last_launch) -> (expression, G)"""
    expr, sep, grid = s.rpartition(" grid ")
    if not sep or not expr or not grid.isdigit():
        raise ValueError(f"not a launch record: {s!r}")
    return expr, int(grid)


def out_hw(geometry):
    N, Cin, H, W, Cout, KH, KW, S, ph, pw = geometry
    return (H + 2 * ph - KH) // S + 1, (W + 2 * pw - KW) // S + 1


def zero_patches(K):
    """column ranges of the zero data: [-0 | +0 | -(smallest subnormal) | ordinary values to the end of the row]; a patch is
    wider than the filter, so it has columns whose whole window lies inside it"""
    p = max(4, K + 1)
    return (0, p), (p, 2 * p), (2 * p, 3 * p)


def case_data(r):
    """{'x': NCHW, 'w': OIHW ((C, 1, K, K) for depthwise), 'b': bias or None, 'res': [...]}, float32, seeded from the row's
    id (or the id it shares data with).
    normal:    x = normal * 3, w = normal * 0.05, b = normal, residuals = normal
    zeros:     x in column patches of -0, +0, -2^-149 and ordinary values, every weight in [0.25, 0.375), bias -0.  Where
               the chain starts at the bias the -0 patch gives -0, and +0 wherever a zero of the padding is multiplied in;
               where it starts at +0 the -2^-149 patch gives -0 (each product rounds to -0, and +0 + -0 is the only
               sum of zeros that is not the first operand), and again +0 next to the padding.
    subnormal: x = normal * 1e-20, w = normal * 1e-20, b = normal * 1e-40: every product and sum is subnormal
    cancel:    x = 3 (1 + normal / 100), w = normal * 0.05 less its mean over the filter (over each filter row / column for
               cancel_rows / cancel_columns: planes of one row / column), b = normal / 100: the products cancel to a
               hundredth of their size, so the rounding errors of the partial sums are many ulps of the result and two
               summation rules differ almost everywhere.  For the rows with two or three products per output, where the
               normal data tells rule blocks from the chain in 0.23 - 0.42 of the elements only."""
    rid, entry, geometry, rule, act, slope, nres, bias, env, expected, options = r
    N, Cin, H, W, Cout, KH, KW, S, ph, pw = geometry
    g = np.random.default_rng(zlib.crc32(options.get("seed", rid).encode()))
    wshape = (Cout, 1, KH, KW) if entry == "dwconv" else (Cout, Cin, KH, KW)
    kind = options.get("data", "normal")
    if kind == "normal":
        x = g.standard_normal((N, Cin, H, W), dtype=np.float32) * np.float32(3.0)
        w = g.standard_normal(wshape, dtype=np.float32) * np.float32(0.05)
        b = g.standard_normal(Cout, dtype=np.float32)
    elif kind.startswith("cancel"):
        x = np.float32(3.0) * (np.float32(1.0) + g.standard_normal((N, Cin, H, W), dtype=np.float32) * np.float32(0.01))
        w = g.standard_normal(wshape, dtype=np.float32) * np.float32(0.05)
        w = w - w.mean(axis={"cancel": (1, 2, 3), "cancel_rows": (1, 3), "cancel_columns": (1, 2)}[kind], keepdims=True)
        b = g.standard_normal(Cout, dtype=np.float32) * np.float32(0.01)
    elif kind == "subnormal":
        x = g.standard_normal((N, Cin, H, W), dtype=np.float32) * np.float32(1e-20)
        w = g.standard_normal(wshape, dtype=np.float32) * np.float32(1e-20)
        b = (g.standard_normal(Cout) * 1e-40).astype(np.float32)
    else:
        assert kind == "zeros", rid
        x = g.standard_normal((N, Cin, H, W), dtype=np.float32) * np.float32(3.0)
        (a0, a1), (b0, b1), (c0, c1) = zero_patches(max(KH, KW))
        assert W > c1 and H >= 3
        x[..., a0:a1] = np.float32(-0.0)
        x[..., b0:b1] = np.float32(0.0)
        x[..., c0:c1] = np.array(0x80000001, np.uint32).view(np.float32)
        w = (np.float32(0.25) + g.random(wshape, dtype=np.float32) * np.float32(0.125)).astype(np.float32)
        b = np.full(Cout, -0.0, np.float32)
    Ho, Wo = out_hw(geometry)
    res = [g.standard_normal((N, Cout, Ho, Wo), dtype=np.float32) for _ in range(nres)]
    return {"x": x, "w": w, "b": b if bias else None, "res": res}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def oracle_conv(r, d, rule):
    from pmctf_oracle import clib
    rid, entry, (N, Cin, H, W, Cout, KH, KW, S, ph, pw), *_ = r
    if entry == "dwconv":
        return clib.dwconv2d(d["x"], d["w"], d["b"])
    return clib.conv2d(d["x"], d["w"], d["b"], S, (ph, pw), rule)


def other_rules(r):
    """the rules the row's data must tell the row's rule from.  Rule gemm with one input channel IS rule blocks (one chain
    from zero over the same taps, bias last); gemv is defined for one input channel only."""
    rid, entry, geometry, rule = r[:4]
    if not rule:
        return ()
    if rule == 1:
        return (0,)
    if rule == 2:
        return (0,) if geometry[1] == 1 else (0, 1)
    return (0, 1)


def is_subnormal(a):
    u = bits(a)
    return ((u & 0x7f800000) == 0) & ((u & 0x007fffff) != 0)


def precondition(r, d, conv):
    """(ok, text): what a row's data has to show before the row tests anything — see the module docstring of
    test_valu_conv_census_cpu.py"""
    rid, entry, geometry, rule, act, slope, nres, bias, env, expected, options = r
    kind = options.get("data", "normal")
    if kind == "zeros":
        u = bits(conv)
        neg, pos = int((u == 0x80000000).sum()), int((u == 0).sum())
        return neg > 0 and pos > 0, f"{rid}: the oracle's output holds {neg} times -0 and {pos} times +0"
    if kind == "subnormal":
        n = int(is_subnormal(conv).sum())
        return n > 0, f"{rid}: the oracle's output holds {n} subnormal values"
    text, ok = [], True
    for other in other_rules(r):
        share = float((bits(conv) != bits(oracle_conv(r, d, other))).mean())
        text.append(f"rule {rule} differs from rule {other} in {share:.3f} of the elements")
        ok = ok and share >= MIN_RULE_SHARE
    return ok, f"{rid}: " + ("; ".join(text) or "rule 0")


def activate(v, act, slope):
    from pmctf_oracle import clib
    if act == 1:
        return np.where(v < 0, np.float32(0), v)             # max(0, v) as ATen takes it: -0 and NaN stay (pm::relu_)
    if act == 2:
        return np.where(v > 0, v, v * np.float32(slope)).astype(np.float32)
    if act == 3:
        return clib.tanh(v)
    if act == 4:
        return clib.sigmoid(v)
    return v


_REFERENCES = {}


def reference(r):
    """(expected outputs [NCHW, ...], precondition ok, precondition text) from the oracle: clib.conv2d under the row's rule
    (clib.dwconv2d for depthwise rows), then the activation by the oracle's maps, then + res1 + res2.  cin1_dual rows
    expect [conv, act(conv)], or [conv] without y2.  Computed once per (data, arithmetic) and shared: a row behind an
    environment switch expects what its twin on the default kernel expects."""
    rid, entry, geometry, rule, act, slope, nres, bias, env, expected, options = r
    key = (options.get("seed", rid), options.get("data", "normal"), entry, geometry, rule, act, slope, nres, bias,
           options.get("y2", True))
    if key not in _REFERENCES:
        d = case_data(r)
        conv = oracle_conv(r, d, rule)
        ok, text = precondition(r, d, conv)
        if entry == "cin1_dual":
            outs = [conv] + ([activate(conv, act, slope)] if options.get("y2", True) else [])
        else:
            v = activate(conv, act, slope)
            for q in d["res"]:
                v = v + q
            outs = [v]
        _REFERENCES[key] = (outs, ok, text)
    return _REFERENCES[key]


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU (torch and the product are imported here, not above)
SENTINEL = 0xf6b2a5c3          # a float32 of about -1.8e33: no convolution of these inputs gives it
GUARD = 256                    # floats on either side of an output (a multiple of 4: the kernels store 16 bytes at a time)


def _between_sentinels(torch, shapes):
    """one buffer [guard | out_0 | guard | out_1 | guard ...] filled with the sentinel, and the views out_i"""
    sizes = [int(np.prod(s)) for s in shapes]
    pad = [(-n) % 4 for n in sizes]
    total = GUARD + sum(n + p + GUARD for n, p in zip(sizes, pad))
    buf = torch.full((total,), int(np.array(SENTINEL, np.uint32).view(np.int32)), dtype=torch.int32, device="cuda").view(torch.float32)
    views, at = [], GUARD
    for s, n, p in zip(shapes, sizes, pad):
        views.append(buf[at:at + n].view(s))
        at += n + p + GUARD
    return buf, views


def _guards_intact(torch, buf, views):
    mask = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    base = buf.data_ptr()
    for v in views:
        a = (v.data_ptr() - base) // 4
        mask[a:a + v.numel()] = False
    sent = int(np.array(SENTINEL, np.uint32).view(np.int32))
    return bool((buf.view(torch.int32)[mask] == sent).all())


def run_row(r):
    """the row on the GPU: ([outputs NCHW], launch record, guards intact).  Every output lies between sentinels; without
    y2 the slot where y2 would be is part of the guard."""
    import torch
    from pMCTF.hip import lib, ops
    rid, entry, (N, Cin, H, W, Cout, KH, KW, S, ph, pw), rule, act, slope, nres, bias, env, expected, options = r
    d = case_data(r)
    nhwc = lambda a: torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 3, 1))).cuda()
    x = nhwc(d["x"])
    wt = torch.from_numpy(d["w"])
    bt = None if d["b"] is None else torch.from_numpy(d["b"])
    Ho, Wo = out_hw(r[2])
    shape = (N, Ho, Wo, Cout)
    if entry == "dwconv":
        buf, (y,) = _between_sentinels(torch, [shape])
        outs = [ops.DepthwiseConv2d(wt, bt)(x, out=y)]
    elif entry == "cin1_dual":
        conv = ops.Conv2d(wt, bt, 1, (1, 1), rule=rule)
        buf, (y, y2) = _between_sentinels(torch, [shape, shape])
        if options.get("c_entry"):
            with_y2 = options.get("y2", True)
            lib.check(lib.hip().pmctf_conv3x3_cin1_dual_f32(ops._p(x), ops._p(conv.w), ops._p(conv.b), ops._p(y),
                                                            ops._p(y2) if with_y2 else None, N, H, W, 16, int(act),
                                                            float(slope), rule, ops._stream()), rid)
            outs = [y, y2] if with_y2 else [y]
        else:
            assert slope == 0.0                               # the wrapper has no slope argument
            outs = list(ops.conv3x3_cin1_dual(conv, x, act, out=y, out2=y2))
    else:
        conv = ops.Conv2d(wt, bt, S, (ph, pw), rule=rule)
        assert conv.few == (entry == "fewcout") and conv.small == (entry == "smallcin"), rid
        res = [nhwc(q) for q in d["res"]]
        buf, (y,) = _between_sentinels(torch, [shape])
        outs = [conv(x, act=act, slope=slope, res1=res[0] if nres > 0 else None, res2=res[1] if nres > 1 else None, out=y)]
    launched = ops.valu_conv_last_launch()
    torch.cuda.synchronize()
    intact = _guards_intact(torch, buf, outs)
    return [np.ascontiguousarray(o.cpu().numpy().transpose(0, 3, 1, 2)) for o in outs], launched, intact


def main():
    """child process: every row that needs the switch argv[1] at "0", outputs and launch records to the file argv[2]"""
    switch, path = sys.argv[1:3]
    assert switch in SWITCHES and os.environ.get(switch) == "0", f"{switch} must be set to 0"
    for p in (os.path.join(ROOT, "learned-pmctf_amd"), os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    out = {}
    for r in rows_for(switch):
        ys, launched, intact = run_row(r)
        for i, y in enumerate(ys):
            out[f"{r[0]}__y{i}"] = y
        out[f"{r[0]}__launch"] = np.array(launched)
        out[f"{r[0]}__intact"] = np.array(intact)
    np.savez(path, **out)


if __name__ == "__main__":
    main()
