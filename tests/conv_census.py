"""Census of the convolution dispatcher in csrc/conv_mfma.hip: a row for every kernel instantiation (expression, MT, NT)
the library holds and a knob setting reaches, on the smallest plane that is still ragged and with the full epilogue;
the instantiations no setting reaches are listed in UNREACHABLE.  A row names the
kernels it must launch (what pmctf_conv2d_last_launch reports), so a changed threshold that moves a case onto another
kernel fails here instead of leaving the abandoned kernel without a test.  Plain data and helpers: no GPU import.

test_gpu_conv_census.py runs the rows, test_conv_census_cpu.py holds this table against the source text."""
import re
import zlib

import numpy as np

# the tuning knobs of g_knobs with their defaults: a row names the ones it changes, all others run at these values
KNOBS = {"WAVE": 1, "NT": 0, "MSPLIT_PX": 70000, "SPLIT": 1, "BIGPX": 131072, "RES": 0, "MSPLIT_NT": 1, "C16": 1,
         "C16_WGS": 512, "C16_OCC": 2, "V1": 0, "V2": 0, "NBUF1": 1, "K33": 1, "WAVE_SMALL": 1, "K11": 1, "K77": 1,
         "K33_SMALL": 1, "K11_MIN_TILES": 7, "BIGPX_NOSPLIT": 200000, "BSUM_TILEOUTER": 1}

# Rows: (id, geometry, rule, act, slope, residual adds, knobs, expected)
#   geometry = (N, Cin, H, W, Cout, K, stride, pad); rule 0 = chain, 1 = blocks, 32 = reduce blocks of 32 channels
#   act 0 none, 1 relu, 2 leaky(slope), 3 tanh, 4 sigmoid
#   expected = [(kernel expression, MT, NT, TW16), ...] in launch order: the expression is the source text of the launch
#   (template arguments as written there), the numbers are those of the "[MT=.. NT=.. TW16=..]" bracket.
# The standard plane is 2 x 13 x 37 with 32 input channels: ragged for 4x16 and for 8x32 tiles, the last wave tile partly
# outside the plane, two channel chunks.  Couts 8 / 24 / 56 / 100 / 120 give MT = 1 / 2 / 4 / 7 / 8 with a partial last
# tile.  Larger planes only where a path needs them (a pixel threshold, or a grid of at least 512 workgroups).
# The cout-split rows "msplit_wave_*" run 2 x 15 x 32 and 2 x 16 x 31: the wave-private kernel is taken only when both
# the 4x16 and the 8x32 padding of the plane stay below 10 %, which 2 x 12 x 32 (a third of the second tile row empty)
# misses.
CENSUS = [
    # ---- wave-private 3x3 (8x32 workgroup tiles, a 4x16 tile and a patch per wave)
    ("wave33_nbuf1_mt1", (2, 32, 13, 37, 8, 3, 1, 1), 0, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0},
     [("conv3x3s1_wave_kernel<MT, 1>", 1, 4, 2)]),
    ("wave33_nbuf1_mt2", (2, 32, 13, 37, 24, 3, 1, 1), 0, 1, 0.0, 1, {"NT": 4, "MSPLIT_PX": 0},
     [("conv3x3s1_wave_kernel<MT, 1>", 2, 4, 2)]),
    ("wave33_nbuf1_mt4", (2, 32, 13, 37, 56, 3, 1, 1), 0, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0},
     [("conv3x3s1_wave_kernel<MT, 1>", 4, 4, 2)]),
    ("wave33_nbuf2_mt1", (2, 32, 13, 37, 8, 3, 1, 1), 0, 0, 0.0, 0, {"NT": 4, "MSPLIT_PX": 0, "NBUF1": 0},
     [("conv3x3s1_wave_kernel<MT, 2>", 1, 4, 2)]),
    ("wave33_nbuf2_mt2", (2, 32, 13, 37, 24, 3, 1, 1), 0, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0, "NBUF1": 0},
     [("conv3x3s1_wave_kernel<MT, 2>", 2, 4, 2)]),
    ("wave33_nbuf2_mt4", (2, 32, 13, 37, 56, 3, 1, 1), 0, 2, 0.2, 1, {"NT": 4, "MSPLIT_PX": 0, "NBUF1": 0},
     [("conv3x3s1_wave_kernel<MT, 2>", 4, 4, 2)]),
    ("wave33_nbuf2_mt7", (2, 32, 13, 37, 100, 3, 1, 1), 0, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0},
     [("conv3x3s1_wave_kernel<MT, 2>", 7, 4, 2)]),
    ("wave33_nbuf2_mt7_whole", (2, 32, 13, 37, 112, 3, 1, 1), 0, 1, 0.0, 1, {"NT": 4, "MSPLIT_PX": 0},
     [("conv3x3s1_wave_kernel<MT, 2>", 7, 4, 2)]),
    ("wave33_blocks_mt1", (2, 32, 13, 37, 8, 3, 1, 1), 1, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0},
     [("conv3x3s1_wave_kernel<MT, NB, true>", 1, 4, 2)]),
    ("wave33_blocks_mt2", (2, 32, 13, 37, 24, 3, 1, 1), 1, 0, 0.0, 0, {"NT": 4, "MSPLIT_PX": 0},
     [("conv3x3s1_wave_kernel<MT, NB, true>", 2, 4, 2)]),
    ("wave33_blocks_mt4", (2, 32, 13, 37, 56, 3, 1, 1), 1, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0},
     [("conv3x3s1_wave_kernel<MT, NB, true>", 4, 4, 2)]),
    ("wave33_blocks_mt4_whole", (2, 32, 13, 37, 64, 3, 1, 1), 1, 1, 0.0, 1, {"NT": 4, "MSPLIT_PX": 0},
     [("conv3x3s1_wave_kernel<MT, NB, true>", 4, 4, 2)]),
    ("wave33_blocks_mt7_tileouter", (2, 32, 13, 37, 100, 3, 1, 1), 1, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0},
     [("conv3x3s1_blocks_tileouter_kernel", 7, 4, 2)]),
    ("wave33_blocks_mt7_two_launches", (2, 32, 13, 37, 100, 3, 1, 1), 1, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0, "BSUM_TILEOUTER": 0},
     [("conv3x3s1_wave_kernel<4, 2, true, 0>", 7, 4, 2), ("conv3x3s1_wave_kernel<3, 2, true, 4>", 7, 4, 2)]),
    ("wave33_blocks_mt7_tileouter_whole", (2, 32, 13, 37, 112, 3, 1, 1), 1, 1, 0.0, 1, {"NT": 4, "MSPLIT_PX": 0},
     [("conv3x3s1_blocks_tileouter_kernel", 7, 4, 2)]),
    ("wave33_blocks_mt7_two_launches_whole", (2, 32, 13, 37, 112, 3, 1, 1), 1, 1, 0.0, 1, {"NT": 4, "MSPLIT_PX": 0, "BSUM_TILEOUTER": 0},
     [("conv3x3s1_wave_kernel<4, 2, true, 0>", 7, 4, 2), ("conv3x3s1_wave_kernel<3, 2, true, 4>", 7, 4, 2)]),
    # ---- generic wave-private kernel (K33 = 0, and a 1x1 filter with K11 = 0)
    ("wavegen_nbuf1_mt1", (2, 32, 13, 37, 8, 3, 1, 1), 0, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0, "K33": 0},
     [("conv_mfma_wave_kernel<MT, 7, 1>", 1, 4, 2)]),
    ("wavegen_nbuf1_mt2", (2, 32, 13, 37, 24, 3, 1, 1), 0, 0, 0.0, 0, {"NT": 4, "MSPLIT_PX": 0, "K33": 0},
     [("conv_mfma_wave_kernel<MT, 7, 1>", 2, 4, 2)]),
    ("wavegen_nbuf1_mt4", (2, 32, 13, 37, 56, 3, 1, 1), 0, 1, 0.0, 1, {"NT": 4, "MSPLIT_PX": 0, "K33": 0},
     [("conv_mfma_wave_kernel<MT, 7, 1>", 4, 4, 2)]),
    ("wavegen_nbuf2_mt7", (2, 32, 13, 37, 100, 3, 1, 1), 0, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0, "K33": 0},
     [("conv_mfma_wave_kernel<MT, 7>", 7, 4, 2)]),
    ("wavegen_nbuf2_mt1", (2, 32, 13, 37, 8, 3, 1, 1), 0, 1, 0.0, 1, {"NT": 4, "MSPLIT_PX": 0, "K33": 0, "NBUF1": 0},
     [("conv_mfma_wave_kernel<MT, 7>", 1, 4, 2)]),
    ("wavegen_nbuf2_mt2", (2, 32, 13, 37, 24, 3, 1, 1), 0, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0, "K33": 0, "NBUF1": 0},
     [("conv_mfma_wave_kernel<MT, 7>", 2, 4, 2)]),
    ("wavegen_nbuf2_mt4", (2, 32, 13, 37, 56, 3, 1, 1), 0, 0, 0.0, 0, {"NT": 4, "MSPLIT_PX": 0, "K33": 0, "NBUF1": 0},
     [("conv_mfma_wave_kernel<MT, 7>", 4, 4, 2)]),
    ("wavegen_1x1_mt4", (2, 32, 13, 37, 56, 1, 1, 0), 0, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0, "K11": 0},
     [("conv_mfma_wave_kernel<MT, 7, 1>", 4, 4, 2)]),
    # ---- 7x7 (pad 3): the pipelined 7x7 kernel on 8x32 and 4x16 tiles, then what runs without it
    ("k77_nt4_chain_mt1", (2, 16, 13, 37, 8, 7, 1, 3), 0, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0},
     [("conv7x7s1_pipe_kernel<MT, NT>", 1, 4, 2)]),
    ("k77_nt4_blocks_mt1", (2, 32, 13, 37, 8, 7, 1, 3), 1, 0, 0.0, 0, {"NT": 4, "MSPLIT_PX": 0},
     [("conv7x7s1_pipe_kernel<MT, NT, true>", 1, 4, 2)]),
    ("k77_nt4_chain_mt2", (2, 32, 13, 37, 24, 7, 1, 3), 0, 1, 0.0, 1, {"NT": 4, "MSPLIT_PX": 0},
     [("conv7x7s1_pipe_kernel<MT, NT>", 2, 4, 2)]),
    ("k77_nt4_blocks_mt2", (2, 16, 13, 37, 24, 7, 1, 3), 1, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0},
     [("conv7x7s1_pipe_kernel<MT, NT, true>", 2, 4, 2)]),
    ("k77_nt4_chain_mt4", (2, 16, 13, 37, 56, 7, 1, 3), 0, 0, 0.0, 0, {"NT": 4, "MSPLIT_PX": 0},
     [("conv7x7s1_pipe_kernel<MT, NT>", 4, 4, 2)]),
    ("k77_nt4_blocks_mt4", (2, 32, 13, 37, 56, 7, 1, 3), 1, 2, 0.2, 1, {"NT": 4, "MSPLIT_PX": 0},
     [("conv7x7s1_pipe_kernel<MT, NT, true>", 4, 4, 2)]),
    ("k77_nt1_chain_mt1", (2, 32, 13, 37, 8, 7, 1, 3), 0, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0},
     [("conv7x7s1_pipe_kernel<MT, NT>", 1, 1, 1)]),
    ("k77_nt1_blocks_mt1", (2, 16, 13, 37, 8, 7, 1, 3), 1, 0, 0.0, 0, {"NT": 1, "MSPLIT_PX": 0},
     [("conv7x7s1_pipe_kernel<MT, NT, true>", 1, 1, 1)]),
    ("k77_nt1_chain_mt2", (2, 16, 13, 37, 24, 7, 1, 3), 0, 1, 0.0, 1, {"NT": 1, "MSPLIT_PX": 0},
     [("conv7x7s1_pipe_kernel<MT, NT>", 2, 1, 1)]),
    ("k77_nt1_blocks_mt2", (2, 32, 13, 37, 24, 7, 1, 3), 1, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0},
     [("conv7x7s1_pipe_kernel<MT, NT, true>", 2, 1, 1)]),
    ("k77_nt1_chain_mt4", (2, 32, 13, 37, 56, 7, 1, 3), 0, 0, 0.0, 0, {"NT": 1, "MSPLIT_PX": 0},
     [("conv7x7s1_pipe_kernel<MT, NT>", 4, 1, 1)]),
    ("k77_nt1_blocks_mt4", (2, 16, 13, 37, 56, 7, 1, 3), 1, 2, 0.2, 1, {"NT": 1, "MSPLIT_PX": 0},
     [("conv7x7s1_pipe_kernel<MT, NT, true>", 4, 1, 1)]),
    ("k77_off_nt4_chain_mt4", (2, 32, 13, 37, 56, 7, 1, 3), 0, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0, "K77": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 4, 4, 2)]),
    ("k77_off_nt1_chain_mt2", (2, 16, 13, 37, 24, 7, 1, 3), 0, 1, 0.0, 1, {"NT": 1, "MSPLIT_PX": 0, "K77": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 2, 1, 1)]),
    ("k77_off_nt4_blocks_mt4", (2, 32, 13, 37, 56, 7, 1, 3), 1, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0, "K77": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 4, 4, 2)]),
    ("k77_off_nt1_blocks_mt1", (2, 16, 13, 37, 8, 7, 1, 3), 1, 0, 0.0, 0, {"NT": 1, "MSPLIT_PX": 0, "K77": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 1, 1, 1)]),
    ("k77_nt4_chain_mt7", (2, 16, 13, 37, 100, 7, 1, 3), 0, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 9>", 7, 4, 2)]),
    # ---- pipelined 3x3 on 4x16 tiles
    ("pipe33_chain_mt7", (2, 32, 13, 37, 100, 3, 1, 1), 0, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0},
     [("conv3x3s1_pipe_kernel<MT>", 7, 1, 1)]),
    ("pipe33_chain_mt8", (2, 32, 13, 37, 120, 3, 1, 1), 0, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0},
     [("conv3x3s1_pipe_kernel<MT>", 8, 1, 1)]),
    ("pipe33_chain_mt1", (2, 32, 13, 37, 8, 3, 1, 1), 0, 1, 0.0, 1, {"NT": 1, "MSPLIT_PX": 0},
     [("conv3x3s1_pipe_kernel<MT>", 1, 1, 1)]),
    ("pipe33_chain_mt2", (2, 32, 13, 37, 24, 3, 1, 1), 0, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0, "V2": 1},
     [("conv3x3s1_pipe_kernel<MT>", 2, 1, 1)]),
    ("pipe33_chain_mt4", (2, 32, 13, 37, 56, 3, 1, 1), 0, 0, 0.0, 0, {"NT": 1, "MSPLIT_PX": 0, "V2": 1},
     [("conv3x3s1_pipe_kernel<MT>", 4, 1, 1)]),
    ("pipe33_s2_chain_mt7", (2, 32, 13, 37, 100, 3, 2, 1), 0, 1, 0.0, 1, {"NT": 1, "MSPLIT_PX": 0},
     [("conv3x3s1_pipe_kernel<MT, 2>", 7, 1, 1)]),
    ("pipe33_s2_chain_mt8", (2, 32, 13, 37, 120, 3, 2, 1), 0, 0, 0.0, 0, {"NT": 1, "MSPLIT_PX": 0},
     [("conv3x3s1_pipe_kernel<MT, 2>", 8, 1, 1)]),
    ("pipe33_s2_chain_mt1", (2, 32, 13, 37, 8, 3, 2, 1), 0, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0},
     [("conv3x3s1_pipe_kernel<MT, 2>", 1, 1, 1)]),
    ("pipe33_s2_chain_mt2", (2, 32, 13, 37, 24, 3, 2, 1), 0, 2, 0.2, 1, {"NT": 1, "MSPLIT_PX": 0, "V2": 1},
     [("conv3x3s1_pipe_kernel<MT, 2>", 2, 1, 1)]),
    ("pipe33_s2_chain_mt4", (2, 32, 13, 37, 56, 3, 2, 1), 0, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0, "V2": 1},
     [("conv3x3s1_pipe_kernel<MT, 2>", 4, 1, 1)]),
    ("pipe33_blocks_mt1", (2, 32, 13, 37, 8, 3, 1, 1), 1, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0},
     [("conv3x3s1_pipe_kernel<MT, 1, true>", 1, 1, 1)]),
    ("pipe33_blocks_mt7", (2, 32, 13, 37, 100, 3, 1, 1), 1, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0},
     [("conv3x3s1_pipe_kernel<MT, 1, true>", 7, 1, 1)]),
    ("pipe33_blocks_mt8", (2, 32, 13, 37, 120, 3, 1, 1), 1, 1, 0.0, 1, {"NT": 1, "MSPLIT_PX": 0},
     [("conv3x3s1_pipe_kernel<MT, 1, true>", 8, 1, 1)]),
    ("pipe33_s2_blocks_mt1", (2, 32, 13, 37, 8, 3, 2, 1), 1, 0, 0.0, 0, {"NT": 1, "MSPLIT_PX": 0},
     [("conv3x3s1_pipe_kernel<MT, 2, true>", 1, 1, 1)]),
    ("pipe33_s2_blocks_mt7", (2, 32, 13, 37, 100, 3, 2, 1), 1, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0},
     [("conv3x3s1_pipe_kernel<MT, 2, true>", 7, 1, 1)]),
    ("pipe33_s2_blocks_mt8", (2, 32, 13, 37, 120, 3, 2, 1), 1, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0},
     [("conv3x3s1_pipe_kernel<MT, 2, true>", 8, 1, 1)]),
    ("pipe33_blocks_mt2_generic", (2, 32, 13, 37, 24, 3, 1, 1), 1, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 2, 1, 1)]),
    ("pipe33_blocks_mt4_generic", (2, 32, 13, 37, 56, 3, 1, 1), 1, 1, 0.0, 1, {"NT": 1, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 4, 1, 1)]),
    # ---- generic pipelined kernel (6 and 9 staging slots) and the single-buffer kernel behind V1
    ("pipegen6_nt2_mt7", (2, 32, 13, 37, 100, 3, 1, 1), 0, 2, 0.2, 2, {"NT": 2, "MSPLIT_PX": 0},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 6>", 7, 2, 1)]),
    ("pipegen6_nt2_mt8", (2, 32, 13, 37, 120, 3, 1, 1), 0, 1, 0.0, 1, {"NT": 2, "MSPLIT_PX": 0},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 6>", 8, 2, 1)]),
    ("pipegen9_nt2_s2_mt7", (2, 32, 13, 37, 100, 3, 2, 1), 0, 0, 0.0, 0, {"NT": 2, "MSPLIT_PX": 0},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 9>", 7, 2, 1)]),
    ("pipegen9_nt2_s2_mt8", (2, 32, 13, 37, 120, 3, 2, 1), 0, 2, 0.2, 2, {"NT": 2, "MSPLIT_PX": 0},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 9>", 8, 2, 1)]),
    ("pipegen6_nt2_v2_mt1", (2, 32, 13, 37, 8, 3, 1, 1), 0, 2, 0.2, 2, {"NT": 2, "MSPLIT_PX": 0, "V2": 1},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 6>", 1, 2, 1)]),
    ("pipegen6_nt2_v2_mt2", (2, 32, 13, 37, 24, 3, 1, 1), 0, 0, 0.0, 0, {"NT": 2, "MSPLIT_PX": 0, "V2": 1},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 6>", 2, 2, 1)]),
    ("pipegen6_nt2_v2_mt4", (2, 32, 13, 37, 56, 3, 1, 1), 0, 2, 0.2, 2, {"NT": 2, "MSPLIT_PX": 0, "V2": 1},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 6>", 4, 2, 1)]),
    ("pipegen9_nt2_s2_v2_mt1", (2, 32, 13, 37, 8, 3, 2, 1), 0, 1, 0.0, 1, {"NT": 2, "MSPLIT_PX": 0, "V2": 1},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 9>", 1, 2, 1)]),
    ("pipegen9_nt2_s2_v2_mt2", (2, 32, 13, 37, 24, 3, 2, 1), 0, 2, 0.2, 2, {"NT": 2, "MSPLIT_PX": 0, "V2": 1},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 9>", 2, 2, 1)]),
    ("pipegen9_nt2_s2_v2_mt4", (2, 32, 13, 37, 56, 3, 2, 1), 0, 2, 0.2, 1, {"NT": 2, "MSPLIT_PX": 0, "V2": 1},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 9>", 4, 2, 1)]),
    ("pipegen6_nt4_nowave_mt7", (2, 32, 13, 37, 100, 3, 1, 1), 0, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0, "WAVE": 0},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 6>", 7, 4, 2)]),
    ("pipegen6_nt1_1x1_mt2", (2, 32, 13, 37, 24, 1, 1, 0), 0, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0, "K11": 0},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 6>", 2, 1, 1)]),
    ("v1_nt2_mt7", (2, 32, 13, 37, 100, 3, 1, 1), 0, 2, 0.2, 2, {"NT": 2, "MSPLIT_PX": 0, "V1": 1},
     [("conv_mfma_kernel<MT, NT, TW16>", 7, 2, 1)]),
    ("v1_nt2_mt8", (2, 32, 13, 37, 120, 3, 1, 1), 0, 0, 0.0, 0, {"NT": 2, "MSPLIT_PX": 0, "V1": 1},
     [("conv_mfma_kernel<MT, NT, TW16>", 8, 2, 1)]),
    ("v1_nt1_mt7", (2, 32, 13, 37, 100, 3, 1, 1), 0, 1, 0.0, 1, {"NT": 1, "MSPLIT_PX": 0, "V1": 1},
     [("conv_mfma_kernel<MT, NT, TW16>", 7, 1, 1)]),
    # ---- generic single-buffer and block-sum kernels on every tile shape: 5x5, Cin = 8, tanh / sigmoid, reduce rule 32
    ("gen_nt1_5x5_chain_mt4", (2, 32, 13, 37, 56, 5, 1, 2), 0, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 4, 1, 1)]),
    ("gen_nt1_5x5_blocks_mt4", (2, 32, 13, 37, 56, 5, 1, 2), 1, 1, 0.0, 1, {"NT": 1, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 4, 1, 1)]),
    ("gen_nt1_5x5_chain_mt7", (2, 16, 13, 37, 100, 5, 1, 2), 0, 0, 0.0, 0, {"NT": 1, "MSPLIT_PX": 0},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 6>", 7, 1, 1)]),
    ("gen_nt1_cin8_chain_mt2", (2, 8, 13, 37, 24, 3, 1, 1), 0, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 2, 1, 1)]),
    ("gen_nt1_cin8_blocks_mt7", (2, 8, 13, 37, 100, 3, 1, 1), 1, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 7, 1, 1)]),
    ("gen_nt1_cin8_chain_mt1", (2, 8, 13, 37, 8, 3, 1, 1), 0, 1, 0.0, 1, {"NT": 1, "MSPLIT_PX": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 1, 1, 1)]),
    ("gen_nt1_tanh_chain_mt8", (2, 32, 13, 37, 120, 3, 1, 1), 0, 3, 0.0, 2, {"NT": 1, "MSPLIT_PX": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 8, 1, 1)]),
    ("gen_nt1_sigmoid_chain_mt1", (2, 32, 13, 37, 8, 3, 1, 1), 0, 4, 0.0, 1, {"NT": 1, "MSPLIT_PX": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 1, 1, 1)]),
    ("gen_nt1_tanh_blocks_mt2", (2, 32, 13, 37, 24, 3, 1, 1), 1, 3, 0.0, 0, {"NT": 1, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 2, 1, 1)]),
    ("gen_nt1_sigmoid_blocks_mt7", (2, 32, 13, 37, 100, 3, 1, 1), 1, 4, 0.0, 2, {"NT": 1, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 7, 1, 1)]),
    ("gen_nt1_reduce32_mt1", (2, 64, 13, 37, 8, 3, 1, 1), 32, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 1, 1, 1)]),
    ("gen_nt1_reduce32_mt4", (2, 64, 13, 37, 56, 3, 1, 1), 32, 0, 0.0, 0, {"NT": 1, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 4, 1, 1)]),
    ("gen_nt1_reduce32_mt7", (2, 64, 13, 37, 100, 3, 1, 1), 32, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 7, 1, 1)]),
    ("gen_nt1_reduce32_mt8", (2, 64, 13, 37, 120, 3, 1, 1), 32, 1, 0.0, 1, {"NT": 1, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 8, 1, 1)]),
    ("gen_nt1_cin8_blocks_mt8", (2, 8, 13, 37, 120, 3, 1, 1), 1, 0, 0.0, 0, {"NT": 1, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 8, 1, 1)]),
    ("gen_nt1_cin8_chain_mt4", (2, 8, 13, 37, 56, 3, 1, 1), 0, 2, 0.2, 1, {"NT": 1, "MSPLIT_PX": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 4, 1, 1)]),
    ("gen_nt2_5x5_chain_mt4", (2, 32, 13, 37, 56, 5, 1, 2), 0, 2, 0.2, 2, {"NT": 2, "MSPLIT_PX": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 4, 2, 1)]),
    ("gen_nt2_5x5_blocks_mt4", (2, 32, 13, 37, 56, 5, 1, 2), 1, 1, 0.0, 1, {"NT": 2, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 4, 2, 1)]),
    ("gen_nt2_5x5_chain_mt7", (2, 16, 13, 37, 100, 5, 1, 2), 0, 0, 0.0, 0, {"NT": 2, "MSPLIT_PX": 0},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 6>", 7, 2, 1)]),
    ("gen_nt2_cin8_chain_mt2", (2, 8, 13, 37, 24, 3, 1, 1), 0, 2, 0.2, 2, {"NT": 2, "MSPLIT_PX": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 2, 2, 1)]),
    ("gen_nt2_cin8_blocks_mt7", (2, 8, 13, 37, 100, 3, 1, 1), 1, 2, 0.2, 2, {"NT": 2, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 7, 2, 1)]),
    ("gen_nt2_cin8_chain_mt1", (2, 8, 13, 37, 8, 3, 1, 1), 0, 1, 0.0, 1, {"NT": 2, "MSPLIT_PX": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 1, 2, 1)]),
    ("gen_nt2_tanh_chain_mt8", (2, 32, 13, 37, 120, 3, 1, 1), 0, 3, 0.0, 2, {"NT": 2, "MSPLIT_PX": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 8, 2, 1)]),
    ("gen_nt2_sigmoid_chain_mt1", (2, 32, 13, 37, 8, 3, 1, 1), 0, 4, 0.0, 1, {"NT": 2, "MSPLIT_PX": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 1, 2, 1)]),
    ("gen_nt2_tanh_blocks_mt2", (2, 32, 13, 37, 24, 3, 1, 1), 1, 3, 0.0, 0, {"NT": 2, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 2, 2, 1)]),
    ("gen_nt2_sigmoid_blocks_mt7", (2, 32, 13, 37, 100, 3, 1, 1), 1, 4, 0.0, 2, {"NT": 2, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 7, 2, 1)]),
    ("gen_nt2_reduce32_mt1", (2, 64, 13, 37, 8, 3, 1, 1), 32, 2, 0.2, 2, {"NT": 2, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 1, 2, 1)]),
    ("gen_nt2_reduce32_mt4", (2, 64, 13, 37, 56, 3, 1, 1), 32, 0, 0.0, 0, {"NT": 2, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 4, 2, 1)]),
    ("gen_nt2_reduce32_mt7", (2, 64, 13, 37, 100, 3, 1, 1), 32, 2, 0.2, 2, {"NT": 2, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 7, 2, 1)]),
    ("gen_nt2_reduce32_mt8", (2, 64, 13, 37, 120, 3, 1, 1), 32, 1, 0.0, 1, {"NT": 2, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 8, 2, 1)]),
    ("gen_nt2_cin8_blocks_mt8", (2, 8, 13, 37, 120, 3, 1, 1), 1, 0, 0.0, 0, {"NT": 2, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 8, 2, 1)]),
    ("gen_nt2_cin8_chain_mt4", (2, 8, 13, 37, 56, 3, 1, 1), 0, 2, 0.2, 1, {"NT": 2, "MSPLIT_PX": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 4, 2, 1)]),
    ("gen_nt4_5x5_chain_mt4", (2, 32, 13, 37, 56, 5, 1, 2), 0, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 4, 4, 2)]),
    ("gen_nt4_5x5_blocks_mt4", (2, 32, 13, 37, 56, 5, 1, 2), 1, 1, 0.0, 1, {"NT": 4, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 4, 4, 2)]),
    ("gen_nt4_5x5_chain_mt7", (2, 16, 13, 37, 100, 5, 1, 2), 0, 0, 0.0, 0, {"NT": 4, "MSPLIT_PX": 0},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 9>", 7, 4, 2)]),
    ("gen_nt4_cin8_chain_mt2", (2, 8, 13, 37, 24, 3, 1, 1), 0, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 2, 4, 2)]),
    ("gen_nt4_cin8_blocks_mt7", (2, 8, 13, 37, 100, 3, 1, 1), 1, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 7, 2, 1)]),
    ("gen_nt4_cin8_chain_mt1", (2, 8, 13, 37, 8, 3, 1, 1), 0, 1, 0.0, 1, {"NT": 4, "MSPLIT_PX": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 1, 4, 2)]),
    ("gen_nt4_tanh_chain_mt7", (2, 32, 13, 37, 100, 3, 1, 1), 0, 3, 0.0, 2, {"NT": 4, "MSPLIT_PX": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 7, 4, 2)]),
    ("gen_nt4_sigmoid_chain_mt1", (2, 32, 13, 37, 8, 3, 1, 1), 0, 4, 0.0, 1, {"NT": 4, "MSPLIT_PX": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 1, 4, 2)]),
    ("gen_nt4_tanh_blocks_mt2", (2, 32, 13, 37, 24, 3, 1, 1), 1, 3, 0.0, 0, {"NT": 4, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 2, 4, 2)]),
    ("gen_nt4_sigmoid_blocks_mt4", (2, 32, 13, 37, 56, 3, 1, 1), 1, 4, 0.0, 2, {"NT": 4, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 4, 4, 2)]),
    ("gen_nt4_reduce32_mt1", (2, 64, 13, 37, 8, 3, 1, 1), 32, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 1, 4, 2)]),
    ("gen_nt4_reduce32_mt4", (2, 64, 13, 37, 56, 3, 1, 1), 32, 0, 0.0, 0, {"NT": 4, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 4, 4, 2)]),
    ("gen_nt4_reduce32_mt7", (2, 64, 13, 37, 100, 3, 1, 1), 32, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 7, 2, 1)]),
    ("gen_nt4_cin8_chain_mt4", (2, 8, 13, 37, 56, 3, 1, 1), 0, 2, 0.2, 1, {"NT": 4, "MSPLIT_PX": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 4, 4, 2)]),
    # ---- cout-split small-plane path: an MT = 1 kernel over weights packed for MTP tiles, grid.z = MTP * MB
    ("msplit_wave_mtp2_chain", (2, 32, 15, 32, 24, 3, 1, 1), 0, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40},
     [("conv3x3s1_wave_kernel<MT, 1>", 1, 4, 2)]),
    ("msplit_pipe33_mtp2_chain", (2, 32, 13, 37, 24, 3, 1, 1), 0, 1, 0.0, 1, {"MSPLIT_PX": 1 << 40},
     [("conv3x3s1_pipe_kernel<MT>", 1, 1, 1)]),
    ("msplit_generic_mtp2_chain", (2, 32, 13, 37, 24, 3, 1, 1), 0, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40, "K33_SMALL": 0, "WAVE_SMALL": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 1, 1, 1)]),
    ("msplit_nt2_mtp2_chain", (2, 32, 13, 37, 24, 3, 1, 1), 0, 1, 0.0, 1, {"MSPLIT_PX": 1 << 40, "MSPLIT_NT": 2},
     [("conv_mfma_kernel<MT, NT, TW16>", 1, 2, 1)]),
    ("msplit_nt4_mtp2_chain", (2, 32, 13, 37, 24, 3, 1, 1), 0, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40, "MSPLIT_NT": 4},
     [("conv3x3s1_wave_kernel<MT, 1>", 1, 4, 2)]),
    ("msplit_wave_mtp2_blocks", (2, 32, 15, 32, 24, 3, 1, 1), 1, 0, 0.0, 0, {"MSPLIT_PX": 1 << 40},
     [("conv3x3s1_wave_kernel<MT, NB, true>", 1, 4, 2)]),
    ("msplit_pipe33_mtp2_blocks", (2, 32, 13, 37, 24, 3, 1, 1), 1, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40},
     [("conv3x3s1_pipe_kernel<MT, 1, true>", 1, 1, 1)]),
    ("msplit_generic_mtp2_blocks", (2, 32, 13, 37, 24, 3, 1, 1), 1, 0, 0.0, 0, {"MSPLIT_PX": 1 << 40, "K33_SMALL": 0, "WAVE_SMALL": 0},
     [("conv3x3s1_pipe_kernel<MT, 1, true>", 1, 1, 1)]),
    ("msplit_nt2_mtp2_blocks", (2, 32, 13, 37, 24, 3, 1, 1), 1, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40, "MSPLIT_NT": 2},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 1, 2, 1)]),
    ("msplit_nt4_mtp2_blocks", (2, 32, 13, 37, 24, 3, 1, 1), 1, 0, 0.0, 0, {"MSPLIT_PX": 1 << 40, "MSPLIT_NT": 4},
     [("conv3x3s1_wave_kernel<MT, NB, true>", 1, 4, 2)]),
    ("msplit_wave_mtp4_chain", (2, 32, 16, 31, 56, 3, 1, 1), 0, 1, 0.0, 1, {"MSPLIT_PX": 1 << 40},
     [("conv3x3s1_wave_kernel<MT, 1>", 1, 4, 2)]),
    ("msplit_pipe33_mtp4_chain", (2, 32, 13, 37, 56, 3, 1, 1), 0, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40},
     [("conv3x3s1_pipe_kernel<MT>", 1, 1, 1)]),
    ("msplit_generic_mtp4_chain", (2, 32, 13, 37, 56, 3, 1, 1), 0, 1, 0.0, 1, {"MSPLIT_PX": 1 << 40, "K33_SMALL": 0, "WAVE_SMALL": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 1, 1, 1)]),
    ("msplit_nt2_mtp4_chain", (2, 32, 13, 37, 56, 3, 1, 1), 0, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40, "MSPLIT_NT": 2},
     [("conv_mfma_kernel<MT, NT, TW16>", 1, 2, 1)]),
    ("msplit_nt4_mtp4_chain", (2, 32, 13, 37, 56, 3, 1, 1), 0, 1, 0.0, 1, {"MSPLIT_PX": 1 << 40, "MSPLIT_NT": 4},
     [("conv3x3s1_wave_kernel<MT, 1>", 1, 4, 2)]),
    ("msplit_wave_mtp4_blocks", (2, 32, 16, 31, 56, 3, 1, 1), 1, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40},
     [("conv3x3s1_wave_kernel<MT, NB, true>", 1, 4, 2)]),
    ("msplit_pipe33_mtp4_blocks", (2, 32, 13, 37, 56, 3, 1, 1), 1, 2, 0.2, 1, {"MSPLIT_PX": 1 << 40},
     [("conv3x3s1_pipe_kernel<MT, 1, true>", 1, 1, 1)]),
    ("msplit_generic_mtp4_blocks", (2, 32, 13, 37, 56, 3, 1, 1), 1, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40, "K33_SMALL": 0, "WAVE_SMALL": 0},
     [("conv3x3s1_pipe_kernel<MT, 1, true>", 1, 1, 1)]),
    ("msplit_nt2_mtp4_blocks", (2, 32, 13, 37, 56, 3, 1, 1), 1, 2, 0.2, 1, {"MSPLIT_PX": 1 << 40, "MSPLIT_NT": 2},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 1, 2, 1)]),
    ("msplit_nt4_mtp4_blocks", (2, 32, 13, 37, 56, 3, 1, 1), 1, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40, "MSPLIT_NT": 4},
     [("conv3x3s1_wave_kernel<MT, NB, true>", 1, 4, 2)]),
    ("msplit_wave_mtp7_chain", (2, 32, 15, 32, 100, 3, 1, 1), 0, 1, 0.0, 1, {"MSPLIT_PX": 1 << 40},
     [("conv3x3s1_wave_kernel<MT, 1>", 1, 4, 2)]),
    ("msplit_pipe33_mtp7_chain", (2, 32, 13, 37, 100, 3, 1, 1), 0, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40},
     [("conv3x3s1_pipe_kernel<MT>", 1, 1, 1)]),
    ("msplit_generic_mtp7_chain", (2, 32, 13, 37, 100, 3, 1, 1), 0, 1, 0.0, 1, {"MSPLIT_PX": 1 << 40, "K33_SMALL": 0, "WAVE_SMALL": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 1, 1, 1)]),
    ("msplit_nt2_mtp7_chain", (2, 32, 13, 37, 100, 3, 1, 1), 0, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40, "MSPLIT_NT": 2},
     [("conv_mfma_kernel<MT, NT, TW16>", 1, 2, 1)]),
    ("msplit_nt4_mtp7_chain", (2, 32, 13, 37, 100, 3, 1, 1), 0, 1, 0.0, 1, {"MSPLIT_PX": 1 << 40, "MSPLIT_NT": 4},
     [("conv3x3s1_wave_kernel<MT, 1>", 1, 4, 2)]),
    ("msplit_wave_mtp7_blocks", (2, 32, 15, 32, 100, 3, 1, 1), 1, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40},
     [("conv3x3s1_wave_kernel<MT, NB, true>", 1, 4, 2)]),
    ("msplit_pipe33_mtp7_blocks", (2, 32, 13, 37, 100, 3, 1, 1), 1, 2, 0.2, 1, {"MSPLIT_PX": 1 << 40},
     [("conv3x3s1_pipe_kernel<MT, 1, true>", 1, 1, 1)]),
    ("msplit_generic_mtp7_blocks", (2, 32, 13, 37, 100, 3, 1, 1), 1, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40, "K33_SMALL": 0, "WAVE_SMALL": 0},
     [("conv3x3s1_pipe_kernel<MT, 1, true>", 1, 1, 1)]),
    ("msplit_nt2_mtp7_blocks", (2, 32, 13, 37, 100, 3, 1, 1), 1, 2, 0.2, 1, {"MSPLIT_PX": 1 << 40, "MSPLIT_NT": 2},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 1, 2, 1)]),
    ("msplit_nt4_mtp7_blocks", (2, 32, 13, 37, 100, 3, 1, 1), 1, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40, "MSPLIT_NT": 4},
     [("conv3x3s1_wave_kernel<MT, NB, true>", 1, 4, 2)]),
    ("msplit_wave_mtp8_chain", (2, 32, 16, 31, 120, 3, 1, 1), 0, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40},
     [("conv3x3s1_wave_kernel<MT, 1>", 1, 4, 2)]),
    ("msplit_pipe33_mtp8_chain", (2, 32, 13, 37, 120, 3, 1, 1), 0, 1, 0.0, 1, {"MSPLIT_PX": 1 << 40},
     [("conv3x3s1_pipe_kernel<MT>", 1, 1, 1)]),
    ("msplit_generic_mtp8_chain", (2, 32, 13, 37, 120, 3, 1, 1), 0, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40, "K33_SMALL": 0, "WAVE_SMALL": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 1, 1, 1)]),
    ("msplit_nt2_mtp8_chain", (2, 32, 13, 37, 120, 3, 1, 1), 0, 1, 0.0, 1, {"MSPLIT_PX": 1 << 40, "MSPLIT_NT": 2},
     [("conv_mfma_kernel<MT, NT, TW16>", 1, 2, 1)]),
    ("msplit_nt4_mtp8_chain", (2, 32, 13, 37, 120, 3, 1, 1), 0, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40, "MSPLIT_NT": 4},
     [("conv3x3s1_wave_kernel<MT, 1>", 1, 4, 2)]),
    ("msplit_wave_mtp8_blocks", (2, 32, 16, 31, 120, 3, 1, 1), 1, 0, 0.0, 0, {"MSPLIT_PX": 1 << 40},
     [("conv3x3s1_wave_kernel<MT, NB, true>", 1, 4, 2)]),
    ("msplit_pipe33_mtp8_blocks", (2, 32, 13, 37, 120, 3, 1, 1), 1, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40},
     [("conv3x3s1_pipe_kernel<MT, 1, true>", 1, 1, 1)]),
    ("msplit_generic_mtp8_blocks", (2, 32, 13, 37, 120, 3, 1, 1), 1, 0, 0.0, 0, {"MSPLIT_PX": 1 << 40, "K33_SMALL": 0, "WAVE_SMALL": 0},
     [("conv3x3s1_pipe_kernel<MT, 1, true>", 1, 1, 1)]),
    ("msplit_nt2_mtp8_blocks", (2, 32, 13, 37, 120, 3, 1, 1), 1, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40, "MSPLIT_NT": 2},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 1, 2, 1)]),
    ("msplit_nt4_mtp8_blocks", (2, 32, 13, 37, 120, 3, 1, 1), 1, 0, 0.0, 0, {"MSPLIT_PX": 1 << 40, "MSPLIT_NT": 4},
     [("conv3x3s1_wave_kernel<MT, NB, true>", 1, 4, 2)]),
    ("msplit_two_m_blocks_mtp7_chain", (2, 32, 13, 37, 200, 3, 1, 1), 0, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40},
     [("conv3x3s1_pipe_kernel<MT>", 1, 1, 1)]),
    ("msplit_s2_whole_mtp7_chain", (2, 16, 130, 130, 112, 3, 2, 1), 0, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40},
     [("conv3x3s1_pipe_kernel<MT, 2>", 7, 1, 1)]),
    ("msplit_s2_whole_mtp7_blocks", (2, 16, 130, 130, 100, 3, 2, 1), 1, 1, 0.0, 1, {"MSPLIT_PX": 1 << 40},
     [("conv3x3s1_pipe_kernel<MT, 2, true>", 7, 1, 1)]),
    ("msplit_s2_below_8000px_mtp7_chain", (2, 32, 13, 37, 100, 3, 2, 1), 0, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40},
     [("conv3x3s1_pipe_kernel<MT, 2>", 1, 1, 1)]),
    # ---- couts that are no multiple of 4: the epilogue stores element by element
    ("oddcout_wave33_mt7", (2, 32, 13, 37, 99, 3, 1, 1), 0, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0},
     [("conv3x3s1_wave_kernel<MT, 2>", 7, 4, 2)]),
    ("oddcout_wave33_blocks_mt4", (2, 32, 13, 37, 50, 3, 1, 1), 1, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0},
     [("conv3x3s1_wave_kernel<MT, NB, true>", 4, 4, 2)]),
    ("oddcout_tileouter_mt7", (2, 32, 13, 37, 99, 3, 1, 1), 1, 1, 0.0, 1, {"NT": 4, "MSPLIT_PX": 0},
     [("conv3x3s1_blocks_tileouter_kernel", 7, 4, 2)]),
    ("oddcout_wavegen_mt2", (2, 32, 13, 37, 21, 3, 1, 1), 0, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0, "K33": 0},
     [("conv_mfma_wave_kernel<MT, 7, 1>", 2, 4, 2)]),
    ("oddcout_k77_nt4_mt2", (2, 16, 13, 37, 21, 7, 1, 3), 0, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0},
     [("conv7x7s1_pipe_kernel<MT, NT>", 2, 4, 2)]),
    ("oddcout_k77_nt1_blocks_mt1", (2, 32, 13, 37, 7, 7, 1, 3), 1, 1, 0.0, 1, {"NT": 1, "MSPLIT_PX": 0},
     [("conv7x7s1_pipe_kernel<MT, NT, true>", 1, 1, 1)]),
    ("oddcout_pipe33_mt7", (2, 32, 13, 37, 99, 3, 1, 1), 0, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0},
     [("conv3x3s1_pipe_kernel<MT>", 7, 1, 1)]),
    ("oddcout_pipe33_s2_blocks_mt8", (2, 32, 13, 37, 118, 3, 2, 1), 1, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0},
     [("conv3x3s1_pipe_kernel<MT, 2, true>", 8, 1, 1)]),
    ("oddcout_pipegen6_nt2_mt8", (2, 32, 13, 37, 118, 3, 1, 1), 0, 2, 0.2, 2, {"NT": 2, "MSPLIT_PX": 0},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 6>", 8, 2, 1)]),
    ("oddcout_gen_nt2_5x5_blocks_mt4", (2, 32, 13, 37, 50, 5, 1, 2), 1, 2, 0.2, 2, {"NT": 2, "MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 4, 2, 1)]),
    ("oddcout_msplit_wave_mtp7", (2, 32, 15, 32, 99, 3, 1, 1), 0, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40},
     [("conv3x3s1_wave_kernel<MT, 1>", 1, 4, 2)]),
    ("oddcout_res2_mtp4", (2, 32, 13, 37, 50, 3, 1, 1), 0, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40, "RES": 2},
     [("conv_mfma_res_kernel<MT>", 4, 1, 1)]),
    ("oddcout_gemm1x1_cout99", (1, 32, 129, 130, 99, 1, 1, 0), 0, 2, 0.2, 2, {}, [("conv1x1_kernel<MTW, NT>", 2, 2, 1)]),
    # ---- instantiations only a second knob reaches: generic pipelined kernel on the remaining (MT, NT), 1x1 GEMM at 64 pixels
    ("pipegen6_nt4_nowave_v2_mt1", (2, 32, 13, 37, 8, 3, 1, 1), 0, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0, "WAVE": 0, "V2": 1},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 6>", 1, 4, 2)]),
    ("pipegen6_nt4_nowave_v2_mt2", (2, 32, 13, 37, 24, 3, 1, 1), 0, 1, 0.0, 1, {"NT": 4, "MSPLIT_PX": 0, "WAVE": 0, "V2": 1},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 6>", 2, 4, 2)]),
    ("pipegen6_nt4_nowave_v2_mt4", (2, 32, 13, 37, 56, 3, 1, 1), 0, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0, "WAVE": 0, "V2": 1},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 6>", 4, 4, 2)]),
    ("pipegen9_nt4_5x5_v2_mt1", (2, 32, 13, 37, 8, 5, 1, 2), 0, 1, 0.0, 1, {"NT": 4, "MSPLIT_PX": 0, "V2": 1},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 9>", 1, 4, 2)]),
    ("pipegen9_nt4_5x5_v2_mt2", (2, 32, 13, 37, 24, 5, 1, 2), 0, 2, 0.2, 2, {"NT": 4, "MSPLIT_PX": 0, "V2": 1},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 9>", 2, 4, 2)]),
    ("pipegen9_nt4_5x5_v2_mt4", (2, 32, 13, 37, 56, 5, 1, 2), 0, 0, 0.0, 0, {"NT": 4, "MSPLIT_PX": 0, "V2": 1},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 9>", 4, 4, 2)]),
    ("pipegen6_nt1_1x1_mt1", (2, 32, 13, 37, 8, 1, 1, 0), 0, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0, "K11": 0},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 6>", 1, 1, 1)]),
    ("pipegen6_nt1_5x5_mt8", (2, 32, 13, 37, 120, 5, 1, 2), 0, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 6>", 8, 1, 1)]),
    ("pipegen9_nt1_7x7_s2_v2_mt1", (2, 16, 13, 37, 8, 7, 2, 3), 0, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0, "V2": 1},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 9>", 1, 1, 1)]),
    ("pipegen9_nt1_5x5_s2_v2_mt2", (2, 16, 13, 37, 24, 5, 2, 2), 0, 1, 0.0, 1, {"NT": 1, "MSPLIT_PX": 0, "V2": 1},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 9>", 2, 1, 1)]),
    ("pipegen9_nt1_7x7_s2_v2_mt4", (2, 16, 13, 37, 56, 7, 2, 3), 0, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0, "V2": 1},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 9>", 4, 1, 1)]),
    ("pipegen9_nt1_5x5_s2_mt7", (2, 16, 13, 37, 100, 5, 2, 2), 0, 2, 0.2, 2, {"NT": 1, "MSPLIT_PX": 0},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 9>", 7, 1, 1)]),
    ("pipegen9_nt1_7x7_s2_mt8", (2, 16, 13, 37, 120, 7, 2, 3), 0, 2, 0.2, 1, {"NT": 1, "MSPLIT_PX": 0},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 9>", 8, 1, 1)]),
    ("gemm1x1_nt4_four_tiles_cout56", (2, 32, 129, 130, 56, 1, 1, 0), 0, 2, 0.2, 2, {"K11_MIN_TILES": 4},
     [("conv1x1_kernel<MTW, NT>", 1, 4, 1)]),
    ("gemm1x1_reduce32_nt4_cout56", (2, 64, 129, 130, 56, 1, 1, 0), 32, 1, 0.0, 1, {},
     [("conv1x1_kernel<MTW, NT, true>", 1, 4, 1)]),
    ("gemm1x1_reduce32_nt4_cout100", (2, 64, 129, 130, 100, 1, 1, 0), 32, 2, 0.2, 2, {},
     [("conv1x1_kernel<MTW, NT, true>", 2, 4, 1)]),
    ("gemm1x1_reduce32_nt4_cout180", (2, 64, 129, 130, 180, 1, 1, 0), 32, 0, 0.0, 0, {},
     [("conv1x1_kernel<MTW, NT, true>", 3, 4, 1)]),
    # ---- resident-patch kernel
    ("res1_mtp2", (2, 32, 13, 37, 24, 3, 1, 1), 0, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40, "RES": 1},
     [("conv_mfma_res_kernel<MT>", 1, 1, 1)]),
    ("res1_mtp4", (2, 32, 13, 37, 56, 3, 1, 1), 0, 1, 0.0, 1, {"MSPLIT_PX": 1 << 40, "RES": 1},
     [("conv_mfma_res_kernel<MT>", 1, 1, 1)]),
    ("res1_mtp7", (2, 32, 13, 37, 100, 3, 1, 1), 0, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40, "RES": 1},
     [("conv_mfma_res_kernel<MT>", 1, 1, 1)]),
    ("res1_mtp8", (2, 32, 13, 37, 120, 3, 1, 1), 0, 0, 0.0, 0, {"MSPLIT_PX": 1 << 40, "RES": 1},
     [("conv_mfma_res_kernel<MT>", 1, 1, 1)]),
    ("res2_mtp2", (2, 32, 13, 37, 24, 3, 1, 1), 0, 0, 0.0, 0, {"MSPLIT_PX": 1 << 40, "RES": 2},
     [("conv_mfma_res_kernel<MT>", 2, 1, 1)]),
    ("res2_mtp4", (2, 32, 13, 37, 56, 3, 1, 1), 0, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40, "RES": 2},
     [("conv_mfma_res_kernel<MT>", 4, 1, 1)]),
    ("res2_mtp7", (2, 32, 13, 37, 100, 3, 1, 1), 0, 1, 0.0, 1, {"MSPLIT_PX": 1 << 40, "RES": 2},
     [("conv_mfma_res_kernel<MT>", 7, 1, 1)]),
    ("res2_mtp8", (2, 32, 13, 37, 120, 3, 1, 1), 0, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40, "RES": 2},
     [("conv_mfma_res_kernel<MT>", 8, 1, 1)]),
    ("res2_mtp7_cin112", (2, 112, 13, 37, 100, 3, 1, 1), 0, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40, "RES": 2},
     [("conv_mfma_res_kernel<MT>", 7, 1, 1)]),
    ("res1_mtp4_cin112", (2, 112, 13, 37, 64, 3, 1, 1), 0, 2, 0.2, 1, {"MSPLIT_PX": 1 << 40, "RES": 1},
     [("conv_mfma_res_kernel<MT>", 1, 1, 1)]),
    ("res1_blocks_is_not_resident", (2, 32, 13, 37, 56, 3, 1, 1), 1, 2, 0.2, 2, {"MSPLIT_PX": 1 << 40, "RES": 1},
     [("conv3x3s1_pipe_kernel<MT, 1, true>", 1, 1, 1)]),
    # ---- 16 -> 16 trunk (at least 16384 pixels): band kernel at 2 - 4 workgroups per CU, persistent kernel
    ("c16_band_occ2_chain", (2, 16, 90, 100, 16, 3, 1, 1), 0, 3, 0.0, 0, {"C16_OCC": 2},
     [("conv16_band_kernel", 2, 1, 1)]),
    ("c16_band_occ2_blocks", (2, 16, 90, 100, 16, 3, 1, 1), 1, 2, 0.2, 2, {"C16_OCC": 2},
     [("conv16_band_kernel", 2, 1, 1)]),
    ("c16_band_occ3_chain", (2, 16, 90, 100, 16, 3, 1, 1), 0, 2, 0.2, 2, {"C16_OCC": 3},
     [("conv16_band_kernel", 3, 1, 1)]),
    ("c16_band_occ3_blocks", (2, 16, 90, 100, 16, 3, 1, 1), 1, 3, 0.0, 0, {"C16_OCC": 3},
     [("conv16_band_kernel", 3, 1, 1)]),
    ("c16_band_occ4_chain", (2, 16, 90, 100, 16, 3, 1, 1), 0, 3, 0.0, 2, {"C16_OCC": 4},
     [("conv16_band_kernel", 4, 1, 1)]),
    ("c16_band_occ4_blocks", (2, 16, 90, 100, 16, 3, 1, 1), 1, 2, 0.2, 2, {"C16_OCC": 4},
     [("conv16_band_kernel", 4, 1, 1)]),
    ("c16_persistent_chain", (2, 16, 90, 100, 16, 3, 1, 1), 0, 2, 0.2, 2, {"C16_OCC": 0},
     [("conv16_persistent_kernel", 1, 1, 1)]),
    ("c16_persistent_blocks", (2, 16, 90, 100, 16, 3, 1, 1), 1, 3, 0.0, 0, {"C16_OCC": 0},
     [("conv16_persistent_kernel", 1, 1, 1)]),
    ("c16_persistent_3wgs_chain", (2, 16, 90, 100, 16, 3, 1, 1), 0, 3, 0.0, 0, {"C16_OCC": 0, "C16_WGS": 3},
     [("conv16_persistent_kernel", 1, 1, 1)]),
    ("c16_persistent_3wgs_blocks", (2, 16, 90, 100, 16, 3, 1, 1), 1, 2, 0.2, 2, {"C16_OCC": 0, "C16_WGS": 3},
     [("conv16_persistent_kernel", 1, 1, 1)]),
    ("c16_off_chain", (2, 16, 90, 100, 16, 3, 1, 1), 0, 2, 0.2, 2, {"C16": 0},
     [("conv_mfma_kernel<MT, NT, TW16>", 1, 2, 1)]),
    # ---- row split of a large plane: whole rounds on 8x32 tiles, the remaining rows on 4x16 tiles
    ("rowsplit_chain", (1, 16, 264, 520, 112, 3, 1, 1), 0, 2, 0.2, 2, {},
     [("conv3x3s1_wave_kernel<MT, 2>", 7, 4, 2), ("conv3x3s1_pipe_kernel<MT>", 7, 1, 1)]),
    ("rowsplit_blocks", (1, 16, 264, 520, 112, 3, 1, 1), 1, 2, 0.2, 1, {},
     [("conv3x3s1_blocks_tileouter_kernel", 7, 4, 2), ("conv3x3s1_pipe_kernel<MT, 1, true>", 7, 1, 1)]),
    ("rowsplit_off_chain", (1, 16, 264, 520, 112, 3, 1, 1), 0, 0, 0.0, 0, {"SPLIT": 0},
     [("conv3x3s1_pipe_kernel<MT>", 7, 1, 1)]),
    # ---- 1x1 GEMM kernel: cout tiles per wave 1 - 4, 32- and 64-pixel workgroups; reduce rule 32; rule blocks goes elsewhere
    ("gemm1x1_nt2_cout256", (1, 32, 129, 130, 256, 1, 1, 0), 0, 2, 0.2, 2, {}, [("conv1x1_kernel<MTW, NT>", 4, 2, 1)]),
    ("gemm1x1_nt2_cout192", (1, 32, 129, 130, 192, 1, 1, 0), 0, 1, 0.0, 1, {}, [("conv1x1_kernel<MTW, NT>", 3, 2, 1)]),
    ("gemm1x1_nt2_cout112", (1, 32, 129, 130, 112, 1, 1, 0), 0, 0, 0.0, 0, {}, [("conv1x1_kernel<MTW, NT>", 2, 2, 1)]),
    ("gemm1x1_nt4_cout250", (2, 32, 129, 130, 250, 1, 1, 0), 0, 2, 0.2, 2, {}, [("conv1x1_kernel<MTW, NT>", 4, 4, 1)]),
    ("gemm1x1_nt4_cout180", (2, 32, 129, 130, 180, 1, 1, 0), 0, 0, 0.0, 0, {}, [("conv1x1_kernel<MTW, NT>", 3, 4, 1)]),
    ("gemm1x1_nt4_cout100", (2, 32, 129, 130, 100, 1, 1, 0), 0, 2, 0.2, 2, {}, [("conv1x1_kernel<MTW, NT>", 2, 4, 1)]),
    ("gemm1x1_tiny_plane_cout112", (2, 32, 9, 7, 112, 1, 1, 0), 0, 2, 0.2, 2, {},
     [("conv1x1_kernel<MTW, NT>", 1, 2, 1)]),
    ("gemm1x1_tiny_plane_cout100", (2, 32, 9, 7, 100, 1, 1, 0), 0, 1, 0.0, 1, {},
     [("conv1x1_kernel<MTW, NT>", 1, 2, 1)]),
    ("gemm1x1_reduce32_nt2_cout64", (1, 64, 129, 130, 64, 1, 1, 0), 32, 2, 0.2, 2, {},
     [("conv1x1_kernel<MTW, NT, true>", 1, 2, 1)]),
    ("gemm1x1_reduce32_nt2_cout112", (1, 64, 129, 130, 112, 1, 1, 0), 32, 1, 0.0, 1, {},
     [("conv1x1_kernel<MTW, NT, true>", 2, 2, 1)]),
    ("gemm1x1_reduce32_nt2_cout192", (1, 64, 129, 130, 192, 1, 1, 0), 32, 0, 0.0, 0, {},
     [("conv1x1_kernel<MTW, NT, true>", 3, 2, 1)]),
    ("gemm1x1_reduce32_nt2_cout256", (1, 64, 129, 130, 256, 1, 1, 0), 32, 2, 0.2, 2, {},
     [("conv1x1_kernel<MTW, NT, true>", 4, 2, 1)]),
    ("gemm1x1_reduce32_nt4_cout250", (2, 64, 129, 130, 250, 1, 1, 0), 32, 2, 0.2, 2, {},
     [("conv1x1_kernel<MTW, NT, true>", 4, 4, 1)]),
    ("gemm1x1_reduce32_nt2_cout100", (1, 64, 129, 130, 100, 1, 1, 0), 32, 2, 0.2, 2, {},
     [("conv1x1_kernel<MTW, NT, true>", 2, 2, 1)]),
    ("gemm1x1_blocks_takes_the_tap_kernels", (2, 32, 13, 37, 112, 1, 1, 0), 1, 2, 0.2, 2, {},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 1, 1, 1)]),
    ("gemm1x1_blocks_large_plane", (1, 32, 129, 130, 100, 1, 1, 0), 1, 1, 0.0, 1, {"MSPLIT_PX": 0},
     [("conv_mfma_bsum_kernel<MT, NT, TW16>", 7, 1, 1)]),
    ("gemm1x1_below_min_tiles", (2, 32, 13, 37, 56, 1, 1, 0), 0, 2, 0.2, 2, {"MSPLIT_PX": 0},
     [("conv_mfma_pipe_kernel<MT, NT, TW16, 6>", 4, 1, 1)]),]

# ---- rows on special data, derived from the rows above ---------------------------------------------------------------------
# DATA: row id -> "zeros" | "subnormal" | "nobias"; a row without an entry runs on the ordinary data of case_data.
#   zeros      the data of valu_conv_census.case_data(..., data="zeros"): column patches of -0, +0, -2^-149 and ordinary
#              values, weights in [0.25, 0.375), bias -0 — a -0 accumulator next to the padding, where "multiply the padded
#              zero in" (the oracle's dense convolution, and every kernel here) differs from "skip the tap", and where a
#              padded k-step, a padded cout row or a masked halo slot shows.  No residual adds: they would bury the zeros.
#   subnormal  every product and every sum subnormal
#   nobias     ordinary data, bias = None
# One zero, one no-bias and one subnormal row per (launched expressions, rule) of the table, each on the geometry, knobs and activation of the first row of the table that launches them with an activation that
# keeps the sign of a zero (none / relu / leaky; the dispatcher looks at the activation).  The generic kernels are the only
# ones that take Cin % 16 != 0: they get zero rows at Cin = 8 and Cin = 20, where the last k-step is padded.
DATA = {}
N_BASE = len(CENSUS)


def _derive():
    first = {}
    for r in sorted(CENSUS, key=lambda r: r[3] > 2):                       # stable: rows with act <= leaky first
        exprs = tuple(e[0] for e in r[7])
        first.setdefault((exprs, r[2]), r)
    rows = []
    for (exprs, rule), r in first.items():
        rows.append((r[0] + "__zeros", r[1], rule, r[3] if r[3] <= 2 else 0, r[4], 0, r[6], r[7]))
        DATA[rows[-1][0]] = "zeros"
        rows.append((r[0] + "__nobias", r[1], r[2], r[3], r[4], r[5], r[6], r[7]))
        DATA[rows[-1][0]] = "nobias"
        rows.append((r[0] + "__subnormal", r[1], r[2], r[3] if r[3] <= 2 else 0, r[4], 0, r[6], r[7]))
        DATA[rows[-1][0]] = "subnormal"
    for rid in ("gen_nt1_cin8_chain_mt2", "gen_nt1_cin8_blocks_mt7", "gen_nt4_cin8_chain_mt2", "gen_nt2_cin8_blocks_mt7"):
        r = next(q for q in CENSUS if q[0] == rid)
        for cin in (8, 20):
            g = (r[1][0], cin) + r[1][2:]
            rows.append((f"{rid}__zeros_cin{cin}", g, r[2], r[3], r[4], 0, r[6], r[7]))
            DATA[rows[-1][0]] = "zeros"
    return rows


CENSUS += _derive()

# Instantiations the library holds that no knob setting reaches: (kernel expression, MT, NT, excluding condition).
# dispatch_tile<8> calls launch<8, 4, 2> behind run-time conditions, so these kernels are compiled, but every such call
# sits behind `MTP < 8` (the forced NT = 4 and the large-plane branch alike), and the cout-split path launches MT = 1.
# (launch<8, 4, 2> under a block rule forwards to launch<8, 2, 1>, and its 7x7 and single-buffer wave forms are
# `if constexpr (MT <= 4)`: no further instantiation hangs off it.)
_MTP8 = "dispatch_tile: NT = 4 is taken only when MTP < 8"
UNREACHABLE = [
    ("conv3x3s1_wave_kernel<MT, 2>", 8, 4, _MTP8),
    ("conv_mfma_wave_kernel<MT, 7>", 8, 4, _MTP8),
    ("conv_mfma_pipe_kernel<MT, NT, TW16, 6>", 8, 4, _MTP8),
    ("conv_mfma_pipe_kernel<MT, NT, TW16, 9>", 8, 4, _MTP8),
    ("conv_mfma_kernel<MT, NT, TW16>", 8, 4, _MTP8),
]

# kernels that exist for Cout = 16 only: no partial cout tile to test
WHOLE_TILE_ONLY = {"conv16_band_kernel", "conv16_persistent_kernel"}

_PART = re.compile(r"^(.*) \[MT=(\d+) NT=(\d+) TW16=(\d+)\] grid \d+x\d+x\d+$")


def strip_parens(expr):
    """'(kernel<A, B>)' -> 'kernel<A, B>': a templated kernel is parenthesised where it is a macro argument"""
    expr = expr.strip()
    return expr[1:-1].strip() if expr.startswith("(") and expr.endswith(")") else expr


def parse_launch(s):
    """'expr [MT=7 NT=4 TW16=2] grid 2x1x1 + ...' (pmctf_conv2d_last_launch) -> [(expr, MT, NT, TW16), ...]"""
    keys = []
    for part in s.split(" + "):
        m = _PART.match(part)
        if m is None:
            raise ValueError(f"not a launch record: {part!r} in {s!r}")
        keys.append((strip_parens(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4))))
    return keys


def row(rid):
    return next(r for r in CENSUS if r[0] == rid)


def out_hw(geometry):
    N, Cin, H, W, Cout, K, S, pad = geometry
    return (H + 2 * pad - K) // S + 1, (W + 2 * pad - K) // S + 1


def case_data(r, amplitude=3.0):
    """(x, w, b, [residuals]) of a row, NCHW / OIHW float32, seeded from the row id: x = normal * 3, w = normal * 0.05,
    b = normal, residuals = normal — the law under which the oracle's summation rules differ in 70 - 96 % of the elements.
    Rows named in DATA: the zero / subnormal data of valu_conv_census.case_data (one generator for both censuses), or no
    bias (b = None)."""
    rid, (N, Cin, H, W, Cout, K, S, pad), rule, act, slope, nres, knobs, expected = r
    kind = DATA.get(rid, "normal")
    if kind in ("zeros", "subnormal"):
        import valu_conv_census as vc
        d = vc.case_data((rid, "dense", (N, Cin, H, W, Cout, K, K, S, pad, pad), rule, act, slope, nres, True, None, None,
                          {"data": kind}))
        return d["x"], d["w"], d["b"], d["res"]
    g = np.random.default_rng(zlib.crc32(rid.encode()))
    x = g.standard_normal((N, Cin, H, W), dtype=np.float32) * np.float32(amplitude)
    w = g.standard_normal((Cout, Cin, K, K), dtype=np.float32) * np.float32(0.05)
    b = g.standard_normal(Cout, dtype=np.float32)
    Ho, Wo = out_hw(r[1])
    res = [g.standard_normal((N, Cout, Ho, Wo), dtype=np.float32) for _ in range(nres)]
    return x, w, (None if kind == "nobias" else b), res


def skipping_conv(x, w, b, S, pad, rule):
    """the convolution as a kernel that SKIPS the taps outside the image would compute it (what the depthwise oracle does,
    and what no dense kernel may do), from the oracle itself.  Skipping a tap is adding a product of -0, the one addend that
    changes no accumulator (+0 + -0 = +0, -0 + -0 = -0): with the positive weights of the zero data that is the oracle's
    convolution, without padding, of the image extended by pixels of -0."""
    from pmctf_oracle import clib
    assert (w > 0).all()
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)), constant_values=np.float32(-0.0))
    assert pad == 0 or np.signbit(xp[0, 0, 0, 0])
    return clib.conv2d(xp, w, b, S, (0, 0), rule)


# ---- zero data through the per-class padding of pmctf_conv2d_nhwc_geom_f32 ---------------------------------------------------
# ops.conv_at_class evaluates a 'same' 3x3 convolution at the positions (2i + py, 2j + px) of one parity class: stride 2,
# top / left padding 1 - py / 1 - px, so class 0 has a halo above and to the left only and class 3 below and to the right
# only — one edge where a zero of the padding is multiplied in and one where there is none.
# (id, (N, Cin, H, W, Cout), rule): a small plane (the cout-split path) and the 2x130x130 plane of the s2_whole exception
# (at least 8 000 output pixels and 7 cout tiles: the stride-2 pipelined kernel with every cout tile per workgroup).
GEOM_ZERO = [(f"geom_{name}_rule{rule}", g, rule) for name, g in (("small", (2, 32, 14, 38, 24)), ("s2_whole", (2, 16, 130, 130, 112)))
             for rule in (0, 1)]


def geom_zero_data(case):
    """(x, w, b) of a GEOM_ZERO case: the zero data of the censuses' one generator, its three patches repeated on the
    last columns, so that the right edge (padded by the odd-column classes only) lies in zeros too: in the -2^-149 patch,
    the one that shows a padded last tap where the chain starts at +0"""
    import valu_conv_census as vc
    rid, (N, Cin, H, W, Cout), rule = case
    d = vc.case_data((rid, "dense", (N, Cin, H, W, Cout, 3, 3, 1, 1, 1), rule, 0, 0.0, 0, True, None, None, {"data": "zeros"}))
    x, p = d["x"], vc.zero_patches(3)[2][1]
    assert W >= 3 * p
    x[..., W - p:] = x[..., :p]
    return x, d["w"], d["b"]


def geom_zero_reference(case):
    """-> ({cls: the oracle's full convolution at the positions of the class}, {cls: the same from a kernel that skipped the
    taps outside the image})"""
    from pmctf_oracle import clib
    x, w, b = geom_zero_data(case)
    full, skipped = clib.conv2d(x, w, b, 1, (1, 1), case[2]), skipping_conv(x, w, b, 1, 1, case[2])
    cut = lambda y, cls: np.ascontiguousarray(y[:, :, (cls >> 1)::2, (cls & 1)::2])
    return {cls: cut(full, cls) for cls in range(4)}, {cls: cut(skipped, cls) for cls in range(4)}
