/* pmctf_hip.h — C ABI of libpmctf_hip.so: the gfx950 (MI355X) kernels behind the
 * pMCTF temporal-decomposition encode path.
 *
 * Every entry point replaces one torch functional op (or a fixed group of them)
 * that the reference's hot path calls; the reference file:line is given per
 * function.  Signatures use plain pointers and sizes only.  All pointers are
 * DEVICE pointers unless said otherwise; `stream` is a hipStream_t passed as
 * void*.  Nothing allocates or synchronises; launches are asynchronous on
 * `stream`.  Return value: 0 on success, negative on a rejected shape
 * (PMCTF_EINVAL) or a HIP launch error (PMCTF_ELAUNCH).
 *
 * Layout: feature maps are NHWC ("channels last") float32, dense.  Single-channel
 * planes (frames, subbands, flow components) are therefore identical to the
 * reference's NCHW tensors.  Arithmetic follows the PM-F32 spec in DESIGN.md:
 * IEEE binary32, one rounding per stated operation, convolution sums as an
 * ordered fmaf chain (exactly what v_mfma_f32_16x16x4_f32 computes).
 */
#ifndef PMCTF_HIP_H
#define PMCTF_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PMCTF_OK 0
#define PMCTF_EINVAL (-1)
#define PMCTF_ELAUNCH (-2)

/* activation codes for conv epilogues / elementwise maps */
/* Summation rule of a convolution (the argument `sum_rule`): the ORDER in which the products of one output element are
 * added, which fixes its last bits.  Both are k-ordered fmaf chains over 16-channel blocks of the input, (ky, kx, ci)
 * ascending inside a block:
 *   PMCTF_SUM_CHAIN   acc = bias, then one chain through all blocks.  What ATen's CPU path computes for the 1x1 layers of
 *                     the path whose reduction is one block (oneDNN jit_1x1) and for depthwise layers.
 *   PMCTF_SUM_BLOCKS  every block a chain from zero, S_0 .. S_last; result (..((S_0 + bias) + S_1) + ..) + S_last.  What
 *                     ATen's CPU path (oneDNN direct convolution) computes for every KH*KW > 1 layer, measured bit for bit
 *                     (tools/aten_conv_rules.py).  The drop-in path uses it for every KH*KW > 1 layer with at most 16 input
 *                     channels and for the multi-block layers of the signal path (motion estimation, motion codec, temporal
 *                     and spatial lifting): the layers whose last bits decide symbols (profiles/round4_flip_attribution.md).
 *   B >= 16, B % 16 == 0 ("reduce-B", entry points with an MFMA path only): blocks of B input channels; the FIRST block's
 *                     chain starts at the bias, later blocks at zero, block results added in turn (B >= Cin is the chain).
 *                     What ATen's jit_1x1 kernel computes for the 1x1 layers whose reduction it blocks; B follows from the
 *                     layer's shape (pMCTF/hip/aten_rules.py, e.g. 256 -> 64 on a 576x960 plane: B = 96).
 *   PMCTF_SUM_GEMM    (pmctf_conv2d_smallcin_f32 only) ONE chain from zero over (ci, ky, kx), bias added last: ATen's
 *                     im2col + sgemm path, which it takes instead of oneDNN for a single image of at most 20 480 input
 *                     elements and filters up to 3x3 (Convolution.cpp use_mkldnn).  With one input channel it equals BLOCKS.
 */
#define PMCTF_SUM_CHAIN 0
#define PMCTF_SUM_BLOCKS 1
#define PMCTF_SUM_GEMM 2
/* (pmctf_conv2d_smallcin_f32 only; Cin = 1, 3x3) the same path with ONE output channel is a matrix-vector product over the
 * nine im2col columns p_k = x_k * w_k (k = 3 ky + kx); MKL's kernel sums eight at a time in four chains, the ninth after:
 *   E = fma(p4, fma(p6, bias));  O = fma(p5, round(p7));  A = fma(p0, round(p2)) + fma(p1, round(p3));  y = fma(p8, (E + O) + A)
 * (measured with probe inputs: tools/aten_gemv_probe.py; the 1 -> 1 "lower_level_subband" layer on planes <= 20 480 px) */
#define PMCTF_SUM_GEMV_3X3 3

#define PMCTF_ACT_NONE 0
#define PMCTF_ACT_RELU 1    /* nn.ReLU                 video_net.py:77      */
#define PMCTF_ACT_LEAKY 2   /* nn.LeakyReLU(slope)     video/layers.py:57-60, context_fusion_4step.py:13 */
#define PMCTF_ACT_TANH 3    /* torch.tanh              lifting_1d.py:39,42  */
#define PMCTF_ACT_SIGMOID 4 /* torch.sigmoid           long_context.py:24   */

/* Number of floats pmctf_conv2d_pack_weights() writes for a (Cout,Cin,KH,KW) filter. */
int64_t pmctf_conv2d_packed_size(int Cout, int Cin, int KH, int KW);

/* HOST-side re-layout of an OIHW float filter + bias into the MFMA A-fragment
 * order consumed by pmctf_conv2d_nhwc_f32 (both pointers are host pointers).
 * bias_packed receives pmctf_conv2d_packed_bias_size(Cout) floats (zero padded). */
int pmctf_conv2d_pack_weights(const float *w_oihw, const float *bias, int Cout, int Cin, int KH, int KW,
                              float *w_packed, float *bias_packed);
int64_t pmctf_conv2d_packed_bias_size(int Cout);

/* Launch-shape tuning of pmctf_conv2d_nhwc*_f32 (never changes results, only how the work is cut into workgroups).
 * Names (also read once from the environment as PMCTF_CONV_<NAME>): "WAVE" 0/1 wave-private kernel, "NT" force 1/2/4
 * pixel segments per wave, "MSPLIT_PX" planes with at most this many output pixels run one cout tile per workgroup,
 * "SPLIT" 0/1 cut the partial last round of 8x32 tiles into 4x16 tiles, "BIGPX" smallest plane given 8x32 tiles,
 * "V1"/"V2" force the single-buffer / pipelined kernel, "RES" 0/1/2 resident-patch kernel for the
 * cout-split planes (off / one cout tile / all cout tiles per workgroup), "MSPLIT_NT" 1/2/4 tile rows per wave on the
 * cout-split planes, "C16" 0/1 persistent 16->16 kernel with "C16_WGS" workgroups at most, "NBUF1" 0/1 single patch buffer
 * (three workgroups per CU) for the wave-private kernel on layers of at most 64 couts, "K33" 0/1 the 3x3 stride-1
 * specialisations (wave-private and pipelined kernels, stride 1 and 2: no vector-ALU work in the tap loop), "K77" 0/1 the
 * 7x7 stride-1 pipelined kernel (8x32 and 4x16 tiles), "K33_SMALL" 0/1 the specialised 3x3 pipelined kernel with one cout
 * tile per workgroup on the cout-split planes the wave-private kernel does not take, "K11" 0/1 the flat GEMM kernel for 1x1 layers with at least "K11_MIN_TILES" (7) 16-cout tiles, "WAVE_SMALL" 0/1 the
 * wave-private kernel with one cout tile per workgroup on cout-split 3x3 planes that fill the waves' 4x16 tiles to >= 90 %,
 * "BSUM_TILEOUTER" 0/1 rule "blocks" 3x3 layers of 7 cout tiles on 8x32 tiles: one launch of the tile-outer kernel (1) or
 * the 4 + 3 tiles in two launches of the wave-private kernel (0).
 * Environment only: PMCTF_FEWCOUT_LDS=0 / PMCTF_DWCONV_COLUMN=0 select the older one/two-cout and depthwise kernels. */
int pmctf_conv2d_set_option(const char *name, long value);
/* current value of a knob (-1: unknown name).  The launch plans of the drop-in path record their convolutions with
 * "SPLIT" = 0: luma's and chroma's coders run side by side there, the other stream fills the tail of a launch, and
 * cutting a launch into whole rounds + remainder only adds launches (5.41 -> 5.49 frames/s on the 1080p GOP-16 encode);
 * on a single stream the cut pays (the default). */
long pmctf_conv2d_get_option(const char *name);
/* Measurement aid (no reference counterpart): which kernel(s) the LAST pmctf_conv2d_nhwc[_geom]_f32 call of the calling
 * thread launched — kernel expression, tile parameters and grid, several joined by " + " when the launch was cut
 * (whole rounds of workgroups + remainder).  bench.py names the kernel behind its roofline figure from this. */
int pmctf_conv2d_last_launch(char *buf, int capacity);

/* nn.Conv2d forward (groups=1, zero padding), optionally fused with what follows it
 * in the reference: y = act(conv(x) + bias) [+ res1] [+ res2].
 *   reference: F.conv2d behind every nn.Conv2d on the path, e.g.
 *   pMCTF/layers/video/video_net.py:78-90 (SpyNet 7x7), pMCTF/layers/context_fusion_4step.py:12-20
 *   (ContextResidual), pMCTF/layers/postprocessing.py:9-18,35-44, pMCTF/layers/long_context.py:13-14,
 *   pMCTF/layers/video/layers.py:22-136, pMCTF/layers/context_fusion.py:56-128 (masked filters are
 *   multiplied by their mask at pack time, layers.py:49-51).
 * x: [N,H,W,Cin]  y/res1/res2: [N,Ho,Wo,Cout], Ho=(H+2*pad_h-KH)/stride+1.  Cin % 4 == 0.
 * Sum order per output: bias, then 16-channel chunks (ky,kx raster inside a chunk, channel ascending). */
int pmctf_conv2d_nhwc_f32(const float *x, const float *w_packed, const float *bias_packed,
                          const float *res1, const float *res2, float *y,
                          int N, int H, int W, int Cin, int Cout, int KH, int KW,
                          int stride, int pad_h, int pad_w, int act, float slope, void *stream);

/* The same call with the summation rule (above; pmctf_conv2d_nhwc_f32 is PMCTF_SUM_CHAIN) and the launch-shape options of
 * THIS launch handed over as arguments instead of read from the
 * process-wide knobs (a field < 0, or opts == NULL, takes the knob of that name): "split" = "SPLIT", "msplit_px" =
 * "MSPLIT_PX" above.  The captured launch plans of the drop-in path record their convolutions with their own values
 * (two coders side by side fill each other's launch tails), and do so per launch: nothing process-wide changes while a
 * plan is recorded, so a second model on another host thread keeps its own launch shapes.  Results never depend on them. */
typedef struct pmctf_conv_launch_opts {
    long split;      /* 0/1: cut the partial last round of 8x32 tiles into 4x16 tiles; < 0: process-wide knob */
    long msplit_px;  /* planes with at most this many output pixels run one cout tile per workgroup; < 0: knob */
} pmctf_conv_launch_opts;
int pmctf_conv2d_nhwc_opts_f32(const float *x, const float *w_packed, const float *bias_packed,
                               const float *res1, const float *res2, float *y,
                               int N, int H, int W, int Cin, int Cout, int KH, int KW,
                               int stride, int pad_h, int pad_w, int act, float slope, int sum_rule,
                               const pmctf_conv_launch_opts *opts, void *stream);

/* Explicit-geometry form: output size (Ho,Wo) and top/left padding given by the caller; taps falling outside the
 * input read zero.  Used to evaluate a stride-1 convolution only at one 2x2 parity class of positions
 * (stride 2, pad = 1 - parity): the four-step coder needs the last ContextResidual conv and the 1x1 parameter head of
 * each step only where that step's mask is set (context_fusion_4step.py:127-137,160-189), a quarter of the plane. */
int pmctf_conv2d_nhwc_geom_f32(const float *x, const float *w_packed, const float *bias_packed,
                               const float *res1, const float *res2, float *y,
                               int N, int H, int W, int Cin, int Cout, int KH, int KW,
                               int stride, int pad_top, int pad_left, int Ho, int Wo, int act, float slope,
                               void *stream);

int pmctf_conv2d_nhwc_geom_opts_f32(const float *x, const float *w_packed, const float *bias_packed,
                                    const float *res1, const float *res2, float *y,
                                    int N, int H, int W, int Cin, int Cout, int KH, int KW,
                                    int stride, int pad_top, int pad_left, int Ho, int Wo, int act, float slope,
                                    int sum_rule, const pmctf_conv_launch_opts *opts, void *stream);

/* Same contract for Cin <= 4 (any Cin >= 1), plain OIHW weights on the device: direct convolution on the vector ALU
 * (first layers: PredictUpdate conv1 1->16 lifting_1d.py:38; PostProcess conv1 1->64 postprocessing.py:35; four-step
 * y_spatial_prior_k.0 1->112 and conv1_context 1|2->112 context_fusion_4step.py:48,63,73,83; masked 1->128
 * context_fusion.py:79; MV encoder first conv 2->64 video_net.py:128).  In this entry point and the two below a tap outside
 * the image is a zero that is multiplied in (fmaf(+0, w, acc), which turns an accumulator of -0 into +0 for w > 0), as
 * in the zero-padded copy the specification convolves (tests/valu_conv_census.py, the zero rows). */
int pmctf_conv2d_smallcin_f32(const float *x, const float *w_oihw, const float *bias,
                              const float *res1, const float *res2, float *y,
                              int N, int H, int W, int Cin, int Cout, int KH, int KW,
                              int stride, int pad_h, int pad_w, int act, float slope, int sum_rule, void *stream);

/* PredictUpdate conv1 (pMCTF/layers/lifting_1d.py:38,44-45): 3x3, stride 1, pad 1, one input channel, Cout = 16
 * (other Cout: PMCTF_EINVAL).  y = conv(x); if y2 != NULL also y2 = act2(conv(x)) — the block needs both conv1 and
 * tanh(conv1).  x [N,H,W] plane, w OIHW on the device, y/y2 [N,H,W,16]. */
int pmctf_conv3x3_cin1_dual_f32(const float *x, const float *w_oihw, const float *bias, float *y, float *y2,
                                int N, int H, int W, int Cout, int act2, float slope, int sum_rule, void *stream);

/* KxK, stride 1, pad K/2, one or two output channels (PredictUpdate conv4 16->1 lifting_1d.py:41, PostProcess 64->1,
 * SpyNet 16->2 7x7): vector-ALU kernel, plain OIHW weights on the device, same sum order as pmctf_conv2d_nhwc_f32.
 * pmctf_conv2d_fewcout_supported() tells which (Cin, Cout, K) exist; others return PMCTF_EINVAL. */
int pmctf_conv2d_fewcout_supported(int Cin, int Cout, int K);
int pmctf_conv2d_fewcout_f32(const float *x, const float *w_oihw, const float *bias, const float *res1,
                             const float *res2, float *y, int N, int H, int W, int Cin, int Cout, int K,
                             int act, float slope, int sum_rule, void *stream);

/* depthwise KxK conv, stride 1, pad K/2 (pMCTF/layers/video/layers.py:117-118); x,y [N,H,W,C], w [C,1,K,K].  Here a tap
 * outside the image is skipped, not multiplied in as a zero: an accumulator of -0 stays -0 beside the border. */
int pmctf_dwconv2d_nhwc_f32(const float *x, const float *w, const float *bias, float *y,
                            int N, int H, int W, int C, int K, void *stream);

/* Measurement aid (no reference counterpart): which kernel the LAST call of pmctf_conv2d_smallcin_f32,
 * pmctf_conv3x3_cin1_dual_f32, pmctf_conv2d_fewcout_f32 or pmctf_dwconv2d_nhwc_f32 on the calling thread launched: the
 * launch expression with its template arguments and the grid, e.g. "conv_smallcin_reg_kernel<3, 2> grid 140"; empty
 * when that call refused its arguments.  Host text only: no launch, no synchronisation, no allocation.
 * tests/valu_conv_census.py names the kernel every row must reach. */
int pmctf_valu_conv_last_launch(char *buf, int capacity);

/* flow_warp / torch_warp (pMCTF/layers/video/video_net.py:32-55): bilinear grid_sample,
 * border padding, align_corners=True.  im,out: [N,C,H,W] planar; flow: [flowN,2,H,W] planar
 * (flowN = 1 broadcasts over N, pMCTF_L.py:299-300); lin_x[W], lin_y[H] are the cached
 * linspace(-1,1,.) tables of video_net.py:36-40.  flow_sign = -1 warps with -flow (pMCTF_L.py:307). */
int pmctf_flow_warp_f32(const float *im, const float *flow, const float *lin_x, const float *lin_y,
                        float *out, int N, int C, int H, int W, int flowN, float flow_sign, void *stream);

/* F.avg_pool2d(k=2,s=2) on NC planes (video_net.py:106-108): 0 + ((((0 + a00) + a01) + a10) + a11) / 4, never -0 */
int pmctf_avgpool2_f32(const float *x, float *y, int NC, int H, int W, void *stream);
/* F.interpolate bilinear x2, align_corners=False, result times `scale` (video_net.py:58-63,114) */
int pmctf_bilinear_up2_f32(const float *x, float *y, int NC, int H, int W, float scale, void *stream);
/* F.interpolate bilinear /2, align_corners=False, result divided by `div` (video_net.py:66-71; pMCTF_L.py:317,401) */
int pmctf_bilinear_down2_f32(const float *x, float *y, int NC, int H, int W, float div, void *stream);
/* the same two for factor 2, 4 or 8: bilinearupsacling / bilineardownsacling(x, factor) of the me_downsample paths
 * (video_net.py:58-71; pMCTF_L.py:255-257,274-275,456-458,475-476,516-517) */
int pmctf_bilinear_up_f32(const float *x, float *y, int NC, int H, int W, int factor, float scale, void *stream);
int pmctf_bilinear_down_f32(const float *x, float *y, int NC, int H, int W, int factor, float div, void *stream);

/* ---- elementwise / layout family -------------------------------------------------------------
 * One strided kernel covers the reference's glue tensor ops (torch add/sub/mul/div, slicing, cat,
 * chunk, permute, tile, clamp, round, leaky_relu).  Operands are 4-D views (n,c,h,w) given by element
 * strides so[4]/sa[4]/sb[4] (HOST pointers to int64[4]; 0 = broadcast); b may be NULL.  cfast != 0
 * iterates c fastest (NHWC outputs), else w fastest (planar outputs).  One IEEE rounding per written
 * operation, never fused. */
#define PMCTF_EW_COPY 0              /* a                                                        */
#define PMCTF_EW_ADD 1               /* a + b            e.g. L = ref + inv, pMCTF_L.py:311       */
#define PMCTF_EW_SUB 2               /* a - b            e.g. H = cur - pred, pMCTF_L.py:305      */
#define PMCTF_EW_MUL 3               /* a * b                                                    */
#define PMCTF_EW_DIV 4               /* a / b                                                    */
#define PMCTF_EW_MULS 5              /* a * alpha        e.g. out * quant_step, video_net.py:143  */
#define PMCTF_EW_DIVS 6              /* a / alpha        e.g. subband / QP, pWave.py:199          */
#define PMCTF_EW_ADD_MULS 7          /* a + b*alpha                                              */
#define PMCTF_EW_SUB_MULS 8          /* a - b*alpha                                              */
#define PMCTF_EW_ADD_MULS_MULS 9     /* (a + b*alpha)*beta   predict/update_filter, wavelet_transform_temporal_mctf.py:27-45 */
#define PMCTF_EW_CLAMP_MULS 10       /* clamp(a*alpha, -beta, beta)   quantize_subband, pWave.py:184-189 */
#define PMCTF_EW_ROUND_CLAMP_MULS 11 /* round(clamp(a*alpha, -beta, beta))   pWave.py:408        */
#define PMCTF_EW_ROUND 12            /* round half to even (torch.round)                         */
#define PMCTF_EW_LEAKY 13            /* a > 0 ? a : a*alpha                                      */
#define PMCTF_EW_ADD_MULS2 14        /* a + (b*alpha)*beta   lifting step, lifting_1d.py:108-111  */
#define PMCTF_EW_SUB_MULS2 15        /* a - (b*alpha)*beta   inverse lifting, lifting_1d.py:155-160 */
#define PMCTF_EW_ROUND_CLAMP 16      /* round(clamp(a, alpha, beta))   harness, test_pMCTF_flex.py:299-300 */
#define PMCTF_EW_TANH 17             /* PM-F32 tanh(a)        lifting_1d.py:39                     */
#define PMCTF_EW_LAST 17
int pmctf_ew_f32(int op, float *out, const int64_t *so, const float *a, const int64_t *sa, const float *b,
                 const int64_t *sb, int N, int C, int H, int W, float alpha, float beta, int cfast, void *stream);
/* Measurement aid: the kernel the last call of pmctf_ew_f32, pmctf_nearest_up2_nhwc_f32 or pmctf_pixel_shuffle2_nhwc_f32 on
 * the calling thread launched, as the launch expression with its template arguments, " channels" or " rows" for the two
 * forms of ew_c4_kernel, and the grid, e.g. "ew_c4_kernel<int> rows grid 3"; empty when that call refused its arguments.
 * Host text only: no launch, no synchronisation, no allocation.  tests/ew_census.py names the kernel every row must
 * reach. */
int pmctf_ew_last_launch(char *buf, int capacity);

/* SpyNet level input torch.cat([im1, warp(im2), flow_up]) (video_net.py:116-119) for Y-only frames
 * (3 identical channels, pMCTF_L.py:453-454): planes im1[HW], warped[HW], flow_up[2][HW] -> NHWC [HW,8]. */
int pmctf_spynet_pack8_f32(const float *im1, const float *warped, const float *flow_up, float *out, int H, int W,
                           void *stream);
/* AUXILIARY reduced-precision profile of the dense 3x3 'same' stride-1 convolutions (conv_split.hip; SURVEY.md §7 step 5,
 * second variant): bf16-input / f32-accumulate MFMA with both operands split into nsplit bf16 planes (3: ~2^-22 relative
 * per product, 2: ~2^-16, 1: plain bf16).  Same interface and epilogue as pmctf_conv2d_nhwc_f32 (same reference call sites:
 * context_fusion_4step.py:12-20, postprocessing.py:9-18,35-44, context_fusion.py:56-128); NOT bit-exact against the
 * oracle — selected only by HipEngine(precision=...), never by the parity path.  Cin % 16 == 0, Cout in {64, 112}. */
int pmctf_conv3x3_split_supported(int Cin, int Cout);
int64_t pmctf_conv3x3_split_packed_size(int Cout, int Cin, int nsplit);          /* uint16 elements */
int pmctf_conv3x3_split_pack_weights(const float *w_oihw, const float *bias, int Cout, int Cin, int nsplit,
                                     uint16_t *w_packed, float *bias_packed);     /* HOST pointers */
int pmctf_conv3x3_split_f32(const float *x, const uint16_t *w_packed, const float *bias_packed, const float *res1,
                            const float *res2, float *y, int N, int H, int W, int Cin, int Cout, int nsplit, int act,
                            float slope, void *stream);
/* the same arithmetic at stride 2 with explicit geometry (the shape of pmctf_conv2d_nhwc_geom_f32: the quarter-resolution
 * context convolutions of context_fusion_4step.py:176-191, evaluated only at one parity class); 112 couts */
int pmctf_conv3x3_split_geom_f32(const float *x, const uint16_t *w_packed, const float *bias_packed, const float *res1,
                                 const float *res2, float *y, int N, int H, int W, int Cin, int Cout, int nsplit,
                                 int stride, int pad_h, int pad_w, int Ho, int Wo, int act, float slope, void *stream);

/* The whole PredictUpdate CNN of a lifting step as ONE launch (pu_fused.hip): 1->16, 16->16 tanh, 16->16 (+c1), 16->1,
 * 3x3 zero-padded, with the arithmetic around it.  x / other / out: single-channel planes (N,1,H,W).
 *   mode 0 — temporal predict / update filter, pMCTF/layers/wavelet_transform_temporal_mctf.py:27-45:
 *            out = (x + PU(x) * 0.1) * c                                     (c = 1/sqrt2 predict, 0.5 update)
 *   mode 1 — one branch of the iWave lifting step, pMCTF/layers/lifting_1d.py:103-145 (forward) / :147-189 (backward):
 *            skip = conv3x1(reflect_pad_H(x)) + lbias;  out = other + sign * (skip + (PU(skip / 256) * 256) * 0.1)
 * PredictUpdate itself: pMCTF/layers/lifting_1d.py:25-49.  w1/b1, w4/b4: OIHW device filters (16,1,3,3)+(16), (1,16,3,3)+(1);
 * w2/w3: pmctf_conv2d_pack_weights() output for the two (16,16,3,3) layers.  Same sums, same order as the separate
 * launches (pmctf_conv3x3_cin1_dual_f32, pmctf_conv2d_nhwc_f32, pmctf_conv2d_fewcout_f32, pmctf_lift_skip3_f32, pmctf_ew_f32). */
int pmctf_predict_update_fused_f32(const float *x, const float *other, float *out, const float *w1, const float *b1,
                                   const float *w2_packed, const float *b2_packed, const float *w3_packed,
                                   const float *b3_packed, const float *w4, const float *b4, int N, int H, int W, int mode,
                                   float c, float sign, float lw0, float lw1, float lw2, float lbias, int sum_rule,
                                   int skip_sum_rule, void *stream);

/* ReflectionPad2d((0,0,1,1)) + 3x1 conv on NC single-channel planes (lifting_1d.py:98,105-106).  sum_rule: one input
 * channel = one block, so PMCTF_SUM_BLOCKS is "three fmaf from zero, bias last" (ATen's oneDNN path), PMCTF_SUM_CHAIN "bias
 * first" — which is what ATen computes when the padded input of ONE plane has at most 20 480 elements and the reference
 * tensor holds one plane (its im2col + gemv path; Convolution.cpp `use_mkldnn`): the caller passes the rule of the
 * REFERENCE's tensor shape, not of a batch it may have stacked. */
int pmctf_lift_skip3_f32(const float *x, float *y, int NC, int H, int W, float w0, float w1, float w2, float bias,
                         int sum_rule, void *stream);
/* nn.Upsample(scale_factor=2, mode="nearest") on NHWC (context_fusion_4step.py:50, long_context.py:50) */
int pmctf_nearest_up2_nhwc_f32(const float *x, float *y, int N, int H, int W, int C, void *stream);
/* nn.PixelShuffle(2) on NHWC [N,H,W,4C] -> [N,2H,2W,C], optional activation (video/layers.py:34-38,96-104) */
int pmctf_pixel_shuffle2_nhwc_f32(const float *x, float *y, int N, int H, int W, int C, int act, float slope,
                                  void *stream);
/* ConvFFN3 gate: leaky(x1,0.1)+leaky(x2,0.01), x = [x1|x2] NHWC [P,2C] -> [P,C] (video/layers.py:163-167) */
int pmctf_ffn3_mix_f32(const float *x, float *y, int64_t P, int C, void *stream);
/* LSTM2D gates (long_context.py:20-33); xh = conv_in(x)+conv_hidden(h), NHWC [P,C]; cell [P,Ccell], Ccell in {1,C} */
int pmctf_lstm_gates_f32(const float *xh, const float *cell, float *cell_out, float *hid_out, int64_t P, int C,
                         int Ccell, void *stream);
/* The same with torch.sigmoid as ATen evaluates it on the reference's contiguous (ref_planes, C, H, W) gate tensor with
 * aten_threads intra-op threads: whole strides of 32 floats of a thread's slice through SLEEF, the rest of the slice
 * through libm's expf (pm_glibc_expf.h).  HW = H * W; xh holds P / HW planes, ref_planes per reference tensor.
 * aten_threads = 0: no tails (= pmctf_lstm_gates_f32). */
int pmctf_lstm_gates_aten_f32(const float *xh, const float *cell, float *cell_out, float *hid_out, int64_t P, int C,
                              int Ccell, int64_t HW, int ref_planes, int aten_threads, void *stream);

/* ---- quantisation + symbol hand-off --------------------------------
 * sym/idx receive one full-size push (int16 symbol, int16 CDF row) in the reference's flattening order
 * (NCHW), exactly what EntropyCoder.encode_with_indexes is given (entropy_models.py:37-40,269-278). */
/* One step of ContextFusionFourStep.forward(write=True): process_with_mask + build_indexes for parity class k
 * (context_fusion_4step.py:127-137,156-189); x, so_far planes [N,1,H,W].
 * params: NHWC [N,H,W,2] (scale, mean) (params_sub = 0) or, for params computed only at the class-k positions,
 * [N,H/2,W/2,2] (params_sub = 1; H and W even). */
int pmctf_fourstep_quant_f32(const float *x, const float *params, float *so_far, int16_t *sym, int16_t *idx, int N,
                             int H, int W, int k, int params_sub, float log_scale_min, float log_scale_step,
                             void *stream);
/* LL subband, one-shot path of pWave.compress (pWave.py:408-418; CompressionModel.process gaussian_model.py:59-63):
 * ll_hat = round(round(round(ll) - mean) + mean), symbol round(round(ll) - mean), CDF row of scale.
 * planes > 0: push in the order of the sequential coder (_compress_subband_ar, pWave.py:531-555): position-major,
 * plane-minor (total = planes * positions); planes = 0: plane-major NCHW order of the one-shot path (pWave.py:418). */
int pmctf_ll_quant_f32(const float *ll, const float *params, float *ll_hat, int16_t *sym, int16_t *idx, int64_t total,
                       int planes, float log_scale_min, float log_scale_step, void *stream);
/* MV hyper latent (pMCTF_L.py:463-464,478): z_hat = round(z) (NHWC [HW][C]); symbols [C][HW] with CDF row = channel
 * (BitEstimator.build_indexes / encode, entropy_models.py:181-195) */
int pmctf_z_symbols_f32(const float *z, float *z_hat, int16_t *sym, int16_t *idx, int HW, int C, void *stream);
/* step t of MVCoderQuad.forward_four_part_prior(write=True) (four_part_prior.py:89-208): y [HW][64], common [HW][192]
 * (quant step | scales | means, LowerBound 0.5 on the step), sp [HW][128] spatial-prior output (t > 0); writes the
 * step's y_hat contribution into so_far [HW][64] and the 16-channel symbol/row planes [16][HW] */
int pmctf_mv_fourpart_step_f32(const float *y, const float *common, const float *sp, float *so_far, int16_t *sym,
                               int16_t *idx, int H, int W, int t, float log_scale_min, float log_scale_step,
                               void *stream);
/* y_hat = so_far * q_dec with q_dec = max(quant step, 0.5) (four_part_prior.py:194-197; video_net.py:14-20) */
int pmctf_mv_dequant_f32(const float *so_far, const float *common, float *y_hat, int64_t HW, void *stream);

/* ---- decoder side ----------------------------------------------------------------
 * LL subband: pWave._decompress_subband_ar + ContextFusionSubband.forward_sequential (pWave.py:557-584,
 * context_fusion.py:140-204) as one persistent workgroup that evaluates the causal masked-conv network per
 * position and decodes the position's symbols from the rANS stream inside the kernel.
 *   w_packed: pmctf_ll_ar_pack_weights() output on the device; stream_words: the rANS payload (after the 1-byte
 *   header) as little-endian uint32 on the device; (x0,pos0) / state_out[0..1]: Rans64 state and next-word index
 *   before / after (state_out[2] != 0: stream exhausted); cdf/sizes/offsets: the Laplace tables on the device;
 *   ll_out [N][H][W]; scratch_zeroed: pmctf_ll_ar_scratch_floats(N,H,W) floats, zero-filled.  N <= 4
 *   planes per stream (Y 1, UV 2, RGB 3).  pack_weights takes the masked weights of maskedConv1 (w_a,b_a), the five
 *   type-B layers residualBlocks.{0,1}.conv{1,2} + maskedConv2 (w_b,b_b) and convs.{0,1,2} (context_fusion.py:79-135). */
int64_t pmctf_ll_ar_packed_size(void);
int pmctf_ll_ar_pack_weights(const float *w_a, const float *b_a, const float *const *w_b, const float *const *b_b,
                             const float *w_p0, const float *b_p0, const float *w_p1, const float *b_p1,
                             const float *w_p2, const float *b_p2, float *out);      /* HOST pointers */
int64_t pmctf_ll_ar_scratch_floats(int N, int H, int W);
int pmctf_ll_ar_decode_f32(const float *w_packed, const uint32_t *stream_words, int64_t n_words, uint64_t x0,
                           int64_t pos0, const int32_t *cdf, const int32_t *sizes, const int32_t *offsets, int cdf_cols,
                           float log_scale_min, float log_scale_step, float *ll_out, float *scratch_zeroed, int N, int H,
                           int W, uint64_t *state_out, void *stream);
/* The same decode under the summation rules the encoder's one-shot LL network ran with (PMCTF_SUM_*): sum_rule_3x3 for
 * the masked 3x3 layers (CHAIN or BLOCKS), sum_rule_head for convs.0 / convs.1 and sum_rule_head_out for convs.2
 * (CHAIN, or the block size B of "reduce-B", a multiple of 16).  pmctf_ll_ar_decode_f32 = all three CHAIN. */
int pmctf_ll_ar_decode_rules_f32(const float *w_packed, const uint32_t *stream_words, int64_t n_words, uint64_t x0,
                                 int64_t pos0, const int32_t *cdf, const int32_t *sizes, const int32_t *offsets,
                                 int cdf_cols, float log_scale_min, float log_scale_step, float *ll_out,
                                 float *scratch_zeroed, int N, int H, int W, uint64_t *state_out, int sum_rule_3x3,
                                 int sum_rule_head, int sum_rule_head_out, void *stream);
/* Batched row-wise decode: n_jobs independent streams of the SAME geometry (P planes of H x W) in one series of launches,
 * one workgroup per job — per row ONE launch pair for all jobs (2*H launches per batch and plane pass instead of 2*H per
 * stream).  The job table lives in DEVICE memory; the tables, cdf_cols and the scale grid are common to the batch.
 *   state: [0] = Rans64 state, [1] = next word index, [2] = error flag — read on entry AND written on exit, so a job
 *   starts wherever its host decoder stands; a job whose stream runs out sets its own flag, the others are unaffected.
 *   scratch: pmctf_ll_ar_scratch_floats(P, H, W) floats.  sum_rule_3x3 must be PMCTF_SUM_BLOCKS (the row-wise form).
 * plane_order: PMCTF_LL_ORDER_POSITION — the P planes' symbols alternate per position (pWave.compress with
 *   ar_order = True, what pmctf_ll_ar_decode_rules_f32 reads); PMCTF_LL_ORDER_PLANE — all of plane 0, then all of plane 1
 *   (the one-shot order of ar_order = False): the planes are decoded one after the other as single-plane problems, each
 *   continuing from the coder state the previous one left in `state`.  P = 1: the same launches either way.
 * pmctf_ll_ar_batch_form: 0 = the batched form does not cover the geometry (P > 2, or planes too wide for LDS: decode such
 *   streams one by one with pmctf_ll_ar_decode_rules_f32), 1 = one thread per channel, 2 = the two-half row kernel.
 *   decode_batch returns PMCTF_EINVAL where batch_form is 0 or n_jobs > PMCTF_LL_BATCH_MAX_JOBS. */
#define PMCTF_LL_ORDER_POSITION 0
#define PMCTF_LL_ORDER_PLANE 1
#define PMCTF_LL_BATCH_MAX_JOBS 32
typedef struct pmctf_ll_job {
    const float *w_packed;              /* the job's coder: pmctf_ll_ar_pack_weights() output on the device */
    const uint32_t *stream_words;       /* rANS payload words on the device */
    int64_t n_words;
    uint64_t *state;                    /* [3], device */
    float *ll_out;                      /* [P][H][W] */
    float *scratch;
    int32_t sum_rule_3x3, sum_rule_head, sum_rule_head_out, reserved;
} pmctf_ll_job;                         /* 64 bytes */
int pmctf_ll_ar_batch_form(int P, int W, int cdf_cols, int plane_order);
int pmctf_ll_ar_decode_batch_f32(const pmctf_ll_job *jobs_dev, int n_jobs, const int32_t *cdf, const int32_t *sizes,
                                 const int32_t *offsets, int cdf_cols, float log_scale_min, float log_scale_step, int P,
                                 int H, int W, int plane_order, void *stream);
/* Decoder output stage: padded float planes (N,1,Hp,Wp) -> cropped 8-bit planes (N,h,w), rint(clamp(x, 0, 255)) with ties
 * to even (torch.round), NaN -> 0.  h <= Hp, w <= Wp, N*Hp*Wp < 2^31; out at any address.  The uint8_t instantiation of
 * the body of pmctf_planes_to_u16 (csrc/picture_ops.hip). */
int pmctf_planes_to_u8(const float *x, uint8_t *out, int N, int Hp, int Wp, int h, int w, void *stream);
/* ContextFusionFourStep.decompress (context_fusion_4step.py:196-249): CDF rows handed to decode_stream for step k
 * (0 off the mask), then x_hat = (q + mean) on the mask.  params as in pmctf_fourstep_quant_f32. */
int pmctf_fourstep_indexes_f32(const float *params, int16_t *idx, int N, int H, int W, int k, int params_sub,
                               float log_scale_min, float log_scale_step, void *stream);
int pmctf_fourstep_dequant_f32(const int16_t *sym, const float *params, float *so_far, int N, int H, int W, int k,
                               int params_sub, void *stream);
/* MVCoderQuad.decompress_four_part_prior (four_part_prior.py:217-280), step t; idx/sym: [16][H*W] */
int pmctf_mv_fourpart_indexes_f32(const float *common, const float *sp, int16_t *idx, int H, int W, int t,
                                  float log_scale_min, float log_scale_step, void *stream);
int pmctf_mv_fourpart_dequant_f32(const int16_t *sym, const float *common, const float *sp, float *so_far, int H, int W,
                                  int t, void *stream);
/* decoded int16 symbols [C][HW] -> float NHWC [HW][C] (mv_z_hat, pMCTF_L.py:504-505) */
int pmctf_sym_to_nhwc_f32(const int16_t *sym, float *out, int HW, int C, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Estimate-mode forward (pMCTF.forward_one_stage, pMCTF_L.py:332-379; pWave.forward_one_channel, pWave.py:243-312):
 * Laplace / factorized bit ESTIMATES (gaussian_model.py:36-53,65-67) and squared-error sums instead of range coding.
 * Per element: sigma = clamp(s, 1e-5, 1e10); cdf(v) = 0.5 - 0.5*sign(v)*(exp(-|v|/sigma) - 1);
 * bits = max(-log2(cdf(y+0.5) - cdf(y-0.5) + 1e-5), 0) in f32; totals are f64 sums.  Every function ADDS to device
 * doubles the caller has zeroed. */

/* step k of ContextFusionFourStep.forward (context_fusion_4step.py:156-186): writes x_hat at the class-k positions
 * of so_far (zeroes the rest when k == 0) and adds their bits to bits_per_plane[n].  Layouts as pmctf_fourstep_quant_f32. */
int pmctf_fourstep_estimate_f32(const float *x, const float *params, float *so_far, int N, int H, int W, int k,
                                int params_sub, double *bits_per_plane, void *stream);
/* LL subband (pWave.py:255-263): bits of ll_hat - mean (not rounded again) under scale; params [N*HW][2]. */
int pmctf_ll_estimate_f32(const float *ll_hat, const float *params, int N, int64_t HW, double *bits_per_plane,
                          void *stream);
/* MV hyper latent (pMCTF_L.py:262,283; entropy_models.py:72-77,114-122): z_hat = round(z) (NHWC [HW][C]) and the bits
 * of the factorized prior; consts [11][C] = softplus(h) of f1..f4, b of f1..f4, tanh(a) of f1..f3. */
int pmctf_z_estimate_f32(const float *z, float *z_hat, const float *consts, int64_t HW, int C, double *bits,
                         void *stream);
/* step t of MVCoderQuad.forward_four_part_prior (four_part_prior.py:89-195); layouts as pmctf_mv_fourpart_step_f32. */
int pmctf_mv_fourpart_estimate_f32(const float *y, const float *common, const float *sp, float *so_far, int H, int W,
                                   int t, double *bits, void *stream);
/* nn.MSELoss numerator (pMCTF_L.py:351,373; pWave.py:309): sum += sum((a[i]-b[i])^2) */
int pmctf_sqdiff_sum_f32(const float *a, const float *b, int64_t n, double *sum, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Picture quality of one frame, what the evaluation harness reports (test_pMCTF_flex.py:293-327): squared-error sums
 * behind Y-, Cb-, Cr- and RGB-PSNR, and the map means behind MS-SSIM of the rounded RGB pictures.
 *   rec_y (1,1,Hp,Wp), rec_c (2,1,Hp/2,Wp/2): the reconstruction as the temporal synthesis returns it (padded, neither
 *   clamped nor rounded); taken as rint(clamp(v, 0, 255)) (ties to even, NaN -> 0) and cropped to the top-left h x w.
 *   org_y (1,1,h,w), org_c (2,1,h/2,w/2): the un-padded originals (integers).  h, w even; h <= Hp, w <= Wp.
 *   Chroma is up-sampled x2 bilinearly (align_corners=False) and both pictures go through ycbcr2rgb
 *   (pMCTF/utils/util.py) in float32 in its written order, then rint, no clamp.
 *   out[0..3]: sums of squared differences of Y, Cb, Cr and of the three RGB planes together — integers, exact.
 *   msssim != 0: out[4 + 6*s + 2*c + k], s = scale 0..4, c = R,G,B, k = 0: spatial mean of the contrast-structure map
 *   cs, k = 1: of the ssim map (11-tap Gaussian window, sigma 1.5, no padding; C1 = 2.55^2, C2 = 7.65^2; 2x2 average
 *   pool with zero padding of size % 2 between scales).  Needs min(h, w) > 160, PMCTF_EINVAL otherwise.  The final
 *   product  mean_c( prod_{s<4} relu(cs_s)^w_s * relu(ssim_4)^w_4 )  is left to the caller (15 numbers).
 *   msssim == 0: out[4..] is not written.
 *   scratch: pmctf_msssim_scratch_floats(h, w) floats (PMCTF_QUALITY_FRONT_FLOATS are enough when msssim == 0), 8-byte
 *   aligned, no initial contents required; out: PMCTF_QUALITY_OUT_DOUBLES doubles.  Both on the device.
 *   Per-workgroup partial sums are added in a fixed order: the same input gives the same bits on every run.
 *   Launches: 1 (front end) + 5 (one per scale, if msssim) + 1 (final sums); no memset, no synchronisation.
 * pmctf_msssim_scratch_floats: PMCTF_EINVAL for non-positive, odd or > 16384 sizes. */
#define PMCTF_QUALITY_FRONT_FLOATS 8192
#define PMCTF_QUALITY_OUT_DOUBLES 34
int64_t pmctf_msssim_scratch_floats(int h, int w);
int pmctf_frame_quality_f32(const float *rec_y, const float *rec_c, const float *org_y, const float *org_c, int Hp, int Wp,
                            int h, int w, int msssim, float *scratch, double *out, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Pictures in and out (csrc/picture_ops.hip).  One launch each, no synchronisation.  h, w even, positive and at most
 * 16384; PMCTF_EINVAL otherwise, and for a null pointer, before anything is launched.
 *
 * pmctf_yuv420_to_rgb8_f32: the decoded picture the harness saves as a PNG (test_pMCTF_flex.py:76-79,301-317,334-336).
 *   rec_y (1,1,Hp,Wp), rec_c (2,1,Hp/2,Wp/2) as for pmctf_frame_quality_f32 (padded, neither clamped nor rounded) ->
 *   rgb: h*w*3 bytes, [h][w][3] interleaved R,G,B (4-byte aligned).  Per pixel, in the order of the quality front end:
 *   rint(clamp(.)) of luma and of the four chroma taps, x2 bilinear (align_corners=False), ycbcr2rgb, rint, then the
 *   clamp(., 0, 255) and cast of save_torch_image.  Hp >= h, Wp >= w, both even.
 * pmctf_yuv420_u8_to_planes_f32: one picture as it lies in a planar 8-bit 4:2:0 file (h*w luma bytes, then two planes of
 *   (h/2)*(w/2)) -> the model's inputs (test_pMCTF_flex.py:151-192): y_pad (1,1,Hp,Wp) and c_pad (2,1,Hp/2,Wp/2), the
 *   bytes as float32, zero outside the picture (the kernel writes the padding itself; 16-byte aligned), and, unless
 *   null, the un-padded y_org (1,1,h,w) and c_org (2,1,h/2,w/2).  The counterpart of pmctf_planes_to_u8.
 * pmctf_rgb8_to_yuv420_u8: rgb [h][w][3] bytes -> one picture in the file layout above.  rgb2ycbcr
 *   (pMCTF/utils/util.py:21-40, as the data path applies it, pMCTF/datasets/video.py:146) in float32 in its written order:
 *   y = (0.299 R + 0.587 G) + 0.114 B, cb = (B - y) 0.564 + 128, cr = (R - y) 0.713 + 128 on the unrounded y; the Y byte
 *   is rint(clamp(y, 0, 255)), a chroma byte rint(clamp((((c00 + c01) + c10) + c11) * 0.25, 0, 255)) of the unrounded
 *   values of its 2x2 block (upper pair first), ties to even. */
int pmctf_yuv420_to_rgb8_f32(const float *rec_y, const float *rec_c, uint8_t *rgb, int Hp, int Wp, int h, int w,
                             void *stream);
int pmctf_yuv420_u8_to_planes_f32(const uint8_t *src, float *y_pad, float *c_pad, float *y_org, float *c_org, int Hp, int Wp,
                                  int h, int w, void *stream);
int pmctf_rgb8_to_yuv420_u8(const uint8_t *rgb, uint8_t *yuv, int h, int w, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * High-bit-depth pictures in and out (the uint16_t instantiations of csrc/picture_ops.hip, and csrc/picture_hbd.hip): planar 4:2:0 sources of bitdepth b = 9..16, every sample a
 * little-endian 16-bit word (yuv420p10le / p12le / p16le).  The codec's float planes keep their 0..255 range: with
 * s = b - 8 and max = 2^b - 1 a sample v enters as v * 2^-s (exact for every 16-bit v) and a reconstruction x leaves as
 * rint(clamp(x * 2^s, 0, max)), ties to even, NaN -> 0; out(in(v)) == v for every v <= max.  No synchronisation.
 * PMCTF_EINVAL, before anything is launched, for a null pointer (the two originals of the first may be null), a
 * bitdepth outside 9..16, a pointer less aligned than its element type, Hp < h or Wp < w, and sizes that are not
 * positive or above 16384; the first and the third take whole pictures and want h, w, Hp, Wp even as well.
 *
 * pmctf_yuv420_u16_to_planes_f32: the 16-bit pmctf_yuv420_u8_to_planes_f32.  src: h*w luma samples, then two planes of
 *   (h/2)*(w/2), 2-byte aligned (samples above max are converted as they are) -> y_pad (1,1,Hp,Wp), c_pad
 *   (2,1,Hp/2,Wp/2), zero outside the picture (16-byte aligned) and, unless null, y_org (1,1,h,w), c_org (2,1,h/2,w/2).
 *   One launch.
 * pmctf_planes_to_u16: the 16-bit pmctf_planes_to_u8.  x (N,1,Hp,Wp) -> out (N,h,w) samples, 2-byte aligned; any
 *   positive h <= Hp, w <= Wp (the chroma planes of a 6x10 picture are 3x5); N*Hp*Wp < 2^31.  One launch.
 * pmctf_frame_sse_u16_f32: rec_y (1,1,Hp,Wp), rec_c (2,1,Hp/2,Wp/2) padded, neither clamped nor rounded; org_y (1,1,h,w),
 *   org_c (2,1,h/2,w/2) the originals as the first function returns them -> sse3[0..2] = sum of (v_hat - v)^2 over Y, Cb,
 *   Cr with v_hat = rint(clamp(rec * 2^s, 0, max)) and v = org * 2^s: integers, accumulated in 64 bits (one term can be
 *   65535^2), exact and the same on every run (integer atomic adds, one per workgroup and plane).  sse3: three values on
 *   the device, 8-byte aligned.  One clear of sse3 and one launch. */
int pmctf_yuv420_u16_to_planes_f32(const uint16_t *src, float *y_pad, float *c_pad, float *y_org, float *c_org, int Hp,
                                   int Wp, int h, int w, int bitdepth, void *stream);
int pmctf_planes_to_u16(const float *x, uint16_t *out, int N, int Hp, int Wp, int h, int w, int bitdepth, void *stream);
int pmctf_frame_sse_u16_f32(const float *rec_y, const float *rec_c, const float *org_y, const float *org_c, int Hp, int Wp,
                            int h, int w, int bitdepth, uint64_t *sse3, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Resampling of 4:2:0 pictures (csrc/picture_scale.hip): one packed planar picture of h_in x w_in (h_in*w_in luma samples,
 * then two planes of (h_in/2)*(w_in/2), as it lies in a .yuv file) -> one of h_out x w_out, by the separable Catmull-Rom
 * bicubic with antialiasing stretch and 14-bit integer coefficients of DESIGN 5l.  Bytes for the u8 entry (bitdepth 8),
 * 16-bit samples of bitdepth 9..16 for the u16 entry; max = 2^bitdepth - 1.
 *   luma_x, luma_y, chroma_x, chroma_y: the tables of the four axes (w_in -> w_out, h_in -> h_out and the same of the
 *   halved sizes), built on the host (pmctf_scale.axis_table), in DEVICE memory, 4-byte aligned.  A table of n_out rows of
 *   T taps is int32 start[n_out] followed by int16 coef[n_out][T]; every row sums to 16384 and rows shorter than T are
 *   zero-filled.  taps: the four T in that order, an array on the HOST, each 1..20.
 *   Per plane: t = (sum_k coef_x[ox][k] * src[r][min(start_x[ox] + k, w_in - 1)] + 32) >> 6 (arithmetic shift, int32), then
 *   out = clamp((sum_k coef_y[oy][k] * t[min(start_y[oy] + k, h_in - 1)][ox] + 2^21) >> 22, 0, max) in 64-bit integers.
 *   Integer sums: the result does not depend on the order of summation and is the same on every run.  Every index taken
 *   from a table is clamped before use; start must not decrease along a table (the kernel takes a tile's source rows
 *   from its first and last row).
 * One launch for the three planes, nothing intermediate in global memory, no synchronisation.  PMCTF_EINVAL, before the
 * launch and with dst untouched, for a null pointer, a size that is odd, not positive or above 16384, h_out / h_in or
 * w_out / w_in outside [1/4, 4], a tap count outside 1..20, a bitdepth the entry does not take, src or dst less aligned
 * than a sample, a table less aligned than 4 bytes. */
int pmctf_resize_yuv420_u8(const uint8_t *src, uint8_t *dst, int h_in, int w_in, int h_out, int w_out, const void *luma_x,
                           const void *luma_y, const void *chroma_x, const void *chroma_y, const int taps[4], int bitdepth,
                           void *stream);
int pmctf_resize_yuv420_u16(const uint16_t *src, uint16_t *dst, int h_in, int w_in, int h_out, int w_out, const void *luma_x,
                            const void *luma_y, const void *chroma_x, const void *chroma_y, const int taps[4], int bitdepth,
                            void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Chroma format conversion (csrc/picture_chroma.hip): one packed planar picture of h x w in format fmt_in ->
 * the picture in fmt_out, both given as 420, 422 or 444 (Y of h x w, then Cb and Cr of h/sy x w/sx each with (sx, sy) =
 * (2,2), (2,1), (1,1), as the picture lies in a .yuv or .y4m file).  Replaces an outside tool's chroma conversion on the
 * way into and out of the codec; nothing in the reference.  Bytes for the u8 entry (bitdepth 8), 16-bit samples of
 * bitdepth 9..16 for the u16 entry; max = 2^bitdepth - 1.
 *   Y is copied, 16 bytes per thread where the distance between src and dst allows.  Cb and Cr each go through the two
 *   passes of pmctf_resize_yuv420_u8 above with chroma_x (w/sx_in -> w/sx_out) and chroma_y (h/sy_in -> h/sy_out): tables
 *   in that layout, in DEVICE memory, 4-byte aligned, built on the host (pmctf_chroma.chroma_tables); taps: their two T,
 *   an array on the HOST, each 1..17.  An axis whose length does not change has the single-tap table (start[i] = i,
 *   coef[i] = {16384}), whose pass is exact; the kernel does not read it.  Every index taken from a table is clamped
 *   before use; start must not decrease along a table.  fmt_in == fmt_out copies the picture.
 * One launch, nothing intermediate in global memory, no synchronisation.  PMCTF_EINVAL, before the launch and with dst
 * untouched, for a null pointer, a side that is odd, not positive or above 16384, a format other than the three, a tap
 * count outside 1..17, a bitdepth the entry does not take, src or dst less aligned than a sample, a table less aligned
 * than 4 bytes. */
int pmctf_convert_chroma_u8(const uint8_t *src, uint8_t *dst, int h, int w, int fmt_in, int fmt_out, const void *chroma_x,
                            const void *chroma_y, const int taps[2], int bitdepth, void *stream);
int pmctf_convert_chroma_u16(const uint16_t *src, uint16_t *dst, int h, int w, int fmt_in, int fmt_out,
                             const void *chroma_x, const void *chroma_y, const int taps[2], int bitdepth, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Pixel layouts (csrc/picture_layout.hip): a picture of h x w as a decoder surface or a capture file holds it
 * <-> the packed planar picture of the layout's chroma format (Y, then Cb, then Cr, tight, low-bit-aligned: what
 * pmctf_convert_chroma_* and pmctf_yuv420_*_to_planes_f32 take).  Pure bit movement, exact.  "Word": a little-endian 16-bit
 * word; a sample v of depth b is stored in a word as v << (16 - b).
 *   NV12 / NV21 / NV16 (u8 entries, 4:2:0, 4:2:0, 4:2:2): h rows of w Y bytes, then h/2 (NV16: h) rows of w bytes
 *     Cb0 Cr0 Cb1 Cr1 .. (NV21: Cr first).  P010 / P012 / P016 and P210 / P212 / P216 (u16 entries, bitdepth 10, 12, 16):
 *     NV12 and NV16 in words.  The chroma plane has the luma plane's pitch and starts at pitch * luma_rows.
 *   YUYV / UYVY (u8, 4:2:2): rows of 2w bytes Y0 Cb Y1 Cr / Cb Y0 Cr Y1 per pixel pair.  Y210 / Y212 / Y216 (u16): YUYV in
 *     words.
 *   V210 (u16 entries, bitdepth 10, 4:2:2): six pixels in four little-endian 32-bit words of three 10-bit values at bits
 *     0-9, 10-19, 20-29: (Cb0, Y0, Cr0) (Y1, Cb1, Y2) (Cr1, Y3, Cb2) (Y4, Cr2, Y5); a row is ((w + 47) / 48) * 128 bytes.
 *   pitch: bytes from one row to the next; a multiple of the container (1, 2; 4 for V210), at least the row's bytes and at
 *   most 2^20.  luma_rows: rows of the luma plane of a semi-planar surface, h..2^17 (validated for every layout, used by
 *   the semi-planar ones).  surface: aligned to the container; the planar picture: to its sample.
 *   Unpacking drops the low 16 - b bits of a word and ignores bits 30-31 of a V210 word, V210 values beyond the width and
 *   everything between a row's end and the pitch.  Packing masks every sample to b bits, writes the low 16 - b bits, V210
 *   bits 30-31, V210 values beyond the width and the rest of a V210 row as zero, and writes nothing between a row's end
 *   and the pitch, nor anywhere else outside the rows.  Source and destination may not overlap (not checked).
 * One launch per picture, all planes in one grid, no LDS, no synchronisation; byte offsets are 64-bit.  PMCTF_EINVAL, before
 * the launch, for a null pointer, a side that is odd, not positive or above 16384, an unknown layout or one of the other
 * sample width, a bitdepth that is not the layout's, a pitch or luma_rows outside the rules, a pointer less aligned than
 * stated. */
#define PMCTF_LAYOUT_NV12 1
#define PMCTF_LAYOUT_NV21 2
#define PMCTF_LAYOUT_NV16 3
#define PMCTF_LAYOUT_P010 4
#define PMCTF_LAYOUT_P012 5
#define PMCTF_LAYOUT_P016 6
#define PMCTF_LAYOUT_P210 7
#define PMCTF_LAYOUT_P212 8
#define PMCTF_LAYOUT_P216 9
#define PMCTF_LAYOUT_YUYV 10
#define PMCTF_LAYOUT_UYVY 11
#define PMCTF_LAYOUT_Y210 12
#define PMCTF_LAYOUT_Y212 13
#define PMCTF_LAYOUT_Y216 14
#define PMCTF_LAYOUT_V210 15
#define PMCTF_LAYOUT_MAX_PITCH (1 << 20)
#define PMCTF_LAYOUT_MAX_LUMA_ROWS (1 << 17)
int pmctf_unpack_layout_u8(const void *surface, uint8_t *frame, int layout, int h, int w, int64_t pitch, int luma_rows,
                           void *stream);
int pmctf_unpack_layout_u16(const void *surface, uint16_t *frame, int layout, int h, int w, int bitdepth, int64_t pitch,
                            int luma_rows, void *stream);
int pmctf_pack_layout_u8(const uint8_t *frame, void *surface, int layout, int h, int w, int64_t pitch, int luma_rows,
                         void *stream);
int pmctf_pack_layout_u16(const uint16_t *frame, void *surface, int layout, int h, int w, int bitdepth, int64_t pitch,
                          int luma_rows, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Sequence structure pre-analysis (csrc/scene_ops.hip): the luma histogram of one picture and its sum of absolute
 * differences against the previous one, the figures pmctf_seq.scene_cuts decides scene changes from.
 *
 * pmctf_luma_activity_f32: cur, prev: dense un-padded luma originals (1,1,h,w) as pmctf_yuv420_u8_to_planes_f32 /
 *   pmctf_yuv420_u16_to_planes_f32 return them (a sample v is v * 2^-s, s = bitdepth - 8), 16-byte aligned; prev may be
 *   null.  Per element u = rint(clamp(x * 2^s, 0, 65535)) as an integer (exact for every original; NaN -> 0);
 *   hist256[min(u >> s, 255)] += 1 over cur (256 values on the device, 4-byte aligned) and, unless prev is null,
 *   *sad = sum |u_cur - u_prev| (one value on the device, 8-byte aligned; with a null prev it is not touched and may be
 *   null).  bitdepth 8..16; any h, w in 1..16384.  Integer atomic adds only (LDS, then one per workgroup and non-zero
 *   bin, one 64-bit one per workgroup for the SAD): exact and the same on every run.  One clear per output and one
 *   launch, no synchronisation.  PMCTF_EINVAL, before anything is enqueued, for a null cur or hist256, a null sad with a
 *   prev, a bitdepth or a size out of range and a pointer less aligned than stated. */
int pmctf_luma_activity_f32(const float *cur, const float *prev, int h, int w, int bitdepth, uint32_t *hist256,
                            uint64_t *sad, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Picture hashes (csrc/picture_hash.hip): crc_out[s] = CRC-32 of the bytes [data, data + bytes) of segs[s], s < n_segs, as
 * zlib.crc32 computes it (reflected polynomial 0xEDB88320, initial value and final XOR 0xFFFFFFFF).  The encoder records
 * the hashes of its reconstructed pictures, the decoder recomputes and compares them (pmctf_gop.picture_hashes).
 *   segs: the table of ranges, in DEVICE memory like the ranges themselves, 8-byte aligned.  A range may start at any byte
 *   address (plane 1 of a cropped 4:2:0 chroma tensor starts at an odd one for some sizes); bytes == 0 gives 0 and its
 *   data is not looked at.  crc_out: n_segs values on the device, 4-byte aligned; nothing around them is written.
 *   slices: workgroups per range, 1..1024, a launch shape only (0: 64); a range's 16-byte pieces are dealt to them in
 *   spans of whole tiles of PMCTF_CRC32_TILE_BYTES.  Results do not depend on it.
 * Two launches whatever n_segs and the lengths are, no memset, no synchronisation.  Partial remainders are combined with
 * integer XOR atomics, which do not depend on the order of arrival: the same input gives the same bits on every run.
 * n_segs == 0 launches nothing.  PMCTF_EINVAL, before any launch, for a null or misaligned table or output, n_segs < 0
 * or > 65535, slices out of range. */
#define PMCTF_CRC32_TILE_BYTES 4096
typedef struct pmctf_crc_segment {
    const void *data;
    uint64_t bytes;
} pmctf_crc_segment;                    /* 16 bytes */
int pmctf_crc32_segments(const pmctf_crc_segment *segs, int n_segs, int slices, uint32_t *crc_out, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * DIAGNOSTIC entry point; the codec never calls it.  Evaluates one of the scalar functions behind every kernel above
 * (csrc/pm_device_math.h, pm_sleef_f32.h, pm_glibc_expf.h) on n float32 bit patterns, as the GPU compiler built them:
 * y[i] = fn(bits[i]), or fn(first_bits + i) (mod 2^32) when bits == NULL, so that all 2^32 inputs can be swept without
 * an input array.  The suite compares it with the oracle on every float32 (tests/test_gpu_math_sweep.py).
 *   fn: PMCTF_PROBE_TANH        tanh, interval table read from global memory   (torch.tanh, lifting_1d.py:39,42)
 *       PMCTF_PROBE_TANH_LDS    tanh, table copied to LDS by the workgroup
 *       PMCTF_PROBE_SIGMOID     1 / (1 + Sleef_expf(-x))                        (torch.sigmoid, long_context.py:24)
 *       PMCTF_PROBE_SIGMOID_SCALAR  1 / (1 + expf(-x)), glibc's expf: ATen's scalar tail
 *       PMCTF_PROBE_LOG         log as the CDF-row index takes it               (torch.log, entropy_models.py:271)
 *       PMCTF_PROBE_LOG_POLY    its polynomial schedule outside [2^-100, 2^100), on every input
 *       PMCTF_PROBE_EXP         exp of the estimate-mode kernels
 *       PMCTF_PROBE_GLIBC_EXP   the transcription of glibc's expf alone
 *       PMCTF_PROBE_ACT + PMCTF_ACT_{RELU,LEAKY,TANH,SIGMOID}   the conv epilogue's activation; `slope` is the leaky slope
 *   (ignored by every other fn).
 * bits (may be NULL), y: device pointers; y 16-byte aligned (four results per store).  0 < n <= 2^32.
 * PMCTF_EINVAL, before any launch, for a null or misaligned y, n out of range and an unknown fn. */
#define PMCTF_PROBE_TANH 0
#define PMCTF_PROBE_TANH_LDS 1
#define PMCTF_PROBE_SIGMOID 2
#define PMCTF_PROBE_SIGMOID_SCALAR 3
#define PMCTF_PROBE_LOG 4
#define PMCTF_PROBE_LOG_POLY 5
#define PMCTF_PROBE_EXP 6
#define PMCTF_PROBE_GLIBC_EXP 7
#define PMCTF_PROBE_ACT 8
int pmctf_math_probe_f32(int fn, const uint32_t *bits, uint32_t first_bits, int64_t n, float *y, float slope,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif
