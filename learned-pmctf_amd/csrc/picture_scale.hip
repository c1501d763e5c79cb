// Resampling of planar 4:2:0 pictures as one gfx950 kernel: the separable Catmull-Rom bicubic (a = -1/2) with an
// antialiasing stretch of DESIGN 5l, in integers.  The host (pmctf_scale.py) builds, per axis, a table
//     int32 start[n_out];  int16 coef[n_out][T];          (one device buffer, 4-byte aligned)
// whose rows sum to 16384.  Per plane, with max = 2^b - 1:
//     horizontal  t   = (sum_k coef_x[ox][k] * src[r][min(start_x[ox] + k, w_in - 1)] + 32) >> 6             (int32)
//     vertical    out = clamp((sum_k coef_y[oy][k] * t[min(start_y[oy] + k, h_in - 1)][ox] + 2^21) >> 22, 0, max)   (int64)
// All sums are integer sums: the result does not depend on their order.
//
// One launch per picture: the grid holds the tiles of Y, then of Cb, then of Cr.  A workgroup of 256 threads owns a tile
// of S_TH x S_TW output samples and runs the two passes through LDS (picture_resample.h: resample_tile, shared with
// picture_chroma.hip); nothing intermediate goes to HBM.
//
// A 16-row tile at the steepest reduction (4:1, 17 taps) needs 15 * 4 + 1 + 17 = 78 source rows: S_ROWS = 80 rows of
// S_TW int32 are 20 KiB, the x coefficients (S_TAPS x S_TW int32) 5 KiB more, so six workgroups fit the 160 KiB of a CU.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pmctf_hip.h"
#include "launch.h"
#include "picture_resample.h"

struct ScaleArgs {
    ScalePlane p[3];
};

template <typename S>
__global__ __launch_bounds__(P_THREADS) void resize_yuv420_kernel(const S *__restrict__ src, S *__restrict__ dst,
                                                                   const ScaleArgs a, int top) {
    __shared__ __attribute__((aligned(16))) int tmp[S_ROWS * S_TW];
    __shared__ int cx[S_TAPS * S_TW];

    unsigned tile = blockIdx.x;
    int pi = 0;
    if (tile >= a.p[0].tiles) {
        tile -= a.p[0].tiles;
        pi = 1;
        if (tile >= a.p[1].tiles) {
            tile -= a.p[1].tiles;
            pi = 2;
        }
    }
    const ScalePlane &P = a.p[pi];
    if (tile >= P.tiles) return;
    resample_tile<S, false, false>(src, dst, P, tile, top, tmp, cx);
}

static bool ratio_ok(int n_in, int n_out) { return 4L * n_out >= n_in && n_out <= 4L * n_in; }
static bool taps_ok(int t) { return t >= 1 && t <= S_TAPS; }

template <typename S>
static int resize_yuv420(const S *src, S *dst, int h_in, int w_in, int h_out, int w_out, const void *luma_x,
                         const void *luma_y, const void *chroma_x, const void *chroma_y, const int taps[4], int bitdepth,
                         void *stream) {
    if (!src || !dst || !luma_x || !luma_y || !chroma_x || !chroma_y || !taps || !side_ok(h_in) || !side_ok(w_in) ||
        !side_ok(h_out) || !side_ok(w_out) || !ratio_ok(h_in, h_out) || !ratio_ok(w_in, w_out) || !taps_ok(taps[0]) ||
        !taps_ok(taps[1]) || !taps_ok(taps[2]) || !taps_ok(taps[3]) ||
        (((uintptr_t)src | (uintptr_t)dst) & (sizeof(S) - 1)) ||
        (((uintptr_t)luma_x | (uintptr_t)luma_y | (uintptr_t)chroma_x | (uintptr_t)chroma_y) & 3))
        return PMCTF_EINVAL;
    ScaleArgs a;
    const int hci = h_in >> 1, wci = w_in >> 1, hco = h_out >> 1, wco = w_out >> 1;
    const size_t ny_in = (size_t)h_in * w_in, nc_in = (size_t)hci * wci;
    const size_t ny_out = (size_t)h_out * w_out, nc_out = (size_t)hco * wco;
    set_plane(a.p[0], h_in, w_in, h_out, w_out, luma_x, taps[0], luma_y, taps[1], 0, 0);
    set_plane(a.p[1], hci, wci, hco, wco, chroma_x, taps[2], chroma_y, taps[3], ny_in, ny_out);
    set_plane(a.p[2], hci, wci, hco, wco, chroma_x, taps[2], chroma_y, taps[3], ny_in + nc_in, ny_out + nc_out);
    const unsigned blocks = a.p[0].tiles + a.p[1].tiles + a.p[2].tiles;
    PM_LAUNCH(resize_yuv420_kernel<S>, dim3(blocks), dim3(P_THREADS), 0, (hipStream_t)stream, src, dst, a,
              (1 << bitdepth) - 1);
    return pm_launch_status();
}

extern "C" int pmctf_resize_yuv420_u8(const uint8_t *src, uint8_t *dst, int h_in, int w_in, int h_out, int w_out,
                                      const void *luma_x, const void *luma_y, const void *chroma_x, const void *chroma_y,
                                      const int taps[4], int bitdepth, void *stream) {
    if (bitdepth != 8) return PMCTF_EINVAL;
    return resize_yuv420<uint8_t>(src, dst, h_in, w_in, h_out, w_out, luma_x, luma_y, chroma_x, chroma_y, taps, 8, stream);
}

extern "C" int pmctf_resize_yuv420_u16(const uint16_t *src, uint16_t *dst, int h_in, int w_in, int h_out, int w_out,
                                       const void *luma_x, const void *luma_y, const void *chroma_x, const void *chroma_y,
                                       const int taps[4], int bitdepth, void *stream) {
    if (!depth_ok(bitdepth)) return PMCTF_EINVAL;
    return resize_yuv420<uint16_t>(src, dst, h_in, w_in, h_out, w_out, luma_x, luma_y, chroma_x, chroma_y, taps, bitdepth,
                                   stream);
}
