// Picture-quality metrics of the evaluation harness (test_pMCTF_flex.py:293-327) as gfx950 kernels:
//   quality_front_kernel   reconstruction -> clamp, round, crop; exact squared-error sums of Y, Cb, Cr and of the rounded
//                          RGB pictures (chroma x2 bilinear, ycbcr2rgb in the written order); optionally the two RGB
//                          pictures as planar float32 for MS-SSIM
//   msssim_scale_kernel    one MS-SSIM scale of the three RGB planes   } quality_msssim.h, shared with the per-plane
//   quality_finish_kernel  the 4 sums and the 30 map means             } entries of quality_planar.hip
// The library is compiled with -ffp-contract=off, so the colour conversion below is evaluated exactly as written; the
// MS-SSIM moments ask for fused multiply-adds by name (fmaf).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/pmctf_hip.h"
#include "launch.h"
#include "picture_common.h"
#include "picture_math.h"
#include "quality_msssim.h"

#define Q_FRONT_BLOCKS 1024                      // partial sums of the front end: [Q_FRONT_BLOCKS][4] doubles

static_assert(PMCTF_QUALITY_FRONT_FLOATS == 2 * 4 * Q_FRONT_BLOCKS, "front-end partial sums: header and kernel disagree");
static_assert(PMCTF_QUALITY_OUT_DOUBLES == 4 + 2 * 3 * Q_SCALES, "result layout: header and kernel disagree");

__global__ __launch_bounds__(P_THREADS) void quality_front_kernel(
    const float *__restrict__ rec_y, const float *__restrict__ rec_c, const float *__restrict__ org_y,
    const float *__restrict__ org_c, int Hp, int Wp, int h, int w, float *__restrict__ rgb_rec,
    float *__restrict__ rgb_org, double *__restrict__ partial) {
    __shared__ double red[P_THREADS / 64];
    const int hc = h >> 1, wc = w >> 1, Wc = Wp >> 1;
    const long plane_p = (long)(Hp >> 1) * Wc, plane_o = (long)hc * wc, n = (long)h * w;
    double sy = 0.0, scb = 0.0, scr = 0.0, srgb = 0.0;
    for (long i = (long)blockIdx.x * P_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * P_THREADS) {
        const int y = (int)((unsigned)i / (unsigned)w), x = (int)((unsigned)i % (unsigned)w);
        const float ry = round_u8(rec_y[(long)y * Wp + x]), oy = org_y[i];
        sy += (double)((ry - oy) * (ry - oy));
        int r0, r1, c0, c1;
        float wr, wcol;
        up2_taps(y, hc, r0, r1, wr);
        up2_taps(x, wc, c0, c1, wcol);
        float up[4];                                 // rec Cb, rec Cr, org Cb, org Cr at (y, x)
        for (int p = 0; p < 2; ++p) {
            const float *rp = rec_c + p * plane_p, *op = org_c + p * plane_o;
            const float a00 = round_u8(rp[(long)r0 * Wc + c0]), a01 = round_u8(rp[(long)r0 * Wc + c1]);
            const float a10 = round_u8(rp[(long)r1 * Wc + c0]), a11 = round_u8(rp[(long)r1 * Wc + c1]);
            const float b00 = op[(long)r0 * wc + c0], b01 = op[(long)r0 * wc + c1];
            const float b10 = op[(long)r1 * wc + c0], b11 = op[(long)r1 * wc + c1];
            up[p] = wr * (wcol * a00 + (1.0f - wcol) * a01) + (1.0f - wr) * (wcol * a10 + (1.0f - wcol) * a11);
            up[2 + p] = wr * (wcol * b00 + (1.0f - wcol) * b01) + (1.0f - wr) * (wcol * b10 + (1.0f - wcol) * b11);
            if (((x | y) & 1) == 0) {                // one thread per chroma sample: (y/2, x/2) is tap (r1, c1) here
                const float d = a11 - b11;
                if (p == 0) scb += (double)(d * d); else scr += (double)(d * d);
            }
        }
        float rr, rg, rb, orr, og, ob;
        to_rgb(ry, up[0], up[1], rr, rg, rb);
        to_rgb(oy, up[2], up[3], orr, og, ob);
        srgb += (double)((rr - orr) * (rr - orr)) + (double)((rg - og) * (rg - og)) + (double)((rb - ob) * (rb - ob));
        if (rgb_rec) {
            rgb_rec[i] = rr; rgb_rec[n + i] = rg; rgb_rec[2 * n + i] = rb;
            rgb_org[i] = orr; rgb_org[n + i] = og; rgb_org[2 * n + i] = ob;
        }
    }
    sy = block_sum(sy, red);
    scb = block_sum(scb, red);
    scr = block_sum(scr, red);
    srgb = block_sum(srgb, red);
    if (threadIdx.x == 0) {
        double *o = partial + 4 * (long)blockIdx.x;
        o[0] = sy; o[1] = scb; o[2] = scr; o[3] = srgb;
    }
}

// ---------------------------------------------------------------------------------------------------- host side
static QLayout rgb_layout(int h, int w) { return layout_for(h, w, 3, 4L * Q_FRONT_BLOCKS, 0); }

extern "C" int64_t pmctf_msssim_scratch_floats(int h, int w) {
    if (!size_ok(h, w)) return PMCTF_EINVAL;
    return rgb_layout(h, w).total_floats;
}

extern "C" int pmctf_frame_quality_f32(const float *rec_y, const float *rec_c, const float *org_y, const float *org_c,
                                       int Hp, int Wp, int h, int w, int msssim, float *scratch, double *out,
                                       void *stream) {
    if (!rec_y || !rec_c || !org_y || !org_c || !scratch || !out || !size_ok(h, w) || !padded_ok(Hp, Wp, h, w) ||
        ((uintptr_t)scratch & 7) || ((uintptr_t)out & 7))
        return PMCTF_EINVAL;
    if (msssim && (h < w ? h : w) <= Q_MIN_SIDE) return PMCTF_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    const QLayout L = rgb_layout(h, w);
    double *partial = (double *)scratch;
    const long n = (long)h * w;
    const int blocks = (int)((n + P_THREADS - 1) / P_THREADS < Q_FRONT_BLOCKS ? (n + P_THREADS - 1) / P_THREADS : Q_FRONT_BLOCKS);
    float *rgb_rec = msssim ? scratch + L.plane_off[0] : nullptr;
    float *rgb_org = msssim ? rgb_rec + 3 * n : nullptr;
    PM_LAUNCH(quality_front_kernel, dim3(blocks), dim3(P_THREADS), 0, st, rec_y, rec_c, org_y, org_c, Hp, Wp, h, w, rgb_rec,
              rgb_org, partial);
    int rc = pm_launch_status();
    if (rc) return rc;
    QSegments<1 + Q_SCALES> segs;
    segs.s[0] = {partial, out, blocks, 4, 1.0};
    int nseg = 1;
    if (msssim) {
        static const QWindow win = gauss_window();
        const float C1 = (0.01f * 255.0f) * (0.01f * 255.0f), C2 = (0.03f * 255.0f) * (0.03f * 255.0f);
        for (int s = 0; s < Q_SCALES; ++s) {
            const float *x = scratch + L.plane_off[s], *y = x + 3L * L.H[s] * L.W[s];
            const bool last = s == Q_SCALES - 1;
            float *nx = last ? nullptr : scratch + L.plane_off[s + 1];
            float *ny = last ? nullptr : nx + 3L * L.H[s + 1] * L.W[s + 1];
            PM_LAUNCH((msssim_scale_kernel<float, 3>), dim3(L.tiles_x[s], L.tiles_y[s], 3), dim3(P_THREADS), 0, st, x, y, L.H[s],
                      L.W[s], nx, ny, last ? 0 : L.H[s + 1], last ? 0 : L.W[s + 1], L.pad_h[s], L.pad_w[s], win, C1, C2, 1.0f,
                      partial + L.partial_off[s]);
            rc = pm_launch_status();
            if (rc) return rc;
            segs.s[nseg++] = {partial + L.partial_off[s], out + 4 + 6 * s, L.tiles_y[s] * L.tiles_x[s], 6,
                              1.0 / ((double)(L.H[s] - (Q_TAPS - 1)) * (double)(L.W[s] - (Q_TAPS - 1)))};
        }
    }
    PM_LAUNCH(quality_finish_kernel<1 + Q_SCALES>, dim3(nseg, 6), dim3(P_THREADS), 0, st, segs);
    return pm_launch_status();
}
