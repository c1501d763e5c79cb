// Picture-quality metrics of the evaluation harness (test_pMCTF_flex.py:293-327) as gfx950 kernels:
//   quality_front_kernel   reconstruction -> clamp, round, crop; exact squared-error sums of Y, Cb, Cr and of the rounded
//                          RGB pictures (chroma x2 bilinear, ycbcr2rgb in the written order); optionally the two RGB
//                          pictures as planar float32 for MS-SSIM
//   msssim_scale_kernel    one MS-SSIM scale (Wang, Simoncelli, Bovik 2003): 11-tap Gaussian moments of both pictures
//                          through LDS, the cs and ssim maps in registers, their sums per workgroup, and the 2x2 average
//                          pool that makes the next scale's pictures
//   quality_finish_kernel  adds the per-workgroup partial sums in a fixed order (no floating-point atomics: two runs on
//                          the same input give the same bits) and writes the 4 sums and the 30 map means
// The library is compiled with -ffp-contract=off, so the colour conversion below is evaluated exactly as written; the
// MS-SSIM moments ask for fused multiply-adds by name (fmaf).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/pmctf_hip.h"
#include "launch.h"
#include "picture_common.h"
#include "picture_math.h"

#define Q_FRONT_BLOCKS 1024                      // partial sums of the front end: [Q_FRONT_BLOCKS][4] doubles
#define Q_TILE 32                                // MS-SSIM output tile (Q_TILE x Q_TILE per workgroup)
#define Q_TAPS 11
#define Q_HALO (Q_TILE + Q_TAPS - 1)             // 42: input tile side
#define Q_STRIDE 44                              // LDS row stride of the input tile: rows start on 16 bytes
#define Q_RUN 4                                  // consecutive outputs per thread in either pass
#define Q_SPAN (Q_RUN + Q_TAPS - 1)              // 14: samples behind Q_RUN outputs
#define Q_SCALES 5

static_assert(P_THREADS * Q_RUN == Q_TILE * Q_TILE && Q_TILE % Q_RUN == 0 && Q_STRIDE % 4 == 0 &&
              Q_STRIDE >= Q_TILE - Q_RUN + 16, "tile shape: one column run per thread, 16-byte rows, four float4 per run");
static_assert(PMCTF_QUALITY_FRONT_FLOATS == 2 * 4 * Q_FRONT_BLOCKS, "front-end partial sums: header and kernel disagree");
static_assert(PMCTF_QUALITY_OUT_DOUBLES == 4 + 2 * 3 * Q_SCALES, "result layout: header and kernel disagree");

struct QWindow {
    float g[Q_TAPS];
};

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

// One scale.  x, y: the two pictures, [3][H][W]; nx, ny: the next scale's pictures [3][Hn][Wn] (null at the last scale),
// 2x2 average, stride 2, zero padding pad_h / pad_w (counted in the average) in front.  The grid covers the INPUT in
// Q_TILE x Q_TILE tiles: a workgroup forms the map values whose window starts in its tile (those inside the (H-10)x(W-10)
// valid region) and the pooled samples (Q_TILE/2)^2 of its tile; blockIdx.z is the channel, so that the small scales, a
// handful of tiles each, are not three channels deep in one workgroup.  partial: [tiles][3][2] sums of cs and ssim.
__global__ __launch_bounds__(P_THREADS) void msssim_scale_kernel(
    const float *__restrict__ x, const float *__restrict__ y, int H, int W, float *__restrict__ nx,
    float *__restrict__ ny, int Hn, int Wn, int pad_h, int pad_w, QWindow win, double *__restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float xs[Q_HALO * Q_STRIDE], ys[Q_HALO * Q_STRIDE];
    __shared__ __attribute__((aligned(16))) float mom[5][Q_HALO * Q_TILE];
    __shared__ float redf[P_THREADS / 64];
    __shared__ double redd[P_THREADS / 64];
    const int tid = threadIdx.x, ty0 = blockIdx.y * Q_TILE, tx0 = blockIdx.x * Q_TILE;
    const long plane = (long)H * W;
    const int rows_in = min(Q_HALO, H - ty0), cols_in = min(Q_HALO, W - tx0);
    const float C1 = (0.01f * 255.0f) * (0.01f * 255.0f), C2 = (0.03f * 255.0f) * (0.03f * 255.0f);
    const int c = blockIdx.z;
    double *out = partial + 6 * ((long)blockIdx.y * gridDim.x + blockIdx.x) + 2 * c;
    const float *xp = x + c * plane, *yp = y + c * plane;
    {
        // every load of the tile is issued before the first one is used: one memory latency per tile, not one per element
        constexpr int PER = (Q_HALO * Q_HALO + P_THREADS - 1) / P_THREADS;
        float a[PER], b[PER], local = 0.0f;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = tid + k * P_THREADS, r = i / Q_HALO, cc = i - r * Q_HALO;
            const bool in = r < rows_in && cc < cols_in;          // r >= Q_HALO past the tile: rows_in <= Q_HALO
            a[k] = in ? xp[(long)(ty0 + r) * W + tx0 + cc] : 0.0f;
            b[k] = in ? yp[(long)(ty0 + r) * W + tx0 + cc] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < PER; ++k) local += a[k];
        // Variances do not change when a constant is subtracted from both pictures; E[x^2] - mu^2 in float32 cancels far
        // less around the tile's own level than around 0.  The shift is an integer: the subtraction is exact at every
        // scale (samples are multiples of 2^-8 below 2^9).
        const float shift = rintf(block_sum(local, redf) / (float)(rows_in * cols_in));
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = tid + k * P_THREADS, r = i / Q_HALO, cc = i - r * Q_HALO;
            if (i < Q_HALO * Q_HALO) { xs[r * Q_STRIDE + cc] = a[k] - shift; ys[r * Q_STRIDE + cc] = b[k] - shift; }
        }
        __syncthreads();
        // Row pass: a thread takes Q_RUN consecutive outputs of one row, so that the Q_SPAN samples behind them are read
        // from LDS once (16-byte reads) instead of Q_TAPS times each.  Every output still adds its taps in the order 0..10.
        for (int it = tid; it < Q_HALO * (Q_TILE / Q_RUN); it += P_THREADS) {
            const int r = it / (Q_TILE / Q_RUN), col = (it % (Q_TILE / Q_RUN)) * Q_RUN;
            const float4 *xr = reinterpret_cast<const float4 *>(xs + r * Q_STRIDE + col);
            const float4 *yr = reinterpret_cast<const float4 *>(ys + r * Q_STRIDE + col);
            float a[16], b[16];                      // the last two are past the span: loaded, never used
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const float4 xa = xr[v], yb = yr[v];
                a[4 * v] = xa.x; a[4 * v + 1] = xa.y; a[4 * v + 2] = xa.z; a[4 * v + 3] = xa.w;
                b[4 * v] = yb.x; b[4 * v + 1] = yb.y; b[4 * v + 2] = yb.z; b[4 * v + 3] = yb.w;
            }
            float aa[Q_SPAN], bb[Q_SPAN], ab[Q_SPAN];
#pragma unroll
            for (int j = 0; j < Q_SPAN; ++j) { aa[j] = a[j] * a[j]; bb[j] = b[j] * b[j]; ab[j] = a[j] * b[j]; }
            float m[5][Q_RUN];
#pragma unroll
            for (int i = 0; i < Q_RUN; ++i) {
                float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f, m3 = 0.0f, m4 = 0.0f;
#pragma unroll
                for (int t = 0; t < Q_TAPS; ++t) {
                    const float g = win.g[t];
                    m0 = fmaf(g, a[i + t], m0); m1 = fmaf(g, b[i + t], m1);
                    m2 = fmaf(g, aa[i + t], m2); m3 = fmaf(g, bb[i + t], m3); m4 = fmaf(g, ab[i + t], m4);
                }
                m[0][i] = m0; m[1][i] = m1; m[2][i] = m2; m[3][i] = m3; m[4][i] = m4;
            }
#pragma unroll
            for (int k = 0; k < 5; ++k)
                *reinterpret_cast<float4 *>(&mom[k][r * Q_TILE + col]) = make_float4(m[k][0], m[k][1], m[k][2], m[k][3]);
        }
        __syncthreads();
        // Column pass and the maps: a thread takes Q_RUN consecutive outputs of one column.
        double cs_sum = 0.0, ssim_sum = 0.0;
        {
            const int ox = tid % Q_TILE, oy0 = (tid / Q_TILE) * Q_RUN;
            float m[5][Q_RUN];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                float v[Q_SPAN];
#pragma unroll
                for (int j = 0; j < Q_SPAN; ++j) v[j] = mom[k][(oy0 + j) * Q_TILE + ox];
#pragma unroll
                for (int i = 0; i < Q_RUN; ++i) {
                    float acc = 0.0f;
#pragma unroll
                    for (int t = 0; t < Q_TAPS; ++t) acc = fmaf(win.g[t], v[i + t], acc);
                    m[k][i] = acc;
                }
            }
#pragma unroll
            for (int i = 0; i < Q_RUN; ++i) {
                if (ty0 + oy0 + i >= H - (Q_TAPS - 1) || tx0 + ox >= W - (Q_TAPS - 1)) continue;
                const float s11 = m[2][i] - m[0][i] * m[0][i], s22 = m[3][i] - m[1][i] * m[1][i];
                const float s12 = m[4][i] - m[0][i] * m[1][i];
                const float mu1 = m[0][i] + shift, mu2 = m[1][i] + shift;
                const float cs = (2.0f * s12 + C2) / (s11 + s22 + C2);
                const float lum = (2.0f * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1);
                cs_sum += (double)cs;
                ssim_sum += (double)(lum * cs);
            }
        }
        cs_sum = block_sum(cs_sum, redd);
        ssim_sum = block_sum(ssim_sum, redd);
        if (tid == 0) { out[0] = cs_sum; out[1] = ssim_sum; }
    }

    if (nx) {                                        // 2x2 average pool of this tile: one sample per thread and picture
        const int j = blockIdx.y * (Q_TILE / 2) + tid / (Q_TILE / 2), i = blockIdx.x * (Q_TILE / 2) + tid % (Q_TILE / 2);
        if (j < Hn && i < Wn) {
            const int r0 = 2 * j - pad_h, c0 = 2 * i - pad_w;
            const long nplane = (long)Hn * Wn;
            float sx = 0.0f, sy = 0.0f;
#pragma unroll
            for (int dr = 0; dr < 2; ++dr)
#pragma unroll
                for (int dc = 0; dc < 2; ++dc) {
                    const int r = r0 + dr, cc = c0 + dc;
                    const bool in = r >= 0 && r < H && cc >= 0 && cc < W;
                    sx += in ? xp[(long)r * W + cc] : 0.0f;
                    sy += in ? yp[(long)r * W + cc] : 0.0f;
                }
            nx[c * nplane + (long)j * Wn + i] = 0.25f * sx;
            ny[c * nplane + (long)j * Wn + i] = 0.25f * sy;
        }
    }
}

struct QSegment {
    const double *src;          // [rows][width]
    double *dst;                // [width]
    int rows, width;
    double scale;               // dst = scale * sum over rows
};
struct QSegments {
    QSegment s[1 + Q_SCALES];
};

// one workgroup per segment and column: thread t adds rows t, t + 256, ... in that order, then the workgroup adds its
// threads
__global__ __launch_bounds__(P_THREADS) void quality_finish_kernel(QSegments segs) {
    __shared__ double red[P_THREADS / 64];
    const QSegment sg = segs.s[blockIdx.x];
    const int k = blockIdx.y;
    if (k >= sg.width) return;
    double v = 0.0;
    for (int r = threadIdx.x; r < sg.rows; r += P_THREADS) v += sg.src[(long)r * sg.width + k];
    v = block_sum(v, red);
    if (threadIdx.x == 0) sg.dst[k] = sg.scale * v;
}

// ---------------------------------------------------------------------------------------------------- host side
struct QLayout {
    int H[Q_SCALES], W[Q_SCALES], pad_h[Q_SCALES], pad_w[Q_SCALES];
    int tiles_y[Q_SCALES], tiles_x[Q_SCALES];
    long partial_off[Q_SCALES];     // in doubles from the scratch base
    long plane_off[Q_SCALES];       // in floats from the scratch base: [2][3][H][W] of scale s
    long total_floats;
};


static QLayout layout_for(int h, int w) {
    QLayout L;
    long doubles = 4L * Q_FRONT_BLOCKS, floats = 0;
    for (int s = 0; s < Q_SCALES; ++s) {
        L.H[s] = s ? (L.H[s - 1] + 2 * L.pad_h[s - 1] - 2) / 2 + 1 : h;
        L.W[s] = s ? (L.W[s - 1] + 2 * L.pad_w[s - 1] - 2) / 2 + 1 : w;
        L.pad_h[s] = L.H[s] & 1;
        L.pad_w[s] = L.W[s] & 1;
        L.tiles_y[s] = (L.H[s] + Q_TILE - 1) / Q_TILE;
        L.tiles_x[s] = (L.W[s] + Q_TILE - 1) / Q_TILE;
        L.partial_off[s] = doubles;
        doubles += 6L * L.tiles_y[s] * L.tiles_x[s];
    }
    for (int s = 0; s < Q_SCALES; ++s) {
        L.plane_off[s] = 2 * doubles + floats;
        floats += 6L * L.H[s] * L.W[s];
    }
    L.total_floats = 2 * doubles + floats;
    return L;
}

static QWindow gauss_window() {
    QWindow wdw;
    double g[Q_TAPS], sum = 0.0;
    for (int i = 0; i < Q_TAPS; ++i) {
        const double d = i - Q_TAPS / 2;
        g[i] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += g[i];
    }
    for (int i = 0; i < Q_TAPS; ++i) wdw.g[i] = (float)(g[i] / sum);
    return wdw;
}

extern "C" int64_t pmctf_msssim_scratch_floats(int h, int w) {
    if (!size_ok(h, w)) return PMCTF_EINVAL;
    return layout_for(h, w).total_floats;
}

extern "C" int pmctf_frame_quality_f32(const float *rec_y, const float *rec_c, const float *org_y, const float *org_c,
                                       int Hp, int Wp, int h, int w, int msssim, float *scratch, double *out,
                                       void *stream) {
    if (!rec_y || !rec_c || !org_y || !org_c || !scratch || !out || !size_ok(h, w) || !padded_ok(Hp, Wp, h, w) ||
        ((uintptr_t)scratch & 7) || ((uintptr_t)out & 7))
        return PMCTF_EINVAL;
    if (msssim && (h < w ? h : w) <= (Q_TAPS - 1) * (1 << (Q_SCALES - 1))) return PMCTF_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    const QLayout L = layout_for(h, w);
    double *partial = (double *)scratch;
    const long n = (long)h * w;
    const int blocks = (int)((n + P_THREADS - 1) / P_THREADS < Q_FRONT_BLOCKS ? (n + P_THREADS - 1) / P_THREADS : Q_FRONT_BLOCKS);
    float *rgb_rec = msssim ? scratch + L.plane_off[0] : nullptr;
    float *rgb_org = msssim ? rgb_rec + 3 * n : nullptr;
    PM_LAUNCH(quality_front_kernel, dim3(blocks), dim3(P_THREADS), 0, st, rec_y, rec_c, org_y, org_c, Hp, Wp, h, w, rgb_rec,
              rgb_org, partial);
    int rc = pm_launch_status();
    if (rc) return rc;
    QSegments segs;
    segs.s[0] = {partial, out, blocks, 4, 1.0};
    int nseg = 1;
    if (msssim) {
        static const QWindow win = gauss_window();
        for (int s = 0; s < Q_SCALES; ++s) {
            const float *x = scratch + L.plane_off[s], *y = x + 3L * L.H[s] * L.W[s];
            const bool last = s == Q_SCALES - 1;
            float *nx = last ? nullptr : scratch + L.plane_off[s + 1];
            float *ny = last ? nullptr : nx + 3L * L.H[s + 1] * L.W[s + 1];
            PM_LAUNCH(msssim_scale_kernel, dim3(L.tiles_x[s], L.tiles_y[s], 3), dim3(P_THREADS), 0, st, x, y, L.H[s], L.W[s], nx,
                      ny, last ? 0 : L.H[s + 1], last ? 0 : L.W[s + 1], L.pad_h[s], L.pad_w[s], win,
                      partial + L.partial_off[s]);
            rc = pm_launch_status();
            if (rc) return rc;
            segs.s[nseg++] = {partial + L.partial_off[s], out + 4 + 6 * s, L.tiles_y[s] * L.tiles_x[s], 6,
                              1.0 / ((double)(L.H[s] - (Q_TAPS - 1)) * (double)(L.W[s] - (Q_TAPS - 1)))};
        }
    }
    PM_LAUNCH(quality_finish_kernel, dim3(nseg, 6), dim3(P_THREADS), 0, st, segs);
    return pm_launch_status();
}
