// MS-SSIM (Wang, Simoncelli, Bovik 2003) as the quality kernels compute it, shared by quality_ops.hip (three float RGB
// planes, data range 255) and quality_planar.hip (one plane of a picture's own samples at its own data range):
//   msssim_scale_kernel<S, CH>   one scale: 11-tap Gaussian moments of both pictures through LDS, the cs and ssim maps in
//                                registers, their sums per workgroup, and the 2x2 average pool that makes the next scale's
//                                pictures.  S is the sample type the scale reads (float, or uint8_t / uint16_t at scale 0 of
//                                a plane read where it lies), CH the number of channels
//   quality_finish_kernel<N>     adds per-workgroup partial sums in a fixed order (no floating-point atomics: two runs on
//                                the same input give the same bits)
// and the host arithmetic both entries lay their scratch out with.  The moments ask for fused multiply-adds by name (fmaf).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <type_traits>

#include "picture_common.h"

#define Q_TILE 32                                // MS-SSIM output tile (Q_TILE x Q_TILE per workgroup)
#define Q_TAPS 11
#define Q_HALO (Q_TILE + Q_TAPS - 1)             // 42: input tile side
#define Q_STRIDE 44                              // LDS row stride of the input tile: rows start on 16 bytes
#define Q_RUN 4                                  // consecutive outputs per thread in either pass
#define Q_SPAN (Q_RUN + Q_TAPS - 1)              // 14: samples behind Q_RUN outputs
#define Q_SCALES 5
#define Q_MIN_SIDE ((Q_TAPS - 1) * (1 << (Q_SCALES - 1)))      // 160: the smaller side must exceed it

static_assert(P_THREADS * Q_RUN == Q_TILE * Q_TILE && Q_TILE % Q_RUN == 0 && Q_STRIDE % 4 == 0 &&
              Q_STRIDE >= Q_TILE - Q_RUN + 16, "tile shape: one column run per thread, 16-byte rows, four float4 per run");

struct QWindow {
    float g[Q_TAPS];
};

// a sample as the moments take it: float planes as they are, integer samples times `up` (2^-(bitdepth - 8), exact)
template <typename S>
__device__ __forceinline__ float q_sample(S v, float up) {
    if constexpr (std::is_same<S, float>::value) return v;
    else return (float)v * up;
}

// One scale.  x, y: the two pictures, [CH][H][W]; nx, ny: the next scale's pictures [CH][Hn][Wn] (null at the last scale),
// 2x2 average, stride 2, zero padding pad_h / pad_w (counted in the average) in front.  The grid covers the INPUT in
// Q_TILE x Q_TILE tiles: a workgroup forms the map values whose window starts in its tile (those inside the (H-10)x(W-10)
// valid region) and the pooled samples (Q_TILE/2)^2 of its tile; blockIdx.z is the channel, so that the small scales, a
// handful of tiles each, are not CH channels deep in one workgroup.  partial: [tiles][CH][2] sums of cs and ssim.
// C1 = (0.01 L)^2, C2 = (0.03 L)^2 for the data range L of the samples as q_sample gives them.
template <typename S, int CH>
__global__ __launch_bounds__(P_THREADS) void msssim_scale_kernel(
    const S *__restrict__ x, const S *__restrict__ y, int H, int W, float *__restrict__ nx, float *__restrict__ ny, int Hn,
    int Wn, int pad_h, int pad_w, QWindow win, float C1, float C2, float up, double *__restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float xs[Q_HALO * Q_STRIDE], ys[Q_HALO * Q_STRIDE];
    __shared__ __attribute__((aligned(16))) float mom[5][Q_HALO * Q_TILE];
    __shared__ float redf[P_THREADS / 64];
    __shared__ double redd[P_THREADS / 64];
    const int tid = threadIdx.x, ty0 = blockIdx.y * Q_TILE, tx0 = blockIdx.x * Q_TILE;
    const long plane = (long)H * W;
    const int rows_in = min(Q_HALO, H - ty0), cols_in = min(Q_HALO, W - tx0);
    const int c = blockIdx.z;
    double *out = partial + 2 * CH * ((long)blockIdx.y * gridDim.x + blockIdx.x) + 2 * c;
    const S *xp = x + c * plane, *yp = y + c * plane;
    {
        // every load of the tile is issued before the first one is used: one memory latency per tile, not one per element
        constexpr int PER = (Q_HALO * Q_HALO + P_THREADS - 1) / P_THREADS;
        float a[PER], b[PER], local = 0.0f;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = tid + k * P_THREADS, r = i / Q_HALO, cc = i - r * Q_HALO;
            const bool in = r < rows_in && cc < cols_in;          // r >= Q_HALO past the tile: rows_in <= Q_HALO
            a[k] = in ? q_sample(xp[(long)(ty0 + r) * W + tx0 + cc], up) : 0.0f;
            b[k] = in ? q_sample(yp[(long)(ty0 + r) * W + tx0 + cc], up) : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < PER; ++k) local += a[k];
        // Variances do not change when a constant is subtracted from both pictures; E[x^2] - mu^2 in float32 cancels far
        // less around the tile's own level than around 0.  The shift is an integer: the subtraction is exact at every
        // scale (samples are multiples of 2^-8 below 2^8 at scale 0, of 2^-(8 + 2k) after k pools: 24 bits at most).
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
                    sx += in ? q_sample(xp[(long)r * W + cc], up) : 0.0f;
                    sy += in ? q_sample(yp[(long)r * W + cc], up) : 0.0f;
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
template <int N>
struct QSegments {
    QSegment s[N];
};

// one workgroup per segment and column: thread t adds rows t, t + 256, ... in that order, then the workgroup adds its
// threads
template <int N>
__global__ __launch_bounds__(P_THREADS) void quality_finish_kernel(QSegments<N> segs) {
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
    long plane_off[Q_SCALES];       // in floats from the scratch base: [2][ch][H][W] of scale s (s >= first_stored)
    long total_floats;
};

// scratch of `ch` channels: head_doubles doubles, the scales' partial sums, then both pictures of every scale from
// first_stored on (scale 0 is not stored where it is read from the caller's samples)
static QLayout layout_for(int h, int w, int ch, long head_doubles, int first_stored) {
    QLayout L;
    long doubles = head_doubles, floats = 0;
    for (int s = 0; s < Q_SCALES; ++s) {
        L.H[s] = s ? (L.H[s - 1] + 2 * L.pad_h[s - 1] - 2) / 2 + 1 : h;
        L.W[s] = s ? (L.W[s - 1] + 2 * L.pad_w[s - 1] - 2) / 2 + 1 : w;
        L.pad_h[s] = L.H[s] & 1;
        L.pad_w[s] = L.W[s] & 1;
        L.tiles_y[s] = (L.H[s] + Q_TILE - 1) / Q_TILE;
        L.tiles_x[s] = (L.W[s] + Q_TILE - 1) / Q_TILE;
        L.partial_off[s] = doubles;
        doubles += 2L * ch * L.tiles_y[s] * L.tiles_x[s];
    }
    for (int s = 0; s < Q_SCALES; ++s) {
        L.plane_off[s] = 2 * doubles + floats;
        if (s >= first_stored) floats += 2L * ch * L.H[s] * L.W[s];
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
