// Quality of pictures as they lie in files (include/pmctf_quality.h): planar 4:2:0, 4:2:2 or 4:4:4 at 8 bits
// (uint8_t samples) or 9..16 bits (uint16_t samples), in the picture's own format and data range.
//   planar_sse_kernel<S>   sums of (a - b)^2 over Y, Cb and Cr of two packed pictures, 64-bit integers: groups of four
//                          samples, loaded as wide as the addresses allow; integer atomic adds, one per workgroup and
//                          plane, so the sums are exact and the same on every run
//   msssim_scale_kernel    (quality_msssim.h) with one channel; scale 0 reads the samples where they lie and takes them to
//                          the codec's 0..255.996 range, v * 2^-(b - 8): MS-SSIM does not change when both planes and the
//                          data range are multiplied by a power of two, and the tile centring stays exact (b + 2k <= 24
//                          significant bits after k pools)
//   quality_finish_kernel  (quality_msssim.h) the ten map means
// One template body per kernel, S = uint8_t / uint16_t, as in picture_ops.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/pmctf_quality.h"
#include "launch.h"
#include "picture_common.h"
#include "quality_msssim.h"

// Workgroups of the error sums at most, and groups of four samples per thread and step.  The atomic adds of all
// workgroups meet in one cache line and are served one after the other: at 1920x1080 4:4:4 the entry took 85 us with 2048
// workgroups, 50 with 1024, 34 with 512 and 30 with 256 (one per compute unit), whatever the step held.
#define PQ_SSE_BLOCKS 256
#define PQ_SSE_UNROLL 4

static_assert(PMCTF_PLANE_MSSSIM_OUT_DOUBLES == 2 * Q_SCALES, "result layout: header and kernel disagree");

// a, b: packed pictures; plane p = 0, 1, 2 starts at sample p ? n_y + (p - 1) * n_c : 0 and has groups_y / groups_c
// groups of four samples, the last one of a plane shorter where its length is no multiple of four
template <typename S>
__global__ __launch_bounds__(P_THREADS) void planar_sse_kernel(const S *__restrict__ a, const S *__restrict__ b, unsigned n_y,
                                                                unsigned n_c, unsigned groups_y, unsigned groups_c,
                                                                unsigned long long *__restrict__ sse3) {
    __shared__ uint64_t red[P_THREADS / 64];
    uint64_t sums[3] = {0, 0, 0};
    const unsigned groups = groups_y + 2u * groups_c, stride = gridDim.x * P_THREADS;
    for (unsigned g0 = blockIdx.x * P_THREADS + threadIdx.x; g0 < groups; g0 += PQ_SSE_UNROLL * stride) {
        unsigned va[PQ_SSE_UNROLL][4], vb[PQ_SSE_UNROLL][4], plane[PQ_SSE_UNROLL], left[PQ_SSE_UNROLL];
        size_t base[PQ_SSE_UNROLL];
        // every load of the step is issued before the first one is used
#pragma unroll
        for (int u = 0; u < PQ_SSE_UNROLL; ++u) {
            const unsigned g = g0 + u * stride;
            const unsigned p = g < groups_y ? 0u : (g - groups_y < groups_c ? 1u : 2u);
            const unsigned i0 = 4u * (p ? g - groups_y - (p - 1u) * groups_c : g), len = p ? n_c : n_y;
            plane[u] = p;
            base[u] = (p ? (size_t)n_y + (size_t)(p - 1u) * n_c : 0) + i0;
            left[u] = g < groups ? len - i0 : 0u;    // samples of the group inside its plane: 4, or 1..3 at a plane's end
            if (left[u] >= 4u) {
                load4(a + base[u], va[u]);
                load4(b + base[u], vb[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < PQ_SSE_UNROLL; ++u) {
            uint64_t s = 0;
            if (left[u] >= 4u) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned d = va[u][k] > vb[u][k] ? va[u][k] - vb[u][k] : vb[u][k] - va[u][k];
                    s += (uint64_t)(d * d);          // d <= 65535: the square fits 32 bits
                }
            } else {
                for (unsigned i = 0; i < left[u]; ++i) {
                    const unsigned x = a[base[u] + i], y = b[base[u] + i], d = x > y ? x - y : y - x;
                    s += (uint64_t)(d * d);
                }
            }
            if (plane[u] == 0) sums[0] += s; else if (plane[u] == 1) sums[1] += s; else sums[2] += s;
        }
    }
    // integers: any order gives the same value
    const uint64_t y = block_sum(sums[0], red), cb = block_sum(sums[1], red), cr = block_sum(sums[2], red);
    if (threadIdx.x == 0) {
        if (y) atomicAdd(sse3, (unsigned long long)y);
        if (cb) atomicAdd(sse3 + 1, (unsigned long long)cb);
        if (cr) atomicAdd(sse3 + 2, (unsigned long long)cr);
    }
}

// ---------------------------------------------------------------------------------------------------- host side
static bool chroma_shift(int fmt, int &sx, int &sy) {
    if (fmt != 420 && fmt != 422 && fmt != 444) return false;
    sx = fmt == 444 ? 0 : 1;
    sy = fmt == 420 ? 1 : 0;
    return true;
}

template <typename S>
static int planar_sse(const S *a, const S *b, int h, int w, int fmt, uint64_t *sse3, void *stream) {
    int sx = 0, sy = 0;
    if (!a || !b || !sse3 || !size_ok(h, w) || !chroma_shift(fmt, sx, sy) ||
        (((uintptr_t)a | (uintptr_t)b) & (sizeof(S) - 1)) || ((uintptr_t)sse3 & 7))
        return PMCTF_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    (void)hipGetLastError();
    if (hipMemsetAsync(sse3, 0, 3 * sizeof(uint64_t), st) != hipSuccess) {           // the clear the atomic adds start from
        (void)pm_launch_status();
        return -2;
    }
    const unsigned n_y = (unsigned)h * (unsigned)w, n_c = (unsigned)(h >> sy) * (unsigned)(w >> sx);
    const unsigned groups_y = (n_y + 3u) / 4u, groups_c = (n_c + 3u) / 4u;
    const long per_block = (long)P_THREADS * PQ_SSE_UNROLL;
    const long blocks = ((long)groups_y + 2L * groups_c + per_block - 1) / per_block;
    PM_LAUNCH(planar_sse_kernel<S>, dim3((unsigned)(blocks < PQ_SSE_BLOCKS ? blocks : PQ_SSE_BLOCKS)), dim3(P_THREADS), 0, st, a,
              b, n_y, n_c, groups_y, groups_c, (unsigned long long *)sse3);
    return pm_launch_status();
}

extern "C" int pmctf_planar_sse_u8(const uint8_t *a, const uint8_t *b, int h, int w, int fmt, uint64_t *sse3, void *stream) {
    return planar_sse(a, b, h, w, fmt, sse3, stream);
}

extern "C" int pmctf_planar_sse_u16(const uint16_t *a, const uint16_t *b, int h, int w, int fmt, int bitdepth, uint64_t *sse3,
                                    void *stream) {
    if (!depth_ok(bitdepth)) return PMCTF_EINVAL;
    return planar_sse(a, b, h, w, fmt, sse3, stream);
}

// a plane of MS-SSIM: any positive sides up to the picture limit, the smaller one above 160
static bool plane_ok(int h, int w) {
    return h > Q_MIN_SIDE && w > Q_MIN_SIDE && h <= P_MAX_SIDE && w <= P_MAX_SIDE;
}
static QLayout plane_layout(int h, int w) { return layout_for(h, w, 1, 0, 1); }

extern "C" int64_t pmctf_plane_msssim_scratch_floats(int h, int w) {
    if (!plane_ok(h, w)) return PMCTF_EINVAL;
    return plane_layout(h, w).total_floats;
}

template <typename S>
static int plane_msssim(const S *a, const S *b, int h, int w, int bitdepth, float *scratch, double *out, void *stream) {
    if (!a || !b || !scratch || !out || !plane_ok(h, w) || (((uintptr_t)a | (uintptr_t)b) & (sizeof(S) - 1)) ||
        ((uintptr_t)scratch & 7) || ((uintptr_t)out & 7))
        return PMCTF_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    const QLayout L = plane_layout(h, w);
    double *partial = (double *)scratch;
    const QWindow win = gauss_window();
    // the data range of v * up: (2^b - 1) * 2^-(b - 8) = 256 - 2^-(b - 8)
    const float up = (float)(1.0 / (double)(1 << (bitdepth - 8)));
    const double range = (double)((1 << bitdepth) - 1) * (double)up;
    const float C1 = (float)((0.01 * range) * (0.01 * range)), C2 = (float)((0.03 * range) * (0.03 * range));
    QSegments<Q_SCALES> segs;
    for (int s = 0; s < Q_SCALES; ++s) {
        const bool last = s == Q_SCALES - 1;
        float *nx = last ? nullptr : scratch + L.plane_off[s + 1];
        float *ny = last ? nullptr : nx + (long)L.H[s + 1] * L.W[s + 1];
        const int Hn = last ? 0 : L.H[s + 1], Wn = last ? 0 : L.W[s + 1];
        const dim3 grid(L.tiles_x[s], L.tiles_y[s], 1);
        if (s == 0) {
            PM_LAUNCH((msssim_scale_kernel<S, 1>), grid, dim3(P_THREADS), 0, st, a, b, h, w, nx, ny, Hn, Wn, L.pad_h[0],
                      L.pad_w[0], win, C1, C2, up, partial + L.partial_off[0]);
        } else {
            const float *x = scratch + L.plane_off[s], *y = x + (long)L.H[s] * L.W[s];
            PM_LAUNCH((msssim_scale_kernel<float, 1>), grid, dim3(P_THREADS), 0, st, x, y, L.H[s], L.W[s], nx, ny, Hn, Wn,
                      L.pad_h[s], L.pad_w[s], win, C1, C2, 1.0f, partial + L.partial_off[s]);
        }
        const int rc = pm_launch_status();
        if (rc) return rc;
        segs.s[s] = {partial + L.partial_off[s], out + 2 * s, L.tiles_y[s] * L.tiles_x[s], 2,
                     1.0 / ((double)(L.H[s] - (Q_TAPS - 1)) * (double)(L.W[s] - (Q_TAPS - 1)))};
    }
    PM_LAUNCH(quality_finish_kernel<Q_SCALES>, dim3(Q_SCALES, 2), dim3(P_THREADS), 0, st, segs);
    return pm_launch_status();
}

extern "C" int pmctf_plane_msssim_u8(const uint8_t *a, const uint8_t *b, int h, int w, float *scratch, double *out,
                                     void *stream) {
    return plane_msssim(a, b, h, w, 8, scratch, out, stream);
}

extern "C" int pmctf_plane_msssim_u16(const uint16_t *a, const uint16_t *b, int h, int w, int bitdepth, float *scratch,
                                      double *out, void *stream) {
    if (!depth_ok(bitdepth)) return PMCTF_EINVAL;
    return plane_msssim(a, b, h, w, bitdepth, scratch, out, stream);
}
