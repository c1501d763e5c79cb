// Resampling of planar 4:2:0 pictures as one gfx950 kernel: the separable Catmull-Rom bicubic (a = -1/2) with an
// antialiasing stretch of DESIGN 5l, in integers.  The host (pmctf_scale.py) builds, per axis, a table
//     int32 start[n_out];  int16 coef[n_out][T];          (one device buffer, 4-byte aligned)
// whose rows sum to 16384.  Per plane, with max = 2^b - 1:
//     horizontal  t   = (sum_k coef_x[ox][k] * src[r][min(start_x[ox] + k, w_in - 1)] + 32) >> 6             (int32)
//     vertical    out = clamp((sum_k coef_y[oy][k] * t[min(start_y[oy] + k, h_in - 1)][ox] + 2^21) >> 22, 0, max)   (int64)
// All sums are integer sums: the result does not depend on their order.
//
// One launch per picture: the grid holds the tiles of Y, then of Cb, then of Cr.  A workgroup of 256 threads owns a tile
// of S_TH x S_TW output samples.  It makes the horizontal pass of the source rows the tile needs into LDS (int32, row
// stride S_TW: lane i of a wave touches bank i, no conflicts) and the vertical pass from there, one thread per four
// neighbouring outputs (one 16-byte LDS read per tap).  Nothing intermediate goes to HBM.
//
// A 16-row tile at the steepest reduction (4:1, 17 taps) needs 15 * 4 + 1 + 17 = 78 source rows: S_ROWS = 80 rows of
// S_TW int32 are 20 KiB, the x coefficients (S_TAPS x S_TW int32) 5 KiB more, so six workgroups fit the 160 KiB of a CU.
// Every index read from a table is clamped before use (source column and row, LDS row): a wrong table gives wrong
// samples, never an access outside the two pictures.
//
// Accesses take the widest form the address allows, as picture_hbd.hip does: planes of a packed picture start on odd
// byte (u8) or halfword (u16) boundaries.  A thread reads its window of a source row as aligned 32-bit words where the
// window holds whole ones and sample by sample at its ends, and stores its four outputs as one word (u8), or as 8 bytes
// or two words (u16), when they lie in one row at such an address; sample by sample otherwise.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pmctf_hip.h"
#include "launch.h"

#define S_THREADS 256
#define S_TW 64                                  // tile width in output samples
#define S_TH 16                                  // tile height
#define S_ROWS 80                                // source rows of one tile held in LDS
#define S_TAPS 20                                // longest table row accepted (the 4:1 limit needs 17)
#define S_MAX_SIDE 16384

struct ScalePlane {
    int h_in, w_in, h_out, w_out;
    int tx, ty;                                  // taps per row of the x and the y table
    const int32_t *start_x, *start_y;
    const int16_t *coef_x, *coef_y;
    unsigned tiles_x, tiles;                     // tiles per tile row, tiles of the plane
    size_t in_off, out_off;                      // the plane's first sample in src / dst
};

struct ScaleArgs {
    ScalePlane p[3];
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// sum_k c[k * S_TW] * s[k], k < n: s is aligned to its sample type only.  Whole aligned 32-bit words of the window are
// read as words, what lies before and after them sample by sample.
__device__ __forceinline__ int window_sum(const uint8_t *__restrict__ s, int n, const int *__restrict__ c) {
    int acc = 0, k = 0;
    for (; k < n && ((uintptr_t)(s + k) & 3); ++k) acc += c[k * S_TW] * (int)s[k];
    for (; k + 4 <= n; k += 4) {
        const uint32_t u = *reinterpret_cast<const uint32_t *>(s + k);
        acc += c[k * S_TW] * (int)(u & 0xffu) + c[(k + 1) * S_TW] * (int)((u >> 8) & 0xffu) +
               c[(k + 2) * S_TW] * (int)((u >> 16) & 0xffu) + c[(k + 3) * S_TW] * (int)(u >> 24);
    }
    for (; k < n; ++k) acc += c[k * S_TW] * (int)s[k];
    return acc;
}

__device__ __forceinline__ int window_sum(const uint16_t *__restrict__ s, int n, const int *__restrict__ c) {
    int acc = 0, k = 0;
    if (n > 0 && ((uintptr_t)s & 3)) {
        acc += c[0] * (int)s[0];
        k = 1;
    }
    for (; k + 2 <= n; k += 2) {
        const uint32_t u = *reinterpret_cast<const uint32_t *>(s + k);
        acc += c[k * S_TW] * (int)(u & 0xffffu) + c[(k + 1) * S_TW] * (int)(u >> 16);
    }
    if (k < n) acc += c[k * S_TW] * (int)s[k];
    return acc;
}

// four neighbouring outputs of one row, `cols` of them inside the plane
__device__ __forceinline__ void store4(uint8_t *__restrict__ o, const unsigned v[4], int cols) {
    if (cols >= 4 && !((uintptr_t)o & 3)) {
        *reinterpret_cast<uint32_t *>(o) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cols) o[k] = (uint8_t)v[k];
    }
}

__device__ __forceinline__ void store4(uint16_t *__restrict__ o, const unsigned v[4], int cols) {
    const unsigned lo = v[0] | (v[1] << 16), hi = v[2] | (v[3] << 16);
    if (cols >= 4 && !((uintptr_t)o & 7)) {
        *reinterpret_cast<uint2 *>(o) = make_uint2(lo, hi);
    } else if (cols >= 4 && !((uintptr_t)o & 3)) {
        reinterpret_cast<uint32_t *>(o)[0] = lo;
        reinterpret_cast<uint32_t *>(o)[1] = hi;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cols) o[k] = (uint16_t)v[k];
    }
}

template <typename S>
__global__ __launch_bounds__(S_THREADS) void resize_yuv420_kernel(const S *__restrict__ src, S *__restrict__ dst,
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
    const int oy0 = (int)(tile / P.tiles_x) * S_TH, ox0 = (int)(tile % P.tiles_x) * S_TW;
    const int tid = threadIdx.x;

    // the source rows of this tile: start_y never decreases, so its first and last output rows bound them
    const int oy_last = min(oy0 + S_TH, P.h_out) - 1;
    const int r0 = clampi(P.start_y[oy0], 0, P.h_in - 1);
    const int r1 = min(P.start_y[oy_last] + P.ty, P.h_in);
    const int nrows = clampi(r1 - r0, 1, S_ROWS);

    // x coefficients of the tile's columns, tap-major: cx[k][column]; zero past the plane's last column
    for (int i = tid; i < P.tx * S_TW; i += S_THREADS) {
        const int k = i / S_TW, col = i - k * S_TW;
        cx[i] = ox0 + col < P.w_out ? (int)P.coef_x[(size_t)(ox0 + col) * P.tx + k] : 0;
    }
    __syncthreads();

    // horizontal pass: thread -> one column of the tile, every fourth source row
    {
        const int col = tid & (S_TW - 1);
        const bool live = ox0 + col < P.w_out;
        const int xs = live ? clampi(P.start_x[ox0 + col], 0, P.w_in - 1) : 0;
        const int n = live ? min(P.tx, P.w_in - xs) : 0;        // taps past the row's end have zero coefficients
        const S *plane = src + P.in_off;
        for (int r = tid / S_TW; r < nrows; r += S_THREADS / S_TW) {
            const S *s = plane + (size_t)(r0 + r) * (unsigned)P.w_in + xs;
            tmp[r * S_TW + col] = (window_sum(s, n, cx + col) + 32) >> 6;
        }
    }
    __syncthreads();

    // vertical pass: thread -> four neighbouring outputs of one row
    {
        const int oy = oy0 + tid / (S_TW / 4), q = (tid & (S_TW / 4 - 1)) * 4;
        const int cols = P.w_out - (ox0 + q);
        if (oy < P.h_out && cols > 0) {
            const int ys = P.start_y[oy] - r0;
            const int16_t *cy = P.coef_y + (size_t)oy * P.ty;
            long long acc[4] = {0, 0, 0, 0};
            for (int k = 0; k < P.ty; ++k) {
                const long long c = cy[k];
                const int4 t = *reinterpret_cast<const int4 *>(tmp + clampi(ys + k, 0, nrows - 1) * S_TW + q);
                acc[0] += c * t.x;
                acc[1] += c * t.y;
                acc[2] += c * t.z;
                acc[3] += c * t.w;
            }
            unsigned v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long o = (acc[k] + (1LL << 21)) >> 22;
                v[k] = (unsigned)(o < 0 ? 0 : (o > top ? top : o));
            }
            store4(dst + P.out_off + (size_t)oy * (unsigned)P.w_out + (unsigned)(ox0 + q), v, cols);
        }
    }
}

static bool side_ok(int n) { return n > 0 && !(n & 1) && n <= S_MAX_SIDE; }
static bool ratio_ok(int n_in, int n_out) { return 4L * n_out >= n_in && n_out <= 4L * n_in; }
static bool taps_ok(int t) { return t >= 1 && t <= S_TAPS; }

static void set_plane(ScalePlane &p, int h_in, int w_in, int h_out, int w_out, const void *tab_x, int tx, const void *tab_y,
                      int ty, size_t in_off, size_t out_off) {
    p.h_in = h_in, p.w_in = w_in, p.h_out = h_out, p.w_out = w_out;
    p.tx = tx, p.ty = ty;
    p.start_x = (const int32_t *)tab_x;
    p.coef_x = (const int16_t *)(p.start_x + w_out);
    p.start_y = (const int32_t *)tab_y;
    p.coef_y = (const int16_t *)(p.start_y + h_out);
    p.tiles_x = (unsigned)((w_out + S_TW - 1) / S_TW);
    p.tiles = p.tiles_x * (unsigned)((h_out + S_TH - 1) / S_TH);
    p.in_off = in_off, p.out_off = out_off;
}

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
    PM_LAUNCH(resize_yuv420_kernel<S>, dim3(blocks), dim3(S_THREADS), 0, (hipStream_t)stream, src, dst, a,
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
    if (bitdepth < 9 || bitdepth > 16) return PMCTF_EINVAL;
    return resize_yuv420<uint16_t>(src, dst, h_in, w_in, h_out, w_out, luma_x, luma_y, chroma_x, chroma_y, taps, bitdepth,
                                   stream);
}
