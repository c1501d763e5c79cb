// The tile body of the integer picture resampling, shared by picture_scale.hip (4:2:0 pictures to another
// size) and picture_chroma.hip (chroma planes to another chroma format).  Per plane, with max = 2^b - 1:
//     horizontal  t   = (sum_k coef_x[ox][k] * src[r][min(start_x[ox] + k, w_in - 1)] + 32) >> 6             (int32)
//     vertical    out = clamp((sum_k coef_y[oy][k] * t[min(start_y[oy] + k, h_in - 1)][ox] + 2^21) >> 22, 0, max)   (int64)
// A workgroup of P_THREADS threads owns a tile of S_TH x S_TW output samples.  It makes the horizontal pass of the source
// rows the tile needs into LDS (int32, row stride S_TW: lane i of a wave touches bank i, no conflicts) and the vertical
// pass from there, one thread per four neighbouring outputs (one 16-byte LDS read per tap).  Nothing intermediate goes to
// HBM.  Every index read from a table is clamped before use (source column and row, LDS row): a wrong table gives wrong
// samples, never an access outside the two pictures.
//
// An axis whose length does not change has the table start[i] = i, coef[i] = {16384}: its pass is exact (the horizontal
// one gives 256 x, the vertical one (t + 128) >> 8, clamped), so the template flags IDX / IDY compute just that without
// reading a table.
//
// Accesses take the widest form the address allows, as picture_ops.hip does: planes of a packed picture start on odd
// byte (u8) or halfword (u16) boundaries.  A thread reads its window of a source row as aligned 32-bit words where the
// window holds whole ones and sample by sample at its ends, and stores its four outputs with store4 (picture_common.h):
// one word (u8), or 8 bytes or two words (u16), when they lie in one row at such an address; sample by sample otherwise.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "picture_common.h"

#define S_TW 64                                  // tile width in output samples
#define S_TH 16                                  // tile height
#define S_ROWS 80                                // source rows of one tile held in LDS
#define S_TAPS 20                                // longest table row accepted (the 4:1 limit needs 17)

struct ScalePlane {
    int h_in, w_in, h_out, w_out;
    int tx, ty;                                  // taps per row of the x and the y table
    const int32_t *start_x, *start_y;
    const int16_t *coef_x, *coef_y;
    unsigned tiles_x, tiles;                     // tiles per tile row, tiles of the plane
    size_t in_off, out_off;                      // the plane's first sample in src / dst
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

// one tile of plane P; tmp: S_ROWS * S_TW ints of LDS, 16-byte aligned, cx: S_TAPS * S_TW ints of LDS.  The whole
// workgroup calls it (it synchronises).  IDX / IDY: that axis keeps its length, its table is not read.
template <typename S, bool IDX, bool IDY>
__device__ __forceinline__ void resample_tile(const S *__restrict__ src, S *__restrict__ dst, const ScalePlane &P,
                                              unsigned tile, int top, int *__restrict__ tmp, int *__restrict__ cx) {
    const int oy0 = (int)(tile / P.tiles_x) * S_TH, ox0 = (int)(tile % P.tiles_x) * S_TW;
    const int tid = threadIdx.x;

    // the source rows of this tile: start_y never decreases, so its first and last output rows bound them
    const int oy_last = min(oy0 + S_TH, P.h_out) - 1;
    int r0, nrows;
    if constexpr (IDY) {
        r0 = oy0;
        nrows = oy_last - oy0 + 1;
    } else {
        r0 = clampi(P.start_y[oy0], 0, P.h_in - 1);
        const int r1 = min(P.start_y[oy_last] + P.ty, P.h_in);
        nrows = clampi(r1 - r0, 1, S_ROWS);
    }

    if constexpr (!IDX) {
        // x coefficients of the tile's columns, tap-major: cx[k][column]; zero past the plane's last column
        for (int i = tid; i < P.tx * S_TW; i += P_THREADS) {
            const int k = i / S_TW, col = i - k * S_TW;
            cx[i] = ox0 + col < P.w_out ? (int)P.coef_x[(size_t)(ox0 + col) * P.tx + k] : 0;
        }
        __syncthreads();
    }

    // horizontal pass: thread -> one column of the tile, every fourth source row
    {
        const int col = tid & (S_TW - 1);
        const bool live = ox0 + col < P.w_out;
        const S *plane = src + P.in_off;
        if constexpr (IDX) {
            const int xs = live ? min(ox0 + col, P.w_in - 1) : 0;
            for (int r = tid / S_TW; r < nrows; r += P_THREADS / S_TW)
                tmp[r * S_TW + col] = live ? (int)plane[(size_t)(r0 + r) * (unsigned)P.w_in + xs] << 8 : 0;
        } else {
            const int xs = live ? clampi(P.start_x[ox0 + col], 0, P.w_in - 1) : 0;
            const int n = live ? min(P.tx, P.w_in - xs) : 0;        // taps past the row's end have zero coefficients
            for (int r = tid / S_TW; r < nrows; r += P_THREADS / S_TW) {
                const S *s = plane + (size_t)(r0 + r) * (unsigned)P.w_in + xs;
                tmp[r * S_TW + col] = (window_sum(s, n, cx + col) + 32) >> 6;
            }
        }
    }
    __syncthreads();

    // vertical pass: thread -> four neighbouring outputs of one row
    {
        const int oy = oy0 + tid / (S_TW / 4), q = (tid & (S_TW / 4 - 1)) * 4;
        const int cols = P.w_out - (ox0 + q);
        if (oy < P.h_out && cols > 0) {
            unsigned v[4];
            if constexpr (IDY) {
                const int4 t = *reinterpret_cast<const int4 *>(tmp + (oy - r0) * S_TW + q);
                const int o[4] = {(t.x + 128) >> 8, (t.y + 128) >> 8, (t.z + 128) >> 8, (t.w + 128) >> 8};
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = (unsigned)clampi(o[k], 0, top);
            } else {
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
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const long long o = (acc[k] + (1LL << 21)) >> 22;
                    v[k] = (unsigned)(o < 0 ? 0 : (o > top ? top : o));
                }
            }
            store4(dst + P.out_off + (size_t)oy * (unsigned)P.w_out + (unsigned)(ox0 + q), v, cols);
        }
    }
}

static inline void set_plane(ScalePlane &p, int h_in, int w_in, int h_out, int w_out, const void *tab_x, int tx,
                             const void *tab_y, int ty, size_t in_off, size_t out_off) {
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
