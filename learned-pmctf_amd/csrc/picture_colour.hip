// RGB pictures as gfx950 kernels: a picture of h x w in an RGB layout (RGB24, BGR24, RGBA, BGRA, RGB48, GBRP,
// GBRP10 / 12 / 16; include/pmctf_colour.h states each) <-> the packed planar 4:4:4 YCbCr picture, by a 3x3 matrix of
// 29-bit fixed-point integers and three offsets that travel by value in the kernel arguments.  Integers only: a row is three
// 32 x 32 -> 64-bit multiply-adds, a rounding add, an arithmetic shift and a clamp.  No LDS, no division, no float.
//
// One launch per picture.  A thread makes four consecutive pixels of the flat picture (h * w is a multiple of 4, the sides
// being even), so no thread is ragged: 12 samples of an interleaved three-component layout (three load4: one dword each at
// 8 bits, 8 bytes each at 16), the 16 bytes of four RGBA pixels (one access where they are 16-byte aligned), or four
// samples of each of the three planes.  Accesses are as wide as their addresses allow (load4 / store4 of picture_common.h).
// Byte offsets into the surface are 64-bit (a 16384 x 16384 RGB48 picture has 1.6 GB); item indices fit 32 bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pmctf_colour.h"
#include "launch.h"
#include "picture_common.h"

enum { C_PACKED3, C_PACKED4, C_PLANAR };
#define C_BITS PMCTF_COLOUR_FIXED_POINT_BITS

struct ColourArgs {
    int kind;
    int swap;                                            // BGR24, BGRA: blue first
    unsigned items;                                      // h * w / 4
    size_t plane;                                        // h * w: samples of a plane
    unsigned mask;                                       // 2^bitdepth - 1, the largest output too
    int k[9];
    long long o[3];
};

// the 16 bytes of four four-component pixels
__device__ __forceinline__ void load_quad(const uint8_t *__restrict__ s, unsigned q[4]) {
    if (!((uintptr_t)s & 15)) {
        const uint4 u = *reinterpret_cast<const uint4 *>(s);
        q[0] = u.x, q[1] = u.y, q[2] = u.z, q[3] = u.w;
    } else if (!((uintptr_t)s & 3)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = reinterpret_cast<const uint32_t *>(s)[j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            q[j] = (unsigned)s[4 * j] | ((unsigned)s[4 * j + 1] << 8) | ((unsigned)s[4 * j + 2] << 16) |
                   ((unsigned)s[4 * j + 3] << 24);
    }
}

__device__ __forceinline__ void store_quad(uint8_t *__restrict__ d, const unsigned q[4]) {
    if (!((uintptr_t)d & 15)) {
        *reinterpret_cast<uint4 *>(d) = make_uint4(q[0], q[1], q[2], q[3]);
    } else if (!((uintptr_t)d & 3)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) reinterpret_cast<uint32_t *>(d)[j] = q[j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            d[4 * j] = (uint8_t)q[j], d[4 * j + 1] = (uint8_t)(q[j] >> 8);
            d[4 * j + 2] = (uint8_t)(q[j] >> 16), d[4 * j + 3] = (uint8_t)(q[j] >> 24);
        }
    }
}

// row r of the matrix on (x0, x1, x2) with the offset off: rounded, shifted and clamped to 0..top
__device__ __forceinline__ unsigned colour_row(const ColourArgs &a, int r, int x0, int x1, int x2, long long off) {
    long long acc = (off << C_BITS) + (1ll << (C_BITS - 1));
    acc += (long long)a.k[3 * r] * x0;
    acc += (long long)a.k[3 * r + 1] * x1;
    acc += (long long)a.k[3 * r + 2] * x2;
    acc >>= C_BITS;
    return (unsigned)min(max(acc, 0ll), (long long)a.mask);
}

template <typename S>
__global__ __launch_bounds__(P_THREADS) void rgb_to_ycc_kernel(const uint8_t *__restrict__ surf, S *__restrict__ dst,
                                                                const ColourArgs a) {
    const unsigned i = blockIdx.x * P_THREADS + threadIdx.x;
    if (i >= a.items) return;
    unsigned r[4], g[4], b[4];
    if (a.kind == C_PACKED3) {
        const S *s = reinterpret_cast<const S *>(surf) + (size_t)i * 12;
        unsigned t[12];
        load4(s, t);
        load4(s + 4, t + 4);
        load4(s + 8, t + 8);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            r[p] = a.swap ? t[3 * p + 2] : t[3 * p];
            g[p] = t[3 * p + 1];
            b[p] = a.swap ? t[3 * p] : t[3 * p + 2];
        }
    } else if (a.kind == C_PACKED4) {
        unsigned q[4];
        load_quad(surf + (size_t)i * 16, q);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const unsigned c0 = q[p] & 255u, c2 = (q[p] >> 16) & 255u;
            r[p] = a.swap ? c2 : c0;
            g[p] = (q[p] >> 8) & 255u;
            b[p] = a.swap ? c0 : c2;
        }
    } else {
        const S *s = reinterpret_cast<const S *>(surf) + (size_t)i * 4;
        load4(s, g);
        load4(s + a.plane, b);
        load4(s + 2 * a.plane, r);
    }
    unsigned y[4], cb[4], cr[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int x0 = (int)(r[p] & a.mask), x1 = (int)(g[p] & a.mask), x2 = (int)(b[p] & a.mask);
        y[p] = colour_row(a, 0, x0, x1, x2, a.o[0]);
        cb[p] = colour_row(a, 1, x0, x1, x2, a.o[1]);
        cr[p] = colour_row(a, 2, x0, x1, x2, a.o[2]);
    }
    S *o = dst + (size_t)i * 4;
    store4(o, y, 4);
    store4(o + a.plane, cb, 4);
    store4(o + 2 * a.plane, cr, 4);
}

template <typename S>
__global__ __launch_bounds__(P_THREADS) void ycc_to_rgb_kernel(const S *__restrict__ src, uint8_t *__restrict__ surf,
                                                                const ColourArgs a) {
    const unsigned i = blockIdx.x * P_THREADS + threadIdx.x;
    if (i >= a.items) return;
    const S *s = src + (size_t)i * 4;
    unsigned y[4], cb[4], cr[4], r[4], g[4], b[4];
    load4(s, y);
    load4(s + a.plane, cb);
    load4(s + 2 * a.plane, cr);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int x0 = (int)(y[p] & a.mask) - (int)a.o[0], x1 = (int)(cb[p] & a.mask) - (int)a.o[1];
        const int x2 = (int)(cr[p] & a.mask) - (int)a.o[2];
        r[p] = colour_row(a, 0, x0, x1, x2, 0);
        g[p] = colour_row(a, 1, x0, x1, x2, 0);
        b[p] = colour_row(a, 2, x0, x1, x2, 0);
    }
    if (a.kind == C_PACKED3) {
        unsigned t[12];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            t[3 * p] = a.swap ? b[p] : r[p];
            t[3 * p + 1] = g[p];
            t[3 * p + 2] = a.swap ? r[p] : b[p];
        }
        S *o = reinterpret_cast<S *>(surf) + (size_t)i * 12;
        store4(o, t, 4);
        store4(o + 4, t + 4, 4);
        store4(o + 8, t + 8, 4);
    } else if (a.kind == C_PACKED4) {
        unsigned q[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) q[p] = (a.swap ? b[p] : r[p]) | (g[p] << 8) | ((a.swap ? r[p] : b[p]) << 16) | (255u << 24);
        store_quad(surf + (size_t)i * 16, q);
    } else {
        S *o = reinterpret_cast<S *>(surf) + (size_t)i * 4;
        store4(o, g, 4);
        store4(o + a.plane, b, 4);
        store4(o + 2 * a.plane, r, 4);
    }
}

// the launch description of a layout for pictures of S; false for what the entries refuse
template <typename S>
static bool colour_args(ColourArgs &a, int layout, int h, int w, int bitdepth, const int32_t *k, const int64_t *o,
                        const void *surface, const void *frame) {
    if (!surface || !frame || !k || !o || !size_ok(h, w)) return false;
    int depth = 0, kind = 0, swap = 0;
    switch (layout) {
    case PMCTF_RGB_RGB24: depth = 8, kind = C_PACKED3; break;
    case PMCTF_RGB_BGR24: depth = 8, kind = C_PACKED3, swap = 1; break;
    case PMCTF_RGB_RGBA: depth = 8, kind = C_PACKED4; break;
    case PMCTF_RGB_BGRA: depth = 8, kind = C_PACKED4, swap = 1; break;
    case PMCTF_RGB_RGB48: depth = 16, kind = C_PACKED3; break;
    case PMCTF_RGB_GBRP: depth = 8, kind = C_PLANAR; break;
    case PMCTF_RGB_GBRP10: depth = 10, kind = C_PLANAR; break;
    case PMCTF_RGB_GBRP12: depth = 12, kind = C_PLANAR; break;
    case PMCTF_RGB_GBRP16: depth = 16, kind = C_PLANAR; break;
    default: return false;
    }
    if ((depth > 8) != (sizeof(S) == 2) || bitdepth != depth) return false;
    if (((uintptr_t)surface | (uintptr_t)frame) & (sizeof(S) - 1)) return false;
    for (int r = 0; r < 3; ++r)
        if (o[r] < 0 || o[r] > 65535) return false;
    a.kind = kind, a.swap = swap;
    a.plane = (size_t)h * (size_t)w;
    a.items = (unsigned)(a.plane / 4);
    a.mask = (1u << depth) - 1u;
    for (int j = 0; j < 9; ++j) a.k[j] = k[j];
    for (int r = 0; r < 3; ++r) a.o[r] = o[r];
    return true;
}

template <typename S>
static int rgb_to_ycc(const void *rgb, S *ycc, int layout, int h, int w, int bitdepth, const int32_t *k, const int64_t *o,
                      void *stream) {
    ColourArgs a;
    if (!colour_args<S>(a, layout, h, w, bitdepth, k, o, rgb, ycc)) return PMCTF_EINVAL;
    PM_LAUNCH(rgb_to_ycc_kernel<S>, grid_of((long)a.items), dim3(P_THREADS), 0, (hipStream_t)stream,
              reinterpret_cast<const uint8_t *>(rgb), ycc, a);
    return pm_launch_status();
}

template <typename S>
static int ycc_to_rgb(const S *ycc, void *rgb, int layout, int h, int w, int bitdepth, const int32_t *k, const int64_t *o,
                      void *stream) {
    ColourArgs a;
    if (!colour_args<S>(a, layout, h, w, bitdepth, k, o, rgb, ycc)) return PMCTF_EINVAL;
    PM_LAUNCH(ycc_to_rgb_kernel<S>, grid_of((long)a.items), dim3(P_THREADS), 0, (hipStream_t)stream, ycc,
              reinterpret_cast<uint8_t *>(rgb), a);
    return pm_launch_status();
}

extern "C" int pmctf_rgb_to_ycc_u8(const void *rgb, uint8_t *ycc, int layout, int h, int w, const int32_t k[9],
                                   const int64_t o[3], void *stream) {
    return rgb_to_ycc<uint8_t>(rgb, ycc, layout, h, w, 8, k, o, stream);
}

extern "C" int pmctf_rgb_to_ycc_u16(const void *rgb, uint16_t *ycc, int layout, int h, int w, int bitdepth,
                                    const int32_t k[9], const int64_t o[3], void *stream) {
    return rgb_to_ycc<uint16_t>(rgb, ycc, layout, h, w, bitdepth, k, o, stream);
}

extern "C" int pmctf_ycc_to_rgb_u8(const uint8_t *ycc, void *rgb, int layout, int h, int w, const int32_t k[9],
                                   const int64_t o[3], void *stream) {
    return ycc_to_rgb<uint8_t>(ycc, rgb, layout, h, w, 8, k, o, stream);
}

extern "C" int pmctf_ycc_to_rgb_u16(const uint16_t *ycc, void *rgb, int layout, int h, int w, int bitdepth,
                                    const int32_t k[9], const int64_t o[3], void *stream) {
    return ycc_to_rgb<uint16_t>(ycc, rgb, layout, h, w, bitdepth, k, o, stream);
}
