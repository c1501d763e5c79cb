// Pixel layouts as gfx950 kernels: a picture of h x w as a decoder surface or a capture file holds it (NV12,
// NV21, NV16, P010..P216, YUYV, UYVY, Y210..Y216, V210; include/pmctf_hip.h states each) <-> the packed planar picture of
// the layout's chroma format.  Pure bit movement: shifts, masks, loads and stores.
//
// One launch per picture.  A thread moves one item; the grid holds the items of the first range, then of the second:
//   semi-planar: luma items of 4 samples of a row, then chroma items of 8 interleaved samples (4 Cb, 4 Cr) of a chroma row
//   pair (YUYV family): items of 8 pixels of a row, 16 container samples; one range
//   V210: items of one group of six pixels, 16 bytes; packing also writes the zero groups up to the row's 128-byte end
// Every row is cut into items from its own start, so no item spans two rows and nothing between a row's end and the pitch
// is read or written.  Accesses are as wide as their addresses allow (load4 / store4 of picture_common.h, the 16 bytes of
// a V210 group in one access where they are 16-byte aligned), none wider than the samples still inside the row.
// Byte offsets into the surface are 64-bit (pitch * luma_rows passes 2^32); item and sample indices fit 32 bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pmctf_hip.h"
#include "launch.h"
#include "picture_common.h"

enum { L_SEMI, L_PAIR, L_V210 };

struct LayoutArgs {
    int family;
    int h, w;
    int shift;                                           // 16 - bitdepth for words, 0 for bytes
    unsigned mask;                                       // 2^bitdepth - 1
    int swap;                                            // NV21: Cr first; UYVY: chroma first
    int hc;                                              // rows of a chroma plane
    size_t pitch, chroma_off;                            // bytes; chroma_off = pitch * luma_rows
    unsigned per_row[2];                                 // items of one row in range 0 and 1
    unsigned items[2];
    unsigned blocks0;                                    // blocks of range 0
    unsigned data_groups;                                // V210: groups of a row that hold pixels
};

// the first `cols` (0..4) of four samples at s; the rest 0
template <typename S>
__device__ __forceinline__ void load_cols(const S *__restrict__ s, unsigned v[4], int cols) {
    if (cols >= 4) {
        load4(s, v);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = k < cols ? (unsigned)s[k] : 0u;
    }
}

// n (0..6) 16-bit samples of v[6], in pairs where the address allows.  All indices are compile-time constants, so v stays
// in registers.
__device__ __forceinline__ void load_run(const uint16_t *__restrict__ s, unsigned v[6], int n) {
    const int lead = ((uintptr_t)s & 3) ? 1 : 0;                         // pairs start at s + lead
    if (lead && n > 0) v[0] = s[0];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (!lead) {
            const int k = 2 * j;
            if (k + 1 < n) {
                const uint32_t u = *reinterpret_cast<const uint32_t *>(s + k);
                v[k] = u & 0xffffu, v[k + 1] = u >> 16;
            } else if (k < n) {
                v[k] = s[k];
            }
        } else if (j < 2) {
            const int k = 2 * j + 1;
            if (k + 1 < n) {
                const uint32_t u = *reinterpret_cast<const uint32_t *>(s + k);
                v[k] = u & 0xffffu, v[k + 1] = u >> 16;
            } else if (k < n) {
                v[k] = s[k];
            }
        } else if (5 < n) {
            v[5] = s[5];
        }
    }
}

__device__ __forceinline__ void store_run(uint16_t *__restrict__ o, const unsigned v[6], int n) {
    const int lead = ((uintptr_t)o & 3) ? 1 : 0;
    if (lead && n > 0) o[0] = (uint16_t)v[0];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (!lead) {
            const int k = 2 * j;
            if (k + 1 < n)
                *reinterpret_cast<uint32_t *>(o + k) = v[k] | (v[k + 1] << 16);
            else if (k < n)
                o[k] = (uint16_t)v[k];
        } else if (j < 2) {
            const int k = 2 * j + 1;
            if (k + 1 < n)
                *reinterpret_cast<uint32_t *>(o + k) = v[k] | (v[k + 1] << 16);
            else if (k < n)
                o[k] = (uint16_t)v[k];
        } else if (5 < n) {
            o[5] = (uint16_t)v[5];
        }
    }
}

// the four words of a V210 group at a 4-byte aligned address
__device__ __forceinline__ void load_group(const uint8_t *__restrict__ s, uint32_t q[4]) {
    if (!((uintptr_t)s & 15)) {
        const uint4 u = *reinterpret_cast<const uint4 *>(s);
        q[0] = u.x, q[1] = u.y, q[2] = u.z, q[3] = u.w;
    } else if (!((uintptr_t)s & 7)) {
        const uint2 a = reinterpret_cast<const uint2 *>(s)[0], b = reinterpret_cast<const uint2 *>(s)[1];
        q[0] = a.x, q[1] = a.y, q[2] = b.x, q[3] = b.y;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = reinterpret_cast<const uint32_t *>(s)[k];
    }
}

__device__ __forceinline__ void store_group(uint8_t *__restrict__ d, const uint32_t q[4]) {
    if (!((uintptr_t)d & 15)) {
        *reinterpret_cast<uint4 *>(d) = make_uint4(q[0], q[1], q[2], q[3]);
    } else if (!((uintptr_t)d & 7)) {
        reinterpret_cast<uint2 *>(d)[0] = make_uint2(q[0], q[1]);
        reinterpret_cast<uint2 *>(d)[1] = make_uint2(q[2], q[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) reinterpret_cast<uint32_t *>(d)[k] = q[k];
    }
}

// the item of this thread: false past the end; `range` 0 or 1, `row` and `g` (the item's place in its row) otherwise
__device__ __forceinline__ bool item_of(const LayoutArgs &a, int &range, unsigned &row, unsigned &g) {
    unsigned b = blockIdx.x;
    range = b >= a.blocks0;
    if (range) b -= a.blocks0;
    const unsigned i = b * P_THREADS + threadIdx.x;
    if (i >= a.items[range]) return false;
    row = i / a.per_row[range];
    g = i - row * a.per_row[range];
    return true;
}

template <typename S>
__global__ __launch_bounds__(P_THREADS) void unpack_layout_kernel(const uint8_t *__restrict__ surf, S *__restrict__ dst,
                                                                   const LayoutArgs a) {
    int range;
    unsigned r, g;
    if (!item_of(a, range, r, g)) return;
    const unsigned w = a.w, wc = w >> 1, ny = (unsigned)a.h * w, nc = (unsigned)a.hc * wc;
    if (a.family == L_SEMI) {
        if (range == 0) {
            const int cols = min(4, (int)(w - 4 * g));
            unsigned v[4];
            load_cols(reinterpret_cast<const S *>(surf + (size_t)r * a.pitch) + 4 * g, v, cols);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] >>= a.shift;
            store4(dst + r * w + 4 * g, v, cols);
        } else {
            const int cols = min(4, (int)(wc - 4 * g));                  // samples of each of Cb and Cr
            const S *s = reinterpret_cast<const S *>(surf + a.chroma_off + (size_t)r * a.pitch) + 8 * g;
            unsigned t[8], cb[4], cr[4];
            load_cols(s, t, min(4, 2 * cols));
            load_cols(s + 4, t + 4, max(0, 2 * cols - 4));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                cb[k] = (a.swap ? t[2 * k + 1] : t[2 * k]) >> a.shift;
                cr[k] = (a.swap ? t[2 * k] : t[2 * k + 1]) >> a.shift;
            }
            S *o = dst + ny + r * wc + 4 * g;
            store4(o, cb, cols);
            store4(o + nc, cr, cols);
        }
    } else if (a.family == L_PAIR) {
        const int p = min(8, (int)(w - 8 * g));                          // pixels of the item: 2, 4, 6 or 8
        const S *s = reinterpret_cast<const S *>(surf + (size_t)r * a.pitch) + 16 * g;
        unsigned t[16], y[8], cb[4], cr[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (2 * k < p) {
                load4(s + 4 * k, t + 4 * k);
            } else {
                t[4 * k] = t[4 * k + 1] = t[4 * k + 2] = t[4 * k + 3] = 0;
            }
            y[2 * k] = (a.swap ? t[4 * k + 1] : t[4 * k]) >> a.shift;
            y[2 * k + 1] = (a.swap ? t[4 * k + 3] : t[4 * k + 2]) >> a.shift;
            cb[k] = (a.swap ? t[4 * k] : t[4 * k + 1]) >> a.shift;
            cr[k] = (a.swap ? t[4 * k + 2] : t[4 * k + 3]) >> a.shift;
        }
        S *oy = dst + r * w + 8 * g;
        store4(oy, y, min(4, p));
        if (p > 4) store4(oy + 4, y + 4, p - 4);
        S *oc = dst + ny + r * wc + 4 * g;
        store4(oc, cb, p >> 1);
        store4(oc + nc, cr, p >> 1);
    } else {
        if constexpr (sizeof(S) == 2) {
            const int p = min(6, (int)(w - 6 * g));                      // pixels of the group: 2, 4 or 6
            uint32_t q[4];
            load_group(surf + (size_t)r * a.pitch + (size_t)g * 16, q);
            const unsigned m = 1023u;
            const unsigned y[6] = {(q[0] >> 10) & m, q[1] & m, (q[1] >> 20) & m, (q[2] >> 10) & m, q[3] & m, (q[3] >> 20) & m};
            const unsigned cb[6] = {q[0] & m, (q[1] >> 10) & m, (q[2] >> 20) & m, 0, 0, 0};
            const unsigned cr[6] = {(q[0] >> 20) & m, q[2] & m, (q[3] >> 10) & m, 0, 0, 0};
            store_run(dst + r * w + 6 * g, y, p);
            uint16_t *oc = dst + ny + r * wc + 3 * g;
            store_run(oc, cb, p >> 1);
            store_run(oc + nc, cr, p >> 1);
        }
    }
}

template <typename S>
__global__ __launch_bounds__(P_THREADS) void pack_layout_kernel(const S *__restrict__ src, uint8_t *__restrict__ surf,
                                                                 const LayoutArgs a) {
    int range;
    unsigned r, g;
    if (!item_of(a, range, r, g)) return;
    const unsigned w = a.w, wc = w >> 1, ny = (unsigned)a.h * w, nc = (unsigned)a.hc * wc;
    if (a.family == L_SEMI) {
        if (range == 0) {
            const int cols = min(4, (int)(w - 4 * g));
            unsigned v[4];
            load_cols(src + r * w + 4 * g, v, cols);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = (v[k] & a.mask) << a.shift;
            store4(reinterpret_cast<S *>(surf + (size_t)r * a.pitch) + 4 * g, v, cols);
        } else {
            const int cols = min(4, (int)(wc - 4 * g));
            const S *s = src + ny + r * wc + 4 * g;
            unsigned cb[4], cr[4], t[8];
            load_cols(s, cb, cols);
            load_cols(s + nc, cr, cols);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned b = (cb[k] & a.mask) << a.shift, c = (cr[k] & a.mask) << a.shift;
                t[2 * k] = a.swap ? c : b;
                t[2 * k + 1] = a.swap ? b : c;
            }
            S *o = reinterpret_cast<S *>(surf + a.chroma_off + (size_t)r * a.pitch) + 8 * g;
            store4(o, t, min(4, 2 * cols));
            if (cols > 2) store4(o + 4, t + 4, 2 * cols - 4);
        }
    } else if (a.family == L_PAIR) {
        const int p = min(8, (int)(w - 8 * g));
        const S *sy = src + r * w + 8 * g, *sc = src + ny + r * wc + 4 * g;
        unsigned y[8], cb[4], cr[4], t[16];
        load_cols(sy, y, min(4, p));
        load_cols(sy + 4, y + 4, max(0, p - 4));
        load_cols(sc, cb, p >> 1);
        load_cols(sc + nc, cr, p >> 1);
        S *o = reinterpret_cast<S *>(surf + (size_t)r * a.pitch) + 16 * g;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned y0 = (y[2 * k] & a.mask) << a.shift, y1 = (y[2 * k + 1] & a.mask) << a.shift;
            const unsigned b = (cb[k] & a.mask) << a.shift, c = (cr[k] & a.mask) << a.shift;
            t[4 * k] = a.swap ? b : y0;
            t[4 * k + 1] = a.swap ? y0 : b;
            t[4 * k + 2] = a.swap ? c : y1;
            t[4 * k + 3] = a.swap ? y1 : c;
            if (2 * k < p) store4(o + 4 * k, t + 4 * k, 4);
        }
    } else {
        if constexpr (sizeof(S) == 2) {
            uint32_t q[4] = {0, 0, 0, 0};
            if (g < a.data_groups) {
                const int p = min(6, (int)(w - 6 * g));
                unsigned y[6] = {0, 0, 0, 0, 0, 0}, cb[6] = {0, 0, 0, 0, 0, 0}, cr[6] = {0, 0, 0, 0, 0, 0};
                load_run(src + r * w + 6 * g, y, p);
                const uint16_t *sc = src + ny + r * wc + 3 * g;
                load_run(sc, cb, p >> 1);
                load_run(sc + nc, cr, p >> 1);
                const unsigned m = 1023u;
                q[0] = (cb[0] & m) | ((y[0] & m) << 10) | ((cr[0] & m) << 20);
                q[1] = (y[1] & m) | ((cb[1] & m) << 10) | ((y[2] & m) << 20);
                q[2] = (cr[1] & m) | ((y[3] & m) << 10) | ((cb[2] & m) << 20);
                q[3] = (y[4] & m) | ((cr[2] & m) << 10) | ((y[5] & m) << 20);
            }
            store_group(surf + (size_t)r * a.pitch + (size_t)g * 16, q);
        }
    }
}

static size_t v210_row_bytes(int w) { return (size_t)((w + 47) / 48) * 128; }

// the launch description of a layout for pictures of S; false for what the entries refuse
template <typename S>
static bool layout_args(LayoutArgs &a, int layout, int h, int w, int bitdepth, int64_t pitch, int luma_rows,
                        const void *surface, const void *frame, bool pack) {
    if (!surface || !frame || !size_ok(h, w)) return false;
    int fmt = 0, depth = 0, words = 0, family = 0, swap = 0;
    switch (layout) {
    case PMCTF_LAYOUT_NV12: fmt = 420, depth = 8, family = L_SEMI; break;
    case PMCTF_LAYOUT_NV21: fmt = 420, depth = 8, family = L_SEMI, swap = 1; break;
    case PMCTF_LAYOUT_NV16: fmt = 422, depth = 8, family = L_SEMI; break;
    case PMCTF_LAYOUT_P010: fmt = 420, depth = 10, words = 1, family = L_SEMI; break;
    case PMCTF_LAYOUT_P012: fmt = 420, depth = 12, words = 1, family = L_SEMI; break;
    case PMCTF_LAYOUT_P016: fmt = 420, depth = 16, words = 1, family = L_SEMI; break;
    case PMCTF_LAYOUT_P210: fmt = 422, depth = 10, words = 1, family = L_SEMI; break;
    case PMCTF_LAYOUT_P212: fmt = 422, depth = 12, words = 1, family = L_SEMI; break;
    case PMCTF_LAYOUT_P216: fmt = 422, depth = 16, words = 1, family = L_SEMI; break;
    case PMCTF_LAYOUT_YUYV: fmt = 422, depth = 8, family = L_PAIR; break;
    case PMCTF_LAYOUT_UYVY: fmt = 422, depth = 8, family = L_PAIR, swap = 1; break;
    case PMCTF_LAYOUT_Y210: fmt = 422, depth = 10, words = 1, family = L_PAIR; break;
    case PMCTF_LAYOUT_Y212: fmt = 422, depth = 12, words = 1, family = L_PAIR; break;
    case PMCTF_LAYOUT_Y216: fmt = 422, depth = 16, words = 1, family = L_PAIR; break;
    case PMCTF_LAYOUT_V210: fmt = 422, depth = 10, words = 1, family = L_V210; break;
    default: return false;
    }
    if ((depth > 8) != (sizeof(S) == 2) || bitdepth != depth) return false;
    const size_t container = family == L_V210 ? 4 : sizeof(S);
    const size_t row = family == L_V210 ? v210_row_bytes(w) : (family == L_PAIR ? 2 : 1) * (size_t)w * sizeof(S);
    if (pitch <= 0 || pitch > PMCTF_LAYOUT_MAX_PITCH || (size_t)pitch % container || (size_t)pitch < row) return false;
    if (luma_rows < h || luma_rows > PMCTF_LAYOUT_MAX_LUMA_ROWS) return false;
    if (((uintptr_t)surface & (container - 1)) || ((uintptr_t)frame & (sizeof(S) - 1))) return false;
    a.family = family, a.h = h, a.w = w, a.swap = swap;
    a.shift = words && family != L_V210 ? 16 - depth : 0;
    a.mask = (1u << depth) - 1u;
    a.hc = fmt == 420 ? h / 2 : h;
    a.pitch = (size_t)pitch, a.chroma_off = (size_t)pitch * (size_t)luma_rows;
    a.data_groups = (unsigned)((w + 5) / 6);
    a.per_row[1] = 1, a.items[1] = 0;
    if (family == L_SEMI) {
        a.per_row[0] = (unsigned)((w + 3) / 4), a.items[0] = a.per_row[0] * (unsigned)h;
        a.per_row[1] = (unsigned)((w / 2 + 3) / 4), a.items[1] = a.per_row[1] * (unsigned)a.hc;
    } else if (family == L_PAIR) {
        a.per_row[0] = (unsigned)((w + 7) / 8), a.items[0] = a.per_row[0] * (unsigned)h;
    } else {
        a.per_row[0] = pack ? (unsigned)(row / 16) : a.data_groups, a.items[0] = a.per_row[0] * (unsigned)h;
    }
    a.blocks0 = (a.items[0] + P_THREADS - 1) / P_THREADS;
    return true;
}

static unsigned blocks_of(const LayoutArgs &a) { return a.blocks0 + (a.items[1] + P_THREADS - 1) / P_THREADS; }

template <typename S>
static int unpack_layout(const void *surface, S *frame, int layout, int h, int w, int bitdepth, int64_t pitch,
                         int luma_rows, void *stream) {
    LayoutArgs a;
    if (!layout_args<S>(a, layout, h, w, bitdepth, pitch, luma_rows, surface, frame, false)) return PMCTF_EINVAL;
    PM_LAUNCH(unpack_layout_kernel<S>, dim3(blocks_of(a)), dim3(P_THREADS), 0, (hipStream_t)stream,
              reinterpret_cast<const uint8_t *>(surface), frame, a);
    return pm_launch_status();
}

template <typename S>
static int pack_layout(const S *frame, void *surface, int layout, int h, int w, int bitdepth, int64_t pitch, int luma_rows,
                       void *stream) {
    LayoutArgs a;
    if (!layout_args<S>(a, layout, h, w, bitdepth, pitch, luma_rows, surface, frame, true)) return PMCTF_EINVAL;
    PM_LAUNCH(pack_layout_kernel<S>, dim3(blocks_of(a)), dim3(P_THREADS), 0, (hipStream_t)stream, frame,
              reinterpret_cast<uint8_t *>(surface), a);
    return pm_launch_status();
}

extern "C" int pmctf_unpack_layout_u8(const void *surface, uint8_t *frame, int layout, int h, int w, int64_t pitch,
                                      int luma_rows, void *stream) {
    return unpack_layout<uint8_t>(surface, frame, layout, h, w, 8, pitch, luma_rows, stream);
}

extern "C" int pmctf_unpack_layout_u16(const void *surface, uint16_t *frame, int layout, int h, int w, int bitdepth,
                                       int64_t pitch, int luma_rows, void *stream) {
    return unpack_layout<uint16_t>(surface, frame, layout, h, w, bitdepth, pitch, luma_rows, stream);
}

extern "C" int pmctf_pack_layout_u8(const uint8_t *frame, void *surface, int layout, int h, int w, int64_t pitch,
                                    int luma_rows, void *stream) {
    return pack_layout<uint8_t>(frame, surface, layout, h, w, 8, pitch, luma_rows, stream);
}

extern "C" int pmctf_pack_layout_u16(const uint16_t *frame, void *surface, int layout, int h, int w, int bitdepth,
                                     int64_t pitch, int luma_rows, void *stream) {
    return pack_layout<uint16_t>(frame, surface, layout, h, w, bitdepth, pitch, luma_rows, stream);
}
