// Pictures in and out of the codec as gfx950 kernels; three streaming kernels, one launch each:
//   yuv420_to_rgb8_kernel      reconstruction (padded float planes) -> interleaved RGB bytes [h][w][3], the picture the
//                              harness saves as a PNG (test_pMCTF_flex.py:76-79,301-317,334-336): the rounded RGB picture
//                              of quality_front_kernel, clipped to 0..255
//   yuv420_u8_to_planes_kernel one picture as it lies in a .yuv file -> the model's zero-padded float inputs and,
//                              optionally, the un-padded originals (test_pMCTF_flex.py:151-192)
//   rgb8_to_yuv420_u8_kernel   RGB bytes -> planar 8-bit 4:2:0 (rgb2ycbcr, pMCTF/utils/util.py:21-40, 2x2 chroma mean)
// All three index their OUTPUT flat from its base address in groups of four elements, so that the wide stores are aligned
// whatever the picture's width is; a wide access to the other side is taken when its address allows it, narrower ones
// otherwise (the Cr plane of a .yuv picture starts at an odd byte for some sizes).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pmctf_hip.h"
#include "launch.h"
#include "picture_math.h"

#define P_THREADS 256
#define P_MAX_SIDE 16384                         // a plane has at most 2^28 samples: flat indices fit 32 bits

static bool size_ok(int h, int w) { return h > 0 && w > 0 && !((h | w) & 1) && h <= P_MAX_SIDE && w <= P_MAX_SIDE; }
static bool padded_ok(int Hp, int Wp, int h, int w) {
    return Hp >= h && Wp >= w && !((Hp | Wp) & 1) && Hp <= P_MAX_SIDE && Wp <= P_MAX_SIDE;
}
static dim3 grid_of(long items) { return dim3((unsigned)((items + P_THREADS - 1) / P_THREADS)); }

// ------------------------------------------------------------------------------------------------ (a) YUV 4:2:0 -> RGB
// One thread makes four consecutive pixels of the flat output: 12 bytes, three aligned dwords (h * w is a multiple of 4).
__global__ __launch_bounds__(P_THREADS) void yuv420_to_rgb8_kernel(const float *__restrict__ rec_y,
                                                                    const float *__restrict__ rec_c,
                                                                    uint8_t *__restrict__ out, int Hp, int Wp, int h, int w) {
    const int hc = h >> 1, wc = w >> 1, Wc = Wp >> 1;
    const long plane_p = (long)(Hp >> 1) * Wc;
    const unsigned n4 = ((unsigned)h * (unsigned)w) >> 2;
    const unsigned q = blockIdx.x * P_THREADS + threadIdx.x;
    if (q >= n4) return;
    int y = (int)((q * 4u) / (unsigned)w), x = (int)(q * 4u - (unsigned)y * (unsigned)w);
    unsigned bytes[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // the order of quality_front_kernel for the reconstruction
        const float ry = round_u8(rec_y[(long)y * Wp + x]);
        int r0, r1, c0, c1;
        float wr, wcol;
        up2_taps(y, hc, r0, r1, wr);
        up2_taps(x, wc, c0, c1, wcol);
        float up[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const float *rp = rec_c + p * plane_p;
            const float a00 = round_u8(rp[(long)r0 * Wc + c0]), a01 = round_u8(rp[(long)r0 * Wc + c1]);
            const float a10 = round_u8(rp[(long)r1 * Wc + c0]), a11 = round_u8(rp[(long)r1 * Wc + c1]);
            up[p] = wr * (wcol * a00 + (1.0f - wcol) * a01) + (1.0f - wr) * (wcol * a10 + (1.0f - wcol) * a11);
        }
        float r, g, b;
        to_rgb(ry, up[0], up[1], r, g, b);
        // save_torch_image (test_pMCTF_flex.py:78): clamp(0, 255), then the cast; the values are integers already
        bytes[3 * k] = (unsigned)fminf(fmaxf(r, 0.0f), 255.0f);
        bytes[3 * k + 1] = (unsigned)fminf(fmaxf(g, 0.0f), 255.0f);
        bytes[3 * k + 2] = (unsigned)fminf(fmaxf(b, 0.0f), 255.0f);
        if (++x == w) { x = 0; ++y; }
    }
    uint3 v;
    v.x = bytes[0] | (bytes[1] << 8) | (bytes[2] << 16) | (bytes[3] << 24);
    v.y = bytes[4] | (bytes[5] << 8) | (bytes[6] << 16) | (bytes[7] << 24);
    v.z = bytes[8] | (bytes[9] << 8) | (bytes[10] << 16) | (bytes[11] << 24);
    reinterpret_cast<uint3 *>(out)[q] = v;
}

extern "C" int pmctf_yuv420_to_rgb8_f32(const float *rec_y, const float *rec_c, uint8_t *rgb, int Hp, int Wp, int h, int w,
                                        void *stream) {
    if (!rec_y || !rec_c || !rgb || !size_ok(h, w) || !padded_ok(Hp, Wp, h, w) || ((uintptr_t)rgb & 3)) return PMCTF_EINVAL;
    PM_LAUNCH(yuv420_to_rgb8_kernel, grid_of((long)h * w / 4), dim3(P_THREADS), 0, (hipStream_t)stream, rec_y, rec_c, rgb, Hp,
              Wp, h, w);
    return pm_launch_status();
}

// ------------------------------------------------------------------------------------- (b) .yuv picture -> float planes
// `planes` planes of rows x cols bytes at src -> pad [planes][Rp][Cp] (zero outside the picture) and, if org is not null,
// org [planes][rows][cols].  Group g holds the flat elements 4g .. 4g + 3 of pad (fewer at the very end).
__device__ __forceinline__ void planes_group(const uint8_t *__restrict__ src, float *__restrict__ pad, float *__restrict__ org,
                                             unsigned g, int planes, int Rp, int Cp, int rows, int cols) {
    const unsigned plane_p = (unsigned)Rp * (unsigned)Cp, total = (unsigned)planes * plane_p;
    const unsigned plane_o = (unsigned)rows * (unsigned)cols;
    const unsigned i0 = 4u * g;
    const unsigned p = i0 / plane_p, rem = i0 - p * plane_p;
    const int r = (int)(rem / (unsigned)Cp), c = (int)(rem - (unsigned)r * (unsigned)Cp);
    if (c + 3 < Cp) {                                // the four lie in one row (and so inside the tensor)
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (r < rows && c < cols) {
            const size_t at = (size_t)p * plane_o + (size_t)r * (unsigned)cols + (unsigned)c;
            const uint8_t *s = src + at;
            const bool whole = c + 3 < cols;
            if (whole && !((uintptr_t)s & 3)) {
                const uint32_t u = *reinterpret_cast<const uint32_t *>(s);
                v[0] = (float)(u & 255u); v[1] = (float)((u >> 8) & 255u);
                v[2] = (float)((u >> 16) & 255u); v[3] = (float)(u >> 24);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c + k < cols) v[k] = (float)s[k];
            }
            if (org) {
                float *o = org + at;
                if (whole && !((uintptr_t)o & 15)) {
                    *reinterpret_cast<float4 *>(o) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (c + k < cols) o[k] = v[k];
                }
            }
        }
        *reinterpret_cast<float4 *>(pad + i0) = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
    for (unsigned i = i0; i < i0 + 4u && i < total; ++i) {          // a group across a row's or a plane's end
        const unsigned pp = i / plane_p, rm = i - pp * plane_p;
        const int rr = (int)(rm / (unsigned)Cp), cc = (int)(rm - (unsigned)rr * (unsigned)Cp);
        float v = 0.0f;
        if (rr < rows && cc < cols) {
            const size_t at = (size_t)pp * plane_o + (size_t)rr * (unsigned)cols + (unsigned)cc;
            v = (float)src[at];
            if (org) org[at] = v;
        }
        pad[i] = v;
    }
}

__global__ __launch_bounds__(P_THREADS) void yuv420_u8_to_planes_kernel(const uint8_t *__restrict__ src,
                                                                         float *__restrict__ y_pad, float *__restrict__ c_pad,
                                                                         float *__restrict__ y_org, float *__restrict__ c_org,
                                                                         int Hp, int Wp, int h, int w, unsigned groups_y,
                                                                         unsigned groups_c) {
    const unsigned g = blockIdx.x * P_THREADS + threadIdx.x;
    if (g < groups_y)
        planes_group(src, y_pad, y_org, g, 1, Hp, Wp, h, w);
    else if (g - groups_y < groups_c)
        planes_group(src + (size_t)h * (unsigned)w, c_pad, c_org, g - groups_y, 2, Hp >> 1, Wp >> 1, h >> 1, w >> 1);
}

extern "C" int pmctf_yuv420_u8_to_planes_f32(const uint8_t *src, float *y_pad, float *c_pad, float *y_org, float *c_org,
                                             int Hp, int Wp, int h, int w, void *stream) {
    if (!src || !y_pad || !c_pad || !size_ok(h, w) || !padded_ok(Hp, Wp, h, w) || ((uintptr_t)y_pad & 15) ||
        ((uintptr_t)c_pad & 15) || ((uintptr_t)y_org & 3) || ((uintptr_t)c_org & 3))
        return PMCTF_EINVAL;
    const unsigned groups_y = (unsigned)(((long)Hp * Wp + 3) / 4), groups_c = (unsigned)((2L * (Hp >> 1) * (Wp >> 1) + 3) / 4);
    PM_LAUNCH(yuv420_u8_to_planes_kernel, grid_of((long)groups_y + groups_c), dim3(P_THREADS), 0, (hipStream_t)stream, src,
              y_pad, c_pad, y_org, c_org, Hp, Wp, h, w, groups_y, groups_c);
    return pm_launch_status();
}

// ------------------------------------------------------------------------------------------- (c) RGB -> YUV 4:2:0 bytes
// n = 4 or 2 pixels (12 or 6 bytes) at p -> one byte per entry of d
__device__ __forceinline__ void load_rgb(const uint8_t *__restrict__ p, int n, unsigned d[12]) {
    if (n == 4 && !((uintptr_t)p & 3)) {
        const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t u = q[k];
            d[4 * k] = u & 255u; d[4 * k + 1] = (u >> 8) & 255u; d[4 * k + 2] = (u >> 16) & 255u; d[4 * k + 3] = u >> 24;
        }
    } else if (!((uintptr_t)p & 1)) {
        const uint16_t *q = reinterpret_cast<const uint16_t *>(p);
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (k < 3 * n / 2) {
                const unsigned u = q[k];
                d[2 * k] = u & 255u; d[2 * k + 1] = u >> 8;
            }
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k < 3 * n) d[k] = p[k];
    }
}

// the low n (4, 2 or 1) bytes of v to p, as wide as p's address allows
__device__ __forceinline__ void store_u8(uint8_t *__restrict__ p, unsigned v, int n) {
    if (n == 4 && !((uintptr_t)p & 3)) {
        *reinterpret_cast<uint32_t *>(p) = v;
    } else if (n >= 2 && !((uintptr_t)p & 1)) {
        *reinterpret_cast<uint16_t *>(p) = (uint16_t)(v & 0xffffu);
        if (n == 4) *reinterpret_cast<uint16_t *>(p + 2) = (uint16_t)(v >> 16);
    } else {
        for (int k = 0; k < n; ++k) p[k] = (uint8_t)((v >> (8 * k)) & 255u);
    }
}

// One thread takes two rows of four columns (two columns at the end of a row when w % 4 == 2): 24 bytes in, 8 luma bytes
// and 2 + 2 chroma bytes out.
__global__ __launch_bounds__(P_THREADS) void rgb8_to_yuv420_u8_kernel(const uint8_t *__restrict__ rgb, uint8_t *__restrict__ out,
                                                                       int h, int w) {
    const int hc = h >> 1, wc = w >> 1, gw = (w + 3) >> 2;
    const unsigned t = blockIdx.x * P_THREADS + threadIdx.x;
    if (t >= (unsigned)hc * (unsigned)gw) return;
    const int j = (int)(t / (unsigned)gw), c = 4 * (int)(t - (unsigned)j * (unsigned)gw), n = min(4, w - c);
    float cb[2][4], cr[2][4];
#pragma unroll
    for (int dr = 0; dr < 2; ++dr) {
        const size_t px = (size_t)(2 * j + dr) * (unsigned)w + (unsigned)c;
        unsigned d[12];
        load_rgb(rgb + 3 * px, n, d);
        unsigned luma = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) {
                const float R = (float)d[3 * k], G = (float)d[3 * k + 1], B = (float)d[3 * k + 2];
                const float y = (0.299f * R + 0.587f * G) + 0.114f * B;          // util.py:34
                cb[dr][k] = (B - y) * 0.564f + 128.0f;                           // util.py:35, on the unrounded y
                cr[dr][k] = (R - y) * 0.713f + 128.0f;                           // util.py:36
                luma |= (unsigned)round_u8(y) << (8 * k);
            }
        store_u8(out + px, luma, n);
    }
    unsigned vb = 0, vr = 0;
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (2 * k < n) {
            const float mb = (((cb[0][2 * k] + cb[0][2 * k + 1]) + cb[1][2 * k]) + cb[1][2 * k + 1]) * 0.25f;
            const float mr = (((cr[0][2 * k] + cr[0][2 * k + 1]) + cr[1][2 * k]) + cr[1][2 * k + 1]) * 0.25f;
            vb |= (unsigned)round_u8(mb) << (8 * k);
            vr |= (unsigned)round_u8(mr) << (8 * k);
        }
    uint8_t *ob = out + (size_t)h * (unsigned)w + (size_t)j * (unsigned)wc + (unsigned)(c >> 1);
    store_u8(ob, vb, n >> 1);
    store_u8(ob + (size_t)hc * (unsigned)wc, vr, n >> 1);
}

extern "C" int pmctf_rgb8_to_yuv420_u8(const uint8_t *rgb, uint8_t *yuv, int h, int w, void *stream) {
    if (!rgb || !yuv || !size_ok(h, w)) return PMCTF_EINVAL;
    PM_LAUNCH(rgb8_to_yuv420_u8_kernel, grid_of((long)(h >> 1) * ((w + 3) >> 2)), dim3(P_THREADS), 0, (hipStream_t)stream,
              rgb, yuv, h, w);
    return pm_launch_status();
}
