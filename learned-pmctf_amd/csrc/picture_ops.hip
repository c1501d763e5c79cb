// Pictures in and out of the codec as gfx950 kernels; four streaming kernels, one launch each:
//   yuv420_to_rgb8_kernel      reconstruction (padded float planes) -> interleaved RGB bytes [h][w][3], the picture the
//                              harness saves as a PNG (test_pMCTF_flex.py:76-79,301-317,334-336): the rounded RGB picture
//                              of quality_front_kernel, clipped to 0..255
//   yuv420_to_planes_kernel<S> one picture as it lies in a .yuv file -> the model's zero-padded float inputs and,
//                              optionally, the un-padded originals (test_pMCTF_flex.py:151-192)
//   rgb8_to_yuv420_u8_kernel   RGB bytes -> planar 8-bit 4:2:0 (rgb2ycbcr, pMCTF/utils/util.py:21-40, 2x2 chroma mean)
//   planes_to_samples_kernel<S> padded float planes -> cropped planes of samples, the decoder's output stage
// S is the sample type: uint8_t at bit depth 8, uint16_t (little-endian words of a 16-bit .yuv file) at b = 9..16.  With
// s = b - 8 and max = 2^b - 1 a sample v comes in as x = v * 2^-s (exact for every 16-bit v; no multiplication at 8 bits)
// and goes out as rint(clamp(x * 2^s, 0, max)), ties to even, NaN -> 0: both factors are powers of two, so
// out(in(v)) == v for every v <= max.
// All four index their OUTPUT flat from its base address in groups of four elements; a wide access to either side is
// taken when its address allows it, narrower ones otherwise (picture_common.h: load4, store4).  The Cr plane of a .yuv
// picture starts at an odd byte (halfword) for some sizes, and the cropped chroma of a 6x10 picture is 3x5.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pmctf_hip.h"
#include "launch.h"
#include "picture_common.h"
#include "picture_math.h"

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
// a sample as the model's float: v at 8 bits, v * down at more (down = 2^-(b - 8))
template <typename S>
__device__ __forceinline__ float to_float(unsigned v, float down) {
    if constexpr (sizeof(S) == 1) return (float)v;
    else return (float)v * down;
}

// `planes` planes of rows x cols samples at src -> pad [planes][Rp][Cp] (zero outside the picture) and, if org is not null,
// org [planes][rows][cols].  Group g holds the flat elements 4g .. 4g + 3 of pad (fewer at the very end).
template <typename S>
__device__ __forceinline__ void planes_group(const S *__restrict__ src, float *__restrict__ pad, float *__restrict__ org,
                                             unsigned g, int planes, int Rp, int Cp, int rows, int cols, float down) {
    const unsigned plane_p = (unsigned)Rp * (unsigned)Cp, total = (unsigned)planes * plane_p;
    const unsigned plane_o = (unsigned)rows * (unsigned)cols;
    const unsigned i0 = 4u * g;
    const unsigned p = i0 / plane_p, rem = i0 - p * plane_p;
    const int r = (int)(rem / (unsigned)Cp), c = (int)(rem - (unsigned)r * (unsigned)Cp);
    if (c + 3 < Cp) {                                // the four lie in one row (and so inside the tensor)
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (r < rows && c < cols) {
            const size_t at = (size_t)p * plane_o + (size_t)r * (unsigned)cols + (unsigned)c;
            const S *s = src + at;
            const bool whole = c + 3 < cols;
            if (whole) {
                unsigned u[4];
                load4(s, u);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = to_float<S>(u[k], down);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c + k < cols) v[k] = to_float<S>(s[k], down);
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
            v = to_float<S>(src[at], down);
            if (org) org[at] = v;
        }
        pad[i] = v;
    }
}

template <typename S>
__global__ __launch_bounds__(P_THREADS) void yuv420_to_planes_kernel(const S *__restrict__ src, float *__restrict__ y_pad,
                                                                      float *__restrict__ c_pad, float *__restrict__ y_org,
                                                                      float *__restrict__ c_org, int Hp, int Wp, int h, int w,
                                                                      float down, unsigned groups_y, unsigned groups_c) {
    const unsigned g = blockIdx.x * P_THREADS + threadIdx.x;
    if (g < groups_y)
        planes_group(src, y_pad, y_org, g, 1, Hp, Wp, h, w, down);
    else if (g - groups_y < groups_c)
        planes_group(src + (size_t)h * (unsigned)w, c_pad, c_org, g - groups_y, 2, Hp >> 1, Wp >> 1, h >> 1, w >> 1, down);
}

// bitdepth: 8 for uint8_t, checked by the entry for uint16_t
template <typename S>
static int yuv420_to_planes(const S *src, float *y_pad, float *c_pad, float *y_org, float *c_org, int Hp, int Wp, int h, int w,
                            int bitdepth, void *stream) {
    if (!src || !y_pad || !c_pad || !size_ok(h, w) || !padded_ok(Hp, Wp, h, w) || ((uintptr_t)src & (sizeof(S) - 1)) ||
        ((uintptr_t)y_pad & 15) || ((uintptr_t)c_pad & 15) || ((uintptr_t)y_org & 3) || ((uintptr_t)c_org & 3))
        return PMCTF_EINVAL;
    const unsigned groups_y = (unsigned)(((long)Hp * Wp + 3) / 4), groups_c = (unsigned)((2L * (Hp >> 1) * (Wp >> 1) + 3) / 4);
    const float down = 1.0f / (float)(1 << (bitdepth - 8));
    PM_LAUNCH(yuv420_to_planes_kernel<S>, grid_of((long)groups_y + groups_c), dim3(P_THREADS), 0, (hipStream_t)stream, src,
              y_pad, c_pad, y_org, c_org, Hp, Wp, h, w, down, groups_y, groups_c);
    return pm_launch_status();
}

extern "C" int pmctf_yuv420_u8_to_planes_f32(const uint8_t *src, float *y_pad, float *c_pad, float *y_org, float *c_org,
                                             int Hp, int Wp, int h, int w, void *stream) {
    return yuv420_to_planes<uint8_t>(src, y_pad, c_pad, y_org, c_org, Hp, Wp, h, w, 8, stream);
}

extern "C" int pmctf_yuv420_u16_to_planes_f32(const uint16_t *src, float *y_pad, float *c_pad, float *y_org, float *c_org,
                                              int Hp, int Wp, int h, int w, int bitdepth, void *stream) {
    if (!depth_ok(bitdepth)) return PMCTF_EINVAL;
    return yuv420_to_planes<uint16_t>(src, y_pad, c_pad, y_org, c_org, Hp, Wp, h, w, bitdepth, stream);
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

// ------------------------------------------------------------------------------------- (d) float planes -> sample planes
// Padded planes [N][Hp][Wp] -> cropped [N][h][w], one flat array of samples rint(clamp(x * up, 0, top)) with up = 2^(b - 8),
// top = 2^b - 1: a thread makes four consecutive ones (they may straddle a row end when w % 4 != 0) and stores them as
// wide as their address allows; the last total % 4 samples are written one by one.
__device__ __forceinline__ unsigned px_sample(const float *__restrict__ x, unsigned i, int h, int w, int Hp, int Wp, float up,
                                              float top) {
    const unsigned row = i / (unsigned)w, col = i - row * (unsigned)w;
    const unsigned n = row / (unsigned)h, y = row - n * (unsigned)h;
    return round_sample(x[((size_t)n * (unsigned)Hp + y) * (unsigned)Wp + col], up, top);
}

template <typename S>
__global__ __launch_bounds__(P_THREADS) void planes_to_samples_kernel(const float *__restrict__ x, S *__restrict__ out,
                                                                       unsigned total, int Hp, int Wp, int h, int w, float up,
                                                                       float top) {
    const unsigned quads = total >> 2;
    const unsigned q = blockIdx.x * P_THREADS + threadIdx.x;
    if (q < quads) {
        const unsigned i = q << 2;
        unsigned v[4];
        const unsigned row = i / (unsigned)w, col = i - row * (unsigned)w;
        if (col + 3 < (unsigned)w) {                 // one row: one address computation, the loads side by side
            const unsigned n = row / (unsigned)h, y = row - n * (unsigned)h;
            const float *p = x + ((size_t)n * (unsigned)Hp + y) * (unsigned)Wp + col;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = round_sample(p[k], up, top);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = px_sample(x, i + k, h, w, Hp, Wp, up, top);
        }
        store4(out + i, v, 4);
    }
    if (blockIdx.x == 0 && threadIdx.x < (total & 3u)) {
        const unsigned i = (quads << 2) + threadIdx.x;
        out[i] = (S)px_sample(x, i, h, w, Hp, Wp, up, top);
    }
}

// A plane tensor may be the chroma of a picture whose half size is odd (6x10 -> 3x5): odd sizes are valid here.  Each entry
// adds its own refusals; N * Hp * Wp <= 2^31 - 1 keeps every flat index of the kernel on 32 bits.
template <typename S>
static int planes_to_samples(const float *x, S *out, int N, int Hp, int Wp, int h, int w, int bitdepth, void *stream) {
    if (!x || !out || N <= 0 || h <= 0 || w <= 0 || h > Hp || w > Wp) return PMCTF_EINVAL;
    const unsigned total = (unsigned)((long)N * h * w);
    const float up = (float)(1 << (bitdepth - 8)), top = (float)((1 << bitdepth) - 1);
    PM_LAUNCH(planes_to_samples_kernel<S>, grid_of(((long)total + 3) / 4), dim3(P_THREADS), 0, (hipStream_t)stream, x, out,
              total, Hp, Wp, h, w, up, top);
    return pm_launch_status();
}

extern "C" int pmctf_planes_to_u8(const float *x, uint8_t *out, int N, int Hp, int Wp, int h, int w, void *stream) {
    if ((long)N * Hp * Wp > 0x7fffffffL) return PMCTF_EINVAL;          // no side limit, no alignment asked of out
    return planes_to_samples<uint8_t>(x, out, N, Hp, Wp, h, w, 8, stream);
}

extern "C" int pmctf_planes_to_u16(const float *x, uint16_t *out, int N, int Hp, int Wp, int h, int w, int bitdepth,
                                   void *stream) {
    if (Hp > P_MAX_SIDE || Wp > P_MAX_SIDE || !depth_ok(bitdepth) || ((uintptr_t)x & 3) || ((uintptr_t)out & 1) ||
        (long)N * Hp * Wp > 0x7fffffffL)
        return PMCTF_EINVAL;
    return planes_to_samples<uint16_t>(x, out, N, Hp, Wp, h, w, bitdepth, stream);
}
