// High-bit-depth (9..16 bit) planar 4:2:0 pictures in and out of the codec as gfx950 kernels, the 16-bit siblings of
// yuv420_u8_to_planes_kernel (picture_ops.hip), planes_to_u8_kernel (ew_ops.hip) and the Y/Cb/Cr sums of
// quality_front_kernel (quality_ops.hip).  With s = bitdepth - 8 and max = 2^bitdepth - 1:
//   yuv420_u16_to_planes_kernel  one picture as it lies in a little-endian 16-bit .yuv file -> the model's zero-padded
//                                float inputs x = v * 2^-s (exact for every 16-bit v) and, optionally, the originals
//   planes_to_u16_kernel         padded float planes -> cropped 16-bit planes rint(clamp(x * 2^s, 0, max)), ties to even,
//                                NaN -> 0
//   frame_sse_u16_kernel         sums of (v_hat - v)^2 of Y, Cb and Cr at b bits, in 64-bit integers: per thread, per wave,
//                                per workgroup, then one integer atomic add per workgroup and plane (exact, order-free)
// Both multiplications are by a power of two, so out(in(v)) == v for every v <= max.  The library is compiled with
// -ffp-contract=off.  Every kernel indexes one side flat in groups of four samples and takes the widest access the address
// of either side allows: a plane of 16-bit samples starts on a 2-byte boundary only (the Cr plane of a 6x10 picture at byte
// 150), and a group that crosses a row's or a plane's end goes sample by sample.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pmctf_hip.h"
#include "launch.h"

#define H_THREADS 256
#define H_MAX_SIDE 16384                         // a plane has at most 2^28 samples: flat indices fit 32 bits
#define H_SSE_BLOCKS 2048                        // grid cap of the error sums: the rest is a grid-stride loop

static bool size_ok(int h, int w) { return h > 0 && w > 0 && !((h | w) & 1) && h <= H_MAX_SIDE && w <= H_MAX_SIDE; }
static bool padded_ok(int Hp, int Wp, int h, int w) {
    return Hp >= h && Wp >= w && !((Hp | Wp) & 1) && Hp <= H_MAX_SIDE && Wp <= H_MAX_SIDE;
}
static bool depth_ok(int bitdepth) { return bitdepth >= 9 && bitdepth <= 16; }
static dim3 grid_of(long items) { return dim3((unsigned)((items + H_THREADS - 1) / H_THREADS)); }

// rint(clamp(x * up, 0, top)): fmaxf returns its other operand for a NaN, which so becomes 0
__device__ __forceinline__ unsigned round_u16(float x, float up, float top) {
    return (unsigned)(int)rintf(fminf(fmaxf(x * up, 0.0f), top));
}

// ----------------------------------------------------------------------------------- (a) 16-bit .yuv picture -> float planes
// four samples at s (2-byte aligned) -> v[0..3] as integers
__device__ __forceinline__ void load_u16x4(const uint16_t *__restrict__ s, unsigned v[4]) {
    if (!((uintptr_t)s & 7)) {
        const uint2 u = *reinterpret_cast<const uint2 *>(s);
        v[0] = u.x & 0xffffu; v[1] = u.x >> 16; v[2] = u.y & 0xffffu; v[3] = u.y >> 16;
    } else if (!((uintptr_t)s & 3)) {
        const uint32_t a = reinterpret_cast<const uint32_t *>(s)[0], b = reinterpret_cast<const uint32_t *>(s)[1];
        v[0] = a & 0xffffu; v[1] = a >> 16; v[2] = b & 0xffffu; v[3] = b >> 16;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = s[k];
    }
}

// `planes` planes of rows x cols samples at src -> pad [planes][Rp][Cp] (zero outside the picture) and, if org is not null,
// org [planes][rows][cols].  Group g holds the flat elements 4g .. 4g + 3 of pad (fewer at the very end).
__device__ __forceinline__ void planes_group_u16(const uint16_t *__restrict__ src, float *__restrict__ pad,
                                                 float *__restrict__ org, unsigned g, int planes, int Rp, int Cp, int rows,
                                                 int cols, float down) {
    const unsigned plane_p = (unsigned)Rp * (unsigned)Cp, total = (unsigned)planes * plane_p;
    const unsigned plane_o = (unsigned)rows * (unsigned)cols;
    const unsigned i0 = 4u * g;
    const unsigned p = i0 / plane_p, rem = i0 - p * plane_p;
    const int r = (int)(rem / (unsigned)Cp), c = (int)(rem - (unsigned)r * (unsigned)Cp);
    if (c + 3 < Cp) {                                // the four lie in one row (and so inside the tensor)
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (r < rows && c < cols) {
            const size_t at = (size_t)p * plane_o + (size_t)r * (unsigned)cols + (unsigned)c;
            const uint16_t *s = src + at;
            const bool whole = c + 3 < cols;
            if (whole) {
                unsigned u[4];
                load_u16x4(s, u);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = (float)u[k] * down;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c + k < cols) v[k] = (float)s[k] * down;
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
            v = (float)src[at] * down;
            if (org) org[at] = v;
        }
        pad[i] = v;
    }
}

__global__ __launch_bounds__(H_THREADS) void yuv420_u16_to_planes_kernel(const uint16_t *__restrict__ src,
                                                                          float *__restrict__ y_pad, float *__restrict__ c_pad,
                                                                          float *__restrict__ y_org, float *__restrict__ c_org,
                                                                          int Hp, int Wp, int h, int w, float down,
                                                                          unsigned groups_y, unsigned groups_c) {
    const unsigned g = blockIdx.x * H_THREADS + threadIdx.x;
    if (g < groups_y)
        planes_group_u16(src, y_pad, y_org, g, 1, Hp, Wp, h, w, down);
    else if (g - groups_y < groups_c)
        planes_group_u16(src + (size_t)h * (unsigned)w, c_pad, c_org, g - groups_y, 2, Hp >> 1, Wp >> 1, h >> 1, w >> 1, down);
}

extern "C" int pmctf_yuv420_u16_to_planes_f32(const uint16_t *src, float *y_pad, float *c_pad, float *y_org, float *c_org,
                                              int Hp, int Wp, int h, int w, int bitdepth, void *stream) {
    if (!src || !y_pad || !c_pad || !size_ok(h, w) || !padded_ok(Hp, Wp, h, w) || !depth_ok(bitdepth) ||
        ((uintptr_t)src & 1) || ((uintptr_t)y_pad & 15) || ((uintptr_t)c_pad & 15) || ((uintptr_t)y_org & 3) ||
        ((uintptr_t)c_org & 3))
        return PMCTF_EINVAL;
    const unsigned groups_y = (unsigned)(((long)Hp * Wp + 3) / 4), groups_c = (unsigned)((2L * (Hp >> 1) * (Wp >> 1) + 3) / 4);
    const float down = 1.0f / (float)(1 << (bitdepth - 8));
    PM_LAUNCH(yuv420_u16_to_planes_kernel, grid_of((long)groups_y + groups_c), dim3(H_THREADS), 0, (hipStream_t)stream, src,
              y_pad, c_pad, y_org, c_org, Hp, Wp, h, w, down, groups_y, groups_c);
    return pm_launch_status();
}

// ------------------------------------------------------------------------------------- (b) float planes -> 16-bit planes
// Padded planes [N][Hp][Wp] -> cropped [N][h][w], one flat array of 16-bit samples: a thread makes four consecutive ones
// (they may straddle a row end when w % 4 != 0) and stores them as 8 bytes, two dwords or four halfwords, as the address
// allows; the last total % 4 samples are written one by one.
__device__ __forceinline__ unsigned px_u16(const float *__restrict__ x, unsigned i, int h, int w, int Hp, int Wp, float up,
                                           float top) {
    const unsigned row = i / (unsigned)w, col = i - row * (unsigned)w;
    const unsigned n = row / (unsigned)h, y = row - n * (unsigned)h;
    return round_u16(x[((size_t)n * (unsigned)Hp + y) * (unsigned)Wp + col], up, top);
}

__global__ __launch_bounds__(H_THREADS) void planes_to_u16_kernel(const float *__restrict__ x, uint16_t *__restrict__ out,
                                                                   unsigned total, int Hp, int Wp, int h, int w, float up,
                                                                   float top) {
    const unsigned quads = total >> 2;
    const unsigned q = blockIdx.x * H_THREADS + threadIdx.x;
    if (q < quads) {
        const unsigned i = q << 2;
        unsigned v[4];
        const unsigned row = i / (unsigned)w, col = i - row * (unsigned)w;
        if (col + 3 < (unsigned)w) {                 // one row: one address computation, the loads side by side
            const unsigned n = row / (unsigned)h, y = row - n * (unsigned)h;
            const float *p = x + ((size_t)n * (unsigned)Hp + y) * (unsigned)Wp + col;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = round_u16(p[k], up, top);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = px_u16(x, i + k, h, w, Hp, Wp, up, top);
        }
        uint16_t *o = out + i;
        const unsigned lo = v[0] | (v[1] << 16), hi = v[2] | (v[3] << 16);
        if (!((uintptr_t)o & 7)) {
            *reinterpret_cast<uint2 *>(o) = make_uint2(lo, hi);
        } else if (!((uintptr_t)o & 3)) {
            reinterpret_cast<uint32_t *>(o)[0] = lo;
            reinterpret_cast<uint32_t *>(o)[1] = hi;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = (uint16_t)v[k];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (total & 3u)) {
        const unsigned i = (quads << 2) + threadIdx.x;
        out[i] = (uint16_t)px_u16(x, i, h, w, Hp, Wp, up, top);
    }
}

extern "C" int pmctf_planes_to_u16(const float *x, uint16_t *out, int N, int Hp, int Wp, int h, int w, int bitdepth,
                                   void *stream) {
    // a plane tensor may be the chroma of a picture whose half size is odd (6x10 -> 3x5): odd sizes are valid here, as in
    // pmctf_planes_to_u8
    if (!x || !out || N <= 0 || h <= 0 || w <= 0 || h > Hp || w > Wp || Hp > H_MAX_SIDE || Wp > H_MAX_SIDE ||
        !depth_ok(bitdepth) || ((uintptr_t)x & 3) || ((uintptr_t)out & 1) || (long)N * Hp * Wp > 0x7fffffffL)
        return PMCTF_EINVAL;
    const unsigned total = (unsigned)((long)N * h * w);
    const float up = (float)(1 << (bitdepth - 8)), top = (float)((1 << bitdepth) - 1);
    PM_LAUNCH(planes_to_u16_kernel, grid_of(((long)total + 3) / 4), dim3(H_THREADS), 0, (hipStream_t)stream, x, out, total, Hp,
              Wp, h, w, up, top);
    return pm_launch_status();
}

// --------------------------------------------------------------------------------------------- (c) error sums at b bits
// (v_hat - v)^2 of one sample pair: below 2^32, so the square is taken on 32 bits
__device__ __forceinline__ uint64_t sq_err(float rec, float org, float up, float top) {
    const int d = (int)round_u16(rec, up, top) - (int)(org * up);
    const unsigned a = (unsigned)(d < 0 ? -d : d);
    return (uint64_t)(a * a);
}

// sum over the workgroup in thread 0 (integers: any order gives the same value).  `buf` holds H_THREADS / 64 values.
__device__ __forceinline__ uint64_t block_sum_u64(uint64_t v, uint64_t *buf) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down((unsigned long long)v, off, 64);
    __syncthreads();                             // buf may still be read from the previous call
    if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t s = buf[0];
    for (int i = 1; i < H_THREADS / 64; ++i) s += buf[i];
    return s;
}

// org [planes][rows][cols] flat in groups of four (16 bytes per lane where the addresses allow it) against the crop of rec
// [planes][Rp][Cp]; sums[p] gets plane p's terms
__device__ __forceinline__ void sse_group(const float *__restrict__ rec, const float *__restrict__ org, unsigned g, int planes,
                                          int Rp, int Cp, int rows, int cols, float up, float top, uint64_t sums[2]) {
    const unsigned plane_o = (unsigned)rows * (unsigned)cols, total = (unsigned)planes * plane_o;
    const unsigned i0 = 4u * g;
    const unsigned p = i0 / plane_o, rem = i0 - p * plane_o;
    const unsigned r = rem / (unsigned)cols, c = rem - r * (unsigned)cols;
    if (c + 3 < (unsigned)cols) {                    // the four lie in one row
        const float *o = org + i0;
        const float *x = rec + ((size_t)p * (unsigned)Rp + r) * (unsigned)Cp + c;
        float a[4], b[4];
        if (!((uintptr_t)o & 15)) {
            const float4 t = *reinterpret_cast<const float4 *>(o);
            b[0] = t.x; b[1] = t.y; b[2] = t.z; b[3] = t.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) b[k] = o[k];
        }
        if (!((uintptr_t)x & 15)) {
            const float4 t = *reinterpret_cast<const float4 *>(x);
            a[0] = t.x; a[1] = t.y; a[2] = t.z; a[3] = t.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] = x[k];
        }
        uint64_t s = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) s += sq_err(a[k], b[k], up, top);
        if (p == 0) sums[0] += s; else sums[1] += s;
        return;
    }
    for (unsigned i = i0; i < i0 + 4u && i < total; ++i) {          // a group across a row's or a plane's end
        const unsigned pp = i / plane_o, rm = i - pp * plane_o;
        const unsigned rr = rm / (unsigned)cols, cc = rm - rr * (unsigned)cols;
        const uint64_t s = sq_err(rec[((size_t)pp * (unsigned)Rp + rr) * (unsigned)Cp + cc], org[i], up, top);
        if (pp == 0) sums[0] += s; else sums[1] += s;
    }
}

__global__ __launch_bounds__(H_THREADS) void frame_sse_u16_kernel(const float *__restrict__ rec_y, const float *__restrict__ rec_c,
                                                                   const float *__restrict__ org_y, const float *__restrict__ org_c,
                                                                   int Hp, int Wp, int h, int w, float up, float top,
                                                                   unsigned groups_y, unsigned groups_c,
                                                                   unsigned long long *__restrict__ sse3) {
    __shared__ uint64_t red[H_THREADS / 64];
    uint64_t sy[2] = {0, 0}, sc[2] = {0, 0};
    const unsigned groups = groups_y + groups_c;
    for (unsigned g = blockIdx.x * H_THREADS + threadIdx.x; g < groups; g += gridDim.x * H_THREADS) {
        if (g < groups_y)
            sse_group(rec_y, org_y, g, 1, Hp, Wp, h, w, up, top, sy);
        else
            sse_group(rec_c, org_c, g - groups_y, 2, Hp >> 1, Wp >> 1, h >> 1, w >> 1, up, top, sc);
    }
    const uint64_t y = block_sum_u64(sy[0], red), cb = block_sum_u64(sc[0], red), cr = block_sum_u64(sc[1], red);
    if (threadIdx.x == 0) {
        if (y) atomicAdd(sse3, (unsigned long long)y);
        if (cb) atomicAdd(sse3 + 1, (unsigned long long)cb);
        if (cr) atomicAdd(sse3 + 2, (unsigned long long)cr);
    }
}

extern "C" int pmctf_frame_sse_u16_f32(const float *rec_y, const float *rec_c, const float *org_y, const float *org_c, int Hp,
                                       int Wp, int h, int w, int bitdepth, uint64_t *sse3, void *stream) {
    if (!rec_y || !rec_c || !org_y || !org_c || !sse3 || !size_ok(h, w) || !padded_ok(Hp, Wp, h, w) || !depth_ok(bitdepth) ||
        (((uintptr_t)rec_y | (uintptr_t)rec_c | (uintptr_t)org_y | (uintptr_t)org_c) & 3) || ((uintptr_t)sse3 & 7))
        return PMCTF_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    (void)hipGetLastError();
    if (hipMemsetAsync(sse3, 0, 3 * sizeof(uint64_t), st) != hipSuccess) {           // the clear the atomic adds start from
        (void)pm_launch_status();
        return -2;
    }
    const unsigned groups_y = (unsigned)(((long)h * w + 3) / 4), groups_c = (unsigned)((2L * (h >> 1) * (w >> 1) + 3) / 4);
    const long blocks = ((long)groups_y + groups_c + H_THREADS - 1) / H_THREADS;
    const float up = (float)(1 << (bitdepth - 8)), top = (float)((1 << bitdepth) - 1);
    PM_LAUNCH(frame_sse_u16_kernel, dim3((unsigned)(blocks < H_SSE_BLOCKS ? blocks : H_SSE_BLOCKS)), dim3(H_THREADS), 0, st,
              rec_y, rec_c, org_y, org_c, Hp, Wp, h, w, up, top, groups_y, groups_c, (unsigned long long *)sse3);
    return pm_launch_status();
}
