// Quality of a high-bit-depth (b = 9..16) picture as one gfx950 kernel, the 16-bit counterpart of the Y/Cb/Cr sums of
// quality_front_kernel (quality_ops.hip); the pictures themselves come in and go out through picture_ops.hip.  With
// up = 2^(b - 8) and max = 2^b - 1:
//   frame_sse_u16_kernel         sums of (v_hat - v)^2 of Y, Cb and Cr at b bits, v_hat = rint(clamp(x * up, 0, max)) as the
//                                output stage rounds, in 64-bit integers: per thread, per wave, per workgroup, then one
//                                integer atomic add per workgroup and plane (exact, order-free)
// The library is compiled with -ffp-contract=off.  The originals are indexed flat in groups of four samples, 16 bytes per
// lane where the address of either side allows it; a group that crosses a row's or a plane's end goes sample by sample.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pmctf_hip.h"
#include "launch.h"
#include "picture_common.h"

#define H_SSE_BLOCKS 2048                        // grid cap of the error sums: the rest is a grid-stride loop

// (v_hat - v)^2 of one sample pair: below 2^32, so the square is taken on 32 bits
__device__ __forceinline__ uint64_t sq_err(float rec, float org, float up, float top) {
    const int d = (int)round_sample(rec, up, top) - (int)(org * up);
    const unsigned a = (unsigned)(d < 0 ? -d : d);
    return (uint64_t)(a * a);
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

__global__ __launch_bounds__(P_THREADS) void frame_sse_u16_kernel(const float *__restrict__ rec_y, const float *__restrict__ rec_c,
                                                                   const float *__restrict__ org_y, const float *__restrict__ org_c,
                                                                   int Hp, int Wp, int h, int w, float up, float top,
                                                                   unsigned groups_y, unsigned groups_c,
                                                                   unsigned long long *__restrict__ sse3) {
    __shared__ uint64_t red[P_THREADS / 64];
    uint64_t sy[2] = {0, 0}, sc[2] = {0, 0};
    const unsigned groups = groups_y + groups_c;
    for (unsigned g = blockIdx.x * P_THREADS + threadIdx.x; g < groups; g += gridDim.x * P_THREADS) {
        if (g < groups_y)
            sse_group(rec_y, org_y, g, 1, Hp, Wp, h, w, up, top, sy);
        else
            sse_group(rec_c, org_c, g - groups_y, 2, Hp >> 1, Wp >> 1, h >> 1, w >> 1, up, top, sc);
    }
    // integers: any order gives the same value
    const uint64_t y = block_sum(sy[0], red), cb = block_sum(sc[0], red), cr = block_sum(sc[1], red);
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
    const long blocks = ((long)groups_y + groups_c + P_THREADS - 1) / P_THREADS;
    const float up = (float)(1 << (bitdepth - 8)), top = (float)((1 << bitdepth) - 1);
    PM_LAUNCH(frame_sse_u16_kernel, dim3((unsigned)(blocks < H_SSE_BLOCKS ? blocks : H_SSE_BLOCKS)), dim3(P_THREADS), 0, st,
              rec_y, rec_c, org_y, org_c, Hp, Wp, h, w, up, top, groups_y, groups_c, (unsigned long long *)sse3);
    return pm_launch_status();
}
