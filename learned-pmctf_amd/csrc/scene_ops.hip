// Pre-analysis of a sequence's structure as one gfx950 kernel: the luma histogram of a picture and its sum of absolute
// differences against the previous picture, the two figures pmctf_seq.scene_cuts looks at.  With s = bitdepth - 8 a luma
// original x (v * 2^-s, as planes_from_u8 / planes_from_u16 return it) is taken back to its integer
//   u = rint(clamp(x * 2^s, 0, 65535))        (exact for every original; NaN -> 0)
// and   hist256[min(u >> s, 255)] += 1,   sad += |u_cur - u_prev|.
// Everything is integers: a private 256-bin histogram per wave in LDS (LDS atomic adds; a picture of one value puts every
// lane on one bin, which serialises that instruction and nothing else), the waves added after a barrier, every non-zero
// bin flushed with one global integer atomic per workgroup; the SAD in uint64_t per thread, per wave (__shfl_down), per
// workgroup (LDS), one 64-bit integer atomic per workgroup.  Integer atomics commute: the result is exact and the same on
// every run.  The pattern of frame_sse_u16_kernel (picture_hbd.hip): 16-byte loads, a grid-stride loop, at most 2048
// workgroups, the last h*w % 4 elements one by one.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pmctf_hip.h"
#include "launch.h"
#include "picture_common.h"

#define S_WAVES (P_THREADS / 64)
#define S_BINS 256
#define S_MAX_BLOCKS 2048                        // grid cap: the rest is a grid-stride loop

__device__ __forceinline__ unsigned luma_u16(float x, float up) { return round_sample(x, up, 65535.0f); }

__device__ __forceinline__ void count(uint32_t *wave_hist, unsigned u, int shift) {
    const unsigned bin = u >> shift;
    atomicAdd(&wave_hist[bin < S_BINS - 1 ? bin : S_BINS - 1], 1u);
}

__device__ __forceinline__ uint64_t abs_diff(unsigned a, unsigned b) { return (uint64_t)(a > b ? a - b : b - a); }

__global__ __launch_bounds__(P_THREADS) void luma_activity_kernel(const float *__restrict__ cur, const float *__restrict__ prev,
                                                                   unsigned total, float up, int shift,
                                                                   uint32_t *__restrict__ hist256,
                                                                   unsigned long long *__restrict__ sad) {
    __shared__ uint32_t hist[S_WAVES][S_BINS];   // 4 KB: one private histogram per wave
    __shared__ uint64_t red[S_WAVES];
#pragma unroll
    for (int k = 0; k < S_WAVES; ++k) hist[k][threadIdx.x] = 0u;
    __syncthreads();
    uint32_t *mine = hist[threadIdx.x >> 6];
    uint64_t s = 0;
    const unsigned quads = total >> 2;
    for (unsigned q = blockIdx.x * P_THREADS + threadIdx.x; q < quads; q += gridDim.x * P_THREADS) {
        const float4 c = reinterpret_cast<const float4 *>(cur)[q];
        const unsigned u[4] = {luma_u16(c.x, up), luma_u16(c.y, up), luma_u16(c.z, up), luma_u16(c.w, up)};
#pragma unroll
        for (int k = 0; k < 4; ++k) count(mine, u[k], shift);
        if (prev) {
            const float4 p = reinterpret_cast<const float4 *>(prev)[q];
            s += abs_diff(u[0], luma_u16(p.x, up)) + abs_diff(u[1], luma_u16(p.y, up)) + abs_diff(u[2], luma_u16(p.z, up)) +
                 abs_diff(u[3], luma_u16(p.w, up));
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (total & 3u)) {             // the last total % 4 elements, one by one
        const unsigned i = (quads << 2) + threadIdx.x;
        const unsigned u = luma_u16(cur[i], up);
        count(mine, u, shift);
        if (prev) s += abs_diff(u, luma_u16(prev[i], up));
    }
    __syncthreads();
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < S_WAVES; ++k) n += hist[k][threadIdx.x];
    if (n) atomicAdd(hist256 + threadIdx.x, n);
    if (prev) {                                  // uniform over the launch
        // block_sum's leading barrier guards a reuse of red; red is used once here, so that barrier is harmless, not needed
        const uint64_t t = block_sum(s, red);
        if (threadIdx.x == 0 && t) atomicAdd(sad, (unsigned long long)t);
    }
}

extern "C" int pmctf_luma_activity_f32(const float *cur, const float *prev, int h, int w, int bitdepth, uint32_t *hist256,
                                       uint64_t *sad, void *stream) {
    if (!cur || !hist256 || (prev && !sad) || bitdepth < 8 || bitdepth > 16 || h < 1 || w < 1 || h > P_MAX_SIDE ||
        w > P_MAX_SIDE || (((uintptr_t)cur | (uintptr_t)prev) & 15) || ((uintptr_t)hist256 & 3) || ((uintptr_t)sad & 7))
        return PMCTF_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    (void)hipGetLastError();
    // the clears the atomic adds start from
    if (hipMemsetAsync(hist256, 0, S_BINS * sizeof(uint32_t), st) != hipSuccess ||
        (prev && hipMemsetAsync(sad, 0, sizeof(uint64_t), st) != hipSuccess)) {
        (void)pm_launch_status();
        return -2;
    }
    const unsigned total = (unsigned)((long)h * w);
    const long blocks = ((long)(total >> 2) + P_THREADS - 1) / P_THREADS;
    const unsigned grid = (unsigned)(blocks < 1 ? 1 : (blocks < S_MAX_BLOCKS ? blocks : S_MAX_BLOCKS));
    PM_LAUNCH(luma_activity_kernel, dim3(grid), dim3(P_THREADS), 0, st, cur, prev, total, (float)(1 << (bitdepth - 8)),
              bitdepth - 8, hist256, (unsigned long long *)sad);
    return pm_launch_status();
}
