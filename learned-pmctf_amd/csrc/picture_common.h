// What the picture kernels share besides the colour arithmetic (picture_math.h): the launch shape and the size limits
// of picture_ops.hip, picture_hbd.hip, picture_scale.hip, picture_chroma.hip, picture_layout.hip, quality_ops.hip,
// quality_planar.hip and scene_ops.hip, the
// workgroup sum, and the access to four neighbouring samples of either width (uint8_t at bit depth 8, uint16_t at 9..16).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define P_THREADS 256                            // threads of a workgroup, in every picture kernel
#define P_MAX_SIDE 16384                         // a plane has at most 2^28 samples: flat indices fit 32 bits

// one side of a 4:2:0 picture; a picture; the padded size around a picture
static bool side_ok(int n) { return n > 0 && !(n & 1) && n <= P_MAX_SIDE; }
static bool size_ok(int h, int w) { return side_ok(h) && side_ok(w); }
static bool padded_ok(int Hp, int Wp, int h, int w) {
    return Hp >= h && Wp >= w && !((Hp | Wp) & 1) && Hp <= P_MAX_SIDE && Wp <= P_MAX_SIDE;
}
static bool depth_ok(int bitdepth) { return bitdepth >= 9 && bitdepth <= 16; }         // of a picture of uint16_t samples
static dim3 grid_of(long items) { return dim3((unsigned)((items + P_THREADS - 1) / P_THREADS)); }

// sum over the workgroup, the same value in every thread; fixed order.  `buf` holds P_THREADS / 64 values.
template <typename T>
__device__ __forceinline__ T block_sum(T v, T *buf) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();                             // buf may still be read from the previous call
    if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = buf[0];
    for (int i = 1; i < P_THREADS / 64; ++i) s += buf[i];
    return s;
}

// rint(clamp(x * up, 0, top)): fmaxf returns its other operand for a NaN, which so becomes 0
__device__ __forceinline__ unsigned round_sample(float x, float up, float top) {
    return (unsigned)(int)rintf(fminf(fmaxf(x * up, 0.0f), top));
}

// four samples at s (aligned to the sample type only) -> v[0..3] as integers, as wide as the address allows
__device__ __forceinline__ void load4(const uint8_t *__restrict__ s, unsigned v[4]) {
    if (!((uintptr_t)s & 3)) {
        const uint32_t u = *reinterpret_cast<const uint32_t *>(s);
        v[0] = u & 255u; v[1] = (u >> 8) & 255u; v[2] = (u >> 16) & 255u; v[3] = u >> 24;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = s[k];
    }
}

__device__ __forceinline__ void load4(const uint16_t *__restrict__ s, unsigned v[4]) {
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

// four neighbouring samples to o, the first `cols` of them inside the plane: one wide store where all four are and the
// address allows it, sample by sample otherwise
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
