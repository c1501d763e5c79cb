// math_probe.hip — diagnostic entry point: the scalar functions of pm_device_math.h (and the two generated headers it
// includes) evaluated on given float32 bit patterns, one result per pattern.  The codec never calls it; the suite sweeps
// it over all 2^32 inputs against the oracle (tests/test_gpu_math_sweep.py), which is what checks the code the GPU
// compiler makes of these functions: f32 and f64 FMA, division, conversions, subnormals, the table in LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pm_device_math.h"
#include "launch.h"
#include "../../include/pmctf_hip.h"

namespace {

__device__ __forceinline__ float probe_eval(int fn, float x, float slope, const uint4 *tanh_lds) {
    switch (fn) {
    case PMCTF_PROBE_TANH: return pm::tanhf_(x);
    case PMCTF_PROBE_TANH_LDS: return pm::tanhf_rows(x, tanh_lds);
    case PMCTF_PROBE_SIGMOID: return pm::sigmoidf_(x);
    case PMCTF_PROBE_SIGMOID_SCALAR: return pm_aten_sigmoidf_scalar(x);
    case PMCTF_PROBE_LOG: return pm::logf_(x);
    case PMCTF_PROBE_LOG_POLY: return pm::logf_poly_(x);
    case PMCTF_PROBE_EXP: return pm::expf_(x);
    case PMCTF_PROBE_GLIBC_EXP: return pm_glibc_expf(x);
    default: return pm::apply_act(x, fn - PMCTF_PROBE_ACT, slope);     // PMCTF_PROBE_ACT + PMCTF_ACT_*
    }
}

// A thread owns four consecutive elements and writes them with one 16-byte store; the last n % 4 elements are written one
// by one by the first threads of workgroup 0.  Without `bits`, element i is the pattern first_bits + i (mod 2^32).
__global__ __launch_bounds__(256) void math_probe_kernel(int fn, const uint32_t *__restrict__ bits, uint32_t first_bits,
                                                         long n, float *y, float slope) {
    __shared__ uint4 tanh_tab[pm::TANH_LDS_UINT4];
    pm::tanh_rows_to_lds(tanh_tab, threadIdx.x, blockDim.x);
    __syncthreads();
    const long groups = n >> 2;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
        const long i = g * 4;
        float r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t u = bits ? bits[i + k] : first_bits + (uint32_t)(i + k);
            r[k] = probe_eval(fn, pm::u2f(u), slope, tanh_tab);
        }
        *(float4 *)(y + i) = make_float4(r[0], r[1], r[2], r[3]);
    }
    const long i = groups * 4 + threadIdx.x;
    if (blockIdx.x == 0 && i < n) {
        const uint32_t u = bits ? bits[i] : first_bits + (uint32_t)i;
        y[i] = probe_eval(fn, pm::u2f(u), slope, tanh_tab);
    }
}

}  // namespace

extern "C" int pmctf_math_probe_f32(int fn, const uint32_t *bits, uint32_t first_bits, int64_t n, float *y, float slope,
                                    void *stream) {
    const bool known = (fn >= PMCTF_PROBE_TANH && fn <= PMCTF_PROBE_GLIBC_EXP) ||
                       (fn >= PMCTF_PROBE_ACT + PMCTF_ACT_RELU && fn <= PMCTF_PROBE_ACT + PMCTF_ACT_SIGMOID);
    if (!y || ((uintptr_t)y & 15) || n <= 0 || n > ((int64_t)1 << 32) || !known) return PMCTF_EINVAL;
    long blocks = ((n >> 2) + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 16384) blocks = 16384;
    PM_LAUNCH(math_probe_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, fn, bits, first_bits, (long)n,
              y, slope);
    return pm_launch_status();
}
