// Colour arithmetic of the evaluation harness's pictures, shared by the quality kernels (quality_ops.hip) and the picture
// input / output kernels (picture_ops.hip): one copy, so that a decoded PNG holds exactly the RGB picture RGB-PSNR and
// MS-SSIM were taken on.  The library is compiled with -ffp-contract=off: every operation below rounds once to float32.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

__device__ __forceinline__ float round_u8(float v) { return rintf(fminf(fmaxf(v, 0.0f), 255.0f)); }

// x2 bilinear, align_corners=False, of a plane of integers: output sample o takes input samples i0, i1 with weights
// w0, 1 - w0 (0.25 / 0.75, clamped at the edges).  Exact in float32 for integer inputs <= 255.
__device__ __forceinline__ void up2_taps(int o, int n, int &i0, int &i1, float &w0) {
    const int k = o >> 1;
    if (o & 1) {
        i0 = k;
        i1 = min(k + 1, n - 1);
        w0 = 0.75f;
    } else {
        i0 = max(k - 1, 0);
        i1 = k;
        w0 = 0.25f;
    }
}

// pMCTF/utils/util.py:ycbcr2rgb followed by round, in the written order
__device__ __forceinline__ void to_rgb(float y, float cb, float cr, float &r, float &g, float &b) {
    const float dcb = cb - 128.0f, dcr = cr - 128.0f;
    r = rintf(y + 1.403f * dcr);
    g = rintf((y - 0.714f * dcr) - 0.344f * dcb);
    b = rintf(y + 1.773f * dcb);
}
