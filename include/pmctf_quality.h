/* C ABI of the per-plane quality entries of libpmctf_hip.so (csrc/quality_planar.hip): squared-error sums and MS-SSIM of
 * planar pictures as they lie in files, 4:2:0, 4:2:2 or 4:4:4, at 8 bits (uint8_t samples) or 9..16 bits (uint16_t
 * samples), in the picture's own format and data range.  DESIGN.md 5p.
 *
 * These entries have a header of their own: include/pmctf_hip.h is the table the stream-order and product inventories
 * are pinned to, entry for entry; the entries here are held to the same rules by tests/test_gpu_planar_quality.py.
 * Conventions are those of pmctf_hip.h: all pointers are DEVICE pointers, `stream` is a hipStream_t passed as void*,
 * nothing allocates or synchronises, 0 on success, PMCTF_EINVAL for a rejected argument (before anything is enqueued),
 * PMCTF_ELAUNCH for a HIP error.
 */
#ifndef PMCTF_QUALITY_H
#define PMCTF_QUALITY_H
#include <stdint.h>

#include "pmctf_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Sums of squared differences of two packed planar pictures, per plane.
 *   a, b: h*w luma samples followed by two planes of (h/sy)*(w/sx) samples, (sx, sy) = (2,2), (2,1), (1,1) for
 *   fmt = 420, 422, 444 (the integer codes of pmctf_convert_chroma_*).  A u8 picture may start at any byte, a u16 picture
 *   at any even byte; the loads are as wide as each address allows.  h, w even, positive, at most 16384.
 *   sse3[0..2] = sum (a - b)^2 over Y, Cb, Cr: 64-bit integers (one term can be 65535^2), 8-byte aligned.  Integer atomic
 *   adds, one per workgroup and plane: exact, and the same on every run.  bitdepth (u16 entry): 9..16; the samples are
 *   taken as they are.
 * One clear of sse3 and one launch.  PMCTF_EINVAL for a null pointer, a u16 picture at an odd address, a misaligned sse3,
 * an unknown fmt, a bad size and a bitdepth outside 9..16. */
int pmctf_planar_sse_u8(const uint8_t *a, const uint8_t *b, int h, int w, int fmt, uint64_t *sse3, void *stream);
int pmctf_planar_sse_u16(const uint16_t *a, const uint16_t *b, int h, int w, int fmt, int bitdepth, uint64_t *sse3,
                         void *stream);

/* MS-SSIM map means of one plane against another: the algorithm of pmctf_frame_quality_f32 with one channel, at the
 * plane's own data range L = 2^b - 1 (b = 8 for the u8 entry): C1 = (0.01 L)^2, C2 = (0.03 L)^2.
 *   a, b: h x w samples each, aligned to the sample; any h, w up to 16384 (odd ones too) with min(h, w) > 160.
 *   out[2*s + k], s = scale 0..4: spatial mean of the cs map (k = 0) and of the ssim map (k = 1), 10 doubles, 8-byte
 *   aligned.  The product  prod_{s<4} relu(cs_s)^w_s * relu(ssim_4)^w_4  is left to the caller.
 *   The kernels work on v * 2^-(b - 8) with L scaled alike, which leaves every map value unchanged.
 *   scratch: pmctf_plane_msssim_scratch_floats(h, w) floats, 8-byte aligned, no initial contents required.
 *   Per-workgroup partial sums are added in a fixed order: the same input gives the same bits on every run.
 * Launches: 5 (one per scale; scale 0 reads the samples where they lie) + 1 (final sums); no memset.
 * pmctf_plane_msssim_scratch_floats is host arithmetic; PMCTF_EINVAL for the sizes the entries refuse. */
#define PMCTF_PLANE_MSSSIM_OUT_DOUBLES 10
int64_t pmctf_plane_msssim_scratch_floats(int h, int w);
int pmctf_plane_msssim_u8(const uint8_t *a, const uint8_t *b, int h, int w, float *scratch, double *out, void *stream);
int pmctf_plane_msssim_u16(const uint16_t *a, const uint16_t *b, int h, int w, int bitdepth, float *scratch, double *out,
                           void *stream);

#ifdef __cplusplus
}
#endif
#endif
