/* C ABI of the RGB entries of libpmctf_hip.so (csrc/picture_colour.hip): pictures in an RGB layout <-> packed planar 4:4:4
 * YCbCr pictures, by a 3x3 matrix of 29-bit fixed-point integers that the caller hands over (pmctf_colour.coefficients:
 * BT.601 / BT.709 / BT.2020, full or limited range).  DESIGN.md 5s.
 *
 * These entries have a header of their own, as those of pmctf_quality.h have: include/pmctf_hip.h is the table the
 * stream-order and product inventories are pinned to.  Conventions are those of pmctf_hip.h: all picture pointers are DEVICE
 * pointers, `stream` is a hipStream_t passed as void*, nothing allocates or synchronises, 0 on success, PMCTF_EINVAL for a
 * rejected argument (before anything is enqueued), PMCTF_ELAUNCH for a HIP error.
 */
#ifndef PMCTF_COLOUR_H
#define PMCTF_COLOUR_H
#include <stdint.h>

#include "pmctf_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* RGB layouts of a picture of w x h; rows are tight.  "word": little-endian 16 bits, the value in the low bits.
 *   RGB24, BGR24        8 bits   R G B (B G R) bytes per pixel
 *   RGBA, BGRA          8 bits   a fourth byte per pixel: ignored on input, 255 on output
 *   RGB48               16 bits  R G B words per pixel
 *   GBRP                8 bits   planes G, B, R of h x w bytes
 *   GBRP10, 12, 16      10, 12, 16 bits   planes G, B, R of h x w words */
#define PMCTF_RGB_RGB24 0
#define PMCTF_RGB_BGR24 1
#define PMCTF_RGB_RGBA 2
#define PMCTF_RGB_BGRA 3
#define PMCTF_RGB_RGB48 4
#define PMCTF_RGB_GBRP 5
#define PMCTF_RGB_GBRP10 6
#define PMCTF_RGB_GBRP12 7
#define PMCTF_RGB_GBRP16 8
#define PMCTF_COLOUR_FIXED_POINT_BITS 29

/* out = clamp((k[3r] x0 + k[3r+1] x1 + k[3r+2] x2 + (off << 29) + (1 << 28)) >> 29, 0, 2^b - 1) for row r = 0..2, on a
 * 64-bit signed accumulator with an arithmetic shift; b = 8 for the u8 entries, bitdepth for the u16 ones.
 *   rgb_to_ycc: x = (R, G, B), rows give Y, Cb, Cr, off = o[r].  rgb: the surface in `layout`; ycc: h*w samples of Y, then
 *               of Cb, then of Cr.
 *   ycc_to_rgb: x = (Y - o[0], Cb - o[1], Cr - o[2]), rows give R, G, B, off = 0.
 * Samples of a 16-bit input are masked to b bits first.  k and o are HOST pointers, read before the call returns; o[r] is
 * within 0..65535.  Either picture may start at any multiple of its container (1 byte for the u8 entries, 2 for the u16
 * ones); accesses are as wide as each address allows.  h, w even, positive, at most 16384.  bitdepth (u16 entries) is the
 * layout's: 16 for RGB48, 10 / 12 / 16 for GBRP10 / GBRP12 / GBRP16.
 * One launch.  PMCTF_EINVAL for a null pointer (k and o included), an unknown layout, a layout whose depth or container is
 * not the entry's, a 16-bit picture at an odd address, a bad size and an offset outside 0..65535. */
int pmctf_rgb_to_ycc_u8(const void *rgb, uint8_t *ycc, int layout, int h, int w, const int32_t k[9], const int64_t o[3],
                        void *stream);
int pmctf_rgb_to_ycc_u16(const void *rgb, uint16_t *ycc, int layout, int h, int w, int bitdepth, const int32_t k[9],
                         const int64_t o[3], void *stream);
int pmctf_ycc_to_rgb_u8(const uint8_t *ycc, void *rgb, int layout, int h, int w, const int32_t k[9], const int64_t o[3],
                        void *stream);
int pmctf_ycc_to_rgb_u16(const uint16_t *ycc, void *rgb, int layout, int h, int w, int bitdepth, const int32_t k[9],
                         const int64_t o[3], void *stream);

#ifdef __cplusplus
}
#endif
#endif
