// Chroma format conversion of packed planar pictures as one gfx950 kernel: a picture of h x w in 4:2:0,
// 4:2:2 or 4:4:4 (Y of h x w, then Cb and Cr of h/sy x w/sx each, as it lies in a file) -> the picture of another of the
// three formats.  Y is copied; Cb and Cr go through the two integer passes of DESIGN 5l with the host's tables
// (pmctf_chroma.chroma_tables), an axis whose length does not change through the exact short cut of its single-tap table.
//
// One launch per picture.  The grid holds the copy blocks, then the tiles of Cb, then of Cr.
//   copy blocks: the destination range is cut into C_CHUNK-byte chunks on 16-byte boundaries of the DESTINATION.  A
//     thread moves 16-byte slots; a slot that lies wholly inside the range is moved in pieces of g bytes, g the largest
//     power of two up to 16 that divides the distance between source and destination (16: one 128-bit load and store, the
//     case of two tensors from an allocator), a slot that the range's ends cut, byte by byte.  No access is wider than
//     its address allows and none lies outside [src, src + n) or [dst, dst + n).
//   chroma tiles: resample_tile of picture_resample.h, the body picture_scale.hip runs.
// When both formats are the same the whole picture is one copy and there are no tiles.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pmctf_hip.h"
#include "launch.h"
#include "picture_resample.h"

#define C_SLOTS 4                                        // 16-byte slots per thread
#define C_CHUNK (P_THREADS * 16 * C_SLOTS)               // bytes of the destination per copy block
#define C_TAPS 17                                        // longest table row accepted (2:1 needs 7, 1:2 needs 4)

struct ChromaArgs {
    ScalePlane p[2];                                     // Cb, Cr
    size_t copy_bytes;                                   // bytes copied from the start of src to the start of dst
    unsigned copy_blocks;
    int idx, idy;                                        // the chroma planes keep their width / their height
};

template <int G>
__device__ __forceinline__ void copy_slot(const uint8_t *__restrict__ s, uint8_t *__restrict__ d) {
    if constexpr (G == 16) {
        *reinterpret_cast<uint4 *>(d) = *reinterpret_cast<const uint4 *>(s);
    } else if constexpr (G == 8) {
        const uint2 a = reinterpret_cast<const uint2 *>(s)[0], b = reinterpret_cast<const uint2 *>(s)[1];
        *reinterpret_cast<uint4 *>(d) = make_uint4(a.x, a.y, b.x, b.y);
    } else if constexpr (G == 4) {
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = reinterpret_cast<const uint32_t *>(s)[k];
        *reinterpret_cast<uint4 *>(d) = make_uint4(v[0], v[1], v[2], v[3]);
    } else if constexpr (G == 2) {
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            v[k] = (uint32_t)reinterpret_cast<const uint16_t *>(s)[2 * k] |
                   ((uint32_t)reinterpret_cast<const uint16_t *>(s)[2 * k + 1] << 16);
        *reinterpret_cast<uint4 *>(d) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            v[k] = (uint32_t)s[4 * k] | ((uint32_t)s[4 * k + 1] << 8) | ((uint32_t)s[4 * k + 2] << 16) |
                   ((uint32_t)s[4 * k + 3] << 24);
        *reinterpret_cast<uint4 *>(d) = make_uint4(v[0], v[1], v[2], v[3]);
    }
}

// block `b` of the copy of n bytes from src to dst
template <int G>
__device__ __forceinline__ void copy_block(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, size_t n, unsigned b) {
    const ptrdiff_t lead = (ptrdiff_t)((uintptr_t)dst & 15);            // dst - lead is 16-byte aligned
    const ptrdiff_t first = (ptrdiff_t)b * C_CHUNK - lead;               // offset of the chunk from dst (and from src)
#pragma unroll
    for (int i = 0; i < C_SLOTS; ++i) {
        const ptrdiff_t o = first + ((ptrdiff_t)i * P_THREADS + threadIdx.x) * 16;
        if (o >= 0 && (size_t)o + 16 <= n) {
            copy_slot<G>(src + o, dst + o);
        } else {
            for (ptrdiff_t k = o < 0 ? 0 : o; k < o + 16 && (size_t)k < n; ++k) dst[k] = src[k];
        }
    }
}

template <typename S>
__global__ __launch_bounds__(P_THREADS) void convert_chroma_kernel(const S *__restrict__ src, S *__restrict__ dst,
                                                                    const ChromaArgs a, int top) {
    __shared__ __attribute__((aligned(16))) int tmp[S_ROWS * S_TW];
    __shared__ int cx[S_TAPS * S_TW];

    unsigned tile = blockIdx.x;
    if (tile < a.copy_blocks) {
        const uint8_t *s = reinterpret_cast<const uint8_t *>(src);
        uint8_t *d = reinterpret_cast<uint8_t *>(dst);
        const unsigned delta = (unsigned)((uintptr_t)s - (uintptr_t)d) & 15u;
        if (delta == 0)
            copy_block<16>(s, d, a.copy_bytes, tile);
        else if (!(delta & 7))
            copy_block<8>(s, d, a.copy_bytes, tile);
        else if (!(delta & 3))
            copy_block<4>(s, d, a.copy_bytes, tile);
        else if (!(delta & 1))
            copy_block<2>(s, d, a.copy_bytes, tile);
        else
            copy_block<1>(s, d, a.copy_bytes, tile);
        return;
    }
    tile -= a.copy_blocks;
    int pi = 0;
    if (tile >= a.p[0].tiles) {
        tile -= a.p[0].tiles;
        pi = 1;
    }
    const ScalePlane &P = a.p[pi];
    if (tile >= P.tiles) return;
    if (a.idx)
        resample_tile<S, true, false>(src, dst, P, tile, top, tmp, cx);
    else if (a.idy)
        resample_tile<S, false, true>(src, dst, P, tile, top, tmp, cx);
    else
        resample_tile<S, false, false>(src, dst, P, tile, top, tmp, cx);
}

static bool taps_ok(int t) { return t >= 1 && t <= C_TAPS; }

// the subsampling (sx, sy) of a format given as 420, 422 or 444; false for anything else
static bool subsampling(int fmt, int &sx, int &sy) {
    if (fmt == 420) return sx = 2, sy = 2, true;
    if (fmt == 422) return sx = 2, sy = 1, true;
    if (fmt == 444) return sx = 1, sy = 1, true;
    return false;
}

template <typename S>
static int convert_chroma(const S *src, S *dst, int h, int w, int fmt_in, int fmt_out, const void *chroma_x,
                          const void *chroma_y, const int taps[2], int bitdepth, void *stream) {
    int sxi, syi, sxo, syo;
    if (!src || !dst || !chroma_x || !chroma_y || !taps || !side_ok(h) || !side_ok(w) || !subsampling(fmt_in, sxi, syi) ||
        !subsampling(fmt_out, sxo, syo) || !taps_ok(taps[0]) || !taps_ok(taps[1]) ||
        (((uintptr_t)src | (uintptr_t)dst) & (sizeof(S) - 1)) || (((uintptr_t)chroma_x | (uintptr_t)chroma_y) & 3))
        return PMCTF_EINVAL;
    ChromaArgs a;
    const int hci = h / syi, wci = w / sxi, hco = h / syo, wco = w / sxo;
    const size_t ny = (size_t)h * w, nc_in = (size_t)hci * wci, nc_out = (size_t)hco * wco;
    set_plane(a.p[0], hci, wci, hco, wco, chroma_x, taps[0], chroma_y, taps[1], ny, ny);
    set_plane(a.p[1], hci, wci, hco, wco, chroma_x, taps[0], chroma_y, taps[1], ny + nc_in, ny + nc_out);
    a.idx = sxi == sxo, a.idy = syi == syo;
    a.copy_bytes = ny * sizeof(S);
    if (a.idx && a.idy) {                                             // the same format: the picture is copied
        a.copy_bytes = (ny + 2 * nc_in) * sizeof(S);
        a.p[0].tiles = a.p[1].tiles = 0;
    }
    a.copy_blocks = (unsigned)((((uintptr_t)dst & 15) + a.copy_bytes + C_CHUNK - 1) / C_CHUNK);
    const unsigned blocks = a.copy_blocks + a.p[0].tiles + a.p[1].tiles;
    PM_LAUNCH(convert_chroma_kernel<S>, dim3(blocks), dim3(P_THREADS), 0, (hipStream_t)stream, src, dst, a,
              (1 << bitdepth) - 1);
    return pm_launch_status();
}

extern "C" int pmctf_convert_chroma_u8(const uint8_t *src, uint8_t *dst, int h, int w, int fmt_in, int fmt_out,
                                       const void *chroma_x, const void *chroma_y, const int taps[2], int bitdepth,
                                       void *stream) {
    if (bitdepth != 8) return PMCTF_EINVAL;
    return convert_chroma<uint8_t>(src, dst, h, w, fmt_in, fmt_out, chroma_x, chroma_y, taps, 8, stream);
}

extern "C" int pmctf_convert_chroma_u16(const uint16_t *src, uint16_t *dst, int h, int w, int fmt_in, int fmt_out,
                                        const void *chroma_x, const void *chroma_y, const int taps[2], int bitdepth,
                                        void *stream) {
    if (!depth_ok(bitdepth)) return PMCTF_EINVAL;
    return convert_chroma<uint16_t>(src, dst, h, w, fmt_in, fmt_out, chroma_x, chroma_y, taps, bitdepth, stream);
}
