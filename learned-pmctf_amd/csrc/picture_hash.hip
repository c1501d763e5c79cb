// CRC-32 (zlib.crc32: reflected polynomial 0xEDB88320, initial value and final XOR 0xFFFFFFFF) of S byte ranges in device
// memory, two launches whatever S and the lengths are:
//   crc32_init_kernel      out[s] = crc(|M_s| zero bytes), the part of the CRC that depends on the length alone
//   crc32_segments_kernel  out[s] ^= R(M_s), the raw remainder (zero initial value, no final XOR), in pieces
// CRC is linear over GF(2):  crc(M) = R(M) ^ crc(0^|M|),  R(A || B) = R(A) * x^(8|B|) mod P  ^  R(B),  and leading zero bytes
// do not change R.  A range is cut on the 16-byte address grid: the pieces [16q, 16q + 16) inside it (the first one may
// begin before the range; those bytes count as zeros) and a tail of up to 15 bytes.  The pieces are laid out in tiles of
// H_THREADS pieces that END at the last piece (the first tile is filled up with leading zeros), the tiles of a range are
// dealt to gridDim.x workgroups in contiguous spans, and thread t of a workgroup walks piece t of every tile of its span:
// one coalesced 16-byte load per tile, and
//     r = absorb(r * x^(8 (H_TILE - 16)), piece)
// with 4 + 16 lookups in two 4 x 256 tables in LDS (slicing by 4).  At the span's end thread t moves its remainder over
// the 16 (H_THREADS - 1 - t) bytes between its piece and the tile's end, the workgroup XORs its threads' remainders, moves
// the result over the bytes that follow the span and adds it to out[s] with an integer XOR atomic: the sum does not depend
// on the order of arrival, so the same input gives the same bits on every run.
// A value is a polynomial in zlib's bit order (bit 31 is x^0); moving v over n bytes is v * x^(8n) mod P.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pmctf_hip.h"
#include "launch.h"

#define H_THREADS 256
#define H_TILE (H_THREADS * 16)
#define H_POLY 0xEDB88320u
#define H_ONE 0x80000000u                        // x^0
#define H_DEFAULT_SLICES 64
#define H_MAX_SLICES 1024
#define H_MAX_SEGMENTS 65535                     // gridDim.y

static_assert(H_TILE == PMCTF_CRC32_TILE_BYTES, "the header documents the tile the tests are sized by");

// a(x) * b(x) mod P
__host__ __device__ constexpr uint32_t mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        p ^= b & (0u - (a >> 31));
        a <<= 1;
        b = (b >> 1) ^ (H_POLY & (0u - (b & 1u)));
    }
    return p;
}

struct table32 { uint32_t v[32]; };
struct table256 { uint32_t v[H_THREADS]; };

// v[k] = x^(2^k) mod P.  The order of x is 2^32 - 1, so x^(2^(k + 32)) = x^(2^k): the table serves every k through k & 31.
constexpr table32 make_x2n() {
    table32 t{};
    uint32_t p = H_ONE >> 1;
    for (int k = 0; k < 32; ++k) {
        t.v[k] = p;
        p = mulmod(p, p);
    }
    return t;
}

// x^(8n) mod P
constexpr uint32_t xpow_bytes(uint64_t n) {
    const table32 x2n = make_x2n();
    uint32_t p = H_ONE;
    for (int k = 3; n; n >>= 1, ++k)
        if (n & 1) p = mulmod(x2n.v[k & 31], p);
    return p;
}

static_assert((mulmod(0xFFFFFFFFu, xpow_bytes(1)) ^ 0xFFFFFFFFu) == 0xD202EF8Du, "zlib.crc32(b'\\0')");

// v[i] = (1 << i) moved over n bytes: the columns of the linear map behind a 4 x 256 lookup table
constexpr table32 make_columns(uint64_t n) {
    table32 t{};
    const uint32_t xp = xpow_bytes(n);
    for (int i = 0; i < 32; ++i) t.v[i] = mulmod(xp, 1u << i);
    return t;
}

// v[t] = x^(8 * 16 (H_THREADS - 1 - t)): from thread t's piece to the end of the tile
constexpr table256 make_to_tile_end() {
    table256 c{};
    const uint32_t step = xpow_bytes(16);
    uint32_t p = H_ONE;
    for (int t = H_THREADS - 1; t >= 0; --t) {
        c.v[t] = p;
        p = mulmod(p, step);
    }
    return c;
}

__constant__ const table32 d_x2n = make_x2n();
__constant__ const table32 d_cols_4 = make_columns(4);                          // over the 4 bytes of a word
__constant__ const table32 d_cols_tile = make_columns(H_TILE - 16);             // from one tile's piece to the next one's
__device__ const table256 d_to_tile_end = make_to_tile_end();

// x^(8n) mod P by the 64 lanes of a wave (all active): lane k holds x^(8 * 2^k) where bit k of n is set, the product is
// taken as a butterfly.  Every lane returns it.
__device__ __forceinline__ uint32_t xpow_bytes_wave(uint64_t n) {
    const int lane = threadIdx.x & 63;
    uint32_t p = ((n >> lane) & 1) ? d_x2n.v[(lane + 3) & 31] : H_ONE;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) p = mulmod(p, (uint32_t)__shfl_xor((int)p, d, 64));
    return p;
}

__global__ __launch_bounds__(64) void crc32_init_kernel(const pmctf_crc_segment *__restrict__ segs, uint32_t *__restrict__ out) {
    // the register starts as 0xFFFFFFFF and is moved over the whole message; a length of 0 gives 0
    const uint32_t v = mulmod(0xFFFFFFFFu, xpow_bytes_wave(segs[blockIdx.x].bytes)) ^ 0xFFFFFFFFu;
    if (threadIdx.x == 0) out[blockIdx.x] = v;
}

__device__ __forceinline__ uint32_t lookup4(const uint32_t (*tab)[256], uint32_t r) {
    return tab[0][r & 255u] ^ tab[1][(r >> 8) & 255u] ^ tab[2][(r >> 16) & 255u] ^ tab[3][r >> 24];
}

// piece k (counted from the range's first piece at `base`; k < 0: the leading zeros of the first tile) as four
// little-endian words; bytes in front of `first` (the range's start, inside piece 0) read as zeros
__device__ __forceinline__ uint4 load_piece(const uint8_t *__restrict__ base, long k, uintptr_t first) {
    if (k < 0) return make_uint4(0u, 0u, 0u, 0u);
    const uint8_t *p = base + 16 * k;
    if ((uintptr_t)p >= first) return *reinterpret_cast<const uint4 *>(p);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if ((uintptr_t)(p + i) >= first) w[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(H_THREADS) void crc32_segments_kernel(const pmctf_crc_segment *__restrict__ segs,
                                                                    uint32_t *__restrict__ out) {
    __shared__ uint32_t word_tab[4][256], tile_tab[4][256], wave_part[H_THREADS / 64];
    const uint64_t len = segs[blockIdx.y].bytes;
    if (len == 0) return;
    const uintptr_t first = (uintptr_t)segs[blockIdx.y].data, end = first + len;
    const uint64_t q_lo = first >> 4, q_hi = end >> 4;
    const uint64_t pieces = q_hi - q_lo, tiles = (pieces + H_THREADS - 1) / H_THREADS;
    const uintptr_t tail_at = first > (q_hi << 4) ? first : (q_hi << 4);
    const unsigned tail_len = (unsigned)(end - tail_at);                          // 0..15
    // this workgroup's span of tiles, and whether it also takes the tail
    const uint64_t per_group = (tiles + gridDim.x - 1) / gridDim.x;
    const uint64_t j0 = min(blockIdx.x * per_group, tiles), j1 = min(j0 + per_group, tiles);
    const bool takes_tail = blockIdx.x == 0 && tail_len != 0;
    if (j0 == j1 && !takes_tail) return;

    const int t = threadIdx.x;
    if (j0 != j1) {
        // entry b of table k is (b << 8k) moved over 4 bytes, resp. over H_TILE - 16 bytes: the XOR of the columns of b's bits
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t a = 0, b = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint32_t m = 0u - (((unsigned)t >> i) & 1u);
                a ^= d_cols_4.v[8 * k + i] & m;
                b ^= d_cols_tile.v[8 * k + i] & m;
            }
            word_tab[k][t] = a;
            tile_tab[k][t] = b;
        }
    }
    __syncthreads();

    uint32_t r = 0;
    if (j0 != j1) {
        const uint8_t *base = reinterpret_cast<const uint8_t *>(q_lo << 4);
        long k = (long)pieces - (long)(tiles - j0) * H_THREADS + t;
        uint64_t n = j1 - j0;
        auto absorb = [&](const uint4 v) {
            r = lookup4(tile_tab, r);
            r = lookup4(word_tab, r ^ v.x);
            r = lookup4(word_tab, r ^ v.y);
            r = lookup4(word_tab, r ^ v.z);
            r = lookup4(word_tab, r ^ v.w);
        };
        for (; n >= 4; n -= 4, k += 4 * H_THREADS) {                             // four loads in flight per thread
            const uint4 v0 = load_piece(base, k, first), v1 = load_piece(base, k + H_THREADS, first);
            const uint4 v2 = load_piece(base, k + 2 * H_THREADS, first), v3 = load_piece(base, k + 3 * H_THREADS, first);
            absorb(v0); absorb(v1); absorb(v2); absorb(v3);
        }
        for (; n; --n, k += H_THREADS) absorb(load_piece(base, k, first));
        r = mulmod(r, d_to_tile_end.v[t]);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) r ^= (uint32_t)__shfl_xor((int)r, d, 64);
    }
    if ((t & 63) == 0) wave_part[t >> 6] = r;
    __syncthreads();
    if (t >= 64) return;

    uint32_t v = wave_part[0] ^ wave_part[1] ^ wave_part[2] ^ wave_part[3];
    v = mulmod(v, xpow_bytes_wave((tiles - j1) * (uint64_t)H_TILE + tail_len));
    if (t != 0) return;
    if (takes_tail) {
        const uint8_t *p = reinterpret_cast<const uint8_t *>(tail_at);
        uint32_t c = 0;
        for (unsigned i = 0; i < tail_len; ++i) {
            c ^= p[i];
#pragma unroll
            for (int b = 0; b < 8; ++b) c = (c >> 1) ^ (H_POLY & (0u - (c & 1u)));
        }
        v ^= c;
    }
    if (v) atomicXor(out + blockIdx.y, v);
}

extern "C" int pmctf_crc32_segments(const pmctf_crc_segment *segs, int n_segs, int slices, uint32_t *crc_out, void *stream) {
    if (n_segs < 0 || n_segs > H_MAX_SEGMENTS || slices < 0 || slices > H_MAX_SLICES) return PMCTF_EINVAL;
    if (n_segs == 0) return PMCTF_OK;
    if (!segs || !crc_out || ((uintptr_t)segs & 7) || ((uintptr_t)crc_out & 3)) return PMCTF_EINVAL;
    if (slices == 0) slices = H_DEFAULT_SLICES;
    PM_LAUNCH(crc32_init_kernel, dim3((unsigned)n_segs), dim3(64), 0, (hipStream_t)stream, segs, crc_out);
    const int rc = pm_launch_status();
    if (rc) return rc;
    PM_LAUNCH(crc32_segments_kernel, dim3((unsigned)slices, (unsigned)n_segs), dim3(H_THREADS), 0, (hipStream_t)stream, segs,
              crc_out);
    return pm_launch_status();
}
