// simplyp_pack.h -- the lossless codec of the packed output stream: one definition, compiled for the device (the pack
// epilogue of the task-queue kernel, simplyp_fetch_packed) and for the host (the decode pool, the plain C++ encoder of the
// CPU test).  No floating-point operation anywhere: values travel as their 64-bit patterns.
//
// Per (column, member): z = zigzag(u[d] - u[d-1]) modulo 2^64 on the raw patterns of consecutive days.  On the model's daily
// table z needs 49-51 bits at the median and fits 56 bits for all but ~6 values per million, so a
// value travels as 7 bytes.  A 64-member block that holds any z >= 2^56 travels raw as well, exactly.
//
// One record per (time chunk, column), contiguous so that it is one plain copy:
//   header   [cap] uint32   member groups whose blocks sit in the overflow area, in slot order (padded to 256 bytes)
//   row 0    [E] fp64       the chunk's first day, raw: chunks decode independently of each other
//   planes for rows 1 .. nd-1, member axis fastest (a wave's store is one 256-, 128- or 64-byte segment):
//            [nd-1][E] uint32   bits  0..31 of z
//            [nd-1][E] uint16   bits 32..47
//            [nd-1][E] uint8    bits 48..55
//   overflow [cap][nd][64] fp64 raw blocks; only the slots in use travel, in the same copy
// The record's overflow counter lives outside it (one array per run, zeroed with one memset); a counter above `cap` marks the
// record raw: the copier then sends that chunk-column from the fp64 table.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

#if defined(__HIPCC__)
#define SIMPLYP_PACK_HD __host__ __device__
#else
#define SIMPLYP_PACK_HD
#endif

namespace simplyp_pack {

constexpr int GROUP = 64;        // members per block = lanes of a wavefront
constexpr int Z_BITS = 56;       // what the three planes hold

SIMPLYP_PACK_HD inline uint64_t zigzag(uint64_t delta) { return (delta << 1) ^ (uint64_t)((int64_t)delta >> 63); }
SIMPLYP_PACK_HD inline uint64_t unzigzag(uint64_t z) { return (z >> 1) ^ (0ull - (z & 1ull)); }
SIMPLYP_PACK_HD inline uint64_t encode(uint64_t u, uint64_t prev) { return zigzag(u - prev); }
SIMPLYP_PACK_HD inline uint64_t decode(uint64_t z, uint64_t prev) { return prev + unzigzag(z); }
SIMPLYP_PACK_HD inline bool fits(uint64_t z) { return (z >> Z_BITS) == 0ull; }

// Overflow slots of a record with n_groups blocks: an eighth of them (the model's flux columns need 2.3 %), and three more
// so that a small ensemble does not go raw for two unlucky blocks.
SIMPLYP_PACK_HD inline unsigned overflow_capacity(int n_groups) { return (unsigned)n_groups / 8u + 3u; }

struct Layout {
    size_t off_row0, off_lo, off_mid, off_hi, off_ovf;   // bytes from the start of the record
    size_t block_bytes;                                  // one overflow block: nd x 64 doubles
    size_t bytes;                                        // whole record, overflow area included (a multiple of 256)
};

SIMPLYP_PACK_HD inline size_t round_up(size_t v, size_t to) { return (v + to - 1) / to * to; }

SIMPLYP_PACK_HD inline Layout layout(size_t E, int nd, unsigned cap)
{
    Layout L;
    const size_t rows = (size_t)(nd - 1);
    L.off_row0 = round_up((size_t)cap * sizeof(uint32_t), 256);
    L.off_lo = L.off_row0 + E * sizeof(double);
    L.off_mid = L.off_lo + rows * E * sizeof(uint32_t);
    L.off_hi = L.off_mid + rows * E * sizeof(uint16_t);
    L.off_ovf = round_up(L.off_hi + rows * E, 256);
    L.block_bytes = (size_t)nd * GROUP * sizeof(double);
    L.bytes = L.off_ovf + (size_t)cap * L.block_bytes;
    return L;
}

#if defined(__HIPCC__)
// One wavefront packs its own block: members g*64 .. g*64+63 of `nd` rows of one column.  `rows` points at the column's first
// row of the chunk, `stride` is doubles per row.  Loads go out in batches of independent requests; the prediction chain
// (previous day) stays in a register.  `count` is the record's overflow counter.
__device__ __forceinline__ void pack_block(const double* rows, size_t stride, int nd, int E, int g, int lane,
                                           unsigned char* rec, const Layout& L, unsigned* count, unsigned cap)
{
    constexpr int BATCH = 8;
    const int e = g * GROUP + lane;
    const bool live = e < E;
    const unsigned long long* src = (const unsigned long long*)rows + (live ? e : 0);
    uint32_t* lo = (uint32_t*)(rec + L.off_lo) + e;
    uint16_t* mid = (uint16_t*)(rec + L.off_mid) + e;
    uint8_t* hi = (uint8_t*)(rec + L.off_hi) + e;
    unsigned long long prev = live ? src[0] : 0ull;
    if (live) ((unsigned long long*)(rec + L.off_row0))[e] = prev;
    unsigned long long big = 0ull;
    for (int d0 = 1; d0 < nd; d0 += BATCH) {
        unsigned long long u[BATCH];
#pragma unroll
        for (int i = 0; i < BATCH; ++i) u[i] = (live && d0 + i < nd) ? src[(size_t)(d0 + i) * stride] : 0ull;
#pragma unroll
        for (int i = 0; i < BATCH; ++i) {
            if (live && d0 + i < nd) {
                const unsigned long long z = encode(u[i], prev);
                prev = u[i];
                big |= z >> Z_BITS;
                const size_t at = (size_t)(d0 + i - 1) * (size_t)E;
                lo[at] = (uint32_t)z;
                mid[at] = (uint16_t)(z >> 32);
                hi[at] = (uint8_t)(z >> 48);
            }
        }
    }
    if (__ballot(big != 0ull) == 0ull) return;                 // wave-uniform
    unsigned slot = 0u;
    if (lane == 0) slot = atomicAdd(count, 1u);
    slot = (unsigned)__builtin_amdgcn_readfirstlane((int)slot);
    if (slot >= cap) return;                                   // the record travels raw
    if (lane == 0) ((uint32_t*)rec)[slot] = (uint32_t)g;
    unsigned long long* blk = (unsigned long long*)(rec + L.off_ovf + (size_t)slot * L.block_bytes) + lane;
    for (int d = 0; d < nd; ++d) blk[(size_t)d * GROUP] = live ? src[(size_t)d * stride] : 0ull;
}
#endif

// ---- host half ----

// The encoder in plain C++, block by block like the device's: returns the record's overflow counter (which may pass `cap`;
// blocks beyond it are not stored).
inline unsigned encode_record_host(const double* rows, size_t stride, int nd, size_t E, unsigned char* rec, const Layout& L,
                                   unsigned cap)
{
    const uint64_t* src = (const uint64_t*)rows;
    unsigned count = 0;
    const int G = (int)((E + GROUP - 1) / GROUP);
    memcpy(rec + L.off_row0, src, E * sizeof(uint64_t));
    for (int g = 0; g < G; ++g) {
        const size_t e0 = (size_t)g * GROUP, e1 = e0 + GROUP < E ? e0 + GROUP : E;
        bool big = false;
        for (size_t e = e0; e < e1; ++e) {
            uint64_t prev = src[e];
            for (int d = 1; d < nd; ++d) {
                const uint64_t u = src[(size_t)d * stride + e], z = encode(u, prev);
                prev = u;
                big = big || !fits(z);
                const size_t at = (size_t)(d - 1) * E + e;
                const uint32_t l = (uint32_t)z; const uint16_t m = (uint16_t)(z >> 32);
                memcpy(rec + L.off_lo + at * 4, &l, 4);
                memcpy(rec + L.off_mid + at * 2, &m, 2);
                rec[L.off_hi + at] = (uint8_t)(z >> 48);
            }
        }
        if (!big) continue;
        const unsigned slot = count++;
        if (slot >= cap) continue;
        const uint32_t gid = (uint32_t)g;
        memcpy(rec + (size_t)slot * 4, &gid, 4);
        uint64_t* blk = (uint64_t*)(rec + L.off_ovf + (size_t)slot * L.block_bytes);
        for (int d = 0; d < nd; ++d)
            for (size_t i = 0; i < (size_t)GROUP; ++i) blk[(size_t)d * GROUP + i] = e0 + i < E ? src[(size_t)d * stride + e0 + i] : 0ull;
    }
    return count;
}

// Members [e0, e1) of a landed record into `dst` (the column's first row of the chunk, `stride` doubles per row), written with
// non-temporal stores.  `run` holds e1 - e0 words: the running values, which stay in cache from row to row.
// One row of a range: out[i] = run[i] += unzigzag(planes[i]).
inline void decode_row_scalar(const unsigned char* lo, const unsigned char* mid, const unsigned char* hi, uint64_t* run,
                              unsigned long long* out, size_t n)
{
    for (size_t i = 0; i < n; ++i) {
        uint32_t l; uint16_t m;
        memcpy(&l, lo + i * 4, 4);
        memcpy(&m, mid + i * 2, 2);
        const uint64_t z = (uint64_t)l | ((uint64_t)m << 32) | ((uint64_t)hi[i] << 48);
        const uint64_t u = decode(z, run[i]);
        run[i] = u;
        __builtin_nontemporal_store((unsigned long long)u, out + i);
    }
}

#if defined(__x86_64__)
// The same with 256-bit integer operations, eight values per turn; `out` must be 32-byte aligned.
__attribute__((target("avx2"))) inline void decode_row_avx2(const unsigned char* lo, const unsigned char* mid, const unsigned char* hi,
                                                            uint64_t* run, unsigned long long* out, size_t n)
{
    const __m256i one = _mm256_set1_epi64x(1), zero = _mm256_setzero_si256();
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
        const __m256i l = _mm256_loadu_si256((const __m256i*)(lo + i * 4));
        const __m128i m = _mm_loadu_si128((const __m128i*)(mid + i * 2));
        const __m128i h = _mm_loadl_epi64((const __m128i*)(hi + i));
        const __m256i z0 = _mm256_or_si256(_mm256_cvtepu32_epi64(_mm256_castsi256_si128(l)),
                                           _mm256_or_si256(_mm256_slli_epi64(_mm256_cvtepu16_epi64(m), 32),
                                                           _mm256_slli_epi64(_mm256_cvtepu8_epi64(h), 48)));
        const __m256i z1 = _mm256_or_si256(_mm256_cvtepu32_epi64(_mm256_extracti128_si256(l, 1)),
                                           _mm256_or_si256(_mm256_slli_epi64(_mm256_cvtepu16_epi64(_mm_srli_si128(m, 8)), 32),
                                                           _mm256_slli_epi64(_mm256_cvtepu8_epi64(_mm_srli_si128(h, 4)), 48)));
        const __m256i d0 = _mm256_xor_si256(_mm256_srli_epi64(z0, 1), _mm256_sub_epi64(zero, _mm256_and_si256(z0, one)));
        const __m256i d1 = _mm256_xor_si256(_mm256_srli_epi64(z1, 1), _mm256_sub_epi64(zero, _mm256_and_si256(z1, one)));
        const __m256i u0 = _mm256_add_epi64(_mm256_loadu_si256((const __m256i*)(run + i)), d0);
        const __m256i u1 = _mm256_add_epi64(_mm256_loadu_si256((const __m256i*)(run + i + 4)), d1);
        _mm256_storeu_si256((__m256i*)(run + i), u0);
        _mm256_storeu_si256((__m256i*)(run + i + 4), u1);
        _mm256_stream_si256((__m256i*)(out + i), u0);
        _mm256_stream_si256((__m256i*)(out + i + 4), u1);
    }
    decode_row_scalar(lo + i * 4, mid + i * 2, hi + i, run + i, out + i, n - i);
}
#endif

inline void decode_range(const unsigned char* rec, const Layout& L, int nd, size_t E, size_t e0, size_t e1, double* dst,
                         size_t stride, uint64_t* run)
{
    const size_t n = e1 - e0;
    memcpy(run, rec + L.off_row0 + e0 * 8, n * 8);
    unsigned long long* out = (unsigned long long*)dst + e0;       // (doubles: 8-byte aligned)
    for (size_t i = 0; i < n; ++i) __builtin_nontemporal_store((unsigned long long)run[i], out + i);
#if defined(__x86_64__)
    static const bool have_avx2 = __builtin_cpu_supports("avx2");
#endif
    for (int d = 1; d < nd; ++d) {
        const size_t at = (size_t)(d - 1) * E + e0;
        const unsigned char* lo = rec + L.off_lo + at * 4;
        const unsigned char* mid = rec + L.off_mid + at * 2;
        const unsigned char* hi = rec + L.off_hi + at;
        out += stride;
#if defined(__x86_64__)
        if (have_avx2) {
            // scalar up to the first 32-byte boundary of the row, vectors from there
            size_t head = ((32 - ((uintptr_t)out & 31)) & 31) / 8;
            if (head > n) head = n;
            decode_row_scalar(lo, mid, hi, run, out, head);
            decode_row_avx2(lo + head * 4, mid + head * 2, hi + head, run + head, out + head, n - head);
            continue;
        }
#endif
        decode_row_scalar(lo, mid, hi, run, out, n);
    }
}

// The raw blocks of the record's overflow area over what decode_range wrote (after every range of the record is done).
inline void apply_overflow(const unsigned char* rec, const Layout& L, int nd, size_t E, unsigned count, double* dst, size_t stride)
{
    for (unsigned s = 0; s < count; ++s) {
        uint32_t g;
        memcpy(&g, rec + (size_t)s * 4, 4);
        const size_t e0 = (size_t)g * GROUP;
        if (e0 >= E) continue;
        const size_t n = e0 + GROUP < E ? (size_t)GROUP : E - e0;
        const unsigned char* blk = rec + L.off_ovf + (size_t)s * L.block_bytes;
        for (int d = 0; d < nd; ++d) memcpy(dst + (size_t)d * stride + e0, blk + (size_t)d * GROUP * 8, n * 8);
    }
}

}  // namespace simplyp_pack
